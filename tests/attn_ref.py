"""The decode attention without a GPU: an fp64 reference, the seeded inputs of
tests/test_gpu_attn_probe.py and the plan cells it visits (tests/test_attn_ref.py checks all three).

The reference is softmax(K q / sqrt(96)) V per (row, head) in float64 over the STORED K / V values (what
lvx_kv_read returns), so the KV quantisation is not part of the error it measures, and an fp64 merge of
split partials (m, l, o) for the plans whose merge lives in c_proj's prologue.

The inputs make every head's output depend on ONE key at an edge of the kernel's indexing: the query is
that key's direction plus noise, scaled so that the key takes about half of the softmax weight. Losing
the key, or reading its neighbour in its place, then moves the output by about 1; a logit-level check
cannot see that.
"""
import math
from collections import namedtuple

import numpy as np
import torch

HD, NH, D = 96, 8, 768
ATK = 64      # keys per split granule (ar_kernels.hip)
NSPLIT = 16
SCALE = 1.0 / math.sqrt(HD)
# key counts t = P + 1 of the rows: around every 64- and 128-key tile edge up to 1,025; 320 leaves a
# trailing empty split at 4 splits, 513 at 8, 1,025 at 16
T_LIST = [1, 2, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 320, 511, 512, 513, 1023, 1024, 1025]
MAX_POSITIONS = 1152  # 18 chunks of 64: room for the stale rows after key 1,024 up to the end of its 128-key tile
HIST_SEED = 20261019

ATTN_PARTIALS, ATTN_XN, ATTN_XN_PACKED, ATTN_F32_ROWS = 0, 1, 2, 3

# Absolute part of the GPU test's bound per KV dtype: 8 x the largest |device - fp64| measured over every
# cell, call, layer and query set of tests/test_gpu_attn_probe.py on the fp32 output forms (the split
# partials merged in fp64, ATTN_F32_ROWS). The figures and the date of the run: DESIGN.md section 2.
# Rows that the kernels round to bf16 get 2^-8 |ref| on top (round-to-nearest-even is within 2^-9).
ATTN_ABS_MEASURED = {"fp32": 1.25e-6, "bf16": 7.59e-6, "fp8": 9.34e-7}
ATTN_ABS_CAP = 1e-2  # the bound may never exceed this: 1 / 100 of the smallest single-key mutation effect
ATTN_ABS = {kv: 8.0 * m for kv, m in ATTN_ABS_MEASURED.items()}
BF16_REL = 2.0 ** -8
MUTATION_MIN = 0.5     # every single-key mutation moves the output by at least this (absolute)
MUTATION_OVER_TOL = 50.0  # ... and by at least this many times the tolerance in force


def tolerance(kv, ref, bf16_rows):
    """The bound in force on |device - ref|, elementwise."""
    tol = np.full_like(ref, ATTN_ABS[kv], dtype=np.float64)
    return tol + BF16_REL * np.abs(ref) if bf16_rows else tol


# ----------------------------------------------------------------------------------------------------
# The plan cells. kv: the engine ("bf16": bf16 weights / bf16 KV, "fp8": bf16 / fp8 KV, "fp32": fp32 / fp32);
# opts: the options set for the cell; plan: the (nsplit, attn_direct, attn8) that ar_plan_step gives it
# (tests/test_attn_ref.py holds this table to ar_plan.h); form: 0 normalised rows, 1 partials; merged: the
# plan's merge kernel produced the rows (an idle row is then written as zeros).
# ----------------------------------------------------------------------------------------------------
Cell = namedtuple("Cell", "kv B opts plan form merged")


def attn_ns_max(B):
    ns = NSPLIT
    while ns > 1 and ns * NH * B > 256:
        ns >>= 1
    return ns


def _default_cell(kv, B):
    if B <= 2 or B > 64:  # GEMV family: 16 splits, merged in c_proj's prologue
        return Cell(kv, B, {}, (NSPLIT, ATTN_PARTIALS, 0), 1, False)
    if B <= 4:  # 8 splits + ar_merge_bf16_kernel
        return Cell(kv, B, {}, (attn_ns_max(B), ATTN_PARTIALS, 0), 0, True)
    if B <= 8:  # one split, 8-wave blocks, writes xn
        return Cell(kv, B, {}, (1, ATTN_XN, 1), 0, False)
    if B <= 32:  # one split into the fragment-packed xn; fp8 KV keeps the 8-wave blocks up to B = 16
        return Cell(kv, B, {}, (1, ATTN_XN_PACKED, int(kv == "fp8" and B <= 16)), 0, False)
    return Cell(kv, B, {}, (attn_ns_max(B), ATTN_PARTIALS, 0), 0, True)  # v3: partials + the merge kernel


def cells():
    out = []
    for kv in ("bf16", "fp8"):
        # (B = 65: grid 16 x 8 x 65, on one dtype)
        for B in (1, 2, 3, 4, 5, 8, 9) + ((12,) if kv == "fp8" else ()) + (16, 17, 32, 33, 64) + ((65,) if kv == "bf16" else ()):
            out.append(_default_cell(kv, B))
        for B in (8, 16):  # v3 with 4 and 2 splits
            out.append(Cell(kv, B, {"bt": 2}, (attn_ns_max(B), ATTN_PARTIALS, 0), 0, True))
        out.append(Cell(kv, 6, {"ln_max": 4}, (1, ATTN_XN_PACKED, 1), 0, False))  # rows structure, 8-wave, packed
    out.append(Cell("fp32", 1, {"exp": 1024}, (NSPLIT, ATTN_PARTIALS, 0), 1, False))
    out.append(Cell("fp32", 3, {"exp": 1024}, (attn_ns_max(3), ATTN_PARTIALS, 0), 1, False))    # FIN_MERGE
    out.append(Cell("fp32", 12, {"exp": 1024}, (attn_ns_max(12), ATTN_PARTIALS, 0), 1, False))  # FIN_MERGE
    out.append(Cell("fp32", 32, {"exp": 1024}, (1, ATTN_F32_ROWS, 0), 0, False))
    out.append(Cell("fp32", 12, {"f32b": 0}, (NSPLIT, ATTN_PARTIALS, 0), 1, False))             # fp32 GEMV family
    return out


def idle_cells():
    """The cells of the idle-row test: B = 8 and 32 on every engine (fp32 with the one-launch c_attn)."""
    out = [_default_cell(kv, B) for kv in ("bf16", "fp8") for B in (8, 32)]
    out.append(Cell("fp32", 8, {"exp": 1024}, (attn_ns_max(8), ATTN_PARTIALS, 0), 1, False))  # FIN_MERGE
    out.append(Cell("fp32", 32, {"exp": 1024}, (1, ATTN_F32_ROWS, 0), 0, False))
    return out


def cell_id(c):
    o = ",".join(f"{k}={v}" for k, v in c.opts.items())
    return f"{c.kv}-B{c.B}" + (f"-{o}" if o else "")


def max_streams(kv):
    return 65 if kv == "bf16" else 64  # the B = 65 cell runs on the bf16 engine


# ----------------------------------------------------------------------------------------------------
# The split arithmetic of ar_attn_v2_kernel, restated
# ----------------------------------------------------------------------------------------------------
def split_ranges(t, ns_max, kv):
    """[(k0, k1)] of the splits the kernel writes for t keys (k0 >= k1: an empty trailing split, which
    writes m = -inf, l = 0). bf16 / fp8 KV round the split length up to whole 64-key tiles."""
    ns = min(ns_max, (t + ATK - 1) // ATK)
    per = (t + ns - 1) // ns
    chunk = (per + ATK - 1) // ATK * ATK if kv != "fp32" else per
    return [(sp * chunk, min(t, sp * chunk + chunk)) for sp in range(ns)]


def edge_keys(t, ns_max, kv):
    """The keys at which the kernel's indexing changes, for a row of t keys."""
    e = {0, t - 1, t - 2}
    e |= {min(k, t - 1) for k in (63, 64, 127, 128)}
    last = (t - 1) // ATK * ATK
    e |= {last, last - 1}
    for k0, k1 in split_ranges(t, ns_max, kv):
        if k0 < k1:
            e |= {k0, k1 - 1}
    return sorted(k for k in e if 0 <= k < t)


# ----------------------------------------------------------------------------------------------------
# Inputs
# ----------------------------------------------------------------------------------------------------
def quantise(x, kv):
    """float32 array -> the float32 values the KV dtype stores (lvx_kv_write's conversion)."""
    t = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))
    if kv == "bf16":
        t = t.to(torch.bfloat16).float()
    elif kv == "fp8":
        t = t.clamp(-448.0, 448.0).to(torch.float8_e4m3fn).float()
    return t.numpy()


def history(slot, n_pos=MAX_POSITIONS):
    """The unquantised K ~ 0.7 N(0, 1) and V ~ N(0, 1) rows [n_pos][768] of a slot (every engine and layer
    draws its slots' histories from these; a row's first t rows are its keys, the rest its stale rows)."""
    rng = np.random.default_rng([HIST_SEED, slot])
    k = 0.7 * rng.standard_normal((n_pos, D), dtype=np.float32)
    v = rng.standard_normal((n_pos, D), dtype=np.float32)
    return k, v


def row_queries(K, t, edges, slot):
    """Query sets for one row: K the stored keys [>= t][768]. Head h of set i is spiked at key
    edges[(8 i + h) % len(edges)]; sets are added until every edge key was spiked once.
    Returns q float32 [nq][8][96] and the spiked keys int [nq][8]."""
    nq = (len(edges) + NH - 1) // NH
    rng = np.random.default_rng([HIST_SEED, 1, slot, t])
    q = np.empty((nq, NH, HD), dtype=np.float32)
    spiked = np.empty((nq, NH), dtype=np.int64)
    for i in range(nq):
        for h in range(NH):
            j = edges[(NH * i + h) % len(edges)]
            k = K[j, h * HD:(h + 1) * HD].astype(np.float64)
            nrm = float(np.linalg.norm(k))
            c = (math.log(max(t, 2)) + 1.0) * math.sqrt(HD) / nrm
            q[i, h] = (c * k / nrm + 0.5 * rng.standard_normal(HD)).astype(np.float32)
            spiked[i, h] = j
    return q, spiked


def row_positions(B, call):
    """Key counts of the B rows of a cell's call: T_LIST cycled, so that ceil(21 / B) calls visit every t."""
    return [T_LIST[(call * B + b + B) % len(T_LIST)] for b in range(B)]


def n_calls(B):
    return (len(T_LIST) + B - 1) // B


def row_slots(B, S):
    """Rows to slots by a seeded permutation of the engine's S slots, never the identity."""
    rng = np.random.default_rng([HIST_SEED, 2, B, S])
    while True:
        p = rng.permutation(S)[:B]
        if B == 1 and S > 1 and p[0] == 0:
            continue
        if B == 1 or not np.array_equal(p, np.arange(B)):
            return [int(s) for s in p]


# ----------------------------------------------------------------------------------------------------
# The fp64 reference
# ----------------------------------------------------------------------------------------------------
def attention_fp64(q, K, V, t, dtype=np.float64):
    """q [nq][8][96], stored K / V [>= t][768] -> (out [nq][768], softmax weights [nq][8][t]) in `dtype`."""
    Kh = K[:t].astype(dtype).reshape(t, NH, HD)
    Vh = V[:t].astype(dtype).reshape(t, NH, HD)
    s = np.einsum("nhd,thd->nht", q.astype(dtype), Kh) * dtype(SCALE)
    s -= s.max(axis=-1, keepdims=True)
    w = np.exp(s)
    w /= w.sum(axis=-1, keepdims=True)
    out = np.einsum("nht,thd->nhd", w, Vh)
    return out.reshape(q.shape[0], D), w


def merge_fp64(part_o, part_ml, ns):
    """Split partials of one row, part_o [8][16][96] and part_ml [8][16][2] (max, sum), splits [0, ns)
    valid -> the normalised row [768] in float64. An empty split carries m = -inf, l = 0."""
    o = part_o[:, :ns].astype(np.float64)
    m = part_ml[:, :ns, 0].astype(np.float64)
    l = part_ml[:, :ns, 1].astype(np.float64)
    M = m.max(axis=1, keepdims=True)
    with np.errstate(invalid="ignore"):
        f = np.where(np.isneginf(m), 0.0, np.exp(m - M))
    return ((f[:, :, None] * o).sum(axis=1) / (f * l).sum(axis=1, keepdims=True)).reshape(D)


def mutation_effects(q, K, V, t, spiked, out, w):
    """For every (query set, head): how far the head's output moves (max over its 96 dims, and the
    largest ratio to `tol` is left to the caller) when the spiked key is REMOVED and when it is REPLACED
    by its neighbour (the key before it; after it for key 0, which for t = 1 is the first stale row).
    Returns (removed [nq][8][96], replaced [nq][8][96]): the output differences."""
    nq = q.shape[0]
    rem = np.zeros((nq, NH, HD))
    rep = np.zeros((nq, NH, HD))
    o = out.reshape(nq, NH, HD)
    for i in range(nq):
        for h in range(NH):
            j = int(spiked[i, h])
            sl = slice(h * HD, (h + 1) * HD)
            Vh = V[:t, sl].astype(np.float64)
            wj = w[i, h, j]
            # removed: the other keys' weights renormalised (no key left: the output is 0)
            rem[i, h] = (o[i, h] - wj * Vh[j]) / (1.0 - wj) - o[i, h] if t > 1 else -o[i, h]
            jn = j - 1 if j > 0 else j + 1
            Kn = K[:max(t, jn + 1), sl].astype(np.float64).copy()
            Vn = V[:max(t, jn + 1), sl].astype(np.float64).copy()
            Kn[j], Vn[j] = Kn[jn], Vn[jn]
            s = Kn[:t] @ q[i, h].astype(np.float64) * SCALE
            e = np.exp(s - s.max())
            rep[i, h] = (e / e.sum()) @ Vn[:t] - o[i, h]
    return rem, rep
