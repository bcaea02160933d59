"""The decode attention of every plan cell (ar_attn_v2_kernel in each launch shape, its merge kernel)
against the fp64 reference of tests/attn_ref.py, through the test hooks lvx_kv_write / lvx_kv_read /
lvx_attn_probe.

Rows of one call sit at ragged positions around every 64- and 128-key tile edge up to 1,025 keys, in
slots chosen by a seeded permutation; every head's query is spiked at one edge key of the kernel's
indexing (first / last key, tile edges, the first and last key of every split range), so a key lost,
duplicated or read from the neighbouring row moves the output by about 1 (asserted here for every row,
and without a GPU in tests/test_attn_ref.py) against a bound of at most 1e-2 + 2^-8 |ref|. The reference
reads the stored K / V back through lvx_kv_read: the KV quantisation is not part of the error.

Layer 0 of slot s holds history s, layer 3 of slot s history (s + 3) % S: a wrong layer or slot index
reads another history.

The plans that merge their splits inside c_proj's prologue (the GEMV family, fp32 FIN_MERGE) hand out
their partials, merged here in fp64: those prologue merges stay covered at the logit level only.
"""
import numpy as np
import pytest
import torch

from tests import attn_ref as A

pytestmark = pytest.mark.gpu

LAYERS = (0, 3)
ENGINE = {"bf16": ("bf16", "bf16"), "fp8": ("bf16", "fp8"), "fp32": ("fp32", "fp32")}
DEFAULT_OPTS = {"bt": 1, "ln_max": 8, "exp": 0, "f32b": 1}
NAN_BITS = {"fp32": 0x7FC00000, "bf16": 0x7FC0, "fp8": 0x7F}
MAX_FINITE = {"fp32": float(np.finfo(np.float32).max), "bf16": float.fromhex("0x1.fep127"), "fp8": 448.0}
CELLS = A.cells()


class Hist:
    """One engine with every slot's history written through lvx_kv_write and read back."""

    def __init__(self, kv):
        from llmvox_amd.engine import build_engine
        self.kv = kv
        self.S = A.max_streams(kv)
        wd, kvd = ENGINE[kv]
        self.e = e = build_engine(0, wd, kvd, max_streams=self.S, max_positions=A.MAX_POSITIONS, max_codec_frames=16)
        S, P = self.S, A.MAX_POSITIONS
        self.K = np.empty((S, P, A.D), dtype=np.float32)  # stored values of history h (layer 0: slot h)
        self.V = np.empty((S, P, A.D), dtype=np.float32)
        for h in range(S):
            kh, vh = A.history(h)
            k, v = torch.from_numpy(kh).to(e.device), torch.from_numpy(vh).to(e.device)
            e.kv_write(h, 0, 0, k, v)
            e.kv_write((h - 3) % S, 3, 0, k, v)
            k0, v0 = e.kv_read(h, 0, 0, P)
            k3, v3 = e.kv_read((h - 3) % S, 3, 0, P)
            assert torch.equal(k0, k3) and torch.equal(v0, v3), h
            self.K[h], self.V[h] = k0.cpu().numpy(), v0.cpu().numpy()
            # the hook converts as the step's appends do: round to nearest even (fp8: saturated e4m3fn)
            assert np.array_equal(self.K[h], A.quantise(kh, kv)) and np.array_equal(self.V[h], A.quantise(vh, kv)), (kv, h)
        e.check_errors()

    def hist(self, slot, layer):
        h = (slot + layer) % self.S
        return self.K[h], self.V[h]

    def close(self):
        self.e.close()


@pytest.fixture(scope="module")
def hists():
    """The engine of a KV dtype with its histories, built on first use."""
    cur = {}

    def get(kv):
        if kv not in cur:
            cur[kv] = Hist(kv)
        return cur[kv]

    yield get
    for h in cur.values():
        h.close()


MEASURED = {}  # kv -> largest |device - fp64| on the fp32 output forms, over the module


class Call:
    """The rows of one call of a cell: slots, key counts, and per layer the query sets and their spiked keys."""

    def __init__(self, H, cell, call):
        self.B = B = cell.B
        self.slots = A.row_slots(B, H.S)
        self.ts = A.row_positions(B, call)
        self.q, self.spiked = {}, {}
        for layer in LAYERS:
            for b in range(B):
                K, _ = H.hist(self.slots[b], layer)
                edges = A.edge_keys(self.ts[b], cell.plan[0], cell.kv)
                self.q[layer, b], self.spiked[layer, b] = A.row_queries(K, self.ts[b], edges, self.slots[b])
        self.nq = max(q.shape[0] for q in self.q.values())

    def q_rows(self, layer, i):
        """Query set i of every row (rows with fewer sets repeat theirs) as the probe's [B][768]."""
        return np.stack([self.q[layer, b][i % self.q[layer, b].shape[0]].reshape(A.D) for b in range(self.B)])


def _set_opts(e, opts):
    for k, v in {**DEFAULT_OPTS, **opts}.items():
        e.set_option(k, v)


def _place(H, c, slots=None):
    for b, s in enumerate(c.slots if slots is None else slots):
        if s >= 0:
            H.e.set_slot(s, c.ts[b] - 1, 0)


def _probe(H, cell, c, layer, i, slots=None):
    e = H.e
    st = torch.tensor(c.slots if slots is None else slots, dtype=torch.int32, device=e.device)
    form, out, po, pml, plan = e.attn_probe(st, layer, torch.from_numpy(c.q_rows(layer, i)))
    assert plan == cell.plan and form == cell.form, (plan, form)
    return out.cpu().numpy(), po.cpu().numpy(), pml.cpu().numpy()


def _n_splits(cell, t):
    return len(A.split_ranges(t, cell.plan[0], cell.kv))


@pytest.mark.parametrize("cell", CELLS, ids=A.cell_id)
def test_attention_matches_fp64(hists, cell):
    H = hists(cell.kv)
    e = H.e
    _set_opts(e, cell.opts)
    bf16_rows = cell.form == 0 and cell.plan[1] != A.ATTN_F32_ROWS
    worst = dict(err=0.0, ratio=0.0, mut=np.inf, mut_tol=np.inf)
    try:
        for call in range(A.n_calls(cell.B)):
            c = Call(H, cell, call)
            _place(H, c)
            for layer in LAYERS:
                dev = [_probe(H, cell, c, layer, i) for i in range(c.nq)]
                for b in range(c.B):
                    K, V = H.hist(c.slots[b], layer)
                    t, q = c.ts[b], c.q[layer, b]
                    ref, w = A.attention_fp64(q, K, V, t)
                    tol = A.tolerance(cell.kv, ref, bf16_rows)
                    if layer == 0:  # the inputs are sensitive: no single-key mistake fits under the bound
                        for d in A.mutation_effects(q, K, V, t, c.spiked[layer, b], ref, w):
                            worst["mut"] = min(worst["mut"], float(np.abs(d).max(axis=-1).min()))
                            worst["mut_tol"] = min(worst["mut_tol"], float(
                                (np.abs(d) / tol.reshape(-1, A.NH, A.HD)).max(axis=-1).min()))
                    for i in range(q.shape[0]):
                        out, po, pml = dev[i]
                        got = out[b] if cell.form == 0 else A.merge_fp64(po[b], pml[b], _n_splits(cell, t))
                        assert np.isfinite(got).all(), (call, layer, b, i)
                        d = np.abs(got - ref[i])
                        worst["err"] = max(worst["err"], float(d.max()))
                        worst["ratio"] = max(worst["ratio"], float((d / tol[i]).max()))
            e.check_errors()
    finally:
        _set_opts(e, {})
    if not bf16_rows:
        MEASURED[cell.kv] = max(MEASURED.get(cell.kv, 0.0), worst["err"])
    print(f"\n[attn_probe {A.cell_id(cell)}] plan {cell.plan} form {cell.form}: max |device - fp64| {worst['err']:.3e} "
          f"({'bf16 rows' if bf16_rows else 'fp32 output'}), {worst['ratio']:.3f} of the bound; single-key mutation >= "
          f"{worst['mut']:.3f} = {worst['mut_tol']:.0f} x the bound; fp32-output maximum so far {MEASURED.get(cell.kv)}")
    assert A.ATTN_ABS[cell.kv] <= A.ATTN_ABS_CAP
    assert worst["mut"] >= A.MUTATION_MIN and worst["mut_tol"] >= A.MUTATION_OVER_TOL
    assert worst["ratio"] <= 1.0


def _stale_rows(t):
    """The rows after the last key up to the end of its 128-key tile (the kernels load them unconditionally)."""
    return t, min((t + 127) // 128 * 128, A.MAX_POSITIONS)


@pytest.mark.parametrize("cell", CELLS, ids=A.cell_id)
def test_stale_rows_do_not_reach_the_output(hists, cell):
    """The cache rows past a slot's position hold whatever was there: with them set to a finite poison (K
    along the head's query at the largest finite magnitude of the dtype, V +-384) and to NaN bit patterns,
    the output equals the unpoisoned run bit for bit and is finite."""
    H = hists(cell.kv)
    e = H.e
    dev = e.device
    _set_opts(e, cell.opts)
    rng = np.random.default_rng(cell.B)

    def outputs(c, layer):
        """Per row: what the kernels wrote (compared bit for bit) and the row it stands for (finite)."""
        out, po, pml = _probe(H, cell, c, layer, 0)
        if cell.form == 0:
            return [(out[b], out[b]) for b in range(c.B)]
        ns = [_n_splits(cell, t) for t in c.ts]  # (an empty trailing split legitimately carries m = -inf)
        return [(np.concatenate([po[b][:, :ns[b]].ravel(), pml[b][:, :ns[b]].ravel()]), A.merge_fp64(po[b], pml[b], ns[b]))
                for b in range(c.B)]

    try:
        for call in range(A.n_calls(cell.B)):
            c = Call(H, cell, call)
            _place(H, c)
            clean = {layer: outputs(c, layer) for layer in LAYERS}
            for kind in ("finite", "nan"):
                try:
                    for layer in LAYERS:
                        for b in range(c.B):
                            r0, r1 = _stale_rows(c.ts[b])
                            if r1 <= r0:
                                continue
                            if kind == "nan":
                                bits = torch.full((r1 - r0, A.D), NAN_BITS[cell.kv], dtype=torch.int32, device=dev)
                                e.kv_write(c.slots[b], layer, r0, bits, bits, raw=True)
                            else:
                                q = c.q[layer, b][0].astype(np.float64)  # [8][96]
                                kd = (q / np.abs(q).max(axis=1, keepdims=True) * MAX_FINITE[cell.kv]).reshape(1, A.D)
                                k = np.repeat(kd, r1 - r0, axis=0).astype(np.float32)
                                v = (384.0 * rng.choice([-1.0, 1.0], size=(r1 - r0, A.D))).astype(np.float32)
                                e.kv_write(c.slots[b], layer, r0, torch.from_numpy(k).to(dev), torch.from_numpy(v).to(dev))
                    for layer in LAYERS:
                        got = outputs(c, layer)
                        for b in range(c.B):
                            assert np.isfinite(got[b][1]).all(), (kind, call, layer, b, c.ts[b])
                            assert np.array_equal(got[b][0], clean[layer][b][0]), (kind, call, layer, b, c.ts[b])
                finally:  # the history back in place
                    for layer in LAYERS:
                        for b in range(c.B):
                            r0, r1 = _stale_rows(c.ts[b])
                            if r1 > r0:
                                K, V = H.hist(c.slots[b], layer)
                                e.kv_write(c.slots[b], layer, r0, torch.from_numpy(K[r0:r1]).to(dev),
                                           torch.from_numpy(V[r0:r1]).to(dev))
            e.check_errors()
    finally:
        _set_opts(e, {})


@pytest.mark.parametrize("cell", A.idle_cells(), ids=A.cell_id)
def test_idle_row_in_the_middle(hists, cell):
    """One slot -1 in the middle of the call: its output row stays as the previous call left it (zeros where
    the kernels define it: ATTN_F32_ROWS and the merge kernel), and the live rows equal the call without it."""
    H = hists(cell.kv)
    e = H.e
    B = cell.B
    _set_opts(e, cell.opts)
    try:
        c = Call(H, cell, 0)
        _place(H, c)
        idle = B // 2
        with_idle = list(c.slots)
        with_idle[idle] = -1
        for layer in LAYERS:
            full = _probe(H, cell, c, layer, 0)
            part = _probe(H, cell, c, layer, 0, slots=with_idle)
            zero = cell.merged or cell.plan[1] == A.ATTN_F32_ROWS
            live = [b for b in range(B) if b != idle]
            if cell.form == 0:
                assert np.array_equal(part[0][live], full[0][live]), layer
                assert np.array_equal(part[0][idle], np.zeros(A.D, np.float32) if zero else full[0][idle]), layer
            else:  # the partials: the splits each live row wrote; the idle row's are not written
                for a, p in zip(full[1:], part[1:]):
                    for b in live:
                        ns = _n_splits(cell, c.ts[b])
                        assert np.array_equal(p[b][:, :ns], a[b][:, :ns]), (layer, b)
                    assert np.array_equal(p[idle], a[idle]), layer
        e.check_errors()
    finally:
        _set_opts(e, {})


def test_probe_rejects_the_k_split_attention(hists):
    """fp32 at 3 <= B <= 32 with default options sums c_attn's K slices inside the attention: no q rows."""
    from llmvox_amd import _lib
    H = hists("fp32")
    st = torch.arange(4, dtype=torch.int32, device=H.e.device)
    with pytest.raises(_lib.LvxError) as ei:
        H.e.attn_probe(st, 0, torch.zeros(4, A.D))
    assert ei.value.code == _lib.LVX_E_STATE


def test_zz_measured_maxima():
    """The figures of this run for DESIGN.md section 2 (attn_ref.ATTN_ABS_MEASURED is set from them)."""
    print(f"\n[attn_probe] largest |device - fp64| on the fp32 output forms per KV dtype: {MEASURED}; "
          f"bounds in force {A.ATTN_ABS}")
    for kv, m in MEASURED.items():
        assert 8.0 * m <= A.ATTN_ABS_CAP, (kv, m)
        assert m <= A.ATTN_ABS[kv]
