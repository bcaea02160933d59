"""tests/ar_ref.py without a GPU: the fp64 model of the AR step's ops is the pinned oracle in double precision,
the yardsticks of tests/test_gpu_ar_ops.py's bounds are what the model gives, the plan table is ar_plan.h's, and
the inputs are sensitive: every listed defect moves the compared quantity of its op by at least 10 x the bound of
that op in every mode it can occur in.
"""
import os
import subprocess

import numpy as np
import pytest
import torch

from llmvox_amd import weights as LW
from oracle import reference_cpu as O
from tests import ar_ref as R
from tests import attn_ref as A
from tests.test_ar_plan import _hipcc

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def W():
    gw, cw, tt = LW.synthetic_all(1234)
    return gw, tt, cw[R.CODEBOOK_KEY]


@pytest.fixture(scope="module")
def golden_decode(W):
    """The 256 golden steps decoded by the fp32-mode model in float64 (teacher-forced on the golden ids):
    (logits [256][4096], largest |mean| / std of x entering ln_2 with its (step, layer))."""
    g = np.load(os.path.join(GOLDEN, "ar_golden.npz"))
    text_ids, ids = g["text_ids"].tolist(), g["ids"].tolist()
    m = R.model_for(W, "f32", torch.float64)
    n = len(ids)
    K = [torch.zeros(n, R.D, dtype=torch.float64) for _ in range(R.NL)]
    V = [torch.zeros(n, R.D, dtype=torch.float64) for _ in range(R.NL)]
    logits, worst = [], (0.0, -1, -1)
    for i in range(n):
        tr = {}
        rows = ([text_ids[i] if i < len(text_ids) else 384], [ids[i - 1] if i else 0], [i])
        res = m.window(0, R.LM_HEAD, rows, hist=lambda l, b: (K[l], V[l]), trace=tr)
        for l in range(R.NL):
            K[l][i], V[l][i] = tr["k", l][0], tr["v", l][0]
            x2 = tr["x2", l][0]
            worst = max(worst, (float(x2.mean().abs() / x2.std(unbiased=False)), i, l))
        logits.append(res["logits"][0])
    return torch.stack(logits), worst, text_ids, ids


def test_fp32_mode_is_the_oracle(W, golden_decode):
    """The model's decode of the golden sentence against oracle.reference_cpu.gpt_forward (the causal
    full-sequence pass over the same ids), at the fp32 parity bar of the GPU tests."""
    logits, _, text_ids, ids = golden_decode
    gw, tt, cb = W
    n = len(ids)  # all 256 golden steps
    lg = O.teacher_forced_logits(O.to_torch(gw), torch.from_numpy(tt), torch.from_numpy(cb), text_ids, ids[:n])
    err = float((logits[:n] - lg.double()).abs().max())
    print(f"\n[ar_ref] fp32 mode against the oracle over {n} golden steps: max |dlogit| {err:.3e}")
    assert err < 2e-5
    assert logits.argmax(dim=-1).tolist() == ids


def test_mean_over_std_of_the_golden_steps(golden_decode):
    """R.MEAN_OVER_STD is the largest |mean| / std of x entering ln_2 over the 256 golden steps."""
    _, (m, step, layer), _, _ = golden_decode
    print(f"\n[ar_ref] largest |mean| / std of x entering ln_2: {m:.5f} at step {step}, layer {layer}")
    assert 0.99 * R.MEAN_OVER_STD <= m <= R.MEAN_OVER_STD


def test_cells_are_the_plan(tmp_path):
    """Every cell's info against ar_plan_step itself (the header compiles without a GPU)."""
    src = tmp_path / "dump.cpp"
    lines = []
    for c in R.cells():
        o = {**R.DEFAULT_OPTS, **c.opts}
        wd, kvd = R.ENGINES[c.eng]
        dt = {"fp32": "LVX_DTYPE_F32", "bf16": "LVX_DTYPE_BF16", "fp8": "LVX_DTYPE_FP8"}
        lines.append(f'  {{ Opts o; o.bt = {o["bt"]}; o.ln_max = {o["ln_max"]}; o.exp = {o["exp"]}; o.f32b = {o["f32b"]}; '
                     f'o.fuse_mlp = {o["fuse_mlp"]}; ArStepPlan p = ar_plan_step(o, {dt[wd]}, {dt[kvd]}, {c.B}, false, false); '
                     'printf("%d %d %d %d %d %d %d %d\\n", (int)p.path, (int)p.fused_mlp, p.nsplit, p.attn_direct, '
                     '(int)p.attn8, p.xpk, (int)p.ksplit, (int)p.qsplit); }')
    src.write_text('#include "ar_plan.h"\nusing namespace lvx;\nint main() {\n' + "\n".join(lines) + "\n  return 0;\n}\n")
    exe = tmp_path / "dump"
    cc = _hipcc()
    if cc is None:
        pytest.skip("no hipcc to build the plan program with")
    # host-only, as tests/test_ar_plan.py builds its program: the header has no kernels
    subprocess.run([cc, "-O1", "-std=c++17", "-x", "hip", "--offload-host-only", "-I", os.path.join(ROOT, "include"),
                    "-I", os.path.join(ROOT, "llmvox_amd", "csrc"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()
    assert len(out) == len(R.cells())
    for c, line in zip(R.cells(), out):
        plan = tuple(int(v) for v in line.split())
        assert plan == c.info[:8], R.cell_id(c)
        # the pending copies follow from the plan (ar_kernels.hip: YCOPIES 4 fixed-point accumulators of the fused MLP,
        # YCS 2 K slices under PATH_MFMA_LN, YCOPIES K slices under PATH_MFMA_ROWS and the fp32 K split)
        path, fused, ksplit = plan[0], plan[1], plan[6]
        copies = 4 if fused else 2 if path == R.MLN else 4 if (path == R.MROWS or ksplit) else 0
        assert c.info[8:] == (copies, fused), R.cell_id(c)
        assert copies == R.copies_of(c.mode, R.cell_ksplit(c)), R.cell_id(c)


@pytest.fixture(scope="module")
def yardsticks(W):
    return R.ensure_yardsticks(W)


def test_yardsticks(yardsticks):
    """Every (op kind, mode) of the cells has a yardstick of fp32 size: one op of K <= 3,072-term sums evaluated in
    float32 stays within fp32 eps 6e-8 x sqrt(3,072) = 3.3e-6 of float64 per element; c_proj's compared quantity is
    the attention branch alone, a difference of rows (allowed 3 x that). A model that rounds where it should not, or
    a tie flip that leaks into a figure, is 1e-4 or more."""
    for key in sorted(yardsticks):
        print(f"[ar_ref] yardstick {key}: {yardsticks[key]:.3e}, bound {R.MARGIN * yardsticks[key]:.3e}")
    want = {(R.kind_of(w, n), c.mode) for c in R.cells() for w in R.windows(c)
            for n in (("logits", "logits_tail") if w[1] == R.LM_HEAD else (None,))}
    assert set(yardsticks) == want
    for (kind, mode), v in yardsticks.items():
        assert 0.0 < v <= (1e-5 if kind == "c_proj" else 3.3e-6), (kind, mode, v)


def test_adjacent_rows_are_far_apart(W, yardsticks):
    """A misplaced row cannot pass: adjacent reference rows differ by more than 50 x the bound, in every window."""
    worst = np.inf
    for c in R.cells():
        case = R.Case(c)
        m = R.model_for(W, c.mode, torch.float64, R.cell_ksplit(c))
        for win, (_, _, ref, _, _) in R.model_chain(case, m).items():
            for name, r in R.compared(ref, win).items():
                if name == "logits_tail":  # (a misplaced row shows in the whole row of logits)
                    continue
                ratio = R.adjacent_row_distance(r.numpy()) / R.bound(R.kind_of(win, name), c.mode)
                worst = min(worst, ratio)
                assert ratio >= R.MIN_ROW_DISTANCE, (R.cell_id(c), win, name, ratio)
    print(f"\n[ar_ref] adjacent reference rows: at least {worst:.0f} x the bound apart")


# ----------------------------------------------------------------------------------------------------------
# Mutations: (name, window, compared tensor, [(mode, B)], what it stands for). B: the smallest at which the defect
# can occur in that mode's cells. Rows sit in slots 8, 9, ...: positions 0, 1, 63, ... (row 0 at position 0).
# ----------------------------------------------------------------------------------------------------------
ALL = [("f32", 3), ("gemv", 1), ("fused", 1), ("ln", 3), ("rows", 9), ("bt", 33)]
NO_FUSED = [m for m in ALL if m[0] != "fused"]
COPIES = [("f32", 3), ("fused", 1), ("ln", 3), ("rows", 9)]
ROW16 = [("f32", 17), ("gemv", 65), ("rows", 17), ("bt", 33)]
TWO_ROWS = [("f32", 3), ("gemv", 2), ("fused", 2), ("ln", 3), ("rows", 9), ("bt", 33)]
MUTATIONS = [
    ("k_tail32", (5, 5, "x"), "q", ALL, "last 32 of K = 768 dropped"),
    ("k_slice192", (5, 5, "x"), "q", ALL, "one 192-wide K slice dropped"),
    ("k_slice768", (5, 9, "x"), "d", ALL, "one 768-wide K slice of mlp c_proj dropped"),
    ("fc_tail8", (5, 8, "x"), "h", NO_FUSED, "last 8 of c_fc's 3,072 outputs dropped"),
    ("fc_tail8", (5, 9, "x"), "d", [("fused", 1)], "last 8 of c_fc's 3,072 outputs dropped (fused MLP)"),
    ("copy_unfolded", (5, 9, "x"), "d", COPIES, "one pending copy not folded"),
    ("copy_twice", (5, 9, "x"), "d", COPIES, "one pending copy folded twice"),
    ("copy_l0_stale", (0, 0, "x"), "q", COPIES, "the pending copies not cleared at layer 0"),
    ("ln_prev_row", (5, 5, "x"), "q", TWO_ROWS, "row b normalised with row b - 1's statistics"),
    ("ln_prev_row", (5, 8, "x"), "h", [("rows", 9)], "row b's c_fc normalised with row b - 1's xstat"),
    ("row16_is_15", (5, 5, "x"), "q", ROW16, "row 16 a copy of row 15"),
    ("gsum_other_layer", (5, 8, "x"), "h", [("rows", 9)], "fc_gsum of another layer"),
    ("ln2_other_layer", (5, 8, "x"), "h", NO_FUSED, "ln_2.weight of another layer"),
    ("ln2_other_layer", (5, 9, "x"), "d", [("fused", 1)], "ln_2.weight of another layer (fused MLP)"),
    ("ln1_for_ln2", (5, 8, "x"), "h", NO_FUSED, "ln_1.weight in place of ln_2.weight"),
    ("ln1_for_ln2", (5, 9, "x"), "d", [("fused", 1)], "ln_1.weight in place of ln_2.weight (fused MLP)"),
    ("no_residual", (5, 7, "x"), "d", ALL, "residual omitted in c_proj"),
    ("no_residual", (5, 9, "x"), "d", ALL, "residual omitted"),
    ("next_layer_weight", (5, 5, "x"), "q", ALL, "the next layer's weight"),
    ("q767_zero", (5, 5, "x"), "q", ALL, "q column 767 zeroed"),
    ("kv_swap", (5, 5, "x"), "k", ALL, "k and v exchanged"),
    ("wpe_next", (0, 0, "x"), "q", ALL, "wpe[p + 1]"),
    ("no_den", (0, 0, "x"), "q", ALL, "den omitted"),
    ("code_at_p0", (0, 0, "x"), "q", ALL, "the code half not zero at position 0"),
    ("vocab4095_from_4094", (15, 20, "x"), "logits_tail", ALL, "vocabulary row 4,095 taken from 4,094"),
    ("erf_gelu", (5, 8, "x"), "h", [("f32", 3)], "erf GELU for the tanh form (fp32 only)"),
    ("unbiased_var", (5, 5, "x"), "q", [("f32", 3)], "the unbiased variance (fp32 only)"),
]
MODE_CELL = {"f32": ("fp32", (R.F32B, 0, 8, 0, 0, 0, 1, 1, 4, 0)), "gemv": ("bf16", (R.GEMV, 0, 16, 0, 0, 0, 0, 0, 0, 0)),
             "fused": ("bf16", (R.GEMV, 1, 16, 0, 0, 0, 0, 0, 4, 1)), "ln": ("bf16", (R.MLN, 0, 8, 0, 0, 0, 0, 0, 2, 0)),
             "rows": ("bf16", (R.MROWS, 0, 1, 2, 0, 1, 0, 0, 4, 0)), "bt": ("bf16", (R.BT, 0, 1, 0, 0, 0, 0, 0, 0, 0))}
MUTATION_OVER_BOUND = 10.0


def _mutation_ratio(W, name, win, tensor, mode, B):
    """The mutated op, from the buffers the unmutated float64 chain left before it, held as the GPU test holds the
    device: what its buffers would store (as_stored) against the resolved reference, dev_err over the bound."""
    eng, info = MODE_CELL[mode]
    cell = R.Cell(eng, B, {}, info, mode, True)
    case = R.Case(cell, slots=range(8, 8 + B))
    stale = None
    if name == "copy_l0_stale":  # stale copies at the scale of a real MLP branch (the hook's poison is 3.4e38)
        stale = torch.from_numpy(0.13 * np.random.default_rng(B).standard_normal((B, R.copies_of(mode), R.D)))
    m64 = R.model_for(W, mode, torch.float64)
    state, kv_rows = R.model_chain(case, m64, upto=win)[win][:2]
    mres = case.last_op(R.model_for(W, mode, torch.float64, mut={name}), win, state, kv_rows, stale=stale)
    dev = {n: (None if t is None else t.double().numpy()) for n, t in R.as_stored(mres, win).items()}
    ref = R.resolved_reference(case, m64, win, state, kv_rows, dev)
    return float(R.window_errors(case, m64, win, dev, ref)[tensor].max()) / R.bound(R.kind_of(win, tensor), mode)


@pytest.mark.parametrize("name,win,tensor,where,what", MUTATIONS, ids=[f"{m[0]}-{m[1][0]}_{m[1][1]}" for m in MUTATIONS])
def test_mutation_moves_its_op(W, yardsticks, name, win, tensor, where, what):
    for mode, B in where:
        ratio = _mutation_ratio(W, name, win, tensor, mode, B)
        print(f"[ar_ref] {what}: mode {mode}, B = {B}, window {win[0]}..{win[1]}: {ratio:.1f} x the bound")
        assert ratio >= MUTATION_OVER_BOUND, (name, mode, B, ratio)


def test_merge_maximum_over_all_splits_but_one_is_neutral(W):
    """The merge's maximum taken over the live splits but one changes no value in exact arithmetic (M scales the
    numerator and the denominator alike); in fp32 it matters once a split's maximum exceeds M by 88 (exp overflows),
    and the spiked queries put scores of ln(t) + 1 < 6 on their keys. No comparison with a reference can see
    this defect at these inputs: it is stated here, not counted among the mutations above."""
    cell = R.Cell("bf16", 1, {}, MODE_CELL["gemv"][1], "gemv", True)
    case = R.Case(cell, slots=[12])  # position 65: 66 keys, two live splits
    win = (11, 12, "q")
    x, q = case.inputs(win)
    ref = case.reference(R.model_for(W, "gemv", torch.float64), win, x, q)
    mut = case.reference(R.model_for(W, "gemv", torch.float64, mut={"merge_max_skip_one"}), win, x, q)
    assert len(A.split_ranges(66, 16, "bf16")) == 2
    assert float(R.row_err(mut["d"].numpy(), ref["d"].numpy()).max()) < 1e-12


def test_empty_trailing_split_in_the_merge(W, yardsticks):
    """An empty trailing split counted with weight exp(0) in the merge. It exists only past the histories the GPU
    test runs (16 splits: 1,025 keys under bf16 / fp8 KV, where split 15 starts at key 1,088 of 1,025): the GEMV
    family's c_proj (GIN_MERGE) over a synthetic 1,025-key history."""
    t = 1025
    assert A.split_ranges(t, 16, "bf16")[-1][0] >= t and all(a < b for a, b in A.split_ranges(130, 16, "bf16"))
    rng = np.random.default_rng(R.SEED)
    K = torch.from_numpy(A.quantise(0.7 * rng.standard_normal((t, R.D), dtype=np.float32), "bf16"))
    V = torch.from_numpy(A.quantise(rng.standard_normal((t, R.D), dtype=np.float32), "bf16"))
    qs, _ = A.row_queries(K.numpy(), t, A.edge_keys(t, 16, "bf16"), 0)
    q = torch.from_numpy(qs[0].reshape(1, R.D)).double()
    x = torch.from_numpy(R.x_rows(1, (6, 7))).double()
    out = {}
    for mut in (R.NONE, {"empty_split_exp0"}):
        m = R.model_for(W, "gemv", torch.float64, mut=mut)
        out[bool(mut)] = m.c_proj(1, x, m.store(m.attention(q, [K], [V], [t], 16, "bf16"))) - x
    ratio = float(R.row_err(out[True].numpy(), out[False].numpy()).max()) / R.bound("c_proj", "gemv")
    print(f"\n[ar_ref] an empty trailing split with weight exp(0): {ratio:.1f} x the bound")
    assert ratio >= MUTATION_OVER_BOUND
