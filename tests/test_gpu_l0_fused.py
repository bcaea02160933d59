"""The fused layer-0 attention (option l0a 1: ar_attn_l0_kernel runs the previous step's select and layer 0's
q / k / v from the q0 tables for its own (row, head), then the attention) against the two launches it replaces
(l0a 0: ar_q0_rows_kernel, then the plain attention), on one engine, bit for bit: every output is the same
per-column expression of the same inputs in the same reduction order, so there is no tolerance.

Cells: the plan cells that take the fused form, B in {9, 17, 32} with bf16 KV (9: the smallest; 17: the first
with two batch tiles) and B in {17, 32} with fp8 KV. Each run has
  * rows at their first step (position 0: the codebook half of the input is zero, and the only key is the
    block's own),
  * a ragged batch: every third row decodes a 62-step prefix first, so those rows cross the 64-key chunk /
    tile boundary (62 -> 67 and on) while the others sit at 0 -> 5 and on,
  * a permuted slot order and one idle row (slot -1), whose plan step and token buffer must stay untouched,
  * either one call of 6 steps or the calls 3, 17 (a 16-step graph and a 1-step graph), 2: the end-of-call
    commit and the record hand-over between calls, on the graph-replay path (a side stream) and eagerly.
Compared: tok_plan and margin_plan over every step, rowstep, last_logits, and layer 0's K / V rows at every
appended position."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
MAXPOS = 256
PREFIX = 62
CELLS = [("bf16", 9), ("bf16", 17), ("bf16", 32), ("fp8", 17), ("fp8", 32)]


@pytest.fixture(scope="module")
def engines():
    """one engine per KV dtype, built when first asked for"""
    from llmvox_amd.engine import build_engine
    made = {}

    def get(kv):
        if kv not in made:
            made[kv] = build_engine(0, "bf16", kv, max_streams=32, max_positions=MAXPOS, max_codec_frames=64)
        return made[kv]
    yield get
    for e in made.values():
        e.close()


def _texts(B, n, seed):
    return np.random.default_rng(seed).integers(3, 384, size=(B, n)).astype(np.int32)


def _decode(e, B, calls, graphs, opts):
    """Rows 0 .. B - 1 in a permuted slot order with row B // 2 idle; every third live row first decodes
    PREFIX steps (in a batch of its own, under the same options), then all rows run `calls`."""
    dev = e.device
    for k, v in opts.items():
        e.set_option(k, v)
    n = PREFIX + sum(calls)
    texts = _texts(B, n, seed=100 + B)
    slots = np.random.default_rng(B).permutation(32)[:B].astype(np.int32)
    idle = B // 2
    slots[idle] = -1
    pre = [b for b in range(0, B, 3) if b != idle]
    stream = torch.cuda.Stream(device=dev) if graphs else torch.cuda.current_stream(dev)
    if graphs:
        stream.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(stream):
        for s in range(32):
            e.reset_slot(s)
        tok = torch.full((B, n), -7, dtype=torch.int32, device=dev)
        mar = torch.full((B, n), -7.0, dtype=torch.float32, device=dev)
        rowstep = torch.zeros(B, dtype=torch.int32, device=dev)
        # the prefix: rows `pre` alone, into their own buffers, copied into the full ones
        plan_p = torch.from_numpy(texts[pre].copy()).to(dev)
        slots_p = torch.from_numpy(slots[pre].copy()).to(dev)
        rs_p = torch.zeros(len(pre), dtype=torch.int32, device=dev)
        tok_p = torch.full((len(pre), n), -7, dtype=torch.int32, device=dev)
        mar_p = torch.full((len(pre), n), -7.0, dtype=torch.float32, device=dev)
        e.ar_steps(PREFIX, slots_p, plan_p, rs_p, tok_p, mar_p)
        tok[pre] = tok_p
        mar[pre] = mar_p
        rowstep[pre] = rs_p
        plan = torch.from_numpy(texts.copy()).to(dev)
        slots_d = torch.from_numpy(slots.copy()).to(dev)
        for c in calls:
            e.ar_steps(c, slots_d, plan, rowstep, tok, mar)
        e.check_errors()
        lg = e.last_logits(B).cpu().numpy()
        kv = []
        for b in range(B):
            if slots[b] < 0:
                continue
            p0 = PREFIX if b in pre else 0
            k, v = e.kv_read(int(slots[b]), 0, 0, p0 + sum(calls))
            kv.append((k.cpu().numpy(), v.cpu().numpy()))
    if graphs:
        torch.cuda.current_stream(dev).wait_stream(stream)
    torch.cuda.synchronize()
    return dict(tok=tok.cpu().numpy(), mar=mar.cpu().numpy(), rowstep=rowstep.cpu().numpy(), lg=lg, kv=kv,
                idle=idle, pre=pre)


def _restore(e):
    e.set_option("l0a", 1)
    e.set_option("defer_select", 1)


@pytest.mark.parametrize("graphs", [1, 0], ids=["graphs", "eager"])
@pytest.mark.parametrize("calls", [(6,), (3, 17, 2)], ids=["6", "3-17-2"])
@pytest.mark.parametrize("kv,B", CELLS)
def test_fused_layer0_is_bit_identical_to_the_two_launches(engines, kv, B, calls, graphs):
    eng = engines(kv)
    try:
        ref = _decode(eng, B, calls, graphs, {"l0a": 0})
        got = _decode(eng, B, calls, graphs, {"l0a": 1})
    finally:
        _restore(eng)
    idle, pre, n_main = ref["idle"], ref["pre"], sum(calls)
    for r in (ref, got):  # the idle row is untouched, every live row advanced by all its steps
        assert r["rowstep"][idle] == 0 and (r["tok"][idle] == -7).all() and (r["mar"][idle] == -7.0).all()
        for b in range(B):
            if b != idle:
                n_b = n_main + (PREFIX if b in pre else 0)
                assert r["rowstep"][b] == n_b and (r["tok"][b, :n_b] >= 0).all() and (r["tok"][b, n_b:] == -7).all()
    np.testing.assert_array_equal(got["tok"], ref["tok"])
    np.testing.assert_array_equal(got["mar"].view(np.uint32), ref["mar"].view(np.uint32))
    np.testing.assert_array_equal(got["rowstep"], ref["rowstep"])
    live = [b for b in range(B) if b != idle]
    np.testing.assert_array_equal(got["lg"][live].view(np.uint32), ref["lg"][live].view(np.uint32))
    assert len(got["kv"]) == len(ref["kv"]) == B - 1
    for (kg, vg), (kr, vr) in zip(got["kv"], ref["kv"]):
        assert np.abs(kr).max() > 0 and np.abs(vr).max() > 0  # the rows were appended
        np.testing.assert_array_equal(kg.view(np.uint32), kr.view(np.uint32))
        np.testing.assert_array_equal(vg.view(np.uint32), vr.view(np.uint32))


@pytest.mark.parametrize("B", [9, 32])
def test_fused_select_agrees_with_the_argmax_kernel_on_the_same_logits(engines, B):
    """The fused kernel's select held to ar_argmax_kernel with nothing else changed: the same run as one-step
    calls, where the call's only step has no pending select (the fused kernel skips its select chain) and
    ar_argmax_kernel commits the step at the end of the call, so every token is the argmax kernel's. The
    layers are the same kernels with the same inputs either way, so every step's logits are the same bits,
    and tokens, margins, logits and K / V must be too."""
    eng = engines("bf16")
    try:
        ref = _decode(eng, B, (1,) * 22, 1, {"l0a": 1})
        got = _decode(eng, B, (3, 17, 2), 1, {"l0a": 1})
    finally:
        _restore(eng)
    np.testing.assert_array_equal(got["tok"], ref["tok"])
    np.testing.assert_array_equal(got["mar"].view(np.uint32), ref["mar"].view(np.uint32))
    np.testing.assert_array_equal(got["rowstep"], ref["rowstep"])
    live = [b for b in range(B) if b != ref["idle"]]
    np.testing.assert_array_equal(got["lg"][live].view(np.uint32), ref["lg"][live].view(np.uint32))
    for (kg, vg), (kr, vr) in zip(got["kv"], ref["kv"]):
        np.testing.assert_array_equal(kg.view(np.uint32), kr.view(np.uint32))
        np.testing.assert_array_equal(vg.view(np.uint32), vr.view(np.uint32))


@pytest.mark.parametrize("kv,B", [("bf16", 9), ("bf16", 32), ("fp8", 32)])
def test_position_overflow_is_raised_alike(engines, kv, B):
    """Rows that reach max_positions: both forms clamp the position, set the capacity error word (raised by
    check_errors as LvxCapacityError) and leave the same tokens and positions."""
    eng = engines(kv)
    from llmvox_amd import _lib
    dev = eng.device
    texts = _texts(B, 8, seed=B)
    res = []
    try:
        for l0a in (0, 1):
            eng.set_option("l0a", l0a)
            for s in range(32):
                eng.reset_slot(s)
            for s in range(B):
                eng.set_slot(s, MAXPOS - 2 - (s % 2), 5 + s)
            plan = torch.from_numpy(texts.copy()).to(dev)
            slots = torch.arange(B, dtype=torch.int32, device=dev)
            rowstep = torch.zeros(B, dtype=torch.int32, device=dev)
            tok = torch.full((B, 8), -7, dtype=torch.int32, device=dev)
            eng.ar_steps(5, slots, plan, rowstep, tok)
            with pytest.raises(_lib.LvxCapacityError):
                eng.check_errors()
            eng.check_errors()  # taken: clear again
            res.append((tok.cpu().numpy(), rowstep.cpu().numpy(), [eng.slot_position(s) for s in range(B)],
                        eng.last_logits(B).cpu().numpy()))
    finally:
        _restore(eng)
    (t0, r0, p0, l0), (t1, r1, p1, l1) = res
    np.testing.assert_array_equal(t1, t0)
    np.testing.assert_array_equal(r1, r0)
    assert p1 == p0
    np.testing.assert_array_equal(l1.view(np.uint32), l0.view(np.uint32))


# --- the fused form against option defer_select 0 --------------------------------------------------------
# With defer_select 0 the step has no table form: layer 0's c_attn is the GEMM on the bf16-rounded
# LayerNorm'd operand, while the tables multiply it unrounded (include/llmvox.h, option "l0q": "the sums
# differ from the GEMM's in the last bits"; tests/test_gpu_batched.py bounds the logit difference of one
# step by 0.02 max|logit|). Tokens of the two plans can therefore agree over a run only where every
# select of the run is decided by more than that difference. The seeded synthetic weights are not such a
# model: their logits are near-uniform, the smallest top1 - top2 margin of this run is 4.9e-05 (B = 9) /
# 8.9e-05 (B = 32), and on MI355X 35 of 756 / 177 of 2,688 token cells differ from defer_select 0, for the
# two-launch form (l0a 0) exactly as for the fused one. So this check runs on a model with decided selects:
# the synthetic set with (a) the residual branches' c_proj weights x 0.1, so that the embedding row
# dominates the final residual, and (b) an lm_head that reads the embedding back: row v holds codebook row
# perm[v] in the codebook half and, for v < 384, 0.8 x text row v in the text half. A step's logits then
# peak at the v with perm[v] = previous token (at position 0, where the codebook half is zero, at v = text
# id), with top1 - top2 of a quarter of the peak and more (on MI355X 110 .. 355 against max |logit| 434), and
# the tokens walk the permutation: every row decodes its own varying
# sequence, through all four layers, the KV history and the deferred select. The test asserts the
# precondition itself: every margin of the defer_select 0 run exceeds 0.1 max|logit|, five times the
# one-step bound (the drift of the two plans' K / V histories is of the same order as that bound).
def _decided_weights():
    from llmvox_amd import weights as LW
    gw, cw, tt = LW.synthetic_all(1234)
    gw = dict(gw)
    for k in gw:
        if k.endswith("c_proj.weight"):
            gw[k] = (gw[k] * np.float32(0.1)).astype(np.float32)
    cb = np.asarray(cw[LW.CODEBOOK_KEY], dtype=np.float32)
    assert cb.shape == (4096, 512) and tt.shape[1] == 256
    perm = np.random.default_rng(5).permutation(4096)
    lm = np.zeros((4096, 768), dtype=np.float32)
    lm[:, 256:] = cb[perm]
    lm[:384, :256] = np.float32(0.8) * tt[:384]
    gw["lm_head.weight"] = lm
    return gw, cw, tt


@pytest.fixture(scope="module")
def decided_engine():
    from llmvox_amd.engine import build_engine
    e = build_engine(0, "bf16", "bf16", max_streams=32, max_positions=MAXPOS, max_codec_frames=64,
                     weights=_decided_weights())
    yield e
    e.close()


@pytest.mark.parametrize("B", [9, 32])
def test_fused_layer0_tokens_agree_with_defer_select_0(decided_engine, B):
    """Option defer_select 0 (ar_argmax_kernel after every lm_head, layer 0 from the GEMM) against the fused
    form over the same run (ragged prefix, permuted slots, an idle row, the calls 3, 17, 2 replayed as
    graphs): the same tokens, plan steps and positions, on the model whose selects are decided (above)."""
    eng = decided_engine
    calls = (3, 17, 2)
    try:
        ref = _decode(eng, B, calls, 1, {"defer_select": 0})
        got = _decode(eng, B, calls, 1, {"defer_select": 1, "l0a": 1})
    finally:
        _restore(eng)
    idle = ref["idle"]
    live = [b for b in range(B) if b != idle]
    done = ref["tok"][live] >= 0
    margins = ref["mar"][live][done]
    top = float(np.abs(ref["lg"][live]).max())
    d = got["tok"] != ref["tok"]
    print(f"B={B}: {int(d.sum())} of {d.size} token cells differ from defer_select 0; margins of the argmax run "
          f"{margins.min():.3f} .. {margins.max():.3f}, max |logit| {top:.3f}, "
          f"{len(np.unique(ref['tok'][live][done]))} distinct tokens in {int(done.sum())} cells")
    assert margins.min() > 0.1 * top  # the precondition: every select of the run is decided
    assert len(np.unique(ref["tok"][live][done])) > done.sum() // 2  # (the rows decode varying sequences)
    np.testing.assert_array_equal(got["rowstep"], ref["rowstep"])
    np.testing.assert_array_equal(got["tok"], ref["tok"])
    assert got["rowstep"][idle] == 0 and (got["tok"][idle] == -7).all()


