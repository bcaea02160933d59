"""The fused layers form (option laf 1: at layers 1-3 every attention block (row, head) runs the row's LayerNorm and
its head's 288 c_attn rows itself, ar_attn_la_kernel, and c_proj folds the pending mlp copies into x) against the
launches it replaces (laf 0: ar_rows_kernel, the c_attn GEMM, the plain attention), on one engine and seeded
synthetic weights, bit for bit: the LayerNorm is the rows kernel's code, every q / k / v element is the same MFMA
chain over the same K slices summed in the same wave order, and the new key enters its softmax slot last either
way, so there is no tolerance.

Cells: B in {9, 17, 32} with bf16 KV (9: the smallest; 17: the first with two batch tiles in the two-launch
c_attn; 32: one block per CU) and B in {17, 32} with fp8 KV, max_positions 200, six steps per call. Rows start at
the positions {0, 1, 62, 63, 64, 65, 126, 127, 128} spread over the rows (the empty history, and both sides of
the 64-key tile edges, which the six steps then cross), over a seeded K / V history written into all four
layers. Cases: all rows live in slot order under graph replay; an idle row in the middle of the batch; rows in a
permuted slot order; eager (null-stream) calls; two calls of six steps (the records the head-0 blocks of layer 1
copy back are what the next call starts from); rows that reach max_positions (the capacity error).
Compared: tok_plan and margin_plan over every step, rowstep, the last step's logits, the slots' positions and
the K / V rows the steps appended in layers 1-3 (and 0). No entry point reads x out of a running step; x after
layer l's c_proj (and the copies folded into it) is what layer l + 1's appended K / V rows and, after layer 3,
the logits are computed from, so those comparisons hold it too."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
MAXPOS = 200
STARTS = [0, 1, 62, 63, 64, 65, 126, 127, 128]
STEPS = 6


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


@pytest.fixture(scope="module")
def history():
    """seeded K / V rows for positions 0 .. 127 of every layer (a slot reads them rotated by its number)"""
    g = np.random.default_rng(77)
    return [(g.standard_normal((128, 768)).astype(np.float32) * 0.5,
             g.standard_normal((128, 768)).astype(np.float32) * 0.5) for _ in range(4)]


def _decode(e, hist, B, calls, graphs, laf, idle=None, permute=False, starts=STARTS):
    dev = e.device
    e.set_option("laf", laf)
    n = sum(calls)
    texts = np.random.default_rng(300 + B).integers(3, 384, size=(B, n)).astype(np.int32)
    slots = (np.random.default_rng(B).permutation(32)[:B] if permute else np.arange(B)).astype(np.int32)
    if idle is not None:
        slots[idle] = -1
    start = [starts[(b * 4) % len(starts)] for b in range(B)]  # (4 and 9 coprime: every start position occurs)
    stream = torch.cuda.Stream(device=dev) if graphs else torch.cuda.current_stream(dev)
    if graphs:
        stream.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(stream):
        for s in range(32):
            e.reset_slot(s)
        hk = [(torch.from_numpy(k).to(dev), torch.from_numpy(v).to(dev)) for k, v in hist]
        for b in range(B):
            s = int(slots[b])
            if s < 0:
                continue
            e.set_slot(s, start[b], 5 + s)
            if start[b]:
                for layer in range(4):
                    k, v = hk[layer]
                    e.kv_write(s, layer, 0, torch.roll(k, s, 0)[:start[b]].contiguous(),
                               torch.roll(v, s, 0)[:start[b]].contiguous())
        tok = torch.full((B, n), -7, dtype=torch.int32, device=dev)
        mar = torch.full((B, n), -7.0, dtype=torch.float32, device=dev)
        rowstep = torch.zeros(B, dtype=torch.int32, device=dev)
        plan = torch.from_numpy(texts.copy()).to(dev)
        slots_d = torch.from_numpy(slots.copy()).to(dev)
        for c in calls:
            e.ar_steps(c, slots_d, plan, rowstep, tok, mar)
        e.check_errors()
        lg = e.last_logits(B).cpu().numpy()
        kv, pos = [], []
        for b in range(B):
            if slots[b] < 0:
                continue
            pos.append(e.slot_position(int(slots[b])))
            for layer in range(4):
                k, v = e.kv_read(int(slots[b]), layer, start[b], n)
                kv.append((k.cpu().numpy(), v.cpu().numpy()))
    if graphs:
        torch.cuda.current_stream(dev).wait_stream(stream)
    torch.cuda.synchronize()
    return dict(tok=tok.cpu().numpy(), mar=mar.cpu().numpy(), rowstep=rowstep.cpu().numpy(), lg=lg, kv=kv, pos=pos,
                start=start)


def _same(got, ref, B, n, idle):
    live = [b for b in range(B) if b != idle]
    for r in (ref, got):  # every live row advanced by all its steps, an idle row is untouched
        for b in range(B):
            if b == idle:
                assert r["rowstep"][b] == 0 and (r["tok"][b] == -7).all() and (r["mar"][b] == -7.0).all()
            else:
                assert r["rowstep"][b] == n and (r["tok"][b] >= 0).all()
        assert r["pos"] == [r["start"][b] + n for b in live]
    np.testing.assert_array_equal(got["tok"], ref["tok"])
    np.testing.assert_array_equal(got["mar"].view(np.uint32), ref["mar"].view(np.uint32))
    np.testing.assert_array_equal(got["rowstep"], ref["rowstep"])
    np.testing.assert_array_equal(got["lg"][live].view(np.uint32), ref["lg"][live].view(np.uint32))
    assert len(got["kv"]) == len(ref["kv"]) == 4 * len(live)
    for (kg, vg), (kr, vr) in zip(got["kv"], ref["kv"]):
        assert np.abs(kr).max() > 0 and np.abs(vr).max() > 0  # the rows were appended
        np.testing.assert_array_equal(kg.view(np.uint32), kr.view(np.uint32))
        np.testing.assert_array_equal(vg.view(np.uint32), vr.view(np.uint32))


CASES = [
    # kv, B, calls, graphs, idle row, permuted slots
    pytest.param("bf16", 9, (STEPS,), 1, None, False, id="bf16-9"),
    pytest.param("bf16", 17, (STEPS,), 1, None, False, id="bf16-17"),
    pytest.param("bf16", 32, (STEPS,), 1, None, False, id="bf16-32"),
    pytest.param("fp8", 17, (STEPS,), 1, None, False, id="fp8-17"),
    pytest.param("fp8", 32, (STEPS,), 1, None, False, id="fp8-32"),
    pytest.param("bf16", 17, (STEPS,), 1, 8, False, id="bf16-17-idle-row"),
    pytest.param("bf16", 9, (STEPS,), 1, None, True, id="bf16-9-permuted-slots"),
    pytest.param("bf16", 32, (STEPS,), 0, None, False, id="bf16-32-eager"),
    pytest.param("bf16", 32, (STEPS, STEPS), 1, None, False, id="bf16-32-two-calls"),
    pytest.param("fp8", 17, (STEPS, STEPS), 0, 3, True, id="fp8-17-two-calls-eager-idle-permuted"),
]


@pytest.mark.parametrize("kv,B,calls,graphs,idle,permute", CASES)
def test_fused_layers_are_bit_identical_to_the_separate_launches(engines, history, kv, B, calls, graphs, idle, permute):
    eng = engines(kv)
    try:
        ref = _decode(eng, history, B, calls, graphs, 0, idle, permute)
        got = _decode(eng, history, B, calls, graphs, 1, idle, permute)
    finally:
        eng.set_option("laf", 1)
    _same(got, ref, B, sum(calls), idle)


@pytest.mark.parametrize("kv,B", [("bf16", 9), ("fp8", 32)])
def test_position_overflow_is_raised_alike(engines, history, kv, B):
    """Rows that reach max_positions: both forms clamp the position, set the capacity error word (raised by
    check_errors as LvxCapacityError) and leave the same tokens, positions and logits."""
    eng = engines(kv)
    from llmvox_amd import _lib
    dev = eng.device
    texts = np.random.default_rng(B).integers(3, 384, size=(B, 8)).astype(np.int32)
    res = []
    try:
        for laf in (0, 1):
            eng.set_option("laf", laf)
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
        eng.set_option("laf", 1)
    (t0, r0, p0, l0), (t1, r1, p1, l1) = res
    np.testing.assert_array_equal(t1, t0)
    np.testing.assert_array_equal(r1, r0)
    assert p1 == p0
    np.testing.assert_array_equal(l1.view(np.uint32), l0.view(np.uint32))
