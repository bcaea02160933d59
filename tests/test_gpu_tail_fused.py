"""The two tail forms of a fused-layers step against the launches they replace, on one engine and seeded synthetic
weights, bit for bit.

xfold 1: at layers 1-3 the attention block (row, head) stores its 96-column stripe of x + the four pending mlp
copies (the sum it forms for its LayerNorm, in xrow_sum's order) into the second plane of x, and c_proj takes its
residual from there with one load; xfold 0: c_proj loads x and the copies and adds them in the same order.
lmf 1: ln_f of a row group and a vocab slice of lm_head in one launch (ar_lm_rows_kernel: the rows kernel's fold and
LayerNorm by the same functions, the same MFMA chain over the same K slices summed in the same wave order); lmf 0:
ar_rows_kernel and the lm_head GEMM. Neither changes the order of any floating-point operation, so there is no
tolerance.

Cells: bf16 KV at B = 9 (the smallest fused-layers cell, no multiple of the row group; the plan turns xfold on from
B = 16 only, so here it exercises that gate), 16 (the first cell with xfold, one batch tile in c_proj), 17 (one row
into a new group and batch tile), 31 (the last group one short) and 32; fp8 KV at B = 17 and 32; max_positions 200,
six steps per call. Rows start at the positions {0, 1, 62, 63, 64, 65, 126, 127, 128} spread over the rows, over a seeded K / V
history written into all four layers. Cases: all rows live in slot order under graph replay; an idle row in the
middle of the batch, inside a row group whose other rows are live; permuted slots; eager (null-stream) calls; two
calls of six steps; rows that reach max_positions (the capacity error). Every case decodes with (xfold, lmf) =
(0, 0), (1, 0), (0, 1) and (1, 1) and compares the last three with the first: tok_plan and margin_plan over every
step, rowstep, the last step's logits, the slots' positions and the K / V rows the steps appended in all four
layers (layer l + 1's rows are computed from x after layer l's c_proj, the logits from x after layer 3's).
B = 8 is outside the fused layers form: the plan gates both options off and the outputs are equal trivially."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
MAXPOS = 200
STARTS = [0, 1, 62, 63, 64, 65, 126, 127, 128]
STEPS = 6
FORMS = [(0, 0), (1, 0), (0, 1), (1, 1)]  # (xfold, lmf); the first is the reference


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
    """seeded K / V rows for positions 0 .. 127 of every layer (a slot reads them rotated by its number), on the host"""
    g = np.random.default_rng(78)
    return [(torch.from_numpy(g.standard_normal((128, 768)).astype(np.float32) * 0.5),
             torch.from_numpy(g.standard_normal((128, 768)).astype(np.float32) * 0.5)) for _ in range(4)]


def _decode(e, hist, B, calls, graphs, form, idle=None, permute=False):
    dev = e.device
    e.set_option("xfold", form[0])
    e.set_option("lmf", form[1])
    n = sum(calls)
    texts = np.random.default_rng(500 + B).integers(3, 384, size=(B, n)).astype(np.int32)
    slots = (np.random.default_rng(B).permutation(32)[:B] if permute else np.arange(B)).astype(np.int32)
    if idle is not None:
        slots[idle] = -1
    start = [STARTS[(b * 4) % len(STARTS)] for b in range(B)]  # (4 and 9 coprime: every start position occurs)
    stream = torch.cuda.Stream(device=dev) if graphs else torch.cuda.current_stream(dev)
    if graphs:
        stream.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(stream):
        for s in range(32):
            e.reset_slot(s)
        hk = [(k.to(dev), v.to(dev)) for k, v in hist]
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


def _all_forms(eng, hist, B, calls, graphs, idle=None, permute=False):
    try:
        res = [_decode(eng, hist, B, calls, graphs, f, idle, permute) for f in FORMS]
    finally:
        eng.set_option("xfold", 1)
        eng.set_option("lmf", 1)
    for f, got in zip(FORMS[1:], res[1:]):
        try:
            _same(got, res[0], B, sum(calls), idle)
        except AssertionError as ex:
            raise AssertionError(f"(xfold, lmf) = {f} against (0, 0): {ex}") from ex
    return res


CASES = [
    # kv, B, calls, graphs, idle row, permuted slots
    pytest.param("bf16", 9, (STEPS,), 1, None, False, id="bf16-9"),
    pytest.param("bf16", 16, (STEPS,), 1, None, False, id="bf16-16"),
    pytest.param("bf16", 17, (STEPS,), 1, None, False, id="bf16-17"),
    pytest.param("bf16", 31, (STEPS,), 1, None, False, id="bf16-31"),
    pytest.param("bf16", 32, (STEPS,), 1, None, False, id="bf16-32"),
    pytest.param("fp8", 17, (STEPS,), 1, None, False, id="fp8-17"),
    pytest.param("fp8", 32, (STEPS,), 1, None, False, id="fp8-32"),
    pytest.param("bf16", 17, (STEPS,), 1, 10, False, id="bf16-17-idle-row"),  # row 10: inside the group of rows 8-15
    pytest.param("bf16", 31, (STEPS,), 1, 13, False, id="bf16-31-idle-row"),
    pytest.param("bf16", 9, (STEPS,), 1, None, True, id="bf16-9-permuted-slots"),
    pytest.param("bf16", 32, (STEPS,), 0, None, False, id="bf16-32-eager"),
    pytest.param("bf16", 32, (STEPS, STEPS), 1, None, False, id="bf16-32-two-calls"),
    pytest.param("fp8", 17, (STEPS, STEPS), 0, 3, True, id="fp8-17-two-calls-eager-idle-permuted"),
]


@pytest.mark.parametrize("kv,B,calls,graphs,idle,permute", CASES)
def test_tail_forms_are_bit_identical_to_the_launches_they_replace(engines, history, kv, B, calls, graphs, idle, permute):
    _all_forms(engines(kv), history, B, calls, graphs, idle, permute)


def test_outside_the_fused_layers_form_the_options_change_nothing(engines, history):
    """B = 8: the plan is not la_fused, so neither x_folded nor lm_fused is set whatever the options say"""
    _all_forms(engines("bf16"), history, 8, (STEPS,), 1)


@pytest.mark.parametrize("kv,B", [("bf16", 9), ("fp8", 32)])
def test_position_overflow_is_raised_alike(engines, history, kv, B):
    """Rows that reach max_positions: every form clamps the position, sets the capacity error word (raised by
    check_errors as LvxCapacityError) and leaves the same tokens, positions and logits."""
    eng = engines(kv)
    from llmvox_amd import _lib
    dev = eng.device
    texts = np.random.default_rng(B).integers(3, 384, size=(B, 8)).astype(np.int32)
    res = []
    try:
        for xfold, lmf in FORMS:
            eng.set_option("xfold", xfold)
            eng.set_option("lmf", lmf)
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
        eng.set_option("xfold", 1)
        eng.set_option("lmf", 1)
    t0, r0, p0, l0 = res[0]
    for t1, r1, p1, l1 in res[1:]:
        np.testing.assert_array_equal(t1, t0)
        np.testing.assert_array_equal(r1, r0)
        assert p1 == p0
        np.testing.assert_array_equal(l1.view(np.uint32), l0.view(np.uint32))
