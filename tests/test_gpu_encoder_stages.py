"""Every stage of the WavTokenizer encoder against the fp64 model of tests/enc_ref.py, through the test hook
lvx_enc_stages (a window of one stage of lvx_encode's own stage list on a given input), at the shapes where
the kernels can go wrong: one frame (every conv with k > 1 zero-extended), inputs on either side of the pad,
with and without the extra right padding, three 64-row tiles with stream boundaries inside a tile, a second
and a third group of 16 LSTM streams, gates beyond expf's fp32 range, quantiser ties.

A stage with a residual or skip is compared on its branch (out - shortcut(in) for the residual blocks, out - in
for the SLSTM) relative to the reference branch's RMS over the call, the others on their output. The bound of
a cell is enc_ref.MARGIN x enc_ref.YARDSTICK: the deviation of the model evaluated in fp32 on the CPU from itself
in fp64 on the cell's own input (nothing the device computed enters it); tests/test_enc_ref.py shows every
indexing / omission error moving the compared quantity by >= 10 x it.

MEASURED collects the largest device error per (stage kind, shape class) with the yardstick beside it and is
printed at the end of the module (the figures in DESIGN.md section 2, "The encoder stage by stage").
"""
import os

import numpy as np
import pytest
import torch

from tests import enc_ref as ER

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
MAX_SAMPLES = 32000  # the largest golden edge case, 33 x 961


@pytest.fixture(scope="module")
def ctx():
    from llmvox_amd import weights as LW
    from llmvox_amd.encoder import WavEncoder
    W64, W32, cb = ER.load_weights()
    e = WavEncoder(0, LW.synthetic_encoder(1234), cb, max_samples=MAX_SAMPLES)
    yield e, W64, W32, cb
    e.close()


MEASURED = {}  # (stage kind, shape class) -> (largest device error, its yardstick)
LEFT_OUT = [0, 0]  # frames a code comparison left out, frames compared (from the reference's gaps alone)


def _record(kind, cls, err, yard):
    if err >= MEASURED.get((kind, cls), (-1.0, 0.0))[0]:
        MEASURED[kind, cls] = (err, yard)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\nencoder stages, largest device error / yardstick / bound per (stage kind, shape class):")
    for (kind, cls), (err, yard) in sorted(MEASURED.items()):
        print(f"  {kind:9s} {cls:10s} {err:.3e} / {yard:.3e} / {ER.MARGIN * yard:.3e}")
    print(f"  code comparisons left out {LEFT_OUT[0]} of {LEFT_OUT[1]} frames")


def _twice(e, st, x):
    """a cell's output, run twice: the same bits"""
    a = e.stages(st, st, x.to(torch.float32)).cpu()
    b = e.stages(st, st, x.to(torch.float32)).cpu()
    assert torch.equal(a, b)
    return a


def _check(ctx, st, x, cls):
    e, W64, W32, _ = ctx
    out = _twice(e, st, x)
    out_ref, ref = ER.stage(W64, st, x)
    assert out.shape == out_ref.shape
    assert torch.isfinite(out).all()
    err = ER.rel_err(ER.compared(W64, st, out, x), ref)
    yard = ER.YARDSTICK(W64, W32, st, x)
    _record(ER.KINDS[st], cls, err, yard)
    print(f"stage {st} {tuple(x.shape)} {cls}: {err:.3e} (yardstick {yard:.3e}, bound {ER.MARGIN * yard:.3e})")
    assert err <= ER.MARGIN * yard, (err, ER.MARGIN * yard)


def _conv_class(st, B, L):
    if (B, L) in ((1, 1), (3, 43)):
        return f"{B}x{L}"
    k, s = (7, 1) if st == 0 else (2 * ER.stage_ratio(st), ER.stage_ratio(st))
    g = ER.conv_geo(L, k, s)
    return "zero-ext" if g["ex0"] else "extra" if g["extra"] else "no-extra"


CONV_CELLS = ER.conv_cells()


@pytest.mark.parametrize("st,B,L", CONV_CELLS, ids=[f"s{s}-{b}x{l}" for s, b, l in CONV_CELLS])
def test_conv_stage_against_fp64(ctx, st, B, L):
    _check(ctx, st, ER.make_x(st, B, L), _conv_class(st, B, L))


def test_conv_cells_hit_the_padding_cases():
    """conv_geo's rule (lvx_api.cpp), restated: pt = k - stride, pr = pt / 2, pl = pt - pr, extra = ceil(L / stride)
    stride - L, right = pr + extra; an input with L <= max(pl, right) is zero-extended. Per strided stage the B = 2
    cells hold a zero-extended input, a longer one with extra right padding and one without extra right padding."""
    def geo(L, k, s):
        pt = k - s
        pr = pt // 2
        pl = pt - pr
        extra = -(-L // s) * s - L
        return L <= max(pl, pr + extra), extra
    for st in (2, 4, 6, 8):
        r = ER.stage_ratio(st)
        ls = [L for s, B, L in CONV_CELLS if s == st and B == 2]
        assert set(ls) >= {r - 1, r, r + 1, 2 * r + 1}
        cases = {(geo(L, 2 * r, r)[0], geo(L, 2 * r, r)[1] > 0) for L in ls}
        assert any(z for z, _ in cases) and (False, True) in cases and any(not x for _, x in cases)
        assert not geo(2 * r + 1, 2 * r, r)[0] and geo(2 * r + 1, 2 * r, r)[1] > 0 and geo(r, 2 * r, r)[1] == 0
        if r > 2:  # (at r = 2 only L = 1 is zero-extended: the (1, 1) cell and L = r - 1)
            assert any(geo(L, 2 * r, r)[0] and L > 1 for L in ls)
    assert geo(3, 7, 1)[0] and not geo(4, 7, 1)[0]
    for k, s in ((7, 1), (3, 1), (4, 2), (8, 4), (10, 5), (16, 8)):
        assert geo(1, k, s)[0]


@pytest.mark.parametrize("B,T", ER.LSTM_CELLS, ids=[f"{b}x{t}" for b, t in ER.LSTM_CELLS])
def test_slstm_against_fp64(ctx, B, T):
    _check(ctx, 9, ER.make_x(9, B, T), f"{B}x{T}")


def test_slstm_hot_cell(ctx):
    """layer-0 gates beyond +-90 (asserted from the fp64 model): expf(-gate) overflows to inf / underflows to 0 in
    fp32 and the sigmoids must come out 0 / 1, the output finite and within the cell's bound"""
    x = ER.hot_input()
    g = ER.lstm_gates0(ctx[1], x)
    assert float(g.max()) > ER.HOT_GATE and float(g.min()) < -ER.HOT_GATE
    assert tuple(x.shape[:2]) == ER.HOT_CELL
    _check(ctx, 9, x, "17x3 hot")


def test_slstm_successive_calls(ctx):
    """(33, 3) then (2, 5) on one context = (2, 5) on a context that has done nothing else, bit for bit (only the
    first B rows of one half of h, and of c, are cleared between calls)"""
    from llmvox_amd import weights as LW
    from llmvox_amd.encoder import WavEncoder
    e, _, _, cb = ctx
    big, small = ER.make_x(9, 33, 3).to(torch.float32), ER.make_x(9, 2, 5).to(torch.float32)
    e.stages(9, 9, big)
    got = e.stages(9, 9, small).cpu()
    fresh = WavEncoder(0, LW.synthetic_encoder(1234), cb, max_samples=1024)
    try:
        want = fresh.stages(9, 9, small).cpu()
    finally:
        fresh.close()
    assert torch.equal(got, want)


def _vq_check(e, Wq, cbk, x, cls, W32=None):
    codes, feats, scores = e.stages(11, 11, x.to(torch.float32), scores=True)
    codes2, feats2, _ = e.stages(11, 11, x.to(torch.float32))
    assert torch.equal(codes, codes2) and torch.equal(feats, feats2)
    q = ER.vq(Wq, x)
    codes = codes.cpu().numpy()
    assert np.array_equal(codes, q["codes"].numpy())
    np.testing.assert_array_equal(feats.cpu().numpy(), cbk[codes].transpose(0, 2, 1))
    if W32 is not None:
        err = ER.rel_err(scores.cpu(), q["scores"])
        yard = ER.YARDSTICK(Wq, W32, "vq", x)
        _record("vq", cls, err, yard)
        print(f"quantiser scores {cls}: {err:.3e} (yardstick {yard:.3e}, bound {ER.MARGIN * yard:.3e})")
        assert err <= ER.MARGIN * yard, (err, ER.MARGIN * yard)
    return q


@pytest.mark.parametrize("B,T", ER.VQ_CELLS, ids=[f"{b}x{t}" for b, t in ER.VQ_CELLS])
def test_quantiser_constructed_winners(ctx, B, T):
    """codebook row n + small noise: the fp64 runner-up is far behind in every frame (asserted), so the codes
    must be n, the features those rows bit for bit, the scores within the bound"""
    e, W64, W32, cb = ctx
    seen = set()
    for seed in range(4 if B * T == 1 else 1):
        x, n = ER.vq_input(cb, B, T, seed)
        q = _vq_check(e, W64, cb, x, f"{B}x{T}", W32)
        bound = ER.MARGIN * ER.YARDSTICK(W64, W32, "vq", x) * float(q["scores"].pow(2).mean().sqrt())
        assert float(q["gap"].min()) > 1e4 * bound and np.array_equal(q["codes"].numpy(), n)
        seen |= set(n.reshape(-1).tolist())
    if B * T == 1 or B * T >= len(ER.VQ_WINNERS):
        assert seen >= set(ER.VQ_WINNERS)


def test_quantiser_ties():
    """a codebook with copied rows (enc_ref.TIE_SETS: across neighbouring lanes, across waves, across the rounds of
    one thread, first vs last row, a triple, inside wave 3): frames equal to the copied rows get the lowest index
    of their set, the fp64 model ties exactly too"""
    from llmvox_amd import weights as LW
    from llmvox_amd.encoder import WavEncoder
    cb = LW.synthetic_codec(1234)[LW.CODEBOOK_KEY]
    tcb = ER.tie_codebook(cb)
    rows = [r for s in ER.TIE_SETS for r in s]
    x = torch.from_numpy(tcb[rows]).to(torch.float64)
    e = WavEncoder(0, LW.synthetic_encoder(1234), tcb, max_samples=1024)
    try:
        Wt = ER.Weights({}, tcb)
        for shape in ((1, len(rows), 512), (len(rows), 1, 512)):
            q = _vq_check(e, Wt, tcb, x.reshape(shape), "ties")
            assert q["codes"].reshape(-1).tolist() == [s[0] for s in ER.TIE_SETS for _ in s]
            assert float(q["gap"].max()) == 0.0
    finally:
        e.close()


def test_full_window_is_encode(ctx):
    """stages(0, 11) launches what lvx_encode launches: the same codes and features, bit for bit; the conv
    window (0, 8) in one call = nine calls of one stage"""
    e = ctx[0]
    audio = ER.make_x(0, 3, 700).to(torch.float32)
    feats, codes = e.encode(audio)
    emb = e.embedding(3, e.frames(700)).permute(0, 2, 1).cpu()
    codes2, feats2, _ = e.stages(0, 11, audio)
    assert torch.equal(codes[0].cpu(), codes2.long().cpu()) and torch.equal(feats.cpu(), feats2.cpu())
    assert torch.equal(e.stages(0, 10, audio).cpu(), emb)
    whole = e.stages(0, 8, audio).cpu()
    y = audio
    for st in range(9):
        y = e.stages(st, st, y)
    assert torch.equal(whole, y.cpu())


def test_argument_checks(ctx):
    from llmvox_amd import _lib
    e = ctx[0]
    x = torch.zeros(1, 4, 32)
    with pytest.raises(_lib.LvxArgError):
        e.stages(2, 1, x)                       # window order
    with pytest.raises(_lib.LvxArgError):
        e.stages(1, 12, x)                      # past the last stage
    with pytest.raises(_lib.LvxArgError):
        e.stages(-1, 1, x)
    with pytest.raises(_lib.LvxCapacityError):
        e.stages(0, 0, torch.zeros(1, MAX_SAMPLES + 1))
    with pytest.raises(_lib.LvxCapacityError):
        e.stages(10, 11, torch.zeros(400, 1, 512))   # 400 x 4,096 scores beyond the scratch
    with pytest.raises(_lib.LvxCapacityError):
        e.stages(1, 1, torch.zeros(1025, 1, 32))     # B beyond 1,024


def test_edge_golden_through_encode(ctx):
    """the reference's outputs at the edge shapes through WavEncoder.encode: the bars of tests/test_gpu_encoder.py
    (2e-4 x RMS, codes where the reference's gap exceeds 1e-2), and the fp64 chain within the chain's bound"""
    e, W64, W32, cb = ctx
    g = np.load(os.path.join(GOLDEN, "encoder_edge_golden.npz"))
    for tag in sorted(k[len("codes_"):] for k in g.files if k.startswith("codes_")):
        audio = torch.from_numpy(g[f"audio_{tag}"])
        B, N = audio.shape
        feats, codes = e.encode(audio.cuda())
        T = e.frames(N)
        emb = e.embedding(B, T).cpu()
        ref_codes = g[f"codes_{tag}"]
        got = codes.cpu().numpy()
        assert got.shape == ref_codes.shape == (1, B, T)
        robust = g[f"gap_{tag}"].reshape(B, T) > 1e-2
        LEFT_OUT[0] += int((~robust).sum())
        LEFT_OUT[1] += robust.size
        assert np.array_equal(got[0][robust], ref_codes[0][robust]), tag
        np.testing.assert_array_equal(feats.cpu().numpy(), cb[got[0]].transpose(0, 2, 1))
        if f"emb_{tag}" in g.files:
            ref = g[f"emb_{tag}"]
            np.testing.assert_allclose(emb.numpy(), ref, rtol=0, atol=2e-4 * float(np.sqrt(np.mean(ref ** 2))))
        else:
            np.testing.assert_allclose(emb.numpy().reshape(-1)[::7], g[f"emb_{tag}_every7"], rtol=0,
                                       atol=2e-4 * float(g[f"emb_{tag}_rms"]))
        a64 = audio.to(torch.float64)
        e64 = ER.chain(W64, a64)
        q = ER.vq(W64, e64)
        sure = q["gap"].numpy() > 1e-2
        assert np.array_equal(got[0][sure], q["codes"].numpy()[sure]), tag
        err = ER.rel_err(emb.permute(0, 2, 1), e64)
        yard = ER.YARDSTICK(W64, W32, "chain", a64)
        _record("chain", tag, err, yard)
        print(f"chain {tag}: {err:.3e} (yardstick {yard:.3e}, bound {ER.MARGIN * yard:.3e})")
        assert err <= ER.MARGIN * yard, (tag, err, ER.MARGIN * yard)
    # the share of frames the code comparisons of this module leave out, from the reference's gaps alone
    assert LEFT_OUT[1] == 174 and LEFT_OUT[0] <= 0.02 * LEFT_OUT[1]
