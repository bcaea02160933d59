"""tests/enc_ref.py without a GPU: the fp64 model of the encoder against the CPU oracle (torch's own conv1d and
nn.LSTM) and the reference's golden outputs, and the sensitivity of the comparison that
tests/test_gpu_encoder_stages.py makes: every indexing / omission error of MUT_CONV / MUT_LSTM, applied to
the fp32 model on that file's cells, moves the compared quantity by >= 10 x the cell's bound.
"""
import os

import numpy as np
import pytest
import torch

from tests import enc_ref as ER

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
FILES = ("encoder_golden.npz", "encoder_edge_golden.npz")


@pytest.fixture(scope="module")
def W():
    return ER.load_weights()


def _golden():
    for f in FILES:
        g = np.load(os.path.join(GOLDEN, f))
        for tag in sorted(k[len("codes_"):] for k in g.files if k.startswith("codes_")):
            yield g, tag


def test_fp32_chain_equals_oracle(W):
    """the stage functions chained in fp32, and the oracle, within the chain's bound of the fp64 chain and of
    each other; the oracle's codes wherever the fp64 gap exceeds 1e-2"""
    from llmvox_amd import weights as LW
    from oracle import reference_cpu as R
    W64, W32, cb = W
    We = R.to_torch(LW.encoder_effective(LW.synthetic_encoder(1234)))
    edge = np.load(os.path.join(GOLDEN, FILES[1]))
    audios = [torch.from_numpy(edge[f"audio_{t}"]) for t in ("1x1", "2x2", "1x7", "2x319", "1x321", "17x640")]
    audios.append(0.3 * torch.randn(3, 5000, generator=torch.Generator().manual_seed(3)))
    for a in audios:
        e64 = ER.chain(W64, a.to(torch.float64))
        bound = ER.MARGIN * ER.YARDSTICK(W64, W32, "chain", a.to(torch.float64))
        orc = R.seanet_encode(We, a)
        for got in (orc.permute(0, 2, 1), ER.chain(W32, a)):
            assert ER.rel_err(got, e64) <= bound
        assert ER.rel_err(ER.chain(W32, a), orc.permute(0, 2, 1)) <= bound
        codes, _ = R.vq_encode(torch.from_numpy(cb), orc)
        q = ER.vq(W64, e64)
        robust = q["gap"] > 1e-2
        assert torch.equal(codes[robust], q["codes"][robust])


def test_chain_reproduces_golden(W):
    """the reference's own embeddings within the chain's bound, its codes wherever its gap exceeds 1e-2"""
    W64, W32, _ = W
    left_out = frames = 0
    for g, tag in _golden():
        a = torch.from_numpy(g[f"audio_{tag}"]).to(torch.float64)
        e64 = ER.chain(W64, a)
        bound = ER.MARGIN * ER.YARDSTICK(W64, W32, "chain", a)
        ref = e64.permute(0, 2, 1)  # the reference's [B, 512, T]
        if f"emb_{tag}" in g.files:
            err = ER.rel_err(torch.from_numpy(g[f"emb_{tag}"]), ref)
        else:
            err = ER.rel_err(torch.from_numpy(g[f"emb_{tag}_every7"]), ref.reshape(-1)[::7])
        assert err <= bound, (tag, err, bound)
        q = ER.vq(W64, e64)
        robust = g[f"gap_{tag}"].reshape(q["codes"].shape) > 1e-2
        assert np.array_equal(q["codes"].numpy()[robust], g[f"codes_{tag}"][0][robust]), tag
        left_out += int((~robust).sum())
        frames += robust.size
    assert left_out <= 0.02 * frames, (left_out, frames)


def test_lstm_input_scale(W):
    """LSTM_IN_RMS is the real chain's: stage 8's output on a golden case"""
    g = np.load(os.path.join(GOLDEN, FILES[0]))
    x = torch.from_numpy(g["audio_3x4800"]).to(torch.float64)
    for st in range(9):
        x = ER.stage(W[0], st, x)[0]
    assert abs(float(x.pow(2).mean().sqrt()) - ER.LSTM_IN_RMS) < 0.05


def test_geometry_cases_are_hit():
    """conv_cells() holds, for every strided conv, an input no longer than the pad (zero-extended), one longer
    than it with extra right padding and one without extra right padding, and the zero extension at L > 1
    wherever the geometry has one; stage 0 sits on either side of the k7 pad."""
    cells = ER.conv_cells()
    for st in (2, 4, 6, 8):
        r = ER.stage_ratio(st)
        geo = [ER.conv_geo(L, 2 * r, r) | {"L": L} for s, B, L in cells if s == st and B == 2]
        assert {g["L"] for g in geo} >= {r - 1, r, r + 1, 2 * r + 1}
        assert any(g["ex0"] > 0 for g in geo)
        assert any(g["ex0"] == 0 and g["extra"] > 0 for g in geo)
        assert any(g["extra"] == 0 for g in geo)
        possible = any(ER.conv_geo(L, 2 * r, r)["ex0"] for L in range(2, 4 * r))
        assert any(g["ex0"] > 0 and g["L"] > 1 for g in geo) == possible == (r > 2)
    assert ER.conv_geo(3, 7, 1)["ex0"] == 1 and ER.conv_geo(4, 7, 1)["ex0"] == 0
    assert (0, 2, 3) in cells and (0, 2, 4) in cells
    for st in ER.CONV_STAGES:  # at L = 1 every conv with k > 1 is zero-extended
        assert (st, 1, 1) in cells and (st, 3, 43) in cells
    assert all(ER.conv_geo(1, k, s)["ex0"] > 0 for k, s in ((7, 1), (3, 1), (4, 2), (8, 4), (10, 5), (16, 8)))


def test_tap_index_is_the_oracles_padding():
    """tap_index against oracle.reference_cpu._enc_pad on a ramp, every (L, k, stride) of the encoder at small L"""
    from oracle import reference_cpu as R
    for k, s in ((7, 1), (3, 1), (1, 1), (4, 2), (8, 4), (10, 5), (16, 8)):
        for L in range(1, 40):
            x = torch.arange(1.0, L + 1.0).view(1, 1, L)
            pad = R._enc_pad(x, k, s)[0, 0]
            idx = ER.tap_index(L, k, s)
            xz = torch.cat([x[0, 0], torch.zeros(1)])
            want = torch.stack([pad[t * s:t * s + k] for t in range(idx.shape[0])])
            assert torch.equal(xz[idx], want), (k, s, L)
            assert idx.shape[0] == -(-L // s)


# ---- mutations ---------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def cells(W):
    """(stage, B, L) -> (input, fp64 compared quantity, bound), computed once"""
    W64, W32, _ = W
    cache = {}

    def get(st, B, L):
        if (st, B, L) not in cache:
            x = ER.make_x(st, B, L)
            cache[st, B, L] = (x, ER.stage(W64, st, x)[1], ER.MARGIN * ER.YARDSTICK(W64, W32, st, x))
        return cache[st, B, L]

    return get


def _stage_convs(st):
    """(k, stride) of the convs of a conv stage"""
    kind = ER.KINDS[st]
    return ((7, 1),) if kind in ("conv0", "conv15") else ((3, 1), (1, 1)) if kind == "resblock" else \
        ((2 * ER.stage_ratio(st), ER.stage_ratio(st)),)


def _applies(m, st, B, L):
    """a mutation is another program on a cell where it changes which frame some tap reads, or where the cell has
    what it drops"""
    if m in ("reflect_left", "reflect_right", "no_extra_right", "no_zero_ext"):
        return any(not torch.equal(ER.tap_index(L, k, s), ER.tap_index(L, k, s, {m})) for k, s in _stage_convs(st))
    if m == "no_elu":
        return st != 0
    if m == "no_residual":
        return ER.KINDS[st] == "resblock"
    return True  # drop_tap (every stage has a conv with k > 1), drop_k16


@pytest.mark.parametrize("m", ER.MUT_CONV)
def test_conv_mutation_moves_every_cell(W, cells, m):
    W64, W32, _ = W
    hit = set()
    for st, B, L in ER.conv_cells():
        if not _applies(m, st, B, L):
            continue
        x, ref, bound = cells(st, B, L)
        out, _ = ER.stage(W32, st, x.to(torch.float32), {m})
        moved = ER.rel_err(ER.compared(W64, st, out, x), ref)
        assert moved >= 10 * bound, (m, st, B, L, moved, bound)
        hit.add(ER.KINDS[st])
    # every mutation meets every stage kind it can occur in (extra right padding: only a stride > 1 has any)
    want = {"resblock"} if m == "no_residual" else {"down"} if m == "no_extra_right" else \
        {"resblock", "down", "conv15"} | ({"conv0"} if m != "no_elu" else set())
    assert hit == want, (m, hit)


def test_zero_extension_and_extra_padding_cells(cells):
    """the cells the padding mutations apply to are the ones the geometry says: zero-extended / extra > 0"""
    for st, B, L in ER.conv_cells():
        geo = [ER.conv_geo(L, k, s) for k, s in _stage_convs(st)]
        assert _applies("no_zero_ext", st, B, L) == any(g["ex0"] > 0 for g in geo)
        # (inside a zero extension the extra frames may all read zeros: dropping them changes nothing there)
        extra = any(g["extra"] > 0 for g in geo)
        assert _applies("no_extra_right", st, B, L) <= extra
        if not any(g["ex0"] > 0 for g in geo):
            assert _applies("no_extra_right", st, B, L) == extra
        assert _applies("reflect_left", st, B, L)


@pytest.mark.parametrize("m", ER.MUT_LSTM)
def test_lstm_mutation_moves_every_cell(W, cells, m):
    W64, W32, _ = W
    n = 0
    for B, T in ER.LSTM_CELLS:
        if m in ("no_c_carry", "h_prev2") and T < 2:  # no earlier step
            continue
        if m == "h_next_stream" and (B < 2 or T < 2):
            continue
        if m == "h_stream_m16" and (B < 17 or T < 2):
            continue
        x, ref, bound = cells(9, B, T)
        out, _ = ER.stage(W32, 9, x.to(torch.float32), {m})
        moved = ER.rel_err(ER.compared(W64, 9, out, x), ref)
        assert moved >= 10 * bound, (m, B, T, moved, bound)
        n += 1
    assert n >= (2 if m == "h_stream_m16" else 4)


def test_hot_cell_leaves_the_exp_range(W):
    g = ER.lstm_gates0(W[0], ER.hot_input())
    assert float(g.max()) > ER.HOT_GATE and float(g.min()) < -ER.HOT_GATE
    # the fp32 evaluation stays finite and within the cell's own bound of the fp64 one by construction;
    # the ordinary cells stay below the overflow
    for B, T in ER.LSTM_CELLS:
        assert float(ER.lstm_gates0(W[0], ER.make_x(9, B, T)).abs().max()) < 88.0


def test_quantiser_cells(W):
    """constructed winners: the fp64 model picks the planted row in every frame, far ahead; the tie codebook's
    copies tie exactly in the model and the first index wins"""
    W64, W32, cb = W
    seen = set()
    for B, T in ER.VQ_CELLS:
        for seed in range(4 if B * T == 1 else 1):
            x, n = ER.vq_input(cb, B, T, seed)
            q = ER.vq(W64, x)
            assert np.array_equal(q["codes"].numpy(), n)
            bound = ER.MARGIN * ER.YARDSTICK(W64, W32, "vq", x) * float(q["scores"].pow(2).mean().sqrt())
            assert float(q["gap"].min()) > 1e4 * bound  # no frame is left out
            seen |= set(n.reshape(-1).tolist())
    assert seen >= set(ER.VQ_WINNERS)
    tcb = ER.tie_codebook(cb)
    Wt = ER.Weights({}, tcb)
    rows = [r for s in ER.TIE_SETS for r in s]
    q = ER.vq(Wt, torch.from_numpy(tcb[rows]).to(torch.float64).reshape(1, len(rows), 512))
    assert q["codes"].reshape(-1).tolist() == [s[0] for s in ER.TIE_SETS for _ in s]
    assert float(q["gap"].max()) == 0.0
