"""The volume control's rule on the host (llmvox_amd/audio.py: ``level_ref`` and its window and counts; include/llmvox.h,
"PCM level"): the window, chunked = one-shot, the ceiling, transparency, the shape of the gain around an isolated
click, the quality against hard clipping on a sustained harmonic tone, the streaming counts, ``AudioFormat.volume_pct``
and the composition with the other stages in ``StreamRef`` / ``convert_ref``."""
import numpy as np
import pytest

from llmvox_amd import audio as A

AA, R, C = A.LEVEL_A, A.LEVEL_R, A.LEVEL_CEIL


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def test_constants_and_window():
    assert (AA, R) == (120, 1200) and C.dtype == np.float32 and C == np.float32(0.8912509)
    assert abs(20 * np.log10(float(C)) + 1.0) < 1e-6  # -1 dBFS
    assert A.LEVEL_HISTORY >= 3 * AA + R
    w = A.level_window()
    assert w.dtype == np.float32 and w.shape == (241,)
    assert np.array_equal(w, w[::-1]) and np.all(w > 0) and w.argmax() == AA
    assert abs(w.astype(np.float64).sum() - 1.0) < 1e-6


def _chunked(x, pct, size):
    ys, gs, t0 = [], [], 0
    while t0 < x.size:
        n = min(size, x.size - t0)
        final = t0 + n == x.size
        n0 = A.level_emitted_upto(pct, t0, False)
        n1 = A.level_emitted_upto(pct, t0 + n, final)
        assert n1 - n0 == A.level_emitted(pct, t0, n, final)
        y, g = A.level_ref(x[:t0 + n], pct, None, n0, n1)  # (what a call can know: the inputs so far)
        ys.append(y)
        gs.append(g)
        t0 += n
    return np.concatenate(ys), np.concatenate(gs)


@pytest.mark.parametrize("size", [17, 983, 5000])
def test_chunked_equals_one_shot_bitwise(size):
    rng = np.random.default_rng(11)
    x = (rng.standard_normal(6000) * np.linspace(0.02, 0.5, 6000)).astype(np.float32)
    x[2500:2600] = 0.0
    for pct in (250, 37):
        y, g = A.level_ref(x, pct)
        assert 0.05 < float((g < 1).mean()) < 0.999 or pct == 37
        yc, gc = _chunked(x, pct, size)
        assert np.array_equal(_bits(yc), _bits(y)) and np.array_equal(_bits(gc), _bits(g))


def test_batched_rows_are_the_rows_alone():
    rng = np.random.default_rng(12)
    x = (rng.standard_normal((3, 2000)) * 0.3).astype(np.float32)
    y, g = A.level_ref(x, 300)
    for b in range(3):
        yb, gb = A.level_ref(x[b], 300)
        assert np.array_equal(_bits(y[b]), _bits(yb)) and np.array_equal(_bits(g[b]), _bits(gb))
    y2, g2 = A.level_ref(x, 300, A.level_window(), 700, 1300)
    assert np.array_equal(_bits(y2), _bits(y[:, 700:1300])) and np.array_equal(_bits(g2), _bits(g[:, 700:1300]))


def test_ceiling_over_random_signals():
    """max |y| <= c (1 + 2^-22) over 20 seeded Gaussian signals of 4,000 samples at random volumes in [0, 400]."""
    bound = float(C) * (1 + 2.0 ** -22)
    worst = 0.0
    for seed in range(20):
        rng = np.random.default_rng(1000 + seed)
        pct = int(rng.integers(0, 401))
        x = (rng.standard_normal(4000) * rng.uniform(0.05, 2.0)).astype(np.float32)
        y, g = A.level_ref(x, pct)
        assert y.dtype == g.dtype == np.float32 and y.size == g.size == 4000
        assert np.all(g >= 0) and np.all(g <= 1)
        peak = float(np.abs(y).max())
        worst = max(worst, peak / float(C))
        assert peak <= bound, (seed, pct, peak)
    print(f"largest peak / ceiling over the 20 signals: 1 + {worst - 1:.3e}")


def test_transparency():
    rng = np.random.default_rng(13)
    x = (rng.standard_normal(5000) * np.linspace(0.01, 0.4, 5000)).astype(np.float32)
    for pct in (0, 100, 180, 400):
        G = np.float32(pct / 100.0)
        y, g = A.level_ref(x, pct)
        clear = g == 1
        assert np.array_equal(_bits(y[clear]), _bits((G * x)[clear]))  # wherever g == 1: fl(G x) bit for bit
        v = np.abs(G * x)
        # ... and g == 1 wherever no |v| exceeds c in [n - 2 A - R, n + 2 A]
        over = np.concatenate([np.zeros(2 * AA + R), (v > C).astype(np.float64), np.zeros(2 * AA)])
        near = np.convolve(over, np.ones(4 * AA + R + 1), mode="valid") > 0.5
        assert near.size == x.size and np.all(g[~near] == 1)
        if pct in (180, 400):
            assert 0 < clear.sum() < x.size
    # a signal whose |G x| never exceeds c: g == 1 everywhere, y = fl(G x)
    quiet = (x / np.abs(x).max() * (float(C) / 4.0) * 0.999).astype(np.float32)
    assert float(np.abs(np.float32(4.0) * quiet).max()) <= float(C)
    y, g = A.level_ref(quiet, 400)
    assert np.all(g == 1) and np.array_equal(_bits(y), _bits(np.float32(4.0) * quiet))


def test_isolated_click():
    x = np.zeros(4000, dtype=np.float32)
    x[2000] = 1.0
    y, g = A.level_ref(x, 400)
    below = np.nonzero(g < 1)[0]
    assert below[0] == 2000 - 2 * AA and below[-1] == 2000 + R + AA and below.size == 3 * AA + R + 1  # exactly there
    assert np.all(np.diff(g[:2001]) <= 0)  # the gain does not rise before the click
    v = np.float32(4.0) * np.float32(1.0)
    r = C / np.abs(v)
    assert r.dtype == np.float32 and g[2000] == r and y[2000] == v * r
    # the hold: one value, r up to the rounding of the 241-term sum (each of its 2 A + 2 operations within 2^-24)
    hold = g[2001:2000 + R - AA + 1]
    assert np.all(hold == hold[0]) and abs(float(hold[0]) - float(r)) <= (2 * AA + 2) * 2.0 ** -24
    assert np.all(np.diff(g[2000 + R - AA:2000 + R + AA + 2]) >= 0)  # then the release, which does not fall
    assert np.count_nonzero(y) == 1


def test_special_values():
    x = (np.random.default_rng(14).standard_normal(3000) * 0.3).astype(np.float32)
    base_y, base_g = A.level_ref(x, 250)
    xn = x.copy()
    xn[1500] = np.nan
    y, g = A.level_ref(xn, 250)
    assert np.isnan(y[1500]) and int(np.isnan(y).sum()) == 1 and not np.isnan(g).any()
    x0 = x.copy()
    x0[1500] = 0.0  # a NaN has r = 1, like a sample that is not over the ceiling
    assert np.array_equal(_bits(g), _bits(A.level_ref(x0, 250)[1]))
    xi = x.copy()
    xi[1500] = np.inf
    y, g = A.level_ref(xi, 250)
    assert g[1500] == 0 and np.isnan(y[1500]) and int(np.isnan(y).sum()) == 1  # r = 0, and inf times 0
    # the hold: the minimum stays 0, the smoothed gain too, up to the rounding of the 241-term sum
    assert np.all(g[1500 + AA:1500 + R - AA] <= (2 * AA + 2) * 2.0 ** -24)
    finite = np.delete(y, 1500)
    assert np.all(np.abs(finite) <= float(C) * (1 + 2.0 ** -22))
    # volume 0: silence, whatever the input (g = 1: nothing is over the ceiling)
    y, g = A.level_ref(x, 0)
    assert np.all(y == 0) and np.all(g == 1)
    assert base_y.size == x.size and base_g.size == x.size


def test_quality_against_hard_clipping():
    """A sustained tone (eleven 1 / h harmonics of 110 Hz, peak 0.45) at volume 400: after a least-squares scalar fit
    to G x over samples 2400 .. 4800 the limiter leaves an rms residual below 1 / 100 of the hard clipper's on the
    same input: it turns the level down, it does not reshape the wave."""
    n = np.arange(7200, dtype=np.float64)
    s = sum(np.sin(2 * np.pi * 110.0 * h * n / 24000.0) / h for h in range(1, 12))
    x = (s / np.abs(s).max() * 0.45).astype(np.float32)
    y, g = A.level_ref(x, 400)
    v = (np.float32(4.0) * x).astype(np.float64)[2400:4800]

    def residual(o):
        o = o.astype(np.float64)[2400:4800]
        k = (o @ v) / (v @ v)
        return float(np.sqrt(np.mean((o - k * v) ** 2)))

    lim = residual(y)
    clip = residual(np.clip(np.float32(4.0) * x, -C, C))
    ripple = float(g[2400:4800].max() - g[2400:4800].min())
    print(f"rms residual after the scalar fit: limiter {lim:.3e}, hard clipper {clip:.3e}; gain ripple {ripple:.3e}")
    assert lim < clip / 100.0
    assert float(np.abs(y).max()) <= float(C) * (1 + 2.0 ** -22)


def test_counts():
    H = 2 * AA
    for pct in (0, 50, 250, 400):
        for T in (0, 1, H - 1, H, H + 1, 1000, 5800):
            assert A.level_emitted_upto(pct, T, False) == max(0, T - H) and A.level_emitted_upto(pct, T, True) == T
        assert A.level_emitted(pct, 0, 100, False) == 0 and A.level_emitted(pct, 0, 100, True) == 100
        assert A.level_emitted(pct, 100, 200, False) == 60 and A.level_emitted(pct, 300, 320, False) == 320
        assert A.level_emitted(pct, 300, 0, True) == H and A.level_emitted(pct, 100, 0, True) == 100  # flush only
        assert A.level_emitted(pct, 0, 0, True) == 0 and A.level_emitted(pct, 300, 0, False) == 0
        total = sum(A.level_emitted(pct, t0, n, f) for t0, n, f in ((0, 3200, False), (3200, 1, False), (3201, 99, True)))
        assert total == 3300
    assert A.level_emitted(100, 17, 123, False) == 123 and A.level_emitted_upto(100, 55, False) == 55
    for bad in ((-1, 0, 1, False), (401, 0, 1, False), (True, 0, 1, False), (2.5, 0, 1, False), (250, -1, 1, False),
                (250, 0, -1, False)):
        with pytest.raises(ValueError):
            A.level_emitted(*bad)
    with pytest.raises(ValueError):
        A.level_ref(np.zeros(10, np.float32), 401)
    with pytest.raises(ValueError):
        A.level_ref(np.zeros(10, np.float32), 250, np.ones(240, np.float32))


def test_audio_format_volume():
    f = A.AudioFormat()
    assert f.volume_pct == 100 and f.is_default and not f.converts
    assert A.AudioFormat(24000, "f32le", "raw", 100, 100, False, 100) == f  # the last field, positionally
    for pct in (0, 99, 101, 400):
        g = A.AudioFormat(volume_pct=pct)
        assert not g.is_default and g.converts and g != f and g.sample_bytes == 4 and g.stretch_pct == 100
    assert A.AudioFormat(16000, "s16le", volume_pct=100).converts
    for bad in (-1, 401, True, False, 1.5, "100", None, np.float32(2)):
        with pytest.raises(ValueError):
            A.AudioFormat(volume_pct=bad)
    assert A.wav_header(A.AudioFormat(16000, "s16le", "wav", volume_pct=250)) == A.wav_header(A.AudioFormat(16000, "s16le", "wav"))
    for name in ("level_window", "level_emitted", "level_emitted_upto", "level_ref", "LEVEL_A", "LEVEL_R", "LEVEL_CEIL"):
        assert name in A.__all__


def _signal(T, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(T, dtype=np.float64)
    tone = 0.25 * sum(np.sin(2 * np.pi * h * t / 131.0) / h for h in range(1, 6))
    return (tone + rng.uniform(-1, 1, T) * np.linspace(0.0, 0.2, T)).astype(np.float32)


def test_convert_ref_places_the_stage_between_the_ratio_and_the_rate():
    x = _signal(4000, 15)
    fmt = A.AudioFormat(16000, "s16le", "raw", 130, 90, False, 300)
    mid = A.ratio_ref(A.stretch_ref(x, fmt.stretch_pct)[0], *fmt.ratio)
    lev, g = A.level_ref(mid, 300)
    assert float(g.min()) < 0.9  # (the stage has work to do on this signal)
    want = A.quantize_s16(A.resample_ref(lev, 16000))
    assert np.array_equal(A.convert_ref(x, fmt), want)
    assert not np.array_equal(A.convert_ref(x, fmt), A.convert_ref(x, A.AudioFormat(16000, "s16le", "raw", 130, 90)))
    # the stage alone, and volume 100 as before there was one
    assert np.array_equal(_bits(A.convert_ref(x, A.AudioFormat(volume_pct=300))), _bits(A.level_ref(x, 300)[0]))
    assert np.array_equal(_bits(A.convert_ref(x, A.AudioFormat(volume_pct=100))), _bits(x))


@pytest.mark.parametrize("fmt", [A.AudioFormat(16000, "s16le", "raw", 130, 90, True, 300), A.AudioFormat(volume_pct=250),
                                 A.AudioFormat(48000, "f32le", "raw", 80, 100, False, 0)],
                         ids=lambda f: f"{f.sample_rate}-{f.speed_pct}-{f.pitch_pct}-{int(f.join)}-{f.volume_pct}")
def test_stream_ref_composition(fmt):
    """StreamRef over three dumps (context frames where the format joins) is the stages applied one after the other
    to the whole sentence; identical dump renderings make the join a plain concatenation up to its crossfade."""
    x = _signal(5760, 16)
    dumps = [(0, 3200, 0), (3200 - 640, 5120, 2), (5120 - 320, 5760, 1)] if fmt.join else [(0, 3200, 0), (3200, 5120, 0), (5120, 5760, 0)]
    ref = A.StreamRef(fmt)
    parts = [ref.push(x[a:e], k == len(dumps) - 1, c) for k, (a, e, c) in enumerate(dumps)]
    got = np.concatenate(parts)
    assert got.dtype == fmt.dtype
    if fmt.join:
        joined = np.concatenate(A.join_ref([x[a:e] for a, e, _ in dumps], [c for _, _, c in dumps]))
    else:
        joined = x
    want = A.convert_ref(joined, fmt)
    assert got.size == want.size and np.array_equal(got.view(np.uint8), want.view(np.uint8))
    # the counts of the non-final pushes: what every stage could emit so far
    L, M = fmt.ratio
    n = 320 * 9 if fmt.join else 3200
    n = A.stretch_emitted_upto(fmt.stretch_pct, n, False)
    n = A.ratio_emitted_upto(L, M, n, False)
    n = A.level_emitted_upto(fmt.volume_pct, n, False)
    assert parts[0].size == A.emitted_upto(fmt.sample_rate, n, False)
    # a second sentence on the same object starts afresh
    again = np.concatenate([ref.push(x[a:e], k == len(dumps) - 1, c) for k, (a, e, c) in enumerate(dumps)])
    assert np.array_equal(again.view(np.uint8), got.view(np.uint8))
