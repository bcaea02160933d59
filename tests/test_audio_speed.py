"""The speaking-rate rule (include/llmvox.h, "PCM time stretch") as llmvox_amd/audio.py states it in numpy
(CPU): the counts and their independence of chunking, causality of the emitted hops, that the search makes
it WSOLA and not plain overlap-add, silence, NaN, and the ``speed_pct`` field of ``AudioFormat``."""
import numpy as np
import pytest

from llmvox_amd import audio as A

SPEEDS = [50, 77, 130, 200]
H = A.STRETCH_H


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def harmonic(P, n=12000):
    """Seven harmonics of period P samples, amplitudes 1 / h, scaled by 0.2."""
    t = np.arange(n, dtype=np.float64)
    return (0.2 * sum(np.sin(2 * np.pi * h * t / P) / h for h in range(1, 8))).astype(np.float32)


def _signal(T, seed=0):
    rng = np.random.default_rng(seed)
    return (harmonic(96, T) + rng.uniform(-0.1, 0.1, T)).astype(np.float32)


def _fmt(pct, rate=24000, enc="f32le"):
    return A.AudioFormat(rate, enc, "raw", pct)


@pytest.mark.parametrize("pct", [50, 77, 100, 130, 200])
def test_counts_and_chunking(pct):
    rng = np.random.default_rng(pct)
    for T in [0, 1, 239, 240, 479, 480, 481, 719, 720, 961, 1200, 2500, 4801]:
        x = _signal(T, T)
        one = A.StreamRef(_fmt(pct)).push(x, True)
        assert one.size == -(-T * 100 // pct)  # ceil(T 100 / pct)
        assert np.array_equal(_bits(one), _bits(A.convert_ref(x, _fmt(pct))))
        if pct != 100:
            assert np.array_equal(_bits(one), _bits(A.stretch_ref(x, pct)[0]))
        for trial in range(3):
            cuts = sorted(rng.integers(0, T + 1, size=rng.integers(1, 6)).tolist()) if T else [0]
            edges = [0] + cuts + [T]
            ref, parts, ds = A.StreamRef(_fmt(pct)), [], []
            for k in range(len(edges) - 1):
                final = k == len(edges) - 2
                o = ref.push(x[edges[k]:edges[k + 1]], final)
                assert o.size == A.stretch_emitted(pct, edges[k], edges[k + 1] - edges[k], final), (T, edges, k)
                if not final and pct != 100:
                    assert o.size % H == 0  # whole hops before the end
                parts.append(o)
                ds.append(ref.last_d)
            assert np.array_equal(_bits(np.concatenate(parts)), _bits(one)), (T, edges)
            if pct != 100:
                assert np.array_equal(np.concatenate(ds), A.stretch_ref(x, pct)[1])
        # a flush-only final call emits the rest
        ref = A.StreamRef(_fmt(pct))
        first = ref.push(x, False)
        rest = ref.push(np.zeros(0, np.float32), True)
        assert first.size == A.stretch_emitted_upto(pct, T, False) and first.size + rest.size == one.size
        assert np.array_equal(_bits(np.concatenate([first, rest])), _bits(one))


@pytest.mark.parametrize("pct", SPEEDS)
def test_emitted_hops_do_not_read_past_what_was_consumed(pct):
    x = _signal(9000, 3)
    y, d = A.stretch_ref(x, pct)
    for T in (320, 960, 3200, 4000):
        other = x.copy()
        other[T:] = np.random.default_rng(T).uniform(-1, 1, x.size - T).astype(np.float32)
        y2, d2 = A.stretch_ref(other, pct)
        n = A.stretch_emitted_upto(pct, T, False)
        assert n % H == 0 and n <= y.size
        assert np.array_equal(_bits(y[:n]), _bits(y2[:n])) and np.array_equal(d[:n // H], d2[:n // H])
        # and the streaming form, which never saw the rest, emits exactly those
        got = A.StreamRef(_fmt(pct)).push(x[:T], False)
        assert np.array_equal(_bits(got), _bits(y[:n]))


def _autocorr(y, lag):
    a, b = y[:-lag].astype(np.float64), y[lag:].astype(np.float64)
    return float((a * b).sum() / np.sqrt((a * a).sum() * (b * b).sum()))


def _rms(y):
    return float(np.sqrt((y.astype(np.float64) ** 2).mean()))


@pytest.mark.parametrize("P", [96, 150])
@pytest.mark.parametrize("pct", SPEEDS)
def test_it_is_wsola_not_plain_overlap_add(pct, P):
    x = harmonic(P)
    y, d = A.stretch_ref(x, pct)
    plain, d0 = A.stretch_ref(x, pct, force_d0=True)
    assert y.size == plain.size == -(-x.size * 100 // pct) and not d0.any() and d.any()
    inner, inner0 = y[2000:-2000], plain[2000:-2000]
    r, r0, gain = _autocorr(inner, P), _autocorr(inner0, P), _rms(inner) / _rms(x)
    print(f"P {P} speed {pct}: autocorrelation at lag P {r:.5f} (d forced to 0: {r0:.3f}), RMS ratio {gain:.4f}")
    assert r >= 0.99       # the period survives the stretch
    assert r0 < 0.9        # which plain overlap-add at the nominal positions does not achieve
    assert abs(gain - 1.0) <= 0.02


@pytest.mark.parametrize("pct", SPEEDS)
def test_silence_chooses_no_offset(pct):
    y, d = A.stretch_ref(np.zeros(5000, np.float32), pct)
    assert d.size == -(-y.size // H) and not d.any() and not y.any()


@pytest.mark.parametrize("pct", SPEEDS)
def test_a_nan_sample_leaves_the_offsets_defined(pct):
    x = _signal(4800, 9)
    x[2000] = np.nan
    y, d = A.stretch_ref(x, pct)
    assert d.dtype == np.int32 and d.size == -(-y.size // H) and np.abs(d).max() <= A.STRETCH_D and d[0] == 0
    y2, d2 = A.stretch_ref(x, pct)
    assert np.array_equal(d, d2) and np.array_equal(y, y2, equal_nan=True)
    # chunked: the same offsets and samples
    ref, parts, ds = A.StreamRef(_fmt(pct)), [], []
    for lo, hi in [(0, 1900), (1900, 2001), (2001, 4800)]:
        parts.append(ref.push(x[lo:hi], hi == 4800))
        ds.append(ref.last_d)
    assert np.array_equal(np.concatenate(ds), d) and np.array_equal(np.concatenate(parts), y, equal_nan=True)
    assert np.isnan(y).sum() < 3 * H  # the NaN stays where the sample goes; it does not spread over the segment


def test_equal_scores_take_the_smallest_offset_and_of_a_pair_the_negative_one():
    """A signal of period 80 (exactly, in fp32: a repeated table) scores the same at every multiple of the
    period: the rule takes the one nearest the nominal position, and of +-d the negative one."""
    table = np.random.default_rng(1).uniform(-0.5, 0.5, 80).astype(np.float32)
    x = np.tile(table, 60)
    y, d = A.stretch_ref(x, 150)  # a_j = 360 j: e_j - a_j is a multiple of 40
    inner = d[2:-4]
    assert inner.size > 5 and np.all(np.abs(inner) <= 40)
    assert np.all((inner == 0) | (inner == -40))  # (+40 scores the same as -40: the negative one is taken)
    assert (inner == -40).any()
    assert _autocorr(y[400:2400], 80) > 0.999999


def test_windows_are_complementary():
    wr, wf = A.stretch_window()
    assert wr.dtype == wf.dtype == np.float32 and wr.size == wf.size == H
    assert np.all(np.diff(wr) > 0) and 0 < wr[0] < 1e-4 and np.abs(wr + wf - 1).max() <= 2.0 ** -24
    assert np.array_equal(wr, wf[::-1])


def test_composition_is_stretch_then_resample_then_encode():
    x = _signal(3000, 4)
    fmt = _fmt(130, 16000, "s16le")
    want = A.encode_ref(A.resample_ref(A.stretch_ref(x, 130)[0], 16000), fmt)
    assert np.array_equal(A.convert_ref(x, fmt), want) and want.dtype == np.int16
    ref, parts = A.StreamRef(fmt), []
    for lo, hi in [(0, 700), (700, 1800), (1800, 3000)]:
        parts.append(ref.push(x[lo:hi], hi == 3000))
    assert np.array_equal(np.concatenate(parts), want)
    assert want.size == -(-(-(-3000 * 100 // 130)) * 2 // 3)


def test_audio_format_speed_field():
    assert A.AudioFormat().speed_pct == 100 and A.AudioFormat(16000, "s16le", "wav").speed_pct == 100
    assert A.AudioFormat(16000, "s16le", "wav") == A.AudioFormat(16000, "s16le", "wav", 100)
    f = A.AudioFormat(speed_pct=130)
    assert f.converts and not f.is_default and f.sample_rate == 24000 and f.dtype == np.dtype("<f4")
    assert A.AudioFormat(speed_pct=100).is_default and not A.AudioFormat(speed_pct=100).converts
    assert A.AudioFormat(24000, "f32le", "raw", 50).speed_pct == 50 and A.AudioFormat(speed_pct=200).speed_pct == 200
    for bad in (49, 201, 0, -100, 1.3, "130", True, None):
        with pytest.raises(ValueError):
            A.AudioFormat(speed_pct=bad)
    assert A.stretch_emitted(100, 7, 320, False) == 320 and A.stretch_emitted_upto(100, 5, True) == 5
