"""The pitch control's rule on the host (no GPU; include/llmvox.h, "PCM pitch shift"): the library's plan, ratio
filter design and streaming counts (lvx_pcm_pitch_plan / lvx_pcm_ratio_filter / lvx_pcm_ratio_emitted, host-only
entry points) against the numpy statement in llmvox_amd/audio.py, the filters' responses against the header's
figures, the fixed rates as three ratios of the same design, chunked = one-shot, the composition of the three
stages, and the ``pitch_pct`` field of ``AudioFormat``."""
import ctypes
from math import gcd

import numpy as np
import pytest

from llmvox_amd import _lib
from llmvox_amd import audio as A

PAIRS = [(4, 5), (5, 4), (99, 100), (197, 199), (51, 101), (127, 185), (195, 199), (1, 2)]
FIXED = {16000: (2, 3, 72), 8000: (1, 3, 72), 48000: (2, 1, 48)}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _lib_plan(speed, pitch):
    st, L, M = ctypes.c_int(-1), ctypes.c_int(-1), ctypes.c_int(-1)
    rc = _lib.load().lvx_pcm_pitch_plan(speed, pitch, ctypes.byref(st), ctypes.byref(L), ctypes.byref(M))
    return rc, (st.value, L.value, M.value)


def _lib_ratio_filter(L, M):
    lib = _lib.load()
    N = ctypes.c_int()
    _lib.check(lib.lvx_pcm_ratio_filter(L, M, ctypes.byref(N), None, 0))
    taps = np.zeros(2 * N.value + 1, dtype=np.float32)
    _lib.check(lib.lvx_pcm_ratio_filter(L, M, None, taps.ctypes.data_as(ctypes.c_void_p), taps.size))
    return N.value, taps


def _signal(T, seed=0):
    rng = np.random.default_rng(seed)
    t = np.arange(T, dtype=np.float64)
    tone = 0.2 * sum(np.sin(2 * np.pi * h * t / 96) / h for h in range(1, 8))
    return (tone + rng.uniform(-0.1, 0.1, T)).astype(np.float32)


# ---- the plan -----------------------------------------------------------------------------------------

def test_library_plan_is_the_numpy_plan_everywhere():
    valid = invalid = 0
    for speed in range(50, 201):
        for pitch in range(50, 201):
            stretch = (200 * speed + pitch) // (2 * pitch)  # the rule, restated: speed 100 / pitch, half up
            assert stretch == int(np.floor(speed * 100 / pitch + 0.5))
            rc, got = _lib_plan(speed, pitch)
            if 50 <= stretch <= 200:
                g = gcd(stretch, speed)
                assert rc == _lib.LVX_OK and got == (stretch, stretch // g, speed // g) == A.pitch_plan(speed, pitch)
                assert gcd(got[1], got[2]) == 1 and got[2] <= 4 * got[1] and got[1] <= 4 * got[2]
                valid += 1
            else:
                assert rc == _lib.LVX_E_ARG and got == (-1, -1, -1)
                with pytest.raises(ValueError):
                    A.pitch_plan(speed, pitch)
                with pytest.raises(ValueError):
                    A.AudioFormat(speed_pct=speed, pitch_pct=pitch)
                invalid += 1
    assert valid > 15000 and invalid > 1000
    for speed in range(50, 201):  # no pitch: the speed's own stretch and no resampling
        assert A.pitch_plan(speed, 100) == (speed, 1, 1) == _lib_plan(speed, 100)[1]


def test_plan_arguments():
    lib = _lib.load()
    for speed, pitch in [(49, 100), (201, 100), (100, 49), (100, 201), (0, 100), (100, 0), (-100, 100), (100, -100)]:
        assert _lib_plan(speed, pitch)[0] == _lib.LVX_E_ARG
        with pytest.raises(ValueError):
            A.pitch_plan(speed, pitch)
    assert lib.lvx_pcm_pitch_plan(120, 90, None, None, None) == _lib.LVX_OK  # (every output is optional)
    assert lib.lvx_pcm_pitch_plan(200, 50, None, None, None) == _lib.LVX_E_ARG  # a stretch of 400 percent
    assert b"400" in lib.lvx_last_error()
    for bad in (1.2, "120", True, None):
        with pytest.raises(ValueError):
            A.pitch_plan(100, bad)
    assert A.pitch_plan(120, 90) == (133, 133, 120) and A.pitch_plan(100, 125) == (80, 4, 5)
    assert A.pitch_plan(100, 200) == (50, 1, 2) and A.pitch_plan(100, 50) == (200, 2, 1)


# ---- the filter ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("L,M", PAIRS)
def test_library_ratio_filter_is_the_numpy_design(L, M):
    N, taps = _lib_ratio_filter(L, M)
    n, h = A.ratio_design(L, M)
    assert N == n == 24 * max(L, M) == int(round(24 * L / min(1.0, L / M))) and N <= 4800
    assert h.dtype == np.float64 and h.size == 2 * N + 1 == taps.size
    assert np.abs(taps - h).max() <= 1e-6 * np.abs(h).max()
    idx = np.arange(-N, N + 1)
    per_phase = [idx[(idx - p) % L == 0].size for p in range(L)]
    assert max(per_phase) == 2 * N // L + 1  # taps per output
    assert 2 * N // L <= 96  # a plan pair's reach-back
    dc = [taps.astype(np.float64)[(idx - p) % L == 0].sum() for p in range(L)]
    assert np.abs(np.array(dc) - 1.0).max() <= 5e-5, np.abs(np.array(dc) - 1.0).max()


@pytest.mark.parametrize("L,M", PAIRS)
def test_library_ratio_filter_response(L, M):
    """The float64 response of the library's fp32 taps: within 0.1 dB up to 0.765 of the lower Nyquist frequency
    (within 0.022 dB up to 0.75 of it), at most -91 dB from that Nyquist frequency on."""
    N, taps = _lib_ratio_filter(L, M)
    nfft = 1 << 20
    H = np.abs(np.fft.rfft(taps.astype(np.float64), nfft)) / L
    f = np.fft.rfftfreq(nfft) * 2 * L  # the filter runs at 24000 L Hz; 1.0 = the input's Nyquist frequency
    lo = min(1.0, L / M)
    pb = 20 * np.log10(H[f <= 0.765 * lo])
    print(f"{L}/{M}: passband {pb.min():+.4f} .. {pb.max():+.4f} dB")
    assert pb.min() >= -0.1 and pb.max() <= 0.1, (pb.min(), pb.max())
    pb = 20 * np.log10(H[f <= 0.75 * lo])
    assert pb.min() >= -0.022 and pb.max() <= 0.022, (pb.min(), pb.max())
    sb = 20 * np.log10(H[f >= lo].max())
    print(f"{L}/{M}: stopband {sb:.2f} dB")
    assert sb <= -91.0, sb


def test_the_fixed_rates_are_three_ratios_of_the_same_design():
    lib = _lib.load()
    for rate, (L, M, N) in FIXED.items():
        n, taps = _lib_ratio_filter(L, M)
        l, m, nn = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        _lib.check(lib.lvx_pcm_filter(rate, ctypes.byref(l), ctypes.byref(m), ctypes.byref(nn), None, 0))
        fixed = np.zeros(2 * N + 1, dtype=np.float32)
        _lib.check(lib.lvx_pcm_filter(rate, None, None, None, fixed.ctypes.data_as(ctypes.c_void_p), fixed.size))
        assert (l.value, m.value, nn.value) == (L, M, N) and n == N
        assert np.array_equal(_bits(taps), _bits(fixed))
        assert np.array_equal(A.ratio_design(L, M)[1], A.design(rate)[3])
        x = _signal(1000, rate)
        assert np.array_equal(_bits(A.ratio_ref(x, L, M)), _bits(A.resample_ref(x, rate)))


def test_ratio_filter_arguments():
    lib = _lib.load()
    N, taps = _lib_ratio_filter(1, 1)  # the identity
    assert N == 0 and taps.tolist() == [1.0] and A.ratio_design(1, 1)[0] == 0
    assert lib.lvx_pcm_ratio_emitted(1, 1, 7, 320, 0) == 320 == A.ratio_emitted(1, 1, 7, 320, False)
    for L, M in [(2, 4), (100, 200), (0, 1), (1, 0), (-4, 5), (201, 200), (199, 201), (1, 5), (5, 1), (3, 3)]:
        assert lib.lvx_pcm_ratio_filter(L, M, None, None, 0) == _lib.LVX_E_ARG, (L, M)
        assert lib.lvx_pcm_ratio_emitted(L, M, 0, 320, 0) == _lib.LVX_E_ARG, (L, M)
        with pytest.raises(ValueError):
            A.ratio_design(L, M)
        with pytest.raises(ValueError):
            A.ratio_ref(np.zeros(8, np.float32), L, M)
    for L, M in [(1, 4), (4, 1), (200, 199), (50, 199)]:  # wider than the plan produces
        assert lib.lvx_pcm_ratio_filter(L, M, None, None, 0) == _lib.LVX_OK
    small = np.zeros(10, dtype=np.float32)
    assert lib.lvx_pcm_ratio_filter(4, 5, None, small.ctypes.data_as(ctypes.c_void_p), 10) == _lib.LVX_E_ARG
    assert lib.lvx_pcm_ratio_emitted(4, 5, -1, 320, 0) == _lib.LVX_E_ARG
    assert lib.lvx_pcm_ratio_emitted(4, 5, 0, -1, 0) == _lib.LVX_E_ARG


# ---- the counts ---------------------------------------------------------------------------------------

def _formula(L, M, T, final):
    N = 24 * max(L, M)
    full = -(-T * L // M)
    if final:
        return full
    if (T - 1) * L < N:
        return 0
    return min(((T - 1) * L - N) // M + 1, full)


@pytest.mark.parametrize("L,M", PAIRS + [(1, 4), (4, 1)])
def test_ratio_emitted_counts(L, M):
    lib = _lib.load()
    for t0 in list(range(0, 60)) + [95, 96, 97, 192, 193, 319, 320, 321, 3200, 81920, 10 ** 7 + 1]:
        for n_in in (0, 1, 2, 3, 24, 25, 48, 49, 96, 97, 193, 256, 320, 333, 3200):
            for final in (0, 1):
                want = _formula(L, M, t0 + n_in, bool(final)) - _formula(L, M, t0, False)
                assert lib.lvx_pcm_ratio_emitted(L, M, t0, n_in, final) == want == A.ratio_emitted(L, M, t0, n_in, bool(final))
                assert want >= 0
    rng = np.random.default_rng(L * 1000 + M)
    for _ in range(30):  # any chunking of a segment emits ceil(T L / M) samples in all
        chunks = rng.integers(0, 700, size=rng.integers(1, 9)).tolist()
        t0 = total = 0
        for k, c in enumerate(chunks):
            total += lib.lvx_pcm_ratio_emitted(L, M, t0, c, int(k == len(chunks) - 1))
            t0 += c
        assert total == -(-t0 * L // M)


# ---- the numpy rule: chunked = one-shot, composition ---------------------------------------------------

@pytest.mark.parametrize("speed,pitch", [(100, 125), (100, 80), (120, 90), (77, 130), (130, 130), (100, 101)])
def test_reference_chunked_equals_one_shot(speed, pitch):
    x = _signal(5000, speed + pitch)
    x[[0, 5, 3199, 3200, 4999]] = [1.0, -1.0, 1.5, -2.0, 1.0]
    for rate, enc in [(24000, "f32le"), (16000, "s16le")]:
        fmt = A.AudioFormat(rate, enc, "raw", speed, pitch)
        stretch, L, M = A.pitch_plan(speed, pitch)
        assert (fmt.stretch_pct, fmt.ratio) == (stretch, (L, M)) and L != M
        one = A.convert_ref(x, fmt)
        n1 = -(-x.size * 100 // stretch)
        n2 = -(-n1 * L // M)
        l, m, _ = A.RATES[rate]
        assert one.size == -(-n2 * l // m) and one.dtype == fmt.dtype
        for chunks in ([3200, 320, 50, 1, 909, 520], [1] * 5 + [4995], [5000, 0], [100, 60, 4840]):
            ref, parts = A.StreamRef(fmt), []
            o = 0
            for k, c in enumerate(chunks):
                parts.append(ref.push(x[o:o + c], k == len(chunks) - 1))
                o += c
            assert np.array_equal(np.concatenate(parts), one), (rate, chunks)


@pytest.mark.parametrize("L,M", [(4, 5), (5, 4), (51, 101), (1, 4)])
def test_ratio_ref_chunked_counts_and_the_double_yardstick(L, M):
    x = _signal(3000, L + M)
    one = A.ratio_ref(x, L, M)
    assert one.size == -(-x.size * L // M) and one.dtype == np.float32
    parts, o = [], 0
    for k, c in enumerate([700, 1, 40, 1259, 1000]):
        final = k == 4
        m0, m1 = A.ratio_emitted_upto(L, M, o, False), A.ratio_emitted_upto(L, M, o + c, final)
        # the outputs a call emits read no input the segment has not seen yet
        parts.append(A.ratio_ref(x[:o + c], L, M, m0=m0, m1=m1))
        assert parts[-1].size == A.ratio_emitted(L, M, o, c, final)
        o += c
    assert np.array_equal(_bits(np.concatenate(parts)), _bits(one))
    N, h = A.ratio_design(L, M)
    taps = h.astype(np.float32)
    y64 = A.ratio_ref(x, L, M, dtype=np.float64)
    n = 2 * N // L + 1
    idx = np.arange(-N, N + 1)
    worst = max(np.abs(taps.astype(np.float64)[(idx - p) % L == 0]).sum() for p in range(L))
    assert np.abs(one - y64).max() <= (n + 1) * 2.0 ** -24 * worst * np.abs(x).max()


def test_composition_is_stretch_then_ratio_then_resample_then_encode():
    x = _signal(3000, 4)
    fmt = A.AudioFormat(16000, "s16le", "raw", 120, 90)
    assert (fmt.stretch_pct, fmt.ratio) == (133, (133, 120))
    want = A.encode_ref(A.resample_ref(A.ratio_ref(A.stretch_ref(x, 133)[0], 133, 120), 16000), fmt)
    assert np.array_equal(A.convert_ref(x, fmt), want) and want.dtype == np.int16
    assert want.size == -(-(-(-(-(-3000 * 100 // 133)) * 133 // 120)) * 2 // 3)
    # a pitch alone whose stretch is 100 percent has no stretch stage: speed 120, pitch 120
    fmt = A.AudioFormat(24000, "f32le", "raw", 120, 120)
    assert (fmt.stretch_pct, fmt.ratio) == (100, (5, 6))
    assert np.array_equal(_bits(A.convert_ref(x, fmt)), _bits(A.ratio_ref(x, 5, 6)))
    # the duration is the speed's, whatever the pitch (to the rounding of the counts)
    for speed, pitch in [(100, 125), (120, 90), (77, 130), (150, 75)]:
        n = A.convert_ref(x, A.AudioFormat(speed_pct=speed, pitch_pct=pitch)).size
        assert abs(n - 3000 * 100 / speed) <= 2


def test_the_pitch_moves_a_tone_by_the_realised_ratio():
    """A 300 Hz tone at pitch 125 (stretch 80, L / M = 4 / 5) comes out at 375 Hz with the duration it had."""
    t = np.arange(24000, dtype=np.float64)
    x = (0.5 * np.sin(2 * np.pi * 300 * t / 24000)).astype(np.float32)
    y = A.convert_ref(x, A.AudioFormat(speed_pct=100, pitch_pct=125))
    assert y.size == 24000
    spec = np.abs(np.fft.rfft(y[2000:22000].astype(np.float64) * np.hanning(20000)))
    peak = np.argmax(spec) * 24000 / 20000
    assert abs(peak - 375.0) <= 24000 / 20000


# ---- AudioFormat ----------------------------------------------------------------------------------------

def test_audio_format_pitch_field():
    assert A.AudioFormat().pitch_pct == 100 and A.AudioFormat(16000, "s16le", "wav", 130).pitch_pct == 100
    assert A.AudioFormat(16000, "s16le", "wav", 130) == A.AudioFormat(16000, "s16le", "wav", 130, 100)
    # neutrality: pitch 100 is default, or converts, exactly as before
    assert A.AudioFormat(pitch_pct=100).is_default and not A.AudioFormat(pitch_pct=100).converts
    assert A.AudioFormat(24000, "f32le", "raw", 100, 100).is_default
    w = A.AudioFormat(container="wav", pitch_pct=100)
    assert not w.is_default and not w.converts
    for args in [(16000,), (24000, "s16le"), (24000, "f32le", "raw", 130)]:
        f = A.AudioFormat(*args)
        assert f.converts and not f.is_default and f.ratio == (1, 1) and f.stretch_pct == f.speed_pct
    f = A.AudioFormat(pitch_pct=125)
    assert f.converts and not f.is_default and f.sample_rate == 24000 and f.dtype == np.dtype("<f4")
    assert f.stretch_pct == 80 and f.ratio == (4, 5)
    assert A.AudioFormat(speed_pct=130, pitch_pct=130).stretch_pct == 100
    for bad in (49, 201, 0, -100, 1.25, "125", True, None):
        with pytest.raises(ValueError):
            A.AudioFormat(pitch_pct=bad)
    for speed, pitch in [(200, 50), (200, 99), (50, 101), (50, 200)]:  # stretch 400, 202, 49 (49.5 half up: 50?), 25
        stretch = (200 * speed + pitch) // (2 * pitch)
        if 50 <= stretch <= 200:
            A.AudioFormat(speed_pct=speed, pitch_pct=pitch)
        else:
            with pytest.raises(ValueError, match="time stretch"):
                A.AudioFormat(speed_pct=speed, pitch_pct=pitch)
    with pytest.raises(ValueError):
        A.AudioFormat(speed_pct=200, pitch_pct=50)
