"""The PCM output stage's rule on the host (no GPU): the library's filter design and streaming counts
(lvx_pcm_filter / lvx_pcm_emitted, host-only entry points) against the numpy statement of the rule in
llmvox_amd/audio.py, the filters' frequency responses against the figures of include/llmvox.h, the
reference's chunked = one-shot invariant, the WAV header and AudioFormat's validation."""
import ctypes
import struct

import numpy as np
import pytest

from llmvox_amd import _lib
from llmvox_amd import audio as A

TABLE = {16000: (2, 3, 72, 73), 8000: (1, 3, 72, 145), 48000: (2, 1, 48, 49)}  # rate: L, M, N, max taps per output
STOPBAND_DB = {16000: -92.0, 8000: -92.0, 48000: -91.0}


def _lib_filter(rate):
    lib = _lib.load()
    L, M, N = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    _lib.check(lib.lvx_pcm_filter(rate, ctypes.byref(L), ctypes.byref(M), ctypes.byref(N), None, 0))
    taps = np.zeros(2 * N.value + 1, dtype=np.float32)
    _lib.check(lib.lvx_pcm_filter(rate, None, None, None, taps.ctypes.data_as(ctypes.c_void_p), taps.size))
    return L.value, M.value, N.value, taps


@pytest.mark.parametrize("rate", sorted(TABLE))
def test_library_filter_is_the_numpy_design(rate):
    L, M, N, taps = _lib_filter(rate)
    assert (L, M, N) == TABLE[rate][:3] == A.RATES[rate]
    l, m, n, h = A.design(rate)
    assert (l, m, n) == (L, M, N) and h.dtype == np.float64 and h.size == 2 * N + 1 == taps.size
    assert np.abs(taps - h).max() <= 1e-6 * np.abs(h).max()
    # taps per output: the phases of the prototype
    per_phase = [np.arange(-N, N + 1)[(np.arange(-N, N + 1) - p) % L == 0].size for p in range(L)]
    assert max(per_phase) == TABLE[rate][3]
    for p in range(L):  # DC gain of every phase
        assert abs(taps.astype(np.float64)[(np.arange(-N, N + 1) - p) % L == 0].sum() - 1.0) < 1e-5


def test_library_filter_arguments():
    lib = _lib.load()
    L, M, N, taps = _lib_filter(24000)
    assert (L, M, N) == (1, 1, 0) and taps.tolist() == [1.0]
    for bad in (22050, 44100, 0, -16000, 24001):
        assert lib.lvx_pcm_filter(bad, None, None, None, None, 0) == _lib.LVX_E_ARG
        assert lib.lvx_pcm_emitted(bad, 0, 320, 0) == _lib.LVX_E_ARG
    small = np.zeros(10, dtype=np.float32)
    assert lib.lvx_pcm_filter(16000, None, None, None, small.ctypes.data_as(ctypes.c_void_p), 10) == _lib.LVX_E_ARG
    assert lib.lvx_pcm_emitted(16000, -1, 320, 0) == _lib.LVX_E_ARG
    assert lib.lvx_pcm_emitted(16000, 0, -1, 0) == _lib.LVX_E_ARG


@pytest.mark.parametrize("rate", sorted(TABLE))
def test_library_filter_response(rate):
    """The float64 response of the library's fp32 taps: within 0.1 dB up to 0.765 of the lower Nyquist
    frequency, and the table's stopband (with a 1 dB margin) from that Nyquist frequency on."""
    L, M, N, taps = _lib_filter(rate)
    nfft = 1 << 16
    H = np.abs(np.fft.rfft(taps.astype(np.float64), nfft)) / L
    f = np.fft.rfftfreq(nfft) * 2 * L  # the filter runs at 24000 L Hz; 1.0 = the input's Nyquist frequency
    lo = min(1.0, L / M)               # the lower of the input's and the output's Nyquist frequencies
    pb = 20 * np.log10(H[f <= 0.765 * lo])
    assert pb.min() >= -0.1 and pb.max() <= 0.1, (pb.min(), pb.max())
    sb = 20 * np.log10(H[f >= lo].max())
    assert sb <= STOPBAND_DB[rate] + 1.0, sb


def _formula(rate, T, final):
    L, M, N = A.RATES[rate]
    full = -(-T * L // M)
    if final or N == 0:
        return full
    if (T - 1) * L < N:
        return 0
    return min(((T - 1) * L - N) // M + 1, full)


@pytest.mark.parametrize("rate", [24000, 16000, 8000, 48000])
def test_emitted_counts(rate):
    lib = _lib.load()
    for t0 in list(range(0, 200)) + [319, 320, 321, 3200, 81920, 10 ** 7 + 1]:
        for n_in in (0, 1, 2, 3, 36, 37, 72, 73, 145, 160, 320, 333, 3200):
            for final in (0, 1):
                want = _formula(rate, t0 + n_in, bool(final)) - _formula(rate, t0, False)
                assert lib.lvx_pcm_emitted(rate, t0, n_in, final) == want == A.emitted(rate, t0, n_in, bool(final))
                assert want >= 0
    rng = np.random.default_rng(rate)
    L, M, _ = A.RATES[rate]
    for _ in range(50):  # any chunking of a segment emits ceil(T L / M) samples in all
        chunks = rng.integers(0, 700, size=rng.integers(1, 9)).tolist()
        t0 = total = 0
        for k, c in enumerate(chunks):
            total += lib.lvx_pcm_emitted(rate, t0, c, int(k == len(chunks) - 1))
            t0 += c
        assert total == -(-t0 * L // M)


@pytest.mark.parametrize("enc", A.ENCODINGS)
@pytest.mark.parametrize("rate", [24000, 16000, 8000, 48000])
def test_reference_chunked_equals_one_shot(rate, enc):
    rng = np.random.default_rng(7)
    x = rng.uniform(-1, 1, 7040).astype(np.float32)
    x[[0, 5, 3199, 3200, 7039]] = [1.0, -1.0, 1.5, -2.0, 1.0]
    fmt = A.AudioFormat(rate, enc)
    one = A.convert_ref(x, fmt)
    L, M, _ = A.RATES[rate]
    assert one.size == -(-x.size * L // M) and one.dtype == fmt.dtype
    for chunks in ([320, 3200, 960, 320, 2240], [1] * 5 + [7035], [7040], [7040, 0], [100, 60, 6880]):
        ref = A.StreamRef(fmt)
        parts, o = [], 0
        for k, c in enumerate(chunks):
            parts.append(ref.push(x[o:o + c], k == len(chunks) - 1))
            assert parts[-1].size == A.emitted(rate, o, c, k == len(chunks) - 1)
            o += c
        assert np.array_equal(np.concatenate(parts), one), chunks
    # the fp32 order against the same sums in double: the accumulation bound of the GPU test
    y32, y64 = A.resample_ref(x, rate), A.resample_ref(x, rate, dtype=np.float64)
    taps = A.design(rate)[3].astype(np.float32)
    K = max(1, -(-taps.size // L))
    assert np.abs(y32 - y64).max() <= (K + 1) * 2.0 ** -24 * np.abs(taps).sum() * np.abs(x).max()


def test_quantize_rule():
    v = np.array([0.0, 1.0, -1.0, 2.0, -2.0, np.nan, np.inf, -np.inf, 0.5 / 32768, 1.5 / 32768, 2.5 / 32768,
                  -0.5 / 32768, -1.5 / 32768, 32766.5 / 32768, 0.999999, -0.99999, 1e-9], dtype=np.float32)
    q = A.quantize_s16(v)
    assert q.dtype == np.int16
    assert q.tolist() == [0, 32767, -32768, 32767, -32768, 0, 32767, -32768, 0, 2, 2, 0, -2, 32766, 32767, -32768, 0]


def test_wav_header_bytes():
    h = A.wav_header(A.AudioFormat(16000, "s16le", "wav"))
    assert len(h) == 44
    assert h[:4] == b"RIFF" and h[8:16] == b"WAVEfmt " and h[36:40] == b"data"
    assert struct.unpack("<I", h[4:8])[0] == 0xFFFFFFFF and struct.unpack("<I", h[40:44])[0] == 0xFFFFFFFF
    assert struct.unpack("<IHHIIHH", h[16:36]) == (16, 1, 1, 16000, 32000, 2, 16)
    h = A.wav_header(A.AudioFormat(48000, "f32le", "wav"))
    assert len(h) == 44 and struct.unpack("<IHHIIHH", h[16:36]) == (16, 3, 1, 48000, 192000, 4, 32)
    assert struct.unpack("<IHHIIHH", A.wav_header(A.AudioFormat(container="wav"))[16:36]) == (16, 3, 1, 24000, 96000, 4, 32)


def test_audio_format_validation():
    d = A.AudioFormat()
    assert (d.sample_rate, d.encoding, d.container) == (24000, "f32le", "raw")
    assert d.is_default and not d.converts and d.media_type == "application/octet-stream"
    w = A.AudioFormat(container="wav")
    assert not w.is_default and not w.converts and w.media_type == "audio/wav"
    s = A.AudioFormat(24000, "s16le")
    assert not s.is_default and s.converts and s.sample_bytes == 2 and s.dtype == np.dtype("<i2")
    r = A.AudioFormat(8000)
    assert not r.is_default and r.converts and r.sample_bytes == 4 and r.dtype == np.dtype("<f4")
    for kw in ({"sample_rate": 22050}, {"sample_rate": 44100}, {"sample_rate": 0}, {"sample_rate": "16000"},
               {"sample_rate": 16000.0}, {"sample_rate": True}, {"encoding": "s16be"}, {"encoding": "mulaw"},
               {"encoding": None}, {"container": "ogg"}, {"container": ""}):
        with pytest.raises(ValueError):
            A.AudioFormat(**kw)
