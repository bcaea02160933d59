"""The G.711 rule of include/llmvox.h ("PCM G.711") without a GPU: llmvox_amd/audio.py's numpy statement and the
library's host entries (lvx_pcm_g711_encode / lvx_pcm_g711_decode, through ctypes) against the pinned tables, the
rule's stated properties, Python's audioop where it exists, the reference chain (G.711 = the codes of the s16le
stream), the 58-byte WAV header and the format's properties."""
import ctypes
import hashlib
import struct

import numpy as np
import pytest

from llmvox_amd import audio as A

Q = np.arange(-32768, 32768, dtype=np.int32)  # every s16 sample, in order
CODES = np.arange(256, dtype=np.int32)
ENC_SHA = {"ulaw": "90c29de505fb68e766118303bd552a16005dcf810873698bee1d8f3b247ce28c",
           "alaw": "38488f6fd710f4686360edc4d38639f96c491595ef93f8eb8d62d5e07ca6ce7b"}
DEC_SHA = {"ulaw": "3dab54339e520bb2c924826e3b72a917a2b612e9fd12fc867500f1d983a75827",
           "alaw": "e04788d110e58ff8c70c93b8480190d973e3b67876b6119abbaec766cc75c174"}
SPOT = {"ulaw": {0: 0xFF, -1: 0x7F, 32767: 0x80, -32768: 0x00}, "alaw": {0: 0xD5, -1: 0x55, 32767: 0xAA, -32768: 0x2A}}
ZEROS = {"ulaw": 4, "alaw": 16}  # inputs that give the code of 0, and as many that give the code of -1
LAWS = A.G711_LAWS


def _numpy_tables(law):
    return A.g711_encode(Q, law), A.g711_decode(CODES, law)


def _library_tables(law):
    from llmvox_amd import _lib
    lib = _lib.load()
    enc = {"ulaw": _lib.LVX_PCM_ULAW, "alaw": _lib.LVX_PCM_ALAW}[law]
    q, c = Q.astype(np.int16), CODES.astype(np.uint8)
    codes, lin = np.zeros(q.size, dtype=np.uint8), np.zeros(256, dtype=np.int16)
    assert lib.lvx_pcm_g711_encode(enc, q.ctypes.data_as(ctypes.c_void_p), q.size, codes.ctypes.data_as(ctypes.c_void_p)) == 0
    assert lib.lvx_pcm_g711_decode(enc, c.ctypes.data_as(ctypes.c_void_p), c.size, lin.ctypes.data_as(ctypes.c_void_p)) == 0
    return codes, lin


@pytest.fixture(scope="module", params=["numpy", "library"])
def tables(request):
    """{law: (the 65,536 codes of Q, the 256 samples of CODES)} of one of the two statements of the rule."""
    make = _numpy_tables if request.param == "numpy" else _library_tables
    return {law: make(law) for law in LAWS}


@pytest.mark.parametrize("law", LAWS)
def test_the_pinned_tables(tables, law):
    enc, dec = tables[law]
    assert enc.dtype == np.uint8 and enc.shape == (65536,) and dec.dtype == np.int16 and dec.shape == (256,)
    assert hashlib.sha256(enc.tobytes()).hexdigest() == ENC_SHA[law]
    assert hashlib.sha256(dec.astype("<i2").tobytes()).hexdigest() == DEC_SHA[law]


@pytest.mark.parametrize("law", LAWS)
def test_spot_values_and_properties(tables, law):
    enc, dec = (t.astype(np.int32) for t in tables[law])
    for q, c in SPOT[law].items():
        assert enc[q + 32768] == c, (q, hex(c))
    silence = SPOT[law][0]
    assert A.silence_byte(law) == silence == A.silence_byte(A.AudioFormat(8000, law))
    assert int((enc == silence).sum()) == ZEROS[law] == int((enc == silence ^ 0x80).sum())
    assert np.unique(enc).size == 256  # all codes occur
    back = dec[enc]
    assert np.all(np.diff(back) >= 0)  # dec(enc(q)) does not decrease
    assert np.array_equal(enc[::-1], enc ^ 0x80)  # enc(~q) = enc(q) ^ 0x80: Q reversed is ~Q
    again = enc[dec + 32768]  # enc(dec(c))
    keep = CODES != 0x7F if law == "ulaw" else np.ones(256, dtype=bool)
    assert np.array_equal(again[keep], CODES[keep])
    if law == "ulaw":
        assert dec[0x7F] == 0 and again[0x7F] == 0xFF  # negative zero decodes to 0
    err = np.abs(back - Q)
    if law == "alaw":
        assert err.max() == 512
    else:
        assert err[np.abs(Q) <= 32124].max() <= 512 and err.max() == 644  # the clip


def test_numpy_and_library_agree_on_arrays_of_any_shape():
    from llmvox_amd import _lib
    lib = _lib.load()
    rng = np.random.default_rng(711)
    q = rng.integers(-32768, 32768, size=(3, 1001)).astype(np.int16)
    for law, enc in (("ulaw", _lib.LVX_PCM_ULAW), ("alaw", _lib.LVX_PCM_ALAW)):
        want = A.g711_encode(q, law)
        assert want.shape == q.shape and want.dtype == np.uint8
        got = np.zeros(q.shape, dtype=np.uint8)
        assert lib.lvx_pcm_g711_encode(enc, q.ctypes.data_as(ctypes.c_void_p), q.size, got.ctypes.data_as(ctypes.c_void_p)) == 0
        assert np.array_equal(got, want)
        lin = np.zeros(q.shape, dtype=np.int16)
        assert lib.lvx_pcm_g711_decode(enc, got.ctypes.data_as(ctypes.c_void_p), got.size, lin.ctypes.data_as(ctypes.c_void_p)) == 0
        assert np.array_equal(lin, A.g711_decode(want, law)) and lin.dtype == A.g711_decode(want, law).dtype


def test_library_argument_errors():
    from llmvox_amd import _lib
    lib = _lib.load()
    q, c = np.zeros(4, dtype=np.int16), np.full(4, 0xA5, dtype=np.uint8)
    qp, cp = q.ctypes.data_as(ctypes.c_void_p), c.ctypes.data_as(ctypes.c_void_p)
    for enc in (_lib.LVX_PCM_F32LE, _lib.LVX_PCM_S16LE, 2, 3, 5, 8, -1):
        assert lib.lvx_pcm_g711_encode(enc, qp, 4, cp) == _lib.LVX_E_ARG
        assert lib.lvx_pcm_g711_decode(enc, cp, 4, qp) == _lib.LVX_E_ARG
    for enc in (_lib.LVX_PCM_ULAW, _lib.LVX_PCM_ALAW):
        assert lib.lvx_pcm_g711_encode(enc, qp, -1, cp) == _lib.LVX_E_ARG
        assert lib.lvx_pcm_g711_encode(enc, None, 4, cp) == _lib.LVX_E_ARG
        assert lib.lvx_pcm_g711_encode(enc, qp, 4, None) == _lib.LVX_E_ARG
        assert lib.lvx_pcm_g711_decode(enc, cp, -1, qp) == _lib.LVX_E_ARG
        assert lib.lvx_pcm_g711_decode(enc, None, 4, qp) == _lib.LVX_E_ARG
        assert lib.lvx_pcm_g711_decode(enc, cp, 4, None) == _lib.LVX_E_ARG
        assert b"LVX_PCM_ULAW" in lib.lvx_last_error()
        assert lib.lvx_pcm_g711_encode(enc, None, 0, None) == 0 and lib.lvx_pcm_g711_decode(enc, None, 0, None) == 0
    assert np.all(c == 0xA5) and np.all(q == 0)  # nothing was written
    for bad in ("mulaw", "ULAW", "s16le", None):
        with pytest.raises(ValueError):
            A.g711_encode(q, bad)
        with pytest.raises(ValueError):
            A.g711_decode(c, bad)
    with pytest.raises(ValueError):
        A.g711_encode(np.array([32768]), "ulaw")
    with pytest.raises(ValueError):
        A.g711_encode(np.array([0.5]), "alaw")
    with pytest.raises(ValueError):
        A.g711_decode(np.array([256]), "alaw")


@pytest.mark.parametrize("law", LAWS)
def test_audioop_identities(law):
    audioop = pytest.importorskip("audioop")
    enc, dec = _numpy_tables(law)
    lin2 = audioop.lin2ulaw if law == "ulaw" else audioop.lin2alaw
    back = audioop.ulaw2lin if law == "ulaw" else audioop.alaw2lin
    theirs = np.frombuffer(lin2(Q.astype("<i2").tobytes(), 2), dtype=np.uint8).astype(np.int32)
    assert np.array_equal(np.frombuffer(back(CODES.astype(np.uint8).tobytes(), 2), dtype="<i2"), dec)
    if law == "alaw":
        assert np.array_equal(theirs, enc)
        return
    mine = enc.astype(np.int32)
    assert np.array_equal(theirs[Q >= 0], mine[Q >= 0])
    # audioop negates in two's complement and never emits 0x7F: on q < 0 the table is its code of ~q without the sign
    of_not_q = theirs[::-1]
    assert np.array_equal(mine[Q < 0], of_not_q[Q < 0] & 0x7F)
    assert int((theirs != mine).sum()) == 508 and not np.any(theirs == 0x7F)


@pytest.mark.parametrize("law", LAWS)
@pytest.mark.parametrize("rate", [24000, 16000, 8000, 48000])
def test_reference_is_the_codes_of_the_s16le_stream(rate, law):
    rng = np.random.default_rng(rate)
    x = rng.uniform(-1.1, 1.1, 2001).astype(np.float32)
    x[:3] = [2.0, -2.0, 0.0]
    if rate == 24000:  # (elementwise there: a filter would spread them over its taps)
        x[3:6] = [np.nan, np.inf, -np.inf]
    fmt, s16 = A.AudioFormat(rate, law), A.AudioFormat(rate, "s16le")
    one = A.convert_ref(x, fmt)
    assert one.dtype == np.uint8 == fmt.dtype and np.array_equal(one, A.g711_encode(A.convert_ref(x, s16), law))
    assert np.array_equal(A.encode_ref(x, fmt), A.g711_encode(A.quantize_s16(x), law))
    ref, ref16 = A.StreamRef(fmt), A.StreamRef(s16)
    parts, o = [], 0
    for k, c in enumerate([700, 1, 0, 1300]):
        got = ref.push(x[o:o + c], k == 3)
        assert got.dtype == np.uint8 and np.array_equal(got, A.g711_encode(ref16.push(x[o:o + c], k == 3), law))
        parts.append(got)
        o += c
    assert np.array_equal(np.concatenate(parts), one)


@pytest.mark.parametrize("law,tag", [("ulaw", 7), ("alaw", 6)])
@pytest.mark.parametrize("rate", [8000, 24000])
def test_wav_header_is_the_58_byte_form(rate, law, tag):
    h = A.wav_header(A.AudioFormat(rate, law, "wav"))
    assert len(h) == 58
    assert h[0:4] == b"RIFF" and struct.unpack("<I", h[4:8])[0] == 0xFFFFFFFF and h[8:12] == b"WAVE"
    assert h[12:16] == b"fmt " and struct.unpack("<I", h[16:20])[0] == 18
    assert struct.unpack("<HHIIHHH", h[20:38]) == (tag, 1, rate, rate, 1, 8, 0)  # ..., byte rate, block align, bits, cbSize
    assert h[38:42] == b"fact" and struct.unpack("<II", h[42:50]) == (4, 0xFFFFFFFF)
    assert h[50:54] == b"data" and struct.unpack("<I", h[54:58])[0] == 0xFFFFFFFF
    assert len(A.wav_header(A.AudioFormat(rate, "s16le", "wav"))) == 44  # the PCM tags keep theirs


def test_audio_format_properties():
    assert A.ENCODINGS == ("f32le", "s16le", "ulaw", "alaw") and A.G711_LAWS == ("ulaw", "alaw")
    for law in LAWS:
        for rate in A.RATES:
            f = A.AudioFormat(rate, law)
            assert f.sample_bytes == 1 and f.dtype == np.dtype("uint8") and f.converts and not f.is_default
            assert f.media_type == "application/octet-stream"
        assert A.AudioFormat(8000, law, "wav").media_type == "audio/wav"
    assert [A.silence_byte(A.AudioFormat(8000, e)) for e in A.ENCODINGS] == [0, 0, 0xFF, 0xD5]
    assert A.AudioFormat(24000, "s16le").sample_bytes == 2 and A.AudioFormat().sample_bytes == 4
    for bad in ("mulaw", "ULAW", "pcmu", "u8", "g711"):
        with pytest.raises(ValueError, match="ulaw"):
            A.AudioFormat(8000, bad)


def _snr_db(x, y):
    return 10 * np.log10(np.sum(x.astype(np.float64) ** 2) / np.sum((x.astype(np.float64) - y) ** 2))


@pytest.mark.parametrize("law,want", [("ulaw", (37.5, 38.3, 35.5)), ("alaw", (37.4, 38.6, 34.0))])
def test_snr_of_a_sine(law, want):
    """A 440 Hz sine at 8 kHz (one second), at -3, -20 and -40 dBFS, through encode and decode: the figures the README
    quotes, within 0.5 dB. A property of the pinned tables, not of new code."""
    t = np.arange(8000) / 8000.0
    for level, db in zip((-3, -20, -40), want):
        q = A.quantize_s16((10 ** (level / 20) * np.sin(2 * np.pi * 440 * t)).astype(np.float32))
        got = _snr_db(q, A.g711_decode(A.g711_encode(q, law), law))
        print(f"{law} at {level} dBFS: {got:.2f} dB")
        assert abs(got - db) <= 0.5, (law, level, got)


def test_frames_on_the_host():
    assert A.FRAME_MS == (10, 20, 30, 40, 60)
    for rate in A.RATES:
        for enc in A.ENCODINGS:
            for ms in A.FRAME_MS:
                f = A.AudioFormat(rate, enc)
                assert A.frame_bytes(f, ms) * 1000 == rate * ms * f.sample_bytes  # a whole number of bytes
    assert A.frame_bytes(A.AudioFormat(8000, "ulaw"), 20) == 160
    for bad in (0, 15, 20.0, True, "20", 50, -20):
        with pytest.raises(ValueError):
            A.frame_ms_of(bad)
    assert A.frame_ms_of(None) is None and A.frame_ms_of(60) == 60
    fmt = A.AudioFormat(8000, "alaw")
    chunks = [bytes([k]) * n for k, n in enumerate([1, 159, 160, 161, 1000])]
    out = list(A.frame_chunks(iter(chunks), fmt, 20))
    assert all(c and len(c) % 160 == 0 for c in out)
    whole = b"".join(chunks)
    assert b"".join(out) == whole + b"\xd5" * (-len(whole) % 160)
    assert list(A.frame_chunks(iter([b"", b"x" * 320, b""]), fmt, 20)) == [b"x" * 320]  # nothing to fill, nothing added
    assert list(A.frame_chunks(iter([]), fmt, 20)) == []
