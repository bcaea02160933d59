"""The FLAC rule of include/llmvox.h ("PCM FLAC") as llmvox_amd/audio.py states it in numpy, without a GPU: what it
emits is decoded by tests/flac_decode.py, a decoder written from the format that shares no code with it (its own bit
reader, its own CRCs, and every check of the stream's framing), and gives back the samples exactly; the library's host
entries (lvx_flac_subframe, lvx_flac_finish, lvx_flac_stream_header, the counts) give the same bytes; the format and
the media type."""
import ctypes

import numpy as np
import pytest

import flac_decode as D
from flac_signals import KINDS, RATES, lengths, signal, voiced
from llmvox_amd import audio as A

ROUND_TRIP = ("silence", "constant", "sines", "noise", "alternating", "ramp")  # the rest: test_every_subframe_kind_occurs


def test_crc_check_values():
    assert A.flac_crc8(b"123456789") == 0xF4 and A.flac_crc16(b"123456789") == 0xFEE8
    assert D.crc8(b"123456789") == 0xF4 and D.crc16(b"123456789") == 0xFEE8
    assert A.flac_crc8(b"") == 0 and A.flac_crc16(b"") == 0


@pytest.mark.parametrize("rate", RATES)
def test_stream_header(rate):
    h = A.flac_stream_header(rate)
    assert len(h) == 42
    info = D._stream_info(h)
    assert (info["min_bs"], info["max_bs"], info["rate"]) == (16, rate // 25 + 15, rate)
    assert info["min_frame"] == info["max_frame"] == info["total"] == 0 and info["md5"] == bytes(16)
    assert D.decode(h)[0].size == 0  # a stream of no sentence decodes to nothing


@pytest.mark.parametrize("rate", RATES)
def test_frame_cuts(rate):
    bs = rate // 25
    assert A.flac_block(rate) == bs and A.flac_slot_bytes(rate) == (8 + 1 + 2 * (bs + 15) + 15) // 16 * 16
    for T in list(range(0, 40)) + lengths(rate) + [5 * bs + 16, 5 * bs + 15]:
        sizes = A.flac_frames_of(T, rate)
        assert sum(sizes) == T and all(s == bs for s in sizes[:-1])
        if T >= 16:
            assert 16 <= sizes[-1] <= bs + 15
        assert len(sizes) == A.flac_frames_upto(rate, T, True)
        assert A.flac_frames_upto(rate, T, False) == max(0, (T - 16) // bs) <= max(0, len(sizes) - 1)
        assert T - A.flac_frames_upto(rate, T, False) * bs <= bs + 15  # what a slot keeps between calls
    assert A.flac_emitted(rate, bs, 16, False) == 1 and A.flac_emitted(rate, bs + 16, 0, True) == 1
    with pytest.raises(ValueError):
        A.flac_block(44100)


@pytest.mark.parametrize("rate", RATES)
@pytest.mark.parametrize("kind", ROUND_TRIP)
def test_decoding_gives_the_samples_back(rate, kind):
    for T in lengths(rate):
        q = signal(kind, T, rate)
        data = A.flac_encode_ref(q, rate)
        got, frames = D.decode(data)
        assert got.dtype == np.int16 and np.array_equal(got, q), (kind, T)
        assert [f[1] for f in frames] == A.flac_frames_of(T, rate)
        assert all(size <= 2 * n + 17 for _, n, _, size in frames)
        if kind == "noise" and T >= 16:
            assert {f[2] for f in frames} == {"verbatim"}
        if kind in ("silence", "constant"):
            assert {f[2] for f in frames} == {"constant"}


def test_every_subframe_kind_occurs():
    seen = set()
    for rate in (8000, 24000):
        T = 3 * (rate // 25) + 7
        for kind in KINDS:
            q = signal(kind, T, rate)
            got, frames = D.decode(A.flac_encode_ref(q, rate))
            assert np.array_equal(got, q), kind
            seen |= {f[2] for f in frames}
    assert seen == {"constant", "verbatim", "fixed0", "fixed1", "fixed2", "fixed3", "fixed4"}


def test_the_bound_is_reached():
    """White noise and a 36-bit sample number: 2 n + 17 bytes."""
    n = 320 + 15
    q = signal("noise", n, 8000)
    f = A.flac_frame(q, 8000, (1 << 36) - n)
    assert len(f) == 2 * n + 17 and len(A.flac_subframe(q)) == 1 + 2 * n
    got, frames = D.decode(f, first_sample=(1 << 36) - n, header=False, rate=8000)
    assert np.array_equal(got, q) and frames == [((1 << 36) - n, n, "verbatim", 2 * n + 17)]
    assert f[4] == 0xFE and len(A._flac_utf8((1 << 36) - n)) == 7
    with pytest.raises(ValueError):
        A.flac_frame(q, 8000, (1 << 36) - n + 1)
    for v, ln in ((0, 1), (127, 1), (128, 2), (2047, 2), (2048, 3), (65535, 3), (65536, 4), ((1 << 21) - 1, 4), (1 << 21, 5),
                  (1 << 26, 6), ((1 << 31) - 1, 6), (1 << 31, 7)):
        assert len(A._flac_utf8(v)) == ln and D._utf8(A._flac_utf8(v), 0) == (v, ln)


@pytest.mark.parametrize("rate", (8000, 24000))
def test_any_chunking_gives_the_one_shot_bytes(rate):
    bs = rate // 25
    fmt = A.AudioFormat(rate, "flac")
    x = np.random.default_rng(3).uniform(-0.5, 0.5, 3 * 960 + 123).astype(np.float32)  # 24 kHz f32 in front of the stage
    whole = A.StreamRef(fmt).push(x, True)
    assert whole.dtype == np.uint8 and whole.size % A.flac_slot_bytes(rate) == 0 and whole.size > 0
    q = A.convert_ref(x, A.AudioFormat(rate, "s16le"))
    assert np.array_equal(whole, A.convert_ref(x, fmt))
    mux = A.FlacMux(rate)
    assert mux.header() + mux.push(whole) == A.flac_encode_ref(q, rate) and mux.sample_no == q.size
    for step in (1, 17, bs + 16, 1000):
        ref, parts = A.StreamRef(fmt), []
        step_in = step * 24000 // rate  # (the step counted in the stage's own samples, about)
        for at in range(0, x.size, step_in):
            parts.append(ref.push(x[at:at + step_in], at + step_in >= x.size))
        assert np.array_equal(np.concatenate(parts), whole), step


def test_the_librarys_host_entries_state_the_same_rule():
    from llmvox_amd import _lib
    lib = _lib.load()
    out = ctypes.create_string_buffer(42)
    for rate in RATES:
        assert lib.lvx_pcm_flac_block(rate) == rate // 25
        assert lib.lvx_flac_stream_header(rate, out, 42) == 0 and out.raw == A.flac_stream_header(rate)
        for t0, n_in, final in ((0, 0, 1), (0, 15, 0), (0, 16 + rate // 25, 0), (rate // 25 + 15, 1, 0), (40, 5000, 1), (7, 0, 1)):
            assert lib.lvx_pcm_flac_emitted(rate, t0, n_in, final) == A.flac_emitted(rate, t0, n_in, bool(final))
    assert lib.lvx_pcm_flac_block(44100) == _lib.LVX_E_ARG and lib.lvx_flac_stream_header(8000, out, 41) == _lib.LVX_E_ARG
    for rate in (8000, 24000):
        T = 3 * (rate // 25) + 7
        mux, no = A.FlacMux(rate), 0
        for kind in KINDS:
            q = signal(kind, T, rate)
            for n in (1, 5, 16, 335, T):  # single frames of any length
                buf = ctypes.create_string_buffer(1 + 2 * n)
                ln = lib.lvx_flac_subframe(np.ascontiguousarray(q[:n]).ctypes.data_as(ctypes.c_void_p), n, buf, 1 + 2 * n)
                assert ln > 0 and buf.raw[:ln] == A.flac_subframe(q[:n]), (kind, n)
            slots = A.flac_slots_ref(q, rate, 0, len(A.flac_frames_of(T, rate)))
            assert mux.push(slots) == A.flac_encode_ref(q, rate, sample_no=no, header=False), kind
            no += T
            assert mux.sample_no == no
        with pytest.raises(ValueError):
            mux.push(b"\0" * 7)
        with pytest.raises(_lib.LvxArgError):
            mux.push(bytes(A.flac_slot_bytes(rate)))  # a record with n = 0 is none of the stage's
        assert mux.sample_no == no and mux.push(b"") == b""


def test_the_format():
    f = A.AudioFormat(16000, "flac", volume_pct=250)
    assert f.media_type == "audio/flac" and f.converts and not f.is_default and A.FORMAT_ENCODINGS == A.ENCODINGS + ("flac",) and len(A.FORMAT_ENCODINGS) == 5
    with pytest.raises(ValueError, match="its own container"):
        A.AudioFormat(24000, "flac", "wav")
    assert A.AudioFormat(8000, "s16le", "wav").media_type == "audio/wav"


def test_ratio_on_the_synthetic_voiced_signal():
    """Three seconds of flac_signals.voiced (eleven harmonics of a wobbling 110 Hz under a syllable envelope, plus a
    little noise). Measured with this rule: 0.608 of the s16le bytes at 8 kHz, 0.503 at 16 kHz, 0.474 at 24 kHz, 0.442 at
    48 kHz. No threshold beyond < 1: the ratio on a trained checkpoint's speech has not been measured."""
    for rate in RATES:
        q = voiced(3 * rate, rate)
        data = A.flac_encode_ref(q, rate)
        ratio = len(data) / (2 * q.size)
        print(f"flac / s16le bytes at {rate} Hz: {ratio:.3f}")
        assert ratio < 1 and (rate != 8000 or np.array_equal(D.decode(data)[0], q))
