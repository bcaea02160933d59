"""The device FLAC stage (lvx_pcm_flac, pcm_flac_kernel in pcm_kernels.hip) against the rule of include/llmvox.h
("PCM FLAC") as llmvox_amd/audio.py states it in numpy. The rule is integer arithmetic, so every comparison is of bytes:
the slots the device writes, finished on the host by lvx_flac_finish (audio.FlacMux), equal audio.flac_encode_ref at
every sentence length around the frame cuts, one-shot and cut into calls of 1, 17 and BS + 16 samples, three rows with
a different signal each on slots (5, 0, 2); a second sentence right behind a final call; Engine.pcm_convert with a FLAC
format against the same call as s16le through the independent decoder; the argument errors."""
import ctypes

import numpy as np
import pytest
import torch

import flac_decode as D
from flac_signals import KINDS, lengths, signal
from llmvox_amd import audio as A

pytestmark = pytest.mark.gpu
SLOTS = (5, 0, 2)


@pytest.fixture(scope="module")
def eng():
    from llmvox_amd.engine import build_engine
    e = build_engine(0, "fp32", "fp32", max_streams=8, max_positions=64, max_codec_frames=64)
    yield e
    e.close()


def _rows(rate, T, turn):
    """Three sentences of T samples, a different signal kind in each row (the kinds rotate with ``turn``)."""
    return np.stack([signal(KINDS[(turn + 3 * b) % len(KINDS)], T, rate) for b in range(3)])


def _speak(eng, q, rate, step, slots=SLOTS):
    """The rows of q through Engine.pcm_flac in calls of ``step`` samples (None: one call), the last one final: per row
    the slots' bytes, concatenated in call order."""
    B, T = q.shape
    dev = torch.from_numpy(q).to(eng.device)
    size, parts = A.flac_slot_bytes(rate), [[] for _ in range(B)]
    step = step or T
    for at in range(0, T, step):
        final = at + step >= T
        out, frames = eng.pcm_flac(dev[:, at:at + step], slots, [final] * B, rate)
        assert frames == [A.flac_emitted(rate, at, min(step, T - at), final)] * B
        if any(frames):
            host = out.cpu().numpy()
            for b in range(B):
                parts[b].append(host[b, :frames[b] * size].tobytes())
    return [b"".join(p) for p in parts]


def _finished(blob, rate):
    mux = A.FlacMux(rate)
    return mux.header() + mux.push(blob)


@pytest.mark.parametrize("rate", [8000, 24000])
def test_slots_finish_to_the_numpy_rule(eng, rate):
    bs = rate // 25
    for turn, T in enumerate(lengths(rate)):
        q = _rows(rate, T, turn)
        want = [A.flac_encode_ref(q[b], rate) for b in range(3)]
        for step in (None, 1, 17, bs + 16):
            got = _speak(eng, q, rate, step)
            for b in range(3):
                assert _finished(got[b], rate) == want[b], (rate, T, step, b)
                if step is None:  # and the slots themselves, zeros to their ends included
                    assert np.array_equal(np.frombuffer(got[b], np.uint8),
                                          A.flac_slots_ref(q[b], rate, 0, len(A.flac_frames_of(T, rate))))


@pytest.mark.parametrize("rate", [16000, 48000])
def test_the_other_rates(eng, rate):
    bs = rate // 25
    T = 2 * bs + 16
    for turn in (0, 1, 2):  # (every signal kind once in some row)
        q = _rows(rate, T, turn)
        want = [A.flac_encode_ref(q[b], rate) for b in range(3)]
        for step in (None, 17, bs + 16) + ((1,) if turn == 0 else ()):
            got = _speak(eng, q, rate, step)
            assert [_finished(g, rate) for g in got] == want, (rate, turn, step)


def test_every_subframe_kind_came_from_the_device(eng):
    seen = set()
    for rate in (8000, 24000):
        T = 3 * (rate // 25) + 7
        for turn in range(4):
            for blob in _speak(eng, _rows(rate, T, turn), rate, None):
                seen |= {f[2] for f in D.decode(_finished(blob, rate))[1]}
    assert seen == {"constant", "verbatim", "fixed0", "fixed1", "fixed2", "fixed3", "fixed4"}


def test_a_second_sentence_right_behind_a_final_call(eng):
    """The two-buffer turn and the reset: calls that leave the slots' histories full, a final call, then another
    sentence on the same slots, which must not see the first; and lvx_pcm_reset in the middle of a third."""
    rate, bs = 8000, 320
    first, second = _rows(rate, 2 * bs + 15, 1), _rows(rate, bs + 17, 2)
    for step in (17, bs + 16, None):
        a = _speak(eng, first, rate, step)
        b = _speak(eng, second, rate, step)
        assert [_finished(g, rate) for g in a] == [A.flac_encode_ref(first[r], rate) for r in range(3)]
        assert [_finished(g, rate) for g in b] == [A.flac_encode_ref(second[r], rate) for r in range(3)]
    dev = torch.from_numpy(first).to(eng.device)
    _, frames = eng.pcm_flac(dev[:, :bs + 100], SLOTS, [False] * 3, rate)  # an open segment with kept samples
    assert frames == [1, 1, 1]
    for s in SLOTS:
        eng.pcm_reset(s)
    b = _speak(eng, second, rate, 17)
    assert [_finished(g, rate) for g in b] == [A.flac_encode_ref(second[r], rate) for r in range(3)]


def test_pcm_convert_decodes_to_the_s16le_call(eng):
    """Random f32 rows at volume 250 %: the FLAC body decodes to exactly the samples of the same call as s16le, in one
    call and in dumps of 6,400 samples (rows leave the level stage with other counts than they entered)."""
    x = np.random.default_rng(11).uniform(-0.6, 0.6, (3, 19200)).astype(np.float32)
    dev = torch.from_numpy(x).to(eng.device)
    for dump in (19200, 6400):
        got = {}
        for enc in ("s16le", "flac"):
            fmt, parts = A.AudioFormat(8000, enc, volume_pct=250), [[] for _ in range(3)]
            for at in range(0, 19200, dump):
                out, cnt = eng.pcm_convert(dev[:, at:at + dump], SLOTS, [at + dump >= 19200] * 3, fmt)
                assert out.dtype == (torch.uint8 if enc == "flac" else torch.int16)
                host = out.cpu().numpy()
                for b in range(3):
                    parts[b].append(host[b, :cnt[b]].tobytes())
                if enc == "flac":
                    assert all(n % A.flac_slot_bytes(8000) == 0 for n in cnt)
            got[enc] = [b"".join(p) for p in parts]
        for b in range(3):
            want = np.frombuffer(got["s16le"][b], dtype="<i2")
            assert want.size == 6400
            samples, frames = D.decode(_finished(got["flac"][b], 8000))
            assert np.array_equal(samples, want) and len(frames) == len(A.flac_frames_of(6400, 8000))


def test_argument_errors_leave_the_slots_as_they_were(eng):
    from llmvox_amd import _lib
    rate, bs = 8000, 320
    size = A.flac_slot_bytes(rate)
    q = _rows(rate, 2 * bs + 16, 0)
    want = [A.flac_encode_ref(q[b], rate) for b in range(3)]
    dev = torch.from_numpy(q).to(eng.device)
    n1 = bs + 40
    out1, frames = eng.pcm_flac(dev[:, :n1], SLOTS, [False] * 3, rate)  # the segments are open at 8 kHz, samples kept
    assert frames == [1, 1, 1]
    head = out1.cpu().numpy()
    rest = dev[:, n1:].contiguous()
    n2 = rest.shape[1]
    buf = torch.zeros(3, 4 * size, dtype=torch.uint8, device=eng.device)
    cnt = (ctypes.c_int32 * 3)(-7, -7, -7)

    def call(slots=SLOTS, sample_rate=rate, src=rest, in_stride=2 * n2, dst=buf, out_stride=4 * size, B=3, n_in=n2, offset=0):
        return eng.lib.lvx_pcm_flac(eng.h, ctypes.c_void_p(src.data_ptr() + offset), in_stride, B, n_in,
                                    (ctypes.c_int32 * len(slots))(*slots), (ctypes.c_uint8 * 3)(1, 1, 1), sample_rate,
                                    ctypes.c_void_p(dst.data_ptr()), out_stride, cnt, eng.stream_handle())

    bad = [dict(sample_rate=44100), dict(sample_rate=16000),  # no rate of the stage; another than the open segment's
           dict(slots=(5, 0, 5)), dict(slots=(5, 0, 8)), dict(slots=(5, -1, 2)),  # named twice; out of range
           dict(in_stride=2 * n2 - 2), dict(in_stride=2 * n2 + 1), dict(offset=1),  # smaller than a row; odd; odd pointer
           dict(out_stride=2 * size - 16), dict(out_stride=4 * size + 2),  # smaller than the row's slots; no multiple of 4
           dict(B=0), dict(n_in=-1)]
    for kw in bad:
        assert call(**kw) == _lib.LVX_E_ARG, kw
        assert list(cnt) == [-7, -7, -7], kw
    assert not buf.any().item()  # nothing was launched
    assert call() == _lib.LVX_OK and list(cnt) == [2, 2, 2]  # the next call is the one it would have been
    tail = buf.cpu().numpy()
    for b in range(3):
        assert _finished(head[b, :size].tobytes() + tail[b, :2 * size].tobytes(), rate) == want[b], b
