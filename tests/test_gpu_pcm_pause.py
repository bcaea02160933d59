"""The device pause stage (lvx_pcm_pause, pcm_pause_kernel in pcm_kernels.hip) against the rule of include/llmvox.h
("PCM pause") as llmvox_amd/audio.py states it in numpy. Bytes are copied and integers compared, so every comparison is
of bytes: the slots the device writes equal ``audio.pause_slots_ref`` at the 4 rates x 4 encodings and the six sentence
lengths around a block's edge, each sentence in one call and cut into calls of 1, 17 and bl + 16 samples; rows of
different lengths that end at different calls; 33 rows, the second packet of a launch; strided input rows at every
alignment; the threshold's edges; the refused calls, each followed by a good call whose counts show no slot moved; and
Engine.pcm_convert with speed, volume and join set against ``audio.StreamRef``."""
import ctypes

import numpy as np
import pytest
import torch

import pause_signals as PS
from llmvox_amd import audio as A

pytestmark = pytest.mark.gpu
SLOTS = (5, 0, 2, 7, 1, 3)
FMTS = [A.AudioFormat(r, e, pause_ms=0) for r in (8000, 16000, 24000, 48000) for e in A.ENCODINGS]
_TORCH = {"f32le": torch.float32, "s16le": torch.int16, "ulaw": torch.uint8, "alaw": torch.uint8}


@pytest.fixture(scope="module")
def eng():
    from llmvox_amd.engine import build_engine
    e = build_engine(0, "fp32", "fp32", max_streams=40, max_positions=64, max_codec_frames=64)
    yield e
    e.close()


def _lengths(bl):
    return [1, bl - 1, bl, bl + 1, 2 * bl, 3 * bl + 7]


def _sentences(fmt, lengths, seed):
    """One sentence per length, blocks active or silent at random, a different content in each."""
    rng, bl = np.random.default_rng(seed), fmt.sample_rate // 100
    out = []
    for T in lengths:
        pattern = list(rng.integers(0, 2, -(-T // bl)))
        out.append(PS.sentence(fmt, pattern, rng, tail=T - (len(pattern) - 1) * bl))
    return out


def _want(fmt, y):
    return A.pause_slots_ref(y, fmt, 0, A.pause_blocks_upto(fmt.sample_rate, y.size, True)).tobytes()


def _speak(eng, fmt, sentences, step, slots=SLOTS, lead=0):
    """The sentences, one a row, through Engine.pcm_pause in calls of ``step`` samples (None: each sentence one call
    of its own), every row's last call final: per row the slots' bytes, concatenated in call order. The rows are read
    where they lie in one device tensor, ``lead`` samples into its rows: strided, at whatever alignment that gives."""
    B, size = len(sentences), A.pause_slot_bytes(fmt)
    width = lead + max(y.size for y in sentences) + 5
    host = np.zeros((B, width), dtype=fmt.dtype)
    for b, y in enumerate(sentences):
        host[b, lead:lead + y.size] = y
    dev = torch.from_numpy(host).to(eng.device)
    parts, at = [[] for _ in range(B)], [0] * B
    while any(at[b] < sentences[b].size for b in range(B)):
        groups = {}  # the rows still speaking, by what this round brings of them (one n_in a call)
        for b in range(B):
            left = sentences[b].size - at[b]
            if left > 0:
                groups.setdefault((at[b], min(step or left, left)), []).append(b)
        for (t0, n), rows in groups.items():
            finals = [t0 + n == sentences[b].size for b in rows]
            src = dev[rows[0]:rows[0] + len(rows)] if rows == list(range(rows[0], rows[0] + len(rows))) else dev[rows]
            out, blocks = eng.pcm_pause(src[:, lead + t0:lead + t0 + n], [slots[b] for b in rows], finals, fmt)
            assert blocks == [A.pause_emitted(fmt.sample_rate, t0, n, f) for f in finals]
            if any(blocks):
                got = out.cpu().numpy()
                for k, b in enumerate(rows):
                    parts[b].append(got[k, :blocks[k] * size].tobytes())
            for b in rows:
                at[b] += n
    return [b"".join(p) for p in parts]


@pytest.mark.parametrize("fmt", FMTS, ids=lambda f: f"{f.sample_rate}-{f.encoding}")
def test_slots_are_the_numpy_rule(eng, fmt):
    """Six rows, the six lengths: they end at different calls, so the later calls carry fewer rows."""
    bl = fmt.sample_rate // 100
    sentences = _sentences(fmt, _lengths(bl), seed=bl + fmt.sample_bytes)
    want = [_want(fmt, y) for y in sentences]
    for k, step in enumerate((None, 1, 17, bl + 16)):
        assert _speak(eng, fmt, sentences, step, lead=k) == want, step  # (lead: another alignment of the rows each time)
    eng.check_errors()


def test_three_rows_that_end_at_different_calls_and_a_second_sentence_behind(eng):
    fmt = A.AudioFormat(16000, "s16le", max_pause_ms=100)
    first = _sentences(fmt, [2 * 160 + 1, 160, 5 * 160 + 159], seed=1)
    second = _sentences(fmt, [160 + 9, 3 * 160, 7], seed=2)
    for step in (17, 176, 1000):
        assert _speak(eng, fmt, first, step, slots=(5, 0, 2), lead=3) == [_want(fmt, y) for y in first]
        assert _speak(eng, fmt, second, step, slots=(5, 0, 2), lead=1) == [_want(fmt, y) for y in second]
    # lvx_pcm_reset in the middle of a sentence: the next one does not see what the slot kept
    dev = torch.from_numpy(np.stack([y[:150] for y in (first[0], first[2])])).to(eng.device)
    _, blocks = eng.pcm_pause(dev, (5, 2), [False, False], fmt)
    assert blocks == [0, 0]
    eng.pcm_reset(5), eng.pcm_reset(2)
    assert _speak(eng, fmt, second, 17, slots=(5, 0, 2)) == [_want(fmt, y) for y in second]


def test_thirty_three_rows(eng):
    """The second packet of a launch (PCM_ROWS = 32 rows a packet)."""
    fmt = A.AudioFormat(8000, "s16le", pause_ms=0)
    sentences = _sentences(fmt, [3 * 80 + 7] * 33, seed=33)
    assert _speak(eng, fmt, sentences, 96, slots=tuple(range(33)), lead=1) == [_want(fmt, y) for y in sentences]
    assert len({_want(fmt, y) for y in sentences}) == 33


@pytest.mark.parametrize("enc", A.ENCODINGS)
def test_threshold_edges_on_the_device(eng, enc):
    fmt = A.AudioFormat(8000, enc, pause_ms=0)
    if enc == "f32le":
        t = np.float32(103 / 32768)
        edge = np.array([t, -t, np.nextafter(t, np.float32(1)), -np.nextafter(t, np.float32(1)), np.nan, np.inf, 0, -0.0,
                         np.nextafter(t, np.float32(0))], np.float32)
    elif enc == "s16le":
        edge = np.array([103, -103, 104, -104, -32768, 32767, 0], np.int16)
    else:
        edge = np.arange(256, dtype=np.uint8)
    # one block a value: the value somewhere in a block of the encoding's silence
    blocks = np.full((edge.size, 80), A.silence_byte(fmt) if enc in A.G711_LAWS else 0, dtype=fmt.dtype)
    blocks[np.arange(edge.size), np.arange(edge.size) % 80] = edge
    y = blocks.reshape(-1)
    got = _speak(eng, fmt, [y], None, slots=(4,), lead=1)[0]
    assert got == _want(fmt, y)
    marks = [got[j * A.pause_slot_bytes(fmt) + 2] for j in range(edge.size)]
    assert marks == [int(v) for v in A.pause_loud(edge, fmt)] and 0 < sum(marks) < edge.size


def test_refused_calls_leave_the_slots_as_they_were(eng):
    from llmvox_amd import _lib
    fmt = A.AudioFormat(8000, "s16le", pause_ms=0)
    bl, size, slots = 80, A.pause_slot_bytes(fmt), (5, 0, 2)
    sentences = _sentences(fmt, [2 * bl + 16] * 3, seed=5)
    want = [_want(fmt, y) for y in sentences]
    dev = torch.from_numpy(np.stack(sentences)).to(eng.device)
    n1 = bl + 40
    out1, blocks = eng.pcm_pause(dev[:, :n1], slots, [False] * 3, fmt)  # the segments are open at 8 kHz s16le, samples kept
    assert blocks == [1, 1, 1]
    head = out1.cpu().numpy()
    rest = dev[:, n1:].contiguous()
    n2 = rest.shape[1]
    buf = torch.zeros(3, 4 * size, dtype=torch.uint8, device=eng.device)
    cnt = (ctypes.c_int32 * 3)(-7, -7, -7)

    def call(slots=slots, sample_rate=8000, enc=_lib.LVX_PCM_S16LE, in_stride=2 * n2, out_stride=4 * size, B=3, n_in=n2,
             offset=0, out_offset=0):
        return eng.lib.lvx_pcm_pause(eng.h, ctypes.c_void_p(rest.data_ptr() + offset), in_stride, B, n_in,
                                     (ctypes.c_int32 * len(slots))(*slots), (ctypes.c_uint8 * 3)(1, 1, 1), sample_rate, enc,
                                     ctypes.c_void_p(buf.data_ptr() + out_offset), out_stride, cnt, eng.stream_handle())

    bad = [dict(sample_rate=44100), dict(enc=2), dict(enc=_lib.LVX_PCM_ULAW), dict(sample_rate=16000),  # no rate, no encoding; another than the open segment's
           dict(slots=(5, 0, 5)), dict(slots=(5, 0, 40)), dict(slots=(5, -1, 2)),  # named twice; out of range
           dict(in_stride=2 * n2 - 2), dict(in_stride=2 * n2 + 1), dict(offset=1),  # smaller than a row; odd; odd pointer
           dict(out_stride=4 * size + 4), dict(out_offset=4),  # no multiples of 8
           dict(B=0), dict(n_in=-1)]
    for kw in bad:
        assert call(**kw) == _lib.LVX_E_ARG, kw
        assert list(cnt) == [-7, -7, -7], kw
    assert call(out_stride=2 * size - 8) == _lib.LVX_E_CAPACITY and list(cnt) == [-7, -7, -7]  # smaller than the row's slots
    assert not buf.any().item()  # nothing was launched
    assert call() == _lib.LVX_OK and list(cnt) == [2, 2, 2]  # the next call is the one it would have been
    tail = buf.cpu().numpy()
    for b in range(3):
        assert head[b, :size].tobytes() + tail[b, :2 * size].tobytes() == want[b], b
    assert eng.lib.lvx_pcm_pause_slot(8000, _lib.LVX_PCM_S16LE) == size == 168
    assert eng.lib.lvx_pcm_pause_slot(48000, _lib.LVX_PCM_F32LE) == 1928 and eng.lib.lvx_pcm_pause_slot(8000, 2) == _lib.LVX_E_ARG
    assert eng.lib.lvx_pcm_pause_emitted(8000, 79, 2, 0) == 1 and eng.lib.lvx_pcm_pause_emitted(44100, 0, 1, 0) == _lib.LVX_E_ARG
    y = np.ascontiguousarray(sentences[0])
    host = np.zeros(len(want[0]), np.uint8)
    assert eng.lib.lvx_pause_slots(8000, _lib.LVX_PCM_S16LE, y.ctypes.data_as(ctypes.c_void_p), y.size, 0, 3,
                                   host.ctypes.data_as(ctypes.c_void_p), host.size) == host.size
    assert host.tobytes() == want[0]


def test_composition_through_pcm_convert(eng):
    """Join, stretch, level, rate, s16le and the pause stage in one format: three dumps with context frames, against
    StreamRef with the library's tables, byte for byte; the body through PauseMux is pause_ref of the s16le sentence."""
    B, slots = 3, (5, 0, 2)
    x = np.random.default_rng(13).uniform(-0.6, 0.6, (B, 5760)).astype(np.float32)
    x[:, :2400] *= np.float32(0.001)  # (eight silent blocks in front, of which the rule keeps two, and one inside)
    x[:, 3000:3600] *= np.float32(0.001)
    fmt = A.AudioFormat(16000, "s16le", "raw", 125, 100, True, 250, pause_ms=100, max_pause_ms=100)
    tables = (eng.pcm_filter(16000)[3], eng.pcm_stretch_window(), None, eng.pcm_join_window(), eng.pcm_level_window())
    ref = [A.StreamRef(fmt, *tables) for _ in range(B)]
    plain = [A.StreamRef(A.AudioFormat(16000, "s16le", "raw", 125, 100, True, 250), *tables) for _ in range(B)]
    dumps = [(0, 3200, 0), (3200 - 2 * 320, 5120, 2), (5120 - 320, 5760, 1)]  # (start with context, end, context frames)
    xd = torch.from_numpy(x).to(eng.device)
    got, samples = [[] for _ in range(B)], [[] for _ in range(B)]
    for k, (a, e, c) in enumerate(dumps):
        final = k == len(dumps) - 1
        out, cnt = eng.pcm_convert(xd[:, a:e].contiguous(), slots, [final] * B, fmt, ctx_frames=[c] * B)
        host = out.cpu().numpy()
        assert host.dtype == np.uint8
        for b in range(B):
            want = ref[b].push(x[b, a:e], final, c)
            assert cnt[b] == want.size and cnt[b] % A.pause_slot_bytes(fmt) == 0 and np.array_equal(host[b, :cnt[b]], want), (k, b)
            got[b].append(host[b, :cnt[b]].tobytes())
            samples[b].append(plain[b].push(x[b, a:e], final, c))
    for b in range(B):
        y = np.concatenate(samples[b])
        body = PS.pushed(b"".join(got[b]), fmt, 1)
        assert body == A.pause_ref([y], fmt) and 0 < len(body) < y.size * 2  # (something was trimmed or capped)
    eng.check_errors()
