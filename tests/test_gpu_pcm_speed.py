"""The device time stretch (lvx_pcm_stretch, pcm_kernels.hip) against the rule of include/llmvox.h ("PCM time
stretch") as llmvox_amd/audio.py states it in numpy, with the library's own window tables: the samples and the
chosen offsets bit for bit, chunked = one-shot, flush-only calls, row independence, the composition with the
resampler and the quantiser through Engine.pcm_convert, the speed-100 bypass, the argument errors, and a
1.3x 16 kHz s16le stream beside a default one on FusedScheduler(overlap=True)."""
import ctypes

import numpy as np
import pytest
import torch

from llmvox_amd import audio as A

pytestmark = pytest.mark.gpu

CHUNKS = [3200, 320, 960, 320]  # the last one final
T = sum(CHUNKS)
B = 3
SLOTS = [5, 0, 2]
SPEEDS = [50, 77, 130, 200]
H = A.STRETCH_H


@pytest.fixture(scope="module")
def eng():
    from llmvox_amd.engine import build_engine
    e = build_engine(0, "fp32", "fp32", max_streams=8, max_positions=64, max_codec_frames=64)
    yield e
    e.close()


@pytest.fixture(scope="module")
def windows(eng):
    return eng.pcm_stretch_window()


@pytest.fixture(scope="module")
def x():
    """Per row: seven harmonics (periods 96 / 150 / 123) plus uniform noise under an amplitude ramp, a
    400-sample run of exact zeros (equal scores, the 1e-9 term), and a few samples beyond +-1."""
    rng = np.random.default_rng(17)
    t = np.arange(T, dtype=np.float64)
    v = np.zeros((B, T), dtype=np.float32)
    for b, P in enumerate([96, 150, 123]):
        tone = 0.2 * sum(np.sin(2 * np.pi * h * t / P) / h for h in range(1, 8))
        v[b] = (tone + rng.uniform(-1, 1, T) * np.linspace(0.0, 0.3, T)).astype(np.float32)
    v[0, 1500:1900] = 0.0
    v[1, 0:400] = 0.0       # (the segment starts silent: hops whose every score is equal)
    v[2, 3100:3500] = 0.0   # (across the first chunk's edge)
    v[0, [0, 1, 3199, 3200, T - 1]] = [1.0, -1.0, 1.5, -2.0, 1.25]
    v[1, [2007, 4479, 4480]] = [-1.0, 3.0, -1.0]
    v[2, [100, 101]] = [1.5, -1.5]
    return v


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _run(eng, x, slots, chunks, pct, finals=None):
    """The stretch calls of one segment per row: (per row the samples, per row the d_j, per call the counts)."""
    xd = torch.from_numpy(np.ascontiguousarray(x)).to(eng.device)
    n = len(slots)
    parts, ds, counts, o = [[] for _ in slots], [[] for _ in slots], [], 0
    for k, c in enumerate(chunks):
        fin = [k == len(chunks) - 1] * n if finals is None else finals[k]
        out, cnt, d = eng.pcm_stretch(xd[:, o:o + c].contiguous() if c else None, slots, fin, pct, want_d=True)
        host, dh = out.cpu().numpy(), d.cpu().numpy()
        for b in range(n):
            parts[b].append(host[b, :cnt[b]].copy())
            ds[b].append(dh[b, :-(-cnt[b] // H)].copy())
        counts.append(cnt)
        o += c
    eng.check_errors()
    return [np.concatenate(p) for p in parts], [np.concatenate(p) for p in ds], counts


@pytest.fixture(scope="module")
def one_shot(eng, x):
    """The one-call device output of every speed (computed once, shared)."""
    return {pct: _run(eng, x, SLOTS, [T], pct)[:2] for pct in SPEEDS}


@pytest.fixture(scope="module")
def ref(x, windows):
    """The numpy statement of the rule with the library's window tables (computed once, shared)."""
    return {pct: [A.stretch_ref(x[b], pct, windows) for b in range(B)] for pct in SPEEDS}


def test_library_windows_are_the_rule(windows):
    wr, wf = windows
    n = np.arange(H, dtype=np.float64)
    want = 0.5 - 0.5 * np.cos(np.pi * (n + 0.5) / H)
    assert wr.dtype == wf.dtype == np.float32
    # rounded once from double: half an fp32 place below 1, and a libm cosine's last place of a double
    tol = 2.0 ** -25 + 2.0 ** -52
    assert np.abs(wr.astype(np.float64) - want).max() <= tol and np.abs(wf.astype(np.float64) - (1 - want)).max() <= tol


@pytest.mark.parametrize("pct", SPEEDS)
def test_rule_bit_for_bit(one_shot, ref, pct):
    got, got_d = one_shot[pct]
    for b in range(B):
        want, want_d = ref[pct][b]
        assert got[b].size == want.size == -(-T * 100 // pct) and got_d[b].size == want_d.size
        if not np.array_equal(_bits(got[b]), _bits(want)):
            hops = np.nonzero(got_d[b] != want_d)[0]
            first = int(np.nonzero(_bits(got[b]) != _bits(want))[0][0])
            where = (f"first hop whose d_j differs: {int(hops[0])} (device {int(got_d[b][hops[0]])}, rule "
                     f"{int(want_d[hops[0]])}): the search" if hops.size else "every d_j agrees: the output stage")
            raise AssertionError(f"speed {pct} row {b}: samples differ from sample {first} (hop {first // H}); {where}")
        assert np.array_equal(got_d[b], want_d), (pct, b)
    assert any(ref[pct][b][1].any() for b in range(B))  # (the search chose something)


@pytest.mark.parametrize("pct", SPEEDS)
def test_chunked_equals_one_shot(eng, x, one_shot, pct):
    got, got_d, counts = _run(eng, x, SLOTS, CHUNKS, pct)
    o = 0
    for k, c in enumerate(CHUNKS):
        want = eng.lib.lvx_pcm_stretch_emitted(pct, o, c, int(k == len(CHUNKS) - 1))
        assert counts[k] == [want] * B and want == A.stretch_emitted(pct, o, c, k == len(CHUNKS) - 1)
        o += c
    for b in range(B):
        assert np.array_equal(_bits(got[b]), _bits(one_shot[pct][0][b])), (pct, b)
        assert np.array_equal(got_d[b], one_shot[pct][1][b]), (pct, b)


@pytest.mark.parametrize("pct", SPEEDS)
def test_flush_only_emits_the_rest(eng, x, one_shot, pct):
    got, got_d, counts = _run(eng, x, SLOTS, CHUNKS + [0], pct, finals=[[False] * B] * 4 + [[True] * B])
    emitted = A.stretch_emitted_upto(pct, T, False)
    assert counts[-1] == [-(-T * 100 // pct) - emitted] * B and counts[-1][0] > 0
    assert sum(c[0] for c in counts[:-1]) == emitted
    for b in range(B):
        assert np.array_equal(_bits(got[b]), _bits(one_shot[pct][0][b])) and np.array_equal(got_d[b], one_shot[pct][1][b])
    # a flush with nothing behind it emits nothing (the slots were reset by the final call)
    out, cnt, _ = eng.pcm_stretch(None, SLOTS, [True] * B, pct)
    assert cnt == [0] * B
    # pcm_reset drops an unfinished segment: the next call starts one
    xd = torch.from_numpy(x).to(eng.device)
    eng.pcm_stretch(xd[:, :1600].contiguous(), SLOTS, [False] * B, pct)
    for s in SLOTS:
        eng.pcm_reset(s)
    again, again_d, _ = _run(eng, x, SLOTS, [T], pct)
    for b in range(B):
        assert np.array_equal(_bits(again[b]), _bits(one_shot[pct][0][b])) and np.array_equal(again_d[b], one_shot[pct][1][b])


@pytest.mark.parametrize("pct", SPEEDS)
def test_rows_do_not_depend_on_their_neighbours(eng, x, one_shot, pct):
    want = one_shot[pct][0]
    alone, _, _ = _run(eng, x[1:2], [7], CHUNKS, pct)  # another slot, no other row
    assert np.array_equal(_bits(alone[0]), _bits(want[1]))
    rev, _, _ = _run(eng, x[::-1], [1, 3, 4], CHUNKS, pct)  # other slots, other row order
    for b in range(B):
        assert np.array_equal(_bits(rev[B - 1 - b]), _bits(want[b]))
    # rows whose segments stand at different positions share the later launches
    xd = torch.from_numpy(x).to(eng.device)
    out0, c0, _ = eng.pcm_stretch(xd[0:1, :3200].contiguous(), [6], [False], pct)
    parts = [out0.cpu().numpy()[0, :c0[0]].copy()]
    o = 3200
    for k, c in enumerate(CHUNKS[1:]):
        # slot 6 continues row 0 while slot 3 starts row 2's segment from its beginning with the same columns
        pcm = torch.stack([xd[0, o:o + c], xd[2, o - 3200:o - 3200 + c]]).contiguous()
        out, cnt, _ = eng.pcm_stretch(pcm, [6, 3], [k == 2, k == 2], pct)
        parts.append(out.cpu().numpy()[0, :cnt[0]].copy())
        o += c
    eng.check_errors()
    assert np.array_equal(_bits(np.concatenate(parts)), _bits(want[0]))


def test_33_rows_are_two_launches_of_the_same_rows():
    """One more row than a launch's packet holds, a non-final and a final call: the rows on both sides of the
    launches' edge, the second launch's row 32 among them, carry the numpy rule's bits."""
    from llmvox_amd.engine import build_engine
    e = build_engine(0, "fp32", "fp32", max_streams=40, max_positions=64, max_codec_frames=64)
    try:
        rows, pct = 33, 130
        rng = np.random.default_rng(33)
        t = np.arange(1280, dtype=np.float64)
        v = np.stack([0.3 * np.sin(2 * np.pi * t / (90 + 2 * r)) + rng.uniform(-0.1, 0.1, t.size)
                      for r in range(rows)]).astype(np.float32)
        slots = [(7 * r + 3) % 40 for r in range(rows)]
        assert len(set(slots)) == rows
        got, got_d, counts = _run(e, v, slots, [640, 640], pct)
        assert counts == [[A.stretch_emitted(pct, 0, 640, False)] * rows, [A.stretch_emitted(pct, 640, 640, True)] * rows]
        assert counts[0][0] > 0
        windows = e.pcm_stretch_window()
        for r in (0, 31, 32):
            want, want_d = A.stretch_ref(v[r], pct, windows)
            assert np.array_equal(_bits(got[r]), _bits(want)) and np.array_equal(got_d[r], want_d), r
    finally:
        e.close()


@pytest.mark.parametrize("pct", [77, 130])
@pytest.mark.parametrize("rate,enc", [(16000, "s16le"), (48000, "f32le")])
def test_composition_through_pcm_convert(eng, x, windows, rate, enc, pct):
    fmt = A.AudioFormat(rate, enc, "raw", pct)
    taps = eng.pcm_filter(rate)[3]
    xd = torch.from_numpy(x).to(eng.device)
    parts, o = [[] for _ in SLOTS], 0
    # row 1 joins one chunk late (its own segment starts at the second call): the stretched rows of a call
    # hold different counts
    for k, c in enumerate(CHUNKS):
        rows = [0, 1, 2] if k else [0, 2]
        cols = [xd[b, o:o + c] if b != 1 else xd[1, o - 3200:o - 3200 + c] for b in rows]
        out, cnt = eng.pcm_convert(torch.stack(cols).contiguous(), [SLOTS[b] for b in rows],
                                   [k == len(CHUNKS) - 1] * len(rows), fmt)
        host = out.cpu().numpy()
        assert host.dtype == fmt.dtype
        for r, b in enumerate(rows):
            parts[b].append(host[r, :cnt[r]].copy())
        o += c
    eng.check_errors()
    for b in (0, 2):
        assert np.array_equal(np.concatenate(parts[b]), A.convert_ref(x[b], fmt, taps, windows)), (rate, enc, pct, b)
    assert np.array_equal(np.concatenate(parts[1]), A.convert_ref(x[1, :T - 3200], fmt, taps, windows))


def test_speed_100_is_a_bypass(eng, x):
    xd = torch.from_numpy(x).to(eng.device)
    out, cnt = eng.pcm_convert(xd, SLOTS, [True] * B, A.AudioFormat(24000, "f32le", "raw", 100))
    assert cnt == [T] * B and out.data_ptr() == xd.data_ptr()
    out, cnt, d = eng.pcm_stretch(xd, SLOTS, [True] * B, 100)
    assert cnt == [T] * B and out.data_ptr() == xd.data_ptr() and d is None
    # the library: nothing launched, nothing written
    from llmvox_amd import _lib
    guard = torch.full((B, 64), 7.0, device=eng.device)
    n = (ctypes.c_int32 * B)()
    sl, fl = (ctypes.c_int32 * B)(*SLOTS), (ctypes.c_uint8 * B)(0, 0, 0)
    assert eng.lib.lvx_pcm_stretch(eng.h, ctypes.c_void_p(xd.data_ptr()), B, T, sl, fl, 100, ctypes.c_void_p(guard.data_ptr()),
                                   256, n, None, 0, eng.stream_handle()) == _lib.LVX_OK
    assert list(n) == [T] * B and bool((guard == 7.0).all())
    for rate, enc in [(16000, "s16le"), (8000, "f32le"), (24000, "s16le")]:
        a, ca = eng.pcm_convert(xd, SLOTS, [True] * B, A.AudioFormat(rate, enc, "raw", 100))
        b, cb = eng.pcm_convert(xd, SLOTS, [True] * B, A.AudioFormat(rate, enc))
        assert ca == cb and a.dtype == b.dtype and torch.equal(a[:, :ca[0]], b[:, :cb[0]])
        assert np.array_equal(a.cpu().numpy()[1, :ca[1]], A.convert_ref(x[1], A.AudioFormat(rate, enc), eng.pcm_filter(rate)[3]))
    eng.check_errors()


def test_argument_errors(eng, x):
    from llmvox_amd import _lib
    lib = eng.lib
    xd = torch.from_numpy(x[:, :1600].copy()).to(eng.device)
    out = torch.zeros(B, 4096, dtype=torch.float32, device=eng.device)
    cnt = (ctypes.c_int32 * B)()

    def call(slots=(0, 1, 2), pct=130, stride=4096 * 4, n_in=1600, nb=B, optr=None):
        sl = (ctypes.c_int32 * len(slots))(*slots)
        fl = (ctypes.c_uint8 * len(slots))(*([0] * len(slots)))
        return lib.lvx_pcm_stretch(eng.h, ctypes.c_void_p(xd.data_ptr()), nb, n_in, sl, fl, pct,
                                   ctypes.c_void_p(out.data_ptr() if optr is None else optr), stride, cnt, None, 0,
                                   eng.stream_handle())

    for s in SLOTS + [0, 1]:
        eng.pcm_reset(s)
    first = A.stretch_emitted(130, 0, 1600, False)
    bad = [dict(pct=49), dict(pct=201), dict(pct=0), dict(pct=-130), dict(slots=(0, 1, 8)), dict(slots=(0, -1, 2)),
           dict(slots=(0, 1, 0)), dict(stride=first * 4 - 4), dict(stride=0), dict(stride=4096 * 4 + 2),
           dict(optr=out.data_ptr() + 2), dict(nb=0), dict(n_in=-1)]
    for kw in bad:
        assert call(**kw) == _lib.LVX_E_ARG, kw
    assert lib.lvx_pcm_stretch_emitted(49, 0, 320, 0) == _lib.LVX_E_ARG and lib.lvx_pcm_stretch_emitted(130, -1, 320, 0) == _lib.LVX_E_ARG
    small = np.zeros(H - 1, np.float32)
    assert lib.lvx_pcm_stretch_window(small.ctypes.data_as(ctypes.c_void_p), small.ctypes.data_as(ctypes.c_void_p), H - 1) == _lib.LVX_E_ARG
    # none of them moved a slot: the segment still starts here, and a first good call emits a first call's count
    assert first > 0 and call() == 0 and list(cnt) == [first] * B
    # a segment has one speed (100 included)
    assert call(pct=77) == _lib.LVX_E_ARG and call(pct=100) == _lib.LVX_E_ARG
    assert call() == 0 and list(cnt) == [A.stretch_emitted(130, 1600, 1600, False)] * B
    # the optional d_out must hold a row's hops
    dbuf = torch.zeros(B, 64, dtype=torch.int32, device=eng.device)
    sl, fl = (ctypes.c_int32 * B)(0, 1, 2), (ctypes.c_uint8 * B)(0, 0, 0)
    assert lib.lvx_pcm_stretch(eng.h, ctypes.c_void_p(xd.data_ptr()), B, 1600, sl, fl, 130, ctypes.c_void_p(out.data_ptr()),
                               4096 * 4, cnt, ctypes.c_void_p(dbuf.data_ptr()), 1, eng.stream_handle()) == _lib.LVX_E_ARG
    assert call() == 0 and list(cnt) == [A.stretch_emitted(130, 3200, 1600, False)] * B
    for s in (0, 1, 2):
        eng.pcm_reset(s)
    with pytest.raises(ValueError):
        eng.pcm_convert(xd, [0, 1], [False, False], A.AudioFormat(16000, "s16le", "raw", 130))  # rows and slots disagree
    with pytest.raises(ValueError):
        eng.pcm_stretch(xd, [0, 1, 2], [False] * 3, 300)
    assert call() == 0 and list(cnt) == [first] * B  # (neither opened a segment)
    for s in (0, 1, 2):
        eng.pcm_reset(s)
    eng.check_errors()


@pytest.fixture(scope="module")
def sched_eng():
    from llmvox_amd.engine import build_engine
    e = build_engine(0, "fp32", "fp32", max_streams=4, max_positions=256, max_codec_frames=640)
    yield e
    e.close()


def test_scheduler_end_to_end(sched_eng):
    """A 1.3x 16 kHz s16le stream beside a default one on FusedScheduler(overlap=True), same text and slot
    layout as a run of two default streams: the stretched stream's sentence is the rule applied to the f32
    sentence of the same tokens, and the default stream beside it delivers the bytes it always did."""
    from test_gpu_pcm_out import _lib_taps, _speak
    fmt = A.AudioFormat(16000, "s16le", "raw", 130)
    (tok_a, plain), (tok_b, conv) = _speak(sched_eng, [None, fmt], 100)
    (tok_c, alone), (tok_d, other) = _speak(sched_eng, [None, None], 100)
    assert tok_a == tok_c and tok_b == tok_d and len(plain) >= 3
    assert plain == alone  # the default stream's bytes do not know about its neighbour's speed
    x = np.frombuffer(b"".join(other), dtype="<f4")  # the f32 samples of the stretched stream's own tokens
    assert x.size == 320 * len(tok_d)
    got = np.frombuffer(b"".join(conv), dtype="<i2")
    want = A.convert_ref(x, fmt, _lib_taps(16000), sched_eng.pcm_stretch_window())
    assert got.size == want.size == -(-(-(-x.size * 100 // 130)) * 2 // 3) and np.array_equal(got, want)
