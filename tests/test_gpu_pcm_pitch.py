"""The device ratio resampler of the pitch control (lvx_pcm_ratio, pcm_kernels.hip: pcm_ratio_kernel) against the
rule of include/llmvox.h ("PCM pitch shift") as llmvox_amd/audio.py states it in numpy, with the library's own
taps: the samples bit for bit, the fp32 accumulation against float64, the three fixed-rate kernels' bits at their
ratios, chunked = one-shot, flush-only calls, row independence (33 rows: two launches), the 1 / 1 bypass, the
argument errors, the three-stage composition through Engine.pcm_convert, and a pitched stream beside a default
one on FusedScheduler(overlap=True)."""
import ctypes

import numpy as np
import pytest
import torch

from llmvox_amd import audio as A

pytestmark = pytest.mark.gpu

CHUNKS = [3200, 320, 50, 1, 909, 320]  # the last one final; one shorter than the history, one of one sample
T = sum(CHUNKS)
B = 3
SLOTS = [5, 0, 2]
PAIRS = [(4, 5), (5, 4), (99, 100), (197, 199), (51, 101), (1, 4), (4, 1)]
FIXED = [(2, 3, 16000), (1, 3, 8000), (2, 1, 48000)]


@pytest.fixture(scope="module")
def eng():
    from llmvox_amd.engine import build_engine
    e = build_engine(0, "fp32", "fp32", max_streams=8, max_positions=64, max_codec_frames=64)
    yield e
    e.close()


@pytest.fixture(scope="module")
def x():
    """Per row: seven harmonics (periods 96 / 150 / 123) plus uniform noise under an amplitude ramp, a run of
    exact zeros, and a few samples beyond +-1."""
    rng = np.random.default_rng(23)
    t = np.arange(T, dtype=np.float64)
    v = np.zeros((B, T), dtype=np.float32)
    for b, P in enumerate([96, 150, 123]):
        tone = 0.2 * sum(np.sin(2 * np.pi * h * t / P) / h for h in range(1, 8))
        v[b] = (tone + rng.uniform(-1, 1, T) * np.linspace(0.0, 0.3, T)).astype(np.float32)
    v[0, 1500:1900] = 0.0
    v[1, 0:400] = 0.0
    v[2, 3100:3500] = 0.0   # (across the first chunk's edge)
    v[0, [0, 1, 3199, 3200, T - 1]] = [1.0, -1.0, 1.5, -2.0, 1.25]
    v[1, [2007, 4479, 4480]] = [-1.0, 3.0, -1.0]
    v[2, [100, 101]] = [1.5, -1.5]
    return v


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _run(eng, x, slots, chunks, L, M, finals=None):
    """The ratio calls of one segment per row: (per row the samples, per call the counts)."""
    xd = torch.from_numpy(np.ascontiguousarray(x)).to(eng.device)
    n = len(slots)
    parts, counts, o = [[] for _ in slots], [], 0
    for k, c in enumerate(chunks):
        fin = [k == len(chunks) - 1] * n if finals is None else finals[k]
        out, cnt = eng.pcm_ratio(xd[:, o:o + c].contiguous() if c else None, slots, fin, L, M)
        host = out.cpu().numpy()
        for b in range(n):
            parts[b].append(host[b, :cnt[b]].copy())
        counts.append(cnt)
        o += c
    eng.check_errors()
    return [np.concatenate(p) for p in parts], counts


@pytest.fixture(scope="module")
def taps(eng):
    return {(L, M): eng.pcm_ratio_filter(L, M)[1] for L, M in PAIRS}


@pytest.fixture(scope="module")
def one_shot(eng, x):
    """The one-call device output of every pair (computed once, shared)."""
    return {(L, M): _run(eng, x, SLOTS, [T], L, M)[0] for L, M in PAIRS}


@pytest.mark.parametrize("L,M", PAIRS)
def test_rule_bit_for_bit(x, taps, one_shot, L, M):
    want = A.ratio_ref(x, L, M, taps[(L, M)])
    for b in range(B):
        got = one_shot[(L, M)][b]
        assert got.size == want.shape[1] == -(-T * L // M)
        assert np.array_equal(_bits(got), _bits(want[b])), (L, M, b, int(np.nonzero(_bits(got) != _bits(want[b]))[0][0]))


@pytest.mark.parametrize("L,M", PAIRS)
def test_against_the_float64_reference(x, taps, one_shot, L, M):
    """|device - the same sums in double| <= (n + 1) 2^-24 max_p sum |h_p| max |x|, n the taps of an output: the
    bound of a length-n fp32 recursive sum of rounded products."""
    h = taps[(L, M)]
    N = 24 * max(L, M)
    n = 2 * N // L + 1
    idx = np.arange(-N, N + 1)
    worst = max(np.abs(h.astype(np.float64)[(idx - p) % L == 0]).sum() for p in range(L))
    want = A.ratio_ref(x, L, M, h, dtype=np.float64)
    bound = (n + 1) * 2.0 ** -24 * worst * float(np.abs(x).max())
    err = max(np.abs(one_shot[(L, M)][b].astype(np.float64) - want[b]).max() for b in range(B))
    print(f"{L}/{M}: max |device - float64| {err:.3e}, bound {bound:.3e}")
    assert err <= bound


@pytest.mark.parametrize("L,M,rate", FIXED)
def test_same_bits_as_the_fixed_rate_kernels(eng, x, L, M, rate):
    xd = torch.from_numpy(x).to(eng.device)
    fmt = A.AudioFormat(rate, "f32le")
    out, cnt = eng.pcm_convert(xd, SLOTS, [True] * B, fmt)
    fixed = out.cpu().numpy()
    one, _ = _run(eng, x, SLOTS, [T], L, M)
    chunked, counts = _run(eng, x, SLOTS, CHUNKS, L, M)
    o = 0
    for k, c in enumerate(CHUNKS):
        assert counts[k] == [eng.lib.lvx_pcm_emitted(rate, o, c, int(k == len(CHUNKS) - 1))] * B
        o += c
    for b in range(B):
        assert cnt[b] == one[b].size == -(-T * L // M)
        assert np.array_equal(_bits(one[b]), _bits(fixed[b, :cnt[b]])), (rate, b)
        assert np.array_equal(_bits(chunked[b]), _bits(one[b])), (rate, b)
    eng.check_errors()


@pytest.mark.parametrize("L,M", PAIRS)
def test_chunked_equals_one_shot(eng, x, one_shot, L, M):
    got, counts = _run(eng, x, SLOTS, CHUNKS, L, M)
    o = 0
    for k, c in enumerate(CHUNKS):
        want = eng.lib.lvx_pcm_ratio_emitted(L, M, o, c, int(k == len(CHUNKS) - 1))
        assert counts[k] == [want] * B and want == A.ratio_emitted(L, M, o, c, k == len(CHUNKS) - 1)
        o += c
    for b in range(B):
        assert np.array_equal(_bits(got[b]), _bits(one_shot[(L, M)][b])), (L, M, b)


@pytest.mark.parametrize("L,M", [(4, 5), (197, 199), (4, 1)])
def test_flush_only_emits_the_rest(eng, x, one_shot, L, M):
    n = len(CHUNKS)
    got, counts = _run(eng, x, SLOTS, CHUNKS + [0], L, M, finals=[[False] * B] * n + [[True] * B])
    emitted = A.ratio_emitted_upto(L, M, T, False)
    assert counts[-1] == [-(-T * L // M) - emitted] * B and counts[-1][0] > 0
    assert sum(c[0] for c in counts[:-1]) == emitted
    for b in range(B):
        assert np.array_equal(_bits(got[b]), _bits(one_shot[(L, M)][b]))
    # a flush with nothing behind it emits nothing (the slots were reset by the final call)
    out, cnt = eng.pcm_ratio(None, SLOTS, [True] * B, L, M)
    assert cnt == [0] * B
    # pcm_reset drops an unfinished segment: the next call starts one
    xd = torch.from_numpy(x).to(eng.device)
    eng.pcm_ratio(xd[:, :1600].contiguous(), SLOTS, [False] * B, L, M)
    for s in SLOTS:
        eng.pcm_reset(s)
    again, _ = _run(eng, x, SLOTS, [T], L, M)
    for b in range(B):
        assert np.array_equal(_bits(again[b]), _bits(one_shot[(L, M)][b]))


@pytest.mark.parametrize("L,M", [(5, 4), (51, 101), (197, 199)])
def test_rows_do_not_depend_on_their_neighbours(eng, x, one_shot, L, M):
    want = one_shot[(L, M)]
    alone, _ = _run(eng, x[1:2], [7], CHUNKS, L, M)  # another slot, no other row
    assert np.array_equal(_bits(alone[0]), _bits(want[1]))
    rev, _ = _run(eng, x[::-1], [1, 3, 4], CHUNKS, L, M)  # other slots, other row order
    for b in range(B):
        assert np.array_equal(_bits(rev[B - 1 - b]), _bits(want[b]))
    # rows whose segments stand at different positions share the later launches
    xd = torch.from_numpy(x).to(eng.device)
    out0, c0 = eng.pcm_ratio(xd[0:1, :3200].contiguous(), [6], [False], L, M)
    parts = [out0.cpu().numpy()[0, :c0[0]].copy()]
    o = 3200
    for k, c in enumerate(CHUNKS[1:]):
        last = k == len(CHUNKS) - 2
        # slot 6 continues row 0 while slot 3 starts row 2's segment from its beginning with the same columns
        pcm = torch.stack([xd[0, o:o + c], xd[2, o - 3200:o - 3200 + c]]).contiguous()
        out, cnt = eng.pcm_ratio(pcm, [6, 3], [last, last], L, M)
        parts.append(out.cpu().numpy()[0, :cnt[0]].copy())
        o += c
    eng.check_errors()
    assert np.array_equal(_bits(np.concatenate(parts)), _bits(want[0]))


def test_33_rows_are_two_launches_of_the_same_rows():
    """One more row than a launch's packet holds: every row's bits are those of the row run alone."""
    from llmvox_amd.engine import build_engine
    e = build_engine(0, "fp32", "fp32", max_streams=40, max_positions=64, max_codec_frames=64)
    try:
        n, rows = 1500, 33
        rng = np.random.default_rng(33)
        v = rng.uniform(-1, 1, (rows, n)).astype(np.float32)
        slots = [(7 * r + 3) % 40 for r in range(rows)]
        assert len(set(slots)) == rows
        L, M = 51, 101
        chunks = [1100, 400]
        both, counts = _run(e, v, slots, chunks, L, M)
        assert counts == [[A.ratio_emitted(L, M, 0, 1100, False)] * rows, [A.ratio_emitted(L, M, 1100, 400, True)] * rows]
        want = A.ratio_ref(v, L, M, e.pcm_ratio_filter(L, M)[1])
        for r in range(rows):
            alone, _ = _run(e, v[r:r + 1], [slots[r]], chunks, L, M)
            assert np.array_equal(_bits(both[r]), _bits(alone[0])), r
            assert np.array_equal(_bits(both[r]), _bits(want[r])), r
    finally:
        e.close()


def test_one_to_one_is_a_bypass(eng, x):
    from llmvox_amd import _lib
    xd = torch.from_numpy(x).to(eng.device)
    out, cnt = eng.pcm_ratio(xd, SLOTS, [True] * B, 1, 1)
    assert cnt == [T] * B and out.data_ptr() == xd.data_ptr()
    out, cnt = eng.pcm_convert(xd, SLOTS, [True] * B, A.AudioFormat(24000, "f32le", "raw", 100, 100))
    assert cnt == [T] * B and out.data_ptr() == xd.data_ptr()
    # the library: nothing launched, nothing written
    guard = torch.full((B, 64), 7.0, device=eng.device)
    n = (ctypes.c_int32 * B)()
    sl, fl = (ctypes.c_int32 * B)(*SLOTS), (ctypes.c_uint8 * B)(0, 0, 0)
    assert eng.lib.lvx_pcm_ratio(eng.h, ctypes.c_void_p(xd.data_ptr()), B, T, sl, fl, 1, 1, ctypes.c_void_p(guard.data_ptr()),
                                 256, n, eng.stream_handle()) == _lib.LVX_OK
    assert list(n) == [T] * B and bool((guard == 7.0).all())
    assert eng.lib.lvx_pcm_ratio(eng.h, ctypes.c_void_p(xd.data_ptr()), B, T, sl, fl, 1, 1, None, 0, n,
                                 eng.stream_handle()) == _lib.LVX_OK
    # a format with pitch 100 makes the calls, and gets the bytes, of the same format without the field
    for args in [(16000, "s16le", "raw", 100), (8000, "f32le", "raw", 130), (24000, "s16le", "raw", 77)]:
        a, ca = eng.pcm_convert(xd, SLOTS, [True] * B, A.AudioFormat(*args, 100))
        b, cb = eng.pcm_convert(xd, SLOTS, [True] * B, A.AudioFormat(*args))
        assert ca == cb and a.dtype == b.dtype and torch.equal(a[:, :ca[0]], b[:, :cb[0]])
    eng.check_errors()


def test_argument_errors(eng, x):
    from llmvox_amd import _lib
    lib = eng.lib
    xd = torch.from_numpy(x[:, :1600].copy()).to(eng.device)
    out = torch.zeros(B, 4096, dtype=torch.float32, device=eng.device)
    cnt = (ctypes.c_int32 * B)()

    def call(slots=(0, 1, 2), L=4, M=5, stride=4096 * 4, n_in=1600, nb=B, optr=None):
        sl = (ctypes.c_int32 * len(slots))(*slots)
        fl = (ctypes.c_uint8 * len(slots))(*([0] * len(slots)))
        return lib.lvx_pcm_ratio(eng.h, ctypes.c_void_p(xd.data_ptr()), nb, n_in, sl, fl, L, M,
                                 ctypes.c_void_p(out.data_ptr() if optr is None else optr), stride, cnt, eng.stream_handle())

    for s in SLOTS + [0, 1]:
        eng.pcm_reset(s)
    first = A.ratio_emitted(4, 5, 0, 1600, False)
    bad = [dict(L=8, M=10), dict(L=0), dict(M=0), dict(L=-4), dict(L=201, M=200), dict(L=1, M=5), dict(L=5, M=1),
           dict(L=3, M=3), dict(slots=(0, 1, 8)), dict(slots=(0, -1, 2)), dict(slots=(0, 1, 0)),
           dict(stride=first * 4 - 4), dict(stride=0), dict(stride=4096 * 4 + 2), dict(optr=out.data_ptr() + 2),
           dict(nb=0), dict(n_in=-1)]
    for kw in bad:
        assert call(**kw) == _lib.LVX_E_ARG, kw
    # none of them moved a slot: the segment still starts here, and a first good call emits a first call's count
    assert first > 0 and call() == 0 and list(cnt) == [first] * B
    # a segment has one ratio (1 / 1 included)
    assert call(L=5, M=4) == _lib.LVX_E_ARG and call(L=1, M=1) == _lib.LVX_E_ARG and call(L=99, M=100) == _lib.LVX_E_ARG
    assert call() == 0 and list(cnt) == [A.ratio_emitted(4, 5, 1600, 1600, False)] * B
    # slot 1 alone stands in another segment: a call that names it beside fresh slots moves none of them
    assert call(slots=(3, 1, 4), L=5, M=4) == _lib.LVX_E_ARG
    assert call(slots=(3, 4, 6), L=5, M=4) == 0 and list(cnt) == [A.ratio_emitted(5, 4, 0, 1600, False)] * B
    assert call() == 0 and list(cnt) == [A.ratio_emitted(4, 5, 3200, 1600, False)] * B
    for s in (0, 1, 2, 3, 4, 6):
        eng.pcm_reset(s)
    with pytest.raises(ValueError):
        eng.pcm_ratio(xd, [0, 1], [False, False], 4, 5)  # rows and slots disagree
    with pytest.raises(ValueError):
        eng.pcm_ratio(xd, [0, 1, 2], [False] * 3, 300, 299)
    with pytest.raises(ValueError):
        eng.pcm_pitch_plan(200, 50)
    assert eng.pcm_pitch_plan(120, 90) == (133, 133, 120) == A.pitch_plan(120, 90)
    assert call() == 0 and list(cnt) == [first] * B  # (neither opened a segment)
    for s in (0, 1, 2):
        eng.pcm_reset(s)
    eng.check_errors()


@pytest.mark.parametrize("args", [(16000, "s16le", "raw", 120, 90), (24000, "f32le", "raw", 100, 125)],
                         ids=lambda a: f"{a[0]}-{a[1]}-{a[3]}-{a[4]}")
def test_composition_through_pcm_convert(eng, x, args):
    fmt = A.AudioFormat(*args)
    taps = eng.pcm_filter(fmt.sample_rate)[3]
    windows = eng.pcm_stretch_window()
    rtaps = eng.pcm_ratio_filter(*fmt.ratio)[1]
    xd = torch.from_numpy(x).to(eng.device)
    parts, o = [[] for _ in SLOTS], 0
    # row 1 joins one chunk late (its own segment starts at the second call): the rows of a call leave the
    # stretch and the ratio stage with different counts
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
        want = A.convert_ref(x[b], fmt, taps, windows, rtaps)
        got = np.concatenate(parts[b])
        assert got.dtype == want.dtype and np.array_equal(got.view(np.uint8), want.view(np.uint8)), (args, b)
    want = A.convert_ref(x[1, :T - 3200], fmt, taps, windows, rtaps)
    assert np.array_equal(np.concatenate(parts[1]).view(np.uint8), want.view(np.uint8))


@pytest.fixture(scope="module")
def sched_eng():
    from llmvox_amd.engine import build_engine
    e = build_engine(0, "fp32", "fp32", max_streams=4, max_positions=256, max_codec_frames=640)
    yield e
    e.close()


def test_scheduler_end_to_end(sched_eng):
    """A 16 kHz s16le stream at speed 1.2 and pitch 0.9 beside a default one on FusedScheduler(overlap=True), same
    text and slot layout as a run of two default streams: the pitched stream's sentence is the rule applied to the
    f32 sentence of the same tokens, and the default stream beside it delivers the bytes it always did."""
    from test_gpu_pcm_out import _lib_taps, _speak
    fmt = A.AudioFormat(16000, "s16le", "raw", 120, 90)
    (tok_a, plain), (tok_b, conv) = _speak(sched_eng, [None, fmt], 100)
    (tok_c, alone), (tok_d, other) = _speak(sched_eng, [None, None], 100)
    assert tok_a == tok_c and tok_b == tok_d and len(plain) >= 3
    assert plain == alone  # the default stream's bytes do not know about its neighbour's pitch
    x = np.frombuffer(b"".join(other), dtype="<f4")  # the f32 samples of the pitched stream's own tokens
    assert x.size == 320 * len(tok_d)
    got = np.frombuffer(b"".join(conv), dtype="<i2")
    want = A.convert_ref(x, fmt, _lib_taps(16000), sched_eng.pcm_stretch_window(), sched_eng.pcm_ratio_filter(133, 120)[1])
    n1 = -(-x.size * 100 // 133)
    n2 = -(-n1 * 133 // 120)
    assert got.size == want.size == -(-n2 * 2 // 3) and np.array_equal(got, want)
