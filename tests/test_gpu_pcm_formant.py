"""The device formant stage (lvx_pcm_formant, pcm_kernels.hip: pcm_formant_kernel) against the rule of include/llmvox.h
("PCM formant") as llmvox_amd/audio.py states it in numpy (``formant_ref``), with the library's own tables: the tables bit
for bit, the samples bit for bit at five ratios and nine lengths, one-shot and cut into calls of 1, 257 and 1,041 samples,
the per-call counts, every group size of the kernel, row independence (33 rows: two launches), the 1 / 1 bypass, one
ratio per segment, the argument errors, lvx_pcm_reset, the composition through Engine.pcm_convert with the stretch, the
resampler, the level stage and the rate conversion, and a formant stream beside a default one on FusedScheduler(overlap=True)."""
import ctypes

import numpy as np
import pytest
import torch

from llmvox_amd import audio as A

pytestmark = pytest.mark.gpu

RATIOS = ((3, 2), (2, 3), (2, 1), (1, 2), (199, 200))
TS = (1, 255, 256, 257, 767, 768, 769, 1024, 3000)
CUTS = (1, 257, 1041)
B = 3
SLOTS = [5, 0, 2]
H = A.FORMANT_H


@pytest.fixture(scope="module")
def eng():
    from llmvox_amd.engine import build_engine
    e = build_engine(0, "fp32", "fp32", max_streams=8, max_positions=64, max_codec_frames=64)
    yield e
    e.close()


def make_x(T=max(TS), rows=B, seed=41):
    """Per row other content: harmonics of another period under a ramp plus noise of another level; row 1 with a run of
    exact zeros across a hop edge, row 2 with a sample beyond +-1."""
    rng = np.random.default_rng(seed)
    t = np.arange(T, dtype=np.float64)
    v = np.zeros((rows, T), dtype=np.float32)
    for b in range(rows):
        P = (96, 150, 123)[b % 3] + 7 * (b // 3)
        tone = 0.1 * sum(np.sin(2 * np.pi * h * t / P + b) / h for h in range(1, 8))
        v[b] = (tone * np.linspace(0.3, 1.0, T) + rng.standard_normal(T) * 0.01 * (1 + b % 3)).astype(np.float32)
    if T > 1300:
        v[1, 700:1300] = 0.0
    if T > 100:
        v[2 % rows, 100] = 1.5
    return v


@pytest.fixture(scope="module")
def x():
    v = make_x()
    v.setflags(write=False)
    return v


@pytest.fixture(scope="module")
def tabs(eng):
    return eng.pcm_formant_tables()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _cuts(T, cut):
    return [min(cut, T - a) for a in range(0, T, cut)]


def _run(eng, x, slots, chunks, Fn, Fd, finals=None):
    """The formant calls of one segment per row: (per row the samples, per call the counts)."""
    xd = torch.from_numpy(np.array(x, dtype=np.float32)).to(eng.device)
    n = len(slots)
    outs, counts, o = [], [], 0
    for k, c in enumerate(chunks):
        fin = [k == len(chunks) - 1] * n if finals is None else finals[k]
        out, cnt = eng.pcm_formant(xd[:, o:o + c].contiguous() if c else None, slots, fin, Fn, Fd)
        if any(cnt):
            outs.append((out, cnt))  # (read back once, at the end: the calls are stream-ordered)
        counts.append(cnt)
        o += c
    parts = [[] for _ in slots]
    for out, cnt in outs:
        host = out.cpu().numpy()
        for b in range(n):
            parts[b].append(host[b, :cnt[b]])
    eng.check_errors()
    return [np.concatenate(p) if p else np.zeros(0, np.float32) for p in parts], counts


def test_the_library_tables_are_the_rules_bit_for_bit(tabs):
    for got, want, n in zip(tabs, A.formant_tables(), (1024, 25, 1024)):
        assert got.shape == want.shape == (n,) and got.dtype == np.float32
        assert np.array_equal(_bits(got), _bits(want))
    w, c, tw = tabs
    assert np.array_equal(w, w[::-1]) and np.array_equal(c, c[::-1]) and abs(float(c.astype(np.float64).sum()) - 1) < 1e-6
    assert tw[0] == 1.0 and _bits(tw[512:513])[0] == 0x80000000 and tw[512 + 256] == -1.0  # (ti[0] = -sin 0 = -0)


@pytest.fixture(scope="module")
def want(x, tabs):
    """The numpy rule at every ratio and length (computed once, shared, never written to)."""
    out = {}
    for r in RATIOS:
        for T in TS:
            y = A.formant_ref(x[:, :T], *r, tabs)
            y.setflags(write=False)
            out[r, T] = y
    return out


@pytest.mark.parametrize("ratio", RATIOS, ids=lambda r: f"{r[0]}_{r[1]}")
def test_rule_bit_for_bit_one_shot_and_in_cuts(eng, x, want, ratio):
    Fn, Fd = ratio
    for T in TS:
        ref = want[ratio, T]
        for cut in (T,) + CUTS:
            chunks = _cuts(T, cut)
            got, counts = _run(eng, x[:, :T], SLOTS, chunks, Fn, Fd)
            o = 0
            for k, c in enumerate(chunks):
                n = A.formant_emitted(o, c, k == len(chunks) - 1)
                assert counts[k] == [n] * B, (ratio, T, cut, k)
                o += c
            for b in range(B):
                assert got[b].size == T
                same = _bits(got[b]) == _bits(ref[b])
                assert same.all(), (ratio, T, cut, b, int(np.nonzero(~same)[0][0]))
    assert not np.array_equal(_bits(want[ratio, 3000]), _bits(x))  # (the stage did something)


def test_the_bits_do_not_depend_on_the_hop_blocks_a_workgroup_writes(eng, x, want, tabs):
    """Option fmt_group: 1 (a workgroup per hop block), groups that do and do not divide the call's blocks, one larger
    than the call; and the launch's own choice where it is no longer 1 (three rows of 352 hop blocks: two a workgroup)."""
    try:
        for g in (1, 2, 5, 13, 32):
            eng.set_option("fmt_group", g)
            for chunks in ([3000], _cuts(3000, 1041)):
                got, _ = _run(eng, x, SLOTS, chunks, 3, 2)
                for b in range(B):
                    assert np.array_equal(_bits(got[b]), _bits(want[(3, 2), 3000][b])), (g, len(chunks), b)
    finally:
        eng.set_option("fmt_group", 0)
    long = make_x(90000, B, seed=9)
    got, _ = _run(eng, long, SLOTS, [90000], 2, 3)
    ref = A.formant_ref(long, 2, 3, tabs)
    for b in range(B):
        assert np.array_equal(_bits(got[b]), _bits(ref[b])), b


def test_flush_only_and_empty_calls(eng, x, want):
    chunks = [1500, 1500, 0]
    got, counts = _run(eng, x, SLOTS, chunks, 3, 2, finals=[[False] * B, [False] * B, [True] * B])
    assert counts == [[(1500 // H - 3) * H] * B, [(3000 // H - 3) * H - (1500 // H - 3) * H] * B, [3000 - (3000 // H - 3) * H] * B]
    for b in range(B):
        assert np.array_equal(_bits(got[b]), _bits(want[(3, 2), 3000][b]))
    _, cnt = eng.pcm_formant(None, SLOTS, [True] * B, 3, 2)  # nothing behind it: nothing
    assert cnt == [0] * B
    _, cnt = eng.pcm_formant(None, SLOTS, [False] * B, 3, 2)
    assert cnt == [0] * B
    for s in SLOTS:
        eng.pcm_reset(s)


def test_rows_at_different_positions_share_a_launch(eng, x, want):
    xd = torch.from_numpy(np.array(x, dtype=np.float32)).to(eng.device)
    out0, c0 = eng.pcm_formant(xd[0:1, :1041].contiguous(), [6], [False], 2, 3)
    parts = [out0.cpu().numpy()[0, :c0[0]].copy()]
    other = []
    for k, (a, e) in enumerate(((1041, 2082), (2082, 3000))):
        last = k == 1
        # slot 6 continues row 0 while slot 3 runs row 2's segment from its beginning with columns of the same width
        pcm = torch.stack([xd[0, a:e], xd[2, a - 1041:e - 1041]]).contiguous()
        out, cnt = eng.pcm_formant(pcm, [6, 3], [last, last], 2, 3)
        host = out.cpu().numpy()
        parts.append(host[0, :cnt[0]].copy())
        other.append(host[1, :cnt[1]].copy())
    eng.check_errors()
    assert np.array_equal(_bits(np.concatenate(parts)), _bits(want[(2, 3), 3000][0]))
    assert np.array_equal(_bits(np.concatenate(other)), _bits(A.formant_ref(x[2, :3000 - 1041], 2, 3, eng.pcm_formant_tables())))


def test_33_rows_are_two_launches_of_the_same_rows():
    """One more row than a launch's packet holds: every row's bits are those of the row alone."""
    from llmvox_amd.engine import build_engine
    e = build_engine(0, "fp32", "fp32", max_streams=40, max_positions=64, max_codec_frames=64)
    try:
        n, rows = 1500, 33
        v = make_x(n, rows, seed=33)
        slots = [(7 * r + 3) % 40 for r in range(rows)]
        assert len(set(slots)) == rows
        chunks = [1100, 400]
        both, counts = _run(e, v, slots, chunks, 3, 2)
        assert counts == [[(1100 // H - 3) * H] * rows, [n - (1100 // H - 3) * H] * rows]
        y = A.formant_ref(v, 3, 2, e.pcm_formant_tables())
        for r in range(rows):
            assert np.array_equal(_bits(both[r]), _bits(y[r])), r
        for r in (0, 31, 32):  # of the first launch, its last row, and the row of the second launch: each on its own
            alone, _ = _run(e, v[r:r + 1], [slots[r]], chunks, 3, 2)
            assert np.array_equal(_bits(alone[0]), _bits(both[r])), r
    finally:
        e.close()


def test_one_to_one_is_a_bypass(eng, x):
    from llmvox_amd import _lib
    xd = torch.from_numpy(np.array(x, dtype=np.float32)).to(eng.device)
    T = x.shape[1]
    out, cnt = eng.pcm_formant(xd, SLOTS, [True] * B, 1, 1)
    assert cnt == [T] * B and out.data_ptr() == xd.data_ptr()
    for fmt in (A.AudioFormat(formant_pct=100), A.AudioFormat(24000, "f32le", "raw", 100, 100, False, 100, None)):
        out, cnt = eng.pcm_convert(xd, SLOTS, [True] * B, fmt)
        assert cnt == [T] * B and out.data_ptr() == xd.data_ptr()
    # the library: nothing launched, nothing written
    guard = torch.full((B, 64), 7.0, device=eng.device)
    n = (ctypes.c_int32 * B)()
    sl, fl = (ctypes.c_int32 * B)(*SLOTS), (ctypes.c_uint8 * B)(0, 0, 0)
    assert eng.lib.lvx_pcm_formant(eng.h, ctypes.c_void_p(xd.data_ptr()), B, T, sl, fl, 1, 1, ctypes.c_void_p(guard.data_ptr()),
                                   256, n, eng.stream_handle()) == _lib.LVX_OK
    torch.cuda.synchronize()
    assert list(n) == [T] * B and bool((guard == 7.0).all())
    assert eng.lib.lvx_pcm_formant(eng.h, ctypes.c_void_p(xd.data_ptr()), B, T, sl, fl, 1, 1, None, 0, n,
                                   eng.stream_handle()) == _lib.LVX_OK
    # a format whose formant is where the pitch puts the envelope makes the calls, and gets the bytes, of the format
    # without the field
    for args, pct in [((16000, "s16le", "raw", 100, 125, False, 100), 125), ((24000, "f32le", "raw", 100, 80, False, 250), 80)]:
        a, ca = eng.pcm_convert(xd, SLOTS, [True] * B, A.AudioFormat(*args, pct))
        b, cb = eng.pcm_convert(xd, SLOTS, [True] * B, A.AudioFormat(*args))
        assert ca == cb and a.dtype == b.dtype and torch.equal(a[:, :ca[0]], b[:, :cb[0]])
    eng.check_errors()


def test_reset_between_segments(eng, x, want):
    xd = torch.from_numpy(np.array(x, dtype=np.float32)).to(eng.device)
    eng.pcm_formant(xd[:, :1700].contiguous(), SLOTS, [False] * B, 2, 1)  # an unfinished sentence at another ratio
    for s in SLOTS:
        eng.pcm_reset(s)
    again, counts = _run(eng, x, SLOTS, _cuts(3000, 1041), 3, 2)
    assert counts[0] == [(1041 // H - 3) * H] * B
    for b in range(B):
        assert np.array_equal(_bits(again[b]), _bits(want[(3, 2), 3000][b]))


def test_one_ratio_per_segment_and_the_state_survives_the_error(eng, x, want):
    from llmvox_amd import _lib
    xd = torch.from_numpy(np.array(x, dtype=np.float32)).to(eng.device)
    out, cnt = eng.pcm_formant(xd[:, :1041].contiguous(), SLOTS, [False] * B, 3, 2)
    parts = [out.cpu().numpy()[:, :cnt[0]].copy()]
    for other in ((2, 3), (1, 1), (199, 200)):
        with pytest.raises(_lib.LvxArgError) as ei:
            eng.pcm_formant(xd[:, 1041:2082].contiguous(), SLOTS, [False] * B, *other)
        assert ei.value.code == _lib.LVX_E_ARG and "open at the ratio 3 / 2" in str(ei.value)
    # slot 0 alone stands in that segment: a call that names it beside fresh slots moves none of them
    with pytest.raises(_lib.LvxArgError):
        eng.pcm_formant(xd[:, :1041].contiguous(), [3, 0, 4], [False] * B, 2, 3)
    _, cnt = eng.pcm_formant(xd[:, :1041].contiguous(), [3, 4, 6], [False] * B, 2, 3)
    assert cnt == [(1041 // H - 3) * H] * B  # (a first call's count: the refused call opened nothing)
    for s in (3, 4, 6):
        eng.pcm_reset(s)
    for k, (a, e) in enumerate(((1041, 2082), (2082, 3000))):
        out, cnt = eng.pcm_formant(xd[:, a:e].contiguous(), SLOTS, [k == 1] * B, 3, 2)
        parts.append(out.cpu().numpy()[:, :cnt[0]].copy())
    got = np.concatenate(parts, axis=1)
    for b in range(B):
        assert np.array_equal(_bits(got[b]), _bits(want[(3, 2), 3000][b]))
    eng.check_errors()


def test_argument_errors(eng, x):
    from llmvox_amd import _lib
    lib = eng.lib
    xd = torch.from_numpy(x[:, :1600].copy()).to(eng.device)
    out = torch.zeros(B, 4096, dtype=torch.float32, device=eng.device)
    cnt = (ctypes.c_int32 * B)()
    null = object()

    def call(slots=(0, 1, 2), Fn=3, Fd=2, stride=4096 * 4, n_in=1600, nb=B, optr=None, sl=None, fl=None, cn=None, pcm=None,
             final=0):
        sl = (ctypes.c_int32 * len(slots))(*slots) if sl is None else None
        fl = (ctypes.c_uint8 * len(slots))(*([final] * len(slots))) if fl is None else None
        return lib.lvx_pcm_formant(eng.h, None if pcm is null else ctypes.c_void_p(xd.data_ptr()), nb, n_in, sl, fl, Fn, Fd,
                                   None if optr is null else ctypes.c_void_p(out.data_ptr() if optr is None else optr), stride,
                                   cnt if cn is None else None, eng.stream_handle())

    for s in SLOTS + [0, 1]:
        eng.pcm_reset(s)
    first = (1600 // H - 3) * H
    bad = [dict(Fn=0), dict(Fd=0), dict(Fn=-3), dict(Fn=4, Fd=2), dict(Fn=5, Fd=2), dict(Fn=2, Fd=5), dict(Fn=40001, Fd=40000),
           dict(slots=(0, 1, 8)), dict(slots=(0, -1, 2)), dict(slots=(0, 1, 0)), dict(stride=first * 4 - 4), dict(stride=0),
           dict(stride=1600 * 4 - 4, final=1), dict(stride=4096 * 4 + 2), dict(stride=-16), dict(optr=out.data_ptr() + 2),
           dict(optr=null), dict(nb=0), dict(n_in=-1), dict(sl=null), dict(fl=null), dict(cn=null), dict(pcm=null)]
    for kw in bad:
        assert call(**kw) == _lib.LVX_E_ARG, kw
    assert lib.lvx_pcm_formant(None, ctypes.c_void_p(xd.data_ptr()), B, 1600, (ctypes.c_int32 * B)(0, 1, 2),
                               (ctypes.c_uint8 * B)(), 3, 2, ctypes.c_void_p(out.data_ptr()), 4096 * 4, cnt,
                               eng.stream_handle()) == _lib.LVX_E_ARG
    # none of them moved a slot: the segment still starts here, and a first good call emits a first call's count
    assert call() == 0 and list(cnt) == [first] * B
    assert call(stride=(3200 - first) * 4, final=1) == 0 and list(cnt) == [3200 - first] * B  # (a stride that just fits)
    # the host-only entries
    w = np.zeros(1024, dtype=np.float32)
    p = w.ctypes.data_as(ctypes.c_void_p)
    assert lib.lvx_pcm_formant_tables(p, 1023, None, 0, None, 0) == _lib.LVX_E_ARG
    assert lib.lvx_pcm_formant_tables(None, 0, p, 24, None, 0) == _lib.LVX_E_ARG
    assert lib.lvx_pcm_formant_tables(None, 0, None, 0, p, 1023) == _lib.LVX_E_ARG
    assert lib.lvx_pcm_formant_tables(None, 0, None, 0, None, 0) == _lib.LVX_OK
    assert lib.lvx_pcm_formant_tables(p, 1024, None, 0, None, 0) == _lib.LVX_OK and 0 < w[0] < w[511] <= 1
    with pytest.raises(ValueError):
        eng.pcm_formant(xd, [0, 1], [False, False], 3, 2)  # rows and slots disagree
    with pytest.raises(ValueError):
        eng.pcm_formant(xd, [0, 1, 2], [False] * 3, 5, 2)
    assert call() == 0 and list(cnt) == [first] * B  # (neither opened a segment)
    for s in (0, 1, 2):
        eng.pcm_reset(s)
    eng.check_errors()


def test_composition_through_pcm_convert(eng):
    """Stretch, ratio, formant, level, rate and encoding in one format, on a two-sentence stream cut into dumps of 10 and
    30 frames, against convert_ref of each sentence and StreamRef call by call, with the library's tables."""
    fmt = A.AudioFormat(pitch_pct=125, formant_pct=100, volume_pct=200, sample_rate=16000, encoding="s16le")
    assert fmt.stretch_pct == 80 and fmt.ratio == (4, 5) and fmt.formant == (5, 4)
    kw = dict(taps=eng.pcm_filter(16000)[3], windows=eng.pcm_stretch_window(), ratio_taps=eng.pcm_ratio_filter(4, 5)[1],
              level_win=eng.pcm_level_window(), formant_tabs=eng.pcm_formant_tables())
    dumps = [3200, 9600]
    v = make_x(2 * sum(dumps), B, seed=17)
    xd = torch.from_numpy(v).to(eng.device)
    ref = [A.StreamRef(fmt, **kw) for _ in range(B)]
    o = 0
    for sentence in range(2):
        got = [[] for _ in range(B)]
        start = o
        for k, n in enumerate(dumps):
            final = k == len(dumps) - 1
            out, cnt = eng.pcm_convert(xd[:, o:o + n].contiguous(), SLOTS, [final] * B, fmt)
            host = out.cpu().numpy()
            assert host.dtype == np.int16
            for b in range(B):
                step = ref[b].push(v[b, o:o + n], final)
                assert cnt[b] == step.size and np.array_equal(host[b, :cnt[b]], step), (sentence, k, b)
                got[b].append(host[b, :cnt[b]].copy())
            o += n
        for b in range(B):
            whole = A.convert_ref(v[b, start:o], fmt, **kw)
            assert np.array_equal(np.concatenate(got[b]), whole), (sentence, b)
    eng.check_errors()


@pytest.fixture(scope="module")
def sched_eng():
    from llmvox_amd.engine import build_engine
    e = build_engine(0, "fp32", "fp32", max_streams=4, max_positions=256, max_codec_frames=640)
    yield e
    e.close()


def test_scheduler_end_to_end(sched_eng):
    """A formant stream beside a default one on FusedScheduler(overlap=True), same text and slot layout as a run of two
    default streams: the formant stream's sentence is the rule applied to the f32 sentence of the same tokens, every
    sample of it delivered, and the default stream beside it delivers the bytes it delivers alone."""
    from test_gpu_pcm_out import _speak
    fmt = A.AudioFormat(pitch_pct=125, formant_pct=100)
    (tok_a, plain), (tok_b, shaped) = _speak(sched_eng, [None, fmt], 100)
    (tok_c, alone), (tok_d, other) = _speak(sched_eng, [None, None], 100)
    assert tok_a == tok_c and tok_b == tok_d and len(plain) >= 3
    assert plain == alone  # the default stream's bytes do not know about its neighbour's formant
    xs = np.frombuffer(b"".join(other), dtype="<f4")  # the f32 samples of the formant stream's own tokens
    assert xs.size == 320 * len(tok_d)
    got = np.frombuffer(b"".join(shaped), dtype="<f4")
    want = A.convert_ref(xs, fmt, windows=sched_eng.pcm_stretch_window(), ratio_taps=sched_eng.pcm_ratio_filter(4, 5)[1],
                         formant_tabs=sched_eng.pcm_formant_tables())
    assert got.size == want.size == xs.size and np.array_equal(_bits(got), _bits(want))
    pitched = A.convert_ref(xs, A.AudioFormat(pitch_pct=125), windows=sched_eng.pcm_stretch_window(),
                            ratio_taps=sched_eng.pcm_ratio_filter(4, 5)[1])
    assert not np.array_equal(_bits(got), _bits(pitched))


STAGES = ("pcm_join", "pcm_stretch", "pcm_ratio", "pcm_formant", "pcm_level", "_pcm_resample")
J, S, P, F, V, R = STAGES
# per format: the stages each of the two calls of 1,280 samples passes, in order. The formant stage's first call hands
# nothing on (1,280 inputs: 512 out; behind a stretch to 80 percent and 4 / 5 fewer still), so the stages behind it run
# with what it emits; a format without the field never enters it.
PIPELINES = [
    (A.AudioFormat(), [[R], [R]]),
    (A.AudioFormat(pitch_pct=125), [[S, P], [S, P]]),
    (A.AudioFormat(volume_pct=250), [[V], [V]]),
    (A.AudioFormat(formant_pct=100), [[R], [R]]),
    (A.AudioFormat(pitch_pct=125, formant_pct=125), [[S, P], [S, P]]),
    (A.AudioFormat(formant_pct=90), [[F], [F]]),
    (A.AudioFormat(16000, "s16le", "raw", 100, 100, False, 250, 90), [[F, V, R], [F, V, R]]),
]


def test_a_format_makes_exactly_the_stage_calls_it_needs(sched_eng):
    eng, slots = sched_eng, [2, 0, 3]
    log = []

    def recorder(name, inner):
        def call(pcm, slots, *args, **kwargs):
            log.append((name, [int(s) for s in slots]))
            return inner(pcm, slots, *args, **kwargs)
        return call

    xd = torch.from_numpy(make_x(2560, B)).to(eng.device)
    try:
        for name in STAGES:
            setattr(eng, name, recorder(name, getattr(eng, name)))
        for fmt, want in PIPELINES:
            for k in range(2):
                del log[:]
                eng.pcm_convert(xd[:, 1280 * k:1280 * (k + 1)].contiguous(), slots, [k == 1] * B, fmt)
                assert log == [(name, slots) for name in want[k]], (fmt, k, log)
        eng.check_errors()
    finally:
        for name in STAGES:
            eng.__dict__.pop(name, None)
        for s in slots:
            eng.pcm_reset(s)
