"""The device watermark stage (lvx_pcm_mark, pcm_kernels.hip: pcm_mark_kernel) against the rule of include/llmvox.h
("PCM mark") as llmvox_amd/audio.py states it in numpy (``mark_ref``), with the library's own tables: the sign table bit
for bit, the samples bit for bit at five lengths, one-shot and cut into calls of 1, 257 and 1,792 samples with a
flush-only final, two strengths, 1, 3 and 33 rows, every group size of the kernel, silence, lvx_pcm_reset, one mark per
segment, the argument errors, the composition through Engine.pcm_convert with the stretch, the resampler, the formant
stage, the level stage and the rate conversion, the stage calls a format makes, and the detector on the device's output."""
import ctypes

import numpy as np
import pytest
import torch

import mark_signals as MS
from llmvox_amd import audio as A

pytestmark = pytest.mark.gpu

TS = (1, 255, 256, 1025, 7 * 256 + 5)
CUTS = (1, 257, 1792)
B = 3
SLOTS = [5, 0, 2]
H = A.FORMANT_H
KEY, ID = MS.KEY, MS.ID


@pytest.fixture(scope="module")
def eng():
    from llmvox_amd.engine import build_engine
    e = build_engine(0, "fp32", "fp32", max_streams=8, max_positions=64, max_codec_frames=64)
    yield e
    e.close()


def make_x(T=max(TS), rows=B, seed=43):
    """Per row other content: harmonics of another period (many of them inside the marked band) under a ramp plus noise
    of another level; row 1 with a run of exact zeros across a hop edge, row 2 with a sample beyond +-1."""
    rng = np.random.default_rng(seed)
    t = np.arange(T, dtype=np.float64)
    v = np.zeros((rows, T), dtype=np.float32)
    for b in range(rows):
        P = (96, 150, 123)[b % 3] + 7 * (b // 3)
        tone = 0.1 * sum(np.sin(2 * np.pi * h * t / P + b) / h for h in range(1, 16))
        v[b] = (tone * np.linspace(0.3, 1.0, T) + rng.standard_normal(T) * 0.01 * (1 + b % 3)).astype(np.float32)
    if T > 1300:
        v[1 % rows, 700:1300] = 0.0
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


@pytest.fixture(scope="module")
def want(eng, x, tabs):
    """The numpy rule at both strengths and every length, with the library's tables (computed once, never written to)."""
    words = eng.pcm_mark_table(KEY, ID)
    out = {}
    for strength in (2, 3):
        for T in TS:
            y = A.mark_ref(x[:, :T], KEY, ID, strength, tabs, words=words)
            y.setflags(write=False)
            out[strength, T] = y
    return out


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _cuts(T, cut):
    return [min(cut, T - a) for a in range(0, T, cut)]


def _run(eng, x, slots, chunks, strength=2, key=KEY, mark_id=ID, finals=None):
    """The mark calls of one segment per row: (per row the samples, per call the counts)."""
    xd = torch.from_numpy(np.array(x, dtype=np.float32)).to(eng.device)
    n = len(slots)
    outs, counts, o = [], [], 0
    for k, c in enumerate(chunks):
        fin = [k == len(chunks) - 1] * n if finals is None else finals[k]
        out, cnt = eng.pcm_mark(xd[:, o:o + c].contiguous() if c else None, slots, fin, key, mark_id, strength)
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


def test_the_library_sign_table_is_the_rules(eng):
    for key in (0, 1, KEY, MS.OTHER_KEY, (1 << 64) - 1):
        for mark_id in (0, 1, ID, 255):
            got = eng.pcm_mark_table(key, mark_id)
            assert got.dtype == np.uint16 and np.array_equal(got, A.mark_table(key, mark_id)), mark_id
    for bad in (-1, 1 << 64, True, 1.0):
        with pytest.raises(ValueError):
            eng.pcm_mark_table(bad, 0)


@pytest.mark.parametrize("strength", (2, 3))
def test_rule_bit_for_bit_one_shot_and_in_cuts(eng, x, want, strength):
    """Every length one-shot and in every cut, the cut runs ended by a flush-only final call; the per-call counts."""
    for T in TS:
        ref = want[strength, T]
        for cut in (T,) + (CUTS if strength == 2 else CUTS[1:]):
            chunks = _cuts(T, cut) + ([0] if cut != T else [])
            got, counts = _run(eng, x[:, :T], SLOTS, chunks, strength)
            o = 0
            for k, c in enumerate(chunks):
                n = A.mark_emitted(o, c, k == len(chunks) - 1)
                assert counts[k] == [n] * B, (T, cut, k)
                o += c
            for b in range(B):
                assert got[b].size == T
                same = _bits(got[b]) == _bits(ref[b])
                assert same.all(), (strength, T, cut, b, int(np.nonzero(~same)[0][0]))
    T = max(TS)
    assert not np.array_equal(_bits(want[strength, T]), _bits(x[:, :T]))  # (the stage did something)
    assert not np.array_equal(_bits(want[2, T]), _bits(want[3, T]))


def test_the_gain_is_the_strengths(eng):
    """A tone on the middle bin of pair 0's even sub-band (a whole number of periods in a frame, so the window spreads
    it over that sub-band's bins only): the stage scales it by g- or g+ of the strength, whichever the table's bit says,
    block by block."""
    T, k = 16 * 1024, A.MARK_K0 + 2
    tone = (0.2 * np.sin(2 * np.pi * k * np.arange(T) / A.FORMANT_N)).astype(np.float32)[None, :]
    words = A.mark_table(KEY, ID)
    for strength in (1, 2, 3):
        got, _ = _run(eng, tone, [1], [T], strength)
        a = 2.0 ** -(7 - strength)
        for blk in (1, 2, 5, 9):  # hop block 4 blk is covered by the block's own four frames alone
            own = slice(blk * 1024, blk * 1024 + 256)
            ratio = np.sqrt((got[0][own].astype(np.float64) ** 2).sum() / (tone[0][own].astype(np.float64) ** 2).sum())
            g = 1.0 - a if int(words[blk]) & 1 else 1.0 + a  # (a set bit: g- on the even sub-band)
            assert abs(ratio - g) < 1e-4, (strength, blk, ratio, g)


def test_the_bits_do_not_depend_on_the_hop_blocks_a_workgroup_writes(eng, x, want, tabs):
    """Option fmt_group, the formant stage's hook: 1 (a workgroup per hop block), groups that do and do not divide the
    call's blocks, the largest; and the launch's own choice where it is no longer 1 (three rows of 352 hop blocks)."""
    T = max(TS)
    try:
        for g in range(1, 33):
            eng.set_option("fmt_group", g)
            for chunks in ([T], _cuts(T, 257) + [0]) if g in (1, 2, 3, 5, 13, 32) else ([T],):
                got, _ = _run(eng, x, SLOTS, chunks)
                for b in range(B):
                    assert np.array_equal(_bits(got[b]), _bits(want[2, T][b])), (g, len(chunks), b)
    finally:
        eng.set_option("fmt_group", 0)
    long = make_x(90000, B, seed=9)  # (more than a period of blocks: the table wraps)
    ref = A.mark_ref(long, KEY, ID, 2, tabs)
    try:
        for g in (0, 7, 32):
            eng.set_option("fmt_group", g)
            got, _ = _run(eng, long, SLOTS, [90000])
            for b in range(B):
                assert np.array_equal(_bits(got[b]), _bits(ref[b])), (g, b)
    finally:
        eng.set_option("fmt_group", 0)


def test_one_row(eng, x, want):
    T = max(TS)
    for chunks in ([T], _cuts(T, 257) + [0]):
        got, _ = _run(eng, x[1:2], [7], chunks)
        assert np.array_equal(_bits(got[0]), _bits(want[2, T][1]))


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
        both, counts = _run(e, v, slots, chunks)
        assert counts == [[(1100 // H - 3) * H] * rows, [n - (1100 // H - 3) * H] * rows]
        y = A.mark_ref(v, KEY, ID, 2, e.pcm_formant_tables())
        for r in range(rows):
            assert np.array_equal(_bits(both[r]), _bits(y[r])), r
        for r in (0, 31, 32):  # of the first launch, its last row, and the row of the second launch: each on its own
            alone, _ = _run(e, v[r:r + 1], [slots[r]], chunks)
            assert np.array_equal(_bits(alone[0]), _bits(both[r])), r
    finally:
        e.close()


def test_silence_in_silence_out(eng):
    z = np.zeros((B, 3000), dtype=np.float32)
    for chunks in ([3000], [1041, 1041, 918]):
        got, _ = _run(eng, z, SLOTS, chunks, 3)
        for b in range(B):
            assert got[b].size == 3000 and not _bits(got[b]).any()  # (+0.0, every bit)


def test_reset_between_segments(eng, x, want):
    T = max(TS)
    xd = torch.from_numpy(np.array(x, dtype=np.float32)).to(eng.device)
    eng.pcm_mark(xd[:, :1700].contiguous(), SLOTS, [False] * B, MS.OTHER_KEY, 1, 1)  # an unfinished sentence, another mark
    for s in SLOTS:
        eng.pcm_reset(s)
    again, counts = _run(eng, x, SLOTS, _cuts(T, 1041))
    assert counts[0] == [(1041 // H - 3) * H] * B
    for b in range(B):
        assert np.array_equal(_bits(again[b]), _bits(want[2, T][b]))


def test_one_mark_per_segment_and_the_state_survives_the_error(eng, x, want):
    from llmvox_amd import _lib
    T = max(TS)
    xd = torch.from_numpy(np.array(x, dtype=np.float32)).to(eng.device)
    out, cnt = eng.pcm_mark(xd[:, :1041].contiguous(), SLOTS, [False] * B, KEY, ID, 2)
    parts = [out.cpu().numpy()[:, :cnt[0]].copy()]
    for other in ((MS.OTHER_KEY, ID, 2), (KEY, ID ^ 1, 2), (KEY, ID, 3)):
        with pytest.raises(_lib.LvxArgError) as ei:
            eng.pcm_mark(xd[:, 1041:T].contiguous(), SLOTS, [True] * B, *other)
        assert ei.value.code == _lib.LVX_E_ARG and "open at another mark" in str(ei.value)
        assert str(KEY) not in str(ei.value) and hex(KEY)[2:] not in str(ei.value).lower()
    out, cnt = eng.pcm_mark(xd[:, 1041:T].contiguous(), SLOTS, [True] * B, KEY, ID, 2)
    parts.append(out.cpu().numpy()[:, :cnt[0]].copy())
    got = np.concatenate(parts, axis=1)
    for b in range(B):
        assert np.array_equal(_bits(got[b]), _bits(want[2, T][b]))
    eng.check_errors()


def test_argument_errors(eng, x):
    from llmvox_amd import _lib
    lib = eng.lib
    xd = torch.from_numpy(x[:, :1600].copy()).to(eng.device)
    out = torch.zeros(B, 4096, dtype=torch.float32, device=eng.device)
    cnt = (ctypes.c_int32 * B)()
    null = object()

    def call(slots=(0, 1, 2), mark_id=ID, strength=2, stride=4096 * 4, n_in=1600, nb=B, optr=None, sl=None, fl=None, cn=None,
             pcm=None, final=0, h=None):
        sl = (ctypes.c_int32 * len(slots))(*slots) if sl is None else None
        fl = (ctypes.c_uint8 * len(slots))(*([final] * len(slots))) if fl is None else None
        return lib.lvx_pcm_mark(eng.h if h is None else None, None if pcm is null else ctypes.c_void_p(xd.data_ptr()), nb, n_in,
                                sl, fl, KEY, mark_id, strength,
                                None if optr is null else ctypes.c_void_p(out.data_ptr() if optr is None else optr), stride,
                                cnt if cn is None else None, eng.stream_handle())

    for s in SLOTS + [0, 1]:
        eng.pcm_reset(s)
    first = (1600 // H - 3) * H
    bad = [dict(mark_id=-1), dict(mark_id=256), dict(strength=0), dict(strength=4), dict(slots=(0, 1, 8)), dict(slots=(0, -1, 2)),
           dict(slots=(0, 1, 0)), dict(stride=first * 4 - 4), dict(stride=0), dict(stride=1600 * 4 - 4, final=1),
           dict(stride=4096 * 4 + 2), dict(stride=-16), dict(optr=out.data_ptr() + 2), dict(optr=null), dict(nb=0), dict(n_in=-1),
           dict(sl=null), dict(fl=null), dict(cn=null), dict(pcm=null), dict(h=null)]
    for kw in bad:
        assert call(**kw) == _lib.LVX_E_ARG, kw
    # none of them moved a slot: the segment still starts here, and a first good call emits a first call's count
    assert call() == 0 and list(cnt) == [first] * B
    assert call(stride=(3200 - first) * 4, final=1) == 0 and list(cnt) == [3200 - first] * B  # (a stride that just fits)
    # the host-only entries
    w = np.zeros(64, dtype=np.uint16)
    p = w.ctypes.data_as(ctypes.c_void_p)
    assert lib.lvx_pcm_mark_table(KEY, 0, p, 63) == _lib.LVX_E_ARG
    assert lib.lvx_pcm_mark_table(KEY, 0, None, 64) == _lib.LVX_E_ARG
    assert lib.lvx_pcm_mark_table(KEY, 256, p, 64) == _lib.LVX_E_ARG
    assert lib.lvx_pcm_mark_table(KEY, -1, p, 64) == _lib.LVX_E_ARG
    assert lib.lvx_pcm_mark_table(KEY, 255, p, 64) == _lib.LVX_OK and w.any() and not (w >> 12).any()
    assert lib.lvx_pcm_mark_emitted(-1, 0, 0) < 0 and lib.lvx_pcm_mark_emitted(0, -1, 0) < 0
    assert lib.lvx_pcm_mark_emitted(1000, 600, 0) == first and lib.lvx_pcm_mark_emitted(1000, 600, 1) == 1600
    with pytest.raises(ValueError):
        eng.pcm_mark(xd, [0, 1], [False, False], KEY)  # rows and slots disagree
    with pytest.raises(ValueError):
        eng.pcm_mark(xd, [0, 1, 2], [False] * 3, -5)
    with pytest.raises(_lib.LvxArgError):
        eng.pcm_mark(xd, [0, 1, 2], [False] * 3, KEY, 0, 7)
    assert call() == 0 and list(cnt) == [first] * B  # (none of them opened a segment)
    for s in (0, 1, 2):
        eng.pcm_reset(s)
    eng.check_errors()


def test_composition_through_pcm_convert(eng):
    """Stretch, ratio, formant, mark, level, rate and encoding in one format, on a two-sentence stream cut into dumps of
    10 and 30 frames, against convert_ref of each sentence and StreamRef call by call, with the library's tables."""
    fmt = A.AudioFormat(pitch_pct=125, formant_pct=100, volume_pct=200, sample_rate=16000, encoding="s16le", mark_key=KEY,
                        mark_id=ID, mark_strength=3)
    assert fmt.stretch_pct == 80 and fmt.ratio == (4, 5) and fmt.formant == (5, 4) and fmt.marks
    kw = dict(taps=eng.pcm_filter(16000)[3], windows=eng.pcm_stretch_window(), ratio_taps=eng.pcm_ratio_filter(4, 5)[1],
              level_win=eng.pcm_level_window(), formant_tabs=eng.pcm_formant_tables())
    dumps = [3200, 9600]
    v = make_x(2 * sum(dumps), B, seed=17)
    xd = torch.from_numpy(v).to(eng.device)
    ref = [A.StreamRef(fmt, **kw) for _ in range(B)]
    plain = A.AudioFormat(pitch_pct=125, formant_pct=100, volume_pct=200, sample_rate=16000, encoding="s16le")
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
            assert not np.array_equal(whole, A.convert_ref(v[b, start:o], plain, **kw))  # (the mark is in it)
    eng.check_errors()


def test_the_mark_on_device_output_is_found(eng, tabs):
    """Three seconds of the synthetic vowel through the device stage at strength 2, then through the harshest delivery
    (8 kHz mu-law, a leading crop): detected, the payload exact; under another key, and unmarked, not."""
    x = MS.vowel()
    got, _ = _run(eng, x[None, :], [4], [x.size])
    assert np.array_equal(_bits(got[0]), _bits(A.mark_ref(x, KEY, ID, 2, tabs)))
    S, found, mark_id, off = A.mark_detect(got[0], 24000, KEY)
    assert found and mark_id == ID and S >= 10.0 and min(off, 1024 - off) <= 128, (S, mark_id, off)
    phone = MS.delivered(got[0], 8000, "ulaw", MS.CROP)
    S, found, mark_id, _ = A.mark_detect(phone, 8000, KEY)
    assert found and mark_id == ID and S >= 10.0, (S, mark_id)
    assert not A.mark_detect(phone, 8000, MS.OTHER_KEY)[1]
    assert not A.mark_detect(MS.delivered(x, 8000, "ulaw", MS.CROP), 8000, KEY)[1]


STAGES = ("pcm_join", "pcm_stretch", "pcm_ratio", "pcm_formant", "pcm_mark", "pcm_level", "_pcm_resample")
J, S_, P, F, M, V, R = STAGES
# per format: the stages each of the two calls of 1,280 samples passes, in order; a format without a key never enters
# the mark stage and makes the calls it made before. Behind the formant stage the mark's first call gets 512 samples
# and hands nothing on, so the stages behind it wait for the second.
PIPELINES = [
    (A.AudioFormat(), [[R], [R]]),
    (A.AudioFormat(mark_id=7, mark_strength=3), [[R], [R]]),
    (A.AudioFormat(volume_pct=250), [[V], [V]]),
    (A.AudioFormat(formant_pct=90), [[F], [F]]),
    (A.AudioFormat(mark_key=KEY), [[M], [M]]),
    (A.AudioFormat(mark_key=0), [[M], [M]]),
    (A.AudioFormat(volume_pct=250, mark_key=KEY), [[M, V], [M, V]]),
    (A.AudioFormat(16000, "s16le", "raw", 100, 100, False, 250, 90, mark_key=KEY), [[F, M], [F, M, V, R]]),
]


def test_a_format_makes_exactly_the_stage_calls_it_needs(eng):
    slots = [2, 0, 3]
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
