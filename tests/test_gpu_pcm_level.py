"""The device level stage of the volume control (lvx_pcm_level, pcm_kernels.hip: pcm_level_kernel) against the rule
of include/llmvox.h ("PCM level") as llmvox_amd/audio.py states it in numpy (``level_ref``), with the library's own
window: samples and gains bit for bit at four volumes, chunked = one-shot, the per-call counts, flush-only calls,
segments shorter than the hold-back, row independence (33 rows: two launches), the volume-100 bypass, lvx_pcm_reset,
one volume per segment, the argument errors, a NaN sample, the composition through Engine.pcm_convert with every
other stage, and a loud stream beside a default one on FusedScheduler(overlap=True)."""
import ctypes
import dataclasses

import numpy as np
import pytest
import torch

from llmvox_amd import audio as A

pytestmark = pytest.mark.gpu

CHUNKS = [3200, 320, 50, 1, 1909, 320]  # the last one final; one shorter than the 1600-sample history, one of one
T = sum(CHUNKS)                         # sample, one (1909) across the 1024-output block edge
B = 3
SLOTS = [5, 0, 2]
VOLUMES = (0, 50, 250, 400)
HOLD = 2 * A.LEVEL_A


@pytest.fixture(scope="module")
def eng():
    from llmvox_amd.engine import build_engine
    e = build_engine(0, "fp32", "fp32", max_streams=8, max_positions=64, max_codec_frames=64)
    yield e
    e.close()


def make_x():
    """Per row: seven harmonics (periods 96 / 150 / 123) plus uniform noise under an amplitude ramp, quiet enough
    that volume 250 leaves it alone, a louder stretch that does not (across a chunk edge), a run of exact zeros
    across a chunk edge, and isolated samples beyond +-1, one at index 0 and one at T - 1."""
    rng = np.random.default_rng(29)
    t = np.arange(T, dtype=np.float64)
    v = np.zeros((B, T), dtype=np.float32)
    for b, P in enumerate([96, 150, 123]):
        tone = 0.07 * sum(np.sin(2 * np.pi * h * t / P) / h for h in range(1, 8))
        v[b] = (tone + rng.uniform(-1, 1, T) * np.linspace(0.0, 0.12, T)).astype(np.float32)
    v[0, 2900:3300] *= 5.0  # (across the first chunk's edge)
    v[1, 3540:3600] *= 6.0  # (across the edge between the third and the one-sample chunk)
    v[2, 4300:4700] *= 4.0
    v[0, 1500:1900] = 0.0
    v[1, 0:400] = 0.0
    v[2, 3100:3500] = 0.0   # (across the first chunk's edge)
    v[0, [0, T - 1]] = [1.5, -1.25]
    v[1, [4479, 4480]] = [3.0, -1.0]
    v[2, [100, 101]] = [1.5, -1.5]
    return v


@pytest.fixture(scope="module")
def x():
    return make_x()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _run(eng, x, slots, chunks, pct, finals=None):
    """The level calls of one segment per row: (per row the samples, per row the gains, per call the counts)."""
    xd = torch.from_numpy(np.ascontiguousarray(x)).to(eng.device)
    n = len(slots)
    parts, gains, counts, o = [[] for _ in slots], [[] for _ in slots], [], 0
    for k, c in enumerate(chunks):
        fin = [k == len(chunks) - 1] * n if finals is None else finals[k]
        out, cnt, g = eng.pcm_level(xd[:, o:o + c].contiguous() if c else None, slots, fin, pct, want_g=True)
        host, ghost = out.cpu().numpy(), g.cpu().numpy()
        for b in range(n):
            parts[b].append(host[b, :cnt[b]].copy())
            gains[b].append(ghost[b, :cnt[b]].copy())
        counts.append(cnt)
        o += c
    eng.check_errors()
    return [np.concatenate(p) for p in parts], [np.concatenate(p) for p in gains], counts


@pytest.fixture(scope="module")
def win(eng):
    return eng.pcm_level_window()


@pytest.fixture(scope="module")
def want(x, win):
    """The numpy rule at every volume (computed once, shared, never written to)."""
    out = {pct: A.level_ref(x, pct, win) for pct in VOLUMES}
    for y, g in out.values():
        y.setflags(write=False)
        g.setflags(write=False)
    return out


@pytest.fixture(scope="module")
def one_shot(eng, x):
    return {pct: _run(eng, x, SLOTS, [T], pct)[:2] for pct in VOLUMES}


def test_the_library_window_is_the_rules(win):
    assert win.shape == (241,) and np.array_equal(win, win[::-1])
    assert abs(win.astype(np.float64).sum() - 1.0) < 1e-6
    # (both round a double that may differ in its last place: at most one fp32 step apart)
    assert np.abs(win.astype(np.float64) - A.level_window().astype(np.float64)).max() <= float(np.spacing(win.max()))


def test_the_signal_is_partly_limited(want):
    """At volume 250 between 20 % and 80 % of the samples have g < 1: neither all transparent nor all limited."""
    g = want[250][1]
    share = float((g < 1).mean())
    rows = [float((g[b] < 1).mean()) for b in range(B)]
    print(f"share of g < 1 at volume 250: {share:.3f} (rows {rows})")
    assert 0.2 <= share <= 0.8 and all(0.2 <= r <= 0.8 for r in rows)


@pytest.mark.parametrize("pct", VOLUMES)
def test_rule_bit_for_bit(want, one_shot, pct):
    y, g = want[pct]
    got, gg = one_shot[pct]
    for b in range(B):
        assert got[b].size == gg[b].size == T
        assert np.array_equal(_bits(gg[b]), _bits(g[b])), (pct, b, int(np.nonzero(_bits(gg[b]) != _bits(g[b]))[0][0]))
        assert np.array_equal(_bits(got[b]), _bits(y[b])), (pct, b, int(np.nonzero(_bits(got[b]) != _bits(y[b]))[0][0]))
    c = float(A.LEVEL_CEIL)
    assert max(float(np.abs(r).max()) for r in got) <= c * (1 + 2.0 ** -22)


@pytest.mark.parametrize("pct", VOLUMES)
def test_chunked_equals_one_shot(eng, x, one_shot, pct):
    got, gg, counts = _run(eng, x, SLOTS, CHUNKS, pct)
    o = 0
    for k, c in enumerate(CHUNKS):
        n = eng.lib.lvx_pcm_level_emitted(pct, o, c, int(k == len(CHUNKS) - 1))
        assert counts[k] == [n] * B and n == A.level_emitted(pct, o, c, k == len(CHUNKS) - 1)
        o += c
    assert counts[0] == [3200 - HOLD] * B and counts[-1] == [320 + HOLD] * B
    for b in range(B):
        assert np.array_equal(_bits(got[b]), _bits(one_shot[pct][0][b])), (pct, b)
        assert np.array_equal(_bits(gg[b]), _bits(one_shot[pct][1][b])), (pct, b)


def test_flush_only_emits_the_held_back_samples(eng, x, one_shot):
    n = len(CHUNKS)
    got, gg, counts = _run(eng, x, SLOTS, CHUNKS + [0], 250, finals=[[False] * B] * n + [[True] * B])
    assert counts[-1] == [HOLD] * B and sum(c[0] for c in counts[:-1]) == T - HOLD
    for b in range(B):
        assert np.array_equal(_bits(got[b]), _bits(one_shot[250][0][b]))
        assert np.array_equal(_bits(gg[b]), _bits(one_shot[250][1][b]))
    # a flush with nothing behind it emits nothing (the slots were reset by the final call)
    _, cnt, _ = eng.pcm_level(None, SLOTS, [True] * B, 250)
    assert cnt == [0] * B
    # a non-final call without inputs changes nothing
    _, cnt, _ = eng.pcm_level(None, SLOTS, [False] * B, 250)
    assert cnt == [0] * B
    for s in SLOTS:
        eng.pcm_reset(s)


def test_a_segment_shorter_than_the_hold_back(eng, x, win):
    """Fewer than 2 A inputs: nothing until the final call, which emits them all."""
    seg = x[:, 2900:2900 + 199]
    got, gg, counts = _run(eng, seg, SLOTS, [100, 99, 0], 400, finals=[[False] * B, [False] * B, [True] * B])
    assert counts == [[0] * B, [0] * B, [199] * B]
    y, g = A.level_ref(seg, 400, win)
    for b in range(B):
        assert np.array_equal(_bits(got[b]), _bits(y[b])) and np.array_equal(_bits(gg[b]), _bits(g[b]))
    # the hold-back is reached inside the second call
    got, _, counts = _run(eng, x[:, :400], SLOTS, [200, 100, 100], 400)
    assert counts == [[0] * B, [60] * B, [340] * B]
    y, _ = A.level_ref(x[:, :400], 400, win)
    for b in range(B):
        assert np.array_equal(_bits(got[b]), _bits(y[b]))


def test_rows_do_not_depend_on_their_neighbours(eng, x, one_shot):
    want_y, want_g = one_shot[250]
    alone, ga, _ = _run(eng, x[1:2], [7], CHUNKS, 250)  # another slot, no other row
    assert np.array_equal(_bits(alone[0]), _bits(want_y[1])) and np.array_equal(_bits(ga[0]), _bits(want_g[1]))
    rev, _, _ = _run(eng, x[::-1], [1, 3, 4], CHUNKS, 250)  # other slots, other row order
    for b in range(B):
        assert np.array_equal(_bits(rev[B - 1 - b]), _bits(want_y[b]))
    # rows whose segments stand at different positions share the later launches
    xd = torch.from_numpy(x).to(eng.device)
    out0, c0, _ = eng.pcm_level(xd[0:1, :3200].contiguous(), [6], [False], 250)
    parts = [out0.cpu().numpy()[0, :c0[0]].copy()]
    o = 3200
    for k, c in enumerate(CHUNKS[1:]):
        last = k == len(CHUNKS) - 2
        # slot 6 continues row 0 while slot 3 starts row 2's segment from its beginning with the same columns
        pcm = torch.stack([xd[0, o:o + c], xd[2, o - 3200:o - 3200 + c]]).contiguous()
        out, cnt, _ = eng.pcm_level(pcm, [6, 3], [last, last], 250)
        parts.append(out.cpu().numpy()[0, :cnt[0]].copy())
        o += c
    eng.check_errors()
    assert np.array_equal(_bits(np.concatenate(parts)), _bits(want_y[0]))


def test_33_rows_are_two_launches_of_the_same_rows():
    """One more row than a launch's packet holds: every row's bits are those of the rule for the row alone."""
    from llmvox_amd.engine import build_engine
    e = build_engine(0, "fp32", "fp32", max_streams=40, max_positions=64, max_codec_frames=64)
    try:
        n, rows = 1500, 33
        rng = np.random.default_rng(33)
        v = (rng.uniform(-1, 1, (rows, n)) * rng.uniform(0.05, 0.5, (rows, 1))).astype(np.float32)
        slots = [(7 * r + 3) % 40 for r in range(rows)]
        assert len(set(slots)) == rows
        chunks = [1100, 400]
        both, gains, counts = _run(e, v, slots, chunks, 250)
        assert counts == [[1100 - HOLD] * rows, [400 + HOLD] * rows]
        y, g = A.level_ref(v, 250, e.pcm_level_window())
        assert 0 < float((g < 1).mean()) < 1
        for r in range(rows):
            assert np.array_equal(_bits(both[r]), _bits(y[r])), r
            assert np.array_equal(_bits(gains[r]), _bits(g[r])), r
        alone, _, _ = _run(e, v[32:33], [slots[32]], chunks, 250)  # the row of the second launch, on its own
        assert np.array_equal(_bits(alone[0]), _bits(both[32]))
    finally:
        e.close()


def test_volume_100_is_a_bypass(eng, x):
    from llmvox_amd import _lib
    xd = torch.from_numpy(x).to(eng.device)
    out, cnt, g = eng.pcm_level(xd, SLOTS, [True] * B, 100, want_g=True)
    assert cnt == [T] * B and out.data_ptr() == xd.data_ptr() and g is None
    out, cnt = eng.pcm_convert(xd, SLOTS, [True] * B, A.AudioFormat(24000, "f32le", "raw", 100, 100, False, 100))
    assert cnt == [T] * B and out.data_ptr() == xd.data_ptr()
    # the library: nothing launched, nothing written
    guard = torch.full((B, 64), 7.0, device=eng.device)
    n = (ctypes.c_int32 * B)()
    sl, fl = (ctypes.c_int32 * B)(*SLOTS), (ctypes.c_uint8 * B)(0, 0, 0)
    assert eng.lib.lvx_pcm_level(eng.h, ctypes.c_void_p(xd.data_ptr()), B, T, sl, fl, 100, ctypes.c_void_p(guard.data_ptr()),
                                 256, n, ctypes.c_void_p(guard.data_ptr()), 256, eng.stream_handle()) == _lib.LVX_OK
    assert list(n) == [T] * B and bool((guard == 7.0).all())
    assert eng.lib.lvx_pcm_level(eng.h, ctypes.c_void_p(xd.data_ptr()), B, T, sl, fl, 100, None, 0, n, None, 0,
                                 eng.stream_handle()) == _lib.LVX_OK
    assert eng.lib.lvx_pcm_level_emitted(100, 17, 123, 0) == 123
    # a format at volume 100 makes the calls, and gets the bytes, of the same format without the field
    for args in [(16000, "s16le", "raw", 100, 100, False), (8000, "f32le", "raw", 130, 90, False),
                 (24000, "s16le", "raw", 77, 100, False)]:
        a, ca = eng.pcm_convert(xd, SLOTS, [True] * B, A.AudioFormat(*args, 100))
        b, cb = eng.pcm_convert(xd, SLOTS, [True] * B, A.AudioFormat(*args))
        assert ca == cb and a.dtype == b.dtype and torch.equal(a[:, :ca[0]], b[:, :cb[0]])
    eng.check_errors()


def test_reset_between_segments(eng, x, one_shot):
    xd = torch.from_numpy(x).to(eng.device)
    eng.pcm_level(xd[:, :1700].contiguous(), SLOTS, [False] * B, 400)  # an unfinished segment at another volume
    for s in SLOTS:
        eng.pcm_reset(s)
    again, gg, counts = _run(eng, x, SLOTS, CHUNKS, 250)
    assert counts[0] == [3200 - HOLD] * B
    for b in range(B):
        assert np.array_equal(_bits(again[b]), _bits(one_shot[250][0][b]))
        assert np.array_equal(_bits(gg[b]), _bits(one_shot[250][1][b]))


def test_one_volume_per_segment_and_the_state_survives_the_error(eng, x, one_shot):
    from llmvox_amd import _lib
    xd = torch.from_numpy(x).to(eng.device)
    out, cnt, _ = eng.pcm_level(xd[:, :3200].contiguous(), SLOTS, [False] * B, 250)
    parts = [out.cpu().numpy()[:, :cnt[0]].copy()]
    for other in (400, 100, 0):
        with pytest.raises(_lib.LvxArgError):
            eng.pcm_level(xd[:, 3200:3520].contiguous(), SLOTS, [False] * B, other)
    # slot 0 alone stands in that segment: a call that names it beside fresh slots moves none of them
    with pytest.raises(_lib.LvxArgError):
        eng.pcm_level(xd[:, :320].contiguous(), [3, 0, 4], [False] * B, 400)
    _, cnt, _ = eng.pcm_level(xd[:, :320].contiguous(), [3, 4, 6], [False] * B, 400)
    assert cnt == [320 - HOLD] * B
    for s in (3, 4, 6):
        eng.pcm_reset(s)
    o = 3200
    for k, c in enumerate(CHUNKS[1:]):
        out, cnt, _ = eng.pcm_level(xd[:, o:o + c].contiguous(), SLOTS, [k == len(CHUNKS) - 2] * B, 250)
        parts.append(out.cpu().numpy()[:, :cnt[0]].copy())
        o += c
    got = np.concatenate(parts, axis=1)
    for b in range(B):
        assert np.array_equal(_bits(got[b]), _bits(one_shot[250][0][b]))
    eng.check_errors()


def test_argument_errors(eng, x):
    from llmvox_amd import _lib
    lib = eng.lib
    xd = torch.from_numpy(x[:, :1600].copy()).to(eng.device)
    out = torch.zeros(B, 4096, dtype=torch.float32, device=eng.device)
    gout = torch.zeros(B, 4096, dtype=torch.float32, device=eng.device)
    cnt = (ctypes.c_int32 * B)()
    null = object()

    def call(slots=(0, 1, 2), pct=250, stride=4096 * 4, n_in=1600, nb=B, optr=None, gptr=None, gstride=4096 * 4,
             sl=None, fl=None, cn=None, pcm=None):
        sl = (ctypes.c_int32 * len(slots))(*slots) if sl is None else None
        fl = (ctypes.c_uint8 * len(slots))(*([0] * len(slots))) if fl is None else None
        return lib.lvx_pcm_level(eng.h, None if pcm is null else ctypes.c_void_p(xd.data_ptr()), nb, n_in, sl, fl, pct,
                                 None if optr is null else ctypes.c_void_p(out.data_ptr() if optr is None else optr), stride,
                                 cnt if cn is None else None,
                                 None if gptr is null else ctypes.c_void_p(gout.data_ptr() if gptr is None else gptr),
                                 gstride, eng.stream_handle())

    for s in SLOTS + [0, 1]:
        eng.pcm_reset(s)
    first = 1600 - HOLD
    bad = [dict(pct=-1), dict(pct=401), dict(slots=(0, 1, 8)), dict(slots=(0, -1, 2)), dict(slots=(0, 1, 0)),
           dict(stride=first * 4 - 4), dict(stride=0), dict(stride=4096 * 4 + 2), dict(stride=-16),
           dict(optr=out.data_ptr() + 2), dict(optr=null), dict(gstride=first * 4 - 4), dict(gstride=4096 * 4 + 2),
           dict(gptr=gout.data_ptr() + 2), dict(nb=0), dict(n_in=-1), dict(sl=null), dict(fl=null), dict(cn=null),
           dict(pcm=null)]
    for kw in bad:
        assert call(**kw) == _lib.LVX_E_ARG, kw
    assert lib.lvx_pcm_level(None, ctypes.c_void_p(xd.data_ptr()), B, 1600, (ctypes.c_int32 * B)(0, 1, 2),
                             (ctypes.c_uint8 * B)(), 250, ctypes.c_void_p(out.data_ptr()), 4096 * 4, cnt, None, 0,
                             eng.stream_handle()) == _lib.LVX_E_ARG
    # none of them moved a slot: the segment still starts here, and a first good call emits a first call's count
    assert call() == 0 and list(cnt) == [first] * B
    assert call(gptr=null, gstride=0) == 0 and list(cnt) == [1600] * B  # (the gains are optional)
    for s in (0, 1, 2):
        eng.pcm_reset(s)
    # the host-only entries
    w = np.zeros(241, dtype=np.float32)
    assert lib.lvx_pcm_level_window(None, 241) == _lib.LVX_E_ARG
    assert lib.lvx_pcm_level_window(w.ctypes.data_as(ctypes.c_void_p), 240) == _lib.LVX_E_ARG
    assert lib.lvx_pcm_level_window(w.ctypes.data_as(ctypes.c_void_p), 241) == _lib.LVX_OK and w[120] == w.max() > 0
    for args in [(-1, 0, 10, 0), (401, 0, 10, 0), (250, -1, 10, 0), (250, 0, -1, 0)]:
        assert lib.lvx_pcm_level_emitted(*args) < 0, args
    assert lib.lvx_pcm_level_emitted(250, 0, 100, 0) == 0 and lib.lvx_pcm_level_emitted(250, 0, 100, 1) == 100
    assert lib.lvx_pcm_level_emitted(250, 100, 200, 0) == 60 and lib.lvx_pcm_level_emitted(250, 300, 0, 1) == HOLD
    with pytest.raises(ValueError):
        eng.pcm_level(xd, [0, 1], [False, False], 250)  # rows and slots disagree
    with pytest.raises(ValueError):
        eng.pcm_level(xd, [0, 1, 2], [False] * 3, 500)
    assert call() == 0 and list(cnt) == [first] * B  # (neither opened a segment)
    for s in (0, 1, 2):
        eng.pcm_reset(s)
    eng.check_errors()


def test_a_nan_sample_passes_and_leaves_its_neighbours_alone(eng, x, win):
    v = x[:, :2600].copy()
    v[0, 1300] = np.nan
    v[1, 2599] = np.nan
    v[2, 0] = np.nan
    got, gg, _ = _run(eng, v, SLOTS, [1100, 1500], 250)
    y, g = A.level_ref(v, 250, win)
    for b, i in ((0, 1300), (1, 2599), (2, 0)):
        assert np.isnan(got[b][i]) and np.isnan(y[b, i]) and int(np.isnan(got[b]).sum()) == 1
    for b in range(B):
        assert np.array_equal(_bits(gg[b]), _bits(g[b])), b
        keep = ~np.isnan(y[b])
        assert np.array_equal(_bits(got[b][keep]), _bits(y[b][keep])), b


def test_composition_through_pcm_convert(eng, x):
    """Join, stretch, ratio, level, rate and encoding in one format: three dumps with context frames, against StreamRef
    with the library's tables. Row 0's loud stretch at three times its level would pass the ceiling by far; with the
    stage it stays under it, but for the little the rate conversion behind the stage may add."""
    fmt = A.AudioFormat(16000, "s16le", "raw", 130, 90, True, 300)
    tables = (eng.pcm_filter(16000)[3], eng.pcm_stretch_window(), eng.pcm_ratio_filter(*fmt.ratio)[1],
              eng.pcm_join_window(), eng.pcm_level_window())
    ref = [A.StreamRef(fmt, *tables) for _ in range(B)]
    quiet = A.StreamRef(dataclasses.replace(fmt, volume_pct=100), *tables)
    dumps = [(0, 3200, 0), (3200 - 2 * 320, 5120, 2), (5120 - 320, 5760, 1)]  # (start with context, end, context frames)
    xd = torch.from_numpy(x).to(eng.device)
    peak = unlimited = 0
    for k, (a, e, c) in enumerate(dumps):
        final = k == len(dumps) - 1
        out, cnt = eng.pcm_convert(xd[:, a:e].contiguous(), SLOTS, [final] * B, fmt, ctx_frames=[c] * B)
        host = out.cpu().numpy()
        assert host.dtype == np.int16
        for b in range(B):
            want = ref[b].push(x[b, a:e], final, c)
            assert cnt[b] == want.size and np.array_equal(host[b, :cnt[b]], want), (k, b)
        peak = max(peak, int(np.abs(host[0, :cnt[0]].astype(np.int32)).max()))
        unlimited = max(unlimited, 3 * int(np.abs(quiet.push(x[0, a:e], final, c).astype(np.int32)).max()))
    ceil16 = 32768 * float(A.LEVEL_CEIL)
    print(f"row 0: peak {peak}, three times the peak at volume 100 {unlimited}, the ceiling {ceil16:.0f}")
    assert unlimited > 1.5 * ceil16 and peak <= 1.1 * ceil16
    eng.check_errors()


@pytest.fixture(scope="module")
def sched_eng():
    from llmvox_amd.engine import build_engine
    e = build_engine(0, "fp32", "fp32", max_streams=4, max_positions=256, max_codec_frames=640)
    yield e
    e.close()


def test_scheduler_end_to_end(sched_eng):
    """A volume-300 stream beside a default one on FusedScheduler(overlap=True), same text and slot layout as a run of
    two default streams: the loud stream's sentence is the rule applied to the f32 sentence of the same tokens, and the
    default stream beside it delivers the bytes it always did."""
    from test_gpu_pcm_out import _speak
    fmt = A.AudioFormat(volume_pct=300)
    (tok_a, plain), (tok_b, loud) = _speak(sched_eng, [None, fmt], 100)
    (tok_c, alone), (tok_d, other) = _speak(sched_eng, [None, None], 100)
    assert tok_a == tok_c and tok_b == tok_d and len(plain) >= 3
    assert plain == alone  # the default stream's bytes do not know about its neighbour's volume
    xs = np.frombuffer(b"".join(other), dtype="<f4")  # the f32 samples of the loud stream's own tokens
    assert xs.size == 320 * len(tok_d)
    got = np.frombuffer(b"".join(loud), dtype="<f4")
    want = A.convert_ref(xs, fmt, level_win=sched_eng.pcm_level_window())
    assert got.size == want.size == xs.size and np.array_equal(_bits(got), _bits(want))
    assert not np.array_equal(_bits(got), _bits(xs))


STAGES = ("pcm_join", "pcm_stretch", "pcm_ratio", "pcm_level", "_pcm_resample")
J, S, P, V, R = STAGES
# per format: the stages each of the two calls passes, in order (every one with all three slots). In the last format
# the first call's join hands 320 samples on, fewer than the stretch's first hop needs: nothing passes the stretch
# and the stages behind it are not called.
PIPELINES = [
    (A.AudioFormat(), [[R], [R]]),
    (A.AudioFormat(16000, "s16le"), [[R], [R]]),
    (A.AudioFormat(speed_pct=130), [[S], [S]]),
    (A.AudioFormat(pitch_pct=90), [[S, P], [S, P]]),
    (A.AudioFormat(volume_pct=250), [[V], [V]]),
    (A.AudioFormat(join=True), [[J], [J]]),
    (A.AudioFormat(8000, "s16le", "raw", 130, 90, True, 250), [[J, S], [J, S, P, V, R]]),
]


def test_a_format_makes_exactly_the_stage_calls_it_needs(sched_eng):
    """Engine.pcm_convert with every stage of the engine recorded: per format and call the sequence of (stage, slots).
    A format that does not use a stage never enters it, and the rate / encoding stage runs after another stage only
    where the format is not 24 kHz f32le."""
    eng, slots = sched_eng, [2, 0, 3]
    log = []

    def recorder(name, inner):
        def call(pcm, slots, *args, **kwargs):
            log.append((name, [int(s) for s in slots]))
            return inner(pcm, slots, *args, **kwargs)
        return call

    xd = torch.from_numpy(make_x()[:, :1280].copy()).to(eng.device)
    try:
        for name in STAGES:
            setattr(eng, name, recorder(name, getattr(eng, name)))
        for fmt, want in PIPELINES:
            for k in range(2):
                del log[:]
                eng.pcm_convert(xd[:, 640 * k:640 * (k + 1)].contiguous(), slots, [k == 1] * B, fmt)
                assert log == [(name, slots) for name in want[k]], (fmt, k, log)
        eng.check_errors()
    finally:
        for name in STAGES:
            eng.__dict__.pop(name, None)
        for s in slots:
            eng.pcm_reset(s)
