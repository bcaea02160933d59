"""The device dump join (lvx_pcm_join, pcm_kernels.hip: pcm_join_kernel) against the rule of include/llmvox.h
("PCM dump join") as llmvox_amd/audio.py states it in numpy (join_ref), with the library's own windows: the
samples as int32 bit patterns over several slots and calls, rows that are not 16-byte aligned, the argument
errors, lvx_pcm_reset, and joined streams on FusedScheduler through the codec."""
import ctypes

import numpy as np
import pytest
import torch

from llmvox_amd import audio as A

pytestmark = pytest.mark.gpu

H = 320
SLOTS = [5, 0, 2, 7, 3]
# per call: frames of every row (n_in is common to a call), per row (slot index, ctx_frames, final), in row order
CALLS = [
    (1, [(0, 0, False), (1, 0, False), (2, 0, False), (3, 0, False), (4, 0, False)]),    # one-frame first dumps: 0 samples
    (18, [(0, 16, False), (1, 0, False), (2, 1, False), (3, 2, True), (4, 16, False)]),  # a final among them
    (3, [(4, 2, False), (2, 0, False), (3, 0, False), (0, 2, False), (1, 1, False)]),    # out of order; slot 3 starts anew
    (17, [(0, 16, True), (1, 2, True), (2, 1, True), (3, 0, False), (4, 0, False)]),
    (0, [(4, 0, True), (3, 0, True), (1, 0, True)]),                                     # flush only; slot 1 is closed
]
SPECIAL = np.array([0.0, -0.0, 1e30, -1e30, 1e-40, -1e-40], dtype=np.float32)


@pytest.fixture(scope="module")
def eng():
    from llmvox_amd.engine import build_engine
    e = build_engine(0, "fp32", "fp32", max_streams=8, max_positions=64, max_codec_frames=64)
    yield e
    e.close()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _rows(rng, n_rows, frames):
    """Normal draws with +-0, +-1e30 and denormals sprinkled in, also over the frames a crossfade and a tail read."""
    v = rng.standard_normal((n_rows, frames * H)).astype(np.float32)
    for b in range(n_rows):
        at = rng.choice(frames * H, size=min(40, frames * H // 4), replace=False)
        v[b, at] = SPECIAL[rng.integers(0, SPECIAL.size, at.size)]
        v[b, -H:-H + 6] = SPECIAL          # the frame that is held back
        if frames > 1:
            v[b, H - 3:H + 3] = SPECIAL    # round the end of a first context frame
    assert np.isfinite(v).all()
    return v


@pytest.fixture(scope="module")
def played(eng):
    """CALLS on the device, once: per slot index its sentences as [[(row, ctx_frames)], ...] and what each call
    gave it, [(samples, count)], in call order."""
    rng = np.random.default_rng(11)
    for s in SLOTS:
        eng.pcm_reset(s)
    sentences = {i: [[]] for i in range(len(SLOTS))}
    got = {i: [] for i in range(len(SLOTS))}
    for frames, rows in CALLS:
        x = _rows(rng, len(rows), frames) if frames else None
        big = None
        if frames:  # the call's rows gathered out of a larger tensor in another order
            pool = torch.from_numpy(np.concatenate([x[::-1], x[:1]])).to(eng.device)
            big = pool[list(range(len(rows) - 1, -1, -1))]
        out, cnt = eng.pcm_join(big, [SLOTS[i] for i, _, _ in rows], [c for _, c, _ in rows], [f for _, _, f in rows])
        host = out.cpu().numpy()
        for b, (i, c, final) in enumerate(rows):
            sentences[i][-1].append((x[b] if frames else np.zeros(0, np.float32), c))
            got[i].append((host[b, :cnt[b]].copy(), cnt[b]))
            if final:
                sentences[i].append([])
    eng.check_errors()
    return sentences, got


def test_windows_are_the_rules(eng):
    wr, wf = eng.pcm_join_window()
    assert np.array_equal(_bits(wr), _bits(A.join_window()[0])) and np.array_equal(_bits(wf), _bits(A.join_window()[1]))


def test_rule_bit_for_bit(eng, played):
    sentences, got = played
    windows = eng.pcm_join_window()
    n_fades = 0
    for i in range(len(SLOTS)):
        assert not sentences[i][-1]  # every slot's last sentence was ended
        want = []
        for sent in sentences[i][:-1]:
            want += A.join_ref([r for r, _ in sent], [c for _, c in sent], windows)
            n_fades += sum(1 for _, c in sent if c)
        assert len(want) == len(got[i])
        for k, (w, (g, n)) in enumerate(zip(want, got[i])):
            assert n == w.size, (i, k)
            assert np.array_equal(_bits(g), _bits(w)), (i, k, int(np.nonzero(_bits(g) != _bits(w))[0][0]))
        for sent in sentences[i][:-1]:  # a sentence of T frames delivers 320 T samples
            T = sum(r.size // H - c for r, c in sent)
            assert sum(y.size for y in A.join_ref([r for r, _ in sent], [c for _, c in sent], windows)) == H * T
    assert n_fades >= 9
    assert got[0][0][1] == 0 and got[3][1][1] == 16 * H + H  # a one-frame first dump; an open slot's final call
    assert got[1][-1][1] == 0 and got[4][-1][1] == H           # the flush of a closed and of an open slot


def test_one_dump_sentence_is_the_row(eng):
    rng = np.random.default_rng(12)
    x = _rows(rng, 2, 5)
    out, cnt = eng.pcm_join(torch.from_numpy(x).to(eng.device), [1, 4], [0, 0], [True, True])
    assert cnt == [5 * H] * 2 and np.array_equal(_bits(out.cpu().numpy()[:, :5 * H]), _bits(x))


def test_rows_that_are_not_16_byte_aligned(eng):
    """pcm_dev, out_dev and the stride multiples of 4 bytes only: the same bits by the scalar path."""
    from llmvox_amd import _lib
    rng = np.random.default_rng(13)
    a, b = _rows(rng, 2, 3), _rows(rng, 2, 4)
    windows = eng.pcm_join_window()
    want = [A.join_ref([a[r], b[r]], [0, 2], windows) for r in range(2)]
    sl, n = (ctypes.c_int32 * 2)(6, 1), (ctypes.c_int32 * 2)()
    stride = 5 * H + 1  # floats
    outd = torch.full((2 * stride + 8,), 7.0, device=eng.device)
    for k, (x, c, final) in enumerate([(a, 0, 0), (b, 2, 1)]):
        xd = torch.zeros(x.size + 8, device=eng.device)
        xd[1:1 + x.size] = torch.from_numpy(x.reshape(-1)).to(eng.device)
        outd.fill_(7.0)
        assert (xd.data_ptr() + 4) % 16 == 4
        rc = eng.lib.lvx_pcm_join(eng.h, ctypes.c_void_p(xd.data_ptr() + 4), 2, x.shape[1], sl, (ctypes.c_int32 * 2)(c, c),
                                  (ctypes.c_uint8 * 2)(final, final), ctypes.c_void_p(outd.data_ptr() + 4), stride * 4, n,
                                  eng.stream_handle())
        assert rc == _lib.LVX_OK
        host = outd.cpu().numpy()
        for r in range(2):
            w = want[r][k]
            assert n[r] == w.size
            g = host[1 + r * stride:1 + r * stride + w.size]
            assert np.array_equal(_bits(g), _bits(w)), (k, r)
            assert host[1 + r * stride + w.size] == 7.0  # nothing behind the row's count
        assert host[0] == 7.0
    eng.check_errors()


def test_33_rows_are_two_launches_of_the_same_rows():
    """One more row than a launch's packet holds, a non-final call and a final one with a context frame: every
    row's bits, the second launch's row 32 among them, are the numpy rule's."""
    from llmvox_amd.engine import build_engine
    e = build_engine(0, "fp32", "fp32", max_streams=40, max_positions=64, max_codec_frames=64)
    try:
        rows = 33
        rng = np.random.default_rng(33)
        a, b = _rows(rng, rows, 2), _rows(rng, rows, 2)
        slots = [(7 * r + 3) % 40 for r in range(rows)]
        assert len(set(slots)) == rows
        windows = e.pcm_join_window()
        got = []
        for x, c, final in [(a, 0, False), (b, 1, True)]:
            out, cnt = e.pcm_join(torch.from_numpy(x).to(e.device), slots, [c] * rows, [final] * rows)
            got.append((out.cpu().numpy(), cnt))
        e.check_errors()
        assert got[0][1] == [H] * rows and got[1][1] == [2 * H] * rows
        for r in range(rows):
            want = A.join_ref([a[r], b[r]], [0, 1], windows)
            for k in range(2):
                assert np.array_equal(_bits(got[k][0][r, :got[k][1][r]]), _bits(want[k])), (r, k)
    finally:
        e.close()


def test_argument_errors_move_no_slot(eng):
    from llmvox_amd import _lib
    rng = np.random.default_rng(14)
    windows = eng.pcm_join_window()
    for s in (0, 1, 2):
        eng.pcm_reset(s)
    first = _rows(rng, 1, 4)
    out, cnt = eng.pcm_join(torch.from_numpy(first).to(eng.device), [0], [0], [False])  # slot 0 open, 1 and 2 closed
    assert cnt == [3 * H]
    x = _rows(rng, 3, 4)
    xd = torch.from_numpy(x).to(eng.device)
    outd = torch.zeros(3, 6 * H, device=eng.device)
    n = (ctypes.c_int32 * 3)()

    def call(slots=(0, 1, 2), ctx=(2, 0, 0), finals=(0, 0, 0), n_in=4 * H, nb=3, stride=6 * H * 4, optr=None, xptr=0):
        return eng.lib.lvx_pcm_join(eng.h, ctypes.c_void_p(xd.data_ptr() if xptr == 0 else xptr), nb, n_in,
                                    (ctypes.c_int32 * len(slots))(*slots), (ctypes.c_int32 * len(ctx))(*ctx),
                                    (ctypes.c_uint8 * len(finals))(*finals),
                                    ctypes.c_void_p(outd.data_ptr() if optr is None else optr), stride, n, eng.stream_handle())

    bad = [dict(n_in=4 * H - 4), dict(n_in=4 * H + 1), dict(n_in=-H), dict(ctx=(17, 0, 0)), dict(ctx=(-1, 0, 0)),
           dict(ctx=(4, 0, 0)), dict(ctx=(3, 0, 0), n_in=3 * H), dict(ctx=(2, 1, 0)), dict(ctx=(2, 0, 16)),
           dict(n_in=0), dict(n_in=0, finals=(1, 1, 0)), dict(n_in=0, finals=(1, 1, 1), ctx=(1, 0, 0)),
           dict(slots=(0, 1, 8)), dict(slots=(0, -1, 2)), dict(slots=(0, 1, 0)), dict(nb=0),
           dict(stride=3 * H * 4 - 4), dict(stride=0), dict(stride=6 * H * 4 + 2), dict(optr=outd.data_ptr() + 2),
           dict(xptr=None)]
    for kw in bad:
        if kw.get("xptr", 0) is None:
            assert eng.lib.lvx_pcm_join(eng.h, None, 3, 4 * H, (ctypes.c_int32 * 3)(0, 1, 2), (ctypes.c_int32 * 3)(2, 0, 0),
                                        (ctypes.c_uint8 * 3)(0, 0, 0), ctypes.c_void_p(outd.data_ptr()), 6 * H * 4, n,
                                        eng.stream_handle()) == _lib.LVX_E_ARG
        else:
            assert call(**kw) == _lib.LVX_E_ARG, kw
    # none of them moved a slot: the next valid call gives what it gives without them
    assert call() == _lib.LVX_OK and list(n) == [4 * H - 2 * H, 3 * H, 3 * H]
    host = outd.cpu().numpy()
    want0 = A.join_ref([first[0], x[0], np.zeros(0, np.float32)], [0, 2, 0], windows)[1]
    assert np.array_equal(_bits(host[0, :n[0]]), _bits(want0))
    for r in (1, 2):
        assert np.array_equal(_bits(host[r, :n[r]]), _bits(x[r, :3 * H]))
    with pytest.raises(ValueError):
        eng.pcm_join(xd, [0, 1], [0, 0], [False, False])  # rows and slots disagree
    with pytest.raises(ValueError):
        eng.pcm_convert(xd, [0, 1, 2], [False] * 3, A.AudioFormat(16000), ctx_frames=[1, 0, 0])  # context without join
    for s in (0, 1, 2):
        eng.pcm_reset(s)
    eng.check_errors()


def test_reset_closes_the_segment(eng):
    from llmvox_amd import _lib
    rng = np.random.default_rng(15)
    x = _rows(rng, 1, 3)
    xd = torch.from_numpy(x).to(eng.device)
    eng.pcm_reset(6)
    assert eng.pcm_join(xd, [6], [0], [False])[1] == [2 * H]
    assert eng.pcm_join(xd, [6], [1], [False])[1] == [2 * H]  # open: context is welcome, the head comes first
    eng.pcm_reset(6)
    with pytest.raises(_lib.LvxArgError):
        eng.pcm_join(xd, [6], [1], [False])                     # closed: no context
    out, cnt = eng.pcm_join(xd, [6], [0], [True])
    assert cnt == [3 * H] and np.array_equal(_bits(out.cpu().numpy()[0, :3 * H]), _bits(x[0]))  # and no held-back frame
    assert eng.pcm_join(None, [6], [0], [True])[1] == [0]
    eng.check_errors()


# ---- through the codec -----------------------------------------------------------------------------

TEXT = ("The quick brown fox jumps over the lazy dog and then it sleeps near the river bank for a long while "
        "until the evening comes and the wind turns cold and the little boats return to the harbour one by one")
assert len(TEXT) >= 190  # (one decode step per character: enough for dumps of 10, 30 and 90 and a tail)


@pytest.fixture(scope="module")
def sched_eng():
    from llmvox_amd.engine import build_engine
    e = build_engine(0, "fp32", "fp32", max_streams=4, max_positions=256, max_codec_frames=640)
    yield e
    e.close()


def _speak(eng, audios, n_tokens, overlap, dump_sizes=None):
    """Synthetic weights never end a sentence: each stream speaks one, ended by its tail as the service ends a
    request. Per stream: (its tokens, its items)."""
    from llmvox_amd.streaming import FusedScheduler
    sch = FusedScheduler(eng, max_chunk=16, to_bytes=True, overlap=overlap,
                         stop_rule=lambda st, ntok, pos: ntok >= n_tokens)
    sts = []
    for i, fmt in enumerate(audios):
        st = sch.open_stream(index=i, dump_size=(dump_sizes or [10] * len(audios))[i], **({} if fmt is None else {"audio": fmt}))
        for w in TEXT.split(" "):
            st.feed(w)
        sts.append(st)
    assert sch.run_until_idle(max_chunks=500) > 0
    for st in sts:
        toks, st.m.speech_outputs = st.m.speech_outputs, []
        if toks or st.pcm_open:
            sch.queue_tail(st, toks)
    sch.flush()
    out = [(list(st.tokens), [e for e in st.events if isinstance(e, bytes)]) for st in sts]
    for st in sts:
        sch.close_stream(st)
    sch.close()
    eng.check_errors()
    return out


def _context_rows(eng, tokens, cut):
    """The codec's rendering of each dump's context-plus-token row (one call per row, as the scheduler's), and
    the context counts."""
    rows, ctx, at = [], [], 0
    for L in cut:
        c = min(16, at, eng.max_codec_frames - L)
        codes = torch.tensor([tokens[at - c:at + L]], dtype=torch.int32, device=eng.device)
        rows.append(eng.decode_codes(codes).cpu().numpy()[0])
        ctx.append(c)
        at += L
    return rows, ctx


@pytest.mark.parametrize("overlap", [False, True], ids=["serial", "overlap"])
def test_joined_stream_through_the_codec(sched_eng, overlap):
    """Dumps of 10 / 30 / 90 and a short last one: the delivered bytes are join_ref over engine.decode_codes of
    the same context-plus-token rows; with speed 1.3 at 16 kHz s16le, StreamRef's over the same rows."""
    from test_gpu_pcm_out import _lib_taps
    eng = sched_eng
    fmt2 = A.AudioFormat(16000, "s16le", speed_pct=130, join=True)
    ((tok, items),) = _speak(eng, [A.AudioFormat(join=True)], 135, overlap)
    N = len(tok)
    assert 130 < N < 200
    cut = [10, 30, 90, N - 130]
    rows, ctx = _context_rows(eng, tok, cut)
    assert ctx == [0, 10, 16, 16]
    want = A.join_ref(rows, ctx, eng.pcm_join_window())
    assert len(items) == 4 and [len(b) // 4 for b in items] == [9 * H, 30 * H, 90 * H, (N - 129) * H]
    for k, (b, w) in enumerate(zip(items, want)):
        assert np.array_equal(np.frombuffer(b, dtype="<i4"), _bits(w)), k
    # the seams are not those of plain concatenation
    plain = np.concatenate([eng.decode_codes(torch.tensor([tok[a:a + L]], dtype=torch.int32, device=eng.device)).cpu().numpy()[0]
                            for a, L in zip([0, 10, 40, 130], cut)])
    joined = np.frombuffer(b"".join(items), dtype="<f4")
    assert joined.size == plain.size == N * H and np.array_equal(joined[:9 * H], plain[:9 * H])
    for seam in (10, 40, 130):
        assert not np.array_equal(joined[(seam - 1) * H:(seam + 1) * H], plain[(seam - 1) * H:(seam + 1) * H])

    ((tok2, items2),) = _speak(eng, [fmt2], 135, overlap)
    assert tok2 == tok
    ref = A.StreamRef(fmt2, taps=_lib_taps(16000), windows=eng.pcm_stretch_window(), join_windows=eng.pcm_join_window())
    want2 = [ref.push(r, k == 3, ctx_frames=c) for k, (r, c) in enumerate(zip(rows, ctx))]
    assert len(items2) == 4
    for k, (b, w) in enumerate(zip(items2, want2)):
        assert w.dtype == np.int16 and np.array_equal(np.frombuffer(b, dtype="<i2"), w), k
    n1 = -(-N * H * 100 // 130)
    assert sum(len(b) for b in items2) // 2 == -(-n1 * 2 // 3)


def test_plain_stream_beside_a_joined_one(sched_eng):
    """A default stream and a 16 kHz stream without ``join`` deliver, beside a joined stream, the bytes of the run
    in which that third stream is not joined. The third stream dumps 7 / 21 / 63, so that its codec rows (7, 28,
    79 frames joined) never share a call with the others' (10 / 30 / 90) in either run: the codec's rows are
    independent, but a batched call equals single ones to 1e-6 only (test_gpu_parity), not bit for bit."""
    eng = sched_eng
    p16 = A.AudioFormat(16000, "s16le")
    sizes = [10, 10, 7]
    with_join = _speak(eng, [None, p16, A.AudioFormat(join=True)], 135, True, sizes)
    without = _speak(eng, [None, p16, None], 135, True, sizes)
    for k in range(3):
        assert with_join[k][0] == without[k][0]  # the same tokens
    assert with_join[0][1] == without[0][1] and with_join[1][1] == without[1][1]
    a, b = b"".join(with_join[2][1]), b"".join(without[2][1])
    assert len(a) == len(b) and a != b and a[:6 * H * 4] == b[:6 * H * 4]
