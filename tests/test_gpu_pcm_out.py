"""The device PCM output stage (lvx_pcm_convert, pcm_kernels.hip) against the rule of include/llmvox.h as
llmvox_amd/audio.py states it in numpy: chunked = one-shot bit for bit, the fp32 accumulation bound against
a float64 evaluation with the library's own taps, s16 = quantise(f32), row independence, flush-only
calls, the argument errors, and a converted stream beside a default one on FusedScheduler(overlap=True)."""
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
RESAMPLED = [16000, 8000, 48000]
TAPS_PER_OUTPUT = {16000: 73, 8000: 145, 48000: 49}


@pytest.fixture(scope="module")
def eng():
    from llmvox_amd.engine import build_engine
    e = build_engine(0, "fp32", "fp32", max_streams=8, max_positions=64, max_codec_frames=64)
    yield e
    e.close()


@pytest.fixture(scope="module")
def x():
    """Uniform in [-1, 1], with a few samples at +-1 and beyond (at the chunks' edges too)."""
    v = np.random.default_rng(11).uniform(-1, 1, (B, T)).astype(np.float32)
    v[0, [0, 1, 3199, 3200, 3519, 3520, T - 1]] = [1.0, -1.0, 1.5, -2.0, 1.0, -1.0, 1.25]
    v[1, [7, 4479, 4480]] = [-1.0, 3.0, -1.0]
    v[2, [100, 101]] = [1.0, 1.0]
    return v


def _run(eng, x, slots, chunks, fmt, finals=None):
    """The calls of one segment per row: (per row the concatenated samples, per call the counts)."""
    xd = torch.from_numpy(np.ascontiguousarray(x)).to(eng.device)
    parts, counts, o = [[] for _ in slots], [], 0
    for k, c in enumerate(chunks):
        fin = [k == len(chunks) - 1] * len(slots) if finals is None else finals[k]
        out, cnt = eng.pcm_convert(xd[:, o:o + c].contiguous() if c else None, slots, fin, fmt)
        host = out.cpu().numpy()
        for b in range(len(slots)):
            parts[b].append(host[b, :cnt[b]].copy())
        counts.append(cnt)
        o += c
    eng.check_errors()
    return [np.concatenate(p) for p in parts], counts


@pytest.fixture(scope="module")
def one_shot(eng, x):
    """The one-call output of every resampled rate and encoding (computed once, shared)."""
    return {(rate, enc): _run(eng, x, SLOTS, [T], A.AudioFormat(rate, enc))[0]
            for rate in RESAMPLED for enc in A.ENCODINGS}


@pytest.mark.parametrize("enc", A.ENCODINGS)
@pytest.mark.parametrize("rate", RESAMPLED)
def test_chunked_equals_one_shot(eng, x, one_shot, rate, enc):
    fmt = A.AudioFormat(rate, enc)
    got, counts = _run(eng, x, SLOTS, CHUNKS, fmt)
    L, M, _ = A.RATES[rate]
    o = 0
    for k, c in enumerate(CHUNKS):
        assert counts[k] == [A.emitted(rate, o, c, k == len(CHUNKS) - 1)] * B
        o += c
    for b in range(B):
        assert got[b].dtype == fmt.dtype and got[b].size == -(-T * L // M)
        assert np.array_equal(got[b], one_shot[rate, enc][b]), (rate, enc, b)


@pytest.mark.parametrize("rate", RESAMPLED)
def test_f32_against_the_float64_reference(eng, x, one_shot, rate):
    L, M, N, taps = eng.pcm_filter(rate)
    want = A.resample_ref(x, rate, taps, dtype=np.float64)
    got = np.stack(one_shot[rate, "f32le"])
    # the fp32 accumulation bound: K rounded products and K rounded sums of terms bounded by |h_k| max|x|
    tol = (TAPS_PER_OUTPUT[rate] + 1) * 2.0 ** -24 * np.abs(taps.astype(np.float64)).sum() * np.abs(x).max()
    err = np.abs(got - want).max()
    print(f"rate {rate}: max |device - float64| {err:.3e}, bound {tol:.3e}")
    assert got.shape == want.shape and err <= tol
    # and the rule's fixed fp32 order on the host gives the device's bits
    assert np.array_equal(got, A.resample_ref(x, rate, taps))


@pytest.mark.parametrize("rate", RESAMPLED)
def test_s16_is_the_quantised_f32(eng, x, one_shot, rate):
    for b in range(B):
        assert np.array_equal(one_shot[rate, "s16le"][b], A.quantize_s16(one_shot[rate, "f32le"][b]))
    got16, _ = _run(eng, x, SLOTS, CHUNKS, A.AudioFormat(rate, "s16le"))
    got32, _ = _run(eng, x, SLOTS, CHUNKS, A.AudioFormat(rate, "f32le"))
    for b in range(B):
        assert np.array_equal(got16[b], A.quantize_s16(got32[b]))


def test_24k_s16le_is_the_numpy_rule(eng):
    v = np.random.default_rng(3).uniform(-1.2, 1.2, (B, 1285)).astype(np.float32)  # (1285: an odd tail, no vector store)
    edge = np.array([np.nan, 1.0, -1.0, 2.0, -2.0, np.inf, -np.inf, 0.0, -0.0, 0.5 / 32768, 1.5 / 32768, 2.5 / 32768,
                     -0.5 / 32768, -1.5 / 32768, -2.5 / 32768, 32766.5 / 32768, 32767.5 / 32768, -32767.5 / 32768,
                     0.99999, -0.99999, 1e-30, 3e38], dtype=np.float32)
    v[0, :edge.size] = edge
    v[2, -edge.size:] = edge[::-1]
    fmt = A.AudioFormat(24000, "s16le")
    for chunks in ([1285], [640, 645]):  # stateless: a non-final call emits everything it is given
        got, counts = _run(eng, v, SLOTS, chunks, fmt)
        assert counts == [[c] * B for c in chunks]
        for b in range(B):
            assert got[b].dtype == np.int16 and np.array_equal(got[b], A.quantize_s16(v[b]))
    # 24 kHz f32le: nothing to do, the rows themselves
    vd = torch.from_numpy(v).to(eng.device)
    out, cnt = eng.pcm_convert(vd, SLOTS, [True] * B, A.AudioFormat())
    assert cnt == [1285] * B and out.data_ptr() == vd.data_ptr()


@pytest.mark.parametrize("rate,enc", [(16000, "s16le"), (8000, "f32le"), (48000, "s16le")])
def test_rows_do_not_depend_on_their_neighbours(eng, x, one_shot, rate, enc):
    fmt = A.AudioFormat(rate, enc)
    alone, _ = _run(eng, x[1:2], [7], CHUNKS, fmt)  # another slot, no other row
    assert np.array_equal(alone[0], one_shot[rate, enc][1])
    rev, _ = _run(eng, x[::-1], [1, 3, 4], CHUNKS, fmt)  # other slots, other row order
    for b in range(B):
        assert np.array_equal(rev[B - 1 - b], one_shot[rate, enc][b])
    # rows whose segments stand at different positions share the later launches
    xd = torch.from_numpy(x).to(eng.device)
    out0, c0 = eng.pcm_convert(xd[0:1, :3200].contiguous(), [6], [False], fmt)
    parts = [out0.cpu().numpy()[0, :c0[0]].copy()]
    o = 3200
    for k, c in enumerate(CHUNKS[1:]):
        # slot 6 continues row 0 while slot 3 starts row 2's segment from its beginning with the same columns
        pcm = torch.stack([xd[0, o:o + c], xd[2, o - 3200:o - 3200 + c]]).contiguous()
        out, cnt = eng.pcm_convert(pcm, [6, 3], [k == 2, k == 2], fmt)
        parts.append(out.cpu().numpy()[0, :cnt[0]].copy())
        o += c
    eng.check_errors()
    assert np.array_equal(np.concatenate(parts), one_shot[rate, enc][0])


@pytest.mark.parametrize("rate", RESAMPLED)
def test_flush_only_emits_the_rest(eng, x, one_shot, rate):
    fmt = A.AudioFormat(rate, "s16le")
    L, M, _ = A.RATES[rate]
    got, counts = _run(eng, x, SLOTS, CHUNKS + [0], fmt, finals=[[False] * B] * 4 + [[True] * B])
    emitted = A.emitted_upto(rate, T, False)
    assert counts[-1] == [-(-T * L // M) - emitted] * B and counts[-1][0] > 0
    assert sum(c[0] for c in counts[:-1]) == emitted
    for b in range(B):
        assert np.array_equal(got[b], one_shot[rate, "s16le"][b])
    # a flush with nothing behind it emits nothing (the slots were reset by the final call)
    out, cnt = eng.pcm_convert(None, SLOTS, [True] * B, fmt)
    assert cnt == [0] * B
    # pcm_reset drops an unfinished segment: the next call starts one
    xd = torch.from_numpy(x).to(eng.device)
    eng.pcm_convert(xd[:, :640].contiguous(), SLOTS, [False] * B, fmt)
    for s in SLOTS:
        eng.pcm_reset(s)
    again, _ = _run(eng, x, SLOTS, [T], fmt)
    for b in range(B):
        assert np.array_equal(again[b], one_shot[rate, "s16le"][b])


def test_33_rows_are_two_launches_of_the_same_rows():
    """One more row than a launch's packet holds, a non-final and a final call: every row's bits, the second
    launch's row 32 among them, are the numpy rule's."""
    from llmvox_amd.engine import build_engine
    e = build_engine(0, "fp32", "fp32", max_streams=40, max_positions=64, max_codec_frames=64)
    try:
        rows = 33
        v = np.random.default_rng(33).uniform(-1, 1, (rows, 1280)).astype(np.float32)
        slots = [(7 * r + 3) % 40 for r in range(rows)]
        assert len(set(slots)) == rows
        for rate, enc in [(16000, "f32le"), (8000, "s16le")]:
            got, counts = _run(e, v, slots, [640, 640], A.AudioFormat(rate, enc))
            assert counts == [[A.emitted(rate, 0, 640, False)] * rows, [A.emitted(rate, 640, 640, True)] * rows]
            want = A.resample_ref(v, rate, e.pcm_filter(rate)[3])
            if enc == "s16le":
                want = A.quantize_s16(want)
            for r in range(rows):
                assert got[r].dtype == want.dtype and np.array_equal(got[r], want[r]), (rate, enc, r)
    finally:
        e.close()


def test_argument_errors(eng, x):
    from llmvox_amd import _lib
    lib = eng.lib
    xd = torch.from_numpy(x[:, :640].copy()).to(eng.device)
    out = torch.zeros(B, 1024, dtype=torch.int16, device=eng.device)
    cnt = (ctypes.c_int32 * B)()

    def call(slots=(0, 1, 2), rate=16000, enc=_lib.LVX_PCM_S16LE, stride=2048, n_in=640, nb=B, optr=None):
        sl = (ctypes.c_int32 * len(slots))(*slots)
        fl = (ctypes.c_uint8 * len(slots))(*([0] * len(slots)))
        return lib.lvx_pcm_convert(eng.h, ctypes.c_void_p(xd.data_ptr()), nb, n_in, sl, fl, rate, enc,
                                   ctypes.c_void_p(out.data_ptr() if optr is None else optr), stride, cnt, eng.stream_handle())

    for s in SLOTS + [0, 1]:
        eng.pcm_reset(s)
    bad = [dict(rate=22050), dict(rate=44100), dict(rate=0), dict(enc=2), dict(enc=-1), dict(slots=(0, 1, 8)),
           dict(slots=(0, -1, 2)), dict(slots=(0, 1, 0)), dict(stride=400), dict(stride=0), dict(stride=2046),
           dict(optr=out.data_ptr() + 2), dict(nb=0), dict(n_in=-1)]
    for kw in bad:
        assert call(**kw) == _lib.LVX_E_ARG, kw
    assert lib.lvx_pcm_reset(eng.h, 8, None) == _lib.LVX_E_ARG and lib.lvx_pcm_reset(eng.h, -1, None) == _lib.LVX_E_ARG
    # none of them moved a slot: the segment still starts here, and a first good call emits a first call's count
    assert call() == 0 and list(cnt) == [A.emitted(16000, 0, 640, False)] * B
    # a segment is resampled at one rate
    assert call(rate=8000) == _lib.LVX_E_ARG
    assert call() == 0 and list(cnt) == [A.emitted(16000, 640, 640, False)] * B
    for s in (0, 1, 2):
        eng.pcm_reset(s)
    with pytest.raises(ValueError):
        eng.pcm_convert(xd, [0, 1], [False, False], A.AudioFormat(16000))  # rows and slots disagree
    eng.check_errors()


@pytest.fixture(scope="module")
def sched_eng():
    from llmvox_amd.engine import build_engine
    e = build_engine(0, "fp32", "fp32", max_streams=4, max_positions=256, max_codec_frames=640)
    yield e
    e.close()


TEXT = "The quick brown fox jumps over the lazy dog."


def _speak(eng, audios, n_tokens):
    """Synthetic weights never end a sentence: each stream speaks one, ended by its tail as the service
    ends a request. Per stream: (its tokens, its items)."""
    from llmvox_amd.streaming import FusedScheduler
    sch = FusedScheduler(eng, max_chunk=16, to_bytes=True, overlap=True,
                         stop_rule=lambda st, ntok, pos: ntok >= n_tokens)
    sts = []
    for i, fmt in enumerate(audios):
        st = sch.open_stream(index=i, dump_size=10, **({} if fmt is None else {"audio": fmt}))
        for w in TEXT.split(" "):
            st.feed(w)
        sts.append(st)
    assert sch.run_until_idle(max_chunks=500) > 0
    for st in sts:
        toks, st.m.speech_outputs = st.m.speech_outputs, []
        if toks or st.pcm_open:  # (no tail and a converted stream: only its filter's flush)
            sch.queue_tail(st, toks)
    sch.flush()
    out = [(list(st.tokens), [e for e in st.events if isinstance(e, bytes)]) for st in sts]
    for st in sts:
        sch.close_stream(st)
    sch.close()
    eng.check_errors()
    return out


def test_scheduler_end_to_end(sched_eng):
    """A 16 kHz s16le stream beside a default one on FusedScheduler(overlap=True), same text and slot
    layout as a run of two default streams: the converted stream's sentence is the rule applied to the f32
    sentence of the same tokens, and the default stream beside it delivers the bytes it always did."""
    fmt = A.AudioFormat(16000, "s16le")
    (tok_a, plain), (tok_b, conv) = _speak(sched_eng, [None, fmt], 100)
    (tok_c, alone), (tok_d, other) = _speak(sched_eng, [None, None], 100)
    assert tok_a == tok_c and tok_b == tok_d and len(plain) >= 3
    assert plain == alone  # the default stream's bytes do not know about its neighbour's format
    x = np.frombuffer(b"".join(other), dtype="<f4")  # the f32 samples of the converted stream's own tokens
    assert x.size == 320 * len(tok_d) and len(conv) == len(other)
    got = np.frombuffer(b"".join(conv), dtype="<i2")
    assert got.size == -(-x.size * 2 // 3) and np.array_equal(got, A.convert_ref(x, fmt, _lib_taps(16000)))


def test_scheduler_flush_without_a_tail(sched_eng):
    """A stream stopped on a dump boundary (10 + 30 tokens) has no tail to decode: the flush-only call
    still ends its sentence, in an item of its own."""
    fmt = A.AudioFormat(8000, "f32le")
    ((tok, conv),) = _speak(sched_eng, [fmt], 40)
    ((tok_p, plain),) = _speak(sched_eng, [None], 40)
    assert tok == tok_p and len(tok) == 40 and len(plain) == 2 and len(conv) == 3
    x = np.frombuffer(b"".join(plain), dtype="<f4")
    got = np.frombuffer(b"".join(conv), dtype="<f4")
    assert got.size == -(-x.size // 3) and np.array_equal(got, A.convert_ref(x, fmt, _lib_taps(8000)))


def _lib_taps(rate):
    from llmvox_amd import _lib
    lib = _lib.load()
    n = 2 * A.RATES[rate][2] + 1
    taps = np.zeros(n, dtype=np.float32)
    _lib.check(lib.lvx_pcm_filter(rate, None, None, None, taps.ctypes.data_as(ctypes.c_void_p), n))
    return taps
