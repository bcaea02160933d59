"""The G.711 encodings of the device PCM output stage (lvx_pcm_convert with LVX_PCM_ULAW / LVX_PCM_ALAW,
pcm_kernels.hip) against the rule of include/llmvox.h ("PCM G.711") as llmvox_amd/audio.py states it in numpy. The rule is
integer arithmetic behind the s16 quantisation, so every comparison is of bytes: all 65,536 quantised values and the
non-finite inputs at 24 kHz, every tail length of the dword store, the resampled rates chunked and one-shot against the
device's own s16le output and against convert_ref, 33 rows, a format that uses every stage, the argument errors, and a
mu-law stream beside a default one on FusedScheduler(overlap=True)."""
import ctypes

import numpy as np
import pytest
import torch

from llmvox_amd import audio as A
from test_gpu_pcm_out import B, CHUNKS, RESAMPLED, SLOTS, T, _lib_taps, _run, _speak
from test_gpu_pcm_out import x  # noqa: F401  (the fixture: the inputs of the s16le / f32le tests)

pytestmark = pytest.mark.gpu
LAWS = A.G711_LAWS


@pytest.fixture(scope="module")
def eng():
    from llmvox_amd.engine import build_engine
    e = build_engine(0, "fp32", "fp32", max_streams=8, max_positions=64, max_codec_frames=64)
    yield e
    e.close()


@pytest.fixture(scope="module")
def every_q():
    """4 rows of 16,389: row r its quarter of q / 32768, q = -32768 .. 32767 (exact in fp32), rows 1 and 3 descending,
    each followed by NaN, +inf, -inf, 2.0, -2.0. The odd length: the last block of a row ends in a byte-store tail, and
    rows 1 .. 3 start off a dword boundary of the input."""
    q = np.arange(-32768, 32768, dtype=np.float32).reshape(4, 16384) / np.float32(32768.0)
    q[1], q[3] = q[1, ::-1].copy(), q[3, ::-1].copy()
    tail = np.array([np.nan, np.inf, -np.inf, 2.0, -2.0], dtype=np.float32)
    v = np.concatenate([q, np.tile(tail, (4, 1))], axis=1)
    assert v.shape == (4, 16389)
    return np.ascontiguousarray(v)


@pytest.mark.parametrize("law", LAWS)
def test_every_quantised_value_at_24k(eng, every_q, law):
    qs = A.quantize_s16(every_q)
    assert np.array_equal(np.sort(qs[:, :16384].reshape(-1)), np.arange(-32768, 32768))  # the input does cover every q
    assert qs[:, 16384:].tolist() == [[0, 32767, -32768, 32767, -32768]] * 4
    got, counts = _run(eng, every_q, [0, 1, 2, 3], [16389], A.AudioFormat(24000, law))
    assert counts == [[16389] * 4]
    want = A.g711_encode(qs, law)
    for r in range(4):
        assert got[r].dtype == np.uint8 and np.array_equal(got[r], want[r]), (law, r, np.nonzero(got[r] != want[r])[0][:8])
    # the library's host entry gives the same bytes: the kernel and it share one statement of the companding
    assert np.array_equal(eng.g711_encode(qs, law), want)
    assert np.array_equal(eng.g711_decode(want, law), A.g711_decode(want, law))


@pytest.mark.parametrize("n_in", [1, 2, 3, 5, 1285])
def test_short_rows_at_24k(eng, n_in):
    """Every tail length of a thread's dword (1, 2, 3, then 4 + 1) and a block boundary (1,024 + 261), as one call and
    as two: stateless, a non-final call emits all it is given."""
    v = np.random.default_rng(n_in).uniform(-1.1, 1.1, (B, n_in)).astype(np.float32)
    for law in LAWS:
        want = A.g711_encode(A.quantize_s16(v), law)
        for chunks in ([n_in], [n_in // 2, n_in - n_in // 2]):
            got, counts = _run(eng, v, SLOTS, chunks, A.AudioFormat(24000, law))
            assert counts == [[c] * B for c in chunks]
            for b in range(B):
                assert got[b].dtype == np.uint8 and np.array_equal(got[b], want[b]), (law, chunks, b)


def test_rows_beside_a_short_row_stay_untouched(eng):
    """What lies behind a row's n_out bytes is not written: the tail's byte stores stop at the row's end."""
    v = np.random.default_rng(5).uniform(-1, 1, (2, 1285)).astype(np.float32)
    out, cnt = eng.pcm_convert(torch.from_numpy(v).to(eng.device), [0, 1], [True, True], A.AudioFormat(24000, "ulaw"))
    assert cnt == [1285, 1285] and out.dtype == torch.uint8 and out.shape[1] % 16 == 0 and out.shape[1] >= 1285
    assert out.data_ptr() % 16 == 0 and out.stride(0) % 16 == 0  # rows on 16-byte boundaries at one byte a sample
    # the same call through the C entry into a row pre-filled with a marker
    buf = torch.full((2, 1296), 0x33, dtype=torch.uint8, device=eng.device)
    n = (ctypes.c_int32 * 2)()
    xd = torch.from_numpy(v).to(eng.device)
    from llmvox_amd import _lib
    rc = eng.lib.lvx_pcm_convert(eng.h, ctypes.c_void_p(xd.data_ptr()), 2, 1285, (ctypes.c_int32 * 2)(0, 1),
                                 (ctypes.c_uint8 * 2)(1, 1), 24000, _lib.LVX_PCM_ULAW, ctypes.c_void_p(buf.data_ptr()), 1296, n,
                                 eng.stream_handle())
    assert rc == 0 and list(n) == [1285, 1285]
    host = buf.cpu().numpy()
    assert np.array_equal(host[:, :1285], A.g711_encode(A.quantize_s16(v), "ulaw")) and np.all(host[:, 1285:] == 0x33)
    eng.check_errors()


@pytest.fixture(scope="module")
def s16_chunked(eng, x):  # noqa: F811
    """The device's own s16le output of the chunked calls, per rate (computed once, shared)."""
    return {rate: _run(eng, x, SLOTS, CHUNKS, A.AudioFormat(rate, "s16le"))[0] for rate in RESAMPLED}


@pytest.mark.parametrize("law", LAWS)
@pytest.mark.parametrize("rate", RESAMPLED)
def test_resampled_chunked_one_shot_and_reference(eng, x, s16_chunked, rate, law):  # noqa: F811
    fmt = A.AudioFormat(rate, law)
    got, counts = _run(eng, x, SLOTS, CHUNKS, fmt)
    o = 0
    for k, c in enumerate(CHUNKS):
        assert counts[k] == [A.emitted(rate, o, c, k == len(CHUNKS) - 1)] * B
        o += c
    one, _ = _run(eng, x, SLOTS, [T], fmt)
    want = A.convert_ref(x, fmt, eng.pcm_filter(rate)[3])
    L, M, _ = A.RATES[rate]
    for b in range(B):
        assert got[b].dtype == np.uint8 and got[b].size == -(-T * L // M)
        assert np.array_equal(got[b], A.g711_encode(s16_chunked[rate][b], law)), (rate, law, b)  # the s16le stream's codes
        assert np.array_equal(got[b], want[b]), (rate, law, b)
        assert np.array_equal(got[b], one[b]), (rate, law, b)


def test_33_rows_equal_their_one_row_results():
    """One more row than a launch's packet holds, at 8 kHz mu-law, a non-final and a final call: every row, the second
    launch's row 32 among them, gives the bytes it gives alone."""
    from llmvox_amd.engine import build_engine
    e = build_engine(0, "fp32", "fp32", max_streams=40, max_positions=64, max_codec_frames=64)
    try:
        rows, fmt = 33, A.AudioFormat(8000, "ulaw")
        v = np.random.default_rng(33).uniform(-1, 1, (rows, 1280)).astype(np.float32)
        slots = [(7 * r + 3) % 40 for r in range(rows)]
        assert len(set(slots)) == rows
        got, counts = _run(e, v, slots, [640, 640], fmt)
        assert counts == [[A.emitted(8000, 0, 640, False)] * rows, [A.emitted(8000, 640, 640, True)] * rows]
        want = A.convert_ref(v, fmt, e.pcm_filter(8000)[3])
        for r in range(rows):
            alone, _ = _run(e, v[r:r + 1], [slots[r]], [640, 640], fmt)
            assert got[r].dtype == np.uint8 and np.array_equal(got[r], alone[0]), r
            assert np.array_equal(got[r], want[r]), r
    finally:
        e.close()


def test_composition_through_pcm_convert(eng):
    """Join, stretch, ratio, level, rate and A-law in one format: three dumps with context frames, against StreamRef
    with the library's tables, byte for byte."""
    x = np.random.default_rng(13).uniform(-0.6, 0.6, (B, 5760)).astype(np.float32)  # (volume 250: the limiter works)
    fmt = A.AudioFormat(8000, "alaw", "raw", 130, 90, True, 250)
    tables = (eng.pcm_filter(8000)[3], eng.pcm_stretch_window(), eng.pcm_ratio_filter(*fmt.ratio)[1],
              eng.pcm_join_window(), eng.pcm_level_window())
    ref = [A.StreamRef(fmt, *tables) for _ in range(B)]
    dumps = [(0, 3200, 0), (3200 - 2 * 320, 5120, 2), (5120 - 320, 5760, 1)]  # (start with context, end, context frames)
    xd = torch.from_numpy(x).to(eng.device)
    total = 0
    for k, (a, e, c) in enumerate(dumps):
        final = k == len(dumps) - 1
        out, cnt = eng.pcm_convert(xd[:, a:e].contiguous(), SLOTS, [final] * B, fmt, ctx_frames=[c] * B)
        host = out.cpu().numpy()
        assert host.dtype == np.uint8
        for b in range(B):
            want = ref[b].push(x[b, a:e], final, c)
            assert cnt[b] == want.size and np.array_equal(host[b, :cnt[b]], want), (k, b)
        total += cnt[0]
    assert total > 1000
    eng.check_errors()


def test_argument_errors(eng, x):  # noqa: F811
    from llmvox_amd import _lib
    lib = eng.lib
    xd = torch.from_numpy(x[:, :640].copy()).to(eng.device)
    out = torch.full((B, 1024), 0x33, dtype=torch.uint8, device=eng.device)
    cnt = (ctypes.c_int32 * B)()
    first = A.emitted(16000, 0, 640, False)
    assert 400 < first <= 1020

    def call(enc=_lib.LVX_PCM_ULAW, stride=1024, optr=None):
        sl, fl = (ctypes.c_int32 * B)(0, 1, 2), (ctypes.c_uint8 * B)(0, 0, 0)
        return lib.lvx_pcm_convert(eng.h, ctypes.c_void_p(xd.data_ptr()), B, 640, sl, fl, 16000, enc,
                                   ctypes.c_void_p(out.data_ptr() if optr is None else optr), stride, cnt, eng.stream_handle())

    for s in SLOTS + [0, 1]:
        eng.pcm_reset(s)
    bad = [dict(enc=2), dict(enc=3), dict(enc=5), dict(enc=8), dict(enc=-1), dict(stride=1022), dict(optr=out.data_ptr() + 1),
           dict(stride=first // 4 * 4 - 4), dict(stride=400), dict(stride=0)]
    for kw in bad:
        for enc in ([kw["enc"]] if "enc" in kw else [_lib.LVX_PCM_ULAW, _lib.LVX_PCM_ALAW]):
            assert call(**dict(kw, enc=enc)) == _lib.LVX_E_ARG, kw
    assert call(enc=8) == _lib.LVX_E_ARG and all(n in lib.lvx_last_error().decode() for n in
                                                 ("LVX_PCM_F32LE", "LVX_PCM_S16LE", "LVX_PCM_ULAW", "LVX_PCM_ALAW"))
    torch.cuda.synchronize()
    assert bool((out == 0x33).all())  # nothing was launched
    # none of them moved a slot: a first good call emits a first call's count, the next one the second's
    assert call(stride=(first + 3) // 4 * 4) == 0 and list(cnt) == [first] * B  # (a stride a row's bytes just fit)
    assert call() == 0 and list(cnt) == [A.emitted(16000, 640, 640, False)] * B
    assert call(enc=_lib.LVX_PCM_ALAW) == 0  # (the encoding is no part of a segment: a per-sample epilogue)
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
    """An 8 kHz mu-law stream beside a default one on FusedScheduler(overlap=True): the default stream's bytes are those
    of a run alone, and the G.711 stream's bytes are the codes of the same stream run as s16le (and of the rule applied
    to the f32 sentence of the same tokens)."""
    fmt, s16 = A.AudioFormat(8000, "ulaw"), A.AudioFormat(8000, "s16le")
    (tok_a, plain), (tok_b, conv) = _speak(sched_eng, [None, fmt], 100)
    (tok_c, alone), (tok_d, other) = _speak(sched_eng, [None, None], 100)
    (tok_e, _), (tok_f, as16) = _speak(sched_eng, [None, s16], 100)
    assert tok_a == tok_c == tok_e and tok_b == tok_d == tok_f and len(plain) >= 3
    assert plain == alone  # the default stream's bytes do not know about its neighbour's encoding
    assert len(conv) == len(as16)
    for c, s in zip(conv, as16):  # item by item: one byte per sample, the code of the s16le stream's sample
        assert c == A.g711_encode(np.frombuffer(s, dtype="<i2"), "ulaw").tobytes()
    xs = np.frombuffer(b"".join(other), dtype="<f4")
    got = np.frombuffer(b"".join(conv), dtype=np.uint8)
    assert got.size == -(-xs.size // 3) and np.array_equal(got, A.convert_ref(xs, fmt, _lib_taps(8000)))
