"""FusedScheduler with a stream that asks for another volume, on the CPU stand-in engine of test_scheduler_audio (its
``pcm_convert`` is ``audio.StreamRef``: join, stretch, ratio, level, resample, encode): the loud stream's sentences are
``convert_ref`` of their own f32 sentences, the default stream beside it is untouched, a slot's calls keep dump order
and carry one volume, streams that differ in their volume alone never share a call, and a volume-100 stream makes the
calls of before."""
import numpy as np
import pytest
import torch

from llmvox_amd import audio as A
from llmvox_amd import streaming as S
from test_scheduler_audio import EOA, TEXT, AudioEngine, _same_events, _segments

LOUD = A.AudioFormat(volume_pct=300)


class VolumeEngine(AudioEngine):
    """AudioEngine that also records the volume of every ``pcm_convert`` call and refuses a change inside a slot's
    segment, as the library does."""

    def __init__(self, **kw):
        super().__init__(**kw)
        self.volumes = []

    def pcm_convert(self, pcm, slots, finals, fmt):
        for slot in slots:
            if slot in self.refs:
                assert self.refs[slot].fmt.volume_pct == fmt.volume_pct, "another volume inside a segment"
            self.volumes.append((slot, fmt.volume_pct))
        return super().pcm_convert(pcm, slots, finals, fmt)


def _run(overlap, audios, n_tokens=150, to_bytes=False):
    eng = VolumeEngine(max_streams=4, max_positions=4096, eoa=EOA)
    sch = S.FusedScheduler(eng, max_chunk=16, to_bytes=to_bytes, overlap=overlap,
                           stop_rule=lambda st, ntok, pos: ntok >= n_tokens)
    sts = []
    for i, fmt in enumerate(audios):
        kw = {"eoa_id": EOA}
        if fmt is not None:
            kw["audio"] = fmt
        st = sch.open_stream(index=i, dump_size=10, **kw)
        for w in TEXT.split(" "):
            st.feed(w)
        sts.append(st)
    assert sch.run_until_idle(max_chunks=2000) > 0
    out = [(st.slot, list(st.events), list(st.tokens)) for st in sts]
    for st in sts:
        sch.close_stream(st)
    sch.close()
    return eng, out


def _check_stream(eng, slot, events, plain_events, fmt):
    segs, plain = _segments(events), _segments(plain_events)
    assert len(segs) == len(plain) and len(segs) >= 3
    limited = 0
    for (items, ended), (pitems, pended) in zip(segs, plain):
        assert ended == pended
        x = np.concatenate(pitems)
        got = np.concatenate(items)
        assert got.dtype == fmt.dtype and all(i.dtype == fmt.dtype for i in items)
        want = A.convert_ref(x, fmt)
        if ended:  # a whole sentence: one sample per input of the level stage, the samples of the one-shot conversion
            assert got.size == want.size and np.array_equal(got.view(np.uint8), want.view(np.uint8))
        else:      # the run stopped inside it: the stage still holds its last 240 samples back
            L, M = fmt.ratio
            n = A.ratio_emitted_upto(L, M, A.stretch_emitted_upto(fmt.stretch_pct, x.size, False), False)
            n = A.emitted_upto(fmt.sample_rate, A.level_emitted_upto(fmt.volume_pct, n, False), False)
            assert got.size == n and np.array_equal(got.view(np.uint8), want[:n].view(np.uint8))
        if fmt.sample_rate == 24000 and fmt.encoding == "f32le" and fmt.stretch_pct == 100:
            limited += int((A.level_ref(x, fmt.volume_pct)[1] < 1).sum())
            assert float(np.abs(got).max()) <= float(A.LEVEL_CEIL) * (1 + 2.0 ** -22)
    # the slot's calls: one per dump, in dump order, final exactly at the sentences' ends, all at one volume
    calls = [c for c in eng.log if c[0] == "pcm_convert" and c[1] == slot]
    want_calls = []
    for pitems, pended in plain:
        for k, p in enumerate(pitems):
            want_calls.append((p.size, pended and k == len(pitems) - 1))
    assert [(c[2], c[3]) for c in calls] == want_calls
    assert [v for v in eng.volumes if v[0] == slot] == [(slot, fmt.volume_pct)] * len(calls)
    return limited


@pytest.mark.parametrize("overlap", [False, True], ids=["serial", "overlap"])
def test_loud_stream_beside_a_default_one(overlap):
    eng0, plain = _run(overlap, [None, None])
    assert not [c for c in eng0.log if c[0].startswith("pcm_")]
    eng, mixed = _run(overlap, [None, LOUD])
    assert mixed[0][2] == plain[0][2] and mixed[1][2] == plain[1][2]  # the same tokens
    _same_events(mixed[0][1], plain[0][1])  # the default stream's items: byte-identical to a run without the neighbour
    assert not [c for c in eng.log if c[0].startswith("pcm_") and c[1] == mixed[0][0]]
    assert _check_stream(eng, mixed[1][0], mixed[1][1], plain[1][1], LOUD) > 0  # (the limiter had work to do)
    # the default stream's engine calls are those of a run without the loud one
    mine = lambda log, slot: [c for c in log if len(c) > 1 and c[1] == slot]
    assert mine(eng.log, mixed[0][0]) == mine(eng0.log, plain[0][0])


@pytest.mark.parametrize("fmt", [A.AudioFormat(16000, "s16le", "raw", 120, 90, False, 250),
                                 A.AudioFormat(48000, "f32le", "raw", 100, 100, False, 40),
                                 A.AudioFormat(24000, "s16le", "wav", 100, 100, False, 0)],
                         ids=lambda f: f"{f.sample_rate}-{f.speed_pct}-{f.pitch_pct}-{f.volume_pct}")
def test_two_volumes_in_one_scheduler(fmt):
    _, plain = _run(True, [None, None])
    eng, both = _run(True, [LOUD, fmt])
    _check_stream(eng, both[0][0], both[0][1], plain[0][1], LOUD)
    _check_stream(eng, both[1][0], both[1][1], plain[1][1], fmt)


def test_streams_that_differ_in_volume_alone_are_separate_calls():
    """The bucket key holds the volume: two streams of one codec call at two volumes never share a ``pcm_convert``."""
    eng = VolumeEngine(max_streams=4)
    sch = S.FusedScheduler(eng, max_chunk=8, to_bytes=False, overlap=False)
    a = sch.open_stream(index=0, dump_size=10, audio=A.AudioFormat(16000, "s16le", volume_pct=300))
    b = sch.open_stream(index=1, dump_size=10, audio=A.AudioFormat(16000, "s16le", volume_pct=50))
    c = sch.open_stream(index=0, dump_size=10, audio=A.AudioFormat(16000, "s16le"))
    d = sch.open_stream(index=1, dump_size=10, audio=A.AudioFormat(16000, "s16le", volume_pct=300))
    seen = []
    inner = eng.pcm_convert
    eng.pcm_convert = lambda pcm, slots, finals, fmt: (seen.append((sorted(slots), fmt.volume_pct)),
                                                       inner(pcm, slots, finals, fmt))[1]
    res, err = sch._decode([(a, [7] * 10), (b, [9] * 10), (c, [11] * 10), (d, [13] * 10)], {0, 1, 2, 3})
    assert err is None
    assert sorted(seen) == sorted([(sorted([a.slot, d.slot]), 300), ([b.slot], 50), ([c.slot], 100)])
    pcm = eng.decode_codes(torch.tensor([[7] * 10, [9] * 10, [11] * 10, [13] * 10])).numpy()
    for r, st in enumerate((a, b, c, d)):
        assert np.array_equal(res[r], A.convert_ref(pcm[r], st.audio))
    for st in (a, b, c, d):
        sch.close_stream(st)
    sch.close()


def test_a_volume_100_stream_makes_the_calls_of_before():
    plain_fmt = A.AudioFormat(16000, "s16le", "raw", 130)
    named = A.AudioFormat(16000, "s16le", "raw", 130, 100, False, 100)
    eng_a, out_a = _run(True, [None, plain_fmt])
    eng_b, out_b = _run(True, [None, named])
    assert eng_a.log == eng_b.log
    for (_, ev_a, tok_a), (_, ev_b, tok_b) in zip(out_a, out_b):
        assert tok_a == tok_b
        _same_events(ev_a, ev_b)
    # a volume alone needs the stage; volume 100 and nothing else does not reach it
    eng, out = _run(True, [A.AudioFormat(volume_pct=50)])
    assert [c for c in eng.log if c[0] == "pcm_convert"] and out[0][1][0].dtype == np.float32
    eng, out = _run(True, [A.AudioFormat(24000, "f32le", "raw", 100, 100, False, 100)])
    assert not [c for c in eng.log if c[0].startswith("pcm_")]
    _, plain = _run(True, [None])
    _same_events(out[0][1], plain[0][1])


def test_service_streams_the_loud_sentence():
    from llmvox_amd.server import TTSService
    eng = VolumeEngine(max_streams=4, max_positions=4096)
    svc = TTSService([eng], max_chunk=16, max_tokens=55)  # (the request stops between two dumps: it has a tail)
    try:
        plain = b"".join(svc.chunks(svc.submit("Hello there."), timeout=0.01))
        assert not [c for c in eng.log if c[0].startswith("pcm_")]
        loud = b"".join(svc.chunks(svc.submit("Hello there.", audio=LOUD), timeout=0.01))
        soft = b"".join(svc.chunks(svc.submit("Hello there.", audio=A.AudioFormat(16000, "s16le", "wav", volume_pct=50)),
                                   timeout=0.01))
    finally:
        svc.shutdown()
    x = np.frombuffer(plain, dtype="<f4")
    got = np.frombuffer(loud, dtype="<f4")
    assert got.size == x.size  # every held-back sample is delivered at the end
    assert np.array_equal(got.view(np.uint32), A.convert_ref(x, LOUD).view(np.uint32))
    fmt = A.AudioFormat(16000, "s16le", "wav", volume_pct=50)
    assert soft[:44] == A.wav_header(fmt)
    assert np.array_equal(np.frombuffer(soft[44:], dtype="<i2"), A.convert_ref(x, fmt))
