"""FusedScheduler and the service with a stream that asks for another speaking rate, on the CPU stand-in
engine of test_scheduler_audio (its ``pcm_convert`` is ``audio.StreamRef``: stretch, resample, encode): the
stretched stream's sentences are ``convert_ref`` of their own f32 sentences, the default stream beside it is
untouched, a slot's calls keep dump order and carry one speed, and ``POST /tts`` takes ``speed``."""
import numpy as np
import pytest
import torch

from llmvox_amd import audio as A
from llmvox_amd import streaming as S
from test_scheduler_audio import EOA, TEXT, AudioEngine, _same_events, _segments

FAST = A.AudioFormat(16000, "s16le", "raw", 130)


class SpeedEngine(AudioEngine):
    """AudioEngine that also records the speed of every ``pcm_convert`` call and refuses a speed change
    inside a slot's segment, as the library does."""

    def __init__(self, **kw):
        super().__init__(**kw)
        self.speeds = []

    def pcm_convert(self, pcm, slots, finals, fmt):
        for slot in slots:
            if slot in self.refs:
                assert self.refs[slot].fmt.speed_pct == fmt.speed_pct, "another speed inside a segment"
            self.speeds.append((slot, fmt.speed_pct))
        return super().pcm_convert(pcm, slots, finals, fmt)


def _run(overlap, audios, n_tokens=150, to_bytes=False):
    eng = SpeedEngine(max_streams=4, max_positions=4096, eoa=EOA)
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
    L, M, _ = A.RATES[fmt.sample_rate]
    for (items, ended), (pitems, pended) in zip(segs, plain):
        assert ended == pended
        x = np.concatenate(pitems)
        got = np.concatenate(items)
        assert got.dtype == fmt.dtype and all(i.dtype == fmt.dtype for i in items)
        want = A.convert_ref(x, fmt)
        if ended:  # a whole sentence: ceil(ceil(T 100 / pct) L / M) samples, those of the one-shot conversion
            assert got.size == want.size == -(-(-(-x.size * 100 // fmt.speed_pct)) * L // M)
            assert np.array_equal(got, want)
        else:      # the run stopped inside it: what the stretch and the filter could emit so far
            n = A.emitted_upto(fmt.sample_rate, A.stretch_emitted_upto(fmt.speed_pct, x.size, False), False)
            assert got.size == n and np.array_equal(got, want[:n])
    # the slot's calls: one per dump, in dump order, final exactly at the sentences' ends, all at one speed
    calls = [c for c in eng.log if c[0] == "pcm_convert" and c[1] == slot]
    want_calls = []
    for pitems, pended in plain:
        for k, p in enumerate(pitems):
            want_calls.append((p.size, pended and k == len(pitems) - 1))
    assert [(c[2], c[3]) for c in calls] == want_calls
    assert [s for s in eng.speeds if s[0] == slot] == [(slot, fmt.speed_pct)] * len(calls)


@pytest.mark.parametrize("overlap", [False, True], ids=["serial", "overlap"])
def test_stretched_stream_beside_a_default_one(overlap):
    eng0, plain = _run(overlap, [None, None])
    assert not [c for c in eng0.log if c[0].startswith("pcm_")]
    eng, mixed = _run(overlap, [None, FAST])
    assert mixed[0][2] == plain[0][2] and mixed[1][2] == plain[1][2]  # the same tokens
    _same_events(mixed[0][1], plain[0][1])  # the default stream's items: byte-identical to a run without the neighbour
    assert not [c for c in eng.log if c[0].startswith("pcm_") and c[1] == mixed[0][0]]
    _check_stream(eng, mixed[1][0], mixed[1][1], plain[1][1], FAST)


@pytest.mark.parametrize("fmt", [A.AudioFormat(speed_pct=77), A.AudioFormat(48000, "f32le", "raw", 200),
                                 A.AudioFormat(8000, "s16le", "wav", 50)], ids=lambda f: f"{f.sample_rate}-{f.speed_pct}")
def test_two_speeds_in_one_scheduler(fmt):
    """Two streams at different speeds never share an engine call: the bucket key holds the speed."""
    _, plain = _run(True, [None, None])
    eng, both = _run(True, [FAST, fmt])
    _check_stream(eng, both[0][0], both[0][1], plain[0][1], FAST)
    _check_stream(eng, both[1][0], both[1][1], plain[1][1], fmt)


def test_same_rate_and_encoding_at_two_speeds_are_two_calls():
    eng = SpeedEngine(max_streams=4)
    sch = S.FusedScheduler(eng, max_chunk=8, to_bytes=False, overlap=False)
    a = sch.open_stream(index=0, dump_size=10, audio=FAST)
    b = sch.open_stream(index=1, dump_size=10, audio=A.AudioFormat(16000, "s16le", "raw", 77))
    c = sch.open_stream(index=0, dump_size=10, audio=A.AudioFormat(16000, "s16le"))
    seen = []
    inner = eng.pcm_convert
    eng.pcm_convert = lambda pcm, slots, finals, fmt: (seen.append((list(slots), fmt.speed_pct)), inner(pcm, slots, finals, fmt))[1]
    res, err = sch._decode([(a, [7] * 10), (b, [9] * 10), (c, [11] * 10)], {0, 1, 2})
    assert err is None and sorted(seen) == sorted([([a.slot], 130), ([b.slot], 77), ([c.slot], 100)])
    pcm = eng.decode_codes(torch.tensor([[7] * 10, [9] * 10, [11] * 10])).numpy()
    for r, st in zip(range(3), (a, b, c)):
        assert np.array_equal(res[r], A.convert_ref(pcm[r], st.audio))
    for st in (a, b, c):
        sch.close_stream(st)
    sch.close()


def test_speed_alone_needs_the_stage_and_speed_100_does_not():
    eng, out = _run(True, [A.AudioFormat(speed_pct=130)])
    assert [c for c in eng.log if c[0] == "pcm_convert"] and out[0][1][0].dtype == np.float32
    eng, out = _run(True, [A.AudioFormat(24000, "f32le", "raw", 100)])
    assert not [c for c in eng.log if c[0].startswith("pcm_")]
    _, plain = _run(True, [None])
    _same_events(out[0][1], plain[0][1])


# ---- POST /tts ----------------------------------------------------------------------------------

def _client(svc, **kw):
    from fastapi.testclient import TestClient
    from llmvox_amd.server import create_app
    return TestClient(create_app(svc, **kw))


def test_tts_speed_field_and_header_round_trip():
    from test_server_audio import _AudioService
    svc = _AudioService()
    c = _client(svc)
    r = c.post("/tts", json={"text": "hi.", "speed": 1.3})
    assert r.status_code == 200 and svc.kwargs[-1] == {"audio": A.AudioFormat(24000, "f32le", "raw", 130)}
    assert r.headers["x-audio-speed"] == "1.30" and r.headers["x-audio-sample-rate"] == "24000"
    r = c.post("/tts", json={"text": "hi.", "speed": 0.5, "sample_rate": 16000, "encoding": "s16le", "container": "wav"})
    assert r.status_code == 200 and svc.kwargs[-1] == {"audio": A.AudioFormat(16000, "s16le", "wav", 50)}
    assert r.headers["x-audio-speed"] == "0.50" and r.headers["content-type"] == "audio/wav"
    r = c.post("/tts", json={"text": "hi.", "speed": 2})
    assert r.status_code == 200 and svc.kwargs[-1]["audio"].speed_pct == 200 and r.headers["x-audio-speed"] == "2.00"
    # no speed, or 1.0: the request reaches the service exactly as it always did
    for body in ({"text": "plain."}, {"text": "plain.", "speed": 1.0}, {"text": "plain.", "speed": 1.004}):
        r = c.post("/tts", json=body)
        assert r.status_code == 200 and svc.kwargs[-1] == {} and r.headers["x-audio-speed"] == "1.00"


@pytest.mark.parametrize("speed", [0.4, 2.5, 0, -1.0, 0.494, 2.006, "fast"])
def test_tts_speed_out_of_range_is_422(speed):
    from test_server_audio import _AudioService
    svc = _AudioService()
    r = _client(svc).post("/tts", json={"text": "hello.", "speed": speed})
    assert r.status_code == 422 and not svc.texts  # nothing was submitted


def test_server_default_speed():
    from llmvox_amd.server import create_app
    from test_server_audio import _AudioService
    svc = _AudioService()
    c = _client(svc, speed=0.77)
    r = c.post("/tts", json={"text": "hi."})
    assert svc.kwargs[-1] == {"audio": A.AudioFormat(speed_pct=77)} and r.headers["x-audio-speed"] == "0.77"
    r = c.post("/tts", json={"text": "hi.", "speed": 1.0})
    assert svc.kwargs[-1] == {} and r.headers["x-audio-speed"] == "1.00"
    for bad in (0.3, 2.5, float("nan")):
        with pytest.raises(ValueError):
            create_app(svc, speed=bad)


def test_service_streams_the_stretched_sentence():
    from llmvox_amd.server import TTSService
    eng = SpeedEngine(max_streams=4, max_positions=4096)
    svc = TTSService([eng], max_chunk=16, max_tokens=55)  # (the request stops between two dumps: it has a tail)
    try:
        plain = b"".join(svc.chunks(svc.submit("Hello there."), timeout=0.01))
        assert not [c for c in eng.log if c[0].startswith("pcm_")]
        fast = b"".join(svc.chunks(svc.submit("Hello there.", audio=FAST), timeout=0.01))
        slow = b"".join(svc.chunks(svc.submit("Hello there.", audio=A.AudioFormat(speed_pct=77)), timeout=0.01))
    finally:
        svc.shutdown()
    x = np.frombuffer(plain, dtype="<f4")
    assert np.array_equal(np.frombuffer(fast, dtype="<i2"), A.convert_ref(x, FAST))
    got = np.frombuffer(slow, dtype="<f4")
    assert got.size == -(-x.size * 100 // 77) and np.array_equal(got, A.convert_ref(x, A.AudioFormat(speed_pct=77)))
