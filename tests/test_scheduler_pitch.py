"""FusedScheduler and the service with a stream that asks for another pitch, on the CPU stand-in engine of
test_scheduler_audio (its ``pcm_convert`` is ``audio.StreamRef``: stretch, ratio, resample, encode): the pitched
stream's sentences are ``convert_ref`` of their own f32 sentences, the default stream beside it is untouched, a
slot's calls keep dump order and carry one pitch, a pitch-100 stream makes the calls of before, and ``POST /tts``
takes ``pitch``."""
import numpy as np
import pytest
import torch

from llmvox_amd import audio as A
from llmvox_amd import streaming as S
from test_scheduler_audio import EOA, TEXT, AudioEngine, _same_events, _segments

PITCHED = A.AudioFormat(16000, "s16le", "raw", 120, 90)


class PitchEngine(AudioEngine):
    """AudioEngine that also records the speed and pitch of every ``pcm_convert`` call and refuses a change of
    either inside a slot's segment, as the library does."""

    def __init__(self, **kw):
        super().__init__(**kw)
        self.pitches = []

    def pcm_convert(self, pcm, slots, finals, fmt):
        for slot in slots:
            if slot in self.refs:
                held = self.refs[slot].fmt
                assert (held.speed_pct, held.pitch_pct) == (fmt.speed_pct, fmt.pitch_pct), "another pitch inside a segment"
            self.pitches.append((slot, fmt.speed_pct, fmt.pitch_pct))
        return super().pcm_convert(pcm, slots, finals, fmt)


def _run(overlap, audios, n_tokens=150, to_bytes=False):
    eng = PitchEngine(max_streams=4, max_positions=4096, eoa=EOA)
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


def _emitted_so_far(fmt, T):
    """What the three stages could emit of a sentence that has T samples so far and has not ended."""
    L, M = fmt.ratio
    n = A.stretch_emitted_upto(fmt.stretch_pct, T, False)
    n = A.ratio_emitted_upto(L, M, n, False)
    return A.emitted_upto(fmt.sample_rate, n, False)


def _check_stream(eng, slot, events, plain_events, fmt):
    segs, plain = _segments(events), _segments(plain_events)
    assert len(segs) == len(plain) and len(segs) >= 3
    l, m, _ = A.RATES[fmt.sample_rate]
    L, M = fmt.ratio
    for (items, ended), (pitems, pended) in zip(segs, plain):
        assert ended == pended
        x = np.concatenate(pitems)
        got = np.concatenate(items)
        assert got.dtype == fmt.dtype and all(i.dtype == fmt.dtype for i in items)
        want = A.convert_ref(x, fmt)
        if ended:  # a whole sentence: the three counts of the plan, the samples of the one-shot conversion
            n1 = -(-x.size * 100 // fmt.stretch_pct)
            n2 = -(-n1 * L // M)
            assert got.size == want.size == -(-n2 * l // m)
            assert np.array_equal(got, want)
        else:      # the run stopped inside it
            n = _emitted_so_far(fmt, x.size)
            assert got.size == n and np.array_equal(got, want[:n])
    # the slot's calls: one per dump, in dump order, final exactly at the sentences' ends, all at one pitch
    calls = [c for c in eng.log if c[0] == "pcm_convert" and c[1] == slot]
    want_calls = []
    for pitems, pended in plain:
        for k, p in enumerate(pitems):
            want_calls.append((p.size, pended and k == len(pitems) - 1))
    assert [(c[2], c[3]) for c in calls] == want_calls
    assert [p for p in eng.pitches if p[0] == slot] == [(slot, fmt.speed_pct, fmt.pitch_pct)] * len(calls)


@pytest.mark.parametrize("overlap", [False, True], ids=["serial", "overlap"])
def test_pitched_stream_beside_a_default_one(overlap):
    eng0, plain = _run(overlap, [None, None])
    assert not [c for c in eng0.log if c[0].startswith("pcm_")]
    eng, mixed = _run(overlap, [None, PITCHED])
    assert mixed[0][2] == plain[0][2] and mixed[1][2] == plain[1][2]  # the same tokens
    _same_events(mixed[0][1], plain[0][1])  # the default stream's items: byte-identical to a run without the neighbour
    assert not [c for c in eng.log if c[0].startswith("pcm_") and c[1] == mixed[0][0]]
    _check_stream(eng, mixed[1][0], mixed[1][1], plain[1][1], PITCHED)


@pytest.mark.parametrize("fmt", [A.AudioFormat(pitch_pct=125), A.AudioFormat(48000, "f32le", "raw", 130, 130),
                                 A.AudioFormat(8000, "s16le", "wav", 77, 110)],
                         ids=lambda f: f"{f.sample_rate}-{f.speed_pct}-{f.pitch_pct}")
def test_two_pitches_in_one_scheduler(fmt):
    _, plain = _run(True, [None, None])
    eng, both = _run(True, [PITCHED, fmt])
    _check_stream(eng, both[0][0], both[0][1], plain[0][1], PITCHED)
    _check_stream(eng, both[1][0], both[1][1], plain[1][1], fmt)


def test_same_rate_encoding_and_speed_at_two_pitches_are_two_calls():
    """Two streams that differ in their pitch alone never share an engine call: the bucket key holds it."""
    eng = PitchEngine(max_streams=4)
    sch = S.FusedScheduler(eng, max_chunk=8, to_bytes=False, overlap=False)
    a = sch.open_stream(index=0, dump_size=10, audio=PITCHED)
    b = sch.open_stream(index=1, dump_size=10, audio=A.AudioFormat(16000, "s16le", "raw", 120, 110))
    c = sch.open_stream(index=0, dump_size=10, audio=A.AudioFormat(16000, "s16le", "raw", 120))
    seen = []
    inner = eng.pcm_convert
    eng.pcm_convert = lambda pcm, slots, finals, fmt: (seen.append((list(slots), fmt.speed_pct, fmt.pitch_pct)),
                                                       inner(pcm, slots, finals, fmt))[1]
    res, err = sch._decode([(a, [7] * 10), (b, [9] * 10), (c, [11] * 10)], {0, 1, 2})
    assert err is None and sorted(seen) == sorted([([a.slot], 120, 90), ([b.slot], 120, 110), ([c.slot], 120, 100)])
    pcm = eng.decode_codes(torch.tensor([[7] * 10, [9] * 10, [11] * 10])).numpy()
    for r, st in zip(range(3), (a, b, c)):
        assert np.array_equal(res[r], A.convert_ref(pcm[r], st.audio))
    for st in (a, b, c):
        sch.close_stream(st)
    sch.close()


def test_a_pitch_100_stream_makes_the_calls_of_before():
    plain_fmt, named = A.AudioFormat(16000, "s16le", "raw", 130), A.AudioFormat(16000, "s16le", "raw", 130, 100)
    eng_a, out_a = _run(True, [None, plain_fmt])
    eng_b, out_b = _run(True, [None, named])
    assert eng_a.log == eng_b.log and eng_a.pitches == eng_b.pitches
    for (_, ev_a, tok_a), (_, ev_b, tok_b) in zip(out_a, out_b):
        assert tok_a == tok_b
        _same_events(ev_a, ev_b)
    # a pitch alone needs the stage; pitch 100 and nothing else does not reach it
    eng, out = _run(True, [A.AudioFormat(pitch_pct=125)])
    assert [c for c in eng.log if c[0] == "pcm_convert"] and out[0][1][0].dtype == np.float32
    eng, out = _run(True, [A.AudioFormat(24000, "f32le", "raw", 100, 100)])
    assert not [c for c in eng.log if c[0].startswith("pcm_")]
    _, plain = _run(True, [None])
    _same_events(out[0][1], plain[0][1])


# ---- POST /tts ----------------------------------------------------------------------------------

def _client(svc, **kw):
    from fastapi.testclient import TestClient
    from llmvox_amd.server import create_app
    return TestClient(create_app(svc, **kw))


def test_tts_pitch_field_and_header_round_trip():
    from test_server_audio import _AudioService
    svc = _AudioService()
    c = _client(svc)
    r = c.post("/tts", json={"text": "hi.", "pitch": 1.25})
    assert r.status_code == 200 and svc.kwargs[-1] == {"audio": A.AudioFormat(24000, "f32le", "raw", 100, 125)}
    assert r.headers["x-audio-pitch"] == "1.2500" and r.headers["x-audio-speed"] == "1.00"
    r = c.post("/tts", json={"text": "hi.", "pitch": 0.9, "speed": 1.2, "sample_rate": 16000, "encoding": "s16le",
                             "container": "wav"})
    assert r.status_code == 200 and svc.kwargs[-1] == {"audio": A.AudioFormat(16000, "s16le", "wav", 120, 90)}
    # the realised ratio: speed_pct / stretch_pct = 120 / 133, not 0.9
    assert r.headers["x-audio-pitch"] == f"{120 / 133:.4f}" == "0.9023" and r.headers["x-audio-speed"] == "1.20"
    assert r.headers["content-type"] == "audio/wav"
    r = c.post("/tts", json={"text": "hi.", "pitch": 2})
    assert r.status_code == 200 and svc.kwargs[-1]["audio"].pitch_pct == 200 and r.headers["x-audio-pitch"] == "2.0000"
    # no pitch, or 1.0: the request reaches the service exactly as it always did
    for body in ({"text": "plain."}, {"text": "plain.", "pitch": 1.0}, {"text": "plain.", "pitch": 1.004}):
        r = c.post("/tts", json=body)
        assert r.status_code == 200 and svc.kwargs[-1] == {} and r.headers["x-audio-pitch"] == "1.0000"
    r = c.post("/tts", json={"text": "fast.", "speed": 1.3})
    assert svc.kwargs[-1] == {"audio": A.AudioFormat(24000, "f32le", "raw", 130)} and r.headers["x-audio-pitch"] == "1.0000"


@pytest.mark.parametrize("body", [{"pitch": 0.4}, {"pitch": 2.5}, {"pitch": 0}, {"pitch": -1.0}, {"pitch": 0.494},
                                  {"pitch": 2.006}, {"pitch": "high"}, {"pitch": 0.5, "speed": 2.0},
                                  {"pitch": 2.0, "speed": 0.5}, {"pitch": 0.99, "speed": 2.0}],
                         ids=lambda b: "-".join(f"{k}{v}" for k, v in b.items()))
def test_tts_pitch_out_of_range_is_422(body):
    from test_server_audio import _AudioService
    svc = _AudioService()
    r = _client(svc).post("/tts", json={"text": "hello.", **body})
    assert r.status_code == 422 and not svc.texts  # nothing was submitted
    if "speed" in body:  # the plan's message
        assert "time stretch" in r.json()["detail"]


def test_server_default_pitch():
    from llmvox_amd import server
    from test_server_audio import _AudioService
    svc = _AudioService()
    c = _client(svc, pitch=0.8)
    r = c.post("/tts", json={"text": "hi."})
    assert svc.kwargs[-1] == {"audio": A.AudioFormat(pitch_pct=80)} and r.headers["x-audio-pitch"] == "0.8000"
    r = c.post("/tts", json={"text": "hi.", "pitch": 1.0})
    assert svc.kwargs[-1] == {} and r.headers["x-audio-pitch"] == "1.0000"
    r = c.post("/tts", json={"text": "hi.", "speed": 2.0})  # the default pitch with this speed has no plan
    assert r.status_code == 422
    for bad in (dict(pitch=0.3), dict(pitch=2.5), dict(pitch=float("nan")), dict(pitch=0.5, speed=2.0)):
        with pytest.raises(ValueError):
            server.create_app(svc, **bad)
    # the command line reaches create_app
    d = server.app_options(server.arg_parser().parse_args(["--pitch", "1.1", "--speed", "0.9"]))
    assert (d["pitch"], d["speed"]) == (1.1, 0.9)
    assert server.app_options(server.arg_parser().parse_args([]))["pitch"] == 1.0
    r = _client(svc, **d).post("/tts", json={"text": "hi."})
    assert svc.kwargs[-1] == {"audio": A.AudioFormat(speed_pct=90, pitch_pct=110)}
    assert r.headers["x-audio-pitch"] == f"{90 / 82:.4f}"


def test_service_streams_the_pitched_sentence():
    from llmvox_amd.server import TTSService
    eng = PitchEngine(max_streams=4, max_positions=4096)
    svc = TTSService([eng], max_chunk=16, max_tokens=55)  # (the request stops between two dumps: it has a tail)
    try:
        plain = b"".join(svc.chunks(svc.submit("Hello there."), timeout=0.01))
        assert not [c for c in eng.log if c[0].startswith("pcm_")]
        low = b"".join(svc.chunks(svc.submit("Hello there.", audio=PITCHED), timeout=0.01))
        high = b"".join(svc.chunks(svc.submit("Hello there.", audio=A.AudioFormat(pitch_pct=125)), timeout=0.01))
    finally:
        svc.shutdown()
    x = np.frombuffer(plain, dtype="<f4")
    assert np.array_equal(np.frombuffer(low, dtype="<i2"), A.convert_ref(x, PITCHED))
    got = np.frombuffer(high, dtype="<f4")
    assert got.size == -(-(-(-x.size * 100 // 80)) * 4 // 5)
    assert np.array_equal(got, A.convert_ref(x, A.AudioFormat(pitch_pct=125)))
