"""``"encoding": "flac"`` of POST /tts (CPU). With fake services: the field reaches submit, the media type and the
headers, the two new 422 cases (the wav container, frame_ms), the unknown-encoding message with its five names, and that
a request without flac reaches the service exactly as before. Then the real TTSService on a stand-in engine: the body
of a request of several sentences, whose two replica streams interleave, is a FLAC stream that tests/flac_decode.py
decodes to exactly the samples of the same request as s16le, with contiguous sample numbers."""
import numpy as np
import pytest
import torch

import flac_decode as D
import test_scheduler_g711 as G
from llmvox_amd import audio as A
from test_server_g711 import _body_chunks, _client, _FramingService, _TextOnlyService

TEXT = "Hello there. How are you. I am fine. Thanks a lot. See you soon."


def test_flac_reaches_submit_and_the_headers_say_so():
    svc = _FramingService()
    c = _client(svc)
    r = c.post("/tts", json={"text": "hi.", "sample_rate": 16000, "encoding": "flac", "volume": 2.5, "speed": 1.25})
    fmt = A.AudioFormat(16000, "flac", speed_pct=125, volume_pct=250)
    assert r.status_code == 200 and svc.calls == [("submit", "hi.", {"audio": fmt}), ("chunks", {})]
    assert r.headers["content-type"] == "audio/flac" and r.headers["x-audio-encoding"] == "flac"
    assert r.headers["x-audio-sample-rate"] == "16000" and r.headers["x-audio-frame-ms"] == "0"
    for rate in (8000, 24000, 48000):
        assert c.post("/tts", json={"text": "hi.", "sample_rate": rate, "encoding": "flac"}).status_code == 200


@pytest.mark.parametrize("body,says", [({"encoding": "flac", "container": "wav"}, "its own container"),
                                       ({"encoding": "flac", "frame_ms": 20}, "no fixed byte size"),
                                       ({"encoding": "flac", "sample_rate": 8000, "frame_ms": 40}, "no fixed byte size")])
def test_the_two_new_422_cases(body, says):
    svc = _FramingService()
    r = _client(svc).post("/tts", json=dict(body, text="hello."))
    assert r.status_code == 422 and says in r.text and "flac" in r.text and not svc.calls  # nothing was submitted


def test_unknown_encoding_lists_five_names():
    svc = _FramingService()
    r = _client(svc).post("/tts", json={"text": "hello.", "encoding": "FLAC"})
    assert r.status_code == 422 and not svc.calls
    assert len(A.FORMAT_ENCODINGS) == 5 and all(name in r.text for name in ("f32le", "s16le", "ulaw", "alaw", "flac"))


def test_a_request_without_flac_is_unchanged():
    svc = _TextOnlyService()
    r = _client(svc).post("/tts", json={"text": "hello world."})
    assert r.status_code == 200 and svc.calls == [("submit", "hello world."), ("chunks",)]
    assert r.content == b"".join(_body_chunks()) and r.headers["content-type"] == "application/octet-stream"
    svc = _FramingService()
    c = _client(svc)
    c.post("/tts", json={"text": "s16.", "sample_rate": 16000, "encoding": "s16le"})
    c.post("/tts", json={"text": "law.", "sample_rate": 8000, "encoding": "ulaw", "container": "wav", "frame_ms": 20})
    assert svc.calls == [("submit", "s16.", {"audio": A.AudioFormat(16000, "s16le")}), ("chunks", {}),
                         ("submit", "law.", {"audio": A.AudioFormat(8000, "ulaw", "wav")}), ("chunks", {"frame_ms": 20})]


def test_server_defaults_and_the_command_line():
    from llmvox_amd.server import app_options, arg_parser, create_app
    svc = _FramingService()
    r = _client(svc, sample_rate=8000, encoding="flac").post("/tts", json={"text": "hi."})
    assert svc.calls == [("submit", "hi.", {"audio": A.AudioFormat(8000, "flac")}), ("chunks", {})]
    assert r.headers["content-type"] == "audio/flac"
    for bad in ({"encoding": "flac", "frame_ms": 20}, {"encoding": "flac", "container": "wav"}):
        with pytest.raises(ValueError):
            create_app(svc, **bad)
    assert app_options(arg_parser().parse_args(["--encoding", "flac", "--sample-rate", "48000"]))["encoding"] == "flac"


def _service(monkeypatch):
    from llmvox_amd.server import TTSService
    monkeypatch.setitem(G._TORCH, "flac", torch.uint8)  # (the stand-in's dtype table knows the four older encodings)
    eng = G.G711Engine(max_streams=4, max_positions=4096, eoa=G.EOA)  # (end-of-audio every 41 positions: sentences end)
    return eng, TTSService([eng], max_chunk=16, max_tokens=200, eoa_id=G.EOA)


@pytest.mark.parametrize("fmt", [A.AudioFormat(8000, "flac"), A.AudioFormat(24000, "flac", volume_pct=250, speed_pct=125)],
                         ids=["8000", "24000-loud-fast"])
def test_service_body_decodes_to_the_s16le_request(monkeypatch, fmt):
    eng, svc = _service(monkeypatch)
    as16 = A.AudioFormat(fmt.sample_rate, "s16le", speed_pct=fmt.speed_pct, volume_pct=fmt.volume_pct)
    try:
        s16 = b"".join(svc.chunks(svc.submit(TEXT, audio=as16), timeout=0.01))
        calls16 = [c for c in eng.log if c[0] == "pcm_convert"]
        del eng.log[:]
        items = list(svc.chunks(svc.submit(TEXT, audio=fmt), timeout=0.01))
        calls = [c for c in eng.log if c[0] == "pcm_convert"]
        with pytest.raises(ValueError, match="no fixed byte size"):
            list(svc.chunks(svc.submit(TEXT, audio=fmt), timeout=0.01, frame_ms=20))
        assert not svc.workers[0].sessions  # (the refused session was closed)
    finally:
        svc.shutdown()
    want = np.frombuffer(s16, dtype="<i2")
    assert items[0] == A.flac_stream_header(fmt.sample_rate) and all(items[1:])
    got, frames = D.decode(b"".join(items))  # (the decoder holds the sample numbers contiguous from 0)
    assert np.array_equal(got, want) and len(frames) >= 4
    # both replicas spoke: finals on two slots, and the calls are those of the s16le request but for the encoding
    finals = {c[1] for c in calls if c[3]}
    assert len(finals) == 2 and sum(c[3] for c in calls) >= 3
    def shape(cs):  # (a request takes whichever two slots are free: they are named by their first appearance)
        names = {}
        return [(names.setdefault(c[1], len(names)),) + c[2:5] for c in cs]
    assert shape(calls) == shape(calls16) and {c[5] for c in calls} == {"flac"}
