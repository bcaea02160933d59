"""The G.711 encodings and the ``frame_ms`` field of POST /tts with fake services (CPU): validation, the response's
headers, the WAV header in front of the frames, the frames themselves for awkward chunk sizes, and that a request that
names neither reaches the service exactly as before. Then the real TTSService on a stand-in engine: a framed 8 kHz
mu-law sentence is the codes of the same request as s16le, re-cut and filled with silence."""
import numpy as np
import pytest

from llmvox_amd import audio as A

SIZES = [1, 159, 160, 161, 1000]  # bytes of the fake service's chunks: none of them a frame's, their sum neither


def _body_chunks():
    return [bytes([17 + k]) * n for k, n in enumerate(SIZES)]


class _TextOnlyService:
    """The service as it was before any optional field: submit(text), chunks(session)."""

    def __init__(self):
        self.error = None
        self.sessions = []
        self.calls = []

    def submit(self, text):
        self.calls.append(("submit", text))
        return None

    def chunks(self, session):
        self.calls.append(("chunks",))
        yield from _body_chunks()


class _FramingService(_TextOnlyService):
    """Records what reaches it, and frames as TTSService.chunks does: the header, then audio.frame_chunks."""

    def submit(self, text, **kw):
        self.calls.append(("submit", text, kw))
        return kw.get("audio")

    def chunks(self, fmt, **kw):
        self.calls.append(("chunks", kw))
        fmt = fmt if fmt is not None else A.AudioFormat()
        if fmt.container == "wav":
            yield A.wav_header(fmt)
        body = iter(_body_chunks())
        yield from (A.frame_chunks(body, fmt, kw["frame_ms"]) if "frame_ms" in kw else body)


def _client(svc, **kw):
    from fastapi.testclient import TestClient
    from llmvox_amd.server import create_app
    return TestClient(create_app(svc, **kw))


@pytest.mark.parametrize("body", [{"encoding": "mulaw"}, {"encoding": "ULAW"}, {"encoding": "pcmu"}, {"frame_ms": 0},
                                  {"frame_ms": 15}, {"frame_ms": 20.0}, {"frame_ms": True}, {"frame_ms": "20"},
                                  {"frame_ms": 50}, {"frame_ms": -20}, {"encoding": "ulaw", "frame_ms": 25}])
def test_invalid_fields_give_422(body):
    svc = _FramingService()
    r = _client(svc).post("/tts", json=dict(body, text="hello."))
    assert r.status_code == 422 and not svc.calls  # nothing was submitted
    if "encoding" in body and body.get("frame_ms") is None:
        assert all(name in r.text for name in A.ENCODINGS)  # the message lists the four


def test_a_request_without_the_new_fields_is_unchanged():
    svc = _TextOnlyService()
    r = _client(svc).post("/tts", json={"text": "hello world."})
    assert r.status_code == 200 and svc.calls == [("submit", "hello world."), ("chunks",)]
    assert r.content == b"".join(_body_chunks())
    assert r.headers["x-audio-frame-ms"] == "0" and r.headers["x-audio-encoding"] == "f32le"
    assert r.headers["content-type"] == "application/octet-stream"
    svc = _FramingService()
    c = _client(svc)
    r = c.post("/tts", json={"text": "plain.", "frame_ms": None})  # null is absent
    assert svc.calls == [("submit", "plain.", {}), ("chunks", {})] and r.headers["x-audio-frame-ms"] == "0"
    del svc.calls[:]
    c.post("/tts", json={"text": "s16.", "sample_rate": 16000, "encoding": "s16le"})
    assert svc.calls == [("submit", "s16.", {"audio": A.AudioFormat(16000, "s16le")}), ("chunks", {})]


@pytest.mark.parametrize("law", A.G711_LAWS)
def test_the_encodings_reach_submit_and_the_headers_say_so(law):
    svc = _FramingService()
    c = _client(svc)
    r = c.post("/tts", json={"text": "hi.", "sample_rate": 8000, "encoding": law})
    assert r.status_code == 200 and svc.calls[0] == ("submit", "hi.", {"audio": A.AudioFormat(8000, law)})
    assert svc.calls[1] == ("chunks", {})  # no frame size named: chunks is called as before
    assert r.headers["x-audio-encoding"] == law and r.headers["x-audio-sample-rate"] == "8000"
    assert r.headers["x-audio-frame-ms"] == "0" and r.headers["content-type"] == "application/octet-stream"
    assert r.content == b"".join(_body_chunks())
    r = c.post("/tts", json={"text": "hi.", "encoding": law, "container": "wav"})  # G.711 at 24 kHz is allowed
    assert svc.calls[-2] == ("submit", "hi.", {"audio": A.AudioFormat(24000, law, "wav")})
    assert r.headers["content-type"] == "audio/wav" and r.content[:58] == A.wav_header(A.AudioFormat(24000, law, "wav"))


@pytest.mark.parametrize("enc,fill", [("ulaw", 0xFF), ("alaw", 0xD5), ("s16le", 0), ("f32le", 0)])
@pytest.mark.parametrize("container", ["raw", "wav"])
def test_frames(enc, fill, container):
    """8 kHz, 20 ms: 160 samples a frame. The header first and unframed, then chunks of whole frames whose
    concatenation is the service's bytes and a fill of silence shorter than one frame."""
    from fastapi.testclient import TestClient
    from llmvox_amd.server import create_app
    svc = _FramingService()
    fmt = A.AudioFormat(8000, enc, container)
    size = 160 * fmt.sample_bytes
    with TestClient(create_app(svc)) as c:
        with c.stream("POST", "/tts", json={"text": "hi.", "sample_rate": 8000, "encoding": enc, "container": container,
                                            "frame_ms": 20}) as r:
            assert r.status_code == 200 and r.headers["x-audio-frame-ms"] == "20" and r.headers["x-audio-encoding"] == enc
            got = r.read()
    assert svc.calls == [("submit", "hi.", {"audio": fmt}), ("chunks", {"frame_ms": 20})]  # never a submit argument
    head = A.wav_header(fmt) if container == "wav" else b""
    assert got[:len(head)] == head and len(head) == {"raw": 0, "wav": 58 if enc in A.G711_LAWS else 44}[container]
    body, whole = got[len(head):], b"".join(_body_chunks())
    assert len(body) % size == 0 and body[:len(whole)] == whole
    pad = body[len(whole):]
    assert len(pad) == -len(whole) % size and 0 < len(pad) < size and pad == bytes([fill]) * len(pad)
    # chunk by chunk, as the service yields them
    items = list(svc.chunks(fmt, frame_ms=20))
    if head:
        assert items.pop(0) == head
    assert items and all(len(i) % size == 0 and i for i in items) and b"".join(items) == body


def test_server_defaults_and_the_command_line():
    from llmvox_amd.server import app_options, arg_parser, create_app
    svc = _FramingService()
    c = _client(svc, sample_rate=8000, encoding="ulaw", frame_ms=20)
    r = c.post("/tts", json={"text": "hi."})
    assert svc.calls == [("submit", "hi.", {"audio": A.AudioFormat(8000, "ulaw")}), ("chunks", {"frame_ms": 20})]
    assert r.headers["x-audio-frame-ms"] == "20" and len(r.content) % 160 == 0
    r = c.post("/tts", json={"text": "hi.", "frame_ms": 60, "encoding": "alaw"})
    assert svc.calls[-1] == ("chunks", {"frame_ms": 60}) and r.headers["x-audio-frame-ms"] == "60" and len(r.content) % 480 == 0
    for bad in (15, True, 20.0):
        with pytest.raises(ValueError):
            create_app(svc, frame_ms=bad)
    a = arg_parser().parse_args(["--encoding", "alaw", "--sample-rate", "8000", "--frame-ms", "30"])
    opts = app_options(a)
    assert (opts["encoding"], opts["sample_rate"], opts["frame_ms"]) == ("alaw", 8000, 30)
    assert app_options(arg_parser().parse_args([]))["frame_ms"] is None
    for argv in (["--encoding", "mulaw"], ["--frame-ms", "15"]):
        with pytest.raises(SystemExit):
            arg_parser().parse_args(argv)


def test_service_frames_the_converted_sentence():
    from llmvox_amd.server import TTSService
    from test_scheduler_g711 import G711Engine
    eng = G711Engine(max_streams=4, max_positions=4096)
    svc = TTSService([eng], max_chunk=16, max_tokens=55)
    fmt = A.AudioFormat(8000, "ulaw", "wav")
    try:
        s16 = b"".join(svc.chunks(svc.submit("Hello there.", audio=A.AudioFormat(8000, "s16le")), timeout=0.01))
        loose = list(svc.chunks(svc.submit("Hello there.", audio=fmt), timeout=0.01))
        framed = list(svc.chunks(svc.submit("Hello there.", audio=fmt), timeout=0.01, frame_ms=20))
        plain = list(svc.chunks(svc.submit("Hello there."), timeout=0.01, frame_ms=10))  # any encoding: f32le at 24 kHz
    finally:
        svc.shutdown()
    codes = A.g711_encode(np.frombuffer(s16, dtype="<i2"), "ulaw").tobytes()
    assert loose[0] == A.wav_header(fmt) and b"".join(loose[1:]) == codes
    assert framed[0] == A.wav_header(fmt) and all(len(i) % 160 == 0 and i for i in framed[1:])
    assert len(codes) % 160 != 0  # (the sentence does not end on a frame: there is something to fill)
    assert b"".join(framed[1:]) == codes + b"\xff" * (-len(codes) % 160)
    assert all(len(i) % 960 == 0 and i for i in plain) and np.frombuffer(b"".join(plain), dtype="<f4").size % 240 == 0
