"""``pause_ms`` and ``max_pause_ms`` of POST /tts (CPU). With fake services: the fields reach submit, the headers, the
422 cases (bad values, either field with flac), the server's defaults and command line, and that a request which names
neither reaches the service exactly as before. Then the real TTSService on a stand-in engine whose codec renders some
frames silent: the body of a request of several sentences, whose two replica streams interleave, is ``audio.pause_ref``
of the sentences in speaking order, behind the WAV header, with ``frame_ms`` cut after the trimming; and the engine
calls of the request are those of the same request without the fields."""
import struct

import numpy as np
import pytest

from llmvox_amd import audio as A
from test_scheduler_audio import EOA
from test_scheduler_pause import PauseEngine
from test_server_g711 import _body_chunks, _client, _FramingService, _TextOnlyService

TEXT = "Hello there. How are you. I am fine. Thanks a lot. See you soon."


def test_the_fields_reach_submit_and_the_headers_say_so():
    svc = _FramingService()
    c = _client(svc)
    r = c.post("/tts", json={"text": "hi.", "pause_ms": 150, "encoding": "s16le", "container": "wav"})
    fmt = A.AudioFormat(24000, "s16le", "wav", pause_ms=150)
    assert r.status_code == 200 and svc.calls == [("submit", "hi.", {"audio": fmt}), ("chunks", {})]
    assert r.headers["x-audio-pause"] == "150" and r.headers["x-audio-max-pause"] == "none"
    r = c.post("/tts", json={"text": "hi.", "max_pause_ms": 400, "frame_ms": 20})
    assert svc.calls[-2:] == [("submit", "hi.", {"audio": A.AudioFormat(max_pause_ms=400)}), ("chunks", {"frame_ms": 20})]
    assert r.headers["x-audio-pause"] == "none" and r.headers["x-audio-max-pause"] == "400"
    r = c.post("/tts", json={"text": "hi.", "pause_ms": 0, "max_pause_ms": 2000, "sample_rate": 8000, "encoding": "ulaw"})
    assert svc.calls[-2][2] == {"audio": A.AudioFormat(8000, "ulaw", pause_ms=0, max_pause_ms=2000)}
    assert r.headers["x-audio-pause"] == "0" and r.headers["x-audio-max-pause"] == "2000"
    r = c.post("/tts", json={"text": "hi."})
    assert r.headers["x-audio-pause"] == "none" and r.headers["x-audio-max-pause"] == "none"


@pytest.mark.parametrize("body,says", [({"pause_ms": 15}, "pause_ms"), ({"pause_ms": -10}, "pause_ms"), ({"pause_ms": 2010}, "pause_ms"),
                                       ({"pause_ms": 20.0}, "pause_ms"), ({"pause_ms": True}, "pause_ms"), ({"pause_ms": "20"}, "pause_ms"),
                                       ({"max_pause_ms": 90}, "max_pause_ms"), ({"max_pause_ms": 105}, "max_pause_ms"),
                                       ({"max_pause_ms": 400.0}, "max_pause_ms"), ({"max_pause_ms": False}, "max_pause_ms"),
                                       ({"pause_ms": 100, "encoding": "flac"}, "flac"), ({"max_pause_ms": 100, "encoding": "flac"}, "flac")])
def test_invalid_values_give_422(body, says):
    svc = _FramingService()
    r = _client(svc).post("/tts", json=dict(body, text="hello."))
    assert r.status_code == 422 and says in r.text and not svc.calls  # nothing was submitted


def test_a_request_without_the_fields_is_unchanged():
    svc = _TextOnlyService()
    r = _client(svc).post("/tts", json={"text": "hello world."})
    assert r.status_code == 200 and svc.calls == [("submit", "hello world."), ("chunks",)]
    assert r.content == b"".join(_body_chunks()) and r.headers["content-type"] == "application/octet-stream"
    svc = _FramingService()
    c = _client(svc)
    c.post("/tts", json={"text": "s16.", "sample_rate": 16000, "encoding": "s16le"})
    c.post("/tts", json={"text": "law.", "sample_rate": 8000, "encoding": "ulaw", "container": "wav", "frame_ms": 20})
    c.post("/tts", json={"text": "null.", "pause_ms": None, "max_pause_ms": None, "encoding": "flac"})
    assert svc.calls == [("submit", "s16.", {"audio": A.AudioFormat(16000, "s16le")}), ("chunks", {}),
                         ("submit", "law.", {"audio": A.AudioFormat(8000, "ulaw", "wav")}), ("chunks", {"frame_ms": 20}),
                         ("submit", "null.", {"audio": A.AudioFormat(24000, "flac")}), ("chunks", {})]
    assert not any(call[2]["audio"].pauses for call in svc.calls if call[0] == "submit")


def test_server_defaults_and_the_command_line():
    from llmvox_amd.server import app_options, arg_parser, create_app
    svc = _FramingService()
    c = _client(svc, pause_ms=150, max_pause_ms=400)
    r = c.post("/tts", json={"text": "hi."})
    assert svc.calls == [("submit", "hi.", {"audio": A.AudioFormat(pause_ms=150, max_pause_ms=400)}), ("chunks", {})]
    assert r.headers["x-audio-pause"] == "150" and r.headers["x-audio-max-pause"] == "400"
    r = c.post("/tts", json={"text": "hi.", "pause_ms": 0})
    assert svc.calls[-2][2] == {"audio": A.AudioFormat(pause_ms=0, max_pause_ms=400)} and r.headers["x-audio-pause"] == "0"
    assert c.post("/tts", json={"text": "hi.", "encoding": "flac"}).status_code == 422  # (the default pauses: no flac)
    for bad in (dict(pause_ms=15), dict(max_pause_ms=50), dict(pause_ms=True), dict(pause_ms=100, encoding="flac")):
        with pytest.raises(ValueError):
            create_app(svc, **bad)
    opts = app_options(arg_parser().parse_args(["--pause-ms", "150", "--max-pause-ms", "400"]))
    assert (opts["pause_ms"], opts["max_pause_ms"]) == (150, 400)
    opts = app_options(arg_parser().parse_args([]))
    assert opts["pause_ms"] is None and opts["max_pause_ms"] is None


def _sentences(blobs, fmt):
    """The sentences of the slots that reached the multiplexer, in speaking order (a record's `last` ends one)."""
    size, bps, out, cur = A.pause_slot_bytes(fmt), fmt.sample_bytes, [], []
    for blob in blobs:
        assert len(blob) % size == 0
        for at in range(0, len(blob), size):
            n, _, last, _ = struct.unpack_from("<HBBI", blob, at)
            cur.append(blob[at + 8:at + 8 + n * bps])
            if last:
                out.append(np.frombuffer(b"".join(cur), dtype=fmt.dtype))
                cur = []
    assert not cur
    return out


@pytest.mark.parametrize("fmt", [A.AudioFormat(8000, "s16le", "wav", pause_ms=150), A.AudioFormat(16000, "ulaw", pause_ms=30, max_pause_ms=100,
                                                                                                    volume_pct=200)],
                         ids=["8000-s16le-wav", "16000-ulaw-loud"])
def test_service_body_is_the_rule_over_the_sentences(monkeypatch, fmt):
    from llmvox_amd.server import TTSService
    eng = PauseEngine(max_streams=4, max_positions=4096, eoa=EOA)  # (end-of-audio every 41 positions: sentences end)
    svc = TTSService([eng], max_chunk=16, max_tokens=200, eoa_id=EOA)
    plain = A.AudioFormat(fmt.sample_rate, fmt.encoding, fmt.container, volume_pct=fmt.volume_pct)
    seen, push = [], A.PauseMux.push
    monkeypatch.setattr(A.PauseMux, "push", lambda self, blob: (seen.append(bytes(blob)), push(self, blob))[1])
    head = len(A.wav_header(fmt)) if fmt.container == "wav" else 0
    try:
        whole = b"".join(svc.chunks(svc.submit(TEXT, audio=plain), timeout=0.01))
        calls0 = [c for c in eng.log if c[0] == "pcm_convert"]
        assert not seen  # a format without the fields never meets the multiplexer
        del eng.log[:]
        items = list(svc.chunks(svc.submit(TEXT, audio=fmt), timeout=0.01))
        calls = [c for c in eng.log if c[0] == "pcm_convert"]
        sentences = _sentences(seen, fmt)
        framed = list(svc.chunks(svc.submit(TEXT, audio=fmt), timeout=0.01, frame_ms=20))
    finally:
        svc.shutdown()
    assert all(items) and len(sentences) >= 4
    assert b"".join(items)[:head] == whole[:head] == (A.wav_header(fmt) if head else b"")
    assert b"".join(y.tobytes() for y in sentences) == whole[head:]  # the sentences are the request's without the fields
    want = A.pause_ref(sentences, fmt)
    assert b"".join(items)[head:] == want and want != whole[head:]
    size = A.frame_bytes(fmt, 20)  # frame_ms behind it: whole frames of what the trimming left, the last one filled
    assert framed[0] == b"".join(items)[:head] or not head
    body = b"".join(framed[1:] if head else framed)
    assert all(len(i) % size == 0 and i for i in (framed[1:] if head else framed))
    assert body == want + bytes([A.silence_byte(fmt)]) * (-len(want) % size)
    # both replicas spoke, and the engine calls are those of the request without the fields
    def shape(cs):  # (a request takes whichever two slots are free: they are named by their first appearance)
        names = {}
        return [(names.setdefault(c[1], len(names)),) + c[2:] for c in cs]
    assert len({c[1] for c in calls if c[3]}) == 2 and shape(calls) == shape(calls0)
