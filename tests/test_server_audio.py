"""The audio-format fields of POST /tts with fake services (CPU): validation, the defaults of the
server, the response's media type and headers, the WAV header in front of the stream, and that a request
that names no format reaches the service and leaves it exactly as before. Then the real TTSService on a
stand-in engine: one sentence in WAV / 16 kHz / s16le is the rule applied to the default request's samples."""
import numpy as np
import pytest

from llmvox_amd import audio as A


class _TextOnlyService:
    """The service as it was: submit(text) and nothing else."""

    def __init__(self):
        self.error = None
        self.sessions = []
        self.texts = []

    def submit(self, text):
        self.texts.append(text)
        return text

    def chunks(self, session):
        for i in range(3):
            yield np.full(320 * (i + 1), i, dtype=np.float32).tobytes()


class _AudioService(_TextOnlyService):
    def __init__(self):
        super().__init__()
        self.kwargs = []

    def submit(self, text, **kw):
        self.texts.append(text)
        self.kwargs.append(kw)
        return kw.get("audio")

    def chunks(self, fmt):
        if fmt is not None and fmt.container == "wav":
            yield A.wav_header(fmt)
        for i in range(3):
            yield np.full(16 * (i + 1), i, dtype=fmt.dtype if fmt is not None else np.float32).tobytes()


def _client(svc, **kw):
    from fastapi.testclient import TestClient
    from llmvox_amd.server import create_app
    return TestClient(create_app(svc, **kw))


def test_default_request_is_unchanged():
    svc = _TextOnlyService()
    r = _client(svc).post("/tts", json={"text": "hello world."})
    assert r.status_code == 200 and svc.texts == ["hello world."]
    assert r.headers["content-type"] == "application/octet-stream"
    assert r.content == b"".join(np.full(320 * (i + 1), i, dtype=np.float32).tobytes() for i in range(3))
    assert r.headers["x-audio-sample-rate"] == "24000" and r.headers["x-audio-encoding"] == "f32le"
    # the default format spelled out is still the default request
    r2 = _client(svc).post("/tts", json={"text": "again.", "sample_rate": 24000, "encoding": "f32le", "container": "raw"})
    assert r2.status_code == 200 and r2.content == r.content and svc.texts[-1] == "again."


@pytest.mark.parametrize("body", [{"sample_rate": 22050}, {"sample_rate": 44100}, {"sample_rate": 0}, {"sample_rate": -8000},
                                  {"sample_rate": "fast"}, {"encoding": "s16be"}, {"encoding": "mulaw"}, {"encoding": 16},
                                  {"container": "ogg"}, {"container": "WAV"}, {"sample_rate": 16000, "encoding": "u8"}])
def test_invalid_audio_fields_give_422(body):
    svc = _AudioService()
    r = _client(svc).post("/tts", json=dict(body, text="hello."))
    assert r.status_code == 422
    assert not svc.texts  # nothing was submitted


def test_format_fields_reach_submit_and_the_response_says_what_it_carries():
    svc = _AudioService()
    c = _client(svc)
    r = c.post("/tts", json={"text": "hi.", "sample_rate": 16000, "encoding": "s16le"})
    assert r.status_code == 200 and svc.kwargs[-1] == {"audio": A.AudioFormat(16000, "s16le", "raw")}
    assert r.headers["content-type"] == "application/octet-stream"
    assert r.headers["x-audio-sample-rate"] == "16000" and r.headers["x-audio-encoding"] == "s16le"
    assert np.frombuffer(r.content, dtype="<i2").size == 16 * 6
    r = c.post("/tts", json={"text": "hi.", "container": "wav", "sample_rate": 48000})
    assert svc.kwargs[-1] == {"audio": A.AudioFormat(48000, "f32le", "wav")}
    assert r.headers["content-type"] == "audio/wav"
    assert r.headers["x-audio-sample-rate"] == "48000" and r.headers["x-audio-encoding"] == "f32le"
    assert r.content[:44] == A.wav_header(A.AudioFormat(48000, "f32le", "wav"))  # the header is first
    assert np.frombuffer(r.content[44:], dtype="<f4").size == 16 * 6
    c.post("/tts", json={"text": "plain."})
    assert svc.kwargs[-1] == {}  # no format named, none passed
    # sampling and audio fields together
    c.post("/tts", json={"text": "both.", "temperature": 0.5, "seed": 3, "encoding": "s16le"})
    assert set(svc.kwargs[-1]) == {"sampling", "audio"} and svc.kwargs[-1]["audio"] == A.AudioFormat(24000, "s16le")


def test_server_defaults():
    from llmvox_amd.server import create_app
    svc = _AudioService()
    c = _client(svc, sample_rate=8000, encoding="s16le", container="wav")
    r = c.post("/tts", json={"text": "hi."})
    assert svc.kwargs[-1] == {"audio": A.AudioFormat(8000, "s16le", "wav")} and r.headers["content-type"] == "audio/wav"
    assert r.headers["x-audio-sample-rate"] == "8000" and r.content[:44] == A.wav_header(A.AudioFormat(8000, "s16le", "wav"))
    r = c.post("/tts", json={"text": "hi.", "container": "raw", "sample_rate": 24000, "encoding": "f32le"})
    assert svc.kwargs[-1] == {} and r.headers["content-type"] == "application/octet-stream"
    with pytest.raises(ValueError):
        create_app(svc, sample_rate=11025)


def test_service_streams_a_wav_of_the_converted_sentence():
    from llmvox_amd.server import TTSService
    from test_scheduler_audio import AudioEngine
    eng = AudioEngine(max_streams=4, max_positions=4096)
    svc = TTSService([eng], max_chunk=16, max_tokens=55)  # (the request stops between two dumps: it has a tail)
    fmt = A.AudioFormat(16000, "s16le", "wav")
    try:
        plain = b"".join(svc.chunks(svc.submit("Hello there."), timeout=0.01))
        assert not [c for c in eng.log if c[0].startswith("pcm_")]
        items = list(svc.chunks(svc.submit("Hello there.", audio=fmt), timeout=0.01))
        wav_only = b"".join(svc.chunks(svc.submit("Hello there.", audio=A.AudioFormat(container="wav")), timeout=0.01))
        boundary = TTSService([AudioEngine(max_streams=4, max_positions=4096)], max_chunk=16, max_tokens=40)
        try:  # (40 = 10 + 30: the request stops on a dump boundary; the filter is still flushed)
            plain40 = b"".join(boundary.chunks(boundary.submit("Hello there."), timeout=0.01))
            conv40 = b"".join(boundary.chunks(boundary.submit("Hello there.", audio=A.AudioFormat(16000, "s16le")),
                                              timeout=0.01))
        finally:
            boundary.shutdown()
    finally:
        svc.shutdown()
    x = np.frombuffer(plain, dtype="<f4")
    assert x.size % 320 == 0 and 40 * 320 < x.size < 130 * 320  # the dumps of 10 and 30 frames, then a tail
    assert items[0] == A.wav_header(fmt) and len(items) > 2
    got = np.frombuffer(b"".join(items[1:]), dtype="<i2")
    assert got.size == -(-x.size * 2 // 3) and np.array_equal(got, A.convert_ref(x, fmt))
    finals = [c[1] for c in eng.log if c[0] == "pcm_convert" and c[3]]
    assert finals and len(set(finals)) == len(finals)  # one sentence per fed replica, one final each (its tail)
    assert wav_only == A.wav_header(A.AudioFormat(container="wav")) + plain
    x40 = np.frombuffer(plain40, dtype="<f4")
    assert x40.size == 40 * 320
    assert np.array_equal(np.frombuffer(conv40, dtype="<i2"), A.convert_ref(x40, A.AudioFormat(16000, "s16le")))
