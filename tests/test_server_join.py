"""The ``join`` field of POST /tts with a fake service (CPU): it reaches ``submit`` in the request's
AudioFormat, the response says so in ``X-Audio-Join``, anything but true / false is a 422, ``--join`` sets the
default, and a request without it reaches the service as it always did. Then the real TTSService on a
stand-in engine: a joined request delivers the sample count of a plain one."""
import numpy as np
import pytest

from llmvox_amd import audio as A
from test_server_audio import _AudioService, _client


def test_field_and_header_round_trip():
    svc = _AudioService()
    c = _client(svc)
    r = c.post("/tts", json={"text": "hi.", "join": True})
    assert r.status_code == 200 and svc.kwargs[-1] == {"audio": A.AudioFormat(join=True)}
    assert r.headers["x-audio-join"] == "1" and r.headers["content-type"] == "application/octet-stream"
    assert r.headers["x-audio-sample-rate"] == "24000" and r.headers["x-audio-encoding"] == "f32le"
    r = c.post("/tts", json={"text": "hi.", "join": False})
    assert r.status_code == 200 and svc.kwargs[-1] == {} and r.headers["x-audio-join"] == "0"
    r = c.post("/tts", json={"text": "hi."})
    assert r.status_code == 200 and svc.kwargs[-1] == {} and r.headers["x-audio-join"] == "0"
    r = c.post("/tts", json={"text": "hi.", "join": True, "sample_rate": 16000, "encoding": "s16le", "container": "wav",
                             "speed": 1.3})
    fmt = A.AudioFormat(16000, "s16le", "wav", 130, 100, True)
    assert svc.kwargs[-1] == {"audio": fmt} and r.headers["x-audio-join"] == "1"
    assert r.content[:44] == A.wav_header(fmt) == A.wav_header(A.AudioFormat(16000, "s16le", "wav"))  # the header is unaffected


@pytest.mark.parametrize("value", [1, 0, "true", "yes", 1.0, [], {}, "1"])
def test_a_non_boolean_join_is_a_422(value):
    svc = _AudioService()
    r = _client(svc).post("/tts", json={"text": "hello.", "join": value})
    assert r.status_code == 422
    assert not svc.texts  # nothing was submitted


def test_join_default_of_the_server():
    from llmvox_amd import server
    svc = _AudioService()
    c = _client(svc, join=True)
    r = c.post("/tts", json={"text": "hi."})
    assert svc.kwargs[-1] == {"audio": A.AudioFormat(join=True)} and r.headers["x-audio-join"] == "1"
    r = c.post("/tts", json={"text": "hi.", "join": False})
    assert svc.kwargs[-1] == {} and r.headers["x-audio-join"] == "0"
    with pytest.raises(ValueError):
        server.create_app(svc, join="yes")
    # the command line reaches create_app
    assert server.app_options(server.arg_parser().parse_args(["--join"]))["join"] is True
    assert server.app_options(server.arg_parser().parse_args([]))["join"] is False
    c = _client(svc, **server.app_options(server.arg_parser().parse_args(["--join", "--encoding", "s16le"])))
    c.post("/tts", json={"text": "hi."})
    assert svc.kwargs[-1] == {"audio": A.AudioFormat(24000, "s16le", join=True)}


def test_service_delivers_the_same_count_joined():
    from llmvox_amd.server import TTSService
    from test_scheduler_join import JoinEngine
    svc = TTSService([JoinEngine(max_streams=4, max_positions=4096)], max_chunk=16, max_tokens=55)
    try:
        plain = b"".join(svc.chunks(svc.submit("Hello there."), timeout=0.01))
        joined = b"".join(svc.chunks(svc.submit("Hello there.", audio=A.AudioFormat(join=True)), timeout=0.01))
    finally:
        svc.shutdown()
    x, y = np.frombuffer(plain, dtype="<f4"), np.frombuffer(joined, dtype="<f4")
    assert x.size == y.size and x.size % 320 == 0 and x.size > 40 * 320
    assert np.array_equal(x[:8 * 320], y[:8 * 320]) and not np.array_equal(x, y)  # the seams differ
