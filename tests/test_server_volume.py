"""The ``volume`` field of POST /tts with a fake service (CPU): it reaches ``submit`` in the request's AudioFormat as
``volume_pct``, the response says so in ``X-Audio-Volume``, a bool, a non-number, a non-finite or an out-of-range value
is a 422, ``--volume`` sets the default, and a request without it (or with 1.0) reaches the service as it always did."""
import pytest

from llmvox_amd import audio as A
from test_server_audio import _AudioService, _TextOnlyService, _client


def test_field_and_header_round_trip():
    svc = _AudioService()
    c = _client(svc)
    r = c.post("/tts", json={"text": "hi.", "volume": 2.5})
    assert r.status_code == 200 and svc.kwargs[-1] == {"audio": A.AudioFormat(volume_pct=250)}
    assert r.headers["x-audio-volume"] == "2.50" and r.headers["content-type"] == "application/octet-stream"
    assert r.headers["x-audio-sample-rate"] == "24000" and r.headers["x-audio-encoding"] == "f32le"
    assert r.headers["x-audio-speed"] == "1.00" and r.headers["x-audio-pitch"] == "1.0000" and r.headers["x-audio-join"] == "0"
    r = c.post("/tts", json={"text": "hi.", "volume": 0.333, "speed": 1.3, "pitch": 0.9, "sample_rate": 16000,
                             "encoding": "s16le", "container": "wav", "join": True})
    fmt = A.AudioFormat(16000, "s16le", "wav", 130, 90, True, 33)
    assert r.status_code == 200 and svc.kwargs[-1] == {"audio": fmt} and r.headers["x-audio-volume"] == "0.33"
    assert r.content[:44] == A.wav_header(fmt) and r.headers["content-type"] == "audio/wav"
    for value, pct, header in ((0, 0, "0.00"), (0.0, 0, "0.00"), (4, 400, "4.00"), (4.0, 400, "4.00"), (3, 300, "3.00"),
                               (0.004, 0, "0.00"), (4.004, 400, "4.00"), (1.006, 101, "1.01")):
        r = c.post("/tts", json={"text": "hi.", "volume": value})
        assert r.status_code == 200 and svc.kwargs[-1] == {"audio": A.AudioFormat(volume_pct=pct)}, value
        assert r.headers["x-audio-volume"] == header
    # no volume, or 1.0: the request reaches the service exactly as it always did
    for body in ({"text": "plain."}, {"text": "plain.", "volume": 1.0}, {"text": "plain.", "volume": 1}, {"text": "plain.", "volume": 1.004},
                 {"text": "plain.", "volume": None}):
        r = c.post("/tts", json=body)
        assert r.status_code == 200 and svc.kwargs[-1] == {} and r.headers["x-audio-volume"] == "1.00"
    # ... also a service that knows nothing of formats
    old = _TextOnlyService()
    r = _client(old).post("/tts", json={"text": "as ever.", "volume": 1.0})
    assert r.status_code == 200 and old.texts == ["as ever."] and r.headers["x-audio-volume"] == "1.00"


@pytest.mark.parametrize("value", [True, False, "loud", "2.0", [], {}, [2.0], -0.1, -1, 4.006, 4.5, 5, 400, 1e9, -1e9],
                         ids=repr)
def test_a_bad_volume_is_a_422(value):
    svc = _AudioService()
    r = _client(svc).post("/tts", json={"text": "hello.", "volume": value})
    assert r.status_code == 422
    assert not svc.texts  # nothing was submitted


@pytest.mark.parametrize("literal", ["NaN", "Infinity", "-Infinity", "1e999"])
def test_a_non_finite_volume_is_a_422(literal):
    svc = _AudioService()
    r = _client(svc).post("/tts", content='{"text": "hello.", "volume": %s}' % literal,
                          headers={"content-type": "application/json"})
    assert r.status_code == 422
    assert not svc.texts


def test_volume_pct_of():
    from llmvox_amd.server import volume_pct_of
    assert [volume_pct_of(v) for v in (0, 0.0, 0.5, 1, 1.0, 2.5, 4, 4.0, 0.125, 0.135)] == [0, 0, 50, 100, 100, 250, 400, 400, 12, 14]
    for bad in (True, False, "1.0", None, float("nan"), float("inf"), -float("inf"), -0.006, 4.006, [1.0]):
        with pytest.raises(ValueError):
            volume_pct_of(bad)


def test_volume_default_of_the_server():
    from llmvox_amd import server
    svc = _AudioService()
    c = _client(svc, volume=1.5)
    r = c.post("/tts", json={"text": "hi."})
    assert svc.kwargs[-1] == {"audio": A.AudioFormat(volume_pct=150)} and r.headers["x-audio-volume"] == "1.50"
    r = c.post("/tts", json={"text": "hi.", "volume": 1.0})
    assert svc.kwargs[-1] == {} and r.headers["x-audio-volume"] == "1.00"
    r = c.post("/tts", json={"text": "hi.", "volume": 0.5, "encoding": "s16le"})
    assert svc.kwargs[-1] == {"audio": A.AudioFormat(24000, "s16le", volume_pct=50)}
    for bad in (dict(volume=-0.5), dict(volume=4.5), dict(volume=float("nan")), dict(volume=True), dict(volume="2")):
        with pytest.raises(ValueError):
            server.create_app(svc, **bad)
    # the command line reaches create_app
    d = server.app_options(server.arg_parser().parse_args(["--volume", "2.5", "--speed", "0.9"]))
    assert (d["volume"], d["speed"]) == (2.5, 0.9)
    assert server.app_options(server.arg_parser().parse_args([]))["volume"] == 1.0
    r = _client(svc, **d).post("/tts", json={"text": "hi."})
    assert svc.kwargs[-1] == {"audio": A.AudioFormat(speed_pct=90, volume_pct=250)} and r.headers["x-audio-volume"] == "2.50"
    # the defaults of the server without the option are those of before
    r = _client(svc).post("/tts", json={"text": "hi."})
    assert svc.kwargs[-1] == {} and r.headers["x-audio-volume"] == "1.00"
