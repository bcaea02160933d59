"""The ``formant`` field of POST /tts with a fake service (CPU): it reaches ``submit`` in the request's AudioFormat as
``formant_pct``, the response says by which factor the spectral envelope moved in ``X-Audio-Formant``, a bool, a
non-number, a non-finite or an out-of-range value is a 422 and so is a combination whose correction falls outside
1/2 .. 2, ``--formant`` sets the default, and a request without it reaches the service as it always did."""
import pytest

from llmvox_amd import audio as A
from test_server_audio import _AudioService, _TextOnlyService, _client


def test_field_and_header_round_trip():
    svc = _AudioService()
    c = _client(svc)
    r = c.post("/tts", json={"text": "hi.", "formant": 0.9})
    assert r.status_code == 200 and svc.kwargs[-1] == {"audio": A.AudioFormat(formant_pct=90)}
    assert r.headers["x-audio-formant"] == "0.9000" and r.headers["content-type"] == "application/octet-stream"
    assert r.headers["x-audio-pitch"] == "1.0000" and r.headers["x-audio-volume"] == "1.00" and r.headers["x-audio-speed"] == "1.00"
    # with a pitch: f0 moves by the realised ratio, the envelope by the named factor
    r = c.post("/tts", json={"text": "hi.", "pitch": 1.25, "formant": 1.0})
    fmt = A.AudioFormat(pitch_pct=125, formant_pct=100)
    assert r.status_code == 200 and svc.kwargs[-1] == {"audio": fmt} and fmt.formant == (5, 4)
    assert r.headers["x-audio-pitch"] == "1.2500" and r.headers["x-audio-formant"] == "1.0000"
    # without the field the envelope follows the pitch: the header carries the realised pitch ratio
    r = c.post("/tts", json={"text": "hi.", "pitch": 1.25})
    assert svc.kwargs[-1] == {"audio": A.AudioFormat(pitch_pct=125)}
    assert r.headers["x-audio-formant"] == r.headers["x-audio-pitch"] == "1.2500"
    r = c.post("/tts", json={"text": "hi.", "pitch": 0.9, "speed": 1.3})  # stretch 144: 130 / 144
    assert r.headers["x-audio-formant"] == r.headers["x-audio-pitch"] == f"{130 / 144:.4f}"
    # everything at once
    r = c.post("/tts", json={"text": "hi.", "formant": 1.1, "speed": 1.3, "pitch": 0.9, "sample_rate": 16000,
                             "encoding": "s16le", "container": "wav", "join": True, "volume": 2.5})
    fmt = A.AudioFormat(16000, "s16le", "wav", 130, 90, True, 250, 110)
    assert r.status_code == 200 and svc.kwargs[-1] == {"audio": fmt} and r.headers["x-audio-formant"] == "1.1000"
    assert r.content[:44] == A.wav_header(fmt) and r.headers["content-type"] == "audio/wav"
    for enc, media in (("flac", "audio/flac"), ("ulaw", "application/octet-stream"), ("alaw", "application/octet-stream")):
        r = c.post("/tts", json={"text": "hi.", "formant": 0.8, "encoding": enc, "sample_rate": 8000})
        assert r.status_code == 200 and svc.kwargs[-1] == {"audio": A.AudioFormat(8000, enc, formant_pct=80)}
        assert r.headers["content-type"] == media and r.headers["x-audio-formant"] == "0.8000"
    for value, pct, header in ((0.5, 50, "0.5000"), (2, 200, "2.0000"), (2.0, 200, "2.0000"), (1, 100, "1.0000"),
                               (0.496, 50, "0.5000"), (2.004, 200, "2.0000"), (1.006, 101, "1.0100")):
        r = c.post("/tts", json={"text": "hi.", "formant": value})
        assert r.status_code == 200 and svc.kwargs[-1] == {"audio": A.AudioFormat(formant_pct=pct)}, value
        assert r.headers["x-audio-formant"] == header


def test_a_request_without_the_field_reaches_the_service_as_before():
    svc = _AudioService()
    c = _client(svc)
    for body in ({"text": "plain."}, {"text": "plain.", "formant": None}):
        r = c.post("/tts", json=body)
        assert r.status_code == 200 and svc.kwargs[-1] == {} and r.headers["x-audio-formant"] == "1.0000"
    # the other fields build the formats they built: seven fields, the eighth left alone
    r = c.post("/tts", json={"text": "hi.", "volume": 0.333, "speed": 1.3, "pitch": 0.9, "sample_rate": 16000,
                             "encoding": "s16le", "container": "wav", "join": True})
    assert svc.kwargs[-1] == {"audio": A.AudioFormat(16000, "s16le", "wav", 130, 90, True, 33)}
    assert svc.kwargs[-1]["audio"].formant_pct is None
    # ... also a service that knows nothing of formats
    old = _TextOnlyService()
    r = _client(old).post("/tts", json={"text": "as ever."})
    assert r.status_code == 200 and old.texts == ["as ever."] and r.headers["x-audio-formant"] == "1.0000"


@pytest.mark.parametrize("value", [True, False, "dark", "1.0", [], {}, [1.0], 0.49, 0.494, 0, -1, 2.006, 2.5, 100, 1e9, -1e9],
                         ids=repr)
def test_a_bad_formant_is_a_422(value):
    svc = _AudioService()
    r = _client(svc).post("/tts", json={"text": "hello.", "formant": value})
    assert r.status_code == 422
    assert not svc.texts  # nothing was submitted


@pytest.mark.parametrize("literal", ["NaN", "Infinity", "-Infinity", "1e999"])
def test_a_non_finite_formant_is_a_422(literal):
    svc = _AudioService()
    r = _client(svc).post("/tts", content='{"text": "hello.", "formant": %s}' % literal,
                          headers={"content-type": "application/json"})
    assert r.status_code == 422
    assert not svc.texts


@pytest.mark.parametrize("body", [dict(pitch=2.0, formant=0.5), dict(pitch=0.5, formant=2.0), dict(pitch=1.5, formant=0.7),
                                  dict(pitch=0.6, formant=1.3), dict(speed=2.0, pitch=2.0, formant=0.9)], ids=repr)
def test_a_correction_outside_half_to_two_is_a_422(body):
    svc = _AudioService()
    r = _client(svc).post("/tts", json={"text": "hello.", **body})
    assert r.status_code == 422 and "outside 1/2 .. 2" in r.text
    assert not svc.texts
    # each field alone is fine
    for k, v in body.items():
        assert _client(svc).post("/tts", json={"text": "hello.", k: v}).status_code == 200


def test_formant_pct_of():
    from llmvox_amd.server import formant_pct_of
    assert [formant_pct_of(v) for v in (0.5, 1, 1.0, 0.9, 2, 2.0, 1.125, 1.135, None)] == [50, 100, 100, 90, 200, 200, 112, 114, None]
    for bad in (True, False, "1.0", float("nan"), float("inf"), -float("inf"), 0.494, 2.006, 0, [1.0]):
        with pytest.raises(ValueError):
            formant_pct_of(bad)


def test_formant_default_of_the_server():
    from llmvox_amd import server
    svc = _AudioService()
    c = _client(svc, formant=1.0, pitch=1.25)
    r = c.post("/tts", json={"text": "hi."})
    assert svc.kwargs[-1] == {"audio": A.AudioFormat(pitch_pct=125, formant_pct=100)} and r.headers["x-audio-formant"] == "1.0000"
    r = c.post("/tts", json={"text": "hi.", "formant": 0.9, "pitch": 1.0})
    assert svc.kwargs[-1] == {"audio": A.AudioFormat(formant_pct=90)} and r.headers["x-audio-formant"] == "0.9000"
    r = c.post("/tts", json={"text": "hi.", "formant": None})  # null is "the default", as for every other field
    assert svc.kwargs[-1] == {"audio": A.AudioFormat(pitch_pct=125, formant_pct=100)}
    r = c.post("/tts", json={"text": "hi.", "pitch": 0.4 + 0.05})  # the default formant with this pitch: rho = 0.45
    assert r.status_code == 422
    for bad in (dict(formant=0.4), dict(formant=2.5), dict(formant=float("nan")), dict(formant=True), dict(formant="1"),
                dict(formant=0.5, pitch=2.0)):
        with pytest.raises(ValueError):
            server.create_app(svc, **bad)
    # the command line reaches create_app
    d = server.app_options(server.arg_parser().parse_args(["--formant", "1.0", "--pitch", "0.8"]))
    assert (d["formant"], d["pitch"]) == (1.0, 0.8)
    assert server.app_options(server.arg_parser().parse_args([]))["formant"] is None
    r = _client(svc, **d).post("/tts", json={"text": "hi."})
    assert svc.kwargs[-1] == {"audio": A.AudioFormat(pitch_pct=80, formant_pct=100)} and r.headers["x-audio-formant"] == "1.0000"
    assert r.headers["x-audio-pitch"] == "0.8000"
    # the defaults of the server without the option are those of before
    r = _client(svc).post("/tts", json={"text": "hi."})
    assert svc.kwargs[-1] == {} and r.headers["x-audio-formant"] == "1.0000"
