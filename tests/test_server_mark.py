"""``watermark`` and ``watermark_id`` of POST /tts (CPU). With fake services: the fields reach submit as the format's
mark, the ``X-Audio-Watermark`` header, the 422 cases (a bool where an integer is meant and the other way round, a
request for a mark of a server without a key), the server's defaults and command line, a server that refuses to start
marking without a key, that the key appears in no response, and that a request which names neither field reaches the
service exactly as before. Then the real TTSService on a stand-in engine: the body of a marked request is the sentences
of the same request, marked; and ``python -m llmvox_amd.watermark detect`` on WAV files of the service's encodings."""
import json

import numpy as np
import pytest

import mark_signals as MS
from llmvox_amd import audio as A
from test_scheduler_audio import EOA
from test_server_g711 import _body_chunks, _client, _FramingService, _TextOnlyService

KEY = MS.KEY
TEXT = "Hello there. How are you. I am fine. Thanks a lot. See you soon."


def _no_key_in(r):
    """No form of the key in a response: its status line apart, every header and the whole body."""
    seen = (r.text + json.dumps(dict(r.headers))).lower()
    return str(KEY) not in seen and hex(KEY)[2:] not in seen and "mark_key" not in seen


def test_the_fields_reach_submit_and_the_header_says_so():
    svc = _FramingService()
    c = _client(svc, watermark_key=KEY, watermark_id=7, watermark_strength=3)
    r = c.post("/tts", json={"text": "hi.", "watermark": True, "encoding": "s16le", "container": "wav"})
    fmt = A.AudioFormat(24000, "s16le", "wav", mark_key=KEY, mark_id=7, mark_strength=3)
    assert r.status_code == 200 and svc.calls == [("submit", "hi.", {"audio": fmt}), ("chunks", {})]
    assert r.headers["x-audio-watermark"] == "1" and _no_key_in(r)
    r = c.post("/tts", json={"text": "hi.", "watermark": True, "watermark_id": 255, "frame_ms": 20})
    assert svc.calls[-2:] == [("submit", "hi.", {"audio": A.AudioFormat(mark_key=KEY, mark_id=255, mark_strength=3)}),
                              ("chunks", {"frame_ms": 20})]
    assert r.headers["x-audio-watermark"] == "1" and _no_key_in(r)
    r = c.post("/tts", json={"text": "hi.", "watermark": True, "watermark_id": 0})
    assert svc.calls[-2][2] == {"audio": A.AudioFormat(mark_key=KEY, mark_id=0, mark_strength=3)}
    # off, by name or by default: no mark, whatever id is named, and the default request reaches submit bare
    for body in ({"watermark": False}, {}, {"watermark": None}, {"watermark_id": 9}, {"watermark": False, "watermark_id": 9}):
        r = c.post("/tts", json=dict(body, text="hi."))
        assert r.status_code == 200 and svc.calls[-2] == ("submit", "hi.", {}) and r.headers["x-audio-watermark"] == "0"
        assert _no_key_in(r)


@pytest.mark.parametrize("body,says", [({"watermark": 1}, "watermark"), ({"watermark": 0}, "watermark"), ({"watermark": "true"}, "watermark"),
                                       ({"watermark": 1.0}, "watermark"), ({"watermark": [True]}, "watermark"),
                                       ({"watermark": True, "watermark_id": True}, "watermark_id"),
                                       ({"watermark": True, "watermark_id": 256}, "watermark_id"),
                                       ({"watermark": True, "watermark_id": -1}, "watermark_id"),
                                       ({"watermark": True, "watermark_id": 7.0}, "watermark_id"),
                                       ({"watermark": True, "watermark_id": "7"}, "watermark_id"),
                                       ({"watermark_id": False}, "watermark_id"), ({"watermark_id": 300}, "watermark_id")])
def test_invalid_values_give_422(body, says):
    svc = _FramingService()
    r = _client(svc, watermark_key=KEY).post("/tts", json=dict(body, text="hello."))
    assert r.status_code == 422 and says in r.text and not svc.calls  # nothing was submitted
    assert _no_key_in(r)


def test_a_server_without_a_key():
    from llmvox_amd.server import create_app, main
    svc = _FramingService()
    c = _client(svc)
    r = c.post("/tts", json={"text": "hi.", "watermark": True})
    assert r.status_code == 422 and "no watermark key" in r.text and not svc.calls
    r = c.post("/tts", json={"text": "hi.", "watermark": False})
    assert r.status_code == 200 and svc.calls[-2] == ("submit", "hi.", {}) and r.headers["x-audio-watermark"] == "0"
    with pytest.raises(ValueError, match="no watermark key"):  # marking by default needs a key: the reason, at start-up
        create_app(svc, watermark=True)
    for bad in (dict(watermark_key=-1), dict(watermark_key=1 << 64), dict(watermark_key=True), dict(watermark_key=1.5),
                dict(watermark_id=256), dict(watermark_id=True), dict(watermark_strength=0), dict(watermark_strength=4),
                dict(watermark=1, watermark_key=KEY)):
        with pytest.raises(ValueError) as ei:
            create_app(svc, **bad)
        assert str(KEY) not in str(ei.value)
    with pytest.raises(SystemExit) as ei:  # the command line: refused before anything is built
        main(["--watermark"])
    assert ei.value.code == 2


def test_server_defaults_and_the_command_line(capsys):
    from llmvox_amd.server import app_options, arg_parser
    svc = _FramingService()
    c = _client(svc, watermark=True, watermark_key=KEY, watermark_id=0xA5)
    r = c.post("/tts", json={"text": "hi."})
    assert svc.calls == [("submit", "hi.", {"audio": A.AudioFormat(mark_key=KEY, mark_id=0xA5)}), ("chunks", {})]
    assert r.headers["x-audio-watermark"] == "1" and _no_key_in(r)
    r = c.post("/tts", json={"text": "hi.", "watermark": False})
    assert svc.calls[-2] == ("submit", "hi.", {}) and r.headers["x-audio-watermark"] == "0"
    r = c.post("/tts", json={"text": "hi.", "watermark_id": 3, "sample_rate": 8000, "encoding": "ulaw"})
    assert svc.calls[-2][2] == {"audio": A.AudioFormat(8000, "ulaw", mark_key=KEY, mark_id=3)}
    for path in ("/", "/health", "/openapi.json"):
        r = c.get(path)
        assert r.status_code == 200 and _no_key_in(r)
    opts = app_options(arg_parser().parse_args(["--watermark", "--watermark-key", hex(KEY), "--watermark-id", "9",
                                                "--watermark-strength", "1"]))
    assert (opts["watermark"], opts["watermark_key"], opts["watermark_id"], opts["watermark_strength"]) == (True, KEY, 9, 1)
    assert app_options(arg_parser().parse_args(["--watermark-key", str(KEY)]))["watermark_key"] == KEY
    opts = app_options(arg_parser().parse_args([]))
    assert (opts["watermark"], opts["watermark_key"], opts["watermark_id"], opts["watermark_strength"]) == (False, None, 0, 2)


def test_a_request_without_the_fields_is_unchanged():
    svc = _TextOnlyService()
    r = _client(svc).post("/tts", json={"text": "hello world."})
    assert r.status_code == 200 and svc.calls == [("submit", "hello world."), ("chunks",)]
    assert r.content == b"".join(_body_chunks()) and r.headers["content-type"] == "application/octet-stream"
    svc = _TextOnlyService()  # a server that holds a key but does not mark by default: still submit(text) alone
    r = _client(svc, watermark_key=KEY).post("/tts", json={"text": "hello world."})
    assert r.status_code == 200 and svc.calls == [("submit", "hello world."), ("chunks",)]
    svc = _FramingService()
    c = _client(svc, watermark_key=KEY)
    c.post("/tts", json={"text": "s16.", "sample_rate": 16000, "encoding": "s16le"})
    c.post("/tts", json={"text": "law.", "sample_rate": 8000, "encoding": "ulaw", "container": "wav", "frame_ms": 20})
    assert svc.calls == [("submit", "s16.", {"audio": A.AudioFormat(16000, "s16le")}), ("chunks", {}),
                         ("submit", "law.", {"audio": A.AudioFormat(8000, "ulaw", "wav")}), ("chunks", {"frame_ms": 20})]
    assert not any(call[2]["audio"].marks for call in svc.calls if call[0] == "submit")


class _Recorder:
    """Keeps, per pcm_convert call of the engine, what went in and what came out of every row."""

    def __init__(self, eng):
        self.rows, inner = [], eng.pcm_convert

        def convert(pcm, slots, finals, fmt):
            out, cnt = inner(pcm, slots, finals, fmt)
            for b, (slot, final) in enumerate(zip(slots, finals)):
                x = np.zeros(0, np.float32) if pcm is None else pcm[b].numpy().copy()
                self.rows.append((slot, bool(final), x, out[b, :cnt[b]].numpy().copy()))
            return out, cnt
        eng.pcm_convert = convert

    def sentences(self):
        """(input samples, output samples) per sentence: a slot's rows up to each final one."""
        open_, done = {}, []
        for slot, final, x, y in self.rows:
            open_.setdefault(slot, []).append((x, y))
            if final:
                rows = open_.pop(slot)
                done.append((np.concatenate([r[0] for r in rows]), np.concatenate([r[1] for r in rows])))
        assert not open_
        return done


def test_service_body_is_the_marked_sentences():
    """The real TTSService on the stand-in engine: every sentence of a marked request is ``convert_ref`` of its own
    samples, marked as a signal of its own from frame 0; the body is made of those sentences; and the engine calls are
    those of the request without the field."""
    from llmvox_amd.server import TTSService
    from test_scheduler_g711 import G711Engine
    eng = G711Engine(max_streams=4, max_positions=4096, eoa=EOA)  # (end-of-audio every 41 positions: sentences end)
    rec = _Recorder(eng)
    svc = TTSService([eng], max_chunk=16, max_tokens=200, eoa_id=EOA)
    plain, fmt = A.AudioFormat(16000, "s16le"), A.AudioFormat(16000, "s16le", mark_key=KEY, mark_id=MS.ID)
    try:
        whole = b"".join(svc.chunks(svc.submit(TEXT, audio=plain), timeout=0.01))
        calls0 = [c for c in eng.log if c[0] == "pcm_convert"]
        del eng.log[:], rec.rows[:]
        marked = b"".join(svc.chunks(svc.submit(TEXT, audio=fmt), timeout=0.01))
        calls = [c for c in eng.log if c[0] == "pcm_convert"]
    finally:
        svc.shutdown()
    sentences = rec.sentences()
    assert len(sentences) >= 4
    for x, y in sentences:
        assert y.dtype == np.int16 and np.array_equal(y, A.convert_ref(x, fmt))
        assert not np.array_equal(y, A.convert_ref(x, plain))
    assert len(marked) == len(whole) == sum(2 * y.size for _, y in sentences) and marked != whole
    assert sorted(marked) == sorted(b"".join(y.tobytes() for _, y in sentences))  # (the replicas' sentences interleave)

    def shape(cs):  # (a request takes whichever two slots are free: they are named by their first appearance)
        names = {}
        return [(names.setdefault(c[1], len(names)),) + c[2:] for c in cs]
    assert shape(calls) == shape(calls0)


def _wav(x, rate, encoding):
    fmt = A.AudioFormat(rate, encoding, "wav")
    return A.wav_header(fmt) + A.convert_ref(x, fmt).tobytes()


@pytest.mark.parametrize("rate,encoding", [(24000, "f32le"), (16000, "s16le"), (8000, "ulaw"), (8000, "alaw"), (48000, "s16le")])
def test_the_command_line_detector(tmp_path, capsys, rate, encoding):
    from llmvox_amd.watermark import main, read_wav
    x = MS.vowel()
    y = A.mark_ref(x, KEY, MS.ID, 2)
    path = tmp_path / "marked.wav"
    path.write_bytes(_wav(y, rate, encoding))
    samples, got_rate, got_enc = read_wav(path.read_bytes())
    assert (got_rate, got_enc) == (rate, encoding) and np.array_equal(samples, MS.delivered(y, rate, encoding))
    assert main(["detect", str(path), "--key", hex(KEY)]) == 0
    out = capsys.readouterr().out
    assert "watermark: found, id 165 (0xa5)" in out and str(KEY) not in out and hex(KEY)[2:] not in out.lower()
    assert main(["detect", str(path), "--key", str(MS.OTHER_KEY)]) == 1
    assert "watermark: not found" in capsys.readouterr().out
    plain = tmp_path / "plain.wav"
    plain.write_bytes(_wav(x, rate, encoding))
    assert main(["detect", str(plain), "--key", str(KEY), "--window-s", "2.0"]) == 1


def test_the_command_line_detector_refuses_what_it_cannot_read(tmp_path, capsys):
    from llmvox_amd.watermark import main, read_wav
    bad = tmp_path / "bad.wav"
    bad.write_bytes(b"fLaC" + bytes(100))
    assert main(["detect", str(bad), "--key", "1"]) == 2 and "not a RIFF" in capsys.readouterr().err
    assert main(["detect", str(tmp_path / "absent.wav"), "--key", "1"]) == 2
    stereo = bytearray(A.wav_header(A.AudioFormat(16000, "s16le", "wav")) + bytes(64))
    stereo[22] = 2
    with pytest.raises(ValueError, match="channel"):
        read_wav(bytes(stereo))
    # a header with real sizes, an odd-sized chunk in front of the data, reads the same samples
    q = (np.arange(100, dtype=np.int16) - 50) * 300
    fmt = A.AudioFormat(8000, "s16le", "wav")
    import struct
    body = q.tobytes()
    sized = (b"RIFF" + struct.pack("<I", 4 + 24 + 8 + 4 + 8 + len(body)) + b"WAVE" + A.wav_header(fmt)[12:36]
             + b"LIST" + struct.pack("<I", 3) + b"abc\0" + b"data" + struct.pack("<I", len(body)) + body)
    got, rate, enc = read_wav(sized)
    assert (rate, enc) == (8000, "s16le") and np.array_equal(got, q.astype(np.float32) / 32768)
