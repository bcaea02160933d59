"""FusedScheduler with streams that ask for FLAC, on the CPU stand-in engine of test_scheduler_g711.py (rows of the
encoding's own dtype: uint8 slots for FLAC): every sentence delivers whole slots which, finished by ``audio.FlacMux``
and decoded by tests/flac_decode.py, are exactly the s16le samples of the same stream; the bucket key keeps FLAC rows
apart; a stream without ``audio`` beside them sees the items it always saw, and a run without FLAC logs the calls it
always logged."""
import numpy as np
import pytest
import torch

import flac_decode as D
import test_scheduler_g711 as G
from llmvox_amd import audio as A
from test_scheduler_audio import _same_events, _segments


@pytest.fixture(autouse=True)
def _flac_rows(monkeypatch):
    monkeypatch.setitem(G._TORCH, "flac", torch.uint8)  # (the stand-in's dtype table knows the four older encodings)


def _decode_stream(events, rate):
    """The stream's items through one FlacMux, in order: (samples per sentence, all samples, the frames)."""
    mux, data, per = A.FlacMux(rate), [], []
    for items, _ in _segments(events):
        assert all(i.dtype == np.uint8 and i.size % A.flac_slot_bytes(rate) == 0 for i in items)
        first = mux.sample_no
        data.append(b"".join(mux.push(i) for i in items))
        per.append(D.decode(data[-1], first_sample=first, header=False, rate=rate)[0])
    whole, frames = D.decode(mux.header() + b"".join(data))
    return per, whole, frames


@pytest.mark.parametrize("overlap", [False, True], ids=["serial", "overlap"])
@pytest.mark.parametrize("rate", [8000, 24000])
def test_flac_stream_decodes_to_the_s16le_stream(overlap, rate):
    fmt = A.AudioFormat(rate, "flac")
    _, plain = G._run(overlap, [None, None])
    log, mixed = G._run(overlap, [None, fmt])
    log16, as16 = G._run(overlap, [None, A.AudioFormat(rate, "s16le")])
    assert mixed[0][2] == plain[0][2] and mixed[1][2] == plain[1][2] == as16[1][2]  # the same tokens
    _same_events(mixed[0][1], plain[0][1])  # the stream beside it sees what it always saw
    per, whole, frames = _decode_stream(mixed[1][1], rate)
    segs16 = _segments(as16[1][1])
    assert len(per) == len(segs16) >= 3
    bs = rate // 25
    for got, (items16, ended) in zip(per, segs16):
        want = np.concatenate(items16)
        if ended:  # a whole sentence: every sample of the s16le stream, exactly
            assert np.array_equal(got, want)
        else:      # the run stopped inside it: the whole frames so far
            assert got.size == max(0, (want.size - 16) // bs) * bs and np.array_equal(got, want[:got.size])
    assert frames and frames[0][0] == 0  # (decode() has held the numbers contiguous and the sizes to STREAMINFO)
    assert whole.size == sum(p.size for p in per)
    # the slot's calls are those of the s16le stream: the format changes no call's inputs or finals
    calls = [c[:4] for c in log if c[0] == "pcm_convert" and c[1] == mixed[1][0]]
    assert calls == [c[:4] for c in log16 if c[0] == "pcm_convert" and c[1] == as16[1][0]]


def test_flac_rows_are_a_bucket_of_their_own():
    fmts = [A.AudioFormat(8000, "flac"), A.AudioFormat(8000, "s16le"), A.AudioFormat(8000, "flac"), A.AudioFormat(8000, "ulaw")]
    log, out = G._run(True, fmts)
    slot_enc = {o[0]: f.encoding for o, f in zip(out, fmts)}
    calls = [c for c in log if c[0] == "pcm_call"]
    assert calls
    for _, slots, enc in calls:
        assert {slot_enc[s] for s in slots} == {enc}
    flac = {s for s, e in slot_enc.items() if e == "flac"}
    assert any(set(slots) == flac for _, slots, _ in calls)
    for o, f in zip(out, fmts):
        if f.encoding == "flac":
            _decode_stream(o[1], 8000)


def test_a_run_without_flac_logs_what_it_logged():
    fmts = [None, A.AudioFormat(8000, "ulaw"), A.AudioFormat(16000, "s16le")]
    log_a, out_a = G._run(True, fmts)
    log_b, out_b = G._run(True, fmts + [A.AudioFormat(8000, "flac")])
    slots = {o[0] for o in out_a}
    keep = [c for c in log_b if (c[0] == "pcm_call" and set(c[1]) <= slots) or (c[0] != "pcm_call" and c[1] in slots)]
    assert keep == log_a
    for a, b in zip(out_a, out_b):
        _same_events(a[1], b[1])


def test_bytes_are_the_slots():
    fmt = A.AudioFormat(8000, "flac")
    _, arr = G._run(True, [fmt], to_bytes=False)
    _, byt = G._run(True, [fmt], to_bytes=True)
    assert len(arr[0][1]) == len(byt[0][1])
    for a, b in zip(arr[0][1], byt[0][1]):
        if isinstance(a, np.ndarray):
            assert isinstance(b, bytes) and b == a.tobytes()
        else:
            assert a == b
