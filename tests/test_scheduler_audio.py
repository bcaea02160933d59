"""FusedScheduler with streams that ask for another audio format, on a CPU stand-in engine whose
``pcm_convert`` is the numpy statement of the rule (llmvox_amd/audio.py) and which records its calls:
what each sentence delivers, which dumps are final, the order of a slot's calls, and that a stream
without ``audio`` never reaches the output stage and sees the items it always saw."""
import numpy as np
import pytest
import torch

from llmvox_amd import audio as A
from llmvox_amd import streaming as S
from test_service_multidevice import StateEngine

TEXT = "The quick brown fox jumps over the lazy dog. Then it sleeps near the river bank. The end."
EOA = 4000  # the stand-in emits it at every position divisible by 41: segments end mid-chunk
FMT = A.AudioFormat(16000, "s16le")
_W = np.random.default_rng(5).uniform(-1, 1, 320).astype(np.float32)  # the stand-in codec's frame shape


class AudioEngine(StateEngine):
    """StateEngine + a codec whose PCM lies in [-1, 1] and varies inside a frame, the output stage from
    the numpy reference (one StreamRef per slot) and the log of the calls that matter here."""

    def __init__(self, **kw):
        super().__init__(**kw)
        self.log = []
        self.refs = {}

    def reset_slot(self, slot):
        self.log.append(("reset_slot", slot))
        super().reset_slot(slot)

    def decode_codes(self, codes, bandwidth_id=0, out=None):
        amp = codes.float() / 2048.0 - 1.0
        return (amp[:, :, None] * torch.from_numpy(_W)[None, None, :]).reshape(codes.shape[0], -1)

    def pcm_reset(self, slot):
        self.log.append(("pcm_reset", slot))
        self.refs.pop(slot, None)

    def pcm_convert(self, pcm, slots, finals, fmt):
        n_in = 0 if pcm is None else int(pcm.shape[1])
        assert len(set(slots)) == len(slots), "a slot named twice in one call"
        outs = []
        for b, (slot, final) in enumerate(zip(slots, finals)):
            self.log.append(("pcm_convert", slot, n_in, bool(final), fmt.sample_rate, fmt.encoding))
            ref = self.refs.setdefault(slot, A.StreamRef(fmt))
            assert (ref.fmt.sample_rate, ref.fmt.encoding) == (fmt.sample_rate, fmt.encoding)
            outs.append(ref.push(pcm[b].numpy() if n_in else np.zeros(0, np.float32), bool(final)))
        width = max(8, max(o.size for o in outs) + 3)  # (rows are wider than their counts, as the device's are)
        out = torch.full((len(slots), width), 77, dtype=torch.int16 if fmt.encoding == "s16le" else torch.float32)
        for b, o in enumerate(outs):
            out[b, :o.size] = torch.from_numpy(o.copy())
        return out, [o.size for o in outs]


def _run(overlap, audios, eoa=EOA, to_bytes=False, n_tokens=150, **machine_kw):
    eng = AudioEngine(max_streams=4, max_positions=4096, eoa=eoa)
    sch = S.FusedScheduler(eng, max_chunk=16, to_bytes=to_bytes, overlap=overlap,
                           stop_rule=lambda st, ntok, pos: ntok >= n_tokens)
    sts = []
    for i, fmt in enumerate(audios):
        kw = dict(machine_kw)
        if eoa is not None:
            kw["eoa_id"] = eoa
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
    return eng.log, out


def _segments(events):
    """[(items of the sentence, ended by a signal?)]"""
    segs, cur = [], []
    for e in events:
        if isinstance(e, (bytes, np.ndarray)):
            cur.append(e)
        else:
            segs.append((cur, True))
            cur = []
    if cur:
        segs.append((cur, False))
    return segs


def _same_events(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        if isinstance(x, np.ndarray):
            assert isinstance(y, np.ndarray) and x.dtype == y.dtype and np.array_equal(x, y)
        else:
            assert type(x) is type(y) and x == y


def _check_stream(log, slot, events, plain_events, fmt):
    segs, plain = _segments(events), _segments(plain_events)
    assert len(segs) == len(plain) and len(segs) >= 3
    rate = fmt.sample_rate
    for (items, ended), (pitems, pended) in zip(segs, plain):
        assert ended == pended
        x = np.concatenate(pitems)
        got = np.concatenate(items)
        assert got.dtype == fmt.dtype and all(i.dtype == fmt.dtype for i in items)
        want = A.convert_ref(x, fmt)
        if ended:  # a whole sentence: exactly ceil(T L / M) samples, those of the one-shot conversion
            assert got.size == want.size == -(-x.size * A.RATES[rate][0] // A.RATES[rate][1])
            assert np.array_equal(got, want)
        else:      # the run stopped inside it: what the filter could emit so far
            assert got.size == A.emitted_upto(rate, x.size, False) and np.array_equal(got, want[:got.size])
    # the slot's calls: one per dump, in dump order, final exactly at the sentences' ends
    calls = [c for c in log if c[0] == "pcm_convert" and c[1] == slot]
    want_calls = []
    for pitems, pended in plain:
        for k, p in enumerate(pitems):
            want_calls.append((p.size, pended and k == len(pitems) - 1))
    assert [(c[2], c[3]) for c in calls] == want_calls
    assert sum(c[3] for c in calls) == sum(1 for _, ended in segs if ended)
    assert all(c[4:] == (fmt.sample_rate, fmt.encoding) for c in calls)


@pytest.mark.parametrize("overlap", [False, True], ids=["serial", "overlap"])
def test_converted_stream_delivers_the_rule_per_sentence(overlap):
    log0, plain = _run(overlap, [None, None])
    assert not [c for c in log0 if c[0].startswith("pcm_")]  # no audio format: the stage is never reached
    log, mixed = _run(overlap, [None, FMT])
    assert mixed[0][2] == plain[0][2] and mixed[1][2] == plain[1][2]  # the same tokens
    _same_events(mixed[0][1], plain[0][1])  # the stream beside it sees what it always saw
    assert not [c for c in log if c[0].startswith("pcm_") and c[1] == mixed[0][0]]
    slot = mixed[1][0]
    _check_stream(log, slot, mixed[1][1], plain[1][1], FMT)
    # opened: reset behind reset_slot; closed: reset again
    mine = [c for c in log if c[1] == slot and c[0] in ("reset_slot", "pcm_reset", "pcm_convert")]
    assert mine[0] == ("reset_slot", slot) and mine[1] == ("pcm_reset", slot) and mine[2][0] == "pcm_convert"
    assert mine[-1] == ("pcm_reset", slot) and [c[0] for c in mine].count("pcm_reset") == 2


@pytest.mark.parametrize("fmt", [A.AudioFormat(8000, "f32le"), A.AudioFormat(48000, "s16le"), A.AudioFormat(24000, "s16le"),
                                 A.AudioFormat(16000, "f32le", "wav")], ids=lambda f: f"{f.sample_rate}-{f.encoding}")
def test_other_formats_and_two_converting_streams(fmt):
    _, plain = _run(True, [None, None])
    log, both = _run(True, [FMT, fmt])
    _check_stream(log, both[0][0], both[0][1], plain[0][1], FMT)
    _check_stream(log, both[1][0], both[1][1], plain[1][1], fmt)


@pytest.mark.parametrize("overlap", [False, True], ids=["serial", "overlap"])
def test_sentence_ended_by_the_length_reset_is_flushed(overlap):
    """No end of audio: the sentence ends when its undumped outputs pass max_audio_length, and they are
    dropped: no dump follows the sentence's last audio, so a flush-only call ends it."""
    kw = dict(eoa=None, max_audio_len=50, n_tokens=200)
    _, plain = _run(overlap, [None], **kw)
    log, conv = _run(overlap, [FMT], **kw)
    assert conv[0][2] == plain[0][2]
    flushes = [c for c in log if c[0] == "pcm_convert" and c[2] == 0]
    assert flushes and all(c[3] for c in flushes)
    segs, psegs = _segments(conv[0][1]), _segments(plain[0][1])
    assert len(segs) == len(psegs) >= 2
    n_final = 0
    for (items, ended), (pitems, pended) in zip(segs, psegs):
        assert ended == pended
        if not pitems:  # (a sentence whose outputs were all dropped: nothing to flush)
            assert not items
            continue
        want = A.convert_ref(np.concatenate(pitems), FMT)
        got = np.concatenate(items)
        if ended:
            n_final += 1
            assert len(items) == len(pitems) + 1  # the flush's samples are an item of their own
            assert np.array_equal(got, want)
        else:
            assert np.array_equal(got, want[:got.size])
    assert sum(c[3] for c in log if c[0] == "pcm_convert") == n_final


def test_bytes_are_the_arrays_bytes():
    _, arr = _run(True, [FMT], to_bytes=False)
    _, byt = _run(True, [FMT], to_bytes=True)
    assert len(arr[0][1]) == len(byt[0][1])
    for a, b in zip(arr[0][1], byt[0][1]):
        if isinstance(a, np.ndarray):
            assert isinstance(b, bytes) and b == a.astype("<i2").tobytes()
        else:
            assert a == b


def test_default_format_is_no_format():
    for fmt in (A.AudioFormat(), A.AudioFormat(container="wav")):  # (the header is the service's business)
        log, out = _run(True, [fmt])
        assert not [c for c in log if c[0].startswith("pcm_")]
        _, plain = _run(True, [None])
        _same_events(out[0][1], plain[0][1])


def test_engine_without_pcm_convert_raises_at_open_stream():
    sch = S.FusedScheduler(StateEngine(max_streams=2), max_chunk=8, to_bytes=False, overlap=False)
    free = list(sch.free_slots)
    with pytest.raises(RuntimeError, match="pcm_convert"):
        sch.open_stream(index=0, dump_size=10, audio=FMT)
    assert sch.free_slots == free and not sch.streams  # nothing was taken
    st = sch.open_stream(index=0, dump_size=10, audio=A.AudioFormat())  # the default needs no stage
    st.feed("Hello.")
    assert sch.run_chunk() > 0
    sch.close_stream(st)
    sch.close()


def test_a_slots_calls_keep_dump_order_across_codec_groups():
    """Two dumps of one stream in one decode, the later one in the group that is decoded first: its
    conversion waits for the earlier dump's; the other stream's row of that group does not."""
    eng = AudioEngine(max_streams=4)
    sch = S.FusedScheduler(eng, max_chunk=8, to_bytes=False, overlap=False)
    a = sch.open_stream(index=0, dump_size=10, audio=FMT)
    b = sch.open_stream(index=1, dump_size=10, audio=FMT)
    c = sch.open_stream(index=0, dump_size=10)
    dumps = [(b, [7] * 10), (a, [9] * 30), (a, [11] * 10), (c, [5] * 10)]
    del eng.log[:]
    res, err = sch._decode(dumps, {2})
    assert err is None
    calls = [c_[1:4] for c_ in eng.log if c_[0] == "pcm_convert"]
    assert calls == [(b.slot, 3200, False), (a.slot, 9600, False), (a.slot, 3200, True)]
    pcm = eng.decode_codes(torch.tensor([[9] * 30 + [11] * 10])).numpy()[0]
    assert np.array_equal(np.concatenate([res[1], res[2]]), A.convert_ref(pcm, FMT))
    assert res[3].dtype == np.float32 and res[3].size == 3200 and res[0].dtype == np.int16
    for st in (a, b, c):
        sch.close_stream(st)
    sch.close()


def test_failed_stream_gets_a_reset_and_nothing_more():
    eng = AudioEngine(max_streams=2)
    sch = S.FusedScheduler(eng, max_chunk=8, to_bytes=False, overlap=False)
    a = sch.open_stream(index=0, dump_size=10, audio=FMT)
    sch.failed.add(a)
    del eng.log[:]
    res, err = sch._decode([(a, [3] * 10)], set())
    assert res == [None] and [c[0] for c in eng.log] == ["pcm_reset"]
    sch.close_stream(a)
    sch.close()
