"""FusedScheduler with streams that ask for G.711, on the CPU stand-in engine of test_scheduler_audio.py with rows of the
encoding's own dtype (uint8 for G.711): what each sentence delivers, that two streams differing only in their encoding
are two ``pcm_convert`` buckets, that the host copies keep one byte per sample, and that a stream without ``audio`` beside
them sees the items it always saw."""
import numpy as np
import pytest
import torch

from llmvox_amd import audio as A
from llmvox_amd import streaming as S
from test_scheduler_audio import EOA, TEXT, AudioEngine, _check_stream, _same_events, _segments

_TORCH = {"f32le": torch.float32, "s16le": torch.int16, "ulaw": torch.uint8, "alaw": torch.uint8}


class G711Engine(AudioEngine):
    """AudioEngine whose converted rows have the encoding's dtype, as the device's do, and whose log keeps each call's
    slots together: ("pcm_call", slots, encoding) beside the per-row records."""

    def pcm_convert(self, pcm, slots, finals, fmt):
        n_in = 0 if pcm is None else int(pcm.shape[1])
        assert len(set(slots)) == len(slots), "a slot named twice in one call"
        self.log.append(("pcm_call", tuple(slots), fmt.encoding))
        outs = []
        for b, (slot, final) in enumerate(zip(slots, finals)):
            self.log.append(("pcm_convert", slot, n_in, bool(final), fmt.sample_rate, fmt.encoding))
            ref = self.refs.setdefault(slot, A.StreamRef(fmt))
            assert ref.fmt == fmt
            outs.append(ref.push(pcm[b].numpy() if n_in else np.zeros(0, np.float32), bool(final)))
        width = max(16, max(o.size for o in outs) + 3)  # (rows are wider than their counts, as the device's are)
        out = torch.full((len(slots), width), 77, dtype=_TORCH[fmt.encoding])
        for b, o in enumerate(outs):
            out[b, :o.size] = torch.from_numpy(o.copy())
        return out, [o.size for o in outs]


def _run(overlap, audios, to_bytes=False, n_tokens=150):
    """test_scheduler_audio._run on a G711Engine: (the engine's log, per stream (slot, events, tokens))."""
    eng = G711Engine(max_streams=4, max_positions=4096, eoa=EOA)
    sch = S.FusedScheduler(eng, max_chunk=16, to_bytes=to_bytes, overlap=overlap,
                           stop_rule=lambda st, ntok, pos: ntok >= n_tokens)
    sts = []
    for i, fmt in enumerate(audios):
        st = sch.open_stream(index=i, dump_size=10, eoa_id=EOA, **({} if fmt is None else {"audio": fmt}))
        for w in TEXT.split(" "):
            st.feed(w)
        sts.append(st)
    assert sch.run_until_idle(max_chunks=2000) > 0
    out = [(st.slot, list(st.events), list(st.tokens)) for st in sts]
    for st in sts:
        sch.close_stream(st)
    sch.close()
    return eng.log, out


@pytest.mark.parametrize("overlap", [False, True], ids=["serial", "overlap"])
@pytest.mark.parametrize("fmt", [A.AudioFormat(8000, "ulaw"), A.AudioFormat(8000, "alaw"), A.AudioFormat(24000, "ulaw"),
                                 A.AudioFormat(48000, "alaw")], ids=lambda f: f"{f.sample_rate}-{f.encoding}")
def test_g711_stream_delivers_the_rule_per_sentence(overlap, fmt):
    _, plain = _run(overlap, [None, None])
    log, mixed = _run(overlap, [None, fmt])
    assert mixed[0][2] == plain[0][2] and mixed[1][2] == plain[1][2]  # the same tokens
    _same_events(mixed[0][1], plain[0][1])  # the stream beside it sees what it always saw
    _check_stream(log, mixed[1][0], mixed[1][1], plain[1][1], fmt)  # uint8 items, convert_ref's codes, per sentence
    # and those codes are the codes of the same stream run as s16le
    _, as16 = _run(overlap, [None, A.AudioFormat(fmt.sample_rate, "s16le")])
    for (items, _), (items16, _) in zip(_segments(mixed[1][1]), _segments(as16[1][1])):
        assert len(items) == len(items16)
        for i, j in zip(items, items16):
            assert i.dtype == np.uint8 and np.array_equal(i, A.g711_encode(j, fmt.encoding))


def test_streams_differing_only_in_encoding_are_two_buckets():
    fmts = [A.AudioFormat(8000, "ulaw"), A.AudioFormat(8000, "alaw"), A.AudioFormat(8000, "ulaw"), A.AudioFormat(8000, "s16le")]
    log, out = _run(True, fmts)
    slot_enc = {o[0]: f.encoding for o, f in zip(out, fmts)}
    calls = [c for c in log if c[0] == "pcm_call"]
    assert calls
    for _, slots, enc in calls:  # a call carries one encoding's rows only
        assert {slot_enc[s] for s in slots} == {enc}
    # the two mu-law streams do share calls; neither ever shares one with the A-law or the s16le stream
    ulaw = {s for s, e in slot_enc.items() if e == "ulaw"}
    assert any(set(slots) == ulaw for _, slots, _ in calls)
    _, plain = _run(True, [None] * 4)
    for o, p, f in zip(out, plain, fmts):
        _check_stream(log, o[0], o[1], p[1], f)


def test_bytes_are_one_byte_per_sample():
    fmt = A.AudioFormat(8000, "ulaw")
    _, arr = _run(True, [fmt], to_bytes=False)
    _, byt = _run(True, [fmt], to_bytes=True)
    assert len(arr[0][1]) == len(byt[0][1])
    n = 0
    for a, b in zip(arr[0][1], byt[0][1]):
        if isinstance(a, np.ndarray):
            assert a.dtype == np.uint8 and isinstance(b, bytes) and b == a.tobytes() and len(b) == a.size
            n += 1
        else:
            assert a == b
    assert n >= 3
