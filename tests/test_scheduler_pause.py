"""FusedScheduler with streams whose format pauses, on the CPU stand-in engine of test_scheduler_g711.py with a codec
that renders some frames silent and rows of whole slots (uint8) for a pausing format: every sentence delivers the
slots of ``audio.pause_slots_ref`` of the samples the same stream delivers without the pause fields, and through
``audio.PauseMux`` they are ``audio.pause_ref`` of the sentences; the bucket key keeps pausing rows apart; a stream
without the fields beside them sees the items it always saw, and a run without them logs the calls it always logged."""
import numpy as np
import pytest
import torch

import test_scheduler_g711 as G
from llmvox_amd import audio as A
from llmvox_amd import streaming as S
from test_scheduler_audio import EOA, TEXT, _same_events, _segments


class PauseEngine(G.G711Engine):
    """G711Engine whose codec renders three frames of five silent (so sentences have silence at their edges and
    inside) and whose rows are uint8, whole slots, for a format that pauses, as the device's are."""

    def decode_codes(self, codes, bandwidth_id=0, out=None):
        pcm = super().decode_codes(codes, bandwidth_id, out)
        loud = (codes % 5 >= 3).float()
        return pcm * loud[:, :, None].expand(-1, -1, 320).reshape(codes.shape[0], -1)

    def pcm_convert(self, pcm, slots, finals, fmt):
        if not fmt.pauses:
            return super().pcm_convert(pcm, slots, finals, fmt)
        n_in = 0 if pcm is None else int(pcm.shape[1])
        assert len(set(slots)) == len(slots), "a slot named twice in one call"
        self.log.append(("pcm_call", tuple(slots), fmt.encoding))
        outs = []
        for b, (slot, final) in enumerate(zip(slots, finals)):
            self.log.append(("pcm_convert", slot, n_in, bool(final), fmt.sample_rate, fmt.encoding))
            ref = self.refs.setdefault(slot, A.StreamRef(fmt))
            assert ref.fmt == fmt
            outs.append(ref.push(pcm[b].numpy() if n_in else np.zeros(0, np.float32), bool(final)))
        out = torch.full((len(slots), max(16, max(o.size for o in outs) + 3)), 77, dtype=torch.uint8)
        for b, o in enumerate(outs):
            out[b, :o.size] = torch.from_numpy(o.copy())
        return out, [o.size for o in outs]


def _run(overlap, audios, to_bytes=False, n_tokens=150):
    eng = PauseEngine(max_streams=4, max_positions=4096, eoa=EOA)
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


def _plain(fmt):
    return A.AudioFormat(fmt.sample_rate, fmt.encoding, fmt.container, fmt.speed_pct, fmt.pitch_pct, fmt.join, fmt.volume_pct,
                         fmt.formant_pct)


FMTS = [A.AudioFormat(8000, "s16le", pause_ms=150, max_pause_ms=100), A.AudioFormat(24000, "f32le", pause_ms=0),
        A.AudioFormat(16000, "ulaw", max_pause_ms=100), A.AudioFormat(8000, "alaw", volume_pct=200, pause_ms=40)]


@pytest.mark.parametrize("overlap", [False, True], ids=["serial", "overlap"])
@pytest.mark.parametrize("fmt", FMTS, ids=lambda f: f"{f.sample_rate}-{f.encoding}-{f.pause_ms}-{f.max_pause_ms}")
def test_pausing_stream_delivers_the_rule(overlap, fmt):
    _, plain = _run(overlap, [None, None])
    log, mixed = _run(overlap, [None, fmt])
    log0, base = _run(overlap, [None, _plain(fmt)])
    assert mixed[0][2] == plain[0][2] and mixed[1][2] == plain[1][2] == base[1][2]  # the same tokens
    _same_events(mixed[0][1], plain[0][1])  # the stream beside it sees what it always saw
    segs, segs0 = _segments(mixed[1][1]), _segments(base[1][1])
    assert len(segs) == len(segs0) >= 3
    size, mux, body, sentences = A.pause_slot_bytes(fmt), A.PauseMux(fmt), [], []
    for (items, ended), (items0, ended0) in zip(segs, segs0):
        assert ended == ended0 and all(i.dtype == np.uint8 and i.size % size == 0 for i in items)
        y = np.concatenate(items0)
        assert y.dtype == fmt.dtype
        K = A.pause_blocks_upto(fmt.sample_rate, y.size, ended)
        assert np.array_equal(np.concatenate(items), A.pause_slots_ref(y, fmt, 0, K))  # the slots of the same samples
        if ended:
            sentences.append(y)
            body += [mux.push(i) for i in items]
    want = A.pause_ref(sentences, fmt)
    assert b"".join(body) == want and len(sentences) >= 2
    if fmt.pause_ms is not None:  # (edges to trim and gaps to put in; the codec's silences are shorter than the cap)
        assert want != b"".join(y.tobytes() for y in sentences)
    # the slot's calls are those of the stream without the fields: they change no call's inputs or finals
    calls = [c[2:] for c in log if c[0] == "pcm_convert" and c[1] == mixed[1][0]]
    calls0 = [c[2:] for c in log0 if c[0] == "pcm_convert" and c[1] == base[1][0]]
    if _plain(fmt).converts:
        assert calls == calls0
    else:  # (24 kHz f32le without the fields is no format at all: one call a dump, final at the sentences' ends)
        assert not calls0
        assert [(c[0], c[1]) for c in calls] == [(i.size, ended and k == len(items) - 1)
                                                 for items, ended in segs0 for k, i in enumerate(items)]


def test_pausing_rows_are_a_bucket_of_their_own():
    pausing, plain = A.AudioFormat(8000, "s16le", pause_ms=150), A.AudioFormat(8000, "s16le")
    fmts = [pausing, plain, pausing, plain]
    log, out = _run(True, fmts)
    pauses = {o[0]: f.pauses for o, f in zip(out, fmts)}
    calls = [c for c in log if c[0] == "pcm_call"]
    assert calls
    for _, slots, _ in calls:  # a call carries pausing rows or rows that do not pause, never both
        assert len({pauses[s] for s in slots}) == 1
    both = {s for s, p in pauses.items() if p}
    assert any(set(slots) == both for _, slots, _ in calls)  # and the two pausing streams do share calls


def test_a_run_without_the_fields_logs_what_it_logged():
    fmts = [None, A.AudioFormat(8000, "ulaw"), A.AudioFormat(16000, "s16le")]
    log_a, out_a = _run(True, fmts)
    log_b, out_b = _run(True, fmts + [A.AudioFormat(16000, "s16le", pause_ms=150)])
    slots = {o[0] for o in out_a}
    keep = [c for c in log_b if (c[0] == "pcm_call" and set(c[1]) <= slots) or (c[0] != "pcm_call" and c[1] in slots)]
    assert keep == log_a
    for a, b in zip(out_a, out_b):
        _same_events(a[1], b[1])
    log_c, _ = G._run(True, fmts)  # (and on the engine the older tests use, whose codec renders no silence)
    assert [c for c in log_c if c[0] == "pcm_call"] == [c for c in log_a if c[0] == "pcm_call"]


def test_bytes_are_the_slots():
    fmt = A.AudioFormat(8000, "ulaw", pause_ms=0)
    _, arr = _run(True, [fmt], to_bytes=False)
    _, byt = _run(True, [fmt], to_bytes=True)
    assert len(arr[0][1]) == len(byt[0][1])
    for a, b in zip(arr[0][1], byt[0][1]):
        if isinstance(a, np.ndarray):
            assert isinstance(b, bytes) and b == a.tobytes()
        else:
            assert a == b
