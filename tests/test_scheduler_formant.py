"""FusedScheduler with a stream that names a formant, on the CPU stand-in engine of test_scheduler_audio (its
``pcm_convert`` is ``audio.StreamRef``: join, stretch, ratio, formant, level, resample, encode): the stream's sentences
are ``convert_ref`` of their own f32 sentences with exactly the samples the plan predicts, the default stream beside it is
untouched and makes the engine calls it always made, a slot's calls keep dump order and carry one formant, streams that
differ in their formant alone never share a call, and the stage combines with speed, join, volume and every encoding."""
import numpy as np
import pytest
import torch

from llmvox_amd import audio as A
from llmvox_amd import streaming as S
from test_scheduler_audio import EOA, TEXT, AudioEngine, _same_events, _segments

SHAPED = A.AudioFormat(pitch_pct=125, formant_pct=100)
_TORCH = {"f32le": torch.float32, "s16le": torch.int16, "ulaw": torch.uint8, "alaw": torch.uint8, "flac": torch.uint8}


class FormantEngine(AudioEngine):
    """AudioEngine whose converted rows have the encoding's dtype, that takes the join's context frames, records the
    formant of every ``pcm_convert`` call and refuses a change inside a slot's segment, as the library does."""

    def __init__(self, **kw):
        super().__init__(**kw)
        self.formants = []
        self.pcm_calls = []

    def pcm_convert(self, pcm, slots, finals, fmt, ctx_frames=None):
        n_in = 0 if pcm is None else int(pcm.shape[1])
        assert len(set(slots)) == len(slots), "a slot named twice in one call"
        self.pcm_calls.append((tuple(slots), fmt.formant_pct))
        outs = []
        for b, (slot, final) in enumerate(zip(slots, finals)):
            self.log.append(("pcm_convert", slot, n_in, bool(final), fmt.sample_rate, fmt.encoding))
            self.formants.append((slot, fmt.formant_pct))
            ref = self.refs.setdefault(slot, A.StreamRef(fmt))
            assert ref.fmt == fmt, "another format inside a segment"
            outs.append(ref.push(pcm[b].numpy() if n_in else np.zeros(0, np.float32), bool(final),
                                 int(ctx_frames[b]) if ctx_frames is not None else 0))
        width = max(16, max(o.size for o in outs) + 3)  # (rows are wider than their counts, as the device's are)
        out = torch.full((len(slots), width), 77, dtype=_TORCH[fmt.encoding])
        for b, o in enumerate(outs):
            out[b, :o.size] = torch.from_numpy(o.copy())
        return out, [o.size for o in outs]


def _run(overlap, audios, n_tokens=150, to_bytes=False):
    eng = FormantEngine(max_streams=4, max_positions=4096, eoa=EOA)
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
    return eng, out


def _counts(fmt, T, final):
    """Samples of a sentence of T codec samples the chain has delivered: the stages' closed forms one after the other."""
    L, M = fmt.ratio
    n = A.ratio_emitted_upto(L, M, A.stretch_emitted_upto(fmt.stretch_pct, T, final), final)
    if fmt.formant != (1, 1):
        n = A.formant_emitted_upto(n, final)
    return A.emitted_upto(fmt.sample_rate, A.level_emitted_upto(fmt.volume_pct, n, final), final)


def _check_stream(eng, slot, events, plain_events, fmt):
    """A stream without join and FLAC: per sentence the samples of ``convert_ref`` and the plan's counts; the slot's
    calls, one per dump in dump order, final exactly at the sentences' ends, all at one formant."""
    segs, plain = _segments(events), _segments(plain_events)
    assert len(segs) == len(plain) and len(segs) >= 3
    for (items, ended), (pitems, pended) in zip(segs, plain):
        assert ended == pended
        x = np.concatenate(pitems)
        got = np.concatenate(items) if items else np.zeros(0, fmt.dtype)
        assert got.dtype == fmt.dtype
        want = A.convert_ref(x, fmt)
        n = _counts(fmt, x.size, ended)
        if ended:  # a whole sentence: ceil-exact, every held-back sample delivered
            stretched = -(-x.size * 100 // fmt.stretch_pct)
            L, M = fmt.ratio
            rate_L, rate_M, _ = A.RATES[fmt.sample_rate]
            assert n == want.size == -(-(-(-stretched * L // M)) * rate_L // rate_M)
        assert got.size == n and np.array_equal(got.view(np.uint8), want[:n].view(np.uint8))
    calls = [c for c in eng.log if c[0] == "pcm_convert" and c[1] == slot]
    want_calls = []
    for pitems, pended in plain:
        for k, p in enumerate(pitems):
            want_calls.append((p.size, pended and k == len(pitems) - 1))
    assert [(c[2], c[3]) for c in calls] == want_calls
    assert [v for v in eng.formants if v[0] == slot] == [(slot, fmt.formant_pct)] * len(calls)


@pytest.mark.parametrize("overlap", [False, True], ids=["serial", "overlap"])
def test_formant_stream_beside_a_default_one(overlap):
    eng0, plain = _run(overlap, [None, None])
    assert not [c for c in eng0.log if c[0].startswith("pcm_")]
    eng, mixed = _run(overlap, [None, SHAPED])
    assert mixed[0][2] == plain[0][2] and mixed[1][2] == plain[1][2]  # the same tokens
    _same_events(mixed[0][1], plain[0][1])  # the default stream's items: byte-identical to a run without the neighbour
    assert not [c for c in eng.log if c[0].startswith("pcm_") and c[1] == mixed[0][0]]
    _check_stream(eng, mixed[1][0], mixed[1][1], plain[1][1], SHAPED)
    # the formant did something: the sentence is not the pitched one
    x = np.concatenate(_segments(plain[1][1])[0][0])
    got = np.concatenate(_segments(mixed[1][1])[0][0])
    assert not np.array_equal(got, A.convert_ref(x, A.AudioFormat(pitch_pct=125)))
    # the default stream's engine calls are those of a run without the formant stream
    mine = lambda log, slot: [c for c in log if len(c) > 1 and c[1] == slot]
    assert mine(eng.log, mixed[0][0]) == mine(eng0.log, plain[0][0])


@pytest.mark.parametrize("fmt", [A.AudioFormat(16000, "s16le", "raw", 130, 100, False, 100, 90),
                                 A.AudioFormat(24000, "f32le", "raw", 100, 80, False, 250, 100),
                                 A.AudioFormat(8000, "ulaw", "raw", 90, 110, False, 100, 100),
                                 A.AudioFormat(48000, "alaw", "wav", 100, 100, False, 50, 120),
                                 A.AudioFormat(24000, "s16le", "raw", 100, 100, False, 100, 67)],
                         ids=lambda f: f"{f.sample_rate}-{f.encoding}-{f.speed_pct}-{f.pitch_pct}-{f.volume_pct}-{f.formant_pct}")
def test_it_combines_with_speed_volume_rate_and_encoding(fmt):
    _, plain = _run(True, [None, None])
    eng, both = _run(True, [SHAPED, fmt])
    assert fmt.formant != (1, 1)
    _check_stream(eng, both[0][0], both[0][1], plain[0][1], SHAPED)
    _check_stream(eng, both[1][0], both[1][1], plain[1][1], fmt)


def test_it_combines_with_join():
    """Joined dumps re-render frames, so the sentence is not ``convert_ref`` of the plain stream's; the counts are: the
    join and the formant stage each deliver one sample per input by the sentence's end."""
    fmt = A.AudioFormat(join=True, formant_pct=90)
    _, plain = _run(True, [None, None])
    eng, both = _run(True, [None, fmt])
    eng_j, joined = _run(True, [None, A.AudioFormat(join=True)])
    assert both[1][2] == plain[1][2] == joined[1][2]
    segs, psegs, jsegs = _segments(both[1][1]), _segments(plain[1][1]), _segments(joined[1][1])
    assert len(segs) == len(psegs) == len(jsegs) >= 3
    for (items, ended), (pitems, _), (jitems, _) in zip(segs, psegs, jsegs):
        x = np.concatenate(jitems)  # what the join hands the formant stage: the joined stream's sentence
        got = np.concatenate(items) if items else np.zeros(0, np.float32)
        if ended:
            assert got.size == x.size == sum(p.size for p in pitems)
            assert np.array_equal(got.view(np.uint32), A.formant_ref(x, 10, 9).view(np.uint32))
        else:
            assert got.size == A.formant_emitted_upto(x.size, False)
            assert np.array_equal(got.view(np.uint32), A.formant_ref(x, 10, 9)[:got.size].view(np.uint32))
    assert {v[1] for v in eng.formants} == {90}
    # the formant changes no call of the joined stream: the same dumps, context frames and finals
    strip = lambda log, slot: [c[:4] for c in log if c[0] == "pcm_convert" and c[1] == slot]
    assert strip(eng.log, both[1][0]) == strip(eng_j.log, joined[1][0])


def test_it_combines_with_flac():
    """The FLAC stream of a formant format decodes to the s16le stream of the same format."""
    import flac_decode as D
    fmt = A.AudioFormat(16000, "flac", "raw", 100, 125, False, 100, 100)
    s16 = A.AudioFormat(16000, "s16le", "raw", 100, 125, False, 100, 100)
    _, out = _run(True, [fmt, s16])
    assert out[0][2] == out[1][2]
    mux = A.FlacMux(16000)
    n = 0
    for (items, ended), (items16, _) in zip(_segments(out[0][1]), _segments(out[1][1])):
        first = mux.sample_no
        got = D.decode(b"".join(mux.push(i) for i in items), first_sample=first, header=False, rate=16000)[0]
        want = np.concatenate(items16)
        if ended:
            assert np.array_equal(got, want)
            n += 1
        else:
            assert np.array_equal(got, want[:got.size])
    assert n >= 2


def test_streams_that_differ_in_formant_alone_are_separate_calls():
    """The bucket key holds the formant: two streams of one codec call at two formants never share a ``pcm_convert``."""
    eng = FormantEngine(max_streams=4)
    sch = S.FusedScheduler(eng, max_chunk=8, to_bytes=False, overlap=False)
    a = sch.open_stream(index=0, dump_size=10, audio=A.AudioFormat(16000, "s16le", formant_pct=90))
    b = sch.open_stream(index=1, dump_size=10, audio=A.AudioFormat(16000, "s16le", formant_pct=110))
    c = sch.open_stream(index=0, dump_size=10, audio=A.AudioFormat(16000, "s16le"))
    d = sch.open_stream(index=1, dump_size=10, audio=A.AudioFormat(16000, "s16le", formant_pct=90))
    res, err = sch._decode([(a, [7] * 10), (b, [9] * 10), (c, [11] * 10), (d, [13] * 10)], {0, 1, 2, 3})
    assert err is None
    assert sorted(eng.pcm_calls, key=repr) == sorted([(tuple(sorted([a.slot, d.slot])), 90), ((b.slot,), 110), ((c.slot,), None)], key=repr)
    pcm = eng.decode_codes(torch.tensor([[7] * 10, [9] * 10, [11] * 10, [13] * 10])).numpy()
    for r, st in enumerate((a, b, c, d)):
        assert np.array_equal(res[r], A.convert_ref(pcm[r], st.audio))
    for st in (a, b, c, d):
        sch.close_stream(st)
    sch.close()


def test_a_stream_without_the_field_makes_the_calls_of_before():
    """The recorded engine calls of a run whose formats do not name the field are those of the same run with formats
    built as before the field existed (positionally, seven fields); a formant that the pitch already realises changes
    nothing either."""
    old = A.AudioFormat(16000, "s16le", "raw", 130, 90, False, 250)
    assert old.formant_pct is None
    eng_a, out_a = _run(True, [None, old])
    eng_b, out_b = _run(True, [None, A.AudioFormat(16000, "s16le", "raw", 130, 90, False, 250, None)])
    assert eng_a.log == eng_b.log and {v[1] for v in eng_a.formants} == {None}
    for (_, ev_a, tok_a), (_, ev_b, tok_b) in zip(out_a, out_b):
        assert tok_a == tok_b
        _same_events(ev_a, ev_b)
    # the log is the one the engine without the stage in its StreamRef wrote: no call more, none less, per dump
    calls = [c for c in eng_a.log if c[0] == "pcm_convert"]
    dumps = sum(len(items) for items, _ in _segments(out_a[0][1]))
    assert len(calls) >= dumps >= 3
    # formant 1.0 and nothing else does not reach the engine's PCM stage at all
    eng, out = _run(True, [A.AudioFormat(formant_pct=100)])
    assert not [c for c in eng.log if c[0].startswith("pcm_")]
    _, plain = _run(True, [None])
    _same_events(out[0][1], plain[0][1])
    # a formant alone does
    eng, out = _run(True, [A.AudioFormat(formant_pct=90)])
    assert [c for c in eng.log if c[0] == "pcm_convert"] and out[0][1][0].dtype == np.float32


def test_service_streams_the_shaped_sentence():
    from llmvox_amd.server import TTSService
    eng = FormantEngine(max_streams=4, max_positions=4096)
    svc = TTSService([eng], max_chunk=16, max_tokens=55)  # (the request stops between two dumps: it has a tail)
    try:
        plain = b"".join(svc.chunks(svc.submit("Hello there."), timeout=0.01))
        assert not [c for c in eng.log if c[0].startswith("pcm_")]
        shaped = b"".join(svc.chunks(svc.submit("Hello there.", audio=SHAPED), timeout=0.01))
        fmt = A.AudioFormat(16000, "s16le", "wav", formant_pct=90)
        dark = b"".join(svc.chunks(svc.submit("Hello there.", audio=fmt), timeout=0.01))
    finally:
        svc.shutdown()
    x = np.frombuffer(plain, dtype="<f4")
    got = np.frombuffer(shaped, dtype="<f4")
    assert got.size == x.size  # every held-back sample is delivered at the end
    assert np.array_equal(got.view(np.uint32), A.convert_ref(x, SHAPED).view(np.uint32))
    assert dark[:44] == A.wav_header(fmt)
    assert np.array_equal(np.frombuffer(dark[44:], dtype="<i2"), A.convert_ref(x, fmt))
