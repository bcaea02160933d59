"""FusedScheduler with streams whose format names a watermark, on the CPU stand-in engine of test_scheduler_g711.py (its
``pcm_convert`` is ``audio.StreamRef``, which runs the mark stage where the format has a key): every finished sentence
delivers ``audio.convert_ref`` of the samples the same stream delivers unmarked, so every sentence restarts the pattern;
the bucket key keeps marked rows, and rows of another id, apart; a stream without the field beside them sees the items
it always saw, and a run without it logs the calls it always logged."""
import numpy as np
import pytest

import mark_signals as MS
import test_scheduler_g711 as G
from llmvox_amd import audio as A
from test_scheduler_audio import _same_events, _segments

KEY, ID = MS.KEY, MS.ID
FMTS = [A.AudioFormat(mark_key=KEY, mark_id=ID), A.AudioFormat(8000, "s16le", mark_key=KEY, mark_id=ID, mark_strength=3),
        A.AudioFormat(16000, "ulaw", volume_pct=200, mark_key=KEY)]


def _plain(fmt):
    return A.AudioFormat(fmt.sample_rate, fmt.encoding, fmt.container, fmt.speed_pct, fmt.pitch_pct, fmt.join, fmt.volume_pct,
                         fmt.formant_pct)


@pytest.mark.parametrize("overlap", [False, True], ids=["serial", "overlap"])
@pytest.mark.parametrize("fmt", FMTS, ids=lambda f: f"{f.sample_rate}-{f.encoding}-{f.mark_strength}")
def test_marked_stream_delivers_the_rule_per_sentence(overlap, fmt):
    _, plain = G._run(overlap, [None, None])
    log, mixed = G._run(overlap, [None, fmt])
    assert mixed[0][2] == plain[0][2] and mixed[1][2] == plain[1][2]  # the same tokens
    _same_events(mixed[0][1], plain[0][1])  # the stream beside it sees what it always saw
    segs, raw = _segments(mixed[1][1]), _segments(plain[1][1])
    assert len(segs) == len(raw) >= 3
    finished = 0
    for (items, ended), (ritems, rended) in zip(segs, raw):
        assert ended == rended
        x = np.concatenate(ritems)  # the f32 samples of the sentence's own tokens
        got = np.concatenate(items) if items else np.zeros(0, fmt.dtype)
        want = A.convert_ref(x, fmt)
        assert got.dtype == fmt.dtype
        if ended:  # a whole sentence: the one-shot conversion, every sample of it, and the mark is in it
            assert np.array_equal(got, want) and not np.array_equal(want, A.convert_ref(x, _plain(fmt)))
            finished += 1
        else:  # the run stopped inside it: a prefix, short by what the stages hold back
            assert got.size < want.size and np.array_equal(got, want[:got.size])
    assert finished >= 2
    # the slot's calls: one per dump, in dump order, final exactly at the sentences' ends, as without the mark
    calls = [c for c in log if c[0] == "pcm_convert" and c[1] == mixed[1][0]]
    assert [(c[2], c[3]) for c in calls] == [(p.size, rended and k == len(ritems) - 1) for ritems, rended in raw
                                             for k, p in enumerate(ritems)]


def test_marked_rows_are_a_bucket_of_their_own():
    marked, other_id, plain = (A.AudioFormat(8000, "s16le", mark_key=KEY, mark_id=ID),
                               A.AudioFormat(8000, "s16le", mark_key=KEY, mark_id=ID ^ 1), A.AudioFormat(8000, "s16le"))
    fmts = [marked, plain, marked, other_id]
    log, out = G._run(True, fmts)
    of = {o[0]: f for o, f in zip(out, fmts)}
    calls = [c for c in log if c[0] == "pcm_call"]
    assert calls
    for _, slots, _ in calls:  # a call carries rows of one (key, id, strength) only
        assert len({(of[s].mark_key, of[s].mark_id, of[s].mark_strength) for s in slots}) == 1
    both = {s for s, f in of.items() if f == marked}
    assert len(both) == 2 and any(set(slots) == both for _, slots, _ in calls)  # and the two marked streams do share calls


def test_a_run_without_the_field_logs_what_it_logged():
    fmts = [None, A.AudioFormat(8000, "ulaw"), A.AudioFormat(16000, "s16le")]
    log_a, out_a = G._run(True, fmts)
    log_b, out_b = G._run(True, fmts + [A.AudioFormat(16000, "s16le", mark_key=KEY)])
    slots = {o[0] for o in out_a}
    keep = [c for c in log_b if (c[0] == "pcm_call" and set(c[1]) <= slots) or (c[0] != "pcm_call" and c[1] in slots)]
    assert keep == log_a
    for a, b in zip(out_a, out_b):
        _same_events(a[1], b[1])


def test_a_format_without_a_key_is_the_format_it_was():
    """The new fields change nothing about a format that names no key: equal to, hashed as and converted like before."""
    old = A.AudioFormat(16000, "s16le", "raw", 100, 125, False, 200, 100, None, None)
    assert old == A.AudioFormat(16000, "s16le", pitch_pct=125, volume_pct=200, formant_pct=100) and not old.marks
    assert A.AudioFormat().is_default and not A.AudioFormat().converts
    marked = A.AudioFormat(mark_key=0)
    assert marked.marks and marked.converts and not marked.is_default and marked != A.AudioFormat()
    assert "mark_key" not in repr(marked) and "mark_key" not in repr(A.AudioFormat(mark_key=KEY)) and str(KEY) not in repr(A.AudioFormat(mark_key=KEY))
