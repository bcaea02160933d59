"""FusedScheduler with streams that ask for click-free dump joins (``AudioFormat.join``), on a CPU stand-in
engine whose codec is not causal (a frame's PCM depends on its neighbours in the call, so context matters),
whose ``pcm_convert`` is the numpy statement of the rule (audio.StreamRef) and which records its codec rows and
output-stage calls: the context each dump is decoded with, the capacity rule, where the record of dumped
tokens is cleared, rollbacks, and that a stream without ``join`` makes the calls and sees the items of before."""
import numpy as np
import pytest
import torch

from llmvox_amd import audio as A
from llmvox_amd import streaming as S
from test_scheduler_audio import AudioEngine, TEXT, EOA, _W, _same_events, _segments

JOIN = A.AudioFormat(join=True)
JOIN16 = A.AudioFormat(16000, "s16le", speed_pct=130, join=True)
PLAIN16 = A.AudioFormat(16000, "s16le")


def _codec(codes: torch.Tensor) -> torch.Tensor:
    """A frame's amplitude mixes in its neighbours' codes, zero outside the call: not causal, as the codec."""
    amp = codes.float() / 2048.0 - 1.0
    z = torch.zeros(amp.shape[0], 1)
    mix = amp + 0.3 * torch.cat([z, amp[:, :-1]], 1) + 0.2 * torch.cat([amp[:, 1:], z], 1)
    return (mix[:, :, None] * torch.from_numpy(_W)[None, None, :] * 0.5).reshape(codes.shape[0], -1)


class JoinEngine(AudioEngine):
    def __init__(self, max_codec_frames=1 << 16, **kw):
        super().__init__(**kw)
        self.max_codec_frames = max_codec_frames
        self.codec_rows = []  # every row of every codec call
        self.join_calls = []  # (slot, n_in, final, ctx_frames or None when the keyword was not passed)

    def decode_codes(self, codes, bandwidth_id=0, out=None):
        assert codes.shape[0] * codes.shape[1] <= self.max_codec_frames or codes.shape[0] == 1
        assert codes.shape[1] <= self.max_codec_frames
        self.codec_rows += codes.tolist()
        return _codec(codes)

    def pcm_convert(self, pcm, slots, finals, fmt, **kw):
        assert set(kw) <= {"ctx_frames"} and (("ctx_frames" in kw) == fmt.join)
        n_in = 0 if pcm is None else int(pcm.shape[1])
        assert len(set(slots)) == len(slots), "a slot named twice in one call"
        ctx = kw.get("ctx_frames", [0] * len(slots))
        outs = []
        for b, (slot, final) in enumerate(zip(slots, finals)):
            self.log.append(("pcm_convert", slot, n_in, bool(final), fmt.sample_rate, fmt.encoding))
            self.join_calls.append((slot, n_in, bool(final), ctx[b] if "ctx_frames" in kw else None))
            ref = self.refs.setdefault(slot, A.StreamRef(fmt))
            assert ref.fmt == fmt
            outs.append(ref.push(pcm[b].numpy() if n_in else np.zeros(0, np.float32), bool(final), ctx_frames=ctx[b]))
        width = max(8, max(o.size for o in outs) + 3)
        out = torch.full((len(slots), width), 77, dtype=torch.int16 if fmt.encoding == "s16le" else torch.float32)
        for b, o in enumerate(outs):
            out[b, :o.size] = torch.from_numpy(o.copy())
        return out, [o.size for o in outs]


def _run(overlap, audios, eoa=EOA, to_bytes=False, n_tokens=150, tail=False, max_codec_frames=1 << 16, **machine_kw):
    eng = JoinEngine(max_streams=4, max_positions=4096, eoa=eoa, max_codec_frames=max_codec_frames)
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
    if tail:
        for st in sts:
            toks, st.m.speech_outputs = st.m.speech_outputs, []
            sch.queue_tail(st, toks)
        sch.flush()
    out = [(st.slot, list(st.events), list(st.tokens), list(st.joined)) for st in sts]
    for st in sts:
        sch.close_stream(st)
    sch.close()
    return eng, out


def _expected_calls(tokens, lengths, cap=1 << 16):
    """The joined stream's calls from its committed tokens and its sentences' dump lengths ([[frames], ended]):
    (codec row, ctx_frames, final) per dump, by the issue's rule."""
    calls, pos = [], 0
    for dumps, ended in lengths:
        done = 0
        for k, L in enumerate(dumps):
            c = max(0, min(16, done, cap - L))
            calls.append((tokens[pos - c:pos + L], c, ended and k == len(dumps) - 1))
            pos += L
            done += L
    return calls


def _lengths(plain_events):
    return [([i.size // 320 for i in items], ended) for items, ended in _segments(plain_events)]


def _ref_items(calls, fmt):
    ref, items = A.StreamRef(fmt), []
    for row, c, final in calls:
        items.append(ref.push(_codec(torch.tensor([row]))[0].numpy(), final, ctx_frames=c))
    return items


def _audio_items(events):
    return [e for e in events if isinstance(e, (bytes, np.ndarray))]


@pytest.mark.parametrize("overlap", [False, True], ids=["serial", "overlap"])
def test_context_rows_of_dumps_10_30_90_and_the_tail(overlap):
    eng, out = _run(overlap, [JOIN], eoa=None, tail=True, max_audio_len=4096)
    slot, events, t, _ = out[0]
    N = len(t)
    assert 130 < N < 400  # (the run stops, by chunks, behind the dump of 90 and before one of 270)
    want_rows = [t[0:10], t[0:40], t[24:130], t[114:N]]
    assert eng.codec_rows == want_rows
    assert eng.join_calls == [(slot, 3200, False, 0), (slot, 12800, False, 10), (slot, 106 * 320, False, 16),
                              (slot, (N - 114) * 320, True, 16)]
    items = _audio_items(events)
    assert [i.size for i in items] == [9 * 320, 30 * 320, 90 * 320, (N - 129) * 320]  # one frame less first, 320 T in all
    want = _ref_items(list(zip(want_rows, [0, 10, 16, 16], [False, False, False, True])), JOIN)
    for got, w in zip(items, want):
        assert got.dtype == np.float32 and np.array_equal(got.view(np.int32), w.view(np.int32))
    # the seams differ from plain concatenation, the rest of the body does not
    _, plain = _run(overlap, [None], eoa=None, tail=True, max_audio_len=4096)
    p, j = np.concatenate(_audio_items(plain[0][1])), np.concatenate(items)
    assert p.size == j.size == N * 320
    for seam in (10, 40, 130):
        assert not np.array_equal(p[(seam - 1) * 320:(seam + 1) * 320], j[(seam - 1) * 320:(seam + 1) * 320])
    assert np.array_equal(p[:8 * 320], j[:8 * 320])


def test_no_room_in_the_engine_means_no_context():
    eng, out = _run(False, [JOIN], eoa=None, max_audio_len=4096, max_codec_frames=90)
    slot, events, t, _ = out[0]
    assert [c[3] for c in eng.join_calls] == [0, 10, 0]  # (min(16, 40, 90 - 90) = 0 for the dump of 90)
    assert eng.codec_rows == [t[0:10], t[0:40], t[40:130]]
    items = _audio_items(events)
    pcm90 = _codec(torch.tensor([t[40:130]]))[0].numpy()
    held = _codec(torch.tensor([t[0:40]]))[0].numpy()[-320:]
    assert np.array_equal(items[2], np.concatenate([held, pcm90[:-320]]))  # that seam is a plain one


@pytest.mark.parametrize("overlap", [False, True], ids=["serial", "overlap"])
@pytest.mark.parametrize("fmt", [JOIN, JOIN16], ids=["f32", "speed-16k-s16"])
def test_sentences_ended_by_eoa_with_rollback(overlap, fmt):
    """The stand-in ends a sentence at every position divisible by 41, mid-chunk: the overlapped scheduler has
    run ahead by then and rolls back. The record of dumped tokens holds committed tokens only and starts empty in
    every sentence; delivered items are StreamRef's over the expected context-plus-token rows."""
    _, plain = _run(overlap, [None])
    eng, out = _run(overlap, [fmt])
    slot, events, t, joined = out[0]
    assert t == plain[0][2]
    lengths = _lengths(plain[0][1])
    assert len(lengths) >= 3 and all(ended for _, ended in lengths[:-1])
    calls = _expected_calls(t, lengths)
    assert eng.codec_rows == [row for row, _, _ in calls]
    assert eng.join_calls == [(slot, len(row) * 320, final, c) for row, c, final in calls]
    firsts = [k for k, (row, c, final) in enumerate(calls) if k == 0 or calls[k - 1][2]]
    assert len(firsts) >= 3 and all(calls[k][1] == 0 for k in firsts)  # cleared at every sentence's end
    assert any(c == 16 for _, c, _ in calls) and any(0 < c < 16 for _, c, _ in calls)
    want = _ref_items(calls, fmt)
    items = _audio_items(events)
    assert len(items) == len(want)
    for got, w in zip(items, want):
        assert got.dtype == w.dtype and np.array_equal(got, w)
    for (items_s, ended), (pitems, _) in zip(_segments(events), _segments(plain[0][1])):
        if ended and fmt is JOIN:  # a sentence of T frames delivers 320 T samples
            assert sum(i.size for i in items_s) == sum(i.size for i in pitems)
    if lengths[-1][1]:
        assert joined == []
    # serial and overlapped scheduling deliver the same items
    _, other = _run(not overlap, [fmt])
    _same_events(other[0][1], events)


@pytest.mark.parametrize("overlap", [False, True], ids=["serial", "overlap"])
def test_record_cleared_by_the_max_audio_length_reset(overlap):
    eng, out = _run(overlap, [JOIN], eoa=None, max_audio_len=50, n_tokens=120, tail=True)
    slot, events, t, joined = out[0]
    # dumps of 10 and 30, then the outputs pass 50 and are dropped: a flush ends the sentence; the tokens behind
    # the reset belong to a new sentence, whose tail dump carries no context
    assert eng.join_calls[:3] == [(slot, 3200, False, 0), (slot, 12800, False, 10), (slot, 0, True, 0)]
    assert eng.codec_rows[:2] == [t[0:10], t[0:40]]
    assert all(c[3] == 0 for c in eng.join_calls[3:]) and all(c[2] for c in eng.join_calls[3:])
    assert len(eng.join_calls) >= 4 and eng.join_calls[-1][1] > 0  # (the tail of the sentence the run stopped in)
    assert joined == []
    segs = _segments(events)
    assert sum(i.size for i in segs[0][0]) == 40 * 320  # the sentence delivered what it dumped: 320 T


@pytest.mark.parametrize("overlap", [False, True], ids=["serial", "overlap"])
def test_streams_without_join_make_the_calls_of_before(overlap):
    eng0, alone = _run(overlap, [PLAIN16, None])
    eng, mixed = _run(overlap, [PLAIN16, None, JOIN16])
    for k in (0, 1):
        assert mixed[k][0] == alone[k][0] and mixed[k][2] == alone[k][2]
        _same_events(mixed[k][1], alone[k][1])
    s0 = mixed[0][0]
    assert [c for c in eng.log if c[0] == "pcm_convert" and c[1] == s0] == \
        [c for c in eng0.log if c[0] == "pcm_convert" and c[1] == s0]
    assert all(c[3] is None for c in eng.join_calls if c[0] == s0)          # no ctx_frames keyword
    assert all(c[3] is not None for c in eng.join_calls if c[0] == mixed[2][0])
    assert not [c for c in eng.log if c[0].startswith("pcm_") and c[1] == mixed[1][0]]
    assert all(c[3] is None for c in eng0.join_calls)
    # the plain streams' codec rows are their own tokens: no context anywhere
    t0 = alone[0][2]
    own = [r for r in eng.codec_rows if any(r == t0[i:i + len(r)] for i in (0, 10, 40))]
    assert own


def test_bytes_of_a_joined_stream():
    _, arr = _run(True, [JOIN16], to_bytes=False)
    _, byt = _run(True, [JOIN16], to_bytes=True)
    assert len(arr[0][1]) == len(byt[0][1])
    for a, b in zip(arr[0][1], byt[0][1]):
        if isinstance(a, np.ndarray):
            assert isinstance(b, bytes) and b == a.astype("<i2").tobytes()
        else:
            assert a == b


def test_groups_batch_by_decoded_length():
    eng = JoinEngine(max_streams=4, max_codec_frames=64)
    sch = S.FusedScheduler(eng, max_chunk=8, to_bytes=False, overlap=False)
    a = sch.open_stream(index=0, dump_size=10, audio=JOIN)
    b = sch.open_stream(index=1, dump_size=10)
    a.joined = list(range(100, 110))
    row = sch._join_row(a, [7] * 20)
    assert row.ctx == 10 and list(row) == list(range(100, 110)) + [7] * 20 and a.joined == [7] * 16
    dumps = [(a, row), (b, [5] * 30), (b, [6] * 30), (b, [4] * 20)]
    groups = sorted(sch._groups(dumps))
    assert groups == [(20, [3]), (30, [0, 1]), (30, [2])]  # (64 // 30 = 2 rows a call)
    assert sch._join_row(b, [1, 2]) == [1, 2] and sch._join_row(None, [3]) == [3]
    for st in (a, b):
        sch.close_stream(st)
    sch.close()
