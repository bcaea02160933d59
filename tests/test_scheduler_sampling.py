"""FusedScheduler / TTSService with a sampling stream, on a CPU stand-in engine that records its calls:
where in the call order the scheduler queues a slot's sampling parameters (stream order on the device
follows it), which seeds the sentences and the replica streams get, and that a stream opened without
``sampling`` never touches the engine's ``set_sampling``."""
import pytest

from llmvox_amd import streaming as S
from llmvox_amd.sampling import Sampling, segment_seed
from test_service_multidevice import StateEngine

TEXT = "The quick brown fox jumps over the lazy dog. Then it sleeps near the river bank. The end."
EOA = 4000  # the stand-in emits it at every position divisible by 41: segments end mid-chunk


class RecordingEngine(StateEngine):
    """StateEngine + the log of every state call: (name, slot, ...) and ("ar_steps", slots)."""

    def __init__(self, **kw):
        super().__init__(**kw)
        self.log = []

    def reset_slot(self, slot):
        self.log.append(("reset_slot", slot))
        super().reset_slot(slot)

    def set_slot(self, slot, pos, prev=0):
        self.log.append(("set_slot", slot, pos, prev))
        super().set_slot(slot, pos, prev)

    def set_sampling(self, slot, temperature=0.0, top_k=0, seed=0):
        self.log.append(("set_sampling", slot, temperature, top_k, seed))

    def ar_steps(self, n, slots, plan, rowstep, tok, margin=None):
        self.log.append(("ar_steps", tuple(s for s in slots.tolist() if s >= 0)))
        super().ar_steps(n, slots, plan, rowstep, tok, margin)


class GreedyOnlyEngine(StateEngine):  # (no set_sampling: the stand-ins of the older tests)
    pass


def _run(overlap, sampling, n_streams=2, max_chunk=16):
    eng = RecordingEngine(max_streams=4, max_positions=4096, eoa=EOA)
    sch = S.FusedScheduler(eng, max_chunk=max_chunk, to_bytes=False, overlap=overlap,
                           stop_rule=lambda st, ntok, pos: ntok >= 150)
    sts = []
    for i in range(n_streams):
        st = sch.open_stream(index=i, dump_size=10, eoa_id=EOA, sampling=sampling)
        for w in TEXT.split(" "):
            st.feed(w)
        sts.append(st)
    assert sch.run_until_idle(max_chunks=2000) > 0
    slots = [st.slot for st in sts]
    segments = [st.segment for st in sts]
    for st in sts:
        sch.close_stream(st)
    sch.close()
    return eng.log, slots, segments


def _per_slot(log, slot):
    return [c for c in log if c[0] != "ar_steps" and c[1] == slot]


@pytest.mark.parametrize("overlap", [False, True], ids=["serial", "overlap"])
def test_sampling_calls_follow_the_segments(overlap):
    sp = Sampling(0.8, 50, seed=0x1234567890abcdef)
    log, slots, segments = _run(overlap, sp)
    first_chunk = next(i for i, c in enumerate(log) if c[0] == "ar_steps")
    for index, slot in enumerate(slots):
        calls = _per_slot(log, slot)
        # opened: reset, then the first sentence's seed, both before the first chunk
        assert calls[0] == ("reset_slot", slot)
        assert calls[1] == ("set_sampling", slot, 0.8, 50, segment_seed(sp.seed, index, 0))
        assert log.index(calls[1]) < first_chunk
        # every end of audio: the rewind, then the next sentence's seed, adjacent in the call order
        assert segments[index] >= 2
        body = calls[2:-1]
        assert len(body) == 2 * segments[index]
        for g in range(segments[index]):
            a, b = body[2 * g], body[2 * g + 1]
            assert a == ("set_slot", slot, 0, 0)
            assert b == ("set_sampling", slot, 0.8, 50, segment_seed(sp.seed, index, g + 1))
            assert log[log.index(b) - 1] == a  # (b is unique: its seed is)
        # closed: back to greedy
        assert calls[-1] == ("set_sampling", slot, 0.0, 0, 0)
    seeds = [c[4] for c in log if c[0] == "set_sampling" and c[2] > 0]
    assert len(set(seeds)) == len(seeds)  # every sentence of every replica draws from a seed of its own


def test_overlap_and_serial_issue_the_same_calls_per_slot():
    sp = Sampling(1.0, 0, seed=7)
    (log_s, slots_s, seg_s), (log_o, slots_o, seg_o) = _run(False, sp), _run(True, sp)
    assert slots_s == slots_o and seg_s == seg_o
    for slot in slots_s:
        assert _per_slot(log_s, slot) == _per_slot(log_o, slot)


@pytest.mark.parametrize("sampling", [None, Sampling(0.0, 40, 3)], ids=["none", "temperature-0"])
def test_greedy_streams_never_call_set_sampling(sampling):
    log, _, _ = _run(True, sampling)
    assert not [c for c in log if c[0] == "set_sampling"]
    assert [c for c in log if c[0] == "set_slot"]  # (segments did end)
    # and an engine without the method serves them as before
    sch = S.FusedScheduler(GreedyOnlyEngine(max_streams=2), max_chunk=8, to_bytes=False, overlap=False)
    st = sch.open_stream(index=0, dump_size=10)
    st.feed("Hello.")
    assert sch.run_chunk() > 0
    sch.close_stream(st)
    sch.close()


def test_engine_without_set_sampling_raises_at_open_stream():
    sch = S.FusedScheduler(GreedyOnlyEngine(max_streams=2), max_chunk=8, to_bytes=False, overlap=False)
    free = list(sch.free_slots)
    with pytest.raises(RuntimeError, match="set_sampling"):
        sch.open_stream(index=0, dump_size=10, sampling=Sampling(0.8))
    assert sch.free_slots == free and not sch.streams  # nothing was taken
    sch.close()


def test_service_gives_the_replicas_different_seeds():
    from llmvox_amd.server import TTSService
    eng = RecordingEngine(max_streams=4, max_positions=4096)
    svc = TTSService([eng], max_chunk=16, max_tokens=60)
    try:
        sp = Sampling(0.9, 20, seed=99)
        session = svc.submit("Hello there.", sampling=sp)
        audio = b"".join(svc.chunks(session, timeout=0.01))
        assert len(audio) > 0
        greedy = svc.submit("Hello there.")
        b"".join(svc.chunks(greedy, timeout=0.01))
    finally:
        svc.shutdown()
    first = {}
    for c in eng.log:
        if c[0] == "set_sampling" and c[2] > 0:
            first.setdefault(c[1], c)
    assert len(first) == 2
    got = sorted(c[4] for c in first.values())
    assert got == sorted([segment_seed(99, 0, 0), segment_seed(99, 1, 0)]) and got[0] != got[1]
    assert all(c[2:4] == (0.9, 20) for c in first.values())
    # the greedy request that followed on the same slots: the slots were handed back greedy, and it set nothing
    last = {}
    for c in eng.log:
        if c[0] == "set_sampling":
            last[c[1]] = c
    assert all(c[2] == 0.0 for c in last.values())
