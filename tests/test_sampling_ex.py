"""The extended sampling rule on the CPU (top_p, min_p, repetition penalty; include/llmvox.h,
lvx_stream_sampling_ex): tests/sampling_ex_ref.py against the Hugging Face logits processors, ``Sampling``'s
validation, the /tts fields on a fake service and the scheduler's pass-through on a recording engine."""
import math

import numpy as np
import pytest

from llmvox_amd.sampling import Sampling, segment_seed
from tests import sampling_ex_ref as XR

V = XR.VOCAB


# ---- the reference against Hugging Face -------------------------------------------------------------
@pytest.mark.parametrize("T,k,top_p,min_p,R,W", [(1.0, 0, 0.5, 0.0, 1.0, 64), (0.8, 50, 0.9, 0.0, 1.3, 8),
                                                 (0.7, 0, 0.95, 0.05, 1.0, 64), (1.0, 0, 0.9, 0.02, 1.5, 32),
                                                 (0.9, 200, 1.0, 0.1, 0.8, 16)])
def test_kept_set_is_what_hugging_face_leaves_finite(T, k, top_p, min_p, R, W):
    tf = pytest.importorskip("transformers")
    import torch
    procs = [tf.RepetitionPenaltyLogitsProcessor(penalty=float(R)), tf.TemperatureLogitsWarper(float(T))]
    if k:
        procs.append(tf.TopKLogitsWarper(top_k=k))
    if top_p < 1:
        procs.append(tf.TopPLogitsWarper(top_p=float(top_p)))
    if min_p > 0:
        procs.append(tf.MinPLogitsWarper(min_p=float(min_p)))
    rng = np.random.default_rng(int(T * 100) + k)
    compared = 0
    for i in range(40):
        logits = (rng.standard_normal(V) * 3).astype(np.float32)
        window = sorted(set(rng.integers(0, V, size=W).tolist()) | {int(np.argmax(logits))})
        r = XR.rule(logits, T, k, top_p, min_p, R, window)
        # Hugging Face decides min-p on fp32 probabilities: leave out rows with a token within 1e-5 of that boundary,
        # and rows that are not tie-free or whose nucleus the reference calls undetermined
        d = (r.z - r.z.max()).astype(np.float64)
        if not r.determined or len(np.unique(r.z)) < V or (min_p > 0 and np.abs(d - math.log(min_p)).min() < 1e-5):
            continue
        scores = torch.from_numpy(logits)[None]
        ids = torch.tensor([window], dtype=torch.long)
        for p in procs:
            scores = p(ids, scores)
        np.testing.assert_array_equal(np.isfinite(scores[0].numpy()), r.kept, err_msg=f"row {i}")
        compared += 1
    assert compared >= 30


def test_reference_edges():
    row = np.zeros(V, dtype=np.float32)
    row[[5, 1030, 4095]] = 4.0
    # P = 1: only the maximum, and equal maxima stay together
    r = XR.rule(row, 1.0, 0, 2.0 ** -24)
    assert XR.p24(2.0 ** -24) == 1 and XR.p24(1e-12) == 1 and XR.p24(1.0) == 1 << 24
    assert np.nonzero(r.kept)[0].tolist() == [5, 1030, 4095]
    # top_p 1 is off: top-k alone; neutral parameters are sampling_ref's rule
    rng = np.random.default_rng(3)
    row = (rng.standard_normal(V) * 3).astype(np.float32)
    np.testing.assert_array_equal(XR.rule(row, 0.8, 50).kept, XR.SR.kept_set(row, 0.8, 50))
    assert XR.check(row, 0.8, 50, 9, 4)[:2] == XR.SR.check(row, 0.8, 50, 9, 4)
    # the penalty: +2 -> 2 / R, -2 -> -2 R, the zeros keep their signs; it can move the maximum
    row = np.full(V, -1.0, dtype=np.float32)
    row[[1, 2, 3, 4]] = [2.0, -2.0, 0.0, -0.0]
    lp = XR.penalised(row, 1.25, [1, 2, 3, 4, 4])
    assert lp[1] == np.float32(1.6) and lp[2] == np.float32(-2.5)
    assert lp[[3, 4]].view(np.uint32).tolist() == [0, 0x80000000]
    assert XR.window_set([7, 8, 9, 7, 6], 5, 3) == [6, 7, 9] and XR.window_set([7, 8, 9], 3, 256, 2) == [9]
    assert XR.window_set([7, 8], 0, 4) == [] and XR.window_set([7, 8, 9], 2, 4, 2) == []
    # min-p: ln(min_p) in fp32, -inf when off
    assert XR.lnminp(0.0) == -np.inf and XR.lnminp(0.5) == np.float32(math.log(0.5))


# ---- Sampling ------------------------------------------------------------------------------------------
def test_sampling_validation():
    sp = Sampling(0.8, 50, 7)
    assert (sp.top_p, sp.min_p, sp.repetition_penalty, sp.repetition_window) == (1.0, 0.0, 1.0, 64)
    assert not sp.extended and sp.extra() == {}
    sp = Sampling(0.8, 50, 7, 0.9, 0.05, 1.3, 32)  # positional, after seed
    assert sp.extended
    assert sp.extra() == {"top_p": 0.9, "min_p": 0.05, "repetition_penalty": 1.3, "repetition_window": 32}
    assert Sampling(1.0, repetition_penalty=0.5).extended and Sampling(1.0, top_p=1, min_p=0).extra() == {}
    bad = [dict(top_p=0.0), dict(top_p=1.01), dict(top_p=-0.1), dict(top_p=float("nan")), dict(top_p="0.9"),
           dict(top_p=True), dict(top_p=1e-60), dict(min_p=-0.1), dict(min_p=1.0), dict(min_p=float("inf")),
           dict(min_p=1 - 1e-12), dict(repetition_penalty=0.0), dict(repetition_penalty=-1.0),
           dict(repetition_penalty=float("inf")), dict(repetition_penalty=float("nan")), dict(repetition_penalty=1e60),
           dict(repetition_window=0), dict(repetition_window=257), dict(repetition_window=8.0),
           dict(repetition_window=True)]
    for kw in bad:
        with pytest.raises(ValueError):
            Sampling(1.0, **kw)
    for kw in (dict(top_p=1.0), dict(top_p=1e-9), dict(min_p=0.999), dict(repetition_penalty=100.0),
               dict(repetition_window=1), dict(repetition_window=256)):
        Sampling(1.0, **kw)


# ---- /tts ------------------------------------------------------------------------------------------------
class _Service:
    def __init__(self):
        self.error = None
        self.sessions = []
        self.calls = []

    def submit(self, *args, **kw):
        self.calls.append((args, kw))
        return args[0]

    def chunks(self, session):
        yield np.zeros(320, dtype=np.float32).tobytes()


@pytest.fixture
def client_of():
    from fastapi.testclient import TestClient
    from llmvox_amd.server import create_app
    return lambda svc, **kw: TestClient(create_app(svc, **kw))


def test_server_fields_reach_submit(client_of):
    svc = _Service()
    client = client_of(svc)
    body = {"text": "hello.", "temperature": 0.8, "top_k": 50, "seed": 5, "top_p": 0.9, "min_p": 0.05,
            "repetition_penalty": 1.3, "repetition_window": 32}
    assert client.post("/tts", json=body).status_code == 200
    assert svc.calls == [(("hello.",), {"sampling": Sampling(0.8, 50, 5, 0.9, 0.05, 1.3, 32)})]
    # a request that names none of them: the Sampling (and so every engine call) of before
    svc.calls.clear()
    assert client.post("/tts", json={"text": "hello.", "temperature": 0.8, "top_k": 50, "seed": 5}).status_code == 200
    assert svc.calls == [(("hello.",), {"sampling": Sampling(0.8, 50, 5)})] and not svc.calls[0][1]["sampling"].extended
    svc.calls.clear()
    assert client.post("/tts", json={"text": "hello."}).status_code == 200
    assert client.post("/tts", json={"text": "hello.", "top_p": 0.5}).status_code == 200  # greedy: nothing to crop
    assert svc.calls == [(("hello.",), {})] * 2
    # a drawn seed keeps the fields
    svc.calls.clear()
    assert client.post("/tts", json={"text": "a.", "temperature": 1.0, "top_p": 0.5}).status_code == 200
    sp = svc.calls[0][1]["sampling"]
    assert (sp.temperature, sp.top_p, sp.repetition_window) == (1.0, 0.5, 64)


@pytest.mark.parametrize("body", ['{"text": "x", "temperature": 1, "top_p": 0}', '{"text": "x", "temperature": 1, "top_p": 1.5}',
                                  '{"text": "x", "temperature": 1, "top_p": NaN}', '{"text": "x", "top_p": 2}',
                                  '{"text": "x", "temperature": 1, "min_p": 1}', '{"text": "x", "temperature": 1, "min_p": -0.5}',
                                  '{"text": "x", "temperature": 1, "repetition_penalty": 0}',
                                  '{"text": "x", "temperature": 1, "repetition_penalty": Infinity}',
                                  '{"text": "x", "temperature": 1, "repetition_window": 0}',
                                  '{"text": "x", "temperature": 1, "repetition_window": 257}',
                                  '{"text": "x", "temperature": 1, "repetition_window": "wide"}'])
def test_server_invalid_values_give_422(client_of, body):
    svc = _Service()
    r = client_of(svc).post("/tts", content=body, headers={"content-type": "application/json"})
    assert r.status_code == 422, r.text
    assert svc.calls == []


def test_server_defaults_come_from_the_flags(client_of):
    svc = _Service()
    client = client_of(svc, temperature=0.7, top_k=40, top_p=0.92, min_p=0.01, repetition_penalty=1.2, repetition_window=48)
    assert client.post("/tts", json={"text": "a.", "seed": 1}).status_code == 200
    assert client.post("/tts", json={"text": "a.", "seed": 1, "top_p": 0.5, "repetition_window": 8}).status_code == 200
    assert [kw["sampling"] for _, kw in svc.calls] == [Sampling(0.7, 40, 1, 0.92, 0.01, 1.2, 48),
                                                      Sampling(0.7, 40, 1, 0.5, 0.01, 1.2, 8)]
    for kw in (dict(top_p=0.0), dict(min_p=1.0), dict(repetition_penalty=0.0), dict(repetition_window=300)):
        with pytest.raises(ValueError):
            client_of(svc, **kw)
    # the command line reaches create_app: main builds the app from app_options(arg_parser().parse_args(argv))
    import llmvox_amd.server as server
    a = server.arg_parser().parse_args(["--temperature", "0.6", "--top-k", "30", "--top-p", "0.85", "--min-p", "0.02",
                                        "--repetition-penalty", "1.1", "--repetition-window", "16"])
    svc.calls.clear()
    client = client_of(svc, **server.app_options(a))
    assert client.post("/tts", json={"text": "a.", "seed": 2}).status_code == 200
    assert [kw["sampling"] for _, kw in svc.calls] == [Sampling(0.6, 30, 2, 0.85, 0.02, 1.1, 16)]
    d = server.app_options(server.arg_parser().parse_args([]))  # no flag: every new control off
    assert (d["top_p"], d["min_p"], d["repetition_penalty"], d["repetition_window"]) == (1.0, 0.0, 1.0, 64)


# ---- the scheduler ------------------------------------------------------------------------------------------
def _run(sampling, overlap):
    from llmvox_amd import streaming as S
    from test_scheduler_sampling import EOA, TEXT
    from test_service_multidevice import StateEngine

    class Engine(StateEngine):
        def __init__(self, **kw):
            super().__init__(**kw)
            self.log = []

        def set_slot(self, slot, pos, prev=0):
            self.log.append(("set_slot", slot, pos, prev))
            super().set_slot(slot, pos, prev)

        def set_sampling(self, slot, temperature=0.0, top_k=0, seed=0, **kw):
            self.log.append(("set_sampling", slot, temperature, top_k, seed, kw))

    eng = Engine(max_streams=4, max_positions=4096, eoa=EOA)
    sch = S.FusedScheduler(eng, max_chunk=16, to_bytes=False, overlap=overlap, stop_rule=lambda st, ntok, pos: ntok >= 150)
    st = sch.open_stream(index=1, dump_size=10, eoa_id=EOA, sampling=sampling)
    for w in TEXT.split(" "):
        st.feed(w)
    assert sch.run_until_idle(max_chunks=2000) > 0
    slot, segments = st.slot, st.segment
    sch.close_stream(st)
    sch.close()
    return eng.log, slot, segments


@pytest.mark.parametrize("overlap", [False, True], ids=["serial", "overlap"])
def test_scheduler_passes_the_parameters_through(overlap):
    sp = Sampling(0.8, 50, 0xabcdef, top_p=0.9, repetition_penalty=1.3, repetition_window=8)
    log, slot, segments = _run(sp, overlap)
    assert segments >= 2
    sets = [c for c in log if c[0] == "set_sampling"]
    assert len(sets) == segments + 2
    for g, c in enumerate(sets[:-1]):  # every sentence: the same parameters, its own seed (segment_seed is unchanged)
        assert c == ("set_sampling", slot, 0.8, 50, segment_seed(sp.seed, 1, g), sp.extra())
        if g:  # right behind the rewind to position 0: the window never reaches into the previous sentence
            assert log[log.index(c) - 1] == ("set_slot", slot, 0, 0)
    assert sets[-1] == ("set_sampling", slot, 0.0, 0, 0, {})
    # without the new parameters: exactly the calls of before (no keyword at all)
    log, slot, segments = _run(Sampling(0.8, 50, 0xabcdef), overlap)
    assert all(c[5] == {} for c in log if c[0] == "set_sampling")
