"""Nucleus, min-p and repetition-penalty sampling (lvx_stream_sampling_ex, ar_sample_kernel) and the slots'
token history on the GPU, against tests/sampling_ex_ref.py: the select alone over given logits
(lvx_select_probe path 4) with the kept record of lvx_sample_kept, then real decode steps: every GEMM family
from its own logits, the history across graph replays, rewinds, row independence, and the scheduler."""
import ctypes

import numpy as np
import pytest
import torch

from tests import sampling_ex_ref as XR
from tests import sampling_ref as SR
from tests.test_gpu_sampling import _decode, _greedy_all, _schedule

pytestmark = pytest.mark.gpu
V = SR.VOCAB
NEUTRAL = dict(top_p=1.0, min_p=0.0, R=1.0, W=64)


def _engine(dtype, max_streams, max_positions):
    from llmvox_amd.engine import build_engine
    return build_engine(0, dtype, dtype, max_streams=max_streams, max_positions=max_positions, max_codec_frames=64)


@pytest.fixture(scope="module")
def eng32():
    e = _engine("fp32", 4, 512)
    yield e
    e.close()


@pytest.fixture(scope="module")
def eng16():
    e = _engine("bf16", 33, 256)
    yield e
    e.close()


def _set(e, slot, T, k, seed, top_p=1.0, min_p=0.0, R=1.0, W=64):
    e.set_sampling(slot, T, k, seed, top_p=top_p, min_p=min_p, repetition_penalty=R, repetition_window=W)


class Probe:
    """lvx_select_probe path 4 calls over B rows, queued without a synchronisation; ``read`` returns the tokens
    [n, B], the margins [n, B] and the kept records [n, B, 4]."""

    def __init__(self, e, slots):
        self.e, self.dev, self.B = e, e.device, len(slots)
        self.st = torch.tensor(slots, dtype=torch.int32, device=self.dev)
        self.plan = torch.full((self.B, 2), 97, dtype=torch.int32, device=self.dev)
        self.out = []

    def __call__(self, logits):
        rowstep = torch.zeros(self.B, dtype=torch.int32, device=self.dev)
        tok = torch.full((self.B, 2), -7, dtype=torch.int32, device=self.dev)
        marg = torch.full((self.B, 2), -1.0, dtype=torch.float32, device=self.dev)
        lg = logits if isinstance(logits, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(logits, dtype=np.float32))
        self.e.select_probe(4, self.st, lg, self.plan, rowstep, tok, marg)
        self.out.append((tok, marg, self.e.sample_kept(self.B)))

    def read(self):
        torch.cuda.synchronize()
        self.e.check_errors()
        tok = np.stack([t[:, 0].cpu().numpy() for t, _, _ in self.out])
        marg = np.stack([m[:, 0].cpu().numpy() for _, m, _ in self.out])
        rec = np.stack([r.cpu().numpy() for _, _, r in self.out])
        self.out = []
        return tok, marg, rec


def _place(e, slot, p, history=(), jump_from=None):
    """The slot at position p with history[0 .. p) known; jump_from: the slot at position ``jump_from`` with the
    whole history known first, then lvx_stream_set to p: forward (p > jump_from) leaves only entry p - 1 known,
    a rewind keeps what is known below p."""
    e.reset_slot(slot)
    history = [int(t) for t in history]
    if jump_from is not None:
        e.set_slot(slot, jump_from, 0)
        e.write_history(slot, 0, history)
        e.set_slot(slot, p, history[p - 1] if p else 0)
        return
    if not history:  # (a case that looks at no history)
        e.set_slot(slot, p, 0)
        return
    e.set_slot(slot, p, history[p - 1] if p else 0)
    if p:
        e.write_history(slot, 0, history[:p])


def _one(e, slot, row, p, T, k, seed, history=(), jump_from=None, hist_from=0, what="", **kw):
    """One probe of one row at position p, checked against the reference (token, kept record); returns
    (token, margin, record, Rule)."""
    _set(e, slot, T, k, seed, **kw)
    _place(e, slot, p, history, jump_from)
    pr = Probe(e, [slot])
    pr(row[None])
    tok, marg, rec = pr.read()
    par = {**NEUTRAL, **kw}
    window = XR.window_set(history, p, par["W"], hist_from) if len(history) else []
    tally = XR.Tally()
    tally.add(tok[0, 0], rec[0, 0], row, T, k, seed, p, par["top_p"], par["min_p"], par["R"], window, what=what)
    assert e.slot_position(slot) == p + 1
    assert e.stream_history(slot, p, 1).cpu().tolist() == [int(tok[0, 0])], what  # the commit recorded the token
    return int(tok[0, 0]), marg[0, 0], rec[0, 0], XR.rule(row, T, k, par["top_p"], par["min_p"], par["R"], window)


# ---- neutral parameters: the kernel of before ------------------------------------------------------------
def test_neutral_parameters_draw_the_tokens_of_lvx_stream_sampling(eng32):
    from llmvox_amd import _lib
    e, lib = eng32, _lib.load()
    slots = [3, -1, 0, 2]
    params = {3: (1.0, 0, 0x0123456789abcdef), 0: (0.7, 40, 0xfedcba9876543210), 2: (0.25, 5, 42)}
    n = 128
    logits = (np.random.default_rng(2024).standard_normal((n, 4, V)) * 3).astype(np.float32)
    lg = torch.from_numpy(logits).to(e.device)
    runs = []
    try:
        for ex in (False, True):
            for s, (T, k, seed) in params.items():
                if ex:
                    _set(e, s, T, k, seed, **NEUTRAL)
                else:
                    _lib.check(lib.lvx_stream_sampling(e.h, s, ctypes.c_float(T), k, seed, e.stream_handle()))
                e.reset_slot(s)
                e.write_history(s, 0, list(range(100, 164)))  # (a history the neutral penalty must not look at)
            pr = Probe(e, slots)
            for i in range(n):
                pr(lg[i])
            runs.append(pr.read())
    finally:
        _greedy_all(e)
    (tok_a, marg_a, rec_a), (tok_b, marg_b, rec_b) = runs
    np.testing.assert_array_equal(tok_a, tok_b)
    np.testing.assert_array_equal(marg_a.view(np.uint32), marg_b.view(np.uint32))
    np.testing.assert_array_equal(rec_a, rec_b)
    for b, s in enumerate(slots):
        if s < 0:
            continue
        T, k, seed = params[s]
        tally = SR.Tally()
        for i in range(n):
            tally.add(tok_b[i, b], logits[i, b], T, k, seed, i, what=f"row {b} call {i}")
            z = SR.scaled(logits[i, b], T)
            kept = SR.kept_set(logits[i, b], T, k)
            assert rec_b[i, b].tolist() == [int(kept.sum()), int(z[kept].min().view(np.int32)), 0, 0]
        tally.assert_cap(SR.AMBIGUOUS_CAP_FULL if k == 0 else SR.AMBIGUOUS_CAP_TOPK, f"T={T} k={k}")


# ---- the nucleus ----------------------------------------------------------------------------------------------
def test_nucleus_edges(eng32):
    e = eng32
    rng = np.random.default_rng(11)
    try:
        # P = 1, only the maximum: two equal maxima in different waves (threads 0 and 187) are both kept
        row = (rng.standard_normal(V) * 3).astype(np.float32)
        row[[10, 3000]] = row.max() + np.float32(1.0)
        assert XR.p24(2.0 ** -24) == 1
        got = set()
        for p in range(16):
            tok, _, rec, r = _one(e, 0, row, p, 0.9, 0, 11, top_p=2.0 ** -24, what=f"P=1 p={p}")
            assert r.determined and rec[0] == 2 and tok in (10, 3000)
            got.add(tok)
        assert got == {10, 3000}

        # top_p = 1 with top_k = 50 is top-k alone
        row = (rng.standard_normal(V) * 3).astype(np.float32)
        for p in (0, 7, 100):
            tok, _, rec, _ = _one(e, 1, row, p, 0.8, 50, 0xabc, top_p=1.0, what="top_p=1")
            e.set_sampling(1, 0.8, 50, 0xabc)
            _place(e, 1, p)
            pr = Probe(e, [1])
            pr(row[None])
            tok0, _, rec0 = pr.read()
            assert tok == tok0[0, 0] and rec[0] == 50 and rec.tolist() == rec0[0, 0].tolist()

        # the boundary inside three equal logits (threads 0, 64 and 255): w = 1, then 3 x ~0.5; the mass above the
        # three is 0.4 of the total < 0.5, one of them alone would already pass 0.5: all three stay, the rest goes
        row = np.full(V, -40.0, dtype=np.float32)
        row[2] = 3.0
        row[[5, 1030, 4095]] = np.float32(3.0 - 0.6931)
        seen = set()
        for p in range(12):
            tok, _, rec, r = _one(e, 2, row, p, 1.0, 0, 77, top_p=0.5, what=f"three equal p={p}")
            assert r.determined and rec[0] == 4 and np.nonzero(r.kept)[0].tolist() == [2, 5, 1030, 4095]
            seen.add(tok)
        assert len(seen) >= 3
        # (a little less mass wanted: only the maximum)
        tok, _, rec, r = _one(e, 2, row, 0, 1.0, 0, 77, top_p=0.39, what="three equal, 0.39")
        assert r.determined and rec[0] == 1 and tok == 2

        # top_k = 50, then top_p = 0.9: the mass is over the top-k survivors
        row = (rng.standard_normal(V) * 1.5).astype(np.float32)
        full, crop = XR.rule(row, 1.0, 0, 0.9), XR.rule(row, 1.0, 50, 0.9)
        assert full.determined and crop.determined and crop.kept.sum() < 50 < full.kept.sum()
        for p in range(8):
            tok, _, rec, _ = _one(e, 3, row, p, 1.0, 50, 5, top_p=0.9, what=f"top-k then top-p p={p}")
            assert rec[0] == int(crop.kept.sum())
    finally:
        _greedy_all(e)


# ---- min-p ------------------------------------------------------------------------------------------------------
def test_min_p_boundary_is_exact(eng32):
    e = eng32
    try:
        for min_p in (0.25, 0.1, 0.003):
            L = XR.lnminp(min_p)
            row = np.full(V, -50.0, dtype=np.float32)
            row[7], row[100], row[2000] = 0.0, L, np.nextafter(L, np.float32(-np.inf))
            for p in (0, 3):
                tok, _, rec, r = _one(e, 0, row, p, 1.0, 0, 9 + p, min_p=min_p, what=f"min_p={min_p}")
                assert np.nonzero(r.kept)[0].tolist() == [7, 100]
                assert rec.tolist() == [2, int(L.view(np.int32)), 0, 0] and tok in (7, 100)
        # with a temperature: the boundary is on fl(z - zmax)
        rng = np.random.default_rng(5)
        row = (rng.standard_normal(V) * 3).astype(np.float32)
        for p in range(8):
            _one(e, 1, row, p, 0.7, 0, 31, min_p=0.05, what=f"min_p 0.05 p={p}")
            _one(e, 1, row, p, 0.7, 100, 31, top_p=0.95, min_p=0.02, what=f"all crops p={p}")
    finally:
        _greedy_all(e)


# ---- the repetition penalty ------------------------------------------------------------------------------
def test_penalty_cases(eng32):
    e = eng32
    rng = np.random.default_rng(21)
    try:
        # +2, -2, +0, -0 in the window, R = 1.25: 2 / R = 1.6 and -2 R = -2.5, visible as the lowest kept z
        hist = [40, 41, 42, 43]
        row = np.full(V, 3.0, dtype=np.float32)
        row[[40, 41, 42, 43]] = [2.0, -2.0, 0.0, -0.0]
        tok, _, rec, r = _one(e, 0, row, 4, 1.0, 0, 1, history=hist, R=1.25, W=4, what="signs, no crop")
        assert rec.tolist() == [V, int(np.float32(-2.5).view(np.int32)), 4, 0]
        row = np.full(V, 1.0, dtype=np.float32)
        row[100:110] = 5.0
        row[[40, 41, 42, 43]] = [2.0, -2.0, 0.0, -0.0]
        tok, _, rec, r = _one(e, 0, row, 4, 1.0, 11, 1, history=hist, R=1.25, W=4, what="signs, top_k 11")
        assert rec.tolist() == [11, int(np.float32(1.6).view(np.int32)), 4, 0] and r.z[40] == np.float32(1.6)

        # the raw argmax in the window, pushed under the runner-up: zmax moves (min-p is taken from the new one),
        # the margin stays that of the raw logits
        row = np.clip(rng.standard_normal(V), -3, 2).astype(np.float32)
        row[50], row[60], row[70] = 4.0, 3.5, 3.0
        tok, marg, rec, r = _one(e, 1, row, 2, 1.0, 0, 3, history=[50, 50], R=2.0, W=8, min_p=0.5, what="zmax moves")
        assert np.nonzero(r.kept)[0].tolist() == [60, 70] and rec.tolist()[:3] == [2, int(np.float32(3.0).view(np.int32)), 1]
        assert marg == np.float32(0.5)

        # generic rows: the window's tokens carry the largest logits, so a wrong window set moves zmax and the crop
        def generic(history, p, W, slot, what, **kw):
            row = (rng.standard_normal(V) * 3).astype(np.float32)
            for i, t in enumerate(sorted(set(history))):
                row[t] = np.float32(12.0 + 0.37 * i)
            return _one(e, slot, row, p, 0.9, 0, 1234 + p, history=history, R=1.7, W=W, min_p=0.2, top_p=0.98,
                        what=what, **kw)

        _, _, rec, _ = generic([5, 5, 5, 9, 9, 700], 6, 64, 2, "duplicates")
        assert rec[2] == 3
        _, _, rec, _ = generic([11, 12, 13], 3, 1, 2, "W = 1")
        assert rec[2] == 1
        _, _, rec, _ = generic([11, 4095, 0], 3, 256, 2, "W = 256 at p = 3")
        assert rec[2] == 3
        _, _, rec, _ = generic([11, 12, 13], 0, 64, 2, "p = 0")
        assert rec[2] == 0
        h = rng.integers(0, V, size=300).tolist()
        _, _, rec, _ = generic(h, 300, 256, 3, "W = 256, full")
        assert rec[2] == len(set(h[44:]))
        _, _, rec, _ = generic(h, 300, 64, 3, "W = 64")
        assert rec[2] == len(set(h[236:]))
        # a window cut by hist_from: history written, then a forward lvx_stream_set over positions never decoded
        h20 = rng.integers(0, V, size=20).tolist()
        _, _, rec, _ = generic(h20, 20, 8, 3, "forward set", jump_from=3, hist_from=19)
        assert rec[2] == 1
        # a rewind keeps what is known below it
        _, _, rec, _ = generic(h20, 12, 8, 3, "rewind", jump_from=15, hist_from=0)
        assert rec[2] == len(set(h20[4:12]))
    finally:
        _greedy_all(e)


def test_a_slot_that_starts_sampling_knows_no_earlier_token(eng32):
    e = eng32
    try:
        _greedy_all(e)
        e.reset_slot(0)
        e.write_history(0, 0, [7, 8, 9, 10, 11, 12])
        e.set_slot(0, 6, 12)
        row = (np.random.default_rng(2).standard_normal(V) * 3).astype(np.float32)
        row[[7, 8, 9, 10, 11, 12]] = 9.0
        _set(e, 0, 1.0, 0, 5, R=1.5, W=16)  # temperature 0 -> 1: hist_from = 6
        pr = Probe(e, [0])
        pr(row[None])
        pr(row[None])
        tok, _, rec = pr.read()
        assert rec[0, 0, 2] == 0 and rec[1, 0, 2] == 1  # then only its own token of position 6
        t = XR.Tally()
        t.add(tok[0, 0], rec[0, 0], row, 1.0, 0, 5, 6, R=1.5, window=[], what="first step")
        t.add(tok[1, 0], rec[1, 0], row, 1.0, 0, 5, 7, R=1.5, window=[int(tok[0, 0])], what="second step")
    finally:
        _greedy_all(e)


# ---- statistical cases ------------------------------------------------------------------------------------------
def test_nucleus_against_the_reference_400_draws(eng32):
    """Shares of the reference alone on these 400 rows per case (integer rule, float64 exp, EPS = 2^-16): rows
    with an undetermined nucleus 0 %, 0 %, 4.0 %, 7.0 % (cap 8 %); draws with more than one acceptable token
    0.25 %, 0 %, 0.25 %, 0.5 % (cap AMBIGUOUS_CAP_FULL). The run prints both for the device's tokens. These shares
    belong to seed 99 and 400 rows: they are the reference's own, fixed with the rows, and the last case lies
    one point under its cap, so another seed or row count can pass the cap with a correct kernel (the issue
    measured 5.75 % on its rows); re-measure on the CPU (XR.rule(...).determined) before changing either."""
    e = eng32
    cases = [(1.0, 0, 0.5), (0.8, 50, 0.9), (0.7, 0, 0.95), (1.0, 0, 0.9)]
    n = 400
    logits = (np.random.default_rng(99).standard_normal((n, 4, V)) * 3).astype(np.float32)
    lg = torch.from_numpy(logits).to(e.device)
    seeds = [0x5eed0000 + 977 * b for b in range(4)]
    try:
        for b, (T, k, top_p) in enumerate(cases):
            _set(e, b, T, k, seeds[b], top_p=top_p)
            e.reset_slot(b)
        pr = Probe(e, [0, 1, 2, 3])
        for i in range(n):  # the commit advances the positions: the counters run 0 .. 399
            pr(lg[i])
        tok, _, rec = pr.read()
        assert [e.slot_position(b) for b in range(4)] == [n] * 4
    finally:
        _greedy_all(e)
    for b, (T, k, top_p) in enumerate(cases):
        tally = XR.Tally()
        for i in range(n):
            tally.add(tok[i, b], rec[i, b], logits[i, b], T, k, seeds[b], i, top_p=top_p, what=f"case {b} draw {i}")
        tally.assert_caps(SR.AMBIGUOUS_CAP_FULL, f"T={T} k={k} top_p={top_p}")
        assert len(set(tok[:, b].tolist())) > 8


# ---- real steps ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,B", [("bf16", 1), ("bf16", 4), ("bf16", 9), ("bf16", 33), ("fp32", 1), ("fp32", 4)])
def test_every_path_samples_from_its_own_logits_and_history(dtype, B, eng16, eng32):
    e = eng16 if dtype == "bf16" else eng32
    dev = e.device
    T, k, top_p, R, W, steps = 0.8, 0, 0.9, 1.3, 8, 12
    slots = list(range(B))
    seeds = [0x9e3779b97f4a7c15 * (s + 3) & (2 ** 64 - 1) for s in slots]
    plan = torch.from_numpy(np.random.default_rng(B).integers(3, 384, size=(B, steps)).astype(np.int32)).to(dev)
    st = torch.tensor(slots, dtype=torch.int32, device=dev)
    rowstep = torch.zeros(B, dtype=torch.int32, device=dev)
    tok = torch.full((B, steps), -7, dtype=torch.int32, device=dev)
    tally = XR.Tally()
    hist = np.zeros((B, steps), dtype=np.int64)
    try:
        for s in slots:
            _set(e, s, T, k, seeds[s], top_p=top_p, R=R, W=W)
            e.reset_slot(s)
        for j in range(steps):
            e.ar_steps(1, st, plan, rowstep, tok)
            logits = e.last_logits(B).cpu().numpy()
            rec = e.sample_kept(B).cpu().numpy()
            hist[:, j] = tok[:, j].cpu().numpy()
            for b in range(B):
                tally.add(hist[b, j], rec[b], logits[b], T, k, seeds[b], j, top_p=top_p, R=R,
                          window=XR.window_set(hist[b], j, W), what=f"{dtype} B={B} row {b} step {j}")
        e.check_errors()
        for b in (0, B - 1):
            assert e.stream_history(b, 0, steps).cpu().tolist() == hist[b].tolist()
    finally:
        _greedy_all(e)
    print(f"{dtype} B={B}: {tally.undetermined} undetermined, {tally.ambiguous} ambiguous of {tally.n}")


def test_history_records_across_graph_replays(eng16):
    e = eng16
    try:
        _greedy_all(e)
        _set(e, 0, 0.8, 50, 77, top_p=0.9, R=1.3, W=8)
        tok, rowstep, pos, _ = _decode(e, [0, 1], [40])  # graphs of 16 steps, then one-step graphs
        assert pos == [40, 40]
        for s in (0, 1):  # the sampling slot, and the greedy slot beside it
            assert e.stream_history(s, 0, 40).cpu().tolist() == tok[s].tolist()
        eager, *_ = _decode(e, [0, 1], [40], graphs=False)
        np.testing.assert_array_equal(eager, tok)
    finally:
        _greedy_all(e)


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_rewind_reproduces_the_tokens_and_keeps_the_history(dtype, eng16, eng32):
    e = eng16 if dtype == "bf16" else eng32
    slots = [0, 1]
    try:
        for s in slots:
            _set(e, s, 0.9, 0, 300 + s, top_p=0.95, R=1.5, W=16)
        first = _decode(e, slots, [24])
        for s in slots:
            e.set_slot(s, 14, int(first[0][s, 13]))
        for s in slots:  # the run-ahead's entries above the rewind point are still there, those below intact
            assert e.stream_history(s, 0, 24).cpu().tolist() == first[0][s].tolist()
        again = _decode(e, slots, [10], plan=first[3], rowstep0=14, reset=False)
        np.testing.assert_array_equal(again[0][:, 14:24], first[0][:, 14:24])
        assert again[2] == [24, 24]
        for s in slots:
            assert e.stream_history(s, 0, 24).cpu().tolist() == first[0][s].tolist()
        # (the penalty mattered: without it the stream differs)
        for s in slots:
            _set(e, s, 0.9, 0, 300 + s, top_p=0.95)
        plain = _decode(e, slots, [24], plan=first[3])
        assert (plain[0] != first[0]).any()
    finally:
        _greedy_all(e)


def test_row_independence(eng32):
    e = eng32
    rng = np.random.default_rng(8)
    rows = (rng.standard_normal((4, V)) * 3).astype(np.float32)
    h = rng.integers(0, V, size=40).tolist()
    for t in h[-16:]:
        rows[0, t] += 6.0
    rows[3] = rows[0]
    par = dict(top_p=0.9, min_p=0.01, R=1.4, W=16)
    try:
        for p in (1, 17, 40):
            _set(e, 2, 0.8, 60, 0xfeed, **par)
            _place(e, 2, p, h)
            one = Probe(e, [2])
            one(rows[:1])
            tok1, _, rec1 = one.read()
            for s, seed in ((0, 1), (3, 2), (1, 0xfeed)):
                _set(e, s, 0.8, 60, seed, **par)
                _place(e, s, p, h if s == 1 else h[::-1])
            four = Probe(e, [0, 3, 2, 1])  # slot 1 in row 3: the same (seed, position, logits, history)
            _set(e, 2, 0.0, 0, 0)
            four(rows)
            tok4, _, rec4 = four.read()
            assert tok1[0, 0] == tok4[0, 3] and rec1[0, 0].tolist() == rec4[0, 3].tolist()
            assert tok4[0, 2] == int(np.argmax(rows[2]))  # (slot 2 is greedy now)
            t = XR.Tally()
            t.add(tok4[0, 3], rec4[0, 3], rows[3], 0.8, 60, 0xfeed, p, par["top_p"], par["min_p"], par["R"],
                  XR.window_set(h, p, 16), what=f"p={p}")
    finally:
        _greedy_all(e)


def test_arguments(eng32):
    from llmvox_amd import _lib
    e, lib = eng32, _lib.load()
    ok = dict(temperature=1.0, top_k=0, top_p=1.0, min_p=0.0, repetition_penalty=1.0, repetition_window=64, seed=0)
    bad = [("top_p", 0.0), ("top_p", 1.5), ("top_p", float("nan")), ("min_p", 1.0), ("min_p", -0.1),
           ("min_p", float("nan")), ("repetition_penalty", 0.0), ("repetition_penalty", float("inf")),
           ("repetition_penalty", float("nan")), ("repetition_window", 0), ("repetition_window", 257),
           ("temperature", -1.0), ("top_k", -1)]
    for name, v in bad:
        p = _lib.LvxSampling(**{**ok, name: v})
        assert lib.lvx_stream_sampling_ex(e.h, 0, ctypes.byref(p), e.stream_handle()) == _lib.LVX_E_ARG, (name, v)
        assert name in lib.lvx_last_error().decode()
    p = _lib.LvxSampling(**ok)
    assert lib.lvx_stream_sampling_ex(e.h, e.max_streams, ctypes.byref(p), e.stream_handle()) == _lib.LVX_E_ARG
    assert lib.lvx_stream_sampling_ex(e.h, 0, None, e.stream_handle()) == _lib.LVX_E_ARG
    with pytest.raises(_lib.LvxArgError):
        e.set_sampling(0, 1.0, top_p=0.0)
    t = torch.zeros(8, dtype=torch.int32, device=e.device)
    for args, code in (((-1, 0, 8), _lib.LVX_E_ARG), ((e.max_streams, 0, 8), _lib.LVX_E_ARG), ((0, -1, 8), _lib.LVX_E_CAPACITY),
                       ((0, 0, 0), _lib.LVX_E_CAPACITY), ((0, 505, 8), _lib.LVX_E_CAPACITY)):
        for write in (0, 1):
            assert lib.lvx_stream_history(e.h, *args, t.data_ptr(), write, e.stream_handle()) == code, args
    assert lib.lvx_stream_history(e.h, 0, 0, 8, None, 0, e.stream_handle()) == _lib.LVX_E_ARG
    assert lib.lvx_stream_history(e.h, 0, 504, 8, t.data_ptr(), 0, e.stream_handle()) == 0
    assert lib.lvx_sample_kept(e.h, 0, t.data_ptr(), e.stream_handle()) == _lib.LVX_E_ARG
    assert lib.lvx_sample_kept(e.h, 1, None, e.stream_handle()) == _lib.LVX_E_ARG
    torch.cuda.synchronize()
    _greedy_all(e)


# ---- the scheduler on the device ------------------------------------------------------------------------------
def test_scheduler_overlap_and_serial_deliver_the_same_items(eng32):
    from llmvox_amd.sampling import Sampling
    e = eng32
    sp = Sampling(0.8, 50, seed=20240607, top_p=0.9, min_p=0.01, repetition_penalty=1.3, repetition_window=32)
    free = _schedule(e, False, sp, 453)
    eoa = free[0][1][23]  # the token stream 0 draws at step 23 becomes the end-of-audio id
    ser = _schedule(e, False, sp, eoa)
    ovl = _schedule(e, True, sp, eoa)
    assert any(isinstance(x, int) for x in ser[0][0])  # a segment did end
    assert ser[0][1][:ser[0][1].index(eoa)] == free[0][1][:free[0][1].index(eoa)]
    for (a_ev, a_tok), (b_ev, b_tok) in zip(ser, ovl):
        assert len(a_ev) > 0 and len(a_ev) == len(b_ev)
        assert a_tok == b_tok
        for x, y in zip(a_ev, b_ev):
            assert type(x) is type(y) and x == y  # PCM bytes included
    plain = _schedule(e, False, Sampling(0.8, 50, seed=20240607), eoa)
    assert plain[0][1] != ser[0][1]  # (the new parameters reached the device)
    a = _decode(e, [0, 1], [8])  # the slots were handed back greedy
    assert (a[0] >= 0).all()
