"""Seeded temperature / top-k sampling of the decode step (lvx_stream_sampling, ar_sample_kernel,
SEL_SAMPLE) on the GPU, against the CPU reference of tests/sampling_ref.py: the select alone over
given logits (lvx_select_probe path 4), greedy rows beside sampled ones, every GEMM family step by
step, graph replays / call splits / rewinds, the argument checks, and the scheduler's two schedules
on a sampled stream."""
import numpy as np
import pytest
import torch

from tests import sampling_ref as SR

pytestmark = pytest.mark.gpu
V = SR.VOCAB


def _engine(dtype, max_streams):
    from llmvox_amd.engine import build_engine
    return build_engine(0, dtype, dtype, max_streams=max_streams, max_positions=256, max_codec_frames=64)


@pytest.fixture(scope="module")
def eng32():
    e = _engine("fp32", 4)
    yield e
    e.close()


@pytest.fixture(scope="module")
def eng16():
    e = _engine("bf16", 33)
    yield e
    e.close()


def _greedy_all(e):
    for s in range(e.max_streams):
        e.set_sampling(s, 0.0, 0, 0)


def _probe(e, path, slots, logits, pos, stride=2):
    """One lvx_select_probe over logits [B, V] with every live slot at position ``pos`` (a list per row or an int)."""
    dev = e.device
    B = len(slots)
    for b, s in enumerate(slots):
        if s >= 0:
            e.set_slot(s, pos[b] if isinstance(pos, (list, tuple)) else pos, 0)
    st = torch.tensor(slots, dtype=torch.int32, device=dev)
    plan = torch.full((B, stride), 97, dtype=torch.int32, device=dev)
    rowstep = torch.zeros(B, dtype=torch.int32, device=dev)
    tok = torch.full((B, stride), -7, dtype=torch.int32, device=dev)
    marg = torch.full((B, stride), -1.0, dtype=torch.float32, device=dev)
    e.select_probe(path, st, torch.from_numpy(np.ascontiguousarray(logits, dtype=np.float32)), plan, rowstep, tok, marg)
    torch.cuda.synchronize()
    e.check_errors()
    newpos = [e.slot_position(s) if s >= 0 else None for s in slots]
    return tok.cpu().numpy(), marg.cpu().numpy(), rowstep.cpu().numpy(), newpos


# ---- 5. the select alone against the reference --------------------------------------------------------
def test_probe_matches_the_reference(eng32):
    e, dev = eng32, eng32.device
    slots = [3, -1, 0, 2]
    params = {3: (1.0, 0, 0x0123456789abcdef), 0: (0.7, 40, 0xfedcba9876543210), 2: (0.25, 5, 42)}
    n = 128
    rng = np.random.default_rng(2024)
    logits = (rng.standard_normal((n, 4, V)) * 3).astype(np.float32)
    try:
        for s, (T, k, seed) in params.items():
            e.set_sampling(s, T, k, seed)
            e.reset_slot(s)
        st = torch.tensor(slots, dtype=torch.int32, device=dev)
        lg = torch.from_numpy(logits).to(dev)
        plan = torch.full((4, 2), 97, dtype=torch.int32, device=dev)
        rowstep = torch.zeros(n, 4, dtype=torch.int32, device=dev)
        tok = torch.full((n, 4, 2), -7, dtype=torch.int32, device=dev)
        marg = torch.full((n, 4, 2), -1.0, dtype=torch.float32, device=dev)
        for i in range(n):  # the commit advances the positions: the counters run 0..127
            e.select_probe(4, st, lg[i], plan, rowstep[i], tok[i], marg[i])
        torch.cuda.synchronize()
        e.check_errors()
        assert [e.slot_position(s) for s in (3, 0, 2)] == [n] * 3
    finally:
        _greedy_all(e)
    tok, marg, rowstep = tok.cpu().numpy(), marg.cpu().numpy(), rowstep.cpu().numpy()
    for b, s in enumerate(slots):
        if s < 0:  # the idle row's outputs are untouched
            assert (tok[:, b] == -7).all() and (marg[:, b] == -1.0).all() and (rowstep[:, b] == 0).all()
            continue
        T, k, seed = params[s]
        tally = SR.Tally()
        for i in range(n):
            tally.add(tok[i, b, 0], logits[i, b], T, k, seed, i, what=f"row {b} call {i}")
            top2 = np.sort(logits[i, b])[-2:]
            assert marg[i, b, 0] == np.float32(top2[1] - top2[0])  # the raw logits' margin
        assert (tok[:, b, 1] == -7).all() and (rowstep[:, b] == 1).all()
        tally.assert_cap(SR.AMBIGUOUS_CAP_FULL if k == 0 else SR.AMBIGUOUS_CAP_TOPK, f"T={T} k={k}")
        if k == 0:
            assert len(set(tok[:, b, 0].tolist())) > 16  # (a draw, not a constant)


def test_probe_edge_cases(eng32):
    e = eng32
    rng = np.random.default_rng(7)
    try:
        # k = 1: the token is in the tie set of the maximum (of z), whatever u is
        row = (rng.standard_normal(V) * 3).astype(np.float32)
        row[[100, 2000, 4095]] = row.max() + np.float32(1.0)
        e.set_sampling(0, 0.9, 1, 11)
        ties = set(np.nonzero(SR.kept_set(row, 0.9, 1))[0].tolist())
        assert ties == {100, 2000, 4095}
        got = set()
        for pos in range(24):
            tok, *_ = _probe(e, 4, [0], row[None], pos)
            ref, acc = SR.check(row, 0.9, 1, 11, pos)
            assert int(tok[0, 0]) in ties and int(tok[0, 0]) in acc
            got.add(int(tok[0, 0]))
        assert len(got) >= 2

        # k = 4096 and k = 0 agree (no crop), in different slots and rows at the same (seed, position)
        rows = (rng.standard_normal((2, V)) * 3).astype(np.float32)
        rows[1] = rows[0]
        e.set_sampling(1, 1.3, 4096, 5)
        e.set_sampling(2, 1.3, 0, 5)
        for pos in (0, 9, 77):
            tok, *_ = _probe(e, 4, [1, 2], rows, pos)
            assert tok[0, 0] == tok[1, 0]
            assert int(tok[0, 0]) in SR.check(rows[0], 1.3, 0, 5, pos)[1]

        # ties across the k-th value (a 0.25 grid): the token is always in the kept set, and acceptable
        grid = (np.round(rng.standard_normal(V) * 3 * 4) / 4).astype(np.float32)
        tied = [k for k in range(2, 400) if SR.kept_set(grid, 0.5, k).sum() > k]  # k that cut through a tie
        for k in (next(k for k in tied if k >= lo) for lo in (2, 40, 300)):
            kept = SR.kept_set(grid, 0.5, k)
            assert kept.sum() > k
            e.set_sampling(3, 0.5, k, 1000 + k)
            tally = SR.Tally()
            for pos in range(16):
                tok, *_ = _probe(e, 4, [3], grid[None], pos)
                assert kept[int(tok[0, 0])]
                tally.add(tok[0, 0], grid, 0.5, k, 1000 + k, pos, what=f"grid k={k} pos={pos}")

        # an all-equal row: uniform over the vocabulary (exempt from the cap, held to the acceptable set)
        flat = np.full(V, 1.5, dtype=np.float32)
        e.set_sampling(0, 1.0, 0, 77)
        seen = set()
        for pos in range(16):
            tok, marg, *_ = _probe(e, 4, [0], flat[None], pos)
            ref, acc = SR.check(flat, 1.0, 0, 77, pos)
            assert int(tok[0, 0]) in acc and abs(int(tok[0, 0]) - ref) <= 1 and marg[0, 0] == 0.0
            seen.add(int(tok[0, 0]))
        assert len(seen) == 16
        e.set_sampling(0, 1.0, 7, 77)  # (every index ties at the threshold: all kept)
        tok, *_ = _probe(e, 4, [0], flat[None], 3)
        assert int(tok[0, 0]) in SR.check(flat, 1.0, 7, 77, 3)[1]

        # T = 1e-3: the distribution collapses onto the maximum
        row = (rng.standard_normal(V) * 3).astype(np.float32)
        e.set_sampling(0, 1e-3, 0, 3)
        for pos in range(4):
            tok, *_ = _probe(e, 4, [0], row[None], pos)
            assert tok[0, 0] == int(np.argmax(row))

        # the same (seed, position, logits) in different slots and batch rows: the same token
        rows = (rng.standard_normal((4, V)) * 3).astype(np.float32)
        rows[3] = rows[0]
        e.set_sampling(2, 0.8, 50, 0xabcdef0123)
        e.set_sampling(1, 0.8, 50, 0xabcdef0123)
        e.set_sampling(0, 0.8, 50, 1)
        e.set_sampling(3, 0.8, 50, 2)
        for pos in (0, 31, 150):
            tok, *_ = _probe(e, 4, [2, 0, 3, 1], rows, pos)
            assert tok[0, 0] == tok[3, 0]
            assert int(tok[0, 0]) in SR.check(rows[0], 0.8, 50, 0xabcdef0123, pos)[1]
    finally:
        _greedy_all(e)


# ---- 6. greedy rows are the argmax kernel ------------------------------------------------------------
def test_greedy_rows_of_a_sampling_step_are_the_argmax_kernel(eng32):
    from tests.select_cases import near_tie_rows
    e = eng32
    try:
        e.set_sampling(2, 0.8, 50, 9)
        for rep in range(6):
            rows = near_tie_rows(4, seed=500 + rep) if rep < 4 else \
                (np.random.default_rng(rep).standard_normal((4, V)) * 3).astype(np.float32)
            slots = [0, 2, 1, 3]
            ref = _probe(e, 0, slots, rows, 5)
            got = _probe(e, 4, slots, rows, 5)
            for b in (0, 2, 3):  # the greedy rows: tokens, margins, rowstep, positions
                np.testing.assert_array_equal(got[0][b], ref[0][b])
                np.testing.assert_array_equal(got[1][b].view(np.uint32), ref[1][b].view(np.uint32))
                assert got[2][b] == ref[2][b] == 1 and got[3][b] == ref[3][b] == 6
            assert int(got[0][1, 0]) in SR.check(rows[1], 0.8, 50, 9, 5)[1]
            assert got[1][1, 0] == ref[1][1, 0] and got[2][1] == 1 and got[3][1] == 6
    finally:
        _greedy_all(e)


def _decode(e, slots, calls, graphs=True, seed=0, plan=None, rowstep0=0, reset=True, B_plan_seed=None):
    """lvx_ar_steps calls on a side stream (graphs) or the current stream one by one (eager)."""
    dev = e.device
    B, n = len(slots), sum(calls) + rowstep0
    if plan is None:
        rng = np.random.default_rng(B * 31 + 5 if B_plan_seed is None else B_plan_seed)
        plan = rng.integers(3, 384, size=(B, n)).astype(np.int32)
    plan_d = torch.from_numpy(plan[:, :n].copy()).to(dev)
    if reset:
        for s in slots:
            if s >= 0:
                e.reset_slot(s)
    st = torch.tensor(slots, dtype=torch.int32, device=dev)
    rowstep = torch.full((B,), rowstep0, dtype=torch.int32, device=dev)
    tok = torch.full((B, n), -7, dtype=torch.int32, device=dev)
    margin = torch.zeros(B, n, dtype=torch.float32, device=dev)
    e.set_graphs(graphs)
    main = torch.cuda.current_stream(dev)
    side = torch.cuda.Stream(device=dev) if graphs else None
    if side is not None:
        side.wait_stream(main)
    try:
        with torch.cuda.stream(side):
            for c in calls:
                e.ar_steps(c, st, plan_d, rowstep, tok, margin)
            e.check_errors()
            pos = [e.slot_position(s) for s in slots if s >= 0]
    finally:
        e.set_graphs(True)
    if side is not None:
        main.wait_stream(side)
    return tok.cpu().numpy(), rowstep.cpu().numpy(), pos, plan


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_greedy_slot_beside_a_sampling_slot_decodes_the_nodefer_ids(dtype, eng16, eng32):
    e = eng16 if dtype == "bf16" else eng32
    slots = [0, 1, 2, 3]
    e.set_option("defer_select", 0)
    try:
        ref = _decode(e, slots, [20])
    finally:
        e.set_option("defer_select", 1)
    try:
        e.set_sampling(1, 0.8, 50, 123)
        got = _decode(e, slots, [20])
    finally:
        _greedy_all(e)
    for b in (0, 2, 3):
        np.testing.assert_array_equal(got[0][b], ref[0][b])
    assert (got[0][1] != ref[0][1]).any()  # (slot 1 drew)
    assert got[1].tolist() == [20] * 4 and got[2] == [20] * 4


# ---- 7. every path, step by step ----------------------------------------------------------------------
@pytest.mark.parametrize("dtype,B", [("bf16", 1), ("bf16", 4), ("bf16", 9), ("bf16", 33), ("fp32", 1), ("fp32", 4)])
def test_every_path_samples_from_its_own_logits(dtype, B, eng16, eng32):
    e = eng16 if dtype == "bf16" else eng32
    dev = e.device
    T, k, steps = 0.8, 50, 12
    slots = list(range(B))
    seeds = [0x9e3779b97f4a7c15 * (s + 1) & (2 ** 64 - 1) for s in slots]
    plan = torch.from_numpy(np.random.default_rng(B).integers(3, 384, size=(B, steps)).astype(np.int32)).to(dev)
    st = torch.tensor(slots, dtype=torch.int32, device=dev)
    rowstep = torch.zeros(B, dtype=torch.int32, device=dev)
    tok = torch.full((B, steps), -7, dtype=torch.int32, device=dev)
    tally = SR.Tally()
    try:
        for s in slots:
            e.set_sampling(s, T, k, seeds[s])
            e.reset_slot(s)
        for j in range(steps):
            e.ar_steps(1, st, plan, rowstep, tok)
            logits = e.last_logits(B).cpu().numpy()
            t = tok[:, j].cpu().numpy()
            for b in range(B):
                tally.add(t[b], logits[b], T, k, seeds[b], j, what=f"{dtype} B={B} row {b} step {j}")
        e.check_errors()
        assert rowstep.cpu().tolist() == [steps] * B
        assert [e.slot_position(s) for s in (0, B - 1)] == [steps] * 2
    finally:
        _greedy_all(e)
    print(f"{dtype} B={B}: {tally.ambiguous} / {tally.n} draws with more than one acceptable token")


# ---- 8. graphs, calls and rewinds --------------------------------------------------------------------
@pytest.mark.parametrize("dtype,B", [("bf16", 2), ("fp32", 4)])
def test_graphs_calls_and_rewinds(dtype, B, eng16, eng32):
    e = eng16 if dtype == "bf16" else eng32
    slots = list(range(B))
    calls = [3, 17, 1, 16]
    n = sum(calls)
    _greedy_all(e)
    greedy0 = _decode(e, slots, [32])  # default plan, before any slot samples
    try:
        for s in slots:
            e.set_sampling(s, 0.8, 50, 100 + s)
        graph = _decode(e, slots, calls, graphs=True)
        eager = _decode(e, slots, calls, graphs=False)
        single = _decode(e, slots, [1] * n, graphs=True)
        for other, name in ((eager, "eager"), (single, "one-step calls")):
            np.testing.assert_array_equal(graph[0], other[0], err_msg=name)
            np.testing.assert_array_equal(graph[1], other[1], err_msg=name)
            assert graph[2] == other[2] == [n] * B, name
        assert (graph[0] >= 0).all() and (graph[0] < V).all()

        # a rewind reproduces the draws: 12 steps, back to position 5 with token 4, 7 steps again
        first = _decode(e, slots, [12])
        for s in slots:
            e.set_slot(s, 5, int(first[0][s, 4]))
        again = _decode(e, slots, [7], plan=first[3], rowstep0=5, reset=False)
        np.testing.assert_array_equal(again[0][:, 5:12], first[0][:, 5:12])
        assert again[2] == [12] * B

        # another seed, another stream
        base = _decode(e, slots, [32])
        for s in slots:
            e.set_sampling(s, 0.8, 50, 900 + s)
        other = _decode(e, slots, [32])
        for b in range(B):
            assert (base[0][b] != other[0][b]).any()
    finally:
        _greedy_all(e)
    # every slot greedy again: the default plan, the ids of the run before any slot sampled
    greedy1 = _decode(e, slots, [32])
    np.testing.assert_array_equal(greedy1[0], greedy0[0])
    assert greedy1[2] == greedy0[2] == [32] * B
    assert (greedy1[0] != base[0]).any()


# ---- 9. arguments ---------------------------------------------------------------------------------------
def test_arguments(eng32):
    from llmvox_amd import _lib
    e = eng32
    lib = _lib.load()
    bad = [((-1, 1.0, 0, 0), "slot"), ((e.max_streams, 1.0, 0, 0), "slot"), ((0, -0.5, 0, 0), "temperature"),
           ((0, float("nan"), 0, 0), "temperature"), ((0, float("inf"), 0, 0), "temperature"),
           ((0, 1.0, -1, 0), "top_k")]
    for (slot, T, k, seed), name in bad:
        code = lib.lvx_stream_sampling(e.h, slot, T, k, seed, e.stream_handle())
        assert code == _lib.LVX_E_ARG, (slot, T, k)
        assert name in lib.lvx_last_error().decode(), (name, lib.lvx_last_error())
        with pytest.raises(_lib.LvxArgError):
            e.set_sampling(slot, T, k, seed)
    assert lib.lvx_stream_sampling(e.h, 0, 0.0, 5000, 2 ** 64 - 1, e.stream_handle()) == 0
    assert lib.lvx_version() >= 2
    with pytest.raises(_lib.LvxArgError):
        e.select_probe(5, torch.zeros(1, dtype=torch.int32, device=e.device), torch.zeros(1, V),
                       torch.zeros(1, 2, dtype=torch.int32, device=e.device),
                       torch.zeros(1, dtype=torch.int32, device=e.device),
                       torch.zeros(1, 2, dtype=torch.int32, device=e.device))


# ---- 10. the scheduler on the device ------------------------------------------------------------------
def _schedule(e, overlap, sampling, eoa):
    from llmvox_amd import streaming as S
    words = "The quick brown fox jumps over the lazy dog near the river bank.".split(" ")
    # (max_chunk = the largest dump: every chunk ends at a dump boundary in both schedules, so the stop
    # rule, which is looked at between chunks, stops both at the same token)
    sch = S.FusedScheduler(e, max_chunk=30, overlap=overlap, stop_rule=lambda st, ntok, pos: ntok >= 100)
    sts = []
    for i in range(2):  # (dumps of 10, then 30: two streams stay within the engine's 64 codec frames)
        st = sch.open_stream(index=i, dump_size=10, eoa_id=eoa, sampling=sampling, max_dump=30)
        for w in words:
            st.feed(w)
        sts.append(st)
    assert sch.run_until_idle(max_chunks=200) > 0
    assert sch.run_chunk() == 0 and not sch.inflight
    res = [(list(st.events), list(st.tokens)) for st in sts]
    for st in sts:
        sch.close_stream(st)
    sch.close()
    return res


def test_scheduler_overlap_and_serial_deliver_the_same_sampled_items(eng32):
    from llmvox_amd.sampling import Sampling
    e = eng32
    sp = Sampling(0.8, 50, seed=20240607)
    free = _schedule(e, False, sp, 453)
    eoa = free[0][1][23]  # the token stream 0 draws at step 23 becomes the end-of-audio id
    ser = _schedule(e, False, sp, eoa)
    ovl = _schedule(e, True, sp, eoa)
    twice = _schedule(e, True, sp, eoa)
    assert any(isinstance(x, int) for x in ser[0][0])  # a segment did end
    assert ser[0][1][:ser[0][1].index(eoa)] == free[0][1][:free[0][1].index(eoa)]
    for other in (ovl, twice):
        for (a_ev, a_tok), (b_ev, b_tok) in zip(ser, other):
            assert len(a_ev) > 0 and len(a_ev) == len(b_ev)
            assert a_tok == b_tok
            for x, y in zip(a_ev, b_ev):
                assert type(x) is type(y) and x == y  # PCM bytes included
    assert ser[0][1] != ser[1][1]  # the replicas draw from different seeds
    moved = _schedule(e, False, Sampling(0.8, 50, seed=1), eoa)
    assert moved[0][1] != ser[0][1]
    # the slots were handed back greedy: the default plan and ids
    a = _decode(e, [0, 1], [8])
    assert (a[0] >= 0).all()
