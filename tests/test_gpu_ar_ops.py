"""Every GEMM op of the decode step per plan cell (the five kernel families behind launch_op: embedding and
LayerNorm prologues, the LayerNorm after the GEMM, the split merges in c_proj's prologue, the pending mlp c_proj
copies and their fold, lm_head) against the fp64 model of tests/ar_ref.py, through the test hook lvx_ar_ops.

A cell is (weight dtype, KV dtype, B, options); its windows of ops (ar_ref.windows) run on rows in permuted slots at
ragged positions from {0, 1, 63, 64, 65, 127, 128, 129} over histories written with lvx_kv_write, on residual
rows with per-row gain and offset, spiked channels in the rows around every 16-row tile edge and one row with a
large mean. Compared per row: RMS(device - fp64) / RMS(fp64) of what the window's last op left (c_proj and mlp
c_proj: of out - x_in), so one wrong row among 64 fails on its own; the bound is 8 x the deviation of the same
op evaluated in float32 (ar_ref.YARDSTICK, per op kind and mode). Each window is compared as its last op alone,
from the buffers the window before it left on the device; a buffer that holds bf16 / fp8 values is held by the
smallest error consistent with what it stores (ar_ref.dev_err), so tie flips are no part of any figure. Every cell asserts the plan lvx_ar_ops reports against the
table in ar_ref.cells(), so a moved threshold fails the cell it would have moved.
"""
import numpy as np
import pytest
import torch

from tests import ar_ref as R
from tests import attn_ref as A

pytestmark = pytest.mark.gpu

CELLS = R.cells()
MEASURED = {}  # (kind, class) -> largest device row error of the module


@pytest.fixture(scope="module")
def W():
    from llmvox_amd import weights as LW
    gw, cw, tt = LW.synthetic_all(1234)
    w = (gw, tt, cw[R.CODEBOOK_KEY])
    R.ensure_yardsticks(w)
    return w


class Eng:
    """One engine with every (slot, layer)'s history written through lvx_kv_write and read back."""

    def __init__(self, eng):
        from llmvox_amd.engine import build_engine
        wd, self.kv = R.ENGINES[eng]
        self.S = R.MAX_STREAMS[eng]
        self.e = e = build_engine(0, wd, self.kv, max_streams=self.S, max_positions=R.MAX_POSITIONS, max_codec_frames=16)
        for s in range(self.S):
            for l in range(R.NL):
                k, v = R.history(s, l)
                e.kv_write(s, l, 0, torch.from_numpy(k).to(e.device), torch.from_numpy(v).to(e.device))
                kd, vd = e.kv_read(s, l, 0, R.HIST_ROWS)
                Ks, Vs = R.stored_history(self.kv, s, l)
                assert torch.equal(kd.cpu(), Ks) and torch.equal(vd.cpu(), Vs), (eng, s, l)
        e.check_errors()

    def restore_row(self, slot, layer):
        """The history row at the slot's position back in place (a window's c_attn overwrote it)."""
        p = R.slot_pos(slot)
        k, v = R.history(slot, layer)
        self.e.kv_write(slot, layer, p, torch.from_numpy(k[p:p + 1]).to(self.e.device), torch.from_numpy(v[p:p + 1]).to(self.e.device))


@pytest.fixture(scope="module")
def engines():
    cur = {}

    def get(eng):
        if eng not in cur:
            cur[eng] = Eng(eng)
        return cur[eng]

    yield get
    for h in cur.values():
        h.e.close()


def _set_opts(e, opts):
    for k, v in {**R.DEFAULT_OPTS, **opts}.items():
        e.set_option(k, v)


def _place(H, case):
    for s in case.slots:
        if s >= 0:
            H.e.set_slot(s, R.slot_pos(s), R.slot_prev(s))


def _run(H, case, win, x, q, poison=False):
    """One window on the device. The fp32 K-split cells enter an attention under option exp 1024 (the one-launch
    c_attn: their own attention takes no q rows), which changes qsplit alone."""
    e, cell = H.e, case.cell
    first, last, entry = win
    info = cell.info
    if entry == "q":
        for s in case.slots:
            if s >= 0:
                H.restore_row(s, first // 5)
        if info[7]:
            e.set_option("exp", cell.opts.get("exp", 0) | 1024)
            info = info[:7] + (0,) + info[8:]
    try:
        slots = torch.tensor(case.slots, dtype=torch.int32, device=e.device)
        tid = torch.tensor(case.rows[0], dtype=torch.int32) if first == 0 else None
        out = e.ar_ops(slots, first, last, None if x is None else torch.from_numpy(x),
                       None if q is None else torch.from_numpy(q), tid, poison)
    finally:
        if entry == "q" and cell.info[7]:
            e.set_option("exp", cell.opts.get("exp", 0))
    assert out["plan"] == info, (R.cell_id(cell), win, out["plan"], info)
    return out


def _device_rows(H, case, win, out):
    """name -> float64 [B][..] of what the window's last op left in its buffers, under ar_ref.as_stored's names: q, k, v
    (the cache rows at the rows' positions, or the K-split partials summed here in fp64), y (the rows, or the
    partials merged in fp64), x (with the pending copies folded in fp64), h, logits."""
    from llmvox_amd import _lib
    e, cell = H.e, case.cell
    form, o = out["form"], out["out"].cpu().numpy().astype(np.float64)
    if form == _lib.AR_OUT_QKV_PARTS:  # (the attention sums them on the device, in fp32, and appends k / v)
        s = o.sum(axis=0)
        return dict(q=s[:, :R.D], k=s[:, R.D:2 * R.D], v=s[:, 2 * R.D:])
    if form == _lib.AR_OUT_Q:
        k, v = _cache_rows(H, case, win[1] // 5)
        return dict(q=o, k=k.numpy().astype(np.float64), v=v.numpy().astype(np.float64))
    if form == _lib.AR_OUT_ATTN_ROWS:
        return dict(y=o)
    if form == _lib.AR_OUT_ATTN_PARTS:
        po, pml = out["part_o"].cpu().numpy(), out["part_ml"].cpu().numpy()
        return dict(y=np.stack([A.merge_fp64(po[b], pml[b], len(A.split_ranges(p + 1, cell.info[2], case.kv))) if p >= 0
                                else np.zeros(R.D) for b, p in enumerate(case.pos)]))
    if form == _lib.AR_OUT_X:
        cp = out["copies"].cpu().numpy()
        if cp.dtype == np.int64:  # the fused MLP's fixed point: summed exactly, then x 2^-32 (exact in float64)
            fold = cp.sum(axis=1).astype(np.float64) * 2.0 ** -32
        else:
            fold = cp.astype(np.float64).sum(axis=1)
        return dict(x=o + fold)
    return dict(h=o) if form == _lib.AR_OUT_H else dict(logits=o, logits_tail=o[:, R.VOCAB - 16:])


def _cache_rows(H, case, l):
    """(k, v) float32 [B][768]: layer l's cache rows at the rows' positions, read back (an idle row: zeros)."""
    kv = [H.e.kv_read(s, l, R.slot_pos(s), 1) if s >= 0 else None for s in case.slots]
    z = torch.zeros(R.D)
    return (torch.stack([z if r is None else r[0][0].cpu() for r in kv]), torch.stack([z if r is None else r[1][0].cpu() for r in kv]))


@pytest.mark.parametrize("cell", CELLS, ids=R.cell_id)
def test_windows_match_fp64(engines, W, cell):
    """Every window's LAST op against the float64 model of that op, from the buffers the window without it left on
    the device (ar_ref.provider_of): per row, ar_ref.dev_err <= 8 x the op's float32 yardstick in the cell's mode."""
    H = engines(cell.eng)
    e = H.e
    _set_opts(e, cell.opts)
    case = R.Case(cell)
    m64 = R.model_for(W, cell.mode, torch.float64, R.cell_ksplit(cell))
    worst, fails, states = {}, [], {}
    try:
        _place(H, case)
        for win in R.windows(cell):
            x, q = case.inputs(win)
            out = _run(H, case, win, x, q, poison=win[0] == 0)
            dev = _device_rows(H, case, win, out)
            prov = R.provider_of(cell, win)
            state = case.entry_state(m64, win, x, q) if prov is None else states[prov]
            l = R.Case.appended_layer(win)  # the attention read the row this window's c_attn appended: read it back
            kv_rows = None if l is None else {l: _cache_rows(H, case, l)}
            ref = R.resolved_reference(case, m64, win, state, kv_rows, dev)
            for name, err in R.window_errors(case, m64, win, dev, ref).items():
                kind = R.kind_of(win, name)
                bnd = R.bound(kind, cell.mode)
                assert np.isfinite(err).all(), (win, name)
                err = float(err.max())
                worst[kind] = max(worst.get(kind, 0.0), err)
                print(f"[ar_ops {R.cell_id(cell)}] window {win[0]}..{win[1]} {name}: {err:.3e} = {err / bnd:.3f} of the bound {bnd:.3e}")
                if err > bnd:
                    fails.append((win, name, err, bnd))
                if name != "logits_tail":  # (a misplaced row shows in the whole row of logits)
                    assert R.adjacent_row_distance(R.compared(ref, win)[name].numpy()) >= R.MIN_ROW_DISTANCE * bnd, (win, name)
            states[win] = R.Case.next_state(state, win, dev)
            if win[0] == 0 and win[1] in (0, 4, 9):  # layer 0 ignores what the pending copies hold: bit for bit
                clean = _run(H, case, win, x, q, poison=False)
                assert torch.equal(clean["out"], out["out"]) and torch.equal(clean["copies"], out["copies"]), win
        e.check_errors()  # the AR error word is 0
    finally:
        _set_opts(e, {})
    for kind, v in worst.items():
        MEASURED[kind, cell.mode] = max(MEASURED.get((kind, cell.mode), 0.0), v)
    assert not fails, fails


@pytest.mark.parametrize("cell", [c for c in CELLS if c.full], ids=R.cell_id)
def test_full_window_is_the_step(engines, cell):
    """Ops 0 .. 20 through the hook leave the logits of one real lvx_ar_steps step (option defer_select 0) from
    the same state, bit for bit: the hook launches what the step launches."""
    H = engines(cell.eng)
    e = H.e
    _set_opts(e, {**cell.opts, "defer_select": 0})
    case = R.Case(cell)
    B = cell.B
    try:
        _place(H, case)
        out = _run(H, case, (0, R.LM_HEAD, "x"), None, None)
        _place(H, case)
        slots = torch.tensor(case.slots, dtype=torch.int32, device=e.device)
        tp = torch.full((B, 2), 384, dtype=torch.int32)
        tp[:, 0] = torch.tensor(case.rows[0], dtype=torch.int32)
        rowstep = torch.zeros(B, dtype=torch.int32, device=e.device)
        tok = torch.zeros(B, 2, dtype=torch.int32, device=e.device)
        e.ar_steps(1, slots, tp.to(e.device), rowstep, tok)
        step = e.last_logits(B)
        e.check_errors()
        assert rowstep.cpu().tolist() == [1] * B
        assert torch.equal(step, out["out"]), float((step - out["out"]).abs().max())
        assert tok[:, 0].cpu().tolist() == out["out"].argmax(dim=-1).cpu().tolist()
    finally:
        _place(H, case)
        _set_opts(e, {})


IDLE_CELLS = [c for c in CELLS if c.B in (8, 32) and c.full]


@pytest.mark.parametrize("cell", IDLE_CELLS, ids=R.cell_id)
def test_idle_row_in_the_middle(engines, cell):
    """One slot -1 in the middle of the call. The live rows equal the call without it bit for bit, whatever the idle
    row's inputs hold; the cache row of the slot that left the call is not written; the attention leaves the idle
    row's own output as it was (zeros where the plan's merge kernel or ATTN_F32_ROWS defines it, its partials
    unwritten); and c_proj leaves the idle row's x as it entered, bit for bit, wherever the row's attention output
    is defined (every plan but the one-split attention that writes the bf16 operand row itself: there the idle
    row of xn keeps what an earlier call left, and c_proj, which multiplies all B rows, adds its product)."""
    from llmvox_amd import _lib
    H = engines(cell.eng)
    e = H.e
    _set_opts(e, cell.opts)
    full, part = R.Case(cell), R.Case(cell, idle=cell.B // 2)
    idle = cell.B // 2
    gone = full.slots[idle]
    live = [b for b in range(cell.B) if b != idle]
    path, nsplit, direct = cell.info[0], cell.info[2], cell.info[3]
    merged = path == R.BT or (path in (R.MLN, R.MROWS) and nsplit > 1)
    defined = merged or direct in (A.ATTN_PARTIALS, A.ATTN_F32_ROWS)
    try:
        _place(H, full)
        for win in [(0, 2, "x"), (5, 5, "x"), (5, 9, "x"), (11, 11, "q"), (11, 12, "q"), (15, 20, "x")]:
            x, q = full.inputs(win)
            a = _run(H, full, win, x, q)
            before = [e.kv_read(gone, l, R.slot_pos(gone), 1) for l in range(R.NL)]
            outs = []
            for fill in (0.0, 3.0):  # the idle row's own inputs must not matter to anyone else
                xi, qi = (None if x is None else x.copy()), (None if q is None else q.copy())
                if qi is not None:
                    qi[idle] = fill
                if xi is not None and fill:
                    xi[idle] = fill
                outs.append((_run(H, part, win, xi, qi), xi))
            after = [e.kv_read(gone, l, R.slot_pos(gone), 1) for l in range(R.NL)]
            for (k0, v0), (k1, v1) in zip(before, after):
                assert torch.equal(k0, k1) and torch.equal(v0, v1), win
            for b, xi in outs:
                for name in ("out", "copies", "part_o", "part_ml"):
                    ta, tb = a[name], b[name]
                    if name == "out" and a["form"] == _lib.AR_OUT_QKV_PARTS:  # [4][B][2304]
                        ta, tb = ta.transpose(0, 1), tb.transpose(0, 1)
                    assert torch.equal(ta[live], tb[live]), (win, name)
                assert torch.isfinite(b["out"]).all(), win
                if win == (11, 11, "q"):  # the attention's own row of the idle slot
                    if b["form"] == _lib.AR_OUT_ATTN_PARTS:
                        assert torch.equal(b["part_o"][idle], a["part_o"][idle]) and torch.equal(b["part_ml"][idle], a["part_ml"][idle])
                    elif merged or direct == A.ATTN_F32_ROWS:
                        assert not b["out"][idle].any()
                    else:
                        assert torch.equal(b["out"][idle], a["out"][idle])
                if win == (11, 12, "q") and defined:  # x + W . 0
                    assert torch.equal(b["out"][idle].cpu(), torch.from_numpy(xi[idle])), win
        e.check_errors()
    finally:
        _set_opts(e, {})


def test_hook_rejects_what_the_plan_cannot_run(engines):
    """A window cannot start at the fp32 K-split attention (it takes no q rows) nor end at c_fc inside the fused MLP."""
    from llmvox_amd import _lib
    H = engines("fp32")
    st = torch.arange(4, dtype=torch.int32, device=H.e.device)
    z = torch.zeros(4, R.D)
    with pytest.raises(_lib.LvxError) as ei:
        H.e.ar_ops(st, 6, 7, z, z)
    assert ei.value.code == _lib.LVX_E_STATE
    H = engines("bf16")
    with pytest.raises(_lib.LvxError) as ei:
        H.e.ar_ops(st[:1], 5, 8, z[:1])
    assert ei.value.code == _lib.LVX_E_STATE
    for first, last in ((2, 4), (7, 6), (0, 21), (3, 3)):
        with pytest.raises(_lib.LvxError) as ei:
            H.e.ar_ops(st, first, last, z, z, torch.zeros(4, dtype=torch.int32))
        assert ei.value.code == _lib.LVX_E_ARG
    H.e.check_errors()


def test_zz_measured_maxima():
    """The figures of this run for the table in DESIGN.md section 2."""
    for key in sorted(MEASURED):
        y = R.YARDSTICK[key]
        print(f"[ar_ops] {key}: yardstick {y:.3e}, bound {R.MARGIN * y:.3e}, largest device error {MEASURED[key]:.3e}")
    for key, v in MEASURED.items():
        assert v <= R.MARGIN * R.YARDSTICK[key], (key, v)
