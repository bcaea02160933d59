"""The K / V rows the decode step appends, read back through lvx_kv_read and held to the K / V of an fp64
causal forward over the device's own tokens (oracle.reference_cpu.gpt_forward, train_causal), for the
smallest B of every append site:

  bf16 B = 1            ar_q0_gran_kernel (layer 0), ar_gemv_kernel's epilogue (layers 1-3)
  bf16 B = 3            ar_mfma_ln_kernel through step_store, every layer
  bf16 B = 4            ar_q0_rows_kernel (layer 0), ar_mfma_ln_kernel (layers 1-3)
  bf16 B = 4, l0q 0     ar_mfma_ln_kernel's select prologue form (layer 0)
  bf16 B = 9            ar_q0_rows_kernel (layer 0), ar_mfma2_kernel (layers 1-3)
  bf16 B = 33           ar_bt_kernel
  fp8 KV B = 1, 4       the e4m3 conversion of the same sites
  fp32 B = 1            ar_gemv_kernel, fp32 KV
  fp32 B = 3            the attention's own append (K-split c_attn)
  fp32 B = 3, exp 1024  ar_f32b_kernel

Rows start ragged (prefix phases of 0 / 1 / 62 / 63 steps in smaller batches), then all rows run 132 steps
in one call, so every row crosses positions 63 -> 64 and 127 -> 128 (a new 64-position chunk) inside a
batched call. Every cache row is pre-filled with a sentinel: rows past a slot's final position, and the
slots no row uses, must still hold it.

Tolerance: the device value is q(v'), v' the step's fp32 k / v and q the KV dtype's rounding, so
|q(v') - ref| <= |v' - ref| + half a quantisation step at |v'|. |v' - ref| is allowed 4 x the error E of a
CPU emulation of the bf16 step (every GEMM operand and the attention's K / V rounded as the device rounds
them, fp64 otherwise) against the same fp64 forward; fp32 mode: 1e-5. The tolerance must stay below a
quarter of the smallest distance (max over the 768 columns) between the reference rows of adjacent
positions, so a row written one position off cannot pass; rows of different texts differ as much.
Every device row must also be nearer to its own reference row than to the rows of the positions before
and after it. With fp8 KV the layers 1-3 read e4m3 K / V, which the fp64 forward does not model: E there
is that of the emulation with e4m3 K / V (measured on the CPU: 0.067 against 0.0098, a bound of 0.39
against adjacent rows 1.15 apart), the quarter-distance condition is asserted on layer 0 only, and the
neighbour check rules out the misplaced row.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

N_MAIN, CAP, SENTINEL = 132, 256, 1.5
PREFIX = (0, 1, 62, 63)
MATRICES = ("attn.c_attn.weight", "attn.c_proj.weight", "mlp.c_fc.weight", "mlp.c_proj.weight", "lm_head.weight")
CELLS = [("bf16", "bf16", 1, {}), ("bf16", "bf16", 3, {}), ("bf16", "bf16", 4, {}), ("bf16", "bf16", 4, {"l0q": 0}),
         ("bf16", "bf16", 9, {}), ("bf16", "bf16", 33, {}), ("bf16", "fp8", 1, {}), ("bf16", "fp8", 4, {}),
         ("fp32", "fp32", 1, {}), ("fp32", "fp32", 3, {}), ("fp32", "fp32", 3, {"exp": 1024})]


def _cell_id(c):
    return f"{c[0]}-kv{c[1]}-B{c[2]}" + "".join(f"-{k}={v}" for k, v in c[3].items())


def _bf16(x):
    return x.float().bfloat16().double()


def _fp8(x):
    return x.float().clamp(-448.0, 448.0).to(torch.float8_e4m3fn).double()


@pytest.fixture(scope="module")
def model():
    """Synthetic weights in fp64, as they are and with the matrices rounded to bf16 (the bf16 modes), the
    8 texts, and a cache of the reference K / V per (mode, text, tokens)."""
    from llmvox_amd import weights as LW
    gw, cw, tt = LW.synthetic_all(1234)
    W = {k: torch.from_numpy(np.ascontiguousarray(v)).double() for k, v in gw.items()}
    Wb = {k: _bf16(v) if k.endswith(MATRICES) else v for k, v in W.items()}
    from oracle import reference_cpu as R
    texts = np.random.default_rng(97).integers(3, 384, size=(8, PREFIX[-1] + N_MAIN + 1)).astype(np.int32)
    return dict(weights=(gw, cw, tt), W={"fp32": W, "bf16": Wb}, table=torch.from_numpy(tt).double(),
                codebook=torch.from_numpy(np.ascontiguousarray(cw[R.CODEBOOK_KEY])).double(), texts=texts, ref={}, emu={})


def _embed(m, text, toks):
    """The step inputs [1][T][768] that the tokens induce (position 0: no previous token)."""
    from oracle import reference_cpu as R
    T = len(toks)
    te = m["table"][torch.as_tensor(text[:T].astype(np.int64))]
    se = torch.zeros(T, 512, dtype=torch.float64)
    se[1:] = m["codebook"][torch.as_tensor(np.asarray(toks[:-1], dtype=np.int64))]
    return R.build_input(te.unsqueeze(0), se.unsqueeze(0))


def _reference(m, wd, ti, toks):
    """K / V [4][T][768] of the fp64 causal forward over the row's own tokens."""
    from oracle import reference_cpu as R
    key = (wd, ti, tuple(toks))
    if key not in m["ref"]:
        _, cache = R.gpt_forward(m["W"][wd], _embed(m, m["texts"][ti], toks), None, train_causal=True)
        m["ref"][key] = (torch.stack([c[0][0] for c in cache]).numpy(), torch.stack([c[1][0] for c in cache]).numpy())
    return m["ref"][key]


def _emulated(W, emb, rnd, kvq):
    """The same forward with every GEMM operand passed through `rnd` and the attention's K / V through
    `kvq` (the values the cache holds); returns the unquantised K / V [4][T][768] the step would append."""
    from oracle import reference_cpu as R
    T = emb.shape[1]
    x = emb + W["transformer.wpe.weight"][:T].unsqueeze(0)
    ks, vs = [], []
    for i in range(R.N_LAYER):
        p = f"transformer.h.{i}."
        h = F.layer_norm(x, (768,), W[p + "ln_1.weight"], None, 1e-5)
        q, k, v = F.linear(rnd(h), W[p + "attn.c_attn.weight"]).split(768, dim=2)
        ks.append(k[0])
        vs.append(v[0])
        qh, kh, vh = (t.view(1, T, 8, 96).transpose(1, 2) for t in (q, kvq(k), kvq(v)))
        y = F.scaled_dot_product_attention(qh, kh, vh, is_causal=True).transpose(1, 2).reshape(1, T, 768)
        x = x + F.linear(rnd(y), W[p + "attn.c_proj.weight"])
        h2 = F.layer_norm(x, (768,), W[p + "ln_2.weight"], None, 1e-5)
        x = x + F.linear(rnd(R.new_gelu(F.linear(rnd(h2), W[p + "mlp.c_fc.weight"]))), W[p + "mlp.c_proj.weight"])
    return torch.stack(ks).numpy(), torch.stack(vs).numpy()


def _emulation_error(m, kvd, ti, toks):
    """E: max |emulated - fp64| over the K / V of every layer, for one row of the bf16 mode."""
    key = (kvd, ti, tuple(toks))
    if key not in m["emu"]:
        ident = lambda t: t  # noqa: E731
        emb = _embed(m, m["texts"][ti], toks)
        rk, rv = _reference(m, "bf16", ti, toks)
        ik, iv = _emulated(m["W"]["bf16"], emb, ident, ident)  # the emulation's own code, nothing rounded
        assert max(np.abs(ik - rk).max(), np.abs(iv - rv).max()) < 1e-9
        ek, ev = _emulated(m["W"]["bf16"], emb, _bf16, _fp8 if kvd == "fp8" else _bf16)
        m["emu"][key] = float(max(np.abs(ek - rk).max(), np.abs(ev - rv).max()))
    return m["emu"][key]


def _half_step(mag, kvd):
    """Half a quantisation step of the KV dtype for values of magnitude `mag` (fp32: none)."""
    if kvd == "fp32":
        return np.zeros_like(mag)
    e = np.floor(np.log2(np.maximum(mag, 1e-30)))
    return 0.5 * np.exp2(np.maximum(e, -126.0) - 7.0) if kvd == "bf16" else 0.5 * np.exp2(np.maximum(e, -6.0) - 3.0)


@pytest.mark.parametrize("cell", CELLS, ids=_cell_id)
def test_appended_rows_match_fp64_forward(model, cell):
    from llmvox_amd.engine import build_engine
    wd, kvd, B, opts = cell
    m = model
    S = B + 2  # two slots no row uses
    n = PREFIX[-1] + N_MAIN
    e = build_engine(0, wd, kvd, max_streams=S, max_positions=CAP, max_codec_frames=16, weights=m["weights"])
    dev = e.device
    try:
        for k, v in opts.items():
            e.set_option(k, v)
        sent = torch.full((CAP, 768), SENTINEL, dtype=torch.float32, device=dev)
        for s in range(S):
            e.reset_slot(s)
            for layer in range(4):
                e.kv_write(s, layer, 0, sent, sent)
        slots = [int(s) for s in np.random.default_rng(B).permutation(S)[:B]]
        pre = [PREFIX[b % 4] for b in range(B)]
        ti = [b % 8 for b in range(B)]
        toks = np.full((B, n), -1, dtype=np.int64)

        def run(rows, steps, start):
            plan = torch.from_numpy(m["texts"][[ti[b] for b in rows]].copy()).to(dev)
            st = torch.tensor([slots[b] for b in rows], dtype=torch.int32, device=dev)
            rowstep = torch.tensor(start, dtype=torch.int32, device=dev)
            tok = torch.full((len(rows), plan.shape[1]), -1, dtype=torch.int32, device=dev)
            e.ar_steps(steps, st, plan, rowstep, tok)
            t = tok.cpu().numpy()
            for j, b in enumerate(rows):
                toks[b, start[j]:start[j] + steps] = t[j, start[j]:start[j] + steps]

        for p in PREFIX[1:]:  # the ragged starts: each prefix length as a batch of its own
            rows = [b for b in range(B) if pre[b] == p]
            if rows:
                run(rows, p, [0] * len(rows))
        run(list(range(B)), N_MAIN, pre)
        e.check_errors()

        worst = dict(err=0.0, ratio=0.0, tol=0.0, dist=np.inf, E=0.0)
        for b in range(B):
            T = pre[b] + N_MAIN
            assert e.slot_position(slots[b]) == T
            tk = toks[b, :T]
            assert (tk >= 0).all() and (toks[b, T:] == -1).all()
            rk, rv = _reference(m, wd, ti[b], tk)
            Eb = 1e-5 / 4 if wd == "fp32" else _emulation_error(m, "bf16", ti[b], tk)
            E8 = _emulation_error(m, "fp8", ti[b], tk) if kvd == "fp8" else Eb
            for layer in range(4):
                # fp8 KV, layers 1-3: the step legitimately reads e4m3 K / V, which the fp64 forward does not
                # model; their E is that of the emulation with e4m3 K / V, too wide for the quarter-distance
                # condition, so there the neighbour check below is what rules out a misplaced row
                strict = kvd != "fp8" or layer == 0
                E = Eb if strict else E8
                worst["E"] = max(worst["E"], E)
                dk, dv = (t.cpu().numpy() for t in e.kv_read(slots[b], layer, 0, CAP))
                for got, ref in ((dk, rk[layer]), (dv, rv[layer])):
                    assert np.all(got[T:] == SENTINEL), (b, layer)  # nothing written past the final position
                    tol = 4 * E + _half_step(np.abs(ref) + 4 * E, kvd)
                    d = np.abs(got[:T] - ref)
                    worst["err"] = max(worst["err"], float(d.max()))
                    worst["ratio"] = max(worst["ratio"], float((d / tol).max()))
                    if strict:
                        worst["tol"] = max(worst["tol"], float(tol.max()))
                        worst["dist"] = min(worst["dist"], float(np.abs(ref[1:] - ref[:-1]).max(axis=1).min()))
                    # every device row is nearer to its own reference row than to the rows before and after
                    own = d.max(axis=1)
                    assert (own[1:] < np.abs(got[1:T] - ref[:-1]).max(axis=1)).all(), (b, layer)
                    assert (own[:-1] < np.abs(got[:T - 1] - ref[1:]).max(axis=1)).all(), (b, layer)
        for s in set(range(S)) - set(slots):
            for layer in range(4):
                assert all(bool((t == SENTINEL).all()) for t in e.kv_read(s, layer, 0, CAP)), (s, layer)
    finally:
        e.close()
    print(f"\n[kv_append {_cell_id(cell)}] max |device - fp64| {worst['err']:.3e} = {worst['ratio']:.3f} of the bound "
          f"(largest bound {worst['tol']:.3e}; emulation error E {worst['E']:.3e}); adjacent reference rows differ by "
          f">= {worst['dist']:.3f}")
    assert worst["tol"] < 0.25 * worst["dist"]
    assert worst["ratio"] <= 1.0
