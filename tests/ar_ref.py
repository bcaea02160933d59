"""fp64 reference of the ops of one AR decode step, one function per op of ``lvx_ar_ops``, with the rounding
points of each device path, plus the cells, windows and inputs of tests/test_gpu_ar_ops.py (tests/test_ar_ref.py
checks the model, the yardsticks and the sensitivity of the inputs without a GPU).

TEST INFRASTRUCTURE ONLY. The formulas are those ``oracle/reference_cpu.py`` cites (src/model.py, the decode
loop of streaming_server.py); in mode "f32" with ``dt`` float64 they are that reference in double precision.
The other modes insert the roundings of the device paths, each read from ``llmvox_amd/csrc/ar_kernels.hip``
(kernel / statement cited beside it):

  mode     path of ar_plan.h                 roundings
  f32      fp32 weights (GEMV or f32b)       none
  gemv     bf16 GEMV family                  weights
  fused    bf16 GEMV, B <= 2, fused MLP      weights; the MLP's per-block partials to 2^-32 fixed point
  ln       ar_mfma_ln_kernel                 weights; the LayerNorm'd operand rows, gelu(c_fc), attention rows: bf16
  rows     ar_rows_kernel + ar_mfma2_kernel  as ln, with c_fc's LayerNorm applied after the GEMM from the row
                                             statistics and fc_gsum over the operand bf16(x * ln_2.weight)
  bt       ar_bt_kernel                      as ln
  (every mode over a bf16 KV cache: the attention's scaled q as a bf16 hi + lo pair, ar_attn_v2_kernel qsplit_make)

Everything else (accumulation, statistics, softmax, gelu, the residual stream, the pending copies) is unrounded.
Every function takes the model's ``dt`` (torch.float64: the reference; torch.float32: the same model in single
precision, the yardstick of the device bounds) and the model's ``mut``, a set of named mutations (the indexing
and omission errors tests/test_ar_ref.py proves the comparison sensitive to).
"""
from __future__ import annotations

import math
from collections import namedtuple

import numpy as np
import torch

from tests import attn_ref as A

D, DFF, NH, HD, VOCAB, NL = 768, 3072, 8, 96, 4096, 4
OP_QKV, OP_ATTN, OP_CPROJ, OP_FC, OP_MPROJ, LM_HEAD = 0, 1, 2, 3, 4, 20
NONE = frozenset()
MODES = ("f32", "gemv", "fused", "ln", "rows", "bt")
BF16_OPERANDS = ("ln", "rows", "bt")
CODEBOOK_KEY = "feature_extractor.encodec.quantizer.vq.layers.0._codebook.embed"


AMB_REL = 2.0 ** -18  # an fp32 LayerNorm row is within a few 2^-24 of fp64: 2^-18 covers it 16-fold


def bf16_round(x: torch.Tensor) -> torch.Tensor:
    """RNE to bf16 of the fp32 value of x (the device rounds an fp32 register), back in x's dtype."""
    return x.to(torch.float32).to(torch.bfloat16).to(x.dtype)


def kv_round(x: torch.Tensor, kv: str) -> torch.Tensor:
    """store_kv: the fp32 k / v element as the cache dtype stores it (fp32 copy, bf16 RNE, saturated e4m3fn)."""
    f = x.to(torch.float32)
    if kv == "bf16":
        f = f.to(torch.bfloat16).float()
    elif kv == "fp8":
        f = f.clamp(-448.0, 448.0).to(torch.float8_e4m3fn).float()
    return f.to(x.dtype)


def copies_of(mode, ksplit=True):
    """Pending mlp c_proj copies of a path (each a K slice of DFF / count columns; fused: block k of 16 columns adds
    into copy k % 4, ar_mlp_fused_kernel ``a.yfx + (blockIdx.x % YCOPIES) * D``). ksplit: fp32 with the K split."""
    return {"fused": 4, "ln": 2, "rows": 4, "f32": 4 if ksplit else 0}.get(mode, 0)


class Model:
    """The AR weights in ``dt``, the GEMM matrices rounded to bf16 in every mode but f32 (lvx_api.cpp upload:
    ``f32_to_bf16``, RNE; vectors and the gathered tables stay fp32)."""

    def __init__(self, gw, text_table, codebook, mode, dt=torch.float64, mut=NONE, ksplit=True):
        assert mode in MODES
        self.mode, self.dt, self.mut, self.ksplit = mode, dt, frozenset(mut), ksplit
        self.amb, self.force = None, {}  # Model.operand

        def t(a):
            return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float32)))

        def mat(a):
            w = t(a)
            return (w if mode == "f32" else w.to(torch.bfloat16).float()).to(dt)

        self.L = []
        for i in range(NL):
            p = f"transformer.h.{i}."
            lw = dict(ln1=t(gw[p + "ln_1.weight"]).to(dt), ln2=t(gw[p + "ln_2.weight"]).to(dt),
                      attn=mat(gw[p + "attn.c_attn.weight"]), aproj=mat(gw[p + "attn.c_proj.weight"]),
                      fc=mat(gw[p + "mlp.c_fc.weight"]), mproj=mat(gw[p + "mlp.c_proj.weight"]))
            # lvx_api.cpp: ``acc += (double)g2[k] * (double)wv`` over the bf16 weights, ``gs[n] = (float)acc``
            lw["gsum"] = (lw["fc"].double() @ lw["ln2"].double()).float().to(dt)
            self.L.append(lw)
        self.lnf = t(gw["transformer.ln_f.weight"]).to(dt)
        self.lm = mat(gw["lm_head.weight"])
        self.wpe = t(gw["transformer.wpe.weight"])
        self.text_table, self.codebook = t(text_table), t(codebook)

    def layer(self, l):
        return self.L[l + 1 if "next_layer_weight" in self.mut and l + 1 < NL else l]

    # ---- pieces --------------------------------------------------------------------------------------
    def ln_stats(self, x):
        """wave_ln_regs / wave_ln_to_lds: mean, then the biased variance of the centred row, eps 1e-5."""
        mean = x.mean(dim=-1, keepdim=True)
        c = x - mean
        n = D - 1 if "unbiased_var" in self.mut else D
        rstd = 1.0 / torch.sqrt((c * c).sum(dim=-1, keepdim=True) / n + 1e-5)
        if "ln_prev_row" in self.mut and x.shape[0] > 1:  # row b normalised with row b - 1's statistics
            mean, rstd = torch.roll(mean, 1, 0), torch.roll(rstd, 1, 0)
        return mean, rstd

    def operand(self, t):
        """A GEMM's operand row as the MFMA paths store it: bf16, RNE (``pack4_bf16``; ``f32_to_bf16(xn * gpre[k])``).
        The device rounds its own fp32 value, which differs from this one in its last bits, so an element within
        AMB_REL of a rounding boundary may legitimately land on either side: with ``amb`` a list, those elements
        are recorded as (row, column, lower value, upper value), and ``force`` {(row, column): value} overrides
        the rounding (resolved_reference tries both sides and keeps the nearer to what the device left)."""
        if self.mode not in BF16_OPERANDS:
            return t
        r = bf16_round(t)
        if self.amb is not None:
            e = AMB_REL * t.abs()
            lo, hi = bf16_round(t - e), bf16_round(t + e)
            for b, k in (lo != hi).nonzero().tolist():
                self.amb.append((b, k, lo[b, k].item(), hi[b, k].item()))
        if self.force:
            r = r.clone()
            for (b, k), val in self.force.items():
                r[b, k] = val
        return r

    def ln_rows(self, x, g):
        """The LayerNorm'd operand rows of a K = 768 GEMM. bf16 operand paths: ar_rows_kernel / ar_mfma_ln_kernel /
        ar_bt_kernel ``pack4_bf16(v[j])``; the GEMV family and fp32 keep them fp32 (``wave_ln_to_lds`` into xs)."""
        mean, rstd = self.ln_stats(x)
        return self.operand((x - mean) * rstd * g)

    def gelu(self, v):
        if "erf_gelu" in self.mut:
            return 0.5 * v * (1.0 + torch.erf(v / math.sqrt(2.0)))
        return 0.5 * v * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (v + 0.044715 * v * v * v)))

    def _rows_out(self, y):
        if "row16_is_15" in self.mut and y.shape[0] > 16:
            y = y.clone()
            y[16] = y[15]
        return y

    # ---- ops -----------------------------------------------------------------------------------------
    def embed(self, text_ids, prev, pos):
        """embed_row: cat(text_table[t], codebook[c] | 0 at position 0) / max(|.|, 1e-8) + wpe[p]."""
        rows = []
        for tid, c, p in zip(text_ids, prev, pos):
            if p < 0:  # idle row (slot -1): zeros
                rows.append(torch.zeros(D, dtype=self.dt))
                continue
            code = self.codebook[c] if (p > 0 or "code_at_p0" in self.mut) else torch.zeros(512)
            v = torch.cat([self.text_table[tid], code]).to(self.dt)
            den = torch.clamp(torch.sqrt((v * v).sum()), min=1e-8)
            if "no_den" in self.mut:
                den = 1.0
            rows.append(v / den + self.wpe[p + 1 if "wpe_next" in self.mut else p].to(self.dt))
        return torch.stack(rows)

    def c_attn(self, l, x):
        """q, k, v [B][768] of LN1(x) (x: the final residual, pending copies folded)."""
        w = self.layer(l)
        xn = self.ln_rows(x, w["ln1"])
        if "k_tail32" in self.mut:
            xn = xn.clone(); xn[:, D - 32:] = 0
        if "k_slice192" in self.mut:
            xn = xn.clone(); xn[:, 192:384] = 0
        qkv = self._rows_out(xn @ w["attn"].T)
        q, k, v = qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:]
        if "q767_zero" in self.mut:
            q = q.clone(); q[:, D - 1] = 0
        if "kv_swap" in self.mut:
            k, v = v, k
        return q, k, v

    def attention(self, q, K, V, ts, ns_max=1, kv="fp32"):
        """softmax(K q / sqrt(96)) V per (row, head) over the stored K / V rows [0, t) of each row (lists of
        [>= t][768] tensors). The bf16 operand paths store the row as bf16 (ar_attn_v2_kernel ``st.xn[...] =
        f32_to_bf16(ov * (1.0f / lv))``, ar_merge_bf16_kernel ``f32_to_bf16(y)``). The two merge mutations
        evaluate the rows through the split partials of A.split_ranges."""
        out = []
        for b, t in enumerate(ts):
            if t <= 0:
                out.append(torch.zeros(D, dtype=self.dt))
                continue
            Kh = K[b][:t].to(self.dt).view(t, NH, HD)
            Vh = V[b][:t].to(self.dt).view(t, NH, HD)
            qs = q[b].view(NH, HD) * A.SCALE
            if kv == "bf16":  # ar_attn_v2_kernel, bf16 KV: qsplit_make, the scaled q as bf16 hi + lo pairs for v_dot2
                f = qs.to(torch.float32)
                hi = f.to(torch.bfloat16).float()
                qs = (hi + (f - hi).to(torch.bfloat16).float()).to(self.dt)
            s = torch.einsum("hd,thd->ht", qs, Kh)
            if self.mut & {"empty_split_exp0", "merge_max_skip_one"}:
                out.append(self._merge_mut(s, Vh, t, ns_max, kv))
                continue
            w = torch.softmax(s, dim=-1)
            out.append(torch.einsum("ht,thd->hd", w, Vh).reshape(D))
        return self._rows_out(torch.stack(out))  # before the row is stored: Model.store

    def _merge_mut(self, s, Vh, t, ns_max, kv):
        rng = A.split_ranges(t, ns_max, kv)
        m = torch.stack([s[:, a:b].max(dim=1).values if a < b else torch.full((NH,), -math.inf, dtype=self.dt) for a, b in rng], 1)
        live = [i for i, (a, b) in enumerate(rng) if a < b]
        use = live[:-1] if ("merge_max_skip_one" in self.mut and len(live) > 1) else live
        M = m[:, use].max(dim=1, keepdim=True).values
        num, den = torch.zeros(NH, HD, dtype=self.dt), torch.zeros(NH, 1, dtype=self.dt)
        for i, (a, b) in enumerate(rng):
            if a < b:
                e = torch.exp(s[:, a:b] - m[:, i:i + 1])
                f = torch.exp(m[:, i:i + 1] - M)
                num += f * torch.einsum("ht,thd->hd", e, Vh[a:b])
                den += f * e.sum(dim=1, keepdim=True)
            elif "empty_split_exp0" in self.mut:  # an empty trailing split counted with weight exp(0), l = 1
                den += 1.0
        return (num / den).reshape(D)

    def c_proj(self, l, x, y):
        w = self.layer(l)
        o = self._rows_out(y @ w["aproj"].T)
        return o if "no_residual" in self.mut else x + o

    def c_fc(self, l, x):
        """gelu(c_fc(LN2(x))): fp32 h in the GEMV family and fp32 (``a.st.h[...] = gelu_tanh(v)``), bf16 hb on the
        bf16 operand paths (``a.st.hb[...] = f32_to_bf16(gelu_tanh(v))``)."""
        w = self.layer(l)
        g2 = w["ln1"] if "ln1_for_ln2" in self.mut else self.L[(l + 1) % NL]["ln2"] if "ln2_other_layer" in self.mut else w["ln2"]
        if self.mode == "rows":
            # ar_mfma2_kernel OUT_RESID_STATS: ``xb = f32_to_bf16(xn * gpre[k])`` (x * ln_2.weight), (mean, M2) of x;
            # M2X_LN_AFTER: ``v = (v - st.x * gpre[k]) * st.y`` = rstd * (W . xb - mean * G)
            xb = self.operand(x * g2)
            mean, rstd = self.ln_stats(x)
            G = self.L[(l + 1) % NL]["gsum"] if "gsum_other_layer" in self.mut else w["gsum"]
            v = (xb @ w["fc"].T - mean * G) * rstd
        else:
            mean, rstd = self.ln_stats(x)
            xn = (x - mean) * rstd * g2
            v = self.operand(xn) @ w["fc"].T
        h = self._rows_out(self.gelu(v))
        if "fc_tail8" in self.mut:
            h = h.clone(); h[:, DFF - 8:] = 0
        return h  # before hb is stored: Model.store

    def store(self, rows):
        """An attention row or gelu(c_fc) as its buffer holds it: bf16 xn / hb on the MFMA paths, fp32 elsewhere."""
        return bf16_round(rows) if self.mode in BF16_OPERANDS else rows

    def mproj_copies(self, l, h):
        """mlp c_proj as the pending copies the path leaves, [B][n][768] (n = 0: one tensor, the whole output).
        fused: ar_mlp_fused_kernel ``atomicAdd(..., yfx_of(t, ...))``: every block's 16-column partial rounded to
        2^-32 (``__float2ll_rn(t * 4294967296.0f)``), summed exactly in int64."""
        w = self.layer(l)
        if "k_slice768" in self.mut:
            h = h.clone(); h[:, 768:1536] = 0
        B, n = h.shape[0], copies_of(self.mode, self.ksplit)
        if self.mode == "fused":
            part = torch.einsum("bkj,nkj->bkn", h.view(B, DFF // 16, 16), w["mproj"].view(D, DFF // 16, 16))
            part = torch.round(part.double() * 2.0 ** 32) / 2.0 ** 32
            return part.view(B, DFF // 64, 4, D).sum(dim=1).to(self.dt)
        if n == 0:
            return self._rows_out(h @ w["mproj"].T).unsqueeze(1)
        ks = DFF // n
        return torch.stack([self._rows_out(h[:, c * ks:(c + 1) * ks] @ w["mproj"][:, c * ks:(c + 1) * ks].T) for c in range(n)], 1)

    def fold(self, x, copies, l_next=1):
        """x + the pending copies, as the next layer's first kernel (or c_proj) folds them."""
        c = copies
        if "copy_unfolded" in self.mut:
            c = c[:, :-1]
        if "copy_twice" in self.mut:
            c = torch.cat([c, c[:, -1:]], 1)
        o = c.sum(dim=1)
        return o if "no_residual" in self.mut else x + o

    def lm_head(self, x):
        return self._lm_rows(self._rows_out(self.ln_rows(x, self.lnf) @ self.lm.T))

    def _lm_rows(self, lg):
        if "vocab4095_from_4094" in self.mut:
            lg = lg.clone(); lg[:, VOCAB - 1] = lg[:, VOCAB - 2]
        return lg

    # ---- a window of ops ------------------------------------------------------------------------------
    def window(self, first, last, rows, x_in=None, q_in=None, hist=None, kv="fp32", ns_max=1, stale=None, trace=None, kv_rows=None,
               state=None):
        """Ops first .. last on the rows ``rows`` = (text ids, prev tokens, positions; position -1: idle), from
        ``x_in`` / ``q_in`` as lvx_ar_ops takes them. hist(l, b) -> stored (K, V) [>= pos][768] of row b's slot.
        ``stale``: copies [B][n][768] that layer 0 must NOT fold (mutation copy_l0_stale folds them). ``trace``: a
        dict that receives every layer's k, v (("k", l), ("v", l)), the x entering the layer (("x0", l)), entering
        ln_2 (("x2", l)) and leaving the layer (("x4", l)). ``kv_rows``:
        l -> (k, v) [B][768], the rows layer l's attention finds at the rows' positions in place of this window's own
        c_attn output as the cache would round it: the GPU test passes the rows the device stored (held to the
        reference by the c_attn windows), so that, as in tests/attn_ref.py, the cache's rounding of a value that
        differs in its last bits is not part of the error measured downstream.
        ``state``: the window starts at ANY op from given buffers, a dict of x (the final residual), q, y (the stored
        attention rows) and h (the stored gelu(c_fc)): the chained references of the single-op comparisons.
        Returns a dict of what the last op left (y, h: before their buffer's rounding; y_stored, h_stored after it): q / k / v (k, v before the cache's rounding; k_stored, v_stored after it), y (attention rows), x (final: copies folded) with
        d = x - x_entry (x_entry: x_in, or at layer 0 the embedding), h, logits."""
        tid, prev, pos = rows
        dt = self.dt
        st = state or {}
        g = lambda n: None if st.get(n) is None else torch.as_tensor(st[n]).to(dt)
        x = g("x") if state is not None else self.embed(tid, prev, pos) if first == 0 else x_in.to(dt)
        x_entry = x
        if state is None and first == 0 and self.mut:  # the entry row the difference is taken from carries no mutation
            mut, self.mut = self.mut, NONE
            x_entry = self.embed(tid, prev, pos)
            self.mut = mut
        q = g("q") if state is not None else None if q_in is None else q_in.to(dt)
        k = v = None
        y, h = g("y"), g("h")
        res = {}
        for i in range(first, last + 1):
            if i == LM_HEAD:
                res = dict(logits=self.lm_head(x))
                break
            l, op = divmod(i, 5)
            if op == OP_QKV:
                if l == 0 and stale is not None and "copy_l0_stale" in self.mut:
                    x = x + stale.to(dt).sum(dim=1)
                if trace is not None:
                    trace["x0", l] = x
                q, k, v = self.c_attn(l, x)
                k_raw, v_raw = k, v
                k, v = kv_round(k, kv), kv_round(v, kv)
                if trace is not None:
                    trace["k", l], trace["v", l] = k, v
                res = dict(q=q, k=k_raw, v=v_raw, k_stored=k, v_stored=v)
            elif op == OP_ATTN:
                Ks, Vs = [], []
                for b, p in enumerate(pos):
                    if p < 0:
                        Ks.append(None); Vs.append(None)
                        continue
                    Kh, Vh = hist(l, b)
                    Kh, Vh = Kh[:p + 1].to(dt).clone(), Vh[:p + 1].to(dt).clone()
                    if kv_rows is not None and l in kv_rows:
                        Kh[p], Vh[p] = kv_rows[l][0][b].to(dt), kv_rows[l][1][b].to(dt)
                    elif k is not None:  # the row this window's c_attn appended
                        Kh[p], Vh[p] = k[b], v[b]
                    Ks.append(Kh); Vs.append(Vh)
                y_raw = self.attention(q, Ks, Vs, [p + 1 for p in pos], ns_max, kv)
                y = self.store(y_raw)
                k = v = None
                res = dict(y=y_raw, y_stored=y)
            elif op == OP_CPROJ:
                x = self.c_proj(l, x, y)
                if trace is not None:
                    trace["x2", l] = x
                res = dict(x=x, d=x - x_entry)
            elif op == OP_FC:
                h_raw = self.c_fc(l, x)
                h = self.store(h_raw)
                res = dict(h=h_raw, h_stored=h)
            else:
                x = self.fold(x, self.mproj_copies(l, h))
                if trace is not None:
                    trace["x4", l] = x
                res = dict(x=x, d=x - x_entry)
        res["x_entry"] = x_entry
        return res


# ----------------------------------------------------------------------------------------------------------
# The compared quantity
# ----------------------------------------------------------------------------------------------------------
def row_err(got, ref):
    """Per row: RMS(got - ref) / RMS(ref) in float64 (a zero reference row: the absolute RMS)."""
    g, r = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    g, r = g.reshape(g.shape[0], -1), r.reshape(r.shape[0], -1)
    den = np.sqrt((r * r).mean(axis=1))
    return np.sqrt(((g - r) ** 2).mean(axis=1)) / np.where(den > 0, den, 1.0)


KIND_OF_OP = {OP_QKV: "c_attn", OP_ATTN: "attn", OP_CPROJ: "c_proj", OP_FC: "c_fc", OP_MPROJ: "mproj"}


def kind_of(win, name=None):
    """The op kind a window's bound is kept for: its last op (every comparison is of that op alone, from the
    buffers the window without it left); the last 16-row vocabulary tile of the logits is a kind of its own
    (one wrong logit is 1 / 4,096 of a row's energy, and 1 / 16 of the tile's)."""
    if name == "logits_tail":
        return "lm_head_tail"
    return "lm_head" if win[1] == LM_HEAD else KIND_OF_OP[win[1] % 5]


def compared(res, win):
    """The tensors of a window's result that are compared, by name (y, h: before their buffer's rounding)."""
    op = "lm_head" if win[1] == LM_HEAD else KIND_OF_OP[win[1] % 5]
    if op == "c_attn":
        return {n: res[n] for n in ("q", "k", "v")}
    return {"attn": {"y": res.get("y")}, "c_proj": {"d": res.get("d")}, "mproj": {"d": res.get("d")},
            "c_fc": {"h": res.get("h")},
            "lm_head": {"logits": res.get("logits"), "logits_tail": None if res.get("logits") is None else res["logits"][:, VOCAB - 16:]}}[op]


def stored_format(name, mode, kv):
    """The number format of the buffer a compared tensor is read from: k / v the cache's, the attention rows and
    gelu(c_fc) bf16 on the MFMA paths; None: fp32, nothing was rounded."""
    if name in ("k", "v"):
        return None if kv == "fp32" else kv
    return "bf16" if name in ("y", "h") and mode in BF16_OPERANDS else None


def _cell_edges(stored, fmt):
    """[lo, hi] per element: the real values that round (to nearest) to the stored bf16 / e4m3fn value."""
    t = torch.as_tensor(np.ascontiguousarray(stored, dtype=np.float32))
    if fmt == "bf16":
        bits = (t.view(torch.int32) >> 16) & 0xFFFF
        sign, top, val = 0x8000, 0x7F80, lambda o: (torch.where(o < 0, (-o) | 0x8000, o) << 16).to(torch.int32).view(torch.float32)
    else:
        bits = t.clamp(-448.0, 448.0).to(torch.float8_e4m3fn).view(torch.uint8).to(torch.int32)
        sign, top, val = 0x80, 0x7F, lambda o: torch.where(o < 0, (-o) | 0x80, o).to(torch.uint8).view(torch.float8_e4m3fn).float()
    o = torch.where((bits & sign) != 0, -(bits & (sign - 1)), bits)  # ordered: o + 1 is the next value up
    up, dn = o + 1, o - 1
    hi = torch.where(up >= top, torch.full_like(t, math.inf), (val(torch.clamp(up, max=top - 1)).double() + t.double()) / 2)
    lo = torch.where(dn <= -top, torch.full_like(t, -math.inf), (val(torch.clamp(dn, min=-(top - 1))).double() + t.double()) / 2)
    return lo.double().numpy(), hi.double().numpy()


def dev_err(got, ref, fmt=None):
    """Per row, the error of what a buffer holds against the unrounded reference. fp32 buffers: row_err. bf16 / fp8
    buffers: the SMALLEST error consistent with the stored value, i.e. the distance from the reference to the
    interval of reals that round to it (0 inside it), as RMS over the row relative to the RMS of the reference.
    The format's own rounding, ties included, is thereby no part of the figure, and a systematic error is held
    to the same per-row RMS bound as everywhere else."""
    if fmt is None:
        return row_err(got, ref)
    r = np.asarray(ref, dtype=np.float64)
    lo, hi = _cell_edges(got, fmt)
    dist = np.maximum(0.0, np.maximum(lo - r, r - hi)).reshape(r.shape[0], -1)
    den = np.sqrt((r.reshape(r.shape[0], -1) ** 2).mean(axis=1))
    return np.sqrt((dist ** 2).mean(axis=1)) / np.where(den > 0, den, 1.0)


def as_stored(res, win):
    """A model result in the form the device hands a window's result out: name -> what the buffers hold."""
    out = dict(compared(res, win))
    for n in ("k", "v", "y", "h"):
        if n + "_stored" in res:
            out[n] = res[n + "_stored"]
    if "x" in res:
        out["x"] = res["x"]
    return out


# The yardstick of an (op kind, mode): the largest dev_err, over the cells and windows of tests/test_gpu_ar_ops.py
# that end in that op, of the mode's model evaluated in torch float32 on the CPU (its buffers as the device's)
# from the same model in float64, op by op from the same input buffers. The device bound is MARGIN x that: the
# margin the codec stages and the attention tests give for summation order. Tie flips are no part of either
# figure (dev_err for the buffers, Model.operand / resolved_reference for the operand rows inside an op), so the
# figures are fp32-sized in every mode. They are computed where the tests run (once per module): a float32
# sum depends on the order the BLAS adds in; DESIGN.md records those of the run that wrote it.
MARGIN = 8.0
YARDSTICK = {}  # (kind, mode) -> figure, filled by ensure_yardsticks


def bound(kind, mode):
    return MARGIN * YARDSTICK[kind, mode]


# ----------------------------------------------------------------------------------------------------------
# Cells: the plan cells of the GEMM ops. info: (path, fused_mlp, nsplit, attn_direct, attn8, xpk, ksplit, qsplit,
# pending copies, fixed point) as lvx_ar_ops reports the plan (ar_plan.h); mode: the model's.
# ----------------------------------------------------------------------------------------------------------
Cell = namedtuple("Cell", "eng B opts info mode full")
POSITIONS = (0, 1, 63, 64, 65, 127, 128, 129)
MAX_POSITIONS = 256
HIST_ROWS = 192  # rows written per (slot, layer): the keys and the stale rows up to the end of the 128-key tile
ENGINES = {"bf16": ("bf16", "bf16"), "fp8": ("bf16", "fp8"), "fp32": ("fp32", "fp32")}
MAX_STREAMS = {"bf16": 65, "fp8": 17, "fp32": 64}
DEFAULT_OPTS = {"bt": 1, "ln_max": 8, "exp": 0, "f32b": 1, "fuse_mlp": 1, "defer_select": 1}
GEMV, MLN, MROWS, BT, F32B = 0, 1, 2, 3, 4


def cells():
    c = []
    gemv = (GEMV, 0, 16, 0, 0, 0, 0, 0, 0, 0)
    for B in (1, 2):
        c.append(Cell("bf16", B, {}, (GEMV, 1, 16, 0, 0, 0, 0, 0, 4, 1), "fused", True))
        c.append(Cell("bf16", B, {"fuse_mlp": 0}, gemv, "gemv", True))
    c.append(Cell("bf16", 65, {}, gemv, "gemv", True))
    for B in (3, 4):
        c.append(Cell("bf16", B, {}, (MLN, 0, 8, 0, 0, 0, 0, 0, 2, 0), "ln", True))
    for B in (5, 8):
        c.append(Cell("bf16", B, {}, (MLN, 0, 1, 1, 1, 0, 0, 0, 2, 0), "ln", True))
    c.append(Cell("bf16", 6, {"ln_max": 4}, (MROWS, 0, 1, 2, 1, 1, 0, 0, 4, 0), "rows", True))
    for B in (9, 16, 17, 32):
        c.append(Cell("bf16", B, {}, (MROWS, 0, 1, 2, 0, 1, 0, 0, 4, 0), "rows", True))
    for B in (33, 48, 49, 64):
        c.append(Cell("bf16", B, {}, (BT, 0, 1, 0, 0, 0, 0, 0, 0, 0), "bt", True))
    c.append(Cell("bf16", 8, {"bt": 2}, (BT, 0, 4, 0, 0, 0, 0, 0, 0, 0), "bt", True))
    c.append(Cell("bf16", 16, {"bt": 2}, (BT, 0, 2, 0, 0, 0, 0, 0, 0, 0), "bt", True))
    # fp8 KV: the c_attn and (attention, c_proj) windows only
    c.append(Cell("fp8", 1, {}, (GEMV, 1, 16, 0, 0, 0, 0, 0, 4, 1), "fused", False))
    c.append(Cell("fp8", 4, {}, (MLN, 0, 8, 0, 0, 0, 0, 0, 2, 0), "ln", False))
    c.append(Cell("fp8", 8, {}, (MLN, 0, 1, 1, 1, 0, 0, 0, 2, 0), "ln", False))
    c.append(Cell("fp8", 16, {}, (MROWS, 0, 1, 2, 1, 1, 0, 0, 4, 0), "rows", False))
    c.append(Cell("fp8", 17, {}, (MROWS, 0, 1, 2, 0, 1, 0, 0, 4, 0), "rows", False))
    for B, ns in ((3, 8), (16, 2)):
        c.append(Cell("fp32", B, {}, (F32B, 0, ns, 0, 0, 0, 1, 1, 4, 0), "f32", True))
    for B in (17, 32):
        c.append(Cell("fp32", B, {}, (F32B, 0, 1, 3, 0, 0, 1, 1, 4, 0), "f32", True))
    for B in (33, 64):
        c.append(Cell("fp32", B, {}, (F32B, 0, 1, 3, 0, 0, 1, 0, 4, 0), "f32", True))
    c.append(Cell("fp32", 12, {"exp": 512}, (F32B, 0, 2, 0, 0, 0, 0, 0, 0, 0), "f32", True))
    c.append(Cell("fp32", 3, {"exp": 1024}, (F32B, 0, 8, 0, 0, 0, 1, 0, 4, 0), "f32", True))
    c.append(Cell("fp32", 32, {"exp": 1024}, (F32B, 0, 1, 3, 0, 0, 1, 0, 4, 0), "f32", True))
    for B in (3, 12):
        c.append(Cell("fp32", B, {"f32b": 0}, gemv, "f32", True))
    return c


def cell_id(c):
    o = ",".join(f"{k}={v}" for k, v in c.opts.items())
    return f"{c.eng}-B{c.B}" + (f"-{o}" if o else "")


def cell_ksplit(c):
    """Whether the cell's model holds pending copies under fp32 weights (PATH_F32B with the K split)."""
    return bool(c.info[6])


def windows(c):
    """(first, last, entry) of a cell's windows, providers before their dependants; entry "x": at a layer boundary,
    "q": at the attention. Every window (first, last) with last > first is compared as its LAST op alone, the
    reference starting from what the window (first, last - 1) left on the device (provider_of): the windows from
    layers 0, 1 and 3's boundaries to each of their ops, the two-layer windows 0 .. 9 and 10 .. 19 (a real set of
    pending copies folded by the next layer's first kernel) with every window on the way to them, 15 .. 20, and
    (attention, c_proj) with given q after the attention alone."""
    fused = c.info[1]
    w = []

    def chain(first, last):
        for i in range(first, last + 1):
            if fused and i != LM_HEAD and i % 5 == OP_FC:  # no c_fc kernel of its own: on to mlp c_proj
                continue
            if (first, i, "x") not in w:
                w.append((first, i, "x"))

    if c.full:
        chain(0, 9)
        chain(5, 9)
        chain(10, 19)
        chain(15, 20)
    else:
        w += [(5 * l, 5 * l, "x") for l in (0, 1, 3)]
    for l in (0, 2):
        w += [(5 * l + 1, 5 * l + 1, "q"), (5 * l + 1, 5 * l + 2, "q")]
    return w


def provider_of(c, win):
    """The window whose result is the input of `win`'s last op (None: the op starts from the window's own input)."""
    first, last, entry = win
    if last == first:
        return None
    prev = last - 1
    if c.info[1] and prev != LM_HEAD and prev % 5 == OP_FC:
        prev -= 1
    return (first, prev, entry)


# ----------------------------------------------------------------------------------------------------------
# Inputs. The residual rows: per-row gain and offset at the scale of the residual stream entering layers 1-3 of
# the oracle's model (RMS 0.14-0.25); the first, last and every 16th row +- 1 with a seeded
# third of the channels raised 8x; one row per call with mean / std = 2 x MEAN_OVER_STD, the largest |mean| / std
# of x entering ln_2 over the oracle's 256 golden steps (tests/test_ar_ref.py measures it), to load the
# cancellation in rstd * (W . xb - mean * G).
# ----------------------------------------------------------------------------------------------------------
SEED = 20261020
MEAN_OVER_STD = 0.1314  # measured: 0.13137 (layer and step of the maximum: tests/test_ar_ref.py prints them)


def row_slots(B, S):
    return A.row_slots(B, S)


def slot_pos(slot):
    """A slot keeps one position in every cell (its cache rows below it are never overwritten)."""
    return POSITIONS[slot % len(POSITIONS)]


def slot_prev(slot):
    return (slot * 977 + 4095) % VOCAB  # (slot 0: vocabulary row 4,095)


def slot_text(slot):
    return (slot * 131 + 7) % 386


def spiked_rows(B):
    r = {0, B - 1}
    for b in range(16, B + 1, 16):
        r |= {b - 1, b, b + 1}
    return sorted(b for b in r if 0 <= b < B)


def x_rows(B, tag):
    """x_in float32 [B][768] of a window (tag: any ints that name it)."""
    rng = np.random.default_rng([SEED, B] + list(tag))
    x = rng.standard_normal((B, D))
    x = x * rng.uniform(0.12, 0.28, (B, 1)) + rng.uniform(-0.02, 0.02, (B, 1))
    for b in spiked_rows(B):
        ch = rng.permutation(D)[:D // 3]
        x[b, ch] *= 8.0
    big = B // 3  # the row with the large mean
    x[big] += 2.0 * MEAN_OVER_STD * x[big].std() - x[big].mean()
    return x.astype(np.float32)


def history(slot, layer):
    """Unquantised K ~ 0.7 N(0, 1), V ~ N(0, 1) rows [HIST_ROWS][768] of one (slot, layer)."""
    rng = np.random.default_rng([SEED, 7, slot, layer])
    return (0.7 * rng.standard_normal((HIST_ROWS, D), dtype=np.float32), rng.standard_normal((HIST_ROWS, D), dtype=np.float32))


def q_rows(slots, layer, K_of, ns_max, kv):
    """Spiked queries (A.row_queries, set 0) of the rows over their stored keys; an idle row: zeros."""
    q = np.zeros((len(slots), D), dtype=np.float32)
    for b, s in enumerate(slots):
        if s < 0:
            continue
        t = slot_pos(s) + 1
        qs, _ = A.row_queries(K_of(layer, b), t, A.edge_keys(t, ns_max, kv), s)
        q[b] = qs[0].reshape(D)
    return q


MIN_ROW_DISTANCE = 50.0  # adjacent reference rows are further apart than this many times the bound


def adjacent_row_distance(ref):
    """Smallest over b of RMS(ref[b + 1] - ref[b]) / RMS(ref[b + 1]): a misplaced row moves the output by this."""
    r = np.asarray(ref, dtype=np.float64).reshape(len(ref), -1)
    if r.shape[0] < 2:
        return np.inf
    live = [b for b in range(r.shape[0] - 1) if r[b].any() and r[b + 1].any()]
    return min((float(row_err(r[b:b + 1], r[b + 1:b + 2])[0]) for b in live), default=np.inf)


# ----------------------------------------------------------------------------------------------------------
# One cell's rows and one window's inputs and reference, shared by the CPU and the GPU test
# ----------------------------------------------------------------------------------------------------------
_HIST = {}


def stored_history(kv, slot, layer):
    """(K, V) float32 tensors [HIST_ROWS][768]: the history as the cache dtype stores it (what lvx_kv_read
    returns after lvx_kv_write: tests/test_gpu_ar_ops.py asserts that)."""
    key = (kv, slot, layer)
    if key not in _HIST:
        k, v = history(slot, layer)
        _HIST[key] = (torch.from_numpy(A.quantise(k, kv)), torch.from_numpy(A.quantise(v, kv)))
    return _HIST[key]


class Case:
    """The rows of a cell: permuted slots (or the given ones), each at its slot's position, previous token and
    text id."""

    def __init__(self, cell, idle=None, slots=None):
        self.cell, self.B = cell, cell.B
        self.kv = ENGINES[cell.eng][1]
        self.slots = list(slots) if slots is not None else row_slots(cell.B, MAX_STREAMS[cell.eng])
        if idle is not None:
            self.slots[idle] = -1
        self.pos = [slot_pos(s) if s >= 0 else -1 for s in self.slots]
        self.rows = ([slot_text(max(s, 0)) for s in self.slots], [slot_prev(max(s, 0)) for s in self.slots], self.pos)

    def hist(self, l, b):
        return stored_history(self.kv, self.slots[b], l)

    def inputs(self, win, ns_max=None):
        """(x_in, q_in) float32 arrays of a window (None where the entry takes none)."""
        first, last, entry = win
        x = None if first == 0 else x_rows(self.B, (first, int(entry == "q")))  # (one input per chain of windows)
        q = None
        if entry == "q":
            ns = self.cell.info[2] if ns_max is None else ns_max
            q = q_rows(self.slots, first // 5, lambda l, b: self.hist(l, b)[0].numpy(), ns, self.kv)
        return x, q

    def reference(self, model, win, x, q, stale=None, ns_max=None, trace=None, kv_rows=None):
        """The whole window on the model, from the window's own input."""
        first, last, _ = win
        ns = self.cell.info[2] if ns_max is None else ns_max
        return model.window(first, last, self.rows, None if x is None else torch.from_numpy(x),
                            None if q is None else torch.from_numpy(q), self.hist, self.kv, ns, stale, trace, kv_rows)

    def entry_state(self, model, win, x, q):
        """The buffers a chain of windows starts from: x_in (layer 0: the reference embedding) and q_in."""
        first = win[0]
        x0 = model.embed(*self.rows) if first == 0 else torch.from_numpy(x).to(model.dt)
        return dict(x=x0.double(), q=None if q is None else torch.from_numpy(q).double())

    def last_op(self, model, win, state, kv_rows=None, b=None, stale=None):
        """The ops of `win` after its provider's (its last op; c_fc + mlp c_proj inside the fused MLP) on the model,
        from the buffers `state` (x, q, y, h as the provider left them). b: row b alone."""
        prov = provider_of(self.cell, win)
        start = win[0] if prov is None else prov[1] + 1
        rows, hist = self.rows, self.hist
        if b is not None:
            rows = tuple([r[b]] for r in self.rows)
            hist = lambda l, _: self.hist(l, b)
            state = {n: None if t is None else t[b:b + 1] for n, t in state.items()}
            kv_rows = None if kv_rows is None else {l: (k[b:b + 1], v[b:b + 1]) for l, (k, v) in kv_rows.items()}
        if prov is None and win[0] == 0:  # layer 0 embeds itself (the mutations of the embedding apply)
            return model.window(0, win[1], rows, None, None, hist, self.kv, self.cell.info[2], stale, None, kv_rows)
        return model.window(start, win[1], rows, None, None, hist, self.kv, self.cell.info[2], stale, None, kv_rows, state=state)

    @staticmethod
    def next_state(state, win, dev):
        """The buffers after `win`, from those before its last op and what the window handed out (as_stored's names)."""
        st = dict(state)
        for name, key in (("q", "q"), ("y", "y"), ("h", "h"), ("x", "x")):
            if dev.get(name) is not None:
                st[key] = torch.as_tensor(np.asarray(dev[name], dtype=np.float64))
        return st

    @staticmethod
    def appended_layer(win):
        """The layer whose attention, as a window's last op, reads a row that the window's own c_attn appended."""
        first, last, entry = win
        return last // 5 if entry == "x" and last != LM_HEAD and last % 5 == OP_ATTN else None


def window_errors(case, model, win, dev, ref):
    """name -> per-row dev_err of what the device (or another evaluation) left against the reference."""
    out = {}
    for name, r in compared(ref, win).items():
        d = dev["x"] - ref["x_entry"].numpy() if name == "d" else dev[name]
        out[name] = dev_err(np.asarray(d, dtype=np.float64), r.numpy(), stored_format(name, model.mode, case.kv))
    return out


def resolved_reference(case, model, win, state, kv_rows, dev):
    """The float64 reference of a window's last op, with every operand element that lies within AMB_REL of a bf16
    rounding boundary (Model.operand) rounded to the side that brings the row nearer to `dev`: the device rounds
    its own fp32 value of that element, and either side is a correct result. At most 10 such elements per row
    are tried (2^10 evaluations of one row); a row with more keeps round-to-nearest."""
    amb = []
    model.amb = amb
    try:
        ref = case.last_op(model, win, state, kv_rows)
    finally:
        model.amb = None
    if not amb or dev is None:
        return ref
    ref = {n: (t.clone() if torch.is_tensor(t) else t) for n, t in ref.items()}
    rows = {}
    for b, k, lo, hi in amb:
        rows.setdefault(b, []).append((k, lo, hi))
    import itertools
    for b, items in rows.items():
        if len(items) > 10:
            continue
        dev_b = {n: (None if t is None else np.asarray(t)[b:b + 1]) for n, t in dev.items()}
        best = None
        for combo in itertools.product((0, 1), repeat=len(items)):
            model.force = {(0, k): (hi if c else lo) for c, (k, lo, hi) in zip(combo, items)}
            try:
                r = case.last_op(model, win, state, kv_rows, b=b)
            finally:
                model.force = {}
            e = sum(float(v[0]) for v in window_errors(case, model, win, dev_b, r).values())
            if best is None or e < best[0]:
                best = (e, r)
        for n, t in best[1].items():
            if torch.is_tensor(t) and torch.is_tensor(ref.get(n)) and ref[n].shape[1:] == t.shape[1:]:
                ref[n][b] = t[0]
    return ref


# ----------------------------------------------------------------------------------------------------------
# The yardsticks
# ----------------------------------------------------------------------------------------------------------
_MODELS = {}


def model_for(weights, mode, dt, ksplit=True, mut=NONE):
    """Cached Model over weights = (gpt dict, text table, codebook)."""
    key = (id(weights[0]), mode, dt, ksplit, frozenset(mut))
    if key not in _MODELS:
        _MODELS[key] = Model(weights[0], weights[1], weights[2], mode, dt, mut, ksplit)
    return _MODELS[key]


def model_chain(case, m64, upto=None):
    """Every window of the cell on the float64 model, each from what its provider left (the model's own buffers in
    the device's place): win[:2] + entry -> (state before the last op, kv_rows, result). upto: stop after it."""
    out = {}
    for win in windows(case.cell):
        x, q = case.inputs(win)
        prov = provider_of(case.cell, win)
        state = case.entry_state(m64, win, x, q) if prov is None else out[prov][3]
        l = Case.appended_layer(win)
        kv_rows = None if l is None else {l: out[prov][4]}
        res = case.last_op(m64, win, state, kv_rows)
        dev = as_stored(res, win)
        out[win] = (state, kv_rows, res, Case.next_state(state, win, dev), (dev.get("k"), dev.get("v")))
        if win == upto:
            break
    return out


def measure_yardsticks(weights, cell_list=None):
    """(kind, mode) -> the largest row error of the float32 evaluation of an op from the float64 one, both from the
    buffers the float64 chain left, over the cells' windows (a value stored in a rounded buffer: of the value before
    its rounding; the device's buffer is then held to that bound by dev_err, which never exceeds the true error)."""
    out = {}
    for c in (cells() if cell_list is None else cell_list):
        case = Case(c)
        m64 = model_for(weights, c.mode, torch.float64, cell_ksplit(c))
        m32 = model_for(weights, c.mode, torch.float32, cell_ksplit(c))
        for win, (state, kv_rows, _, _, _) in model_chain(case, m64).items():
            ev = case.last_op(m32, win, state, kv_rows)
            dev = {n: (None if t is None else t.double().numpy()) for n, t in as_stored(ev, win).items()}
            ref = resolved_reference(case, m64, win, state, kv_rows, dev)
            for name, e in window_errors(case, m64, win, dev, ref).items():
                if stored_format(name, c.mode, case.kv):  # a rounded buffer: the yardstick is that of the value before
                    e = row_err(compared(ev, win)[name].double().numpy(), compared(ref, win)[name].numpy())  # its rounding
                key = (kind_of(win, name), c.mode)
                out[key] = max(out.get(key, 0.0), float(e.max()))
    return out


def ensure_yardsticks(weights):
    if not YARDSTICK:
        YARDSTICK.update(measure_yardsticks(weights))
    return YARDSTICK
