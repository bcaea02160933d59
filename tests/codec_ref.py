"""fp64 reference of the codec decode, one function per stage of ``lvx_codec_stages``, with the rounding
points of each device mode.

TEST INFRASTRUCTURE ONLY. The formulas are those ``oracle/reference_cpu.py`` cites (decoder/models.py,
modules.py, heads.py, spectral_ops.py); with ``mode="fp32"`` and fp64 weights they are that reference in
double precision. ``mode="bf16"`` inserts the roundings of the bf16 weight mode, each read from
``llmvox_amd/csrc/codec_kernels.hip`` (function / statement cited beside it):

* GEMM weights rounded to bf16 (lvx_api.cpp ``upload_w``: ``h[i] = f32_to_bf16(v[i])``, RNE);
* operands their producer stores as bf16 (``decode_impl``: ``typedef TW TAct`` and the ``gn`` / ``t2a`` /
  ``t1a`` / ``feats`` pointers of that type): GroupNorm(+swish) output (``gn_store`` -> ``store4(bf16_t*)``),
  dwconv + AdaLN output (``dwconv_adaln_tile_kernel``: ``store_out<TO>``), GELU(pwconv1) output (``gemm_w<...,
  E_BIAS_GELU, TAct>``: TC = bf16), final-LN output (``ln_affine_kernel``: ``store_out<TO>``), the gathered
  codebook rows (``codes_gather_bf16_kernel``) and the attention's h (``gemm_act<TW, E_BIAS, TAct>(p, ...)``);
* the fp32 q / k / P / V rounded to bf16 on the way into LDS by ``gemm_mfma_kernel<BF = true>`` (``gemm_act``:
  ``gemm_launch<true, float, float, ...>``);
* ``mode="fp8"`` (codec_dtype FP8 over the bf16 mode: the same activation roundings): GEMM weights quantised by
  lvx_api.cpp ``upload_cw``'s rule (per row ``s = max|w| / 448``, ``q = f32_to_e4m3_host(w / s)``: RNE, saturated
  e4m3fn; ``gemm_bf16_kernel<fp8_t>`` widens q exactly and multiplies the accumulator by ``g.wscale[col]``); for
  the W8A8 pwconv1 (``decode_impl``: ``q8``, >= 192 tiles and codec_exp bit 32 clear) the dwconv + AdaLN output
  quantised per frame instead of rounded to bf16 (``dwconv_adaln_tile_kernel<fp8_t>``: ``sf = m * (1 / 448)``,
  ``inv = 1 / sf``, ``f32_to_fp8(o * inv)``; ``gemm_glds_kernel<fp8_t>`` runs unit E8M0 scales and applies both
  fp32 scales in the epilogue);
* (``mode="fp32"`` at >= 192 tiles of 128 x 192, option codec_g3f = 2: the weight GEMM's bf16x3 products, see
  ``_lin``; no rounding anywhere else in that mode);
* everything else (accumulation, norms, softmax, epilogues, the residual stream, the iSTFT) unrounded.

Every function takes ``dt`` (torch.float64: the reference; torch.float32: the same model evaluated in
single precision, the yardstick of the device bounds) and ``mut``, a set of named mutations (the indexing
and omission errors ``tests/test_codec_ref.py`` proves the comparison sensitive to).

Layout: the residual stream is [B, L, 768] (time-major, as on the device).
"""
from __future__ import annotations

import math
import zlib
from typing import Dict, Optional

import numpy as np
import torch

CD, CFF, CIN, NFFT, HOP, NB = 768, 2304, 512, 1280, 320, 641
N_STAGES = 21
CODEBOOK_KEY = "feature_extractor.encodec.quantizer.vq.layers.0._codebook.embed"
RESNET_OF_STAGE = {1: 0, 2: 1, 4: 3, 5: 4}  # stage -> pos_net index
NONE = frozenset()

# stage kinds: the (stage kind, mode) pairs bounds are kept for
KINDS = {0: "embed", 1: "resnet", 2: "resnet", 3: "attn", 4: "resnet", 5: "resnet", 6: "gn_adaln", 19: "head",
         20: "istft"}
KINDS.update({s: "convnext" for s in range(7, 19)})
HAS_RESIDUAL = {"resnet", "attn", "convnext"}


def e4m3_round(x: torch.Tensor) -> torch.Tensor:
    """RNE to e4m3fn (saturated at +-448) of the fp32 value of x, back in x's dtype."""
    return x.to(torch.float32).clamp(-448.0, 448.0).to(torch.float8_e4m3fn).to(x.dtype)


def bf16_round(x: torch.Tensor) -> torch.Tensor:
    """RNE to bf16 of the fp32 value of x (the device rounds an fp32 register), back in x's dtype."""
    return x.to(torch.float32).to(torch.bfloat16).to(x.dtype)


class Weights:
    """The codec's state dict in ``dt``, GEMM weights rounded per ``mode``; conv weights also tap-major
    [N][T * C] as the device's implicit-conv GEMMs read them (lvx_api.cpp ``repack_conv``)."""

    GEMM_SUFFIX = ("embed.weight", ".conv1.weight", ".conv2.weight", ".q.weight", ".k.weight", ".v.weight",
                   "proj_out.weight", "pwconv1.weight", "pwconv2.weight", "head.out.weight")

    def __init__(self, cw: Dict[str, np.ndarray], mode: str, dt=torch.float64):
        assert mode in ("fp32", "bf16", "fp8")
        self.mode, self.dt = mode, dt
        self.w8a8 = True  # mode "fp8": codec_exp bit 32 clear (the default)
        self.g3f = 2  # option codec_g3f of the engine compared against (default 2)
        self.w = {}
        for k, v in cw.items():
            t = torch.from_numpy(np.ascontiguousarray(np.asarray(v, dtype=np.float32)))
            if mode == "bf16" and k.endswith(self.GEMM_SUFFIX):
                t = t.to(torch.bfloat16).to(torch.float32)  # upload_w
            if mode == "fp8" and k.endswith(self.GEMM_SUFFIX):  # upload_cw (on the repacked rows: the same sets)
                rows = t.reshape(t.shape[0], -1)
                mx = rows.abs().amax(dim=1, keepdim=True)
                sc = torch.where(mx > 0, mx / 448.0, torch.ones_like(mx))  # fp32, as the host computes it
                t = (e4m3_round(rows / sc).to(torch.float64) * sc.to(torch.float64)).reshape(t.shape)
            t = t.to(dt)
            if t.dim() == 3 and not k.endswith("dwconv.weight"):
                t = t.permute(0, 2, 1).reshape(t.shape[0], -1).contiguous()  # [N][C][T] -> [N][T * C]
            self.w[k] = t

    def __getitem__(self, k):
        return self.w[k]

    def x3(self, M: int, N: int, K: int) -> bool:
        """fp32 parity mode: this weight GEMM runs as bf16x3 split products (codec_kernels.hip ``g3_split``:
        option codec_g3f == 2 and ``g3_ok<float>``: K % 32 == 0 and >= 192 tiles of 128 x 192)."""
        return (self.mode == "fp32" and self.g3f == 2 and K % 32 == 0
                and ((M + 127) // 128) * ((N + 191) // 192) >= 192)

    def act(self, x):
        """An operand its producer stores in the GEMM's input precision."""
        return bf16_round(x) if self.mode in ("bf16", "fp8") else x

    def q8(self, M: int) -> bool:
        """mode "fp8": pwconv1 runs W8A8 (``decode_impl``'s ``q8``: ``g3_ok<fp8_t>`` at N = 2,304, K = 768)."""
        return self.mode == "fp8" and self.w8a8 and ((M + 127) // 128) * 12 >= 192

    def act8(self, x):
        """Rows of x as e4m3fn with one fp32 scale per row (dwconv_adaln_tile_kernel<fp8_t>), dequantised."""
        x32 = x.to(torch.float32)
        m = x32.abs().amax(dim=-1, keepdim=True)
        sf = torch.where(m > 0, m * torch.tensor(1.0 / 448.0, dtype=torch.float32), torch.ones_like(m))
        q = e4m3_round(x32 * (1.0 / sf))
        return (q.to(torch.float64) * sf.to(torch.float64)).to(x.dtype)


# ---------------------------------------------------------------------------
# building blocks
# ---------------------------------------------------------------------------

def _split(x):
    hi = bf16_round(x)
    return hi, bf16_round(x - hi)


def _lin(W, a, w, b, mut=NONE):
    """a [.., K] @ w[N][K]^T + b, a weight GEMM of the decode over M = all rows of the call."""
    if "drop_k32" in mut or "drop_k64" in mut:
        n = 32 if "drop_k32" in mut else 64
        a = a.clone()
        a[..., -n:] = 0
    M, (N, K) = a.numel() // a.shape[-1], w.shape
    if W.x3(M, N, K):
        # gemm_glds_kernel<float, SPLIT>: each operand as hi + lo bf16 parts (gn_store / split_store /
        # upload_cw: hi = bf16(x), lo = bf16(x - hi)), the products hi hi + hi lo + lo hi (lo lo dropped)
        (ah, al), (wh, wl) = _split(a), _split(w)
        y = ah @ wh.t() + (ah @ wl.t() + al @ wh.t())
    else:
        y = a @ w.t()
    if b is not None and "no_bias" not in mut:
        y = y + b
    return y


def _taps(x, T, mut=NONE):
    """x [B, L, C] -> [B, L, T * C]: the T frames centred on each frame, zero beyond the stream's ends
    (A_CONV: 'zero padding at every stream's edges'); tap-major like the repacked weights."""
    B, L, C = x.shape
    p = T // 2
    if "conv_leak" in mut:  # the window runs on into the neighbouring streams of the call
        flat = x.reshape(1, B * L, C)
        xp = torch.nn.functional.pad(flat, (0, 0, p, p))
        return torch.cat([xp[:, t:t + B * L] for t in range(T)], dim=2).reshape(B, L, T * C)
    xp = torch.nn.functional.pad(x, (0, 0, p, p))
    return torch.cat([xp[:, t:t + L] for t in range(T)], dim=2)


def _conv(W, x, w, b, T, mut=NONE):
    return _lin(W, _taps(x, T, mut), w, b, mut)


def _gn(x, w, b, mut=NONE):
    """GroupNorm(32, eps 1e-6, affine) over one stream (models.py:15-16); x [B, L, 768]."""
    B, L, C = x.shape
    g = x.reshape(B, L, 32, C // 32)
    mean = g.mean(dim=(1, 3), keepdim=True)
    var = ((g - mean) ** 2).mean(dim=(1, 3), keepdim=True)
    if "gn_next_stream" in mut:
        mean, var = mean.roll(-1, 0), var.roll(-1, 0)
    return ((g - mean) / torch.sqrt(var + 1e-6)).reshape(B, L, C) * w + b


def _swish(x):
    return x * torch.sigmoid(x)


def _ln(x, eps=1e-6):
    m = x.mean(dim=-1, keepdim=True)
    v = ((x - m) ** 2).mean(dim=-1, keepdim=True)
    return (x - m) / torch.sqrt(v + eps)


def _gelu(x):  # F.gelu (erf form), modules.py:52
    return 0.5 * x * (1.0 + torch.erf(x * (1.0 / math.sqrt(2.0))))


def _finish(x, branch, mut):
    """(out, branch) of a stage with a residual."""
    if "last_row_copy" in mut:
        flat = branch.reshape(-1, branch.shape[-1]).clone()
        flat[-1] = flat[-2]
        branch = flat.reshape(branch.shape)
    out = branch if "no_residual" in mut else x + branch
    return out, branch


# ---------------------------------------------------------------------------
# the stages
# ---------------------------------------------------------------------------

def embed(W: Weights, codes, mut=NONE):
    """Stage 0: codebook rows of the codes (pretrained.py:209-239, n_q = 1) -> embed Conv1d k7 pad 3
    (models.py:223). codes int64 [B, L] -> x [B, L, 768]."""
    feats = W.act(W[CODEBOOK_KEY][codes])  # codes_gather_bf16_kernel
    x = _conv(W, feats, W["backbone.embed.weight"], W["backbone.embed.bias"], 7, mut)
    return _finish(None, x, mut | {"no_residual"})


def resnet(W: Weights, i: int, x, mut=NONE):
    """Stages 1, 2, 4, 5: ResnetBlock pos_net.i (models.py:58-78)."""
    p = f"backbone.pos_net.{i}."
    h = W.act(_swish(_gn(x, W[p + "norm1.weight"], W[p + "norm1.bias"], mut)))  # gn_apply: gn_store
    h = _conv(W, h, W[p + "conv1.weight"], W[p + "conv1.bias"], 3, mut)
    h = W.act(_swish(_gn(h, W[p + "norm2.weight"], W[p + "norm2.bias"], mut)))
    return _finish(x, _conv(W, h, W[p + "conv2.weight"], W[p + "conv2.bias"], 3, mut), mut)


def attn(W: Weights, x, mut=NONE):
    """Stage 3: AttnBlock pos_net.2 (models.py:107-127)."""
    p = "backbone.pos_net.2."
    B, L, C = x.shape
    h = W.act(_gn(x, W[p + "norm.weight"], W[p + "norm.bias"], mut))
    wqkv = torch.cat([W[p + "q.weight"], W[p + "k.weight"], W[p + "v.weight"]], 0)
    bqkv = torch.cat([W[p + "q.bias"], W[p + "k.bias"], W[p + "v.bias"]], 0)
    q, k, v = _lin(W, h, wqkv, bqkv, mut).split(C, dim=2)  # fp32 in t1 (gemm_w<..., E_BIAS>: TC = float)
    # gemm_act: gemm_launch<true, float, float>: both operands rounded into LDS (BF = true)
    s = (W.act(q) @ W.act(k).transpose(1, 2)) * (768 ** -0.5)
    if "softmax_pad" in mut:  # the row taken at its padded length (L + 3) & ~3 (the padding holds zeros)
        ld = (L + 3) & ~3
        s = torch.nn.functional.pad(s, (0, ld - L))
        pr = torch.softmax(s, dim=2)[:, :, :L]
    else:
        pr = torch.softmax(s, dim=2)
    hh = W.act(W.act(pr) @ W.act(v))  # gemm_act<TW, E_BIAS, TAct>: h stored as bf16
    return _finish(x, _lin(W, hh, W[p + "proj_out.weight"], W[p + "proj_out.bias"], mut), mut)


def gn_adaln(W: Weights, x, bw: int, mut=NONE):
    """Stage 6: pos_net.5 GroupNorm, then the backbone's AdaLayerNorm (models.py:230-232, modules.py:81-86).
    fp32 in every mode (gn_adaln_kernel writes x)."""
    if "other_bw" in mut:
        bw = (bw + 1) % 4
    y = _gn(x, W["backbone.pos_net.5.weight"], W["backbone.pos_net.5.bias"], mut)
    y = _ln(y) * W["backbone.norm.scale.weight"][bw] + W["backbone.norm.shift.weight"][bw]
    return _finish(None, y, mut | {"no_residual"})


def convnext(W: Weights, i: int, x, bw: int, mut=NONE):
    """Stages 7 .. 18: ConvNeXtBlock i (modules.py:43-60)."""
    p = f"backbone.convnext.{i}."
    B, L, C = x.shape
    if "other_bw" in mut:
        bw = (bw + 1) % 4
    dw = W[p + "dwconv.weight"][:, 0, :]  # [768][7], fp32 in every mode (dwconv_adaln_tile_kernel reads floats)
    t = _taps(x, 7, mut).reshape(B, L, 7, C)
    y = torch.einsum("bltc,ct->blc", t, dw)
    if "no_bias" not in mut:
        y = y + W[p + "dwconv.bias"]
    y = _ln(y) * W[p + "norm.scale.weight"][bw] + W[p + "norm.shift.weight"][bw]
    y = W.act8(y) if W.q8(B * L) else W.act(y)  # store_out<TO> / the fp8 branch of the same kernel
    y = W.act(_gelu(_lin(W, y, W[p + "pwconv1.weight"], W[p + "pwconv1.bias"], mut)))  # E_BIAS_GELU, TC = TAct
    y = _lin(W, y, W[p + "pwconv2.weight"], W[p + "pwconv2.bias"], mut)
    if "no_gamma" not in mut:
        y = W[p + "gamma"] * y  # E_BIAS_GAMMA_RES
    return _finish(x, y, mut)


def head(W: Weights, x, mut=NONE):
    """Stage 19: final LayerNorm (models.py:235) + ISTFTHead.out (heads.py:56). -> spec [B, L, 1282]."""
    y = W.act(_ln(x) * W["backbone.final_layer_norm.weight"] + W["backbone.final_layer_norm.bias"])
    y = _lin(W, y, W["head.out.weight"], W["head.out.bias"], mut)
    if "head_col_1281" in mut:
        y = y.clone()
        y[..., 1281] = 0
    if "head_tile" in mut:  # the last, partial 192-column tile holds the tile before it
        y = y.clone()
        y[..., 1152:] = y[..., 960:960 + 1282 - 1152]
    return _finish(None, y, mut | {"no_residual"})


def istft(spec, mut=NONE):
    """Stage 20: heads.py:57-66 + spectral_ops.py:33-75 (padding "same"). spec [B, L, 1282] -> pcm [B, 320 L].
    The same in every mode (the bf16 mode's native exp / sin / cos are arithmetic, not a rounding point)."""
    B, L, _ = spec.shape
    dt = spec.dtype
    mag = torch.clamp(torch.exp(spec[..., :NB]), max=100.0)
    ph = spec[..., NB:]
    re, im = mag * torch.cos(ph), mag * torch.sin(ph)
    n = torch.arange(NFFT, dtype=torch.float64)
    k = torch.arange(NB, dtype=torch.float64)
    ang = 2.0 * math.pi * torch.outer(k, n) / NFFT  # exact in fp64: the C2R as two real matrix products
    wk = torch.full((NB, 1), 2.0, dtype=torch.float64)
    wk[0] = wk[NB - 1] = 1.0
    cosm = (wk * torch.cos(ang) / NFFT).to(dt)
    sinm = (wk * torch.sin(ang) / NFFT).to(dt)
    sinm[0] = 0  # the C2R ignores the imaginary parts of DC and Nyquist (istft_frames_kernel: x.y = 0.f)
    sinm[NB - 1] = 0
    fr = re @ cosm - im @ sinm  # [B, L, 1280]
    if "istft_dc_imag" in mut:
        # the packed 640-point transform with X[0].y / X[640].y left in: Z[0] moves by
        # (-(a + n) / 2, (a - n) / 2), i.e. the even / odd samples by those over 640
        a, nq = im[..., 0:1], im[..., NB - 1:NB]
        fr = fr.clone()
        fr[..., 0::2] += -(a + nq) / 2 / 640
        fr[..., 1::2] += (a - nq) / 2 / 640
    win = torch.hann_window(NFFT).to(dt)  # the fp32 table the engine uploads (spectral_ops.py:30-31)
    fr = fr * win
    pad = (NFFT - HOP) // 2
    size = (L - 1) * HOP + NFFT
    y = torch.zeros(B, size, dtype=dt)
    env = torch.zeros(size + 2 * HOP, dtype=dt)
    for f in range(L):
        y[:, f * HOP:f * HOP + NFFT] += fr[:, f]
    for f in range(-1, L + 1) if "ola_env_shift" in mut else range(L):
        env[(f + 1) * HOP:(f + 1) * HOP + NFFT] += win * win
    env = env[HOP:HOP + size]
    if "ola_env_shift" in mut:  # one frame too many at the first and the last hop only
        good = torch.zeros(size, dtype=dt)
        for f in range(L):
            good[f * HOP:f * HOP + NFFT] += win * win
        good[pad:pad + HOP] = env[pad:pad + HOP]
        good[size - pad - HOP:size - pad] = env[size - pad - HOP:size - pad]
        env = good
    return (y / env)[:, pad:size - pad]


def stage(W: Weights, st: int, x, bw: int = 0, mut=NONE, widx: Optional[int] = None):
    """(out, compared) of stage ``st`` on its input: the codes [B, L] for 0, x [B, L, 768] for 1 .. 19, the
    spectrum [B, L, 1282] for 20. ``compared`` is what a test compares: the branch for the stages with a
    residual, the output for the others. ``widx``: the block whose weights are used (default: the stage's)."""
    mut = frozenset(mut)
    if st == 0:
        return embed(W, x, mut)
    if st in RESNET_OF_STAGE:
        return resnet(W, RESNET_OF_STAGE[st] if widx is None else widx, x, mut)
    if st == 3:
        return attn(W, x, mut)
    if st == 6:
        return gn_adaln(W, x, bw, mut)
    if 7 <= st <= 18:
        return convnext(W, st - 7 if widx is None else widx, x, bw, mut)
    if st == 19:
        return head(W, x, mut)
    if st == 20:
        y = istft(x, mut)
        return y, y
    raise ValueError(st)


# ---------------------------------------------------------------------------
# inputs that make indexing errors large
# ---------------------------------------------------------------------------

def _seed(*key) -> int:
    return zlib.crc32(repr(key).encode())


def make_x(B: int, L: int, seed: int = 0) -> torch.Tensor:
    """Unit-scale residual stream [B, L, 768] (fp32 values in fp64): every stream with its own offset and
    gain (a GroupNorm taking another stream's statistics shows); the first and last two frames of every
    stream and the last row of the call raised 8x in a seeded third of the channels (conv padding, windows
    crossing a stream boundary inside a tile and the last row of a partial tile all carry weight)."""
    g = np.random.default_rng(_seed("x", B, L, seed))
    x = g.standard_normal((B, L, CD))
    gain = 0.6 + 0.8 * g.random(B)
    off = 0.5 * g.standard_normal(B)
    x = x * gain[:, None, None] + off[:, None, None]
    hot = g.random(CD) < 1.0 / 3.0
    for t in sorted({0, min(1, L - 1), max(L - 2, 0), L - 1}):
        x[:, t, hot] *= 8.0
    x[B - 1, L - 1, hot] *= 1.5  # the very last row differs from the other streams' last rows
    return torch.from_numpy(x.astype(np.float32)).to(torch.float64)


def make_codes(B: int, L: int, seed: int = 0) -> torch.Tensor:
    g = np.random.default_rng(_seed("codes", B, L, seed))
    return torch.from_numpy(g.integers(0, 4096, (B, L)))


def make_spec(B: int, L: int, seed: int = 0, phase: float = 16.0) -> torch.Tensor:
    """Synthetic head output [B, L, 1282]: log-magnitudes uniform in [-8, 6] (crossing the clip at ln 100),
    phases uniform in +-phase; the first / middle / last frame of every stream with all energy in bin 0, bin
    640 and one mid bin, imaginary parts present (phases kept) that the C2R must ignore at DC and Nyquist."""
    g = np.random.default_rng(_seed("spec", B, L, seed))
    s = np.empty((B, L, 2 * NB))
    s[..., :NB] = g.uniform(-8.0, 6.0, (B, L, NB))
    s[..., NB:] = g.uniform(-phase, phase, (B, L, NB))
    for t in sorted({0, L // 2, L - 1}):
        s[:, t, :NB] = -8.0
        for kbin in (0, NB - 1, 257):
            s[:, t, kbin] = 5.5
        s[:, t, NB] = 0.9 + 0.1 * t  # sin far from 0: an un-ignored imaginary part is large
        s[:, t, 2 * NB - 1] = -1.1
    return torch.from_numpy(s.astype(np.float32)).to(torch.float64)


def make_input(st: int, B: int, L: int, seed: int = 0):
    return make_codes(B, L, seed) if st == 0 else make_spec(B, L, seed) if st == 20 else make_x(B, L, seed)


def rel_err(got, ref) -> float:
    """RMS of (got - ref) over the call, relative to the RMS of ref; both taken in fp64."""
    got, ref = got.to(torch.float64), ref.to(torch.float64)
    return float(torch.sqrt(((got - ref) ** 2).mean()) / torch.sqrt((ref ** 2).mean()))


def compared(st: int, out, x_in):
    """The compared quantity of a device (or fp32) output: out - x_in for stages with a residual."""
    out = out.to(torch.float64)
    return out - x_in.to(torch.float64) if KINDS[st] in HAS_RESIDUAL else out


def yardstick(cw, mode: str, st: int, B: int, L: int, bw: int = 0, seed: int = 0, w64=None, w32=None) -> float:
    """Branch-relative deviation of the mode's model evaluated in fp32 from the same model in fp64."""
    w64 = w64 or Weights(cw, mode, torch.float64)
    w32 = w32 or Weights(cw, mode, torch.float32)
    x = make_input(st, B, L, seed)
    _, ref = stage(w64, st, x, bw)
    x32 = x if st == 0 else x.to(torch.float32)
    out32, _ = stage(w32, st, x32, bw)
    return rel_err(compared(st, out32, x) if st else out32, ref)


# ---------------------------------------------------------------------------
# the cells of tests/test_gpu_codec_stages.py (shape -> stages), shared with the yardsticks below
# ---------------------------------------------------------------------------

ALL_STAGES = tuple(range(N_STAGES))
CELLS_ALL = ((1, 1), (3, 5), (2, 9), (3, 43), (1, 385))              # all 21 stages, bf16 and fp32
CELLS_GN = ((1, 341), (1, 342), (1, 512), (1, 513))                  # stages 1, 3, 6, both modes
GN_STAGES = (1, 3, 6)
FORCED_STAGES = (0, 1, 3, 7, 19)                                     # forced families at (3, 5), (3, 43), bf16
CELLS_GLDS = (((3, 641), (3, 7)), ((7, 495), (19,)), ((7, 860), (0, 1, 3, 7)), ((11, 746), (7,)))


FP8_STAGES = (0, 1, 7, 19)
CELLS_FP8 = (((3, 5), FP8_STAGES), ((3, 43), FP8_STAGES), ((3, 641), (7,)))  # codec_dtype fp8; 3 x 641: W8A8 and W8A16


def cell_bw(B: int, L: int) -> int:
    """bandwidth_id of a cell: 0 or 3, fixed by the shape (both occur among the cells of every stage kind
    that reads it)."""
    return 3 if (B + L) % 2 else 0


def all_cells(mode="bf16"):
    """Every (stage, B, L) the GPU test runs in a mode (the option variants of a cell share its reference)."""
    if mode == "fp8":
        return [(st, B, L) for (B, L), sts in CELLS_FP8 for st in sts]
    out = [(st, B, L) for B, L in CELLS_ALL for st in ALL_STAGES]
    out += [(st, B, L) for B, L in CELLS_GN for st in GN_STAGES]
    out += [(st, B, L) for (B, L), sts in CELLS_GLDS for st in sts]
    return out


# Largest branch-relative deviation, over all_cells() of a stage kind, of the mode's model evaluated in fp32
# on the CPU from the same model in fp64 (``yardstick``; `python -m tests.codec_ref` prints the table: it
# was run once and the figures copied here, rounded up to two digits). It holds summation-order noise
# and, in bf16, the double-rounding flips (an fp32 value on the other side of a bf16 tie than its fp64
# value), which the device shows too. The figures depend on the host's BLAS (blocking, threads) by a factor
# of up to about 2; tests/test_codec_ref.py recomputes the fp32 mode's small cells and holds them to half the
# device bound.
YARDSTICK = {
    ("embed", "fp32"): 3.5e-07,     # stage 0 at (2, 9)
    ("resnet", "fp32"): 2.8e-06,    # stage 1 at (7, 860)
    ("attn", "fp32"): 4.6e-06,      # stage 3 at (7, 860)
    ("gn_adaln", "fp32"): 2.0e-07,  # stage 6 at (1, 341)
    ("convnext", "fp32"): 9.7e-06,  # stage 17 at (1, 1): the residual add's rounding, 2^-24 |x| against a branch of 0.03 |x|
    ("head", "fp32"): 7.2e-07,      # stage 19 at (7, 495)
    ("istft", "fp32"): 3.5e-07,     # stage 20 at (1, 1)
    ("embed", "bf16"): 1.6e-07,     # stage 0 at (7, 860): bf16 operands, no flips (the codebook rows round the same way)
    ("resnet", "bf16"): 2.0e-04,    # stage 2 at (3, 5)
    ("attn", "bf16"): 3.2e-04,      # stage 3 at (7, 860)
    ("gn_adaln", "bf16"): 2.0e-07,  # stage 6 at (1, 341) (fp32 in every mode)
    ("convnext", "bf16"): 3.1e-04,  # stage 17 at (2, 9)
    ("head", "bf16"): 5.2e-05,      # stage 19 at (3, 43)
    ("istft", "bf16"): 3.5e-07,     # stage 20 at (1, 1) (the same arithmetic in every mode)
    ("embed", "fp8"): 2.8e-07,      # stage 0 at (3, 43) (over all_cells("fp8"))
    ("resnet", "fp8"): 1.9e-05,     # stage 1 at (3, 43)
    ("convnext", "fp8"): 1.2e-04,   # stage 7 at (3, 641), W8A8
    ("head", "fp8"): 5.2e-05,       # stage 19 at (3, 43)
}
MARGIN = 8.0  # device bound = MARGIN x yardstick: another summation order, its own gelu_erf / expf, and in
              # the bf16 iSTFT the native transcendentals


def bound(st: int, mode: str) -> float:
    return MARGIN * YARDSTICK[(KINDS[st], mode)]


if __name__ == "__main__":
    import sys
    sys.path.insert(0, ".")
    from llmvox_amd import weights as LW
    cw = LW.synthetic_codec(1234)
    for mode in ("fp32", "bf16", "fp8"):
        w64, w32 = Weights(cw, mode, torch.float64), Weights(cw, mode, torch.float32)
        worst = {}
        for a8 in ((True, False) if mode == "fp8" else (True,)):
            w64.w8a8 = w32.w8a8 = a8
            for st, B, L in all_cells(mode):
                y = yardstick(cw, mode, st, B, L, cell_bw(B, L), w64=w64, w32=w32)
                k = KINDS[st]
                if y > worst.get(k, (0.0,))[0]:
                    worst[k] = (y, st, B, L)
        for k, v in worst.items():
            print(f'    ("{k}", "{mode}"): {v[0]:.3e},  # stage {v[1]} at ({v[2]}, {v[3]})', flush=True)
