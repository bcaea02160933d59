"""fp64 reference of the WavTokenizer encoder, one function per stage of ``lvx_enc_stages``.

TEST INFRASTRUCTURE ONLY. The formulas are those ``oracle/reference_cpu.py`` cites for encode_infer
(encoder/modules/seanet.py:94-143, conv.py:54-96,195-211, lstm.py:31-39, quantization/core_vq.py:171-183), written
out so that they run in any dtype: the SConv1d padding as index arithmetic (``tap_index``), an LSTM cell of
its own in aten's order, the quantiser as -((|x|^2 - 2 x.e) + |e|^2) with the first index on ties.

Every function takes its dtype from ``Weights`` (torch.float64: the reference; torch.float32: the same model
evaluated in single precision, the yardstick of the device bounds) and ``mut``, a set of named mutations (the
indexing and omission errors ``tests/test_enc_ref.py`` proves the comparison sensitive to).

Layout: activations are [B, L, C] (time-major, as on the device); the audio is [B, L].
"""
from __future__ import annotations

import functools
import zlib

import numpy as np
import torch

ENC_PREFIX = "feature_extractor.encodec.encoder.model."
N_STAGES = 12
RATIOS = (2, 4, 5, 8)
NONE = frozenset()

# stage -> kind; a residual block / down conv of ratio r is stage 1 + 2 i / 2 + 2 i for r = RATIOS[i]
KINDS = {0: "conv0", 9: "lstm", 10: "conv15", 11: "vq"}
KINDS.update({s: "resblock" for s in (1, 3, 5, 7)})
KINDS.update({s: "down" for s in (2, 4, 6, 8)})
CONV_STAGES = tuple(range(9)) + (10,)

MUT_CONV = ("reflect_left", "reflect_right", "no_extra_right", "no_zero_ext", "no_elu", "no_residual", "drop_tap",
            "drop_k16")
MUT_LSTM = ("gate_order", "no_c_carry", "h_prev2", "h_next_stream", "h_stream_m16", "no_skip", "no_bhh")


def stage_ratio(st: int) -> int:
    return RATIOS[(st - 1) // 2]


def stage_cin(st: int) -> int:
    """channels of the input of stage st (0: the audio, one channel)"""
    return 1 if st == 0 else 512 if st >= 9 else 32 << ((st - 1) // 2)


class Weights:
    """The encoder's effective state dict (llmvox_amd.weights.encoder_effective: weight_norm resolved) and the
    codebook in ``dt``; conv weights tap-major [cout][k * cin], as the gathered operand of ``_conv``."""

    def __init__(self, we, codebook, dt=torch.float64):
        self.dt = dt
        self.w = {k: torch.from_numpy(np.ascontiguousarray(np.asarray(v, dtype=np.float32))).to(dt)
                  for k, v in we.items() if k.startswith(ENC_PREFIX)}
        self.cb = torch.from_numpy(np.ascontiguousarray(np.asarray(codebook, dtype=np.float32))).to(dt)

    def conv(self, name):
        w = self.w[ENC_PREFIX + name + ".conv.conv.weight"]  # [cout][cin][k]
        return w.permute(0, 2, 1).reshape(w.shape[0], -1), self.w[ENC_PREFIX + name + ".conv.conv.bias"], w.shape[2]

    def lstm(self, layer: int):
        p = ENC_PREFIX + "13.lstm."
        return tuple(self.w[p + f"{n}_l{layer}"] for n in ("weight_ih", "bias_ih", "weight_hh", "bias_hh"))


# ---------------------------------------------------------------------------
# SConv1d
# ---------------------------------------------------------------------------

def conv_geo(L: int, k: int, stride: int):
    """SConv1d geometry (conv.py:54-61, 79-96, 195-211; dilation 1): padding_total = k - stride split
    right-heavy-last, the extra right padding that makes the last window full, the zero extension of an input
    no longer than the larger pad. -> dict(pl, pr, extra, right, ex0, T)."""
    pt = k - stride
    nf = -(-L // stride)
    extra = nf * stride - L
    pr = pt // 2
    pl = pt - pr
    right = pr + extra
    max_pad = max(pl, right)
    ex0 = max_pad - L + 1 if L <= max_pad else 0
    return dict(pl=pl, pr=pr, extra=extra, right=right, max_pad=max_pad, ex0=ex0, T=(pl + L + right - k) // stride + 1)


def tap_index(L: int, k: int, stride: int, mut=NONE) -> torch.Tensor:
    """[T][k]: the input frame that tap j of output frame t reads, L for a zero (the zero extension's frames).
    The padded signal is reflect(x + ex0 zeros, (pl, right)) without its last ex0 frames: position p of it is
    index i = p - pl of the extended signal, reflected once at either end."""
    g = conv_geo(L, k, stride)
    lext = L + (0 if "no_zero_ext" in mut else g["ex0"])
    i = torch.arange(g["T"])[:, None] * stride + torch.arange(k)[None, :] - g["pl"]
    dropped = i >= L + g["pr"]  # the extra right padding's frames
    i = torch.where(i < 0, -i - (1 if "reflect_left" in mut else 0), i)
    i = torch.where(i >= lext, 2 * (lext - 1) - i + (1 if "reflect_right" in mut else 0), i)
    if "no_zero_ext" in mut:
        i = i.clamp(0, L - 1)  # (the reference would refuse the pad; an unextended kernel reads what is there)
    i = torch.where(i >= L, torch.full_like(i, L), i)
    if "no_extra_right" in mut:
        i = torch.where(dropped, torch.full_like(i, L), i)
    return i


def _elu(x):
    return torch.where(x > 0, x, torch.expm1(x))


def _conv(W: Weights, name: str, x, stride=1, elu=False, mut=NONE):
    """[ELU ->] SConv1d ``name`` on x [B, L, cin] -> [B, T, cout]: gather the taps, one matrix product, bias."""
    w, b, k = W.conv(name)
    B, L, C = x.shape
    if elu and "no_elu" not in mut:
        x = _elu(x)
    idx = tap_index(L, k, stride, mut)
    xz = torch.cat([x, x.new_zeros(B, 1, C)], dim=1)
    a = xz[:, idx.reshape(-1)].reshape(B, idx.shape[0], k, C)
    pl = conv_geo(L, k, stride)["pl"]  # the tap that reads frame t * stride itself: never padding
    if "drop_tap" in mut and k > 1:
        a = a.clone()
        a[:, :, pl] = 0
    if "drop_k16" in mut:  # one K chunk of the device's loop: 16 channels of one tap
        a = a.clone()
        a[:, :, pl, max(C - 16, 0):] = 0
    return a.reshape(B, idx.shape[0], k * C) @ w.t() + b


def conv0(W, audio, mut=NONE):
    """Stage 0: conv "0" (k7, 1 -> 32). audio [B, L] -> [B, L, 32]."""
    y = _conv(W, "0", audio.unsqueeze(-1), mut=mut)
    return y, y


def shortcut(W, st: int, x):
    return _conv(W, f"{1 + 3 * ((st - 1) // 2)}.shortcut", x)


def resblock(W, st: int, x, mut=NONE):
    """Stages 1, 3, 5, 7 (seanet.py:36-64): shortcut(x) + block.3(ELU block.1(ELU x)). -> (out, branch)."""
    idx = 1 + 3 * ((st - 1) // 2)
    h = _conv(W, f"{idx}.block.1", x, elu=True, mut=mut)
    h = _conv(W, f"{idx}.block.3", h, elu=True, mut=mut)
    sc = _conv(W, f"{idx}.shortcut", x, mut=mut)
    return (h if "no_residual" in mut else sc + h), h


def down(W, st: int, x, mut=NONE):
    """Stages 2, 4, 6, 8: ELU + the strided conv of ratio r (k = 2 r). [B, L, d] -> [B, ceil(L / r), 2 d]."""
    r = stage_ratio(st)
    y = _conv(W, f"{3 * (st // 2)}", x, stride=r, elu=True, mut=mut)
    return y, y


def conv15(W, x, mut=NONE):
    """Stage 10: ELU + conv "15" (k7, 512 -> 512)."""
    y = _conv(W, "15", x, elu=True, mut=mut)
    return y, y


# ---------------------------------------------------------------------------
# SLSTM
# ---------------------------------------------------------------------------

def lstm_layer(W, layer: int, x, mut=NONE, gates_out=None):
    """One nn.LSTM layer over x [B, T, 512] from zero state, aten's LSTMCell order: gates = (h W_hh^T + b_hh) +
    (x W_ih^T + b_ih), chunks i, f, g, o; c' = f c + i g; h' = o tanh(c')."""
    wih, bih, whh, bhh = W.lstm(layer)
    B, T, H = x.shape
    gin = x @ wih.t() + bih
    h = x.new_zeros(B, H)
    c = x.new_zeros(B, H)
    hist = [h, h]  # h_{t-2}, h_{t-1}
    ys = []
    for t in range(T):
        hp = hist[0] if "h_prev2" in mut else hist[1]
        if "h_next_stream" in mut:
            hp = hp.roll(-1, 0)
        if "h_stream_m16" in mut:
            hp = hp.roll(16, 0)
        rec = hp @ whh.t()
        if "no_bhh" not in mut:
            rec = rec + bhh
        gates = rec + gin[:, t]
        if gates_out is not None:
            gates_out.append(gates)
        gi, gf, gg, go = gates.split(H, dim=1)
        if "gate_order" in mut:
            gf, gg = gg, gf
        i, f, g, o = torch.sigmoid(gi), torch.sigmoid(gf), torch.tanh(gg), torch.sigmoid(go)
        c = i * g if "no_c_carry" in mut else f * c + i * g
        h = o * torch.tanh(c)
        hist = [hist[1], h]
        ys.append(h)
    return torch.stack(ys, dim=1)


def slstm(W, x, mut=NONE):
    """Stage 9 (lstm.py:31-39): the two layers, + the input. -> (out, branch = layer 1's h)."""
    y = lstm_layer(W, 1, lstm_layer(W, 0, x, mut), mut)
    return (y if "no_skip" in mut else y + x), y


def lstm_gates0(W, x):
    """every layer-0 gate pre-activation [B, T, 2048]"""
    g = []
    lstm_layer(W, 0, x, gates_out=g)
    return torch.stack(g, dim=1)


# ---------------------------------------------------------------------------
# quantiser
# ---------------------------------------------------------------------------

def vq(W, x):
    """Stage 11 (core_vq.py:175-183). x [B, T, 512] -> dict(codes int64 [B, T] (first index on ties), scores x . e
    [B, T, 4096], dist, gap best - runner-up [B, T], features [B, 512, T])."""
    # row by row, each code's sum taken by the same reduction whatever its index: equal codebook rows tie exactly
    # (a BLAS product may sum the columns of an edge tile in another order than the others)
    s = torch.stack([(W.cb * r).sum(-1) for r in x.reshape(-1, x.shape[-1])]).reshape(*x.shape[:-1], -1)
    dist =-(((x * x).sum(-1, keepdim=True) - 2 * s) + (W.cb * W.cb).sum(-1))
    codes = torch.from_numpy(np.argmax(dist.numpy(), axis=-1))  # numpy: the first occurrence
    top = torch.topk(dist, 2, dim=-1).values
    return dict(codes=codes, scores=s, dist=dist, gap=top[..., 0] - top[..., 1],
                features=W.cb[codes].permute(0, 2, 1))


def stage(W, st: int, x, mut=NONE):
    """(out, compared) of a stage < 11 on its input. ``compared``: the branch for the stages with a residual or
    skip, the output for the others."""
    mut = frozenset(mut)
    k = KINDS[st]
    if k == "conv0":
        return conv0(W, x, mut)
    if k == "resblock":
        return resblock(W, st, x, mut)
    if k == "down":
        return down(W, st, x, mut)
    if k == "lstm":
        return slstm(W, x, mut)
    if k == "conv15":
        return conv15(W, x, mut)
    raise ValueError(st)


def chain(W, audio):
    """audio [B, N] -> the embedding [B, T, 512] (stages 0 .. 10)."""
    x = audio
    for st in range(11):
        x = stage(W, st, x)[0]
    return x


# ---------------------------------------------------------------------------
# inputs, comparison, yardstick
# ---------------------------------------------------------------------------

def _seed(*key) -> int:
    return zlib.crc32(repr(key).encode())


# RMS of the SLSTM's input in the real chain: 0.43 .. 0.46 over the streams of the golden case 3x4800, 0.36 .. 0.48
# over the edge case 33x961 (stage 8's output under the synthetic weights; tests/test_enc_ref.py recomputes it)
LSTM_IN_RMS = 0.44


def make_x(st: int, B: int, L: int, seed: int = 0, scale: float = None) -> torch.Tensor:
    """Seeded input of stage st (fp32 values in fp64): every stream with its own gain and offset (a stream taking
    another's frames or state shows), the first and last two frames of every stream raised 4x in a seeded third
    of the channels (the padding's reads carry weight), the last row of the call different again. Unit scale
    (the audio: 0.3); the SLSTM's input has RMS LSTM_IN_RMS over the call; ``scale`` multiplies either."""
    C = stage_cin(st)
    g = np.random.default_rng(_seed("enc", st, B, L, seed))
    x = g.standard_normal((B, L, C))
    x = x * (0.6 + 0.8 * g.random(B))[:, None, None] + (0.3 * g.standard_normal(B))[:, None, None]
    hot = g.random(C) < 1.0 / 3.0 if C > 1 else np.ones(1, bool)
    for t in sorted({0, min(1, L - 1), max(L - 2, 0), L - 1}):
        x[:, t, hot] *= 4.0 if C > 1 else 2.0
    x[B - 1, L - 1, hot] *= 1.5
    x *= 0.3 if st == 0 else LSTM_IN_RMS / np.sqrt(np.mean(x * x)) if st == 9 else 1.0
    x *= 1.0 if scale is None else scale
    x = torch.from_numpy(x.astype(np.float32)).to(torch.float64)
    return x[..., 0] if st == 0 else x


def rel_err(got, ref) -> float:
    """RMS of (got - ref) over the call, relative to the RMS of ref; both taken in fp64."""
    got, ref = got.to(torch.float64), ref.to(torch.float64)
    return float(torch.sqrt(((got - ref) ** 2).mean()) / torch.sqrt((ref ** 2).mean()))


def compared(W64, st: int, out, x):
    """The compared quantity of a device (or fp32) output of stage st on the fp64 input x: out - x for the SLSTM,
    out - shortcut(x) (the fp64 model's) for the residual blocks, out for the others."""
    out = out.to(torch.float64)
    k = KINDS[st]
    return out - x if k == "lstm" else out - shortcut(W64, st, x) if k == "resblock" else out


MARGIN = 8.0  # device bound = MARGIN x yardstick, codec_ref's figure for its exact-fp32 cells by the same argument:
              # the same products in another summation order, and the device's own expm1f / expf / tanhf


def YARDSTICK(W64, W32, kind, x) -> float:
    """The deviation of the model evaluated in fp32 on the CPU from itself in fp64 on a cell's own input, in the
    cell's compared quantity relative to the fp64 one's RMS. ``kind``: a stage 0 .. 10, "vq" / 11 (the scores), or
    "chain" (stages 0 .. 10 on audio). Nothing a device computed enters it."""
    x32 = x.to(torch.float32)
    if kind == "chain":
        return rel_err(chain(W32, x32), chain(W64, x))
    if kind in ("vq", 11):
        return rel_err(x32 @ W32.cb.t(), x @ W64.cb.t())
    out32, _ = stage(W32, kind, x32)
    return rel_err(compared(W64, kind, out32, x), stage(W64, kind, x)[1])


@functools.lru_cache(maxsize=None)
def load_weights():
    """(W64, W32, codebook fp32 numpy) of the synthetic encoder, seed 1234"""
    from llmvox_amd import weights as LW
    we = LW.encoder_effective(LW.synthetic_encoder(1234))
    cb = LW.synthetic_codec(1234)[LW.CODEBOOK_KEY]
    return Weights(we, cb, torch.float64), Weights(we, cb, torch.float32), cb


# ---------------------------------------------------------------------------
# the cells of tests/test_gpu_encoder_stages.py
# ---------------------------------------------------------------------------

def zero_extended_L(r: int):
    """the largest L > 1 at which the strided conv of ratio r zero-extends its input, or None"""
    ls = [L for L in range(2, 2 * r + 2) if conv_geo(L, 2 * r, r)["ex0"]]
    return max(ls) if ls else None


def conv_cells():
    """(stage, B, L) of every conv cell: (1, 1) and (3, 43) at every stage; stage 0 at L = 3, 4 (either side of
    the k7 pad); every strided stage of ratio r at B = 2 with L = r - 1, r, r + 1, 2 r + 1 and the largest L > 1
    that is still zero-extended (r = 4, 5, 8: 5, 6, 10; at r = 2 only L = 1 is)."""
    out = [(st, B, L) for st in CONV_STAGES for B, L in ((1, 1), (3, 43))]
    out += [(0, 2, 3), (0, 2, 4)]
    for st in (2, 4, 6, 8):
        r = stage_ratio(st)
        ls = [r - 1, r, r + 1, 2 * r + 1]
        z = zero_extended_L(r)
        if z is not None and z not in ls:
            ls.append(z)
        out += [(st, 2, L) for L in ls]
    return out


LSTM_CELLS = ((1, 1), (3, 5), (16, 2), (17, 3), (33, 2))
HOT_CELL = (17, 3)
HOT_GATE = 90.0


def hot_input():
    """The hot SLSTM cell's input: make_x at the smallest amplitude (LSTM_IN_RMS times a power of two) at which,
    by the fp64 model, layer-0 gates pass +HOT_GATE and -HOT_GATE (expf(-gate) overflows fp32 above 88.7)."""
    W64 = load_weights()[0]
    B, T = HOT_CELL
    base = make_x(9, B, T, seed=7)
    a = 1.0
    while True:
        g = lstm_gates0(W64, base * a)
        if float(g.max()) > HOT_GATE and float(g.min()) < -HOT_GATE:
            return base * a
        a *= 2.0


VQ_CELLS = ((1, 1), (3, 5), (17, 2))
VQ_WINNERS = (0, 255, 256, 4095)


def vq_input(codebook, B: int, T: int, seed: int = 0):
    """Constructed winners: frame m is codebook row n_m + N(0, 0.05^2) noise (the rows are N(0, 1): the runner-up is
    ~1,000 behind). The first frames take VQ_WINNERS in turn, the others seeded rows. -> (x fp64 [B, T, 512], n)."""
    g = np.random.default_rng(_seed("vq", B, T, seed))
    n = g.integers(0, 4096, B * T)
    for j in range(min(B * T, len(VQ_WINNERS))):
        n[j] = VQ_WINNERS[(j + seed) % len(VQ_WINNERS)]
    x = np.asarray(codebook, np.float32)[n] + 0.05 * g.standard_normal((B * T, 512)).astype(np.float32)
    return torch.from_numpy(x.astype(np.float32)).to(torch.float64).reshape(B, T, 512), n.reshape(B, T)


# copied codebook rows (source -> copies) of the tie context: neighbouring lanes; wave 0 vs wave 1 (74 = 10 + 64);
# the same thread's next round (266 = 10 + 256); the first and the last row; a triple; a pair inside wave 3
# (thread 200 and 230 of 256: rows 200 + 256 k, 230 + 256 k)
TIE_SETS = ((10, 11, 74, 266), (0, 4095), (300, 301, 2000), (712, 742))


def tie_codebook(codebook):
    cb = np.array(codebook, dtype=np.float32, copy=True)
    for s in TIE_SETS:
        cb[list(s[1:])] = cb[s[0]]
    return cb
