"""Every stage of the codec decode, and every kernel family its GEMMs route to, against the fp64 model of
tests/codec_ref.py, through the test hook lvx_codec_stages (a window of one stage on a given input).

A stage with a residual is compared on its branch, out - x_in, relative to the reference branch's RMS
over the call (the residual stream would hide a branch error 40-fold); the others on their output. The
bound of a (stage kind, mode) is codec_ref.MARGIN x the deviation of the mode's model evaluated in fp32
on the CPU from itself in fp64 (codec_ref.YARDSTICK: nothing the device computed enters it), and
tests/test_codec_ref.py shows every indexing / omission error moving the compared quantity by >= 10x it.

Every cell also asserts the route records of its GEMMs (ROUTES below: kernel family, K splits, in-launch
combine, tile / stage variant), so a changed threshold cannot move a cell off the kernel it is here for.

MEASURED collects the largest device error per (stage kind, config) and is printed at the end of the
module (the figures in DESIGN.md section 2, "The codec decode stage by stage").
"""
import pytest
import torch

from tests import codec_ref as CR

pytestmark = pytest.mark.gpu

MAX_FRAMES = 11 * 746  # the largest cell
DEFAULT_OPTS = {"codec_skinny": 1, "codec_g2": 1, "codec_g3": 1, "codec_g3f": 2, "codec_exp": 0}
# config -> (engine mode, options, the reference's codec_g3f)
CONFIGS = {
    "bf16": ("bf16", {}, 2),
    "fp32": ("fp32", {}, 2),
    "bf16-noskinny": ("bf16", {"codec_skinny": 0}, 2),                  # 64 x 64 / 128 x 128 bf16 MFMA at small M
    "bf16-mfma64": ("bf16", {"codec_skinny": 0, "codec_g2": 0}, 2),     # 64 x 64 at every GEMM
    "fp32-g3f1": ("fp32", {"codec_g3f": 1}, 1),                         # exact-fp32 products on the LDS-DMA kernel
    "fp32-exp16": ("fp32", {"codec_exp": 16}, 2),                       # bf16x3, operands split in registers
    "fp8": ("fp8", {}, 2),                                              # codec_dtype fp8: W8A16, pwconv1 W8A8 at large M
    "fp8-exp32": ("fp8", {"codec_exp": 32}, 32),                        # W8A16 at every GEMM
}


def _cells():
    out = []
    for cfg in ("bf16", "fp32"):
        out += [(cfg, st, B, L) for B, L in CR.CELLS_ALL for st in CR.ALL_STAGES]
        out += [(cfg, st, B, L) for B, L in CR.CELLS_GN for st in CR.GN_STAGES]
    out += [("bf16-noskinny", st, B, L) for B, L in ((3, 5), (3, 43)) for st in CR.FORCED_STAGES]
    out += [("bf16-mfma64", st, 3, 43) for st in CR.FORCED_STAGES]
    for cfg in ("bf16", "fp32", "fp32-g3f1", "fp32-exp16"):
        out += [(cfg, st, B, L) for (B, L), sts in CR.CELLS_GLDS for st in sts]
    out += [("fp8", st, B, L) for (B, L), sts in CR.CELLS_FP8 for st in sts]
    out += [("fp8-exp32", 7, 3, 641)]
    return out


CELLS = _cells()

# ---- expected routes -------------------------------------------------------------------------------
# One record per GEMM of the stage, in launch order: (family, ksplit, inlaunch, v0, v1, v2, N, K).
#   MF(ks, inl, bf, batch, kf): gemm_mfma_kernel 64 x 64      B2(ks, wbytes): gemm_bf16_kernel 128 x 128
#   G3(ns, split, abytes): gemm_glds_kernel 128 x 192         SK(mi, nj, nwv): gemm_skinny_kernel
M64, B128, GLDS, SKINNY = 0, 1, 2, 3
# the GEMMs of a stage: (N, K); None: the attention's scores / P.V (N and K follow L)
STAGE_GEMMS = {"embed": ((768, 3584),), "resnet": ((768, 2304), (768, 2304)),
               "attn": ((2304, 768), None, None, (768, 768)), "gn_adaln": (), "convnext": ((2304, 768), (768, 2304)),
               "head": ((1282, 768),), "istft": ()}


def MF(ks, inl, bf, batch=1, kf=1):
    return (M64, ks, inl, bf, batch, kf)


def B2(ks, wbytes=2):
    return (B128, ks, 0, 2, wbytes, 0)


def G3(ns, split, abytes):
    return (GLDS, 1, 0, ns, split, abytes)


def SK(mi, nj, nwv):
    return (SKINNY, 1, 0, mi, nj, nwv)


# (config, (B, L)) -> stage kind -> routes of the kind's GEMMs, in launch order (attn: qkv, scores, P.V,
# proj_out; convnext: pwconv1, pwconv2). What each shape is here for:
#   bf16 (1, 1), (3, 5): skinny 16 x 16 (8 waves for K > 1,024, else 4); (2, 9): skinny 32 x 16; (3, 43): skinny
#     32 x 32; (1, 385): past SKINNY_MAX_M, the 128 x 128 kernel with split-K; the attention's scores / P.V on
#     the 64 x 64 kernel (in-launch combine only at batch 1 and M <= 16; P.V with K % 32 != 0: KF = 0)
#   fp32 small cells: the exact-fp32 64 x 64 kernel, in-launch combine at M <= 16, a reduce kernel above
#   (3, 641), (7, 495), (7, 860), (11, 746): the LDS-DMA kernel at >= 192 tiles of 128 x 192 (NS 3; NS 2 above
#     256 tiles); fp32: SPLIT 3 = A as a split image, 1 = A split in registers (codec_exp 16, or an operand
#     no producer splits: proj_out's h), 7 / 5 = pwconv1 also writing C as a split image (pwconv2 split
#     too), 0 with 4-byte A = exact fp32 products (codec_g3f 1)
#   fp8: gemm_bf16_kernel<fp8_t> (1-byte W) at any M; 3 x 641: pwconv1 W8A8 on the LDS-DMA kernel (1-byte A)
ROUTES = {
    ("bf16", (1, 1)): {
        "embed": [SK(1, 1, 8)],
        "resnet": [SK(1, 1, 8), SK(1, 1, 8)],
        "attn": [SK(1, 1, 4), MF(4, 1, 1, 1, 1), MF(1, 0, 1, 1, 0), SK(1, 1, 4)],
        "convnext": [SK(1, 1, 4), SK(1, 1, 8)],
        "head": [SK(1, 1, 4)],
    },
    ("bf16", (3, 5)): {
        "embed": [SK(1, 1, 8)],
        "resnet": [SK(1, 1, 8), SK(1, 1, 8)],
        "attn": [SK(1, 1, 4), MF(4, 0, 1, 3, 1), MF(1, 0, 1, 3, 0), SK(1, 1, 4)],
        "convnext": [SK(1, 1, 4), SK(1, 1, 8)],
        "head": [SK(1, 1, 4)],
    },
    ("bf16", (2, 9)): {
        "embed": [SK(2, 1, 8)],
        "resnet": [SK(2, 1, 8), SK(2, 1, 8)],
        "attn": [SK(2, 1, 4), MF(4, 0, 1, 2, 1), MF(1, 0, 1, 2, 0), SK(2, 1, 4)],
        "convnext": [SK(2, 1, 4), SK(2, 1, 8)],
        "head": [SK(2, 1, 4)],
    },
    ("bf16", (3, 43)): {
        "embed": [SK(2, 2, 8)],
        "resnet": [SK(2, 2, 8), SK(2, 2, 8)],
        "attn": [SK(2, 2, 4), MF(4, 0, 1, 3, 1), MF(1, 0, 1, 3, 0), SK(2, 2, 4)],
        "convnext": [SK(2, 2, 4), SK(2, 2, 8)],
        "head": [SK(2, 2, 4)],
    },
    ("bf16", (1, 385)): {
        "embed": [B2(8)],
        "resnet": [B2(8), B2(8)],
        "attn": [B2(2), MF(4, 0, 1, 1, 1), MF(2, 0, 1, 1, 0), B2(2)],
        "convnext": [B2(2), B2(8)],
        "head": [B2(2)],
    },
    ("bf16", (1, 341)): {
        "resnet": [SK(2, 2, 8), SK(2, 2, 8)],
        "attn": [SK(2, 2, 4), MF(4, 0, 1, 1, 1), MF(2, 0, 1, 1, 0), SK(2, 2, 4)],
    },
    ("bf16", (1, 342)): {
        "resnet": [SK(2, 2, 8), SK(2, 2, 8)],
        "attn": [SK(2, 2, 4), MF(4, 0, 1, 1, 1), MF(2, 0, 1, 1, 0), SK(2, 2, 4)],
    },
    ("bf16", (1, 512)): {
        "resnet": [B2(8), B2(8)],
        "attn": [B2(2), MF(4, 0, 1, 1, 1), MF(2, 0, 1, 1, 1), B2(2)],
    },
    ("bf16", (1, 513)): {
        "resnet": [B2(8), B2(8)],
        "attn": [B2(2), MF(2, 0, 1, 1, 1), MF(2, 0, 1, 1, 0), B2(2)],
    },
    ("fp32", (1, 1)): {
        "embed": [MF(16, 1, 0, 1, 1)],
        "resnet": [MF(16, 1, 0, 1, 1), MF(16, 1, 0, 1, 1)],
        "attn": [MF(4, 1, 0, 1, 1), MF(4, 1, 0, 1, 1), MF(1, 0, 0, 1, 0), MF(4, 1, 0, 1, 1)],
        "convnext": [MF(4, 1, 0, 1, 1), MF(16, 1, 0, 1, 1)],
        "head": [MF(4, 1, 0, 1, 1)],
    },
    ("fp32", (3, 5)): {
        "embed": [MF(16, 1, 0, 1, 1)],
        "resnet": [MF(16, 1, 0, 1, 1), MF(16, 1, 0, 1, 1)],
        "attn": [MF(4, 1, 0, 1, 1), MF(4, 0, 0, 3, 1), MF(1, 0, 0, 3, 0), MF(4, 1, 0, 1, 1)],
        "convnext": [MF(4, 1, 0, 1, 1), MF(16, 1, 0, 1, 1)],
        "head": [MF(4, 1, 0, 1, 1)],
    },
    ("fp32", (2, 9)): {
        "embed": [MF(16, 0, 0, 1, 1)],
        "resnet": [MF(16, 0, 0, 1, 1), MF(16, 0, 0, 1, 1)],
        "attn": [MF(4, 0, 0, 1, 1), MF(4, 0, 0, 2, 1), MF(1, 0, 0, 2, 0), MF(4, 0, 0, 1, 1)],
        "convnext": [MF(4, 0, 0, 1, 1), MF(16, 0, 0, 1, 1)],
        "head": [MF(4, 0, 0, 1, 1)],
    },
    ("fp32", (3, 43)): {
        "embed": [MF(8, 0, 0, 1, 1)],
        "resnet": [MF(8, 0, 0, 1, 1), MF(8, 0, 0, 1, 1)],
        "attn": [MF(2, 0, 0, 1, 1), MF(4, 0, 0, 3, 1), MF(1, 0, 0, 3, 0), MF(4, 0, 0, 1, 1)],
        "convnext": [MF(2, 0, 0, 1, 1), MF(8, 0, 0, 1, 1)],
        "head": [MF(4, 0, 0, 1, 1)],
    },
    ("fp32", (1, 385)): {
        "embed": [MF(2, 0, 0, 1, 1)],
        "resnet": [MF(2, 0, 0, 1, 1), MF(2, 0, 0, 1, 1)],
        "attn": [MF(1, 0, 0, 1, 1), MF(4, 0, 0, 1, 1), MF(2, 0, 0, 1, 0), MF(2, 0, 0, 1, 1)],
        "convnext": [MF(1, 0, 0, 1, 1), MF(2, 0, 0, 1, 1)],
        "head": [MF(2, 0, 0, 1, 1)],
    },
    ("fp32", (1, 341)): {
        "resnet": [MF(4, 0, 0, 1, 1), MF(4, 0, 0, 1, 1)],
        "attn": [MF(1, 0, 0, 1, 1), MF(4, 0, 0, 1, 1), MF(2, 0, 0, 1, 0), MF(4, 0, 0, 1, 1)],
    },
    ("fp32", (1, 342)): {
        "resnet": [MF(4, 0, 0, 1, 1), MF(4, 0, 0, 1, 1)],
        "attn": [MF(1, 0, 0, 1, 1), MF(4, 0, 0, 1, 1), MF(2, 0, 0, 1, 0), MF(4, 0, 0, 1, 1)],
    },
    ("fp32", (1, 512)): {
        "resnet": [MF(2, 0, 0, 1, 1), MF(2, 0, 0, 1, 1)],
        "attn": [MF(1, 0, 0, 1, 1), MF(4, 0, 0, 1, 1), MF(2, 0, 0, 1, 1), MF(2, 0, 0, 1, 1)],
    },
    ("fp32", (1, 513)): {
        "resnet": [MF(2, 0, 0, 1, 1), MF(2, 0, 0, 1, 1)],
        "attn": [MF(1, 0, 0, 1, 1), MF(2, 0, 0, 1, 1), MF(2, 0, 0, 1, 0), MF(2, 0, 0, 1, 1)],
    },
    ("bf16-noskinny", (3, 5)): {
        "embed": [MF(16, 1, 1, 1, 1)],
        "resnet": [MF(16, 1, 1, 1, 1), MF(16, 1, 1, 1, 1)],
        "attn": [MF(4, 1, 1, 1, 1), MF(4, 0, 1, 3, 1), MF(1, 0, 1, 3, 0), MF(4, 1, 1, 1, 1)],
        "convnext": [MF(4, 1, 1, 1, 1), MF(16, 1, 1, 1, 1)],
        "head": [MF(4, 1, 1, 1, 1)],
    },
    ("bf16-noskinny", (3, 43)): {
        "embed": [B2(8)],
        "resnet": [B2(8), B2(8)],
        "attn": [B2(2), MF(4, 0, 1, 3, 1), MF(1, 0, 1, 3, 0), B2(2)],
        "convnext": [B2(2), B2(8)],
        "head": [B2(2)],
    },
    ("bf16-mfma64", (3, 43)): {
        "embed": [MF(8, 0, 1, 1, 1)],
        "resnet": [MF(8, 0, 1, 1, 1), MF(8, 0, 1, 1, 1)],
        "attn": [MF(2, 0, 1, 1, 1), MF(4, 0, 1, 3, 1), MF(1, 0, 1, 3, 0), MF(4, 0, 1, 1, 1)],
        "convnext": [MF(2, 0, 1, 1, 1), MF(8, 0, 1, 1, 1)],
        "head": [MF(4, 0, 1, 1, 1)],
    },
    ("bf16", (3, 641)): {
        "attn": [G3(3, 0, 2), MF(1, 0, 1, 3, 1), MF(1, 0, 1, 3, 0), B2(2)],
        "convnext": [G3(3, 0, 2), B2(4)],
    },
    ("bf16", (7, 495)): {
        "head": [G3(3, 0, 2)],
    },
    ("bf16", (7, 860)): {
        "embed": [G3(3, 0, 2)],
        "resnet": [G3(3, 0, 2), G3(3, 0, 2)],
        "attn": [G3(2, 0, 2), MF(1, 0, 1, 7, 1), MF(1, 0, 1, 7, 0), G3(3, 0, 2)],
        "convnext": [G3(2, 0, 2), G3(3, 0, 2)],
    },
    ("bf16", (11, 746)): {
        "convnext": [G3(2, 0, 2), G3(2, 0, 2)],
    },
    ("fp32", (3, 641)): {
        "attn": [G3(3, 3, 4), MF(1, 0, 0, 3, 1), MF(1, 0, 0, 3, 0), MF(1, 0, 0, 1, 1)],
        "convnext": [G3(3, 3, 4), MF(1, 0, 0, 1, 1)],
    },
    ("fp32", (7, 495)): {
        "head": [G3(3, 3, 4)],
    },
    ("fp32", (7, 860)): {
        "embed": [G3(3, 3, 4)],
        "resnet": [G3(3, 3, 4), G3(3, 3, 4)],
        "attn": [G3(2, 3, 4), MF(1, 0, 0, 7, 1), MF(1, 0, 0, 7, 0), G3(3, 1, 4)],
        "convnext": [G3(2, 7, 4), G3(3, 3, 4)],
    },
    ("fp32", (11, 746)): {
        "convnext": [G3(2, 7, 4), G3(2, 3, 4)],
    },
    ("fp32-g3f1", (3, 641)): {
        "attn": [G3(3, 0, 4), MF(1, 0, 0, 3, 1), MF(1, 0, 0, 3, 0), MF(1, 0, 0, 1, 1)],
        "convnext": [G3(3, 0, 4), MF(1, 0, 0, 1, 1)],
    },
    ("fp32-g3f1", (7, 495)): {
        "head": [G3(3, 0, 4)],
    },
    ("fp32-g3f1", (7, 860)): {
        "embed": [G3(3, 0, 4)],
        "resnet": [G3(3, 0, 4), G3(3, 0, 4)],
        "attn": [G3(2, 0, 4), MF(1, 0, 0, 7, 1), MF(1, 0, 0, 7, 0), G3(3, 0, 4)],
        "convnext": [G3(2, 0, 4), G3(3, 0, 4)],
    },
    ("fp32-g3f1", (11, 746)): {
        "convnext": [G3(2, 0, 4), G3(2, 0, 4)],
    },
    ("fp32-exp16", (3, 641)): {
        "attn": [G3(3, 1, 4), MF(1, 0, 0, 3, 1), MF(1, 0, 0, 3, 0), MF(1, 0, 0, 1, 1)],
        "convnext": [G3(3, 1, 4), MF(1, 0, 0, 1, 1)],
    },
    ("fp32-exp16", (7, 495)): {
        "head": [G3(3, 1, 4)],
    },
    ("fp32-exp16", (7, 860)): {
        "embed": [G3(3, 1, 4)],
        "resnet": [G3(3, 1, 4), G3(3, 1, 4)],
        "attn": [G3(2, 1, 4), MF(1, 0, 0, 7, 1), MF(1, 0, 0, 7, 0), G3(3, 1, 4)],
        "convnext": [G3(2, 1, 4), G3(3, 1, 4)],
    },
    ("fp32-exp16", (11, 746)): {
        "convnext": [G3(2, 1, 4), G3(2, 1, 4)],
    },
    ("fp8", (3, 5)): {
        "embed": [B2(8, 1)],
        "resnet": [B2(8, 1), B2(8, 1)],
        "convnext": [B2(2, 1), B2(8, 1)],
        "head": [B2(2, 1)],
    },
    ("fp8", (3, 43)): {
        "embed": [B2(8, 1)],
        "resnet": [B2(8, 1), B2(8, 1)],
        "convnext": [B2(2, 1), B2(8, 1)],
        "head": [B2(2, 1)],
    },
    ("fp8", (3, 641)): {
        "convnext": [G3(3, 0, 1), B2(4, 1)],
    },
    ("fp8-exp32", (3, 641)): {
        "convnext": [B2(1, 1), B2(4, 1)],
    },
}


def expected_routes(cfg, st, B, L):
    kind = CR.KINDS[st]
    gemms = STAGE_GEMMS[kind]
    if not gemms:
        return []
    out = []
    for r, nk in zip(ROUTES[cfg, (B, L)][kind], gemms):
        N, K = nk if nk else ((L, 768) if len(out) == 1 else (768, L))
        out.append(tuple(r) + (N, K))
    return out


# ---- engines and references ------------------------------------------------------------------------

@pytest.fixture(scope="module")
def engines():
    """One engine per mode, built on first use, sized to the largest cell."""
    cur = {}

    def get(mode):
        if mode not in cur:
            from llmvox_amd.engine import build_engine
            wd, cd = ("bf16", "fp8") if mode == "fp8" else (mode, None)
            cur[mode] = build_engine(0, wd, wd, max_streams=1, max_positions=64, codec_dtype=cd,
                                     max_codec_frames=3 * 641 if mode == "fp8" else MAX_FRAMES)
        return cur[mode]

    yield get
    for e in cur.values():
        e.check_errors()
        e.close()


@pytest.fixture(scope="module")
def refs():
    """The fp64 reference of a (mode, g3f, stage, B, L), computed once and shared by the configs that use it.
    (g3f 32 with mode "fp8": codec_exp bit 32, no W8A8.)"""
    from llmvox_amd import weights as LW
    cw = LW.synthetic_codec(1234)
    models, cache = {}, {}

    def get(mode, g3f, st, B, L):
        if (mode, g3f) not in models:
            models[mode, g3f] = CR.Weights(cw, mode)
            models[mode, g3f].g3f = g3f
            models[mode, g3f].w8a8 = g3f != 32
        W = models[mode, g3f]
        # codec_g3f only matters where a GEMM of the stage is split (>= 192 tiles)
        x3 = any(W.x3(B * L, N, K) for N, K in (g for g in STAGE_GEMMS[CR.KINDS[st]] if g))
        key = (mode, g3f if x3 or W.q8(B * L) else 0, st, B, L)
        if key not in cache:
            x = CR.make_input(st, B, L)
            cache[key] = (x, CR.stage(W, st, x, CR.cell_bw(B, L))[1])
        return cache[key]

    return get


MEASURED = {}  # (stage kind, config) -> largest branch-relative device error over the module
MEASURED_PHASE = {}  # mode -> the iSTFT's error at phases in +-256 (not asserted)


def _set_opts(e, opts):
    for k, v in {**DEFAULT_OPTS, **opts}.items():
        e.set_option(k, v)


def _dev_input(st, x, B, L):
    return x.to(torch.int32) if st == 0 else x.reshape(B * L, -1).to(torch.float32)


def _run(e, st, x, B, L, bw, last=None):
    out, routes = e.codec_stages(st, st if last is None else last, _dev_input(st, x, B, L), B, L, bw)
    return out, routes


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\ncodec stages, largest device error / bound per (stage kind, config):")
    for (kind, cfg), v in sorted(MEASURED.items()):
        print(f"  {kind:9s} {cfg:14s} {v:.3e} / {CR.MARGIN * CR.YARDSTICK[kind, CONFIGS[cfg][0]]:.3e}")
    for mode, v in sorted(MEASURED_PHASE.items()):
        print(f"  iSTFT at phases in +-256, {mode}: {v:.3e}")


@pytest.mark.parametrize("cfg,st,B,L", CELLS, ids=[f"{c}-s{s}-{b}x{l}" for c, s, b, l in CELLS])
def test_stage_against_fp64(engines, refs, cfg, st, B, L):
    mode, opts, g3f = CONFIGS[cfg]
    e = engines(mode)
    x, ref = refs(mode, g3f, st, B, L)
    _set_opts(e, opts)
    try:
        out, routes = _run(e, st, x, B, L, CR.cell_bw(B, L))
        out = out.cpu()
    finally:
        _set_opts(e, {})
    e.check_errors()
    got = CR.compared(st, out.reshape(ref.shape), x)
    err = CR.rel_err(got, ref)
    kind = CR.KINDS[st]
    MEASURED[kind, cfg] = max(MEASURED.get((kind, cfg), 0.0), err)
    bound = CR.bound(st, mode)
    print(f"{cfg} stage {st} ({B}, {L}): {err:.3e} (bound {bound:.3e}) routes {[r[:6] for r in routes]}")
    assert routes == expected_routes(cfg, st, B, L)
    assert torch.isfinite(out).all()
    assert err <= bound, (err, bound)


@pytest.mark.parametrize("mode", ("bf16", "fp32"))
@pytest.mark.parametrize("B,L", ((3, 5), (3, 700)))
def test_full_window_is_decode_codes(engines, mode, B, L):
    """stages(0, 20) launches what lvx_codec_decode_codes launches: the same PCM, bit for bit."""
    e = engines(mode)
    _set_opts(e, {})
    codes = CR.make_codes(B, L).to(torch.int32)
    bw = CR.cell_bw(B, L)
    want = e.decode_codes(codes, bw).cpu()
    got, routes = e.codec_stages(0, 20, codes, B, L, bw)
    e.check_errors()
    assert len(routes) == 1 + 4 * 2 + 4 + 12 * 2 + 1
    assert torch.equal(got.cpu(), want)


@pytest.mark.parametrize("mode", ("bf16", "fp32"))
def test_window_equals_single_stages(engines, mode):
    """The ConvNeXt window (7, 18) in one call = twelve calls of one stage, bit for bit."""
    e = engines(mode)
    _set_opts(e, {})
    B, L, bw = 3, 5, 3
    x = CR.make_x(B, L).reshape(B * L, -1).to(torch.float32)
    whole, routes = e.codec_stages(7, 18, x, B, L, bw)
    y, single = x, []
    for st in range(7, 19):
        y, r = e.codec_stages(st, st, y, B, L, bw)
        single += r
    e.check_errors()
    assert torch.equal(whole.cpu(), y.cpu())
    assert routes == single and len(routes) == 24


def test_argument_checks(engines):
    from llmvox_amd import _lib
    e = engines("bf16")
    x = torch.zeros(4, 768)
    with pytest.raises(_lib.LvxArgError):
        e.codec_stages(5, 4, x, 1, 4)       # window order
    with pytest.raises(_lib.LvxArgError):
        e.codec_stages(1, 21, x, 1, 4)      # past the last stage
    with pytest.raises(_lib.LvxArgError):
        e.codec_stages(1, 1, x, 1, 4, bandwidth_id=4)
    with pytest.raises(_lib.LvxCapacityError):
        e.codec_stages(1, 1, torch.zeros(MAX_FRAMES + 1, 768), 1, MAX_FRAMES + 1)
    with pytest.raises(ValueError):
        e.codec_stages(20, 20, x, 1, 4)     # stage 20 takes a spectrum
    e.check_errors()


def test_istft_wide_phases(engines):
    """Measurement only (recorded in DESIGN.md section 2): the iSTFT's error at phases uniform in +-256, where the bf16 mode's
    native v_sin / v_cos are outside the range their comment claims. Printed, not asserted: no one has
    measured what phases a real checkpoint's head produces."""
    B, L = 2, 9
    spec = CR.make_spec(B, L, phase=256.0)
    ref = CR.istft(spec)
    for mode in ("bf16", "fp32"):
        e = engines(mode)
        _set_opts(e, {})
        out, _ = e.codec_stages(20, 20, spec.reshape(B * L, -1).to(torch.float32), B, L, 0)
        e.check_errors()
        err = CR.rel_err(out.cpu(), ref)
        MEASURED_PHASE[mode] = err
        print(f"iSTFT, phases in +-256, {mode}: {err:.3e}")
        assert torch.isfinite(out).all()
