"""The fp64 codec reference of tests/codec_ref.py, without a GPU: it is the oracle's decode, and the
comparison tests/test_gpu_codec_stages.py makes with it is sensitive to every indexing / omission error
listed below by at least 10x the bound the GPU test holds that stage and mode to.

The factor of 10 is a condition on the inputs of ``codec_ref.make_*`` (unit scale, per-stream offset and
gain, raised edge frames, the spectrum's single-bin frames), not a measurement of any kernel.
"""
import pytest
import torch

from llmvox_amd import weights as LW
from oracle import reference_cpu as R
from tests import codec_ref as CR

MODES = ("fp32", "bf16")
FP8_KINDS = ("embed", "resnet", "convnext", "head")  # the stage kinds the fp8 codec weights are tested at


@pytest.fixture(scope="module")
def cw():
    return LW.synthetic_codec(1234)


@pytest.fixture(scope="module")
def models(cw):
    return {(m, dt): CR.Weights(cw, m, dt) for m in MODES + ("fp8",) for dt in (torch.float64, torch.float32)}


def test_fp32_model_is_the_oracle_decode(cw, models):
    """All 21 stages chained in fp64 = oracle/reference_cpu.py's decode_codes on fp64 weights, up to the one
    fp32 operation the oracle keeps there: it squares the fp32 Hann window in fp32 for the envelope
    (2^-24 relative)."""
    Wc = {k: torch.from_numpy(v).double() for k, v in cw.items()}
    W = models["fp32", torch.float64]
    for B, L, bw in ((2, 9, 0), (1, 1, 3), (3, 5, 3)):
        codes = CR.make_codes(B, L)
        x = codes
        for st in range(CR.N_STAGES):
            x, _ = CR.stage(W, st, x, bw)
        ref = R.decode_codes(Wc, codes, bw)
        assert x.shape == (B, 320 * L)
        assert CR.rel_err(x, ref) < 2.0 ** -23, (B, L, bw)


def test_bound_table_is_complete_and_small(models):
    kinds = set(CR.KINDS.values())
    assert set(CR.YARDSTICK) == {(k, m) for k in kinds for m in MODES} | {(k, "fp8") for k in FP8_KINDS}
    # fp32 bf16x3 GEMMs: DESIGN.md's 2^-16 relative loss per product. Every fp32 bound, taken back from
    # the branch's scale to the stage output's, stays at or below it.
    W = models["fp32", torch.float64]
    for st in (0, 1, 3, 6, 7, 19):
        x = CR.make_input(st, 3, 43)
        out, cmp_ = CR.stage(W, st, x, 0)
        scaled = CR.bound(st, "fp32") * float(cmp_.pow(2).mean().sqrt() / out.pow(2).mean().sqrt())
        assert scaled <= 2.0 ** -16, (st, scaled)


def test_fp32_evaluation_stays_inside_the_margin(cw, models):
    """The fp32 evaluation of the fp32 model on this host is itself 'another summation order' (its BLAS
    blocking and thread count differ from the host the table was computed on), the thing the margin is for:
    on the small cells it stays within half the device bound of its stage kind. (On the host of the table
    it is <= the table's entry: `python -m tests.codec_ref`. The bf16 / fp8 figures are dominated by
    double-rounding flips, discrete events whose number on a small cell differs from host to host: they
    are not re-checked here.)"""
    w64, w32 = models["fp32", torch.float64], models["fp32", torch.float32]
    for B, L in CR.CELLS_ALL[:4]:
        for st in CR.ALL_STAGES:
            y = CR.yardstick(cw, "fp32", st, B, L, CR.cell_bw(B, L), w64=w64, w32=w32)
            assert y <= 0.5 * CR.bound(st, "fp32"), (st, B, L, y)


# mutation -> ((stage, B, L), ...): the smallest shapes at which it can occur
# (stage 0 at L = 4: the k7 window's last tap, whose channels are the GEMM's last K, first meets a frame there)
WEIGHT_GEMM_STAGES = ((0, 1, 4), (1, 1, 2), (3, 1, 2), (7, 1, 2), (19, 1, 2))
MUTATIONS = {
    "conv_leak": ((0, 2, 2), (1, 2, 2), (7, 2, 2)),          # k7, k3 and the depthwise k7
    "last_row_copy": WEIGHT_GEMM_STAGES,
    "drop_k32": WEIGHT_GEMM_STAGES,
    "drop_k64": WEIGHT_GEMM_STAGES,
    "head_col_1281": ((19, 3, 5),),                          # one column of 1,282: averaged over 15 rows
    "head_tile": ((19, 1, 1),),
    "softmax_pad": ((3, 1, 5),),
    "gn_next_stream": ((1, 2, 2), (3, 2, 2), (6, 2, 2)),
    "no_bias": WEIGHT_GEMM_STAGES,
    "no_gamma": ((7, 1, 1),),
    "no_residual": ((1, 1, 1), (3, 1, 1), (7, 1, 1)),
    "next_block": ((1, 1, 1), (7, 1, 1), (12, 1, 1)),
    "other_bw": ((6, 1, 1), (7, 1, 1)),
    "istft_dc_imag": ((20, 1, 1), (20, 1, 3)),
    "ola_env_shift": ((20, 1, 1), (20, 1, 3)),
}
CASES = [(mode, m, c) for mode in MODES + ("fp8",) for m, cells in MUTATIONS.items() for c in cells
         if mode != "fp8" or CR.KINDS[c[0]] in FP8_KINDS]


@pytest.mark.parametrize("mode,mut,cell", CASES, ids=[f"{mode}-{m}-s{c[0]}-{c[1]}x{c[2]}" for mode, m, c in CASES])
def test_mutation_moves_the_compared_quantity(models, mode, mut, cell):
    st, B, L = cell
    W = models[mode, torch.float64]
    x = CR.make_input(st, B, L)
    bw = CR.cell_bw(B, L)
    _, ref = CR.stage(W, st, x, bw)
    if mut == "next_block":
        widx = {1: 1, 7: 1, 12: 6}[st]  # the block after the stage's own
        out, _ = CR.stage(W, st, x, bw, widx=widx)
    else:
        out, _ = CR.stage(W, st, x, bw, mut={mut})
    effect = CR.rel_err(CR.compared(st, out, x), ref)
    need = 10.0 * CR.bound(st, mode)
    print(f"{mut} stage {st} ({B}, {L}) {mode}: effect {effect:.3e}, 10 x bound {need:.3e}")
    assert effect >= need, (effect, need)
