"""The decode step's plan (llmvox_amd/csrc/ar_plan.h, ar_plan_step) without a GPU: a small host
program (tests/ar_plan_dump.cpp) built against the header with the Makefile's compiler prints the plan
of every weight dtype, KV dtype, B = 1..66, row mode and table presence under the option sets the GPU
tests use. Checked here: the default rows, that every select form is one its path can run, that the
end-of-call commit matches the select form, that the row forward is the plain GEMV, and option bt 2."""
import os
import shutil
import subprocess
from collections import namedtuple

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "llmvox_amd", "csrc")
OPTION_SETS = ["-", "bt=0", "bt=2", "defer_select=0", "defer_select=2", "l0q=0", "fuse_mlp=0", "f32b=0",
               "ln_max=7", "ln_max=16", "exp=512", "exp=1024", "bt=2,l0q=0", "bt=2,defer_select=0"]
DEFAULTS = dict(defer_select=1, fuse_mlp=1, bt=1, exp=0, f32b=1, ln_max=8, l0q=1)
Row = namedtuple("Row", "opts wd kv B row q0 path sel end fused_mlp q0_gran nsplit attn_direct attn8 selcopy xpk "
                        "ksplit qsplit")
ATTN_PARTIALS, ATTN_XN, ATTN_XN_PACKED, ATTN_F32_ROWS = 0, 1, 2, 3


def _hipcc():
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")):
        if c and os.path.exists(c):
            return c
    return None


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    cc = _hipcc()
    if cc is None:
        pytest.skip("no hipcc to build the plan program with")
    exe = str(tmp_path_factory.mktemp("ar_plan") / "ar_plan_dump")
    # host-only: the header has no kernels, and nothing here touches a device
    subprocess.run([cc, "-O1", "-std=c++17", "-x", "hip", "--offload-host-only", "-Wall", "-Werror",
                    "-I", os.path.join(ROOT, "include"), "-I", CSRC, os.path.join(ROOT, "tests", "ar_plan_dump.cpp"),
                    "-o", exe], check=True)
    out = subprocess.run([exe] + OPTION_SETS, check=True, capture_output=True, text=True).stdout
    rows = {}
    for line in out.splitlines():
        f = line.split()
        r = Row(f[0], f[1], f[2], int(f[3]), int(f[4]), int(f[5]), f[6], f[7], f[8], *map(int, f[9:]))
        rows[(r.opts, r.wd, r.kv, r.B, r.row, r.q0)] = r
    assert len(rows) == len(OPTION_SETS) * 2 * 3 * 67 * 2
    return rows


def _opts(spec):
    o = dict(DEFAULTS)
    if spec != "-":
        o.update((k, int(v)) for k, v in (t.split("=") for t in spec.split(",")))
    return o


def attn_ns_max(B):
    ns = 16
    while ns > 1 and ns * 8 * B > 256:
        ns >>= 1
    return ns


def test_default_plan(plans):
    """Default options, fused mode, tables built for bf16 weights (and none for fp32)."""
    for kv in ("fp32", "bf16", "fp8"):
        for B in range(1, 67):
            r = plans[("-", "bf16", kv, B, 0, 1)]
            got = (r.path, r.sel, r.end)
            if B <= 2:
                assert got == ("gemv", "gran", "select_final"), r
                assert r.q0_gran and r.fused_mlp and r.nsplit == 16 and r.selcopy, r
            elif B == 3:
                assert got == ("mfma_ln", "argmax", "none"), r
                assert r.nsplit == attn_ns_max(3) and r.attn_direct == ATTN_PARTIALS and not r.attn8, r
            elif B == 4:
                assert got == ("mfma_ln", "q0_rows", "argmax"), r
                assert r.nsplit == attn_ns_max(4) and r.attn_direct == ATTN_PARTIALS and not r.attn8, r
            elif B <= 8:
                assert got == ("mfma_ln", "q0_rows", "argmax"), r
                assert r.nsplit == 1 and r.attn_direct == ATTN_XN and r.attn8, r
            elif B <= 32:
                assert got == ("mfma_rows", "q0_rows", "argmax"), r
                assert r.xpk == 1 and r.nsplit == 1 and r.attn_direct == ATTN_XN_PACKED, r
                assert r.attn8 == (kv == "fp8" and B <= 16), r
            elif B <= 64:
                assert got == ("v3", "embed", "argmax"), r
                assert r.nsplit == attn_ns_max(B) and r.attn_direct == ATTN_PARTIALS and not r.attn8, r
            else:
                assert got == ("gemv", "argmax", "none"), r
                assert not r.fused_mlp and r.nsplit == 16, r
            if B > 2:
                assert not r.fused_mlp and not r.q0_gran, r
            if not 9 <= B <= 32:
                assert r.xpk == 0, r
            assert r.selcopy == (r.sel in ("gran", "q0_rows")), r

            r = plans[("-", "fp32", kv, B, 0, 0)]
            got = (r.path, r.sel, r.end)
            assert not r.fused_mlp and not r.q0_gran and not r.attn8 and r.xpk == 0, r
            if B <= 2:
                assert got == ("gemv", "gran", "select_final") and r.nsplit == 16, r
            elif B == 3:
                assert got == ("f32b", "argmax", "none") and r.ksplit, r
            elif B <= 32:
                assert got == ("f32b", "embed", "argmax") and r.ksplit and r.qsplit, r
            elif B <= 64:
                assert got == ("f32b", "argmax", "none") and r.ksplit and not r.qsplit, r
            else:
                assert got == ("gemv", "argmax", "none"), r
            if r.path == "f32b":
                assert r.nsplit == attn_ns_max(B), r
                assert r.attn_direct == (ATTN_F32_ROWS if r.nsplit == 1 else ATTN_PARTIALS), r


def test_select_form_is_legal_for_its_path(plans):
    for r in plans.values():
        o = _opts(r.opts)
        if r.path == "v3":
            assert r.wd == "bf16" and r.sel in ("argmax", "embed"), r
        elif r.path == "f32b":
            assert r.wd == "fp32" and (r.sel == "argmax" or (r.sel == "embed" and r.qsplit)), r
        elif r.path == "gemv":
            assert r.sel == "argmax" or (r.sel == "gran" and r.B <= 2), r
        else:
            assert r.wd == "bf16" and r.path in ("mfma_ln", "mfma_rows"), r
            assert (r.path == "mfma_ln") == (r.B <= o["ln_max"]), r
            if r.sel == "q0_rows":
                assert o["l0q"] and r.q0 and 4 <= r.B <= 32, r
            elif r.sel == "ln_gran":
                assert r.path == "mfma_ln" and 4 <= r.B <= min(o["ln_max"], 8) and o["defer_select"] == 1, r
            else:
                assert r.sel in ("argmax", "embed"), r
        if not o["defer_select"]:
            assert r.sel == "argmax", r
        if r.q0_gran:
            assert r.sel == "gran" and r.q0 and o["l0q"], r


def test_end_commit_follows_the_select_form(plans):
    want = {"argmax": "none", "gran": "select_final", "embed": "argmax", "ln_gran": "argmax", "q0_rows": "argmax"}
    for r in plans.values():
        assert r.end == want[r.sel], r


def test_row_forward_is_the_plain_gemv(plans):
    n = 0
    for r in plans.values():
        if r.row:
            n += 1
            assert (r.B, r.path, r.sel, r.end) == (1, "gemv", "argmax", "none"), r
            assert not r.q0_gran and not r.selcopy and r.nsplit == 16 and r.attn_direct == ATTN_PARTIALS, r
    assert n == len(OPTION_SETS) * 2 * 3 * 2


def test_v3_everywhere_defers_through_the_embed_select_kernel(plans):
    """Option bt 2, defaults otherwise: v3 cannot run the table or granule forms."""
    for kv in ("fp32", "bf16", "fp8"):
        for q0 in (0, 1):
            for B in range(3, 65):
                r = plans[("bt=2", "bf16", kv, B, 0, q0)]
                assert r.path == "v3" and r.sel == ("argmax" if B == 3 else "embed"), r
                assert r.nsplit == attn_ns_max(B) and not r.selcopy and r.xpk == 0, r
