"""The two tail fields of the decode step's plan (llmvox_amd/csrc/ar_plan.h: ArStepPlan::x_folded, the attention
publishes the folded residual for c_proj, and ArStepPlan::lm_fused, ln_f + lm_head in one launch) without a GPU: a
small host program (tests/ar_plan_tail_dump.cpp), built as tests/test_ar_plan.py builds its own, prints them with
la_fused for B = 1..64, the three KV dtypes, bf16 / fp32 weights, with and without the q0 tables and the sample flag,
under every combination of the options xfold / lmf / laf / l0a at 0 / 1. Checked: lm_fused is set exactly where
la_fused is set and its option is on; x_folded likewise, but only from B = 16 up (below that the folded residual
measured no gain and ar_plan_step gates it off, with the numbers there); la_fused itself sits on the cells the
fused layers form was built for (bf16 weights with the tables, greedy, bf16 KV 9 <= B <= 32 or fp8 KV
17 <= B <= 32), so the probes (which plan without the tables) and the sampling plans keep the separate kernels."""
import itertools
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "llmvox_amd", "csrc")
NAMES = ("xfold", "lmf", "laf", "l0a")
OPTION_SETS = [",".join(f"{n}={v}" for n, v in zip(NAMES, vs)) for vs in itertools.product((0, 1), repeat=4)] + ["-"]


def _hipcc():
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")):
        if c and os.path.exists(c):
            return c
    return None


@pytest.fixture(scope="module")
def rows(tmp_path_factory):
    cc = _hipcc()
    if cc is None:
        pytest.skip("no hipcc to build the plan program with")
    exe = str(tmp_path_factory.mktemp("ar_plan_tail") / "ar_plan_tail_dump")
    # host-only: the header has no kernels, and nothing here touches a device
    subprocess.run([cc, "-O1", "-std=c++17", "-x", "hip", "--offload-host-only", "-Wall", "-Werror",
                    "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                    os.path.join(ROOT, "tests", "ar_plan_tail_dump.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe] + OPTION_SETS, check=True, capture_output=True, text=True).stdout
    got = []
    for line in out.splitlines():
        f = line.split()
        got.append(dict(opts=f[0], wd=f[1], kv=f[2], B=int(f[3]), q0=int(f[4]), sample=int(f[5]), path=f[6],
                        l0_fused=int(f[7]), la_fused=int(f[8]), x_folded=int(f[9]), lm_fused=int(f[10])))
    assert len(got) == len(OPTION_SETS) * 2 * 3 * 64 * 2 * 2
    return got


def _opts(spec):
    o = dict.fromkeys(NAMES, 1)
    if spec != "-":
        o.update((k, int(v)) for k, v in (t.split("=") for t in spec.split(",")))
    return o


def test_tail_forms_are_set_exactly_on_fused_layers_steps_with_their_option_on(rows):
    n = {"x_folded": 0, "lm_fused": 0}
    for r in rows:
        o = _opts(r["opts"])
        assert r["x_folded"] == (r["la_fused"] and o["xfold"] and r["B"] >= 16), r
        assert r["lm_fused"] == (r["la_fused"] and o["lmf"]), r
        n["x_folded"] += r["x_folded"]
        n["lm_fused"] += r["lm_fused"]
    assert n["x_folded"] > 0 and n["lm_fused"] > 0


def test_fused_layers_cells(rows):
    """where la_fused (and so either tail form) can be set at all"""
    for r in rows:
        o = _opts(r["opts"])
        cell = (r["wd"] == "bf16" and r["q0"] and not r["sample"] and
                ((r["kv"] == "bf16" and 9 <= r["B"] <= 32) or (r["kv"] == "fp8" and 17 <= r["B"] <= 32)))
        assert r["la_fused"] == int(bool(cell and o["laf"] and o["l0a"])), r
        if r["la_fused"]:
            assert r["l0_fused"] and r["path"] == "mfma_rows", r


def test_defaults_are_on(rows):
    for r in rows:
        if r["opts"] == "-":
            assert r["lm_fused"] == r["la_fused"] and r["x_folded"] == (r["la_fused"] and r["B"] >= 16), r
