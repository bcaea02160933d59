"""The fused layers field of the decode step's plan (llmvox_amd/csrc/ar_plan.h, ArStepPlan::la_fused) without
a GPU: tests/ar_plan_la_dump.cpp, built like tests/ar_plan_l0_dump.cpp, prints every field of the plan for
every weight dtype, KV dtype, B = 1..66, row mode, table presence and sample flag under the option sets below.
Checked: with option laf 1 (the default) the field is set exactly where the fused layer-0 form is: bf16 weights
with the tables, no sampling, a one-split 4-wave attention, bf16 KV at 9 <= B <= 32 and fp8 KV at
17 <= B <= 32; it is clear with laf 0, with l0a 0, without the tables (q0 false: the plan of the per-op probes),
on the 8-wave cells and on fp32 KV; and switching laf changes no other field of any plan."""
import os
import subprocess
from collections import namedtuple

import pytest

from tests.test_ar_plan import CSRC, ROOT, _hipcc

SETS = ["-", "laf=1", "laf=0", "l0a=0", "l0a=0,laf=1", "l0q=0", "defer_select=0", "defer_select=2", "bt=2", "bt=0",
        "f32b=0", "ln_max=4", "ln_max=4,laf=0"]
ON = ("-", "laf=1", "defer_select=2", "bt=0", "f32b=0", "ln_max=4")  # the sets under which the cells take the form
Row = namedtuple("Row", "opts wd kv B row q0 sample path sel end nsplit attn_direct attn8 selcopy l0_fused fused_mlp "
                        "q0_gran xpk ksplit qsplit la_fused")


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    cc = _hipcc()
    if cc is None:
        pytest.skip("no hipcc to build the plan program with")
    exe = str(tmp_path_factory.mktemp("ar_plan_la") / "ar_plan_la_dump")
    subprocess.run([cc, "-O1", "-std=c++17", "-x", "hip", "--offload-host-only", "-Wall", "-Werror",
                    "-I", os.path.join(ROOT, "include"), "-I", CSRC, os.path.join(ROOT, "tests", "ar_plan_la_dump.cpp"),
                    "-o", exe], check=True)
    out = subprocess.run([exe] + SETS, check=True, capture_output=True, text=True).stdout
    rows = {}
    for line in out.splitlines():
        f = line.split()
        r = Row(f[0], f[1], f[2], int(f[3]), int(f[4]), int(f[5]), int(f[6]), f[7], f[8], *map(int, f[9:]))
        rows[(r.opts, r.wd, r.kv, r.B, r.row, r.q0, r.sample)] = r
    assert len(rows) == len(SETS) * 2 * 3 * 67 * 2 * 2
    return rows


def _cell(r):
    """the cells the fused forms are built for"""
    return (r.wd == "bf16" and r.q0 and not r.row and not r.sample and r.B <= 32
            and ((r.kv == "bf16" and r.B >= 9) or (r.kv == "fp8" and r.B >= 17)))


def test_fused_layers_field_is_set_exactly_on_its_cells(plans):
    n = 0
    for r in plans.values():
        want = _cell(r) and r.opts in ON
        assert bool(r.la_fused) == want, r
        n += want
    assert n == len(ON) * ((32 - 9 + 1) + (32 - 17 + 1))


def test_fused_layers_field_is_clear_elsewhere(plans):
    for r in plans.values():
        if (r.sample or r.wd == "fp32" or r.kv == "fp32" or r.row or not r.q0 or r.B <= 8 or r.B > 32 or r.attn8
                or not r.l0_fused or r.opts in ("laf=0", "l0a=0", "l0a=0,laf=1", "l0q=0", "defer_select=0", "bt=2",
                                                "ln_max=4,laf=0")):
            assert not r.la_fused, r
        if r.kv == "fp8" and r.B <= 16:  # the 8-wave cells keep the separate launches
            assert not r.la_fused, r
        if r.la_fused:  # the step it rides on: the fused layer-0 form, one split per (row, head) written into xn
            assert (r.path, r.sel, r.nsplit, r.attn8, r.selcopy, r.l0_fused, r.xpk) == ("mfma_rows", "q0_rows", 1, 0, 1, 1, 1), r


@pytest.mark.parametrize("on,off", [("-", "laf=0"), ("laf=1", "laf=0"), ("ln_max=4", "ln_max=4,laf=0"),
                                    ("l0a=0,laf=1", "l0a=0")])
def test_option_laf_changes_nothing_else(plans, on, off):
    """laf 0 is the same plan without the field: the independent form the fused one is held to."""
    n = 0
    for key, r in plans.items():
        if r.opts != on:
            continue
        o = plans[(off,) + key[1:]]
        assert not o.la_fused, o
        assert o._replace(opts=on, la_fused=r.la_fused) == r, (r, o)
        n += 1
    assert n == 2 * 3 * 67 * 2 * 2
