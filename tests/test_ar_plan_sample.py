"""The decode step's plan with the trailing ``sample`` argument (llmvox_amd/csrc/ar_plan.h), without a
GPU: tests/ar_plan_sample_dump.cpp, built like tests/ar_plan_dump.cpp, prints for every weight dtype,
KV dtype, B = 1..66, row mode and table presence under the option sets of tests/test_ar_plan.py the
six-argument plan, the plans with sample = false / true, and the plan of option defer_select 0.
Checked: sample = true is the defer_select 0 plan with the sampled select in the argmax kernel's place
(no end-of-call commit, no shadow-record copy, no table form), row mode ignores it, and sample =
false is the six-argument call. The same program prints the known answers of the library's host
form of Philox4x32-10 (lvx_common.h), the code the kernel runs."""
import os
import subprocess
from collections import namedtuple

import pytest

from tests.test_ar_plan import CSRC, OPTION_SETS, ROOT, _hipcc
from tests.test_sampling_ref import KAT

Row = namedtuple("Row", "opts wd kv B row q0 path sel end fused_mlp q0_gran nsplit attn_direct attn8 selcopy xpk "
                        "ksplit qsplit")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    cc = _hipcc()
    if cc is None:
        pytest.skip("no hipcc to build the plan program with")
    exe = str(tmp_path_factory.mktemp("ar_plan_sample") / "ar_plan_sample_dump")
    subprocess.run([cc, "-O1", "-std=c++17", "-x", "hip", "--offload-host-only", "-Wall", "-Werror",
                    "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                    os.path.join(ROOT, "tests", "ar_plan_sample_dump.cpp"), "-o", exe], check=True)
    return exe


@pytest.fixture(scope="module")
def plans(exe):
    out = subprocess.run([exe] + OPTION_SETS, check=True, capture_output=True, text=True).stdout
    rows = {}
    for line in out.splitlines():
        f = line.split()
        r = Row(f[1], f[2], f[3], int(f[4]), int(f[5]), int(f[6]), f[7], f[8], f[9], *map(int, f[10:]))
        rows[(f[0], r.opts, r.wd, r.kv, r.B, r.row, r.q0)] = r
    n = len(OPTION_SETS) * 2 * 3 * 2
    assert len(rows) == n * (3 * 67 + 66)
    return rows


def test_sample_is_the_nodefer_plan_with_the_sampled_select(plans):
    n = 0
    for (tag, *key), r in plans.items():
        if tag != "true" or r.row:
            continue
        n += 1
        nd = plans[("nodefer", *key)]
        assert nd.sel == "argmax" and nd.end == "none" and not nd.selcopy and not nd.q0_gran, nd
        assert (r.sel, r.end, r.selcopy, r.q0_gran) == ("sample", "none", 0, 0), r
        assert r._replace(sel="argmax") == nd, (r, nd)
    assert n == len(OPTION_SETS) * 2 * 3 * 66 * 2


def test_row_mode_ignores_sample(plans):
    n = 0
    for (tag, *key), r in plans.items():
        if tag == "true" and r.row:
            n += 1
            assert r == plans[("six", *key)] and r.sel == "argmax", r
    assert n == len(OPTION_SETS) * 2 * 3 * 2


def test_sample_false_is_the_six_argument_call(plans):
    n = 0
    for (tag, *key), r in plans.items():
        if tag == "false":
            n += 1
            assert r == plans[("six", *key)], r
    assert n == len(OPTION_SETS) * 2 * 3 * 67 * 2
    assert any(r.sel not in ("argmax", "sample") for r in plans.values())  # (the deferred forms are in the sweep)


def test_library_philox_known_answers(exe):
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines()
    assert len(out) == len(KAT)
    for line, (counter, key, want) in zip(out, KAT):
        f = line.split()
        assert f[0] == "philox" and f[7] == "->"
        assert tuple(int(x, 16) for x in f[1:7]) == tuple(counter) + tuple(key)
        assert tuple(int(x, 16) for x in f[8:12]) == want, line
