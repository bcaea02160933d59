"""tests/attn_ref.py without a GPU: the inputs of tests/test_gpu_attn_probe.py are sensitive to every
single-key mistake (so that test is not blind), the fp64 merge agrees with the unsplit reference over the
kernel's split ranges, and the table of plan cells is what ar_plan.h decides."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import attn_ref as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "llmvox_amd", "csrc")


def _configs():
    """(kv, nsplit) of every cell: what the split edges, and so the queries, depend on besides (slot, t)."""
    return sorted({(c.kv, c.plan[0]) for c in A.cells() + A.idle_cells()})


@pytest.fixture(scope="module")
def stored():
    """Stored K / V of one slot per KV dtype (the generator's own quantisation)."""
    out = {}
    for i, kv in enumerate(("fp32", "bf16", "fp8")):
        k, v = A.history(3 + 7 * i)
        out[kv] = (3 + 7 * i, A.quantise(k, kv), A.quantise(v, kv))
    return out


def test_cells_cover_the_issue_list():
    ids = [A.cell_id(c) for c in A.cells()]
    assert len(set(ids)) == len(ids)
    for kv in ("bf16", "fp8"):
        for B in (1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64):
            assert f"{kv}-B{B}" in ids
        assert f"{kv}-B8-bt=2" in ids and f"{kv}-B16-bt=2" in ids and f"{kv}-B6-ln_max=4" in ids
    assert "fp8-B12" in ids and "bf16-B65" in ids and "fp32-B12-f32b=0" in ids
    for B in (1, 3, 12, 32):
        assert f"fp32-B{B}-exp=1024" in ids
    for c in A.cells():
        ts = {t for call in range(A.n_calls(c.B)) for t in A.row_positions(c.B, call)}
        assert ts == set(A.T_LIST), A.cell_id(c)  # every cell sees every t
        S = A.max_streams(c.kv)
        sl = A.row_slots(c.B, S)
        assert len(set(sl)) == c.B and all(0 <= s < S for s in sl) and sl != list(range(c.B))


def test_cells_match_the_plan_header(tmp_path):
    """The (nsplit, attn_direct, attn8) each cell expects, and whether it ends in rows or partials, against
    ar_plan_step (tests/ar_plan_dump.cpp, built host-only like tests/test_ar_plan.py does)."""
    cc = next((c for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")) if c and os.path.exists(c)), None)
    if cc is None:
        pytest.skip("no hipcc to build the plan program with")
    exe = str(tmp_path / "ar_plan_dump")
    subprocess.run([cc, "-O1", "-std=c++17", "-x", "hip", "--offload-host-only", "-Wall", "-Werror", "-I",
                    os.path.join(ROOT, "include"), "-I", CSRC, os.path.join(ROOT, "tests", "ar_plan_dump.cpp"), "-o", exe],
                   check=True)
    cells = A.cells() + A.idle_cells()
    specs = sorted({",".join(f"{k}={v}" for k, v in c.opts.items()) or "-" for c in cells})
    rows = {}
    for line in subprocess.run([exe] + specs, check=True, capture_output=True, text=True).stdout.splitlines():
        f = line.split()
        rows[(f[0], f[1], f[2], int(f[3]), int(f[4]), int(f[5]))] = f
    for c in cells:
        spec = ",".join(f"{k}={v}" for k, v in c.opts.items()) or "-"
        wd = "fp32" if c.kv == "fp32" else "bf16"
        f = rows[(spec, wd, c.kv, c.B, 0, 0)]
        path, nsplit, direct, attn8, qsplit = f[6], int(f[11]), int(f[12]), int(f[13]), int(f[17])
        assert (nsplit, direct, attn8) == c.plan, (A.cell_id(c), f)
        assert not qsplit, A.cell_id(c)  # the probe needs an attention that takes st.q
        merged = path == "v3" or (path in ("mfma_ln", "mfma_rows") and nsplit > 1)
        assert merged == c.merged and c.form == int(not merged and direct == A.ATTN_PARTIALS), (A.cell_id(c), f)


@pytest.mark.parametrize("kv,ns_max", _configs())
def test_split_ranges_and_edges(kv, ns_max):
    for t in A.T_LIST:
        r = A.split_ranges(t, ns_max, kv)
        live = [(a, b) for a, b in r if a < b]
        assert live[0][0] == 0 and live[-1][1] == t
        assert all(live[i][1] == live[i + 1][0] for i in range(len(live) - 1))
        assert all(a >= t for a, b in r if a >= b)  # empty splits only trail
        e = A.edge_keys(t, ns_max, kv)
        assert e == sorted(set(e)) and e[0] == 0 and e[-1] == t - 1
        for a, b in live:
            assert a in e and b - 1 in e
    # T_LIST reaches the trailing empty splits of the tile-rounded ranges at every split count: 320 keys
    # at 4 splits (3 x 128), 513 at 8 (5 x 128; 320 keys have only 5 tiles, so 5 live splits), 1,025 at 16
    if kv != "fp32" and ns_max >= 4:
        t = {4: 320, 8: 513, 16: 1025}[ns_max]
        assert any(a >= b for a, b in A.split_ranges(t, ns_max, kv))


@pytest.mark.parametrize("kv,ns_max", _configs())
def test_merge_of_split_partials_is_the_reference(stored, kv, ns_max):
    slot, K, V = stored[kv]
    for t in (1, 65, 320, 1025):
        q, _ = A.row_queries(K, t, A.edge_keys(t, ns_max, kv), slot)
        ref, _ = A.attention_fp64(q[:1], K, V, t)
        r = A.split_ranges(t, ns_max, kv)
        po = np.zeros((A.NH, A.NSPLIT, A.HD))
        pml = np.zeros((A.NH, A.NSPLIT, 2))
        for sp, (k0, k1) in enumerate(r):
            if k0 >= k1:
                pml[:, sp] = (-np.inf, 0.0)
                continue
            Kh = K[k0:k1].astype(np.float64).reshape(-1, A.NH, A.HD)
            Vh = V[k0:k1].astype(np.float64).reshape(-1, A.NH, A.HD)
            s = np.einsum("hd,thd->ht", q[0].astype(np.float64), Kh) * A.SCALE
            m = s.max(axis=1)
            p = np.exp(s - m[:, None])
            po[:, sp] = np.einsum("ht,thd->hd", p, Vh)
            pml[:, sp, 0], pml[:, sp, 1] = m, p.sum(axis=1)
        got = A.merge_fp64(po, pml, len(r))
        assert np.abs(got - ref[0]).max() < 1e-12


@pytest.mark.parametrize("kv,ns_max", _configs())
def test_every_single_key_mutation_is_visible(stored, kv, ns_max):
    """For the generator's inputs at every t: the spiked key holds a large share of the softmax, and
    removing it or replacing it by its neighbour moves the head's output by at least MUTATION_MIN and by
    at least MUTATION_OVER_TOL times the GPU test's tolerance (the bf16-row form of it where this KV
    dtype has one: the larger). The GPU test asserts the same for every row it runs."""
    slot, K, V = stored[kv]
    worst_w, worst_abs, worst_rel, worst32 = 1.0, np.inf, np.inf, 0.0
    for t in A.T_LIST:
        q, spiked = A.row_queries(K, t, A.edge_keys(t, ns_max, kv), slot)
        assert set(spiked.ravel()) == set(A.edge_keys(t, ns_max, kv))
        out, w = A.attention_fp64(q, K, V, t)
        tol = A.tolerance(kv, out, kv != "fp32").reshape(-1, A.NH, A.HD)
        for d in A.mutation_effects(q, K, V, t, spiked, out, w):
            worst_abs = min(worst_abs, float(np.abs(d).max(axis=-1).min()))
            worst_rel = min(worst_rel, float((np.abs(d) / tol).max(axis=-1).min()))
        worst_w = min(worst_w, float(np.take_along_axis(w, spiked[:, :, None], axis=2).min()))
        out32, _ = A.attention_fp64(q, K, V, t, dtype=np.float32)
        worst32 = max(worst32, float(np.abs(out32 - out).max()))
    print(f"\n[attn_ref {kv} ns_max {ns_max}] spiked weight >= {worst_w:.3f}; single-key mutation moves the output "
          f"by >= {worst_abs:.3f} = {worst_rel:.0f} x the tolerance; plain fp32 evaluation within {worst32:.2e}")
    assert A.ATTN_ABS[kv] <= A.ATTN_ABS_CAP
    assert worst_w > 0.3
    assert worst_abs >= A.MUTATION_MIN
    assert worst_rel >= A.MUTATION_OVER_TOL
    # a plain fp32 evaluation: far inside the worst case t 2^-24 max|v| ~ 3e-4 of a 1,025-term sum; what a
    # device path in fp32 can be expected to reach
    assert worst32 < 5e-5
