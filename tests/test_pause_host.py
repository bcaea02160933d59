"""The host side of the pause stage (llmvox_amd/csrc/pcm_host.h) without a GPU and without Python in the way:
tests/host/pause_check.cpp, a program of its own, built with the system compiler under AddressSanitizer and UBSan, runs
the function behind lvx_pause_slots over constructed sentences at every rate, encoding and length around a block's edge,
holds it to the header's rule written a second time, checks the mark at the threshold's edges, the counts against brute
force and the plan_pause rows of pcm_plan, and covers cap too small and the refusals. Exit status 0: every check held
and no sanitizer spoke."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pause_check(tmp_path):
    cxx = shutil.which("g++")
    assert cxx is not None, "no g++ to build the check program with"
    exe = str(tmp_path / "pause_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall",
                    "-Werror", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "llmvox_amd", "csrc"),
                    os.path.join(ROOT, "tests", "host", "pause_check.cpp"), "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "pause host check: ok" in run.stdout
