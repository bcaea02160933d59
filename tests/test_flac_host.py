"""The host side of the FLAC stage (llmvox_amd/csrc/pcm_host.h) without a GPU and without Python in the way:
tests/host/flac_check.cpp, a program of its own, built with the system compiler under AddressSanitizer and UBSan, runs
the functions behind lvx_flac_subframe and lvx_flac_finish over the test signals at every rate and every length around the
frame cuts, holds them to the header's rule written a second time, checks the plan_flac counts of pcm_plan against brute
force, and covers cap too small, n = 0 and the argument errors. Exit status 0: every check held and no sanitizer spoke."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_flac_check(tmp_path):
    cxx = shutil.which("g++")
    assert cxx is not None, "no g++ to build the check program with"
    exe = str(tmp_path / "flac_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall",
                    "-Werror", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "llmvox_amd", "csrc"),
                    os.path.join(ROOT, "tests", "host", "flac_check.cpp"), "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "flac host check: ok" in run.stdout
