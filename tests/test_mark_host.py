"""The host side of the watermark stage (llmvox_amd/csrc/pcm_host.h) without a GPU and without Python in the way:
tests/host/mark_check.cpp, a program of its own, built with the system compiler under AddressSanitizer and UBSan, holds
the sign table to its definition written a second time, its digest, the streaming counts, and drives plan_mark through
pcm_plan and pcm_chunks: refused calls, the alternating history buffers, the final call, 33 rows and a second mark on an
open segment. Exit status 0: every check held and no sanitizer spoke."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_mark_check(tmp_path):
    cxx = shutil.which("g++")
    assert cxx is not None, "no g++ to build the check program with"
    exe = str(tmp_path / "mark_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall",
                    "-Werror", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "llmvox_amd", "csrc"),
                    os.path.join(ROOT, "tests", "host", "mark_check.cpp"), "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "mark host check: ok" in run.stdout
