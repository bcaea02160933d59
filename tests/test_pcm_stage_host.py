"""The PCM stages' host skeleton (llmvox_amd/csrc/pcm_host.h) without a GPU: tests/host/pcm_stage_check.cpp, a program
of its own, built with the system compiler under AddressSanitizer and UBSan, drives every stage's planning, commit and
packets through refused calls, consecutive and final calls, 33 rows, the identity cases and the level's volume 0, and
checks the counts against the header's closed forms. Exit status 0: every check held and no sanitizer spoke."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pcm_stage_check(tmp_path):
    cxx = shutil.which("g++")
    assert cxx is not None, "no g++ to build the check program with"
    exe = str(tmp_path / "pcm_stage_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall",
                    "-Werror", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "llmvox_amd", "csrc"),
                    os.path.join(ROOT, "tests", "host", "pcm_stage_check.cpp"), "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "pcm stage host check: ok" in run.stdout
