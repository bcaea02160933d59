"""The G.711 companding of llmvox_amd/csrc/pcm_host.h without a GPU and without Python in the way: tests/host/g711_check.cpp,
a program of its own, built with the system compiler under AddressSanitizer and UBSan, runs all 65,536 inputs and all
256 codes through the functions lvx_pcm_g711_encode / lvx_pcm_g711_decode and the kernel's epilogue share, holds them to
the header's rule written a second time, and covers n = 0 and the argument errors. Exit status 0: every check held and no
sanitizer spoke."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_g711_check(tmp_path):
    cxx = shutil.which("g++")
    assert cxx is not None, "no g++ to build the check program with"
    exe = str(tmp_path / "g711_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall",
                    "-Werror", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "llmvox_amd", "csrc"),
                    os.path.join(ROOT, "tests", "host", "g711_check.cpp"), "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "g711 host check: ok" in run.stdout
