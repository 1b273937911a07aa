"""csrc/class_batch.h without a GPU: tests/class_batch_check.cpp (its own main, a stub mfx_fail) is compiled with the host
compiler and -fsanitize=address,undefined and run as a child process; nothing is loaded into Python.  The program checks
the binning (order, the two error texts, the first offending voxel), the chunk walk at chunk sizes 1, 4 and whole bins -
the only place the multi-chunk walk runs at a small size: the entry points' byte budgets put a chunk boundary at millions
of voxels - and the row gather and scatter.  What it checks is listed in its source."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "class_batch_check.cpp")


def host_compiler():
    for cxx in (os.environ.get("CXX"), "g++", "clang++", "/opt/rocm/llvm/bin/clang++", "c++"):
        if cxx and shutil.which(cxx):
            return shutil.which(cxx)
    return None


def test_class_batch_under_sanitizers(tmp_path):
    cxx = host_compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler found")
    exe = str(tmp_path / "class_batch_check")
    # the sanitizers' runtimes are linked into the program (clang's default), so that it starts whatever else its
    # environment loads first
    is_clang = "clang" in subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout
    static = [] if is_clang else ["-static-libasan", "-static-libubsan"]
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all"] + static + [SRC, "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(run.stdout)
    assert run.returncode == 0 and run.stdout.strip() == "ok" and run.stderr == "", run.stdout + run.stderr
