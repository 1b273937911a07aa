"""csrc/boot_batch.h without a GPU: tests/boot_batch_check.cpp (its own main) is compiled with the host compiler and
-fsanitize=address,undefined and run as a child process; nothing is loaded into Python.  The program checks the column maps
of every class in every batch against an expectation written by column names, the scatter of a class chunk into a fake
batch of 11 voxels cell by cell (status 0 and not, B = 1 and 3, Q = 0 and 2, keep null and not, sentinels in the voxels
outside the chunk), the round trip of the own fit's rows through the parameter map, and the voxels-per-upload formula at
its seams - the only place this index arithmetic runs at a small size without a device.  What it checks is listed in its
source."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "boot_batch_check.cpp")


def host_compiler():
    for cxx in (os.environ.get("CXX"), "g++", "clang++", "/opt/rocm/llvm/bin/clang++", "c++"):
        if cxx and shutil.which(cxx):
            return shutil.which(cxx)
    return None


def test_boot_batch_under_sanitizers(tmp_path):
    cxx = host_compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler found")
    exe = str(tmp_path / "boot_batch_check")
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
