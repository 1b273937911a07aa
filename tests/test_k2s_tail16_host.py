"""csrc/k2s_tail16_map.h without a GPU: the index maps of the screening kernel's 16-row form (v_mfma_f32_16x16x32_f16 for a
last row tile of at most 16 atoms).  tests/k2s_tail16_map_check.cpp (its own main) is compiled with the host compiler and
-fsanitize=address,undefined and run as a child process; nothing is loaded into Python.  For KS = 4, 8, 13 and 16 it checks
that every (row < MP, atom) of a tile is produced exactly once, that no row >= MP is ever formed (KS = 13: the half-empty
last step), that the C map is a bijection onto 16 x 16, and that even / odd atoms land in sub-tiles 0 / 1."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "k2s_tail16_map_check.cpp")


def host_compiler():
    for cxx in (os.environ.get("CXX"), "g++", "clang++", "/opt/rocm/llvm/bin/clang++", "c++"):
        if cxx and shutil.which(cxx):
            return shutil.which(cxx)
    return None


def test_tail16_maps_under_sanitizers(tmp_path):
    cxx = host_compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler found")
    exe = str(tmp_path / "k2s_tail16_map_check")
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
