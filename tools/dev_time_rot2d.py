#!/usr/bin/env python3
"""Timing of the 2-D protocol rotation on the MI355X (RotateAtom2DTables.rotate and engine.rotate2d_dev).

Fixture protocol (1776 rows, 9 (Delta, delta) pairs) from tests/golden/rot2d_cases.npz, N atoms, B directions
(|d_z| >= 0.1).  Prints one JSON line (appended to --out): directions/s of the host path (copy back included)
and of the device path (events around the two kernels), and the evaluation kernel's effective bytes/s computed
from shapes (output bytes plus table bytes read once) over the device path's time.  Kernel times come from a
separate `rocprofv3 --kernel-trace --stats` run of this script (--iters 3).  --ref-cpu DIR times the reference's
rotate_atom_2Dprotocol per direction on the CPU (DIR: the reference checkout; build machine only).

Usage: python tools/dev_time_rot2d.py [--N 1024] [--B 256] [--iters 10] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def setup(N, B):
    from microstructure_fingerprinting_amd import mf_utils as U
    d = np.load(os.path.join(ROOT, "tests", "golden", "rot2d_cases.npz"))
    sch = d["fix_sch"]
    sig = d["fix_sig"][:, np.arange(N) % 3] * (1.0 + 1e-3 * np.arange(N))
    rng = np.random.default_rng(0)
    v = rng.standard_normal((4 * B, 3))
    v /= np.sqrt(np.sum(v ** 2, axis=1, keepdims=True))
    dirs = np.ascontiguousarray(v[np.abs(v[:, 2]) >= 0.1][:B])
    return U, sch, sig, dirs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=1024)
    ap.add_argument("--B", type=int, default=256)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--ref-cpu", default=None)
    a = ap.parse_args()
    U, sch, sig, dirs = setup(a.N, a.B)
    res = {"what": "rot2d", "M": int(sch.shape[0]), "N": a.N, "B": a.B}
    if a.ref_cpu:
        sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
        import gen_golden
        gen_golden.REF = a.ref_cpu
        mfu, _ = gen_golden.import_reference()
        t0 = time.perf_counter()
        for k in range(4):
            mfu.rotate_atom_2Dprotocol(sig.copy(), sch.copy(), np.array([0.0, 0.0, 1.0]), dirs[k], 2.2e-9)
        res["ref_cpu_s_per_direction"] = (time.perf_counter() - t0) / 4
        print(json.dumps(res), flush=True)
        return
    import torch
    from microstructure_fingerprinting_amd import engine
    T = U.RotateAtom2DTables(sig, sch, np.array([0.0, 0.0, 1.0]), 2.2e-9)
    T.rotate(dirs[:4])                                       # warm-up: tables to HBM, code objects
    t0 = time.perf_counter()
    for _ in range(a.iters):
        T.rotate(dirs)
    res["host_dirs_per_s"] = a.B * a.iters / (time.perf_counter() - t0)
    dd = torch.from_numpy(dirs).cuda()
    out, st = engine.rotate2d_dev(T, dd)                     # warm-up at the timed shape
    torch.cuda.synchronize()
    assert int(st[:, 0].abs().sum()) == 0 and bool(torch.isfinite(out).all())
    del out
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.iters):
        out, st = engine.rotate2d_dev(T, dd)
    e1.record()
    torch.cuda.synchronize()
    s = e0.elapsed_time(e1) / 1e3 / a.iters
    res["dev_s_per_call"] = s
    res["dev_dirs_per_s"] = a.B / s
    out_bytes = 8.0 * a.B * T.M * T.N
    table_bytes = 8.0 * (2 * T._arrays["ky"].size + T._arrays["cst"].size)
    res["out_GB"] = out_bytes / 1e9
    res["dev_path_TBps_effective"] = (out_bytes + table_bytes) / s / 1e12
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
