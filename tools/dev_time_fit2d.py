#!/usr/bin/env python3
"""Timing of the fused two-fascicle fit of 2-D protocols on the MI355X (engine.fit2d_dev, csrc/fit2d.hip).

Sizes (N, M): (200, 66) on the synthetic axis protocol, (512, 1776) and (1024, 1776) on the fixture protocol, both
from tests/golden/rot2d_cases.npz, analytic atoms, V two-fascicle voxels (noisy mixtures of rotated atoms) - V large
enough to give every CU several workgroups.  Per size: warm-up at the timed shape, then `--iters` calls between two
events, repeated `--repeats` times (median and spread are reported).  Beside it the only route the library had
before: engine.rotate2d_dev, then mf_utils.solve_exhaustive_posweights voxel by voxel on the materialised
dictionaries (a host round trip and a dozen launches per voxel), on `--parent-vox` voxels.

One JSON line per size, appended to --out: voxels/s, the ratio to that route, the fraction of the FP64-matrix roof
(2 N^2 M flop per voxel at 78 TFLOP/s) and the bytes/s of table reads the cross-Gram phase generates (every
128 x 128 block reads slope and knot value of 256 atoms per row: 2 * 8 B * 256 * M per block).

Usage: python tools/dev_time_fit2d.py [--sizes 200x66,512x1776,1024x1776] [--V 512] [--iters 3] [--repeats 5] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GAM = 2 * np.pi * 42.577480e6
ROOF = 78e12


def atoms(sch, N, seed):
    rng = np.random.default_rng(seed)
    G, Dl, dl = sch[:, 3], sch[:, 4], sch[:, 5]
    b = (GAM * G * dl) ** 2 * (Dl - dl / 3)
    D = rng.uniform(0.3e-9, 2.5e-9, N)
    a = rng.uniform(-0.2, 0.2, (2, N))
    return np.exp(-np.outer(b, D)) * (1 + np.outer(G * sch[:, 0], a[0]) / 0.1 + np.outer(G * sch[:, 1], a[1]) / 0.1)


def voxels(T, rng, V, zmin):
    v = rng.standard_normal((16 * V, 3))
    v /= np.sqrt(np.sum(v ** 2, axis=1, keepdims=True))
    d = np.ascontiguousarray(v[np.abs(v[:, 2]) >= zmin][:2 * V])
    ids = rng.integers(0, T.N, 2 * V)
    cols = np.concatenate([T.rotate_cols(d[i:i + 256], ids[i:i + 256]) for i in range(0, 2 * V, 256)])
    f = rng.uniform(0.3, 0.7, V)[:, None]
    clean = f * cols[0::2] + (1.0 - f) * cols[1::2]
    s = 1.0 / 30.0
    Y = np.sqrt((clean + s * rng.standard_normal(clean.shape)) ** 2 + (s * rng.standard_normal(clean.shape)) ** 2)
    return Y, np.ascontiguousarray(d.reshape(V, 6))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="200x66,512x1776,1024x1776")
    ap.add_argument("--V", type=int, default=512)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--parent-vox", type=int, default=4)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from microstructure_fingerprinting_amd import engine
    from microstructure_fingerprinting_amd import mf_utils as U
    d = np.load(os.path.join(ROOT, "tests", "golden", "rot2d_cases.npz"))
    for size in a.sizes.split(","):
        N, M = (int(x) for x in size.split("x"))
        sch = d["syn2_sch"] if M == 66 else d["fix_sch"]
        assert sch.shape[0] == M
        T = U.RotateAtom2DTables(atoms(sch, N, 5), sch, np.array([0.0, 0.0, 1.0]), 2.2e-9)
        Y, peaks = voxels(T, np.random.default_rng(1), a.V, 0.1 if M == 66 else 0.3)
        dY, dp = torch.from_numpy(Y).cuda(), torch.from_numpy(peaks).cuda()
        out, st = engine.fit2d_dev(T, dY, dp, 2)                      # warm-up at the timed shape
        torch.cuda.synchronize()
        assert int(st[:, 0].abs().sum()) == 0 and bool(torch.isfinite(out).all())
        times = []
        for _ in range(a.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.iters):
                engine.fit2d_dev(T, dY, dp, 2, out=out)
            e1.record()
            torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1) / 1e3 / a.iters)
        s = float(np.median(times))
        # the route before this kernel: device-resident rotation, then the explicit solver voxel by voxel
        nv = min(a.parent_vox, a.V)
        sizes = np.array([N, N])
        host = out.cpu().numpy()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for v in range(nv):
            D, _ = engine.rotate2d_dev(T, dp[v].reshape(2, 3).contiguous())
            A = np.ascontiguousarray(np.hstack(list(D.cpu().numpy())))
            w, sub, _, obj, _ = U.solve_exhaustive_posweights(A, Y[v], sizes)
            assert np.array_equal(sub, host[v, 3:5].astype(np.int64)), (v, sub, host[v, 3:5])
        parent = (time.perf_counter() - t0) / nv
        nblk = (N + 127) // 128
        table_bytes = nblk * nblk * 2 * 8.0 * 256 * M
        res = {"what": "fit2d_k2", "N": N, "M": M, "V": a.V, "iters": a.iters, "repeats": a.repeats,
               "s_per_call_median": s, "s_per_call_min": float(min(times)), "s_per_call_max": float(max(times)),
               "voxels_per_s": a.V / s, "parent_route_s_per_voxel": parent, "parent_route_voxels": nv,
               "ratio_to_parent_route": parent / (s / a.V),
               "roof_fraction": (2.0 * N * N * M / ROOF) / (s / a.V),
               "gram_table_read_TBps": table_bytes * a.V / s / 1e12}
        line = json.dumps(res)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")
        T.close()


if __name__ == "__main__":
    main()
