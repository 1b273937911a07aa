#!/usr/bin/env python3
"""Timing of the weighted fit, posterior and profile of 2-D protocols on the MI355X (engine.fit2d_weighted_dev,
posterior2d_dev / profile2d_dev with d_W; csrc/w2d.hip).

Sizes (N, M): (200, 66) on the synthetic axis protocol, (512, 1776) and (1024, 1776) on the fixture protocol, both from
tests/golden/rot2d_cases.npz, analytic atoms, V two-fascicle voxels (noisy mixtures of rotated atoms), per-voxel 0/1
masks dropping a tenth of the rows.  Per size and entry point: warm-up at the timed shape, then `--iters` calls between
two events, repeated `--repeats` times (the median is reported).  Beside it
  the earlier route   engine.rotate2d_dev per voxel, rows scaled on the host, mf_utils.solve_exhaustive_posweights voxel
                      by voxel on the materialised dictionaries, on `--parent-vox` voxels (the atoms must agree)
  the unweighted kernels of the same run   fit2d_dev / posterior2d_dev / profile2d_dev on the same voxels

One JSON line per size, appended to --out (default profiles/w2d_dev_time.jsonl): voxels/s of the three weighted entry
points, their ratio to the earlier route (fit) and to the unweighted kernels.  The one gate, asserted here: the weighted
fit is faster than the earlier route at every size.  The ratio to the unweighted kernels is reported, not gated.

Usage: python tools/dev_time_w2d.py [--sizes 200x66,512x1776,1024x1776] [--V 512] [--iters 3] [--repeats 5] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from dev_time_fit2d import atoms, voxels  # noqa: E402


def timed(torch, call, iters, repeats):
    call()                                             # warm-up at the timed shape
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            call()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) / 1e3 / iters)
    return float(np.median(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="200x66,512x1776,1024x1776")
    ap.add_argument("--V", type=int, default=512)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--parent-vox", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "w2d_dev_time.jsonl"))
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
        rng = np.random.default_rng(1)
        V = a.V
        Y, peaks = voxels(T, rng, V, 0.1 if M == 66 else 0.3)
        W = np.ones((V, M))
        for v in range(V):
            W[v, rng.choice(M, M // 10, replace=False)] = 0.0
        dY, dp, dW = torch.from_numpy(Y).cuda(), torch.from_numpy(peaks).cuda(), torch.from_numpy(W).cuda()
        out, st, wst = engine.fit2d_weighted_dev(T, dY, dW, dp, 2)
        torch.cuda.synchronize()
        assert int(st[:, 0].abs().sum()) == 0 and int(wst.abs().sum()) == 0 and bool(torch.isfinite(out).all())
        sse = out[:, -2] * dW.sum(dim=1)
        dT = (2.0 * sse / (M - M // 10 - 2)).contiguous()
        s = {"wfit": timed(torch, lambda: engine.fit2d_weighted_dev(T, dY, dW, dp, 2, out=out), a.iters, a.repeats),
             "fit": timed(torch, lambda: engine.fit2d_dev(T, dY, dp, 2), a.iters, a.repeats),
             "wpost": timed(torch, lambda: engine.posterior2d_dev(T, dY, dp, 2, dT, sse, d_W=dW), a.iters, a.repeats),
             "post": timed(torch, lambda: engine.posterior2d_dev(T, dY, dp, 2, dT, sse), a.iters, a.repeats),
             "wprof": timed(torch, lambda: engine.profile2d_dev(T, dY, dp, 2, d_W=dW), a.iters, a.repeats),
             "prof": timed(torch, lambda: engine.profile2d_dev(T, dY, dp, 2), a.iters, a.repeats)}
        w, ls, pst, _ = engine.posterior2d_dev(T, dY, dp, 2, dT, sse, d_W=dW)
        torch.cuda.synchronize()
        assert int(pst.abs().sum()) == 0
        # the earlier route: device-resident rotation, rows scaled on the host, the explicit solver voxel by voxel
        nv = min(a.parent_vox, V)
        sizes = np.array([N, N])
        host = out.cpu().numpy()
        t0 = time.perf_counter()
        for v in range(nv):
            D, _ = engine.rotate2d_dev(T, dp[v].reshape(2, 3).contiguous())
            sq = np.sqrt(W[v])
            A = np.ascontiguousarray(sq[:, None] * np.hstack(list(D.cpu().numpy())))
            _, sub, _, _, _ = U.solve_exhaustive_posweights(A, sq * Y[v], sizes)
            assert np.array_equal(sub, host[v, 3:5].astype(np.int64)), (v, sub, host[v, 3:5])
        parent = (time.perf_counter() - t0) / nv
        res = {"what": "w2d_k2", "N": N, "M": M, "V": V, "iters": a.iters, "repeats": a.repeats,
               "wfit_voxels_per_s": V / s["wfit"], "wpost_voxels_per_s": V / s["wpost"], "wprofile_voxels_per_s": V / s["wprof"],
               "parent_route_s_per_voxel": parent, "parent_route_voxels": nv, "wfit_ratio_to_parent_route": parent / (s["wfit"] / V),
               "wfit_time_over_fit2d_dev": s["wfit"] / s["fit"], "wpost_time_over_posterior2d_dev": s["wpost"] / s["post"],
               "wprofile_time_over_profile2d_dev": s["wprof"] / s["prof"],
               "fit2d_voxels_per_s": V / s["fit"], "posterior2d_voxels_per_s": V / s["post"], "profile2d_voxels_per_s": V / s["prof"]}
        line = json.dumps(res)
        print(line, flush=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")
        assert res["wfit_ratio_to_parent_route"] > 1.0, "the weighted fit is slower than the earlier route at N = %d, M = %d" % (N, M)
        T.close()


if __name__ == "__main__":
    main()
