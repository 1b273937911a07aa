#!/usr/bin/env python3
"""Timing of the soft fits and objective profiles of 2-D protocols on the MI355X (engine.posterior2d_dev /
profile2d_dev, csrc/soft2d.hip).

Sizes (N, M): (200, 66) on the synthetic axis protocol, (512, 1776) and (1024, 1776) on the fixture protocol, both from
tests/golden/rot2d_cases.npz, analytic atoms, 512 two-fascicle voxels (noisy mixtures of rotated atoms) at the fit's
residual variance.  Per size: warm-up at the timed shape, then `--iters` calls between two events, repeated `--repeats`
times (median and spread are reported).

Two yardsticks taken in the same run:
  (a) the route a user had before: engine.rotate2d_dev for both directions, the Gram by torch.matmul, the closed form
      (the cut included), exp and the sums in torch FP64 on the device, voxel by voxel, on `--route-vox` voxels.  Gate:
      both new kernels are faster at every size.
  (b) engine.fit2d_dev on the same voxels: the same 2 N^2 M matrix work with a scan in place of N^2 exponentials.  The
      ratio is reported without a gate.

One JSON line per size, appended to --out (default profiles/soft2d_dev_time.jsonl).

Usage: python tools/dev_time_soft2d.py [--sizes 200x66,512x1776,1024x1776] [--V 512] [--iters 3] [--repeats 5] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from dev_time_fit2d import ROOF, atoms, voxels  # noqa: E402

CUT = 1e-8


def torch_route(T, dY, dp, dT, dshift, nv):
    """yardstick (a): per voxel, weights and row minima from materialised dictionaries in torch FP64"""
    import torch
    from microstructure_fingerprinting_amd import engine
    ws, objs = [], []
    for v in range(nv):
        D, _ = engine.rotate2d_dev(T, dp[v].reshape(2, 3).contiguous())
        y = dY[v]
        A11, A22, A12 = (D[0] * D[0]).sum(0)[:, None], (D[1] * D[1]).sum(0)[None, :], D[0].T @ D[1]
        Y1, Y2 = (D[0].T @ y)[:, None], (D[1].T @ y)[None, :]
        d1, d2, pd = A22 * Y1 - A12 * Y2, A11 * Y2 - A12 * Y1, A11 * A22
        det = pd - A12 * A12
        single = torch.maximum(Y1.clamp(min=0) ** 2 / A11, Y2.clamp(min=0) ** 2 / A22)
        s = torch.where((d1 > 0) & (d2 > 0) & (det > CUT * pd), (Y1 * d1 + Y2 * d2) / det, single)
        F = (y * y).sum() - s
        t = torch.exp(-(F - dshift[v]) / dT[v])
        Z = t.sum()
        ws.append(torch.stack([t.sum(1) / Z, t.sum(0) / Z]))
        objs.append(torch.stack([F.min(1).values, F.min(0).values]))
    return torch.stack(ws), torch.stack(objs)


def timed(fn, iters, repeats):
    import torch
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) / 1e3 / iters)
    return float(np.median(times)), float(min(times)), float(max(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="200x66,512x1776,1024x1776")
    ap.add_argument("--V", type=int, default=512)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--route-vox", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "soft2d_dev_time.jsonl"))
    a = ap.parse_args()
    import torch
    from microstructure_fingerprinting_amd import engine
    from microstructure_fingerprinting_amd import mf_utils as U
    d = np.load(os.path.join(ROOT, "tests", "golden", "rot2d_cases.npz"))
    gate = True
    for size in a.sizes.split(","):
        N, M = (int(x) for x in size.split("x"))
        sch = d["syn2_sch"] if M == 66 else d["fix_sch"]
        assert sch.shape[0] == M
        T = U.RotateAtom2DTables(atoms(sch, N, 5), sch, np.array([0.0, 0.0, 1.0]), 2.2e-9)
        V = a.V
        Y, peaks = voxels(T, np.random.default_rng(1), V, 0.1 if M == 66 else 0.3)
        dY, dp = torch.from_numpy(Y).cuda(), torch.from_numpy(peaks).cuda()
        fit, st = engine.fit2d_dev(T, dY, dp, 2)
        torch.cuda.synchronize()
        assert int(st[:, 0].abs().sum()) == 0
        dshift = (fit[:, -2] * M).contiguous()
        dT = (2.0 * dshift / (M - 2)).contiguous()
        w, ls, pst, _ = engine.posterior2d_dev(T, dY, dp, 2, dT, dshift)
        obj, _, _ = engine.profile2d_dev(T, dY, dp, 2)
        torch.cuda.synchronize()
        assert int(pst.abs().sum()) == 0 and bool(torch.isfinite(w).all()) and bool(torch.isfinite(obj).all())
        s_post = timed(lambda: engine.posterior2d_dev(T, dY, dp, 2, dT, dshift), a.iters, a.repeats)
        s_prof = timed(lambda: engine.profile2d_dev(T, dY, dp, 2, out=obj), a.iters, a.repeats)
        s_fit = timed(lambda: engine.fit2d_dev(T, dY, dp, 2, out=fit), a.iters, a.repeats)
        nv = min(a.route_vox, V)
        rw, robj = torch_route(T, dY, dp, dT, dshift, nv)
        torch.cuda.synchronize()
        err_w = float((rw - w[:nv]).abs().max())
        err_o = float(((robj - obj[:nv]).abs() / (dY[:nv] * dY[:nv]).sum(1)[:, None, None]).max())
        s_route = timed(lambda: torch_route(T, dY, dp, dT, dshift, nv), 1, a.repeats)
        per_vox = s_route[0] / nv
        res = {"what": "soft2d_k2", "N": N, "M": M, "V": V, "iters": a.iters, "repeats": a.repeats,
               "post_s_per_call_median": s_post[0], "post_s_per_call_min": s_post[1], "post_s_per_call_max": s_post[2],
               "prof_s_per_call_median": s_prof[0], "prof_s_per_call_min": s_prof[1], "prof_s_per_call_max": s_prof[2],
               "post_voxels_per_s": V / s_post[0], "prof_voxels_per_s": V / s_prof[0],
               "torch_route_s_per_voxel": per_vox, "torch_route_voxels": nv, "torch_route_voxels_per_s": 1.0 / per_vox,
               "post_ratio_to_torch_route": per_vox / (s_post[0] / V), "prof_ratio_to_torch_route": per_vox / (s_prof[0] / V),
               "torch_route_max_abs_weight_difference": err_w, "torch_route_max_obj_difference_over_ysq": err_o,
               "fit2d_voxels_per_s": V / s_fit[0], "post_time_over_fit2d": s_post[0] / s_fit[0],
               "prof_time_over_fit2d": s_prof[0] / s_fit[0],
               "post_roof_fraction": (2.0 * N * N * M / ROOF) / (s_post[0] / V),
               "gate_faster_than_torch_route": bool(per_vox > s_post[0] / V and per_vox > s_prof[0] / V)}
        gate = gate and res["gate_faster_than_torch_route"]
        line = json.dumps(res)
        print(line, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as fh:
                fh.write(line + "\n")
        T.close()
    assert gate, "a new kernel is not faster than the torch route at some size"


if __name__ == "__main__":
    main()
