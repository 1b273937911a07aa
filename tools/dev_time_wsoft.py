#!/usr/bin/env python3
"""Cost of the weighted posterior and profile kernels beside their unweighted forms on the MI355X (csrc/posterior.hip,
csrc/profile.hip, include/mfx_wsoft.h).

N = 782 atoms on the C2 protocol of synth.py (M = 200), K = 2, CSF off and on, V two-fascicle voxels (noisy mixtures of
rotated atoms) with real-valued weights in [0, 4], about 15 % of them zero.  Per kernel: warm-up at the timed shape,
then the unweighted and the weighted call alternate, `--iters` calls between two events each, `--repeats` times; the medians,
the spread and the ratio of the medians are reported.  With W = 1 the weighted call's results are asserted equal to the
unweighted call's, bit for bit.

One JSON line per (kernel, csf), appended to --out (default profiles/wsoft_dev_time.jsonl).

Usage: python tools/dev_time_wsoft.py [--N 782] [--V 2048] [--iters 5] [--repeats 7] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
Z = np.array([0.0, 0.0, 1.0])


def alternate(fa, fb, iters, repeats):
    """seconds per call of fa and fb, alternating: (median a, min a, max a, median b, min b, max b)"""
    import torch
    fa(); fb()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(repeats):
        for fn, acc in ((fa, ta), (fb, tb)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                fn()
            e1.record()
            torch.cuda.synchronize()
            acc.append(e0.elapsed_time(e1) / 1e3 / iters)
    return (float(np.median(ta)), float(min(ta)), float(max(ta)), float(np.median(tb)), float(min(tb)), float(max(tb)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=782)
    ap.add_argument("--V", type=int, default=2048)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wsoft_dev_time.jsonl"))
    a = ap.parse_args()
    import torch
    from microstructure_fingerprinting_amd import _lib, engine, synth
    from microstructure_fingerprinting_amd import mf_utils as U
    lib = _lib.lib()
    N, V = a.N, a.V
    sch, dic, _ = synth.make_model("C2", N)
    M = sch.shape[0]
    ms = U.init_PGSE_multishell_interp(dic, sch, Z)
    plan = ms.plan_for(sch)
    rng = np.random.default_rng(1)
    peaks = np.concatenate([synth.unit_vectors(rng, V), synth.unit_vectors(rng, V)], axis=1)
    dp = torch.from_numpy(peaks).cuda()
    ids = rng.integers(0, N, (V, 2)).astype(np.int32)
    f = torch.from_numpy(rng.uniform(0.3, 0.7, (V, 1))).cuda()
    c0 = engine.rotate_columns_dev(plan, dp[:, :3].contiguous(), torch.from_numpy(ids[:, 0].copy()).cuda())
    c1 = engine.rotate_columns_dev(plan, dp[:, 3:].contiguous(), torch.from_numpy(ids[:, 1].copy()).cuda())
    sigma = 500.0 / 30.0
    dY = (500.0 * (f * c0 + (1.0 - f) * c1) + sigma * torch.from_numpy(rng.normal(0, 1, (V, M))).cuda()).contiguous()
    W = rng.uniform(0.0, 4.0, (V, M))
    W[rng.random((V, M)) < 0.15] = 0.0
    dW, dW1 = torch.from_numpy(W).cuda(), torch.ones((V, M), dtype=torch.float64, device="cuda")
    b = (synth.GAMMA_H * sch[:, 3] * sch[:, 5]) ** 2 * (sch[:, 4] - sch[:, 5] / 3)
    dx = torch.from_numpy(np.exp(-sch[:, 6] / 2.0) * np.exp(-b * 3.0e-9)).cuda()
    dT = torch.full((V,), 2.0 * sigma ** 2, dtype=torch.float64, device="cuda")
    for csf in (False, True):
        x = dx if csf else None
        limits = {"post": (lib.mfx_post_max_atoms(plan.handle(), int(csf)), lib.mfx_wsoft_max_atoms(plan.handle(), int(csf), 0)),
                  "profile": (lib.mfx_profile_max_atoms(plan.handle(), int(csf), 0), lib.mfx_wsoft_max_atoms(plan.handle(), int(csf), 1))}
        # shifts: each problem's own minimum, from its profile
        sh_u = engine.profile_dev(plan, dY, dp, 2, csf, x)[:, 0].min(dim=1).values.contiguous()
        sh_w = engine.profile_dev(plan, dY, dp, 2, csf, x, d_W=dW)[:, 0].min(dim=1).values.contiguous()
        # W = 1: the same bits
        pu = engine.posterior_dev(plan, dY, dp, 2, dT, sh_u, csf, x)
        p1 = engine.posterior_dev(plan, dY, dp, 2, dT, sh_u, csf, x, d_W=dW1)
        ou = engine.profile_dev(plan, dY, dp, 2, csf, x)
        o1 = engine.profile_dev(plan, dY, dp, 2, csf, x, d_W=dW1)
        pw = engine.posterior_dev(plan, dY, dp, 2, dT, sh_w, csf, x, d_W=dW)
        torch.cuda.synchronize()
        assert int(pu[2].abs().sum()) == 0 and int(pw[2].abs().sum()) == 0
        assert torch.equal(pu[0], p1[0]) and torch.equal(pu[1], p1[1]) and torch.equal(ou, o1)
        runs = {"post": (lambda: engine.posterior_dev(plan, dY, dp, 2, dT, sh_u, csf, x),
                         lambda: engine.posterior_dev(plan, dY, dp, 2, dT, sh_w, csf, x, d_W=dW)),
                "profile": (lambda: engine.profile_dev(plan, dY, dp, 2, csf, x, out=ou),
                            lambda: engine.profile_dev(plan, dY, dp, 2, csf, x, out=o1, d_W=dW))}
        for what, (fu, fw) in runs.items():
            u, umin, umax, w, wmin, wmax = alternate(fu, fw, a.iters, a.repeats)
            res = {"what": "wsoft_" + what, "N": N, "M": M, "V": V, "csf": csf, "iters": a.iters, "repeats": a.repeats,
                   "unweighted_s_median": u, "unweighted_s_min": umin, "unweighted_s_max": umax,
                   "weighted_s_median": w, "weighted_s_min": wmin, "weighted_s_max": wmax, "weighted_over_unweighted": w / u,
                   "unweighted_voxels_per_s": V / u, "weighted_voxels_per_s": V / w,
                   "max_atoms_unweighted": limits[what][0], "max_atoms_weighted": limits[what][1]}
            line = json.dumps(res)
            print(line, flush=True)
            if a.out:
                os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                with open(a.out, "a") as fh:
                    fh.write(line + "\n")


if __name__ == "__main__":
    main()
