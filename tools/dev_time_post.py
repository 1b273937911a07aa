#!/usr/bin/env python3
"""Timing of the soft fits on the MI355X (engine.posterior_dev) beside the objective profiles (engine.profile_dev) on
the same voxels, HIP events on a warm device.

profile_dev is the yardstick: it does the same matrix work (every atom pair of the voxel on the FP64 MFMA) and keeps
a minimum where the posterior keeps a sum of exponentials - one division and one FP64 exp more per pair.

The shape: 782 atoms, 200 measurements, V voxels per launch (default 512).  Classes: two fascicles, two fascicles +
CSF, one fascicle.  Within a round the two entry points alternate; the warm-up runs at the timed shape.  One JSON line
per class is appended to --out: medians over the rounds of the time per launch, both rates in voxels per second and
their ratio (posterior rate / profile rate).

Usage: python tools/dev_time_post.py [--V 512] [--N 782] [--iters 10] [--rounds 5] [--out profiles/post_dev_time.jsonl]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--V", type=int, default=512)
    ap.add_argument("--N", type=int, default=782)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "post_dev_time.jsonl"))
    a = ap.parse_args()
    import torch
    from microstructure_fingerprinting_amd import engine, synth
    from microstructure_fingerprinting_amd import mf_utils as mfu
    sch, dic, rng = synth.make_model("C2", N=a.N)
    ms = mfu.init_PGSE_multishell_interp(dic, sch, np.array([0.0, 0.0, 1.0]))
    plan = ms.plan_for(sch)
    V, M, N = a.V, sch.shape[0], a.N
    b = (synth.GAMMA_H * sch[:, 3] * sch[:, 5]) ** 2 * (sch[:, 4] - sch[:, 5] / 3)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()  # noqa: E731
    d_csf = t(np.exp(-sch[:, 6] / 2.0) * np.exp(-b * 3.0e-9))
    pk = np.concatenate([synth.unit_vectors(rng, V), synth.unit_vectors(rng, V)], axis=1)
    d_pk = t(pk)
    d_pk1 = d_pk[:, :3].contiguous()
    nu = rng.dirichlet(np.ones(3), V)
    d_Y = torch.zeros((V, M), dtype=torch.float64, device="cuda")
    for k in range(2):
        ids = t(rng.integers(0, N, V).astype(np.int32))
        d_Y += 500.0 * t(nu[:, k:k + 1]) * engine.rotate_columns_dev(plan, d_pk[:, 3 * k:3 * k + 3].contiguous(), ids)
    d_Y += 500.0 * t(nu[:, 2:3]) * d_csf[None, :]
    sigma = 500.0 / 30.0
    d_Y += sigma * torch.randn((V, M), dtype=torch.float64, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
    d_Y = d_Y.contiguous()
    d_T = torch.full((V,), 2.0 * sigma ** 2, dtype=torch.float64, device="cuda")
    out2 = torch.empty((V, 2, N), dtype=torch.float64, device="cuda")
    out1 = torch.empty((V, 1, N), dtype=torch.float64, device="cuda")
    classes = {"k2": (d_pk, 2, False, out2), "k2_csf": (d_pk, 2, True, out2), "k1": (d_pk1, 1, False, out1)}
    shifts, last = {}, {}

    def profile(c):
        p, K, csf, out = classes[c]
        return engine.profile_dev(plan, d_Y, p, K, csf, d_csf if csf else None, out=out)

    def posterior(c):
        p, K, csf, _ = classes[c]
        last[c] = engine.posterior_dev(plan, d_Y, p, K, d_T, shifts[c], csf, d_csf if csf else None)

    for c in classes:   # the shift is each voxel's smallest profile value; warm-up at the timed shape
        shifts[c] = profile(c).amin(dim=(1, 2)).contiguous()
        posterior(c)
    torch.cuda.synchronize()
    for c in classes:
        w, log_sum, status = last[c]
        assert int(status.abs().sum()) == 0 and bool(torch.isfinite(w).all()) and bool(torch.isfinite(log_sum).all()), c
    times = {(c, f.__name__): [] for c in classes for f in (profile, posterior)}
    for _ in range(a.rounds):
        for c in classes:
            for f in (profile, posterior):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.iters):
                    f(c)
                e1.record()
                torch.cuda.synchronize()
                times[(c, f.__name__)].append(e0.elapsed_time(e1) / 1e3 / a.iters)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    for c in classes:
        tp, tq = float(np.median(times[(c, "profile")])), float(np.median(times[(c, "posterior")]))
        res = {"what": "posterior_dev beside profile_dev", "class": c, "V": V, "M": M, "N": N, "iters": a.iters, "rounds": a.rounds,
               "profile_s_per_launch": tp, "posterior_s_per_launch": tq,
               "posterior_s_per_launch_min_max": [float(min(times[(c, "posterior")])), float(max(times[(c, "posterior")]))],
               "profile_voxels_per_s": V / tp, "posterior_voxels_per_s": V / tq, "posterior_over_profile_rate": tp / tq}
        line = json.dumps(res)
        print(line, flush=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
