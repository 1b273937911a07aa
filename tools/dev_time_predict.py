#!/usr/bin/env python3
"""Timing of the forward model on the MI355X (engine.predict_dev), HIP events on a warm device.

V voxels, M = 200 rows (the benchmark's three-shell protocol), N atoms, two fascicles and CSF per voxel:
  a  predict_dev
  b  predict_dev with fused noise (one coil, sigma = M0 / 30 per voxel)
  c  predict_dev with fused residual (sum of squares and R2 per voxel against data)
  d  the composition synth.make_phantom uses: rotate_columns_dev per fascicle, torch element-wise passes over
     [V, M], torch.randn
Each variant is warmed up at the timed shape, then timed --rounds times over --iters calls, the variants alternating
within a round.  Prints one JSON line per variant (appended to --out): the median, minimum and maximum over the
rounds of the time per call, and the effective rate of the V M 8 bytes written at the median.

Usage: python tools/dev_time_predict.py [--V 100000] [--N 1024] [--iters 500] [--rounds 5] [--out FILE]
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
    ap.add_argument("--V", type=int, default=100000)
    ap.add_argument("--N", type=int, default=1024)
    ap.add_argument("--iters", type=int, default=500)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from microstructure_fingerprinting_amd import engine, synth
    from microstructure_fingerprinting_amd import mf_utils as mfu
    sch, dic, rng = synth.make_model("C2", N=a.N)
    ms = mfu.init_PGSE_multishell_interp(dic, sch, np.array([0.0, 0.0, 1.0]))
    plan = ms.plan_for(sch)
    V, M, N = a.V, sch.shape[0], a.N
    b = (synth.GAMMA_H * sch[:, 3] * sch[:, 5]) ** 2 * (sch[:, 4] - sch[:, 5] / 3)
    sig_csf = np.exp(-sch[:, 6] / 2.0) * np.exp(-b * 3.0e-9)
    P = np.zeros((V, engine.num_params(2, True, False)))
    P[:, 0] = 500.0
    P[:, [1, 2, 5]] = rng.dirichlet(np.ones(3), V)
    P[:, 3:5] = rng.integers(0, N, (V, 2))
    pk = np.concatenate([synth.unit_vectors(rng, V), synth.unit_vectors(rng, V)], axis=1)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()  # noqa: E731
    d_P, d_pk, d_csf = t(P), t(pk), t(sig_csf)
    d_sigma = (d_P[:, 0] / 30.0).contiguous()
    out = torch.empty((V, M), dtype=torch.float64, device="cuda")
    common = dict(csf_on=True, d_sig_csf=d_csf, out=out, check=False)
    d_Y = engine.predict_dev(plan, d_P, d_pk, 2, csf_on=True, d_sig_csf=d_csf, sigma_g=d_sigma, ncoils=1, seed=1)
    d_dirs = [d_pk[:, :3].contiguous(), d_pk[:, 3:].contiguous()]
    d_ids = [d_P[:, 3].to(torch.int32), d_P[:, 4].to(torch.int32)]
    d_nu = [d_P[:, 1:2].contiguous(), d_P[:, 2:3].contiguous(), d_P[:, 5:6].contiguous()]
    gen = torch.Generator(device="cuda").manual_seed(1)

    def composition():   # synth.make_phantom's signal path
        Y = torch.zeros((V, M), dtype=torch.float64, device="cuda")
        for k in range(2):
            Y += d_nu[k] * engine.rotate_columns_dev(plan, d_dirs[k], d_ids[k])
        Y += d_nu[2] * d_csf[None, :]
        return 500.0 * Y + (500.0 / 30.0) * torch.randn((V, M), dtype=torch.float64, device="cuda", generator=gen)

    variants = {
        "a_predict": lambda: engine.predict_dev(plan, d_P, d_pk, 2, **common),
        "b_predict_noise": lambda: engine.predict_dev(plan, d_P, d_pk, 2, sigma_g=d_sigma, ncoils=1, seed=1, **common),
        "c_predict_residual": lambda: engine.predict_dev(plan, d_P, d_pk, 2, d_Y=d_Y, **common),
        "d_composition": composition,
    }
    for f in variants.values():   # warm-up at the timed shape: code objects, allocator
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all())
    times = {k: [] for k in variants}
    for _ in range(a.rounds):
        for name, f in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.iters):
                f()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) / 1e3 / a.iters)
    med = {k: float(np.median(v)) for k, v in times.items()}
    for name in variants:
        res = {"what": "predict", "variant": name, "V": V, "M": M, "N": N, "K": 2, "csf": True, "iters": a.iters,
               "rounds": a.rounds, "s_per_call_median": med[name], "s_per_call_min": float(min(times[name])),
               "s_per_call_max": float(max(times[name])), "out_GB": 8.0 * V * M / 1e9,
               "GBps_effective": 8.0 * V * M / med[name] / 1e9, "speedup_vs_composition": med["d_composition"] / med[name]}
        line = json.dumps(res)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
