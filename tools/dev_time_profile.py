#!/usr/bin/env python3
"""Timing of the objective profiles on the MI355X (engine.profile_dev), HIP events on a warm device.

The benchmark's shape: V voxels (default 1e5), 782 atoms, 200 measurements.  Variants, alternating within a round:
  k2          profile_dev, two fascicles
  k2_csf      profile_dev, two fascicles + CSF
  k1          profile_dev, one fascicle
  fp64_fit    the fit's FP64 kernel over the same two-fascicle voxels (screening off): bench.py --full's `fp64_kernel`
              leg, the pass over the same Gram that the profile is held against
Prints one JSON line per variant (appended to --out): median, minimum and maximum over the rounds of the time per
call, voxels per second at the median, and the rate relative to fp64_fit.

Usage: python tools/dev_time_profile.py [--V 100000] [--N 782] [--iters 2] [--rounds 3] [--out FILE]
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
    ap.add_argument("--N", type=int, default=782)
    ap.add_argument("--iters", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from microstructure_fingerprinting_amd import _lib as L
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
    d_Y += (500.0 / 30.0) * torch.randn((V, M), dtype=torch.float64, device="cuda",
                                        generator=torch.Generator(device="cuda").manual_seed(1))
    d_Y = d_Y.contiguous()
    out2 = torch.empty((V, 2, N), dtype=torch.float64, device="cuda")
    out1 = torch.empty((V, 1, N), dtype=torch.float64, device="cuda")
    fit_out = torch.zeros((V, engine.num_params(2, False, False)), dtype=torch.float64, device="cuda")
    lib = L.lib()

    def fp64_fit():
        lib.mfx_debug_set_k2_screen(0)
        try:
            engine.fit_batch_dev(plan, d_Y, d_pk, 2, out=fit_out, check=False)
        finally:
            lib.mfx_debug_set_k2_screen(1)

    variants = {
        "k2": lambda: engine.profile_dev(plan, d_Y, d_pk, 2, out=out2),
        "k2_csf": lambda: engine.profile_dev(plan, d_Y, d_pk, 2, True, d_csf, out=out2),
        "k1": lambda: engine.profile_dev(plan, d_Y, d_pk1, 1, out=out1),
        "fp64_fit": fp64_fit,
    }
    for f in variants.values():   # warm-up at the timed shape
        f()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out2).all()) and bool(torch.isfinite(out1).all())
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
        res = {"what": "profile", "variant": name, "V": V, "M": M, "N": N, "iters": a.iters, "rounds": a.rounds,
               "s_per_call_median": med[name], "s_per_call_min": float(min(times[name])),
               "s_per_call_max": float(max(times[name])), "voxels_per_s": V / med[name],
               "rate_vs_fp64_fit": med["fp64_fit"] / med[name]}
        line = json.dumps(res)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
