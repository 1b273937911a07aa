#!/usr/bin/env python3
"""Timing of the weighted two-fascicle fit on the MI355X (engine.fit_weighted_dev, csrc/fit_w.hip).

Sizes (N, M): (782, 200) on the C2 protocol of synth.py and (782, 552) on a synthetic protocol of 40 b0 rows and four
shells of 128 directions; V two-fascicle voxels (noisy mixtures of rotated atoms, 12 corrupted rows each) with a 0/1
mask of the corrupted rows per voxel - V >= 512, so that two workgroups per CU are in flight.  Per size: warm-up at the
timed shape, then `--iters` calls between two events, repeated `--repeats` times (median and spread are reported).

Two yardsticks taken in the same run:
  (a) the earlier route - the only one the library had for per-voxel weights: mf_utils.interp_PGSE_from_multishell
      (mfx_rotate) per fascicle, the row scaling on the host, mf_utils.solve_exhaustive_posweights per voxel - on
      `--parent-vox` voxels (its atoms are asserted equal to the fused kernel's);
  (b) the unweighted FP64 kernel (mfx_debug_set_k2_screen(0)) on the same voxels: the same matrix work without the
      per-entry product.
`--explicit-vox` voxels of the [N, N, 1] class (a CSF column: the materialise-and-solve route) are timed as well.

One JSON line per size, appended to --out (default profiles/wfit_dev_time.jsonl).

Usage: python tools/dev_time_wfit.py [--sizes 782x200,782x552] [--V 512] [--iters 3] [--repeats 5] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ROOF = 78e12
Z = np.array([0.0, 0.0, 1.0])


def protocol(M, N):
    from microstructure_fingerprinting_amd import synth
    if M == 200:
        sch, dic, _ = synth.make_model("C2", N)
        return sch, dic
    assert M == 552
    rng = np.random.default_rng(7)
    sch = synth.make_scheme(rng, 40, [1000, 3000, 5000, 10000], [128, 128, 128, 128])
    return sch, synth.make_dictionary(rng, sch, N)


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
    ap.add_argument("--sizes", default="782x200,782x552")
    ap.add_argument("--V", type=int, default=512)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--parent-vox", type=int, default=32)
    ap.add_argument("--explicit-vox", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wfit_dev_time.jsonl"))
    a = ap.parse_args()
    assert a.V >= 512, "at least 512 voxels per launch"
    import torch
    from microstructure_fingerprinting_amd import _lib, engine, synth
    from microstructure_fingerprinting_amd import mf_utils as U
    lib = _lib.lib()
    for size in a.sizes.split(","):
        N, M = (int(x) for x in size.split("x"))
        sch, dic = protocol(M, N)
        ms = U.init_PGSE_multishell_interp(dic, sch, Z)
        plan = ms.plan_for(sch)
        assert N <= lib.mfx_wfit_max_atoms(plan.handle(), 2)
        rng = np.random.default_rng(1)
        V = a.V
        peaks = np.concatenate([synth.unit_vectors(rng, V), synth.unit_vectors(rng, V)], axis=1)
        dp = torch.from_numpy(peaks).cuda()
        ids = rng.integers(0, N, (V, 2)).astype(np.int32)
        f = torch.from_numpy(rng.uniform(0.3, 0.7, (V, 1))).cuda()
        c0 = engine.rotate_columns_dev(plan, dp[:, :3].contiguous(), torch.from_numpy(ids[:, 0].copy()).cuda())
        c1 = engine.rotate_columns_dev(plan, dp[:, 3:].contiguous(), torch.from_numpy(ids[:, 1].copy()).cuda())
        Y = (500.0 * (f * c0 + (1.0 - f) * c1)).cpu().numpy() + rng.normal(0, 500.0 / 30.0, (V, M))
        W = np.ones((V, M))
        for v in range(V):
            bad = rng.choice(M, 12, replace=False)
            Y[v, bad] *= rng.uniform(0.1, 0.5, 12)
            W[v, bad] = 0.0
        dY, dW = torch.from_numpy(Y).cuda(), torch.from_numpy(W).cuda()
        out, st = engine.fit_weighted_dev(plan, dY, dW, dp, 2)
        torch.cuda.synchronize()
        assert int(st.abs().sum()) == 0 and bool(torch.isfinite(out).all())
        s, smin, smax = timed(lambda: engine.fit_weighted_dev(plan, dY, dW, dp, 2, out=out), a.iters, a.repeats)
        host = out.cpu().numpy()
        # (b) the unweighted FP64 kernel on the same voxels
        try:
            lib.mfx_debug_set_k2_screen(0)
            plain = engine.fit_batch_dev(plan, dY, dp, 2)
            s_f64, _, _ = timed(lambda: engine.fit_batch_dev(plan, dY, dp, 2, out=plain, check=False), a.iters, a.repeats)
        finally:
            lib.mfx_debug_set_k2_screen(1)
        # (a) the earlier route, voxel by voxel
        nv = min(a.parent_vox, V)
        sizes = np.array([N, N])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for v in range(nv):
            sq = np.sqrt(W[v])
            A = np.hstack([U.interp_PGSE_from_multishell(sch, peaks[v, 3 * k:3 * k + 3], msinterp=ms) for k in range(2)])
            w, sub, _, obj, _ = U.solve_exhaustive_posweights(np.ascontiguousarray(sq[:, None] * A), sq * Y[v], sizes)
            assert np.array_equal(sub, host[v, 3:5].astype(np.int64)), (v, sub, host[v, 3:5])
        parent = (time.perf_counter() - t0) / nv
        # the explicit route of the weighted [N, N, 1] class
        ne = min(a.explicit_vox, V)
        b = (synth.GAMMA_H * sch[:, 3] * sch[:, 5]) ** 2 * (sch[:, 4] - sch[:, 5] / 3)
        sig_csf = np.exp(-sch[:, 6] / 2.0) * np.exp(-b * 3.0e-9)
        arg = (plan, Y[:ne], W[:ne], np.full(ne, 2), np.ones(ne, bool), peaks[:ne], 2, True, sig_csf)
        engine.fit_weighted(*arg)
        t0 = time.perf_counter()
        _, stx = engine.fit_weighted(*arg)
        explicit = (time.perf_counter() - t0) / ne
        assert np.all(stx == 0)
        res = {"what": "wfit_k2", "N": N, "M": M, "V": V, "iters": a.iters, "repeats": a.repeats,
               "s_per_call_median": s, "s_per_call_min": smin, "s_per_call_max": smax, "voxels_per_s": V / s,
               "earlier_route_s_per_voxel": parent, "earlier_route_voxels": nv, "ratio_to_earlier_route": parent / (s / V),
               "unweighted_f64_voxels_per_s": V / s_f64, "ratio_to_unweighted_f64": s_f64 / s,
               "roof_fraction": (2.0 * N * N * M / ROOF) / (s / V),
               "explicit_nn1_voxels_per_s": 1.0 / explicit, "explicit_nn1_voxels": ne}
        line = json.dumps(res)
        print(line, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as fh:
                fh.write(line + "\n")
        assert parent > s / V, "the fused kernel is not faster than the earlier route"


if __name__ == "__main__":
    main()
