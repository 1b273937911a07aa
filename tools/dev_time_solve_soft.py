#!/usr/bin/env python3
"""Time of the solver's soft answers (include/mfx_solve_soft.h) on the MI355X against the per-voxel kernels.

Workload: a multi-shell model of --atoms atoms (default 782) by 200 measurements rotated ONCE onto two fixed directions,
A = [D(d0) | D(d1)] and, for the CSF class, a free-diffusion column appended: sub-dictionaries [782, 782] and [782, 782, 1].
V signals (0.6 of an atom of the first, 0.3 of one of the second, 0.1 of the CSF column, noise), V in {64, 1024}.

  solver      engine.solve_posterior_dev (shift=None: the minimum pass, the exponential pass and the reduce kernels) and
              engine.solve_profile_dev (partner=True) on a mf_utils.ExhaustiveSolver of A; ExhaustiveSolver.posterior /
              .profile on host buffers for the wall time.  `post_given`: mfx_solve_post_dev with the shift given and no
              min F asked for - no minimum pass - so that the minimum pass's share is the difference.
  per_voxel   the comparator, the only other route to these numbers: engine.posterior_dev / engine.profile_dev on the
              plan of the same model with the two directions repeated for every signal (it rotates the dictionary, takes
              its column statistics and forms the 782 x 782 cross-Gram per signal); engine.posterior / engine.profile on
              host buffers for the wall time.  It needs a shift: it is given the solver's min F, outside the timed region.

One process, the routes alternating, one warm-up and --reps timed runs each, medians; device time between two events
around the enqueue, wall time around the host call.  The two routes' answers are compared before anything is timed.
One JSON line per (class, V), appended to --out (default profiles/solve_soft_dev_time.jsonl).

Usage: python tools/dev_time_solve_soft.py [--V 64 1024] [--reps 3] [--atoms 782] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GAMMA = 2.6751525e8


def med(ts):
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--V", type=int, nargs="+", default=[64, 1024])
    ap.add_argument("--atoms", type=int, default=782)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "solve_soft_dev_time.jsonl"))
    a = ap.parse_args()
    import torch
    from microstructure_fingerprinting_amd import _lib, engine, synth
    from microstructure_fingerprinting_amd import mf_utils as mfu
    lib = _lib.lib()
    if lib.mfx_device_count() < 1:
        raise SystemExit("no HIP device: nothing is measured without one")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    torch.zeros(1).cuda()
    sch, dic, rng = synth.make_model("C2", N=a.atoms)
    ms = mfu.init_PGSE_multishell_interp(dic, sch, np.array([0.0, 0.0, 1.0]))
    plan = ms.plan_for(sch)
    M, N = sch.shape[0], a.atoms
    d0 = np.array([0.3, 0.2, 0.93]); d0 /= np.linalg.norm(d0)
    d1 = np.array([0.8, -0.5, 0.33]); d1 /= np.linalg.norm(d1)
    dirs = np.ascontiguousarray(np.stack([d0, d1]))
    D = np.zeros((2, M, N))
    _lib.check(lib.mfx_rotate(plan.handle(), _lib.dptr(dirs), 2, 0, _lib.dptr(D)))
    b = (GAMMA * sch[:, 3] * sch[:, 5]) ** 2 * (sch[:, 4] - sch[:, 5] / 3.0)
    x = np.ascontiguousarray(np.exp(-b * 3.0e-9))
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def dev(fn):
        ev0.record()
        r = fn()
        ev1.record()
        ev1.synchronize()
        return ev0.elapsed_time(ev1) * 1e-3, r

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        return time.perf_counter() - t0, r

    for csf in (False, True):
        A = np.ascontiguousarray(np.concatenate([D[0], D[1]] + ([x[:, None]] if csf else []), axis=1))
        sizes = np.array([N, N, 1] if csf else [N, N])
        S = mfu.ExhaustiveSolver(A, sizes)
        S.handle()
        for V in a.V:
            sig = 0.01 * float(np.abs(D[0]).mean())
            Y = 0.6 * D[0][:, rng.integers(0, N, V)].T + 0.3 * D[1][:, rng.integers(0, N, V)].T + sig * rng.standard_normal((V, M))
            if csf:
                Y = Y + 0.1 * x[None, :]
            Y = np.ascontiguousarray(Y)
            pk = np.ascontiguousarray(np.tile(np.concatenate([d0, d1]), (V, 1)))
            K, flags = np.full(V, 2), (np.full(V, True) if csf else None)
            dY, dpk = torch.from_numpy(Y).cuda(), torch.from_numpy(pk).cuda()
            dx = torch.from_numpy(x).cuda() if csf else None
            dT = torch.full((V,), 2.0 * sig * sig, dtype=torch.float64, device="cuda")
            w, ls, mo, st = engine.solve_posterior_dev(S, dY, dT)
            shift = mo.clone()
            h_shift = shift.cpu().numpy()
            dw0 = torch.empty((V, N), dtype=torch.float64, device="cuda")
            dw1, dls = torch.empty_like(dw0), torch.empty((V,), dtype=torch.float64, device="cuda")
            dst = torch.empty((V,), dtype=torch.int32, device="cuda")
            cur = torch.cuda.current_stream().cuda_stream

            routes = {
                "solver_post_dev": lambda: dev(lambda: engine.solve_posterior_dev(S, dY, dT)),
                "solver_post_given_dev": lambda: dev(lambda: _lib.check(lib.mfx_solve_post_dev(
                    S.handle(), dY.data_ptr(), V, dT.data_ptr(), shift.data_ptr(), 0, dw0.data_ptr(), dw1.data_ptr(), dls.data_ptr(),
                    None, dst.data_ptr(), cur))),
                "per_voxel_post_dev": lambda: dev(lambda: engine.posterior_dev(plan, dY, dpk, 2, dT, shift, csf, dx)),
                "solver_profile_dev": lambda: dev(lambda: engine.solve_profile_dev(S, dY, partner=True)),
                "per_voxel_profile_dev": lambda: dev(lambda: engine.profile_dev(plan, dY, dpk, 2, csf, dx, partner=True)),
                "solver_post_wall": lambda: wall(lambda: S.posterior(Y, sigma=sig)),
                "per_voxel_post_wall": lambda: wall(lambda: engine.posterior(plan, Y, K, flags, pk, 2, csf, x if csf else None, sig,
                                                                             shift=h_shift)),
                "solver_profile_wall": lambda: wall(lambda: S.profile(Y, partner=True)),
                "per_voxel_profile_wall": lambda: wall(lambda: engine.profile(plan, Y, K, flags, pk, 2, csf, x if csf else None,
                                                                              partner=True)),
            }
            warm = {k: f()[1] for k, f in routes.items()}     # the warm-up of every route, and the comparison
            pw, pls, pst = warm["per_voxel_post_dev"]
            assert not st.cpu().numpy().any() and not pst.cpu().numpy().any()
            dwm = max(float((w[k] - pw[:, k]).abs().max()) for k in range(2))
            dlm = float((ls - pls).abs().max())
            pobj = warm["per_voxel_profile_dev"][0]
            sobj = warm["solver_profile_dev"][0]
            scale = float(pobj.abs().max())
            dom = max(float((sobj[k] - pobj[:, k]).abs().max()) for k in range(2)) / scale
            assert dwm < 1e-6 and dlm < 1e-6 and dom < 1e-9, (dwm, dlm, dom)
            t = {k: [] for k in routes}
            for _ in range(a.reps):
                for k, f in routes.items():
                    t[k].append(f()[0])
            rec = {"sizes": [int(s) for s in sizes], "M": int(M), "V": V, "reps": a.reps,
                   "scratch_bytes_per_signal": {"profile": S.soft_bytes_per_signal('profile'), "posterior": S.soft_bytes_per_signal('posterior')},
                   "max_abs_diff": {"w": dwm, "log_sum": dlm, "obj_rel": dom}}
            for k in routes:
                rec[k] = {"median_s": med(t[k]), "signals_per_s": V / med(t[k])}
            rec["minimum_pass_share_of_post_dev"] = 1.0 - med(t["solver_post_given_dev"]) / med(t["solver_post_dev"])
            for what in ("post_dev", "profile_dev", "post_wall", "profile_wall"):
                rec["ratio_" + what] = med(t["per_voxel_" + what]) / med(t["solver_" + what])
            line = json.dumps(rec)
            print(line, flush=True)
            with open(a.out, "a") as f:
                f.write(line + "\n")
        S.close()


if __name__ == "__main__":
    main()
