#!/usr/bin/env python3
"""Time of the batched explicit-dictionary solver on the MI355X against the loop of one-problem solves.

Workload: the reference's own test shape (test_synthetic_data): a randn dictionary of M = 200 rows, sub-dictionaries
[782, 782] and [782, 782, 1], V signals made of one atom of each sub-dictionary plus noise, V in {64, 1024}.

  loop     V calls of mf_utils.solve_exhaustive_posweights(A, Y[v], dicsizes): per call the upload of the dictionary, its
           Gram matrix, the scan and a device synchronisation.  Its cost per signal does not depend on V, so it is timed on
           the first --loop-signals signals (default 64) and reported as signals/s.
  batch    mf_utils.ExhaustiveSolver(A, dicsizes).solve(Y) on host buffers (wall time, upload and download included; the
           handle's creation - upload and Gram, once - is timed apart), and engine.solve_batch_dev on device tensors between
           two device events (device time: the kernels of the batch and nothing else), on the tiled route and on the
           generic route (mfx_solve_debug_set_force_generic)

Both run in one process, alternating, --reps times each after one warm-up each; the minimum and the median are reported.
The rows of the batch on either route are asserted equal, bit for bit, to the loop's on the signals the loop solved.

One JSON line per (shape, V), appended to --out (default profiles/solve_batch_dev_time.jsonl).

Usage: python tools/dev_time_solve_batch.py [--V 64 1024] [--reps 3] [--loop-signals 64] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def problem(sizes, M, V, seed=141414):
    rng = np.random.default_rng(seed)
    sizes = np.asarray(sizes)
    starts = np.concatenate(([0], np.cumsum(sizes)[:-1]))
    A = rng.standard_normal((M, int(sizes.sum())))
    Y = 0.1 * (2.0 * rng.random((V, M)) - 1.0)
    for s0, n in zip(starts, sizes):
        Y += (A[:, s0 + rng.integers(0, n, V)] * rng.random(V)).T
    return A, np.ascontiguousarray(Y), sizes


def stats(ts):
    return {"min_s": float(np.min(ts)), "median_s": float(np.median(ts))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--V", type=int, nargs="+", default=[64, 1024])
    ap.add_argument("--M", type=int, default=200)
    ap.add_argument("--atoms", type=int, default=782)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--loop-signals", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "solve_batch_dev_time.jsonl"))
    a = ap.parse_args()
    import torch
    from microstructure_fingerprinting_amd import _lib, engine
    from microstructure_fingerprinting_amd import mf_utils as mfu
    lib = _lib.lib()
    if lib.mfx_device_count() < 1:
        raise SystemExit("no HIP device: nothing is measured without one")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    torch.zeros(1).cuda()                  # both runtimes up before anything is timed
    mfu.solve_exhaustive_posweights(np.ones((2, 2)), np.ones(2), np.array([1, 1]))
    for sizes in ([a.atoms, a.atoms], [a.atoms, a.atoms, 1]):
        for V in a.V:
            A, Y, sz = problem(sizes, a.M, V)
            nl = min(V, a.loop_signals)

            def loop():
                return [mfu.solve_exhaustive_posweights(A, Y[v], sz) for v in range(nl)]

            t0 = time.perf_counter()
            S = mfu.ExhaustiveSolver(A, sz)
            S.handle()
            t_create = time.perf_counter() - t0
            dY = torch.from_numpy(Y).cuda()
            ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

            def batch_wall():
                return S.solve(Y)

            def batch_dev():
                ev0.record()
                r = engine.solve_batch_dev(S, dY)
                ev1.record()
                ev1.synchronize()
                return ev0.elapsed_time(ev1) * 1e-3, r

            rows = loop()                      # warm-up of every route, and the equality check
            for force in (0, 1):
                lib.mfx_solve_debug_set_force_generic(force)
                got = batch_wall()
                _, dgot = batch_dev()
                for v in range(nl):
                    for k in range(5):
                        assert np.array_equal(got[k][v], rows[v][k]), (sizes, V, force, v, k)
                for k in (0, 1, 2, 3, 4, 5):
                    assert np.array_equal(dgot[k].cpu().numpy(), got[k]), (sizes, V, force, k)
            t = {"loop": [], "tiled_wall": [], "tiled_dev": [], "generic_wall": [], "generic_dev": []}
            for _ in range(a.reps):
                t0 = time.perf_counter(); loop(); t["loop"].append(time.perf_counter() - t0)
                for force, name in ((0, "tiled"), (1, "generic")):
                    lib.mfx_solve_debug_set_force_generic(force)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter(); batch_wall(); t[name + "_wall"].append(time.perf_counter() - t0)
                    t[name + "_dev"].append(batch_dev()[0])
            lib.mfx_solve_debug_set_force_generic(0)
            S.close()
            rec = {"sizes": [int(s) for s in sz], "M": a.M, "V": V, "reps": a.reps, "loop_signals": nl, "create_s": t_create,
                   "loop": dict(stats(t["loop"]), signals_per_s=nl / float(np.median(t["loop"])))}
            for name in ("tiled_wall", "tiled_dev", "generic_wall", "generic_dev"):
                rec[name] = dict(stats(t[name]), signals_per_s=V / float(np.median(t[name])))
            rec["one_shot_signals_per_s"] = V / (t_create + float(np.median(t["tiled_wall"])))
            line = json.dumps(rec)
            print(line, flush=True)
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
