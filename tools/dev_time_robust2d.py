#!/usr/bin/env python3
"""Timing of the robust fit of 2-D protocols on the MI355X: engine.fit2d_robust against the loop a user writes by hand
from engine.fit2d, engine.predict2d, NumPy weights from the median absolute residual and engine.fit2d_weighted, and
against the plain engine.fit2d, all on NumPy arrays (every route uploads its data and waits for its own work).

Workload: the fixture protocol of tests/golden/rot2d_cases.npz (1776 rows), analytic atoms (N = 160, the largest shape of
tests/_w2d_ref.SHAPES), V two-fascicle voxels (noisy mixtures of rotated atoms) with 12 rows per voxel multiplied by
U(0.1, 0.5).  Every route is run once as warm-up at the timed shape, then `--repeats` times, the routes alternating; host
wall clock; the median and the spread are reported.  The two robust routes are asserted to give the same parameters and
weights, bit for bit.

The expectation to confirm or refute: the device loop is not slower than the hand-made loop - it skips the host round
trips and builds the directions' plan once, where the hand-made loop builds it 1 + 2 n_iter times.

`--route NAME` runs one route only (twice), for a kernel trace; `--route predict_kernel` runs the prediction alone on
`--V-predict` voxels three times and then fills its output three times (the write-only floor):
  rocprofv3 --kernel-trace --stats -- python tools/dev_time_robust2d.py --route device_loop --out ''

One JSON line, appended to --out (default profiles/robust2d_time.jsonl).

Usage: python tools/dev_time_robust2d.py [--V 2048] [--N 160] [--n-iter 2] [--repeats 5] [--route NAME] [--V-predict 16384] [--out FILE]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--V", type=int, default=2048)
    ap.add_argument("--N", type=int, default=160)
    ap.add_argument("--n-iter", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--route", default=None)
    ap.add_argument("--V-predict", type=int, default=16384)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "robust2d_time.jsonl"))
    a = ap.parse_args()
    import torch
    from microstructure_fingerprinting_amd import engine
    from microstructure_fingerprinting_amd import mf_utils as U
    sch = np.load(os.path.join(ROOT, "tests", "golden", "rot2d_cases.npz"))["fix_sch"]
    T = U.RotateAtom2DTables(atoms(sch, a.N, 5), sch, np.array([0.0, 0.0, 1.0]), 2.2e-9)
    N, M, V = T.N, T.M, a.V
    rng = np.random.default_rng(1)
    Y, peaks = voxels(T, rng, V, 0.3)
    bad = np.argsort(rng.random((V, M)), axis=1)[:, :12]
    np.put_along_axis(Y, bad, np.take_along_axis(Y, bad, axis=1) * rng.uniform(0.1, 0.5, (V, 12)), axis=1)
    K = np.full(V, 2)
    last = {}
    if a.route == "predict_kernel":           # the prediction kernel alone at a size that fills the chip, beside a fill of its output
        Vp = a.V_predict
        d = rng.standard_normal((8 * Vp, 3))
        d /= np.sqrt(np.sum(d ** 2, axis=1, keepdims=True))
        d = d[np.abs(d[:, 2]) >= 0.3][:2 * Vp]
        prm = np.zeros((Vp, 7))
        prm[:, 0], prm[:, 1:3], prm[:, 3:5] = 1.0, 0.5, rng.integers(0, N, (Vp, 2))
        d_p, d_k = torch.from_numpy(prm).cuda(), torch.from_numpy(np.ascontiguousarray(d.reshape(Vp, 6))).cuda()
        out = torch.empty((Vp, M), dtype=torch.float64, device="cuda")
        for _ in range(3):
            _, _, st, ds = engine.predict2d_dev(T, d_p, d_k, 2, out=out)
        torch.cuda.synchronize()
        assert int(st.abs().sum()) == 0 and int(ds.abs().sum()) == 0 and bool(torch.isfinite(out).all())
        for _ in range(3):
            out.zero_()                        # the write-only floor: V M 8 bytes
        torch.cuda.synchronize()
        return

    def plain():
        last["plain"] = engine.fit2d(T, Y, K, None, peaks, 2, False)[0]

    def device_loop():
        last["dev"] = engine.fit2d_robust(T, Y, K, None, peaks, 2, False, n_iter=a.n_iter)

    def manual_loop():
        p = engine.fit2d(T, Y, K, None, peaks, 2, False)[0]
        W = np.ones((V, M))
        for _ in range(a.n_iter):
            r = np.abs(Y - engine.predict2d(T, p, peaks, 2)[0])
            W = (r <= 4.45 * np.median(r, axis=1, keepdims=True)).astype(np.float64)
            p = engine.fit2d_weighted(T, Y, W, K, None, peaks, 2, False)[0]
        last["man"] = (p, W)

    def weighted():
        engine.fit2d_weighted(T, Y, last["man"][1], K, None, peaks, 2, False)

    def predict():
        engine.predict2d(T, last["plain"], peaks, 2)

    routes = [("plain_fit", plain), ("device_loop", device_loop), ("manual_loop", manual_loop), ("weighted_fit", weighted),
              ("predict", predict)]
    if a.route is not None:
        fn = dict(routes)[a.route]
        if a.route in ("weighted_fit", "predict"):
            plain(); manual_loop()
        for _ in range(2):
            fn()
        torch.cuda.synchronize()
        return
    times = {name: [] for name, _ in routes}
    for rep in range(a.repeats + 1):          # the first pass is the warm-up
        for name, fn in routes:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if rep:
                times[name].append(time.perf_counter() - t0)
    p, W, info = last["dev"]
    assert np.array_equal(p.view(np.int64), last["man"][0].view(np.int64)), "device loop and hand-made loop differ"
    assert np.array_equal(W, last["man"][1])
    res = {"what": "robust2d_fit", "N": N, "M": M, "V": V, "n_iter": a.n_iter, "repeats": a.repeats,
           "n_changed": [int(x) for x in info["n_changed"]], "n_iter_used": info["n_iter_used"],
           "rows_rejected_mean": float(np.count_nonzero(W == 0, axis=1).mean())}
    for name in times:
        t = times[name]
        res[name + "_s_median"], res[name + "_s_min"], res[name + "_s_max"] = float(np.median(t)), float(min(t)), float(max(t))
    res["manual_over_device"] = res["manual_loop_s_median"] / res["device_loop_s_median"]
    res["device_over_plain_plus_weighted"] = res["device_loop_s_median"] / (res["plain_fit_s_median"] + a.n_iter * res["weighted_fit_s_median"])
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
