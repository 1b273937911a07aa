#!/usr/bin/env python3
"""Timing of the robust fit on the MI355X: MFModel.fit(robust={'n_iter': 2}) against the loop the README showed before
it - fit, fit.residuals, weights from the median absolute residual in NumPy, fit(weights=W) - run twice, and against the
plain fit, all through MFModel.fit on the same volume.

Workload: V two-fascicle voxels of config 2 (synth.make_model("C2"): 782 atoms, 200 measurements), noisy mixtures of
rotated atoms at SNR 30 with 12 corrupted rows each, as a (V / 100, 100) volume.  Every route is run once as warm-up at
the timed shape, then `--repeats` times, the routes alternating; host wall clock around calls that wait for their own
work; the median and the spread are reported.  The two robust routes are asserted to give the same parameters, bit for
bit.

The expectation to confirm or refute: the device loop costs about one plain fit plus n_iter weighted fits, and the
hand-made loop is dominated by host work.  One weighted fit alone is timed too (the last fit of the hand-made loop),
and the device loop on base weights (`weights=` one [M] vector with every 11th row out) beside the weighted fit on them:
that loop is n_iter + 1 weighted fits.

One JSON line, appended to --out (default profiles/robust_time.jsonl).

Usage: python tools/dev_time_robust.py [--V 100000] [--n-iter 2] [--repeats 3] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
Z = np.array([0.0, 0.0, 1.0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--V", type=int, default=100000)
    ap.add_argument("--N", type=int, default=782)
    ap.add_argument("--n-iter", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "robust_time.jsonl"))
    a = ap.parse_args()
    assert a.V % 100 == 0
    import torch
    import microstructure_fingerprinting_amd as mf
    from microstructure_fingerprinting_amd import engine, synth
    sch, dic, _ = synth.make_model("C2", a.N)
    N, M, V = dic.shape[1], sch.shape[0], a.V
    rng = np.random.default_rng(1)
    model = mf.MFModel({"dictionary": dic, "sch_mat": sch, "orientation": Z, "num_atom": N, "num_ear": 0, "T2_csf": 2.0,
                        "DIFF_csf": 3.0e-9, "T2_ear": 0.05, "DIFF_ear": np.array([1.0e-9]), "fasc_propnames": ["rad"],
                        "rad": rng.uniform(0.5, 5.0, N)})
    plan = model.ms_interpolator.plan_for(sch)
    peaks = np.concatenate([synth.unit_vectors(rng, V), synth.unit_vectors(rng, V)], axis=1)
    dp = torch.from_numpy(peaks).cuda()
    ids = rng.integers(0, N, (V, 2)).astype(np.int32)
    f = torch.from_numpy(rng.uniform(0.3, 0.7, (V, 1))).cuda()
    c0 = engine.rotate_columns_dev(plan, dp[:, :3].contiguous(), torch.from_numpy(ids[:, 0].copy()).cuda())
    c1 = engine.rotate_columns_dev(plan, dp[:, 3:].contiguous(), torch.from_numpy(ids[:, 1].copy()).cuda())
    Y = (500.0 * (f * c0 + (1.0 - f) * c1)).cpu().numpy() + rng.normal(0, 500.0 / 30.0, (V, M))
    bad = np.argsort(rng.random((V, M)), axis=1)[:, :12]
    np.put_along_axis(Y, bad, np.take_along_axis(Y, bad, axis=1) * rng.uniform(0.1, 0.5, (V, 12)), axis=1)
    del c0, c1, f, dp
    grid = (V // 100, 100)
    data, mask = Y.reshape(grid + (M,)), np.ones(grid)
    kw = dict(peaks=peaks.reshape(grid + (6,)), pgse_scheme=sch, verbose=0)
    last = {}

    def plain():
        last["plain"] = model.fit(data, mask, 2, **kw)

    def device_loop():
        last["dev"] = model.fit(data, mask, 2, robust={"n_iter": a.n_iter}, **kw)

    def manual_loop():
        fit = model.fit(data, mask, 2, **kw)
        for _ in range(a.n_iter):
            r = fit.residuals(data)
            W = np.abs(r) <= 4.45 * np.median(np.abs(r), axis=-1, keepdims=True)
            fit = model.fit(data, mask, 2, weights=W, **kw)
        last["man"], last["W"] = fit, W

    def weighted():
        model.fit(data, mask, 2, weights=last["W"], **kw)

    w0 = np.ones(M)                           # base weights: every 11th row out for good
    w0[::11] = 0.0

    def device_loop_base():
        last["dev0"] = model.fit(data, mask, 2, robust={"n_iter": a.n_iter}, weights=w0, **kw)

    def weighted_base():
        model.fit(data, mask, 2, weights=w0, **kw)

    routes = [("plain_fit", plain), ("device_loop", device_loop), ("manual_loop", manual_loop), ("weighted_fit", weighted),
              ("device_loop_base_weights", device_loop_base), ("weighted_fit_base_weights", weighted_base)]
    times = {name: [] for name, _ in routes}
    for rep in range(a.repeats + 1):          # the first pass is the warm-up
        for name, fn in routes:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if rep:
                times[name].append(time.perf_counter() - t0)
    assert np.array_equal(last["dev"].params_in_mask, last["man"].params_in_mask), "device loop and hand-made loop differ"
    assert np.array_equal(last["dev"].weights_roi, last["W"].reshape(-1, M).astype(np.float64))
    info = last["dev"].robust_info
    res = {"what": "robust_fit", "N": N, "M": M, "V": V, "n_iter": a.n_iter, "repeats": a.repeats,
           "n_changed": [int(x) for x in info["n_changed"]], "rows_rejected_mean": float(last["dev"].n_rejected.mean())}
    for name in times:
        t = times[name]
        res[name + "_s_median"], res[name + "_s_min"], res[name + "_s_max"] = float(np.median(t)), float(min(t)), float(max(t))
    res["manual_over_device"] = res["manual_loop_s_median"] / res["device_loop_s_median"]
    res["device_over_plain_plus_weighted"] = res["device_loop_s_median"] / (res["plain_fit_s_median"] + a.n_iter * res["weighted_fit_s_median"])
    res["device_base_weights_over_weighted_fits"] = res["device_loop_base_weights_s_median"] / (
        res["weighted_fit_base_weights_s_median"] + a.n_iter * res["weighted_fit_s_median"])
    assert np.all(last["dev0"].weights_roi[:, ::11] == 0)
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
