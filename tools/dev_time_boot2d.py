#!/usr/bin/env python3
"""Device time of the bootstrap of a 2-D protocol on the MI355X against the loop one would write by hand.

Workload: V two-fascicle voxels on the 1 776-row protocol of tests/golden/rot2d_cases.npz ("fix"), N smooth atoms
(the recipe of tests/test_fit2d_gpu.atoms), noisy mixtures of rotated atoms at SNR 30, B replicates each (default
256 voxels x 160 atoms x B = 200).

  shared   engine.fit2d_bootstrap_dev with the voxels' own fit and its prediction handed in: per chunk of voxels the
           resampling, the replicate fit that forms a voxel's records, column norms and cross-Gram once
           (include/mfx_boot2d.h), the value table and the statistics
  loop     the same from the entry points that were there before it: engine.boot_resample_dev with the directions copied
           to the replicate rows, engine.fit2d_dev on the expanded rows, the value table with torch, engine.boot_reduce_dev -
           in chunks of voxels sized so that the replicate signals and the rows' direction records (60 bytes per row,
           fascicle and measurement) stay within the same 256 MiB

Both run in one process, alternating, synchronised, --reps times each after one warm-up each; the minimum, the median
and the spread (max - min) of either are reported.  The replicate rows of both are asserted equal bit for bit.

One JSON line, appended to --out (default profiles/boot2d_dev_time.jsonl).

--route shared (or loop) times one route only, for a profiler run of its own (rocprofv3 --kernel-trace --stats -- python
tools/dev_time_boot2d.py --route shared): the per-kernel shares of DESIGN 4.23.

Usage: python tools/dev_time_boot2d.py [--V 256] [--B 200] [--N 160] [--reps 3] [--route both] [--out FILE]
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
GAM = 2 * np.pi * 42.577480e6
BYTES = 256 << 20


def atoms(sch, N, seed):
    rng = np.random.default_rng(seed)
    Gs, Dl, dl = sch[:, 3], sch[:, 4], sch[:, 5]
    b = (GAM * Gs * dl) ** 2 * (Dl - dl / 3)
    D = rng.uniform(0.3e-9, 2.5e-9, N)
    a = rng.uniform(-0.2, 0.2, (2, N))
    return np.exp(-np.outer(b, D)) * (1 + np.outer(Gs * sch[:, 0], a[0]) / 0.1 + np.outer(Gs * sch[:, 1], a[1]) / 0.1)


def directions(rng, n, zmin=0.3):
    v = rng.standard_normal((8 * n + 8, 3))
    v /= np.sqrt(np.sum(v ** 2, axis=1, keepdims=True))
    return np.ascontiguousarray(v[np.abs(v[:, 2]) >= zmin][:n])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--V", type=int, default=256)
    ap.add_argument("--B", type=int, default=200)
    ap.add_argument("--N", type=int, default=160)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--route", choices=("both", "shared", "loop"), default="both", help="time one route only (for a profiler run)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "boot2d_dev_time.jsonl"))
    a = ap.parse_args()
    import torch
    from microstructure_fingerprinting_amd import engine
    from microstructure_fingerprinting_amd import mf_utils as mfu
    sch = np.load(os.path.join(ROOT, "tests", "golden", "rot2d_cases.npz"))["fix_sch"]
    T = mfu.RotateAtom2DTables(atoms(sch, a.N, 5), sch, Z, 2.2e-9)
    V, B, N, M = a.V, a.B, T.N, T.M
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(1)
    peaks = np.zeros((V, 6))
    Y = np.zeros((V, M))
    for v in range(V):
        d = directions(rng, 2)
        while abs(d[0] @ d[1]) > 0.85:
            d = directions(rng, 2)
        peaks[v] = d.reshape(-1)
    ids = rng.integers(0, N, (V, 2))
    c0, c1 = T.rotate_cols(peaks[:, :3], ids[:, 0]), T.rotate_cols(peaks[:, 3:], ids[:, 1])
    f = rng.uniform(0.3, 0.7, (V, 1))
    clean = f * c0 + (1.0 - f) * c1
    Y = np.sqrt((clean + rng.standard_normal((V, M)) / 30.0) ** 2 + (rng.standard_normal((V, M)) / 30.0) ** 2)
    d_Y, d_pk = torch.from_numpy(Y).to(dev), torch.from_numpy(peaks).to(dev)
    props = torch.from_numpy(rng.uniform(0.5, 5.0, (1, N))).to(dev)
    q, seed = (0.025, 0.975), 7
    params, st = engine.fit2d_dev(T, d_Y, d_pk, 2)
    pred = engine.predict2d_dev(T, params, d_pk, 2)[0]
    torch.cuda.synchronize(dev)
    assert not bool(st.any())
    per_vox = B * M * 8 + B * 2 * M * 60
    chunk = max(1, min(V, BYTES // per_vox))

    def shared(keep=False):
        return engine.fit2d_bootstrap_dev(T, d_Y, d_pk, 2, B=B, seed=seed, q=q, d_props=props, d_params=params, d_pred=pred,
                                          max_bytes=BYTES, keep=keep)

    def loop(keep=False):
        stats, rows_all = [], []
        for v0 in range(0, V, chunk):
            s = slice(v0, min(V, v0 + chunk))
            nv = s.stop - s.start
            Ys, pk_rep, _ = engine.boot_resample_dev(d_Y[s], pred[s], params[s], 2, B=B, seed=seed, offset=v0 * M, d_peaks=d_pk[s])
            rows = engine.fit2d_dev(T, Ys.reshape(nv * B, M), pk_rep, 2)[0].reshape(nv, B, -1)
            ok = (rows[:, :, 1:3] > 0)
            X = torch.cat([rows[:, :, 0:3], rows[:, :, 5:6], props[0][rows[:, :, 3:5].long().clamp(0, N - 1)]], dim=2).contiguous()
            valid = torch.cat([torch.ones((nv, B, 4), dtype=torch.bool, device=dev), ok], dim=2).contiguous()
            stats.append(engine.boot_reduce_dev(X, valid.to(torch.uint8), q))
            if keep:
                rows_all.append(rows)
        return torch.cat(stats), (torch.cat(rows_all) if keep else None)

    ref_stats, ref_rows = loop(keep=True)
    res = shared(keep=True)
    torch.cuda.synchronize(dev)
    same = bool(torch.equal(res["replicates"], ref_rows))
    nan_eq = lambda x, y: bool(torch.equal(torch.nan_to_num(x, nan=-1.0), torch.nan_to_num(y, nan=-1.0)))
    same_stats = nan_eq(res["stats"], ref_stats)
    assert same, "the shared replicate fit's rows differ from the plain fit on the same signals"
    del res, ref_rows
    times = {"shared": [], "loop": []}
    for _ in range(a.reps):
        for name, fn in (("loop", loop), ("shared", shared)):
            if a.route not in ("both", name):
                continue
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize(dev)
            times[name].append(time.perf_counter() - t0)
    out = {"what": "boot2d_dev_time", "N": N, "M": M, "V": V, "B": B, "reps": a.reps, "loop_chunk_voxels": chunk,
           "rows_equal": same, "stats_equal": same_stats}
    for name, t in times.items():
        if not t:
            continue
        out[name + "_s_min"], out[name + "_s_median"], out[name + "_s_spread"] = min(t), float(np.median(t)), max(t) - min(t)
        out[name + "_s_all"] = t
    if a.route == "both":
        out["speedup_min_over_min"] = out["loop_s_min"] / out["shared_s_min"]
        out["gain_exceeds_spread"] = bool(out["loop_s_min"] - out["shared_s_min"] > max(out["loop_s_spread"], out["shared_s_spread"]))
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
