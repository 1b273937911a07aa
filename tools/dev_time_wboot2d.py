#!/usr/bin/env python3
"""Device time of the bootstrap of a 2-D protocol conditional on measurement weights on the MI355X, against the loop one
would write by hand from the entry points that were there before it.

Workload: V two-fascicle voxels on the 1 776-row protocol of tests/golden/rot2d_cases.npz ("fix"), N smooth atoms
(the recipe of tests/test_fit2d_gpu.atoms), noisy mixtures of rotated atoms at SNR 30, general per-voxel weights in
[0.25, 4] with a tenth of the rows at weight 0, B replicates each (default 256 voxels x 160 atoms x B = 200).  The voxels'
own weighted fit and its prediction are handed in.

  shared   engine.fit2d_weighted_bootstrap_dev: per chunk of voxels the resampling, the weighted replicate fit that forms a
           voxel's sqrt(W), records, column norms and weighted cross-Gram once (include/mfx_wboot2d.h), the value table
           and the statistics
  plain    the same entry point under mfx_wboot2d_debug_set_force_plain(1) (--plain): weights and directions copied to the
           replicate rows, the weighted fit's class launcher on them
  loop     engine.wboot_resample_dev with the directions copied to the replicate rows, engine.fit2d_weighted_dev on the
           expanded rows with the weight rows repeated, the value table with torch, engine.boot_reduce_dev - in chunks of
           voxels sized so that the replicate signals, the repeated weights, sqrt(W) and y' of the rows and the rows'
           direction records (60 bytes per row, fascicle and measurement) stay within the same 256 MiB

All run in one process, alternating, --reps times each after one warm-up each.  A run's time is the DEVICE time between
two events recorded on the stream around it; the minimum, the median and the spread (max - min) of either are reported.
The replicate rows and statistics of the routes are asserted equal bit for bit.

One JSON line, appended to --out (default profiles/wboot2d_dev_time.jsonl).

Usage: python tools/dev_time_wboot2d.py [--V 256] [--B 200] [--N 160] [--reps 3] [--plain] [--out FILE]
"""
import argparse
import json
import os
import sys

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
    ap.add_argument("--plain", action="store_true", help="also time the entry point's plain path")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wboot2d_dev_time.jsonl"))
    a = ap.parse_args()
    import torch
    from microstructure_fingerprinting_amd import _lib, engine
    from microstructure_fingerprinting_amd import mf_utils as mfu
    sch = np.load(os.path.join(ROOT, "tests", "golden", "rot2d_cases.npz"))["fix_sch"]
    T = mfu.RotateAtom2DTables(atoms(sch, a.N, 5), sch, Z, 2.2e-9)
    V, B, N, M = a.V, a.B, T.N, T.M
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(1)
    peaks = np.zeros((V, 6))
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
    W = 0.25 * 16.0 ** rng.uniform(0.0, 1.0, (V, M))
    W[rng.uniform(0.0, 1.0, (V, M)) < 0.1] = 0.0
    d_Y, d_W, d_pk = torch.from_numpy(Y).to(dev), torch.from_numpy(W).to(dev), torch.from_numpy(peaks).to(dev)
    props = torch.from_numpy(rng.uniform(0.5, 5.0, (1, N))).to(dev)
    q, seed = (0.025, 0.975), 7
    params, st, wst = engine.fit2d_weighted_dev(T, d_Y, d_W, d_pk, 2)
    pred = engine.predict2d_dev(T, params, d_pk, 2)[0]
    torch.cuda.synchronize(dev)
    assert not bool(st.any()) and not bool(wst.any())
    per_vox = B * M * 8 * 4 + B * 2 * M * 60
    chunk = max(1, min(V, BYTES // per_vox))

    def shared(keep=False):
        return engine.fit2d_weighted_bootstrap_dev(T, d_Y, d_W, d_pk, 2, B=B, seed=seed, q=q, d_props=props, d_params=params,
                                                   d_pred=pred, max_bytes=BYTES, keep=keep)

    def plain(keep=False):
        _lib.lib().mfx_wboot2d_debug_set_force_plain(1)
        try:
            return shared(keep)
        finally:
            _lib.lib().mfx_wboot2d_debug_set_force_plain(0)

    def loop(keep=False):
        stats, rows_all = [], []
        for v0 in range(0, V, chunk):
            s = slice(v0, min(V, v0 + chunk))
            nv = s.stop - s.start
            Ys, pk_rep, _ = engine.wboot_resample_dev(d_Y[s], pred[s], d_W[s], params[s], 2, B=B, seed=seed, offset=v0 * M,
                                                      d_peaks=d_pk[s])
            W_rep = d_W[s].repeat_interleave(B, dim=0)
            rows = engine.fit2d_weighted_dev(T, Ys.reshape(nv * B, M), W_rep, pk_rep, 2)[0].reshape(nv, B, -1)
            ok = (rows[:, :, 1:3] > 0)
            X = torch.cat([rows[:, :, 0:3], rows[:, :, 5:6], props[0][rows[:, :, 3:5].long().clamp(0, N - 1)]], dim=2).contiguous()
            valid = torch.cat([torch.ones((nv, B, 4), dtype=torch.bool, device=dev), ok], dim=2).contiguous()
            stats.append(engine.boot_reduce_dev(X, valid.to(torch.uint8), q))
            if keep:
                rows_all.append(rows)
        return torch.cat(stats), (torch.cat(rows_all) if keep else None)

    nan_eq = lambda x, y: bool(torch.equal(torch.nan_to_num(x, nan=-1.0), torch.nan_to_num(y, nan=-1.0)))
    ref_stats, ref_rows = loop(keep=True)          # (the warm-up of either route as well)
    res = shared(keep=True)
    torch.cuda.synchronize(dev)
    same, same_stats = bool(torch.equal(res["replicates"], ref_rows)), nan_eq(res["stats"], ref_stats)
    assert same, "the shared replicate fit's rows differ from the weighted fit on the same signals"
    routes = [("loop", loop), ("shared", shared)]
    out = {"what": "wboot2d_dev_time", "N": N, "M": M, "V": V, "B": B, "reps": a.reps, "loop_chunk_voxels": chunk,
           "rows_equal": same, "stats_equal": same_stats, "clock": "device time between two events"}
    if a.plain:
        resp = plain(keep=True)
        torch.cuda.synchronize(dev)
        out["plain_rows_equal"] = bool(torch.equal(resp["replicates"], ref_rows))
        out["plain_stats_equal"] = nan_eq(resp["stats"], ref_stats)
        assert out["plain_rows_equal"], "the plain path's rows differ from the weighted fit on the same signals"
        routes.append(("plain", plain))
        del resp
    del res, ref_rows
    times = {name: [] for name, _ in routes}
    for _ in range(a.reps):
        for name, fn in routes:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize(dev)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize(dev)
            times[name].append(e0.elapsed_time(e1) / 1000.0)
    for name, t in times.items():
        out[name + "_s_min"], out[name + "_s_median"], out[name + "_s_spread"] = min(t), float(np.median(t)), max(t) - min(t)
        out[name + "_s_all"] = t
    out["speedup_min_over_min"] = out["loop_s_min"] / out["shared_s_min"]
    out["gain_exceeds_both_spreads"] = bool(out["loop_s_min"] - out["shared_s_min"] > out["loop_s_spread"] + out["shared_s_spread"])
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
