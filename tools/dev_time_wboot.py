#!/usr/bin/env python3
"""Device time of the bootstrap conditional on measurement weights on the MI355X against the loop one would write by hand.

Workload: V two-fascicle voxels on synth.make_model("C2", N) (200 rows), noisy mixtures of rotated atoms at SNR 30 with
12 rows spoilt, general weights W ~ U(0.05, 2) with 1e-3 of it on the spoilt rows (the recipe of tests/test_wfit_gpu.py),
B replicates each (default 256 voxels x 782 atoms x B = 200; --N 160 is the small shape).

  shared    engine.fit_weighted_bootstrap_dev with the voxels' own weighted fit and its prediction handed in: per chunk
            of voxels the resampling, the replicate fit that forms a voxel's weighted cross-Gram once
            (include/mfx_wboot.h), the value table and the statistics
  loop      the same from the entry points that were there before it: engine.fit_weighted_dev on the expanded replicate
            rows (weights and directions repeated), the value table with torch, engine.boot_reduce_dev - in chunks of
            voxels sized so that the replicate signals and the repeated weights stay within the same 256 MiB
  resample  engine.wboot_resample_dev alone: it is new on both sides, so the loop is timed on replicate signals made
            before the clock starts and this figure is reported beside it

Every route runs --reps times after one warm-up, alternating, between two events on the stream; the minimum, the median
and the spread (max - min) are reported.  The replicate rows of both routes are asserted equal bit for bit.

One JSON line, appended to --out (default profiles/wboot_dev_time.jsonl).

Usage: python tools/dev_time_wboot.py [--V 256] [--B 200] [--N 782] [--reps 3] [--route both] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
Z = np.array([0.0, 0.0, 1.0])
BYTES = 256 << 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--V", type=int, default=256)
    ap.add_argument("--B", type=int, default=200)
    ap.add_argument("--N", type=int, default=782)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--route", choices=("both", "shared", "loop"), default="both", help="time one route only (for a profiler run)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wboot_dev_time.jsonl"))
    a = ap.parse_args()
    import torch
    from microstructure_fingerprinting_amd import engine, synth
    from microstructure_fingerprinting_amd import mf_utils as mfu
    sch, dic, _ = synth.make_model("C2", a.N)
    plan = mfu.init_PGSE_multishell_interp(dic, sch, Z).plan_for(sch)
    V, B, N, M = a.V, a.B, a.N, sch.shape[0]
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(1)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    peaks = np.concatenate([synth.unit_vectors(rng, V), synth.unit_vectors(rng, V)], axis=1)
    ids = rng.integers(0, N, (V, 2)).astype(np.int32)
    c0 = engine.rotate_columns_dev(plan, t(peaks[:, :3]), t(ids[:, 0])).cpu().numpy()
    c1 = engine.rotate_columns_dev(plan, t(peaks[:, 3:]), t(ids[:, 1])).cpu().numpy()
    f = rng.uniform(0.3, 0.7, (V, 1))
    Y = 500.0 * (f * c0 + (1.0 - f) * c1) + rng.normal(0, 500.0 / 30.0, (V, M))
    W = rng.uniform(0.05, 2.0, (V, M))
    for v in range(V):
        bad = rng.choice(M, 12, replace=False)
        Y[v, bad] *= rng.uniform(0.1, 0.5, 12)
        W[v, bad] *= 1e-3
    d_Y, d_W, d_pk = t(Y), t(W), t(peaks)
    props = t(rng.uniform(0.5, 5.0, (1, N)))
    q, seed = (0.025, 0.975), 7
    params, st = engine.fit_weighted_dev(plan, d_Y, d_W, d_pk, 2)
    pred = engine.predict_dev(plan, params, d_pk, 2)
    pred = pred[0] if isinstance(pred, tuple) else pred
    torch.cuda.synchronize(dev)
    assert not bool(st.any())
    chunk = max(1, min(V, BYTES // (2 * B * M * 8)))

    def resample(s, v0):
        return engine.wboot_resample_dev(d_Y[s], pred[s], d_W[s], params[s], 2, B=B, seed=seed, offset=v0 * M, d_peaks=d_pk[s])

    chunks = [(v0, slice(v0, min(V, v0 + chunk))) for v0 in range(0, V, chunk)]
    made = [resample(s, v0) for v0, s in chunks]          # the loop's replicate signals, made before its clock starts

    def shared(keep=False):
        return engine.fit_weighted_bootstrap_dev(plan, d_Y, d_W, d_pk, 2, B=B, seed=seed, q=q, d_props=props, d_params=params,
                                                 d_pred=pred, max_bytes=BYTES, keep=keep)

    def resample_all(keep=False):
        for v0, s in chunks:
            resample(s, v0)

    def loop(keep=False):
        stats, rows_all = [], []
        for (v0, s), (Ys, pk_rep, _) in zip(chunks, made):
            nv = s.stop - s.start
            W_rep = d_W[s].repeat_interleave(B, dim=0).contiguous()
            rows = engine.fit_weighted_dev(plan, Ys.reshape(nv * B, M), W_rep, pk_rep, 2)[0].reshape(nv, B, -1)
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
    assert same, "the shared replicate fit's rows differ from the weighted fit on the same signals"
    del res, ref_rows
    routes = [("loop", loop), ("shared", shared), ("resample", resample_all)]
    times = {name: [] for name, _ in routes}
    for _ in range(a.reps):
        for name, fn in routes:
            if name != "resample" and a.route not in ("both", name):
                continue
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize(dev)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize(dev)
            times[name].append(e0.elapsed_time(e1) * 1e-3)
    out = {"what": "wboot_dev_time", "N": N, "M": M, "V": V, "B": B, "reps": a.reps, "loop_chunk_voxels": chunk,
           "rows_equal": same, "stats_equal": same_stats}
    for name, ts in times.items():
        if not ts:
            continue
        out[name + "_s_min"], out[name + "_s_median"], out[name + "_s_spread"] = min(ts), float(np.median(ts)), max(ts) - min(ts)
        out[name + "_s_all"] = ts
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
