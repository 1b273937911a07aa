#!/usr/bin/env python3
"""Device time of the bootstrap on the MI355X against its yardstick, the plain fit on the same replicate rows.

Workload: V two-fascicle voxels of config 2 (synth.make_model("C2"): 782 atoms, 200 measurements), noisy mixtures of
rotated atoms at SNR 30, B replicates each (default 1e4 voxels x 100 = 1e6 replicate rows).  Timed with events on
torch's current stream, each route once as warm-up at the timed shape (the scratch arena settles) and then once:

  bootstrap     engine.fit_bootstrap_dev with nothing handed in: the voxels' own fit, its prediction, and per chunk of
                voxels the resampling, the plain fit on the chunk's replicate rows, the value table and the statistics
  bootstrap_in  the same with the voxels' parameters and prediction handed in
  yardstick     engine.fit_batch_dev on the same V B replicate rows, made beforehand by engine.boot_resample_dev with
                the same seed - one call, the path the bootstrap calls per chunk, unchanged by it

The replicate rows of the bootstrap (keep=True) are asserted to equal the yardstick's output bit for bit.  The
expectation to hold the measurement against: bootstrap / yardstick <= 1.15 (the resampling writes and the fit reads
V B M 8 bytes once; the value table and the statistics are smaller still; the rest is the launch tails of the chunks).

One JSON line, appended to --out (default profiles/boot_dev_time.jsonl).

Usage: python tools/dev_time_boot.py [--V 10000] [--B 100] [--N 782] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
Z = np.array([0.0, 0.0, 1.0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--V", type=int, default=10000)
    ap.add_argument("--B", type=int, default=100)
    ap.add_argument("--N", type=int, default=782)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "boot_dev_time.jsonl"))
    a = ap.parse_args()
    import torch
    from microstructure_fingerprinting_amd import _lib as L
    from microstructure_fingerprinting_amd import engine, synth
    from microstructure_fingerprinting_amd import mf_utils as mfu
    sch, dic, _ = synth.make_model("C2", a.N)
    ms = mfu.init_PGSE_multishell_interp(dic, sch, Z)
    plan = ms.plan_for(sch)
    N, M, V, B = dic.shape[1], sch.shape[0], a.V, a.B
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(1)
    peaks = np.concatenate([synth.unit_vectors(rng, V), synth.unit_vectors(rng, V)], axis=1)
    d_pk = torch.from_numpy(peaks).to(dev)
    ids = rng.integers(0, N, (V, 2)).astype(np.int32)
    f = torch.from_numpy(rng.uniform(0.3, 0.7, (V, 1))).to(dev)
    c0 = engine.rotate_columns_dev(plan, d_pk[:, :3].contiguous(), torch.from_numpy(ids[:, 0].copy()).to(dev))
    c1 = engine.rotate_columns_dev(plan, d_pk[:, 3:].contiguous(), torch.from_numpy(ids[:, 1].copy()).to(dev))
    d_Y = (500.0 * (f * c0 + (1.0 - f) * c1) + torch.from_numpy(rng.normal(0, 500.0 / 30.0, (V, M))).to(dev)).contiguous()
    del c0, c1, f
    props = torch.from_numpy(rng.uniform(0.5, 5.0, (1, N))).to(dev)
    seed = 7
    params = engine.fit_batch_dev(plan, d_Y, d_pk, 2)
    pred = engine.predict_dev(plan, params, d_pk, 2)
    Ys, pk_rep, status = engine.boot_resample_dev(d_Y, pred, params, 2, B=B, seed=seed, d_peaks=d_pk)
    assert not bool(status.any())
    rows = Ys.reshape(V * B, M)
    st = torch.cuda.current_stream(dev).cuda_stream

    def timed(fn):
        fn()                                   # warm-up at the timed shape
        torch.cuda.synchronize(dev)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize(dev)
        return e0.elapsed_time(e1) * 1e-3, out

    kw = dict(B=B, seed=seed, d_props=props, keep=True)
    t_yard, ref = timed(lambda: engine.fit_batch_dev(plan, rows, pk_rep, 2, check=False))
    t_boot, res = timed(lambda: engine.fit_bootstrap_dev(plan, d_Y, d_pk, 2, **kw))
    same = bool(torch.equal(res["replicates"].reshape(V * B, -1), ref))
    del res
    t_in, res = timed(lambda: engine.fit_bootstrap_dev(plan, d_Y, d_pk, 2, d_params=params, d_pred=pred, **kw))
    same = same and bool(torch.equal(res["replicates"].reshape(V * B, -1), ref))
    L.check(L.lib().mfx_plan_status(plan.handle(), st))
    assert same, "the bootstrap's replicate rows differ from the plain fit on the same signals"
    agree = res["agree"].double().mean().item() / B
    chunk = max(1, min(V, engine.BOOT_DEFAULT_BYTES // (B * M * 8)))
    out = {"what": "boot_dev_time", "N": N, "M": M, "V": V, "B": B, "chunks": -(-V // chunk), "bootstrap_s": t_boot,
           "bootstrap_handed_in_s": t_in, "yardstick_fit_batch_dev_s": t_yard, "ratio": t_boot / t_yard,
           "ratio_handed_in": t_in / t_yard, "replicate_rows_per_s": V * B / t_boot, "rows_equal_yardstick": same,
           "mean_agreement": agree, "expectation_ratio_at_most": 1.15}
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
