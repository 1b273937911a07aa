#!/usr/bin/env python3
"""Generate tests/golden/predict_cases.npz: the reference's parameter row and its reconstructed signal y_rec
for the voxels of the fit fixtures.

Runs only in the build container, next to gen_golden.py (whose import_reference() it uses).
For every voxel of fit_cases.npz, fit_cases_k1.npz, fit_c2_small.npz and the three real_ukbb_fit_*.npz classes
the reference's own per-voxel routine (mf.py:_fit_voxel) runs: it assembles the voxel's dictionary with
interp_PGSE_from_multishell, calls solve_exhaustive_posweights and packs the parameter row.  The solver's fifth
output, y_rec, which _fit_voxel drops, is caught on its way out.  Stored per class <c>:
  <c>_params [V x num_params]   the reference's parameter rows (M0, nu_f, ID_f, nu_csf, nu_ear, ID_ear, MSE, R2)
  <c>_yrec   [V x M]            the reference's y_rec (zeros where the voxel has no compartment)
  <c>_flags  [3]                maxfasc, csf_on, ear_on of the class
  <c>_numfasc, <c>_csf, <c>_ear [V]   per-voxel compartments
plus the message of gen_SoS_MRI's ValueError and the reference's own agreement between y_rec and its MSE.
Only arrays and strings are stored.

The pure-Python solver needs minutes per voxel at the 986-atom dictionary; voxels are spread over processes.

Usage:  OPENBLAS_NUM_THREADS=1 python tests/golden/gen_golden_predict.py [processes]
"""
import multiprocessing as mp
import os
import sys

os.environ.setdefault("OPENBLAS_NUM_THREADS", "1")
os.environ.setdefault("OMP_NUM_THREADS", "1")

import numpy as np  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden  # noqa: E402

Z = np.array([0.0, 0.0, 1.0])


def load(name):
    return np.load(os.path.join(HERE, name + ".npz"))


def classes():
    """name -> (model arrays, scheme, Y, peaks, numfasc, csf, ear, maxfasc, csf_on, ear_on)"""
    fc, k1, c2, uk = load("fit_cases"), load("fit_cases_k1"), load("fit_c2_small"), load("real_ukbb")
    small = dict(dictionary=fc["dictionary"], sch_mat=fc["sch_ms"], num_atom=int(fc["N"]), num_ear=int(fc["E"]),
                 T2_csf=float(fc["T2_csf"]), DIFF_csf=float(fc["DIFF_csf"]), T2_ear=float(fc["T2_ear"]),
                 DIFF_ear=fc["DIFF_ear"])
    c2m = dict(dictionary=c2["dictionary"], sch_mat=c2["sch_ms"], num_atom=c2["dictionary"].shape[1], num_ear=0,
               T2_csf=2.0, DIFF_csf=3.0e-9, T2_ear=0.08, DIFF_ear=np.zeros(0))
    ukm = dict(dictionary=uk["dictionary"], sch_mat=uk["sch_mat"], num_atom=int(uk["num_atom"]),
               num_ear=int(uk["num_ear"]), T2_csf=float(uk["T2_csf"]), DIFF_csf=float(uk["DIFF_csf"]),
               T2_ear=float(uk["T2_ear"]), DIFF_ear=uk["DIFF_ear"])
    out = {}
    out["fit_cases"] = (small, fc["sch"], fc["Y"], fc["peaks"], fc["numfasc"], fc["csf"], fc["ear"], 2, 1, 1)
    V = k1["Y"].shape[0]
    out["fit_cases_k1"] = (small, fc["sch"], k1["Y"], k1["peaks"], np.ones(V, int), np.zeros(V, bool), np.zeros(V, bool),
                           1, 0, 0)
    V = c2["Y"].shape[0]
    out["fit_c2_small"] = (c2m, c2["sch_ms"], c2["Y"], c2["peaks"], np.full(V, 2), np.zeros(V, bool), np.zeros(V, bool),
                           2, 0, 0)
    for name in ("k2", "k2csf", "k2csfear"):
        r = load("real_ukbb_fit_" + name)
        V = r["Y"].shape[0]
        c, e = int(r["csf"]), int(r["ear"])
        out["real_ukbb_fit_" + name] = (ukm, uk["sch_subj"], r["Y"], r["peaks"], np.full(V, 2), np.full(V, bool(c)),
                                       np.full(V, bool(e)), 2, c, e)
    return out


def run_voxel(task):
    cname, v = task
    mfu, mfmod = gen_golden.import_reference()
    md, sch, Y, peaks, numfasc, csf, ear, maxfasc, csf_on, ear_on = classes()[cname]
    sch = np.ascontiguousarray(sch, dtype=np.float64)
    ms = mfu.init_PGSE_multishell_interp(md["dictionary"], md["sch_mat"], Z)
    gam = mfu.get_gyromagnetic_ratio('H')
    G, Delta, delta, TE = sch[:, 3], sch[:, 4], sch[:, 5], sch[:, 6]
    b = (gam * G * delta) ** 2 * (Delta - delta / 3)
    M, N, E = sch.shape[0], md["num_atom"], md["num_ear"]
    sm = {'ROI_size': Y.shape[0], 'pgse_scheme': sch, 'ms_interpolator': ms, 'num_atom': N, 'num_ear': E,
          'maxfasc': maxfasc, 'csf_on': csf_on, 'ear_on': ear_on, 'VRB': 0, 'disp_int': 1,
          'D': np.zeros((M, maxfasc * N + 1 + E))}
    if csf_on:
        sm['sig_csf'] = np.exp(-TE / md["T2_csf"]) * np.exp(-b * md["DIFF_csf"])
    if ear_on:
        sm['sig_ear'] = np.stack([np.exp(-TE / md["T2_ear"]) * np.exp(-b * d) for d in md["DIFF_ear"]], axis=1)
    caught = []
    solve = mfu.solve_exhaustive_posweights

    def recording(A, y, dicsizes, *a, **k):
        res = solve(A, y, dicsizes, *a, **k)
        caught.append(np.array(res[4], dtype=np.float64))
        return res
    mfu.solve_exhaustive_posweights = recording
    try:
        vox = {'y': Y[v], 'K': int(numfasc[v]), 'csf_i': bool(csf[v]), 'ear_i': bool(ear[v]), 'peaks': peaks[v]}
        row = mfmod._fit_voxel(v, vox, sm)
    finally:
        mfu.solve_exhaustive_posweights = solve
    yrec = caught[0] if caught else np.zeros(M)
    return cname, v, np.asarray(row, dtype=np.float64), yrec


def main():
    nproc = int(sys.argv[1]) if len(sys.argv) > 1 else 8
    cl = classes()
    # the slow classes first so that the pool's tail is short
    order = ["real_ukbb_fit_k2csfear", "real_ukbb_fit_k2csf", "real_ukbb_fit_k2", "fit_c2_small", "fit_cases", "fit_cases_k1"]
    tasks = [(c, v) for c in order for v in range(cl[c][2].shape[0])]
    with mp.Pool(nproc) as pool:
        res = pool.map(run_voxel, tasks, chunksize=1)
    out = {"classes": np.array(sorted(cl))}
    worst = 0.0
    for c in cl:
        md, sch, Y, peaks, numfasc, csf, ear, maxfasc, csf_on, ear_on = cl[c]
        rows = sorted([r for r in res if r[0] == c], key=lambda r: r[1])
        P = np.stack([r[2] for r in rows])
        R = np.stack([r[3] for r in rows])
        out[c + "_params"], out[c + "_yrec"] = P, R
        out[c + "_flags"] = np.array([maxfasc, csf_on, ear_on], dtype=np.int64)
        out[c + "_numfasc"] = np.asarray(numfasc, dtype=np.int64)
        out[c + "_csf"] = np.asarray(csf, dtype=bool)
        out[c + "_ear"] = np.asarray(ear, dtype=bool)
        if c == "fit_cases":   # the reference's own y_rec against its own MSE (the cancellation error of its Gram route)
            mse_sig = np.mean((Y - R) ** 2, axis=1)
            big = P[:, -2] > 1.0
            rel = np.abs(mse_sig[big] - P[big, -2]) / P[big, -2]
            worst = float(rel.max())
            out["fit_cases_ref_mse_rel"] = np.float64(worst)
            out["fit_cases_ref_mse_nvox"] = np.int64(big.sum())
    mfu, _ = gen_golden.import_reference()
    try:
        mfu.gen_SoS_MRI(np.ones((3, 4)), np.ones((4, 3)), 1)
    except ValueError as e:
        out["sos_shape_error"] = np.array(str(e))
    np.savez_compressed(os.path.join(HERE, "predict_cases.npz"), **out)
    print("predict_cases.npz written; reference y_rec vs its MSE on fit_cases: %.3g relative over %d voxels"
          % (worst, int(out["fit_cases_ref_mse_nvox"])))


if __name__ == "__main__":
    main()
