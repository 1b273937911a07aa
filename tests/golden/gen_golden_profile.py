#!/usr/bin/env python3
"""Generate tests/golden/profile_cases.npz: objective profiles from the unmodified reference.

Runs only in the build container, next to gen_golden.py (whose import_reference() it uses).
For every voxel of fit_c2_small.npz (48 atoms, two fascicles), of fit_cases_k1.npz (one fascicle) and the
CSF-flagged, EAR-free voxels of fit_cases.npz that have a fascicle, for every slot k and every atom i of it, the
reference's own solve_exhaustive_posweights runs on the dictionary restricted to that atom,

    [a_i | D_other (| x)]  with sizes [1, N (, 1)],   resp.   [D_other | a_i (| x)]  with sizes [N, 1 (, 1)],
    [a_i (| x)]            with sizes [1 (, 1)] for a single fascicle,

D_k = interp_PGSE_from_multishell(scheme, peaks_k) the rotated dictionaries of the voxel and x the CSF signal of
mf.py:919.  Stored per class <c> (arrays only):
  <c>_vox      [n]                  the voxels of the fixture the rows stand for
  <c>_K, <c>_csf [n]                their number of fascicles and CSF flag
  <c>_obj      [n x maxfasc x N]    the solver's minimum (sum of squares); NaN rows for an absent fascicle
  <c>_partner  [n x maxfasc x N]    the atom the solver chose in the other slot (-1: none)
  <c>_ysq      [n]                  ||y||^2
and the largest difference between the row minima and map_MSE * M of fit_c2_small (both come from the reference's
Gram arithmetic), in units of ||y||^2, which this script prints.

Usage:  OPENBLAS_NUM_THREADS=1 python tests/golden/gen_golden_profile.py
"""
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
    """name -> (dictionary, sch_ms, scheme, Y, peaks, numfasc, csf, voxels in scope, maxfasc, T2_csf, DIFF_csf)"""
    fc, k1, c2 = load("fit_cases"), load("fit_cases_k1"), load("fit_c2_small")
    out = {}
    V = c2["Y"].shape[0]
    out["fit_c2_small"] = (c2["dictionary"], c2["sch_ms"], c2["sch_ms"], c2["Y"], c2["peaks"], np.full(V, 2), np.zeros(V, bool),
                           np.arange(V), 2, 2.0, 3.0e-9)
    V = k1["Y"].shape[0]
    out["fit_cases_k1"] = (fc["dictionary"], fc["sch_ms"], fc["sch"], k1["Y"], k1["peaks"], np.ones(V, int), np.zeros(V, bool),
                           np.arange(V), 1, float(fc["T2_csf"]), float(fc["DIFF_csf"]))
    nf, csf, ear = fc["numfasc"].astype(int), fc["csf"] > 0, fc["ear"] > 0
    scope = np.flatnonzero(csf & ~ear & (nf >= 1) & (nf <= 2))
    out["fit_cases"] = (fc["dictionary"], fc["sch_ms"], fc["sch"], fc["Y"], fc["peaks"], nf, csf, scope, 2,
                        float(fc["T2_csf"]), float(fc["DIFF_csf"]))
    return out


def main():
    mfu, _ = gen_golden.import_reference()
    gam = mfu.get_gyromagnetic_ratio('H')
    out = {"classes": np.array(sorted(classes()))}
    for cname, (dic, sch_ms, sch, Y, peaks, numfasc, csf, scope, maxfasc, T2, Dc) in classes().items():
        sch = np.ascontiguousarray(sch, dtype=np.float64)
        ms = mfu.init_PGSE_multishell_interp(dic, sch_ms, Z)
        N, M = dic.shape[1], sch.shape[0]
        G, Delta, delta, TE = sch[:, 3], sch[:, 4], sch[:, 5], sch[:, 6]
        b = (gam * G * delta) ** 2 * (Delta - delta / 3)
        x = np.exp(-TE / T2) * np.exp(-b * Dc)   # mf.py:919
        obj = np.full((scope.size, maxfasc, N), np.nan)
        par = np.full((scope.size, maxfasc, N), -1, dtype=np.int32)
        for r, v in enumerate(scope):
            K = int(numfasc[v])
            y = np.ascontiguousarray(Y[v], dtype=np.float64)
            D = [np.array(mfu.interp_PGSE_from_multishell(sch, peaks[v, 3 * k:3 * k + 3], msinterp=ms)).reshape(M, N)
                 for k in range(K)]
            tail = [x[:, None]] if csf[v] else []
            for k in range(K):
                for i in range(N):
                    cols, sizes = [None] * K, [N] * K
                    cols[k], sizes[k] = D[k][:, i:i + 1], 1
                    if K == 2:
                        cols[1 - k] = D[1 - k]
                    A = np.ascontiguousarray(np.concatenate(cols + tail, axis=1))
                    w, sub, tot, mo, yrec = mfu.solve_exhaustive_posweights(A, y, np.array(sizes + [1] * len(tail)))
                    obj[r, k, i] = mo
                    if K == 2:
                        par[r, k, i] = int(sub[1 - k])
        out[cname + "_vox"] = scope.astype(np.int64)
        out[cname + "_K"] = numfasc[scope].astype(np.int64)
        out[cname + "_csf"] = np.asarray(csf[scope], dtype=bool)
        out[cname + "_obj"], out[cname + "_partner"] = obj, par
        out[cname + "_ysq"] = np.sum(Y[scope] ** 2, axis=1)
        print("%s: %d voxels, %d atoms" % (cname, scope.size, N))
    c2 = load("fit_c2_small")
    M = c2["Y"].shape[1]
    dev = np.abs(out["fit_c2_small_obj"][:, 0].min(axis=1) - c2["map_MSE"] * M) / out["fit_c2_small_ysq"]
    dev1 = np.abs(out["fit_c2_small_obj"][:, 1].min(axis=1) - c2["map_MSE"] * M) / out["fit_c2_small_ysq"]
    worst = float(max(dev.max(), dev1.max()))
    out["fit_c2_small_min_vs_mse"] = np.float64(worst)
    np.savez_compressed(os.path.join(HERE, "profile_cases.npz"), **out)
    print("profile_cases.npz written; row minima vs map_MSE * M of fit_c2_small: largest difference %.3g ||y||^2 "
          "(4 M eps = %.3g)" % (worst, 4 * M * np.finfo(float).eps))


if __name__ == "__main__":
    main()
