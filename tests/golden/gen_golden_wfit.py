#!/usr/bin/env python3
"""Generate tests/golden/wfit_cases.npz by RUNNING THE REFERENCE's chain on ROW-DELETED protocols: the referee of the
weighted fit (include/mfx_wfit.h) for 0/1 weights.  Per voxel, with `keep` the rows whose weight is 1:

    D_k = interp_PGSE_from_multishell(sch[keep], peaks[3k:3k+3], msinterp)          k < K
    A   = [D_0 | ... | D_{K-1} | sig_csf[keep] if flagged]
    w, ind, _, SoS, y_rec = solve_exhaustive_posweights(A, y[keep], [N]*K (+[1]))
    row = the packing of mf.py:420-450 on the kept rows (MSE = SoS / len(keep), R2 = corrcoef(y[keep], y_rec)^2)

Runs only in the build container, next to gen_golden.py (whose import_reference() it uses).  Two models, neither
stored again: "fc" is the model of fit_cases.npz (14 atoms, 64 rows, 7 of them G-bracketed), "uk" the UKBB dictionary
of real_ukbb.npz sub-sampled to every 27th atom (37 atoms) on the subject's protocol (105 rows, G-bracketed).  Classes
K in {0, 1, 2} with and without a CSF column; every voxel has its own 0/1 mask, and the masked measurements are
corrupted (multiplied by U(0.1, 0.5)) so that a fit which ignored the mask would see another signal.
Stored per model: the atoms' indices, sig_csf, and per voxel the directions, K, the CSF flag, the signal, the mask,
the reference's parameter row, and the best and runner-up objective over ALL index tuples (scipy.optimize.nnls per
tuple).  The generator ASSERTS for every voxel that they differ by at least 1e-8 |y[keep]|^2, so that the reference's
choice is the choice; no voxel is dropped.

Usage:  OPENBLAS_NUM_THREADS=1 python tests/golden/gen_golden_wfit.py
"""
import os
import sys

os.environ.setdefault("OPENBLAS_NUM_THREADS", "1")
os.environ.setdefault("OMP_NUM_THREADS", "1")

import numpy as np  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden  # noqa: E402
from gen_golden_fit2d import pack_row, tuple_objectives  # noqa: E402

GAP = 1e-8
M0, SNR = 500.0, 30.0
# (K, csf, voxels) per model
CLASSES = {"fc": [(0, 0, 1), (0, 1, 2), (1, 0, 3), (1, 1, 3), (2, 0, 5), (2, 1, 3)],
           "uk": [(1, 0, 2), (2, 0, 4), (2, 1, 2)]}
N_MASKED = {"fc": 8, "uk": 12}


def main():
    mfu, _ = gen_golden.import_reference()
    fc = np.load(os.path.join(HERE, "fit_cases.npz"))
    uk = np.load(os.path.join(HERE, "real_ukbb.npz"))
    uk_atoms = np.arange(0, uk["dictionary"].shape[1], 27)
    models = {
        "fc": (fc["dictionary"], fc["sch_ms"], np.array([0.0, 0.0, 1.0]), fc["sch"], float(fc["T2_csf"]), float(fc["DIFF_csf"])),
        "uk": (np.ascontiguousarray(uk["dictionary"][:, uk_atoms]), uk["sch_mat"], uk["orientation"], uk["sch_subj"],
               float(uk["T2_csf"]), float(uk["DIFF_csf"])),
    }
    rng = np.random.default_rng(20261018)
    out = {"uk_atoms": uk_atoms, "gap": np.array(GAP)}
    maxfasc, csf_on = 2, 1
    for name, (dic, sch_ms, ordir, sch, T2c, Dc) in models.items():
        ms = mfu.init_PGSE_multishell_interp(dic.copy(), sch_ms.copy(), ordir.copy())
        M, N = sch.shape[0], dic.shape[1]
        b = (gen_golden.GAM * sch[:, 3] * sch[:, 5]) ** 2 * (sch[:, 4] - sch[:, 5] / 3)
        sig_csf = np.exp(-sch[:, 6] / T2c) * np.exp(-b * Dc)
        peaks, Ks, csfs, Ys, Ws, rows, objs, ysqs = [], [], [], [], [], [], [], []
        for K, csf, nvox in CLASSES[name]:
            for _ in range(nvox):
                dirs = gen_golden.unit(rng, K)
                while K == 2 and abs(dirs[0] @ dirs[1]) > 0.8:
                    dirs = gen_golden.unit(rng, K)
                full = [mfu.interp_PGSE_from_multishell(sch.copy(), d.copy(), msinterp=ms) for d in dirs]
                comps = [D[:, rng.integers(0, N)] for D in full] + ([sig_csf] if csf else [])
                y = rng.normal(0, M0 / SNR, M)
                if comps:
                    y += M0 * np.stack(comps, 1) @ rng.dirichlet(4 * np.ones(len(comps)))
                bad = rng.choice(M, N_MASKED[name], replace=False)
                y[bad] *= rng.uniform(0.1, 0.5, bad.size)
                W = np.ones(M, dtype=np.uint8)
                W[bad] = 0
                keep = np.flatnonzero(W)
                yk = y[keep].copy()
                pk = np.zeros(3 * maxfasc)
                pk[:3 * K] = dirs.reshape(-1)
                if K == 0 and not csf:                      # mf.py:387: nothing to fit, a zero row
                    row, o, ysq = np.zeros(1 + 2 * maxfasc + csf_on + 2), np.zeros(2), float(np.sum(yk ** 2))
                else:
                    sch_k = np.ascontiguousarray(sch[keep])
                    Ds = [mfu.interp_PGSE_from_multishell(sch_k.copy(), d.copy(), msinterp=ms) for d in dirs]
                    for D, F in zip(Ds, full):              # a row's entry does not depend on the other rows
                        assert np.array_equal(D, F[keep])
                    A = np.hstack(Ds + ([sig_csf[keep, None]] if csf else []))
                    sizes = np.array([N] * K + ([1] if csf else []))
                    w, ind, _, SoS, y_rec = mfu.solve_exhaustive_posweights(A.copy(), yk.copy(), sizes)
                    row = pack_row(np.asarray(w, dtype=np.float64), np.asarray(ind), SoS, yk, np.asarray(y_rec), K, csf,
                                   maxfasc, csf_on)
                    ysq = float(np.sum(yk ** 2))
                    if K > 0:
                        o = np.sort(tuple_objectives(Ds, sig_csf[keep] if csf else None, yk))
                        assert abs(o[0] - SoS) <= 1e-9 * ysq, (name, K, csf, o[0], SoS)
                        if o.size > 1:
                            assert o[1] - o[0] >= GAP * ysq, (name, K, csf, (o[1] - o[0]) / ysq)
                        o = np.array([o[0], o[1] if o.size > 1 else np.inf])
                    else:                                   # the CSF column alone: one tuple
                        o = np.array([SoS, np.inf])
                    print(name, "K", K, "csf", csf, "atoms", ind[:K], "gap/|y|^2 %.2e" % ((o[1] - o[0]) / ysq), flush=True)
                peaks.append(pk); Ks.append(K); csfs.append(csf); Ys.append(y); Ws.append(W); rows.append(row)
                objs.append(o); ysqs.append(ysq)
        out[name + "_sig_csf"] = sig_csf
        out[name + "_peaks"] = np.array(peaks)
        out[name + "_K"] = np.array(Ks, dtype=np.int32)
        out[name + "_csf"] = np.array(csfs, dtype=np.uint8)
        out[name + "_Y"] = np.array(Ys)
        out[name + "_W"] = np.array(Ws)
        out[name + "_params"] = np.array(rows)
        out[name + "_obj2"] = np.array(objs)          # best and runner-up objective over all tuples (kept rows)
        out[name + "_ysq"] = np.array(ysqs)           # |y[keep]|^2
    path = os.path.join(HERE, "wfit_cases.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
