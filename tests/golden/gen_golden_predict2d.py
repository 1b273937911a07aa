#!/usr/bin/env python3
"""Generate tests/golden/predict2d_cases.npz by RUNNING THE REFERENCE's chain on every voxel of fit2d_cases.npz and
keeping what the fit's golden file dropped: the solver's own reconstruction,

    D_k = rotate_atom_2Dprotocol(sig, sch_mat, refdir, peaks[3k:3k+3], DIFF)      k < K
    w, ind, _, SoS, y_recons = solve_exhaustive_posweights([D_0 | .. | sig_csf if flagged], y, [N]*K (+[1]))

Runs only in the build container, next to gen_golden.py (whose import_reference() it uses).  Schemes come from
rot2d_cases.npz, dictionaries, directions, classes and signals from fit2d_cases.npz; nothing of them is stored again.
Stored per protocol: y_rec [V x M] (fix as it is: 10 x 1776 doubles, compressed).  The generator asserts that the
reference's parameter row of every voxel is the one fit2d_cases.npz holds, so the two files describe the same fits.

Usage:  OPENBLAS_NUM_THREADS=1 python tests/golden/gen_golden_predict2d.py
"""
import os
import sys

os.environ.setdefault("OPENBLAS_NUM_THREADS", "1")
os.environ.setdefault("OMP_NUM_THREADS", "1")

import numpy as np  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden  # noqa: E402
import gen_golden_fit2d as gf  # noqa: E402

REFDIR = np.array([0.0, 0.0, 1.0])


def main():
    mfu, _ = gen_golden.import_reference()
    rot = np.load(os.path.join(HERE, "rot2d_cases.npz"))
    gold = np.load(os.path.join(HERE, "fit2d_cases.npz"))
    DIFF = float(gold["DIFF"])
    maxfasc, csf_on = 2, 1
    out = {}
    for name in ("syn2", "fix"):
        sch, dic, sig_csf = rot[name + "_sch"], gold[name + "_dic"], gold[name + "_sig_csf"]
        N = dic.shape[1]
        recs = []
        for v in range(gold[name + "_Y"].shape[0]):
            K, csf, y = int(gold[name + "_K"][v]), int(gold[name + "_csf"][v]), gold[name + "_Y"][v]
            dirs = gold[name + "_peaks"][v, :3 * K].reshape(K, 3)
            Ds = [mfu.rotate_atom_2Dprotocol(dic.copy(), sch.copy(), REFDIR.copy(), d.copy(), DIFF) for d in dirs]
            A = np.hstack(Ds + ([sig_csf[:, None]] if csf else []))
            sizes = np.array([N] * K + ([1] if csf else []))
            w, ind, _, SoS, y_rec = mfu.solve_exhaustive_posweights(A.copy(), y.copy(), sizes)
            y_rec = np.asarray(y_rec, dtype=np.float64).reshape(-1)
            row = gf.pack_row(np.asarray(w, dtype=np.float64), np.asarray(ind), SoS, y, y_rec, K, csf, maxfasc, csf_on)
            assert np.array_equal(row, gold[name + "_params"][v]), (name, v)
            recs.append(y_rec)
            print(name, "voxel", v, "K", K, "csf", csf, "max|y_rec| %.3f" % np.abs(y_rec).max(), flush=True)
        out[name + "_y_rec"] = np.array(recs)
    path = os.path.join(HERE, "predict2d_cases.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
