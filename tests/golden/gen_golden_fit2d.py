#!/usr/bin/env python3
"""Generate tests/golden/fit2d_cases.npz by RUNNING THE REFERENCE's chain for voxels of a 2-D protocol:

    D_k = rotate_atom_2Dprotocol(sig, sch_mat, refdir, peaks[3k:3k+3], DIFF)      k < K
    A   = [D_0 | ... | D_{K-1} | sig_csf if flagged]
    w, ind, _, SoS, y_rec = solve_exhaustive_posweights(A, y, [N]*K (+[1]))
    row = the packing of mf.py:420-450 (written out below from the solver's outputs)

Runs only in the build container, next to gen_golden.py (whose import_reference() it uses) and gen_golden_rot2d.py
(whose atoms() makes the dictionaries).  The two schemes come from rot2d_cases.npz and are not stored again.
Protocols: syn2_sch (66 rows, N = 24 atoms) and fix_sch (1776 rows, N = 8 atoms); classes K = 1 and K = 2, some
voxels with a CSF column; signals are noise-free mixtures of reference-rotated atoms with Rician noise at SNR 30.
Stored per protocol: the dictionary, sig_csf, and per voxel the directions, K, the CSF flag, the signal, the
reference's parameter row, and the best and runner-up objective over ALL index tuples (scipy.optimize.nnls per
tuple).  The generator ASSERTS for every voxel that they differ by more than 1e-8 |y|^2 - 100 times what the 1e-10
rotation tolerance can move an objective - so that the reference's choice is the choice; no voxel is dropped.

Usage:  OPENBLAS_NUM_THREADS=1 python tests/golden/gen_golden_fit2d.py
"""
import os
import sys

os.environ.setdefault("OPENBLAS_NUM_THREADS", "1")
os.environ.setdefault("OMP_NUM_THREADS", "1")

import numpy as np  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden  # noqa: E402
import gen_golden_rot2d as g2  # noqa: E402

DIFF = 2.2e-9
D_CSF = 3.0e-9
SNR = 30.0
GAP = 1e-8
REFDIR = np.array([0.0, 0.0, 1.0])
# (K, csf) classes and voxels per class, per protocol
PLAN = {"syn2": (24, 11, 0.1, [(1, 0, 4), (1, 1, 3), (2, 0, 6), (2, 1, 3)]),
        "fix": (8, 12, 0.3, [(1, 0, 2), (1, 1, 2), (2, 0, 4), (2, 1, 2)])}


def pack_row(w, ind, SoS, y, y_rec, K, csf, maxfasc, csf_on):
    """mf.py:420-450 for one voxel without an EAR compartment."""
    row = np.zeros(1 + 2 * maxfasc + csf_on + 2)
    M0 = np.sum(w)
    nu = w / M0 if np.abs(M0) > 0 else w
    row[0] = M0
    row[1:K + 1] = nu[:K]
    row[1 + maxfasc:1 + maxfasc + K] = ind[:K]
    if csf:
        row[1 + 2 * maxfasc] = nu[K]
    row[-2] = SoS / y.size
    if y.size > 1 and np.std(y_rec) > 0 and np.std(y) > 0:
        row[-1] = np.corrcoef(y, y_rec)[0, 1] ** 2
    return row


def tuple_objectives(Ds, xc, y):
    """min_{w >= 0} |y - A_t w|^2 of every index tuple t (one atom per dictionary, then the CSF column)."""
    from scipy.optimize import nnls
    N = Ds[0].shape[1]
    shape = (N,) * len(Ds)
    out = np.zeros(shape)
    for t in np.ndindex(*shape):
        cols = [D[:, i] for D, i in zip(Ds, t)] + ([xc] if xc is not None else [])
        out[t] = nnls(np.stack(cols, axis=1), y)[1] ** 2
    return out.reshape(-1)


def main():
    mfu, _ = gen_golden.import_reference()
    rot = np.load(os.path.join(HERE, "rot2d_cases.npz"))
    rng = np.random.default_rng(20261017)
    out = {}
    maxfasc, csf_on = 2, 1
    for name, (N, seed, zmin, classes) in PLAN.items():
        sch = rot[name + "_sch"]
        dic = g2.atoms(sch, N, seed)
        G, Dl, dl = sch[:, 3], sch[:, 4], sch[:, 5]
        sig_csf = np.exp(-(g2.GAM * G * dl) ** 2 * (Dl - dl / 3) * D_CSF)
        M = sch.shape[0]
        peaks, Ks, csfs, Ys, rows, objs, ysqs = [], [], [], [], [], [], []
        for K, csf, nvox in classes:
            for _ in range(nvox):
                dirs = g2.random_dirs(rng, K, zmin)
                while K == 2 and abs(dirs[0] @ dirs[1]) > 0.8:       # crossing angle above 37 degrees
                    dirs = g2.random_dirs(rng, K, zmin)
                Ds = [mfu.rotate_atom_2Dprotocol(dic.copy(), sch.copy(), REFDIR.copy(), d.copy(), DIFF) for d in dirs]
                ids = rng.integers(0, N, K)
                f_csf = 0.2 if csf else 0.0
                f = rng.uniform(0.35, 0.65, K)
                f = f / f.sum() * (1.0 - f_csf)
                clean = sum(fk * D[:, i] for fk, D, i in zip(f, Ds, ids)) + f_csf * sig_csf
                sigma = 1.0 / SNR
                y = np.sqrt((clean + sigma * rng.standard_normal(M)) ** 2 + (sigma * rng.standard_normal(M)) ** 2)
                A = np.hstack(Ds + ([sig_csf[:, None]] if csf else []))
                sizes = np.array([N] * K + ([1] if csf else []))
                w, ind, _, SoS, y_rec = mfu.solve_exhaustive_posweights(A.copy(), y.copy(), sizes)
                row = pack_row(np.asarray(w, dtype=np.float64), np.asarray(ind), SoS, y, np.asarray(y_rec), K, csf,
                               maxfasc, csf_on)
                o = np.sort(tuple_objectives(Ds, sig_csf if csf else None, y))
                ysq = float(np.sum(y ** 2))
                assert abs(o[0] - SoS) <= 1e-9 * ysq, (name, K, csf, o[0], SoS)
                assert o[1] - o[0] > GAP * ysq, (name, K, csf, (o[1] - o[0]) / ysq)
                print(name, "K", K, "csf", csf, "atoms", ind[:K], "gap/|y|^2 %.2e" % ((o[1] - o[0]) / ysq), flush=True)
                pk = np.zeros(3 * maxfasc)
                pk[:3 * K] = dirs.reshape(-1)
                peaks.append(pk); Ks.append(K); csfs.append(csf); Ys.append(y); rows.append(row)
                objs.append(o[:2]); ysqs.append(ysq)
        out[name + "_dic"] = dic
        out[name + "_sig_csf"] = sig_csf
        out[name + "_peaks"] = np.array(peaks)
        out[name + "_K"] = np.array(Ks, dtype=np.int32)
        out[name + "_csf"] = np.array(csfs, dtype=np.uint8)
        out[name + "_Y"] = np.array(Ys)
        out[name + "_params"] = np.array(rows)
        out[name + "_obj2"] = np.array(objs)          # best and runner-up objective over all tuples
        out[name + "_ysq"] = np.array(ysqs)
    out["DIFF"] = np.array(DIFF)
    out["gap"] = np.array(GAP)
    path = os.path.join(HERE, "fit2d_cases.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
