#!/usr/bin/env python3
"""Generate tests/golden/wfit2d_cases.npz by RUNNING THE REFERENCE's chain for voxels of a 2-D protocol on rows scaled
by s = sqrt(W):

    D_k = rotate_atom_2Dprotocol(sig, sch_mat, refdir, peaks[3k:3k+3], DIFF)      k < K
    A   = s[:, None] * [D_0 | ... | D_{K-1} | sig_csf if flagged],   y' = s * y
    w, ind, _, SoS, y_rec = solve_exhaustive_posweights(A, y', [N]*K (+[1]))
    row = the packing of mf.py:420-450 with MSE = SoS / sum W and the weighted R2 of y and the unscaled y_rec

Runs only in the build container, next to gen_golden.py (whose import_reference() it uses).  The voxels are those of
fit2d_cases.npz (syn2: 66 rows, 24 atoms; fix: 1776 rows, 8 atoms; K = 1 and 2, some with a CSF column; the schemes
come from rot2d_cases.npz); nothing of them is stored again.  Three kinds of weights per protocol <p>:
  mask    <p>_W_mask [V x M] uint8: per voxel about a tenth of the rows dropped
  smooth  <p>_W_smooth [V x M]: 0.25 * 16^u, u the row's delta scaled to [0, 1] (even voxels) or 1 minus it (odd voxels)
  shared  <p>_W_shared [M]: one vector for all voxels, 0.5 + Delta scaled to [0, 1.5], every 13th row 0
Stored per kind <k>: <p>_params_<k> [V x 7] the parameter rows, <p>_obj2_<k> [V x 2] the best and runner-up objective over
ALL index tuples (scipy.optimize.nnls per tuple), <p>_ysq_<k> [V] |y'|^2; for syn2's K = 2 voxels without CSF
(syn2_vox2) also syn2_FW_<k> [n2 x N x N], F_W of every atom pair from the reference's lsqnonneg_2var_opt on np.dot
sums of the scaled columns, syn2_c2_<k> the pairs' 1 - c^2, and syn2_dFW_<k> a bound on how far the rotation's tolerance
can move F_W: gen_golden_soft2d.py's derivation with the scaled column's move e(a) = 1e-10 ||s a|| + 1e-13 ||s||.

The generator ASSERTS for every voxel a top-2 gap above 1e-8 |y'|^2 (no voxel is dropped), and for the masks that the
chain on the rotated dictionaries with the masked rows DELETED returns the same indices.

Usage:  OPENBLAS_NUM_THREADS=1 python tests/golden/gen_golden_wfit2d.py
"""
import os
import sys

os.environ.setdefault("OPENBLAS_NUM_THREADS", "1")
os.environ.setdefault("OMP_NUM_THREADS", "1")

import numpy as np  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden  # noqa: E402
from gen_golden_fit2d import tuple_objectives  # noqa: E402

REFDIR = np.array([0.0, 0.0, 1.0])
GAP = 1e-8
KINDS = ("mask", "smooth", "shared")


def unit(x):
    return (x - x.min()) / (x.max() - x.min())


def weights(sch, V, rng):
    M = sch.shape[0]
    mask = np.ones((V, M), dtype=np.uint8)
    for v in range(V):
        mask[v, rng.choice(M, max(1, M // 10), replace=False)] = 0
    u = unit(sch[:, 5])
    smooth = np.array([0.25 * 16.0 ** (u if v % 2 == 0 else 1.0 - u) for v in range(V)])
    shared = 0.5 + 1.5 * unit(sch[:, 4])
    shared[::13] = 0.0
    return {"mask": mask, "smooth": smooth, "shared": shared}


def weighted_r2(y, yrec, w):
    """the restatement of tests/_wfit_ref.py"""
    if np.count_nonzero(w > 0) < 2:
        return 0.0
    sw = np.sum(w)
    my, mr = np.sum(w * y) / sw, np.sum(w * yrec) / sw
    cyy, crr, cyr = np.sum(w * (y - my) ** 2), np.sum(w * (yrec - mr) ** 2), np.sum(w * (y - my) * (yrec - mr))
    if not (cyy > 0 and crr > 0):
        return 0.0
    return float(np.clip(cyr / np.sqrt(cyy) / np.sqrt(crr), -1.0, 1.0) ** 2)


def main():
    mfu, _ = gen_golden.import_reference()
    rot = np.load(os.path.join(HERE, "rot2d_cases.npz"))
    gold = np.load(os.path.join(HERE, "fit2d_cases.npz"))
    DIFF = float(gold["DIFF"])
    rng = np.random.default_rng(20261018)
    maxfasc, csf_on = 2, 1
    out = {"gap": np.array(GAP)}
    for name in ("syn2", "fix"):
        sch, dic, sig_csf = rot[name + "_sch"], gold[name + "_dic"], gold[name + "_sig_csf"]
        M, N = dic.shape
        Ks, csfs, Y, peaks = gold[name + "_K"], gold[name + "_csf"].astype(bool), gold[name + "_Y"], gold[name + "_peaks"]
        V = Y.shape[0]
        Ws = weights(sch, V, rng)
        vox2 = np.flatnonzero((Ks == 2) & ~csfs)
        res = {k: {"params": [], "obj2": [], "ysq": [], "FW": [], "c2": [], "dF": []} for k in KINDS}
        for v in range(V):
            K, csf, y = int(Ks[v]), bool(csfs[v]), Y[v]
            Ds = [mfu.rotate_atom_2Dprotocol(dic.copy(), sch.copy(), REFDIR.copy(), peaks[v, 3 * k:3 * k + 3].copy(), DIFF)
                  for k in range(K)]
            sizes = np.array([N] * K + ([1] if csf else []))
            for kind in KINDS:
                w = np.asarray(Ws[kind][v] if kind != "shared" else Ws[kind], dtype=np.float64)
                s = np.sqrt(w)
                Dss = [s[:, None] * D for D in Ds]
                xs = s * sig_csf if csf else None
                ys = s * y
                A = np.hstack(Dss + ([xs[:, None]] if csf else []))
                wt, ind, _, SoS, _ = mfu.solve_exhaustive_posweights(A.copy(), ys.copy(), sizes)
                wt, ind = np.asarray(wt, dtype=np.float64), np.asarray(ind)
                Au = np.hstack(Ds + ([sig_csf[:, None]] if csf else []))
                tot = np.concatenate([ind[:K] + N * np.arange(K), [K * N] if csf else []]).astype(int)
                row = np.zeros(1 + 2 * maxfasc + csf_on + 2)
                M0 = np.sum(wt)
                nu = wt / M0 if np.abs(M0) > 0 else wt
                row[0], row[1:K + 1], row[1 + maxfasc:1 + maxfasc + K] = M0, nu[:K], ind[:K]
                if csf:
                    row[1 + 2 * maxfasc] = nu[K]
                row[-2] = SoS / np.sum(w)
                row[-1] = weighted_r2(y, Au[:, tot] @ wt, w)
                o = np.sort(tuple_objectives(Dss, xs, ys))
                ysq = float(np.sum(ys ** 2))
                assert abs(o[0] - SoS) <= 1e-9 * ysq, (name, kind, v, o[0], SoS)
                assert o[1] - o[0] > GAP * ysq, (name, kind, v, (o[1] - o[0]) / ysq)
                if kind == "mask":      # the chain on the deleted rows: the same atoms
                    keep = w > 0
                    _, ind_d, _, SoS_d, _ = mfu.solve_exhaustive_posweights(np.ascontiguousarray(Au[keep]), y[keep].copy(), sizes)
                    assert np.array_equal(np.asarray(ind_d)[:K], ind[:K]), (name, v, ind_d, ind)
                    assert abs(SoS_d - SoS) <= 1e-9 * ysq
                print(name, kind, "voxel", v, "K", K, "csf", int(csf), "atoms", ind[:K], "gap/|y'|^2 %.2e" % ((o[1] - o[0]) / ysq),
                      flush=True)
                r = res[kind]
                r["params"].append(row); r["obj2"].append(o[:2]); r["ysq"].append(ysq)
                if name == "syn2" and v in vox2:
                    F, c2, dF = np.zeros((N, N)), np.zeros((N, N)), np.zeros((N, N))
                    e0, e1 = (1e-10 * np.sqrt(np.sum(D * D, axis=0)) + 1e-13 * np.sqrt(np.sum(w)) for D in Dss)
                    for i in range(N):
                        for j in range(N):
                            a, b = Dss[0][:, i], Dss[1][:, j]
                            A11, A12, A22 = float(np.dot(a, a)), float(np.dot(a, b)), float(np.dot(b, b))
                            w2, F[i, j] = mfu.lsqnonneg_2var_opt(float(np.dot(ys, ys)), A11, A12, A22, float(np.dot(a, ys)),
                                                                 float(np.dot(b, ys)))
                            c2[i, j] = 1.0 - A12 * A12 / (A11 * A22)
                            e = w2[0] * e0[i] + w2[1] * e1[j]
                            dF[i, j] = 2.0 * np.sqrt(max(F[i, j], 0.0)) * e + e * e
                    assert not np.any((c2 >= 1e-8 / 4) & (c2 <= 4e-8)), (name, kind, v, "a pair near the cut")
                    r["FW"].append(F); r["c2"].append(c2); r["dF"].append(dF)
        out[name + "_W_mask"], out[name + "_W_smooth"], out[name + "_W_shared"] = Ws["mask"], Ws["smooth"], Ws["shared"]
        for kind in KINDS:
            r = res[kind]
            assert len(r["params"]) == V      # no voxel is dropped
            out["%s_params_%s" % (name, kind)] = np.array(r["params"])
            out["%s_obj2_%s" % (name, kind)] = np.array(r["obj2"])
            out["%s_ysq_%s" % (name, kind)] = np.array(r["ysq"])
            if name == "syn2":
                assert len(r["FW"]) == vox2.size
                out["syn2_FW_" + kind], out["syn2_c2_" + kind] = np.array(r["FW"]), np.array(r["c2"])
                out["syn2_dFW_" + kind] = np.array(r["dF"])
        if name == "syn2":
            out["syn2_vox2"] = vox2.astype(np.int32)
    path = os.path.join(HERE, "wfit2d_cases.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size < os.path.getsize(os.path.join(HERE, "rot2d_cases.npz")), size
    print("wrote", path, size, "bytes")


if __name__ == "__main__":
    main()
