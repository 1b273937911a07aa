#!/usr/bin/env python3
"""Generate tests/golden/soft2d_cases.npz: the value of every atom pair of voxels of a 2-D protocol from the
unmodified reference.

Runs only in the build container, next to gen_golden.py (whose import_reference() it uses).  Inputs are the voxels
without a CSF column of fit2d_cases.npz (protocols syn2: 24 atoms x 66 rows, fix: 8 atoms x 1776 rows; the schemes come
from rot2d_cases.npz); nothing of them is stored again.  Per voxel the reference rotates the dictionary onto each
direction (rotate_atom_2Dprotocol) and

  K = 2   its own lsqnonneg_2var_opt gives F(i, j) for EVERY atom pair from ||y||^2, A11, A12, A22, Y1, Y2 (np.dot)
  K = 1   its own solve_exhaustive_posweights on the single column gives F(i)

Stored per protocol <p> (arrays only):
  <p>_vox2 [n2], <p>_vox1 [n1]   the voxels of fit2d_cases.npz the rows stand for
  <p>_F2   [n2 x N x N]          F(i, j);   <p>_F1 [n1 x N]  F(i)
  <p>_c2   [n2 x N x N]          1 - c^2 of every pair
  <p>_dF2  [n2 x N x N], <p>_dF1 [n1 x N]   a bound on how far the rotation's tolerance can move F (below)
  <p>_ysq2 [n2], <p>_ysq1 [n1]   ||y||^2
and `cut`, the cut on 1 - c^2 the values were checked against.

dF.  The library's rotation is held to the reference's within |dD| <= 1e-10 |D| + 1e-13 per entry
(tests/test_rot2d_gpu.py), so a column a moves by at most e(a) = 1e-10 ||a|| + 1e-13 sqrt(M) in norm.  F is the minimum
over the weights of ||y - w1 a - w2 b||^2; at the reference's own weights (w1, w2) the residual r has ||r||^2 = F, and
moving the columns moves the residual by at most e = w1 e(a) + w2 e(b), hence the minimum by at most
dF = 2 sqrt(F) e + e^2 (the minimum over w of the moved problem is at most its value at (w1, w2), and the same argument
holds from the other side with weights that differ by O(e)): both terms are computed from the reference's weights.

The generator ASSERTS for every voxel: no pair has 1 - c^2 within [cut / 4, 4 cut] (the cut can fall on one side only);
min F equals the golden fit's MSE * M within the profile tests' bar 16 M eps ||y||^2 / (1 - c^2) of the arg-min pair (both
come from the reference's closed form; only the order of the Gram sums differs); no voxel is dropped.

Usage:  OPENBLAS_NUM_THREADS=1 python tests/golden/gen_golden_soft2d.py
"""
import os
import sys

os.environ.setdefault("OPENBLAS_NUM_THREADS", "1")
os.environ.setdefault("OMP_NUM_THREADS", "1")

import numpy as np  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden  # noqa: E402

REFDIR = np.array([0.0, 0.0, 1.0])
CUT = 1e-8
EPS = float(np.finfo(np.float64).eps)
RTOL, ATOL = 1e-10, 1e-13      # the rotation's bar (tests/test_rot2d_gpu.py)


def col_move(D):
    """e(a) of every column: how far the rotation's tolerance can move it in norm"""
    return RTOL * np.sqrt(np.sum(D * D, axis=0)) + ATOL * np.sqrt(D.shape[0])


def main():
    mfu, _ = gen_golden.import_reference()
    rot = np.load(os.path.join(HERE, "rot2d_cases.npz"))
    gold = np.load(os.path.join(HERE, "fit2d_cases.npz"))
    DIFF = float(gold["DIFF"])
    out = {"cut": np.array(CUT)}
    for name in ("syn2", "fix"):
        sch, dic = rot[name + "_sch"], gold[name + "_dic"]
        M, N = dic.shape
        K, csf = gold[name + "_K"], gold[name + "_csf"].astype(bool)
        Y, peaks, params = gold[name + "_Y"], gold[name + "_peaks"], gold[name + "_params"]
        vox2, vox1 = np.flatnonzero((K == 2) & ~csf), np.flatnonzero((K == 1) & ~csf)
        F2, c2s, dF2, F1, dF1 = [], [], [], [], []
        for v in vox2:
            y = Y[v]
            D0, D1 = (mfu.rotate_atom_2Dprotocol(dic.copy(), sch.copy(), REFDIR.copy(), peaks[v, 3 * k:3 * k + 3].copy(), DIFF)
                      for k in range(2))
            ysq = float(np.dot(y, y))
            e0, e1 = col_move(D0), col_move(D1)
            F, c2, dF = np.zeros((N, N)), np.zeros((N, N)), np.zeros((N, N))
            for i in range(N):
                for j in range(N):
                    a, b = D0[:, i], D1[:, j]
                    A11, A12, A22 = float(np.dot(a, a)), float(np.dot(a, b)), float(np.dot(b, b))
                    w, res = mfu.lsqnonneg_2var_opt(ysq, A11, A12, A22, float(np.dot(a, y)), float(np.dot(b, y)))
                    F[i, j] = res
                    c2[i, j] = 1.0 - A12 * A12 / (A11 * A22)
                    e = w[0] * e0[i] + w[1] * e1[j]
                    dF[i, j] = 2.0 * np.sqrt(max(res, 0.0)) * e + e * e
            assert not np.any((c2 >= CUT / 4) & (c2 <= 4 * CUT)), (name, v, "a pair near the cut")
            im = np.unravel_index(np.argmin(F), F.shape)
            bar = 16 * M * EPS * ysq / c2[im]
            sos = params[v, -2] * M
            assert abs(F.min() - sos) <= bar, (name, v, F.min(), sos, bar)
            assert (im[0], im[1]) == (int(params[v, 3]), int(params[v, 4])), (name, v, im, params[v, 3:5])
            print(name, "K 2 voxel", v, "min F %.6e at %s, |min F - MSE M| = %.2e (bar %.2e), smallest 1 - c^2 %.2e, largest dF / "
                  "|y|^2 %.2e" % (F.min(), im, abs(F.min() - sos), bar, c2.min(), dF.max() / ysq), flush=True)
            F2.append(F); c2s.append(c2); dF2.append(dF)
        for v in vox1:
            y = Y[v]
            D0 = mfu.rotate_atom_2Dprotocol(dic.copy(), sch.copy(), REFDIR.copy(), peaks[v, 0:3].copy(), DIFF)
            e0 = col_move(D0)
            F, dF = np.zeros(N), np.zeros(N)
            for i in range(N):
                w, _, _, res, _ = mfu.solve_exhaustive_posweights(D0[:, i:i + 1].copy(), y.copy(), np.array([1]))
                F[i] = res
                e = float(np.asarray(w).reshape(-1)[0]) * e0[i]
                dF[i] = 2.0 * np.sqrt(max(res, 0.0)) * e + e * e
            ysq = float(np.dot(y, y))
            sos = params[v, -2] * M
            assert abs(F.min() - sos) <= 16 * M * EPS * ysq, (name, v, F.min(), sos)
            assert int(np.argmin(F)) == int(params[v, 3]), (name, v)
            print(name, "K 1 voxel", v, "min F %.6e, |min F - MSE M| = %.2e" % (F.min(), abs(F.min() - sos)), flush=True)
            F1.append(F); dF1.append(dF)
        assert len(F2) == vox2.size and len(F1) == vox1.size and vox2.size and vox1.size      # no voxel is dropped
        out[name + "_vox2"], out[name + "_vox1"] = vox2.astype(np.int32), vox1.astype(np.int32)
        out[name + "_F2"], out[name + "_c2"], out[name + "_dF2"] = np.array(F2), np.array(c2s), np.array(dF2)
        out[name + "_F1"], out[name + "_dF1"] = np.array(F1), np.array(dF1)
        out[name + "_ysq2"] = np.array([float(np.dot(Y[v], Y[v])) for v in vox2])
        out[name + "_ysq1"] = np.array([float(np.dot(Y[v], Y[v])) for v in vox1])
    path = os.path.join(HERE, "soft2d_cases.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size < os.path.getsize(os.path.join(HERE, "fit2d_cases.npz")), size
    print("wrote", path, size, "bytes")


if __name__ == "__main__":
    main()
