"""What the weighted fit's tests share: the two golden models, and the REFEREE of the GPU tests - the oracle's solver on
sqrt(W)-scaled oracle rotations plus the weighted row packing of include/mfx_wfit.h.  tests/test_wfit_host.py checks
this referee against the reference's own results (tests/golden/wfit_cases.npz) without a GPU."""
import os

import numpy as np

from oracle import oracle as orc

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
Z = np.array([0.0, 0.0, 1.0])
RTOL_W, ATOL = 1e-5, 1e-10


def num_params(maxfasc, csf_on):
    return 1 + 2 * maxfasc + int(csf_on) + 2


def golden_models():
    """name -> (dictionary [Mms x N], sch_ms, ordir, sch [M x 7]) of the models of wfit_cases.npz."""
    fc = np.load(os.path.join(G, "fit_cases.npz"))
    uk = np.load(os.path.join(G, "real_ukbb.npz"))
    gold = np.load(os.path.join(G, "wfit_cases.npz"))
    return {"fc": (fc["dictionary"], fc["sch_ms"], Z, fc["sch"]),
            "uk": (np.ascontiguousarray(uk["dictionary"][:, gold["uk_atoms"]]), uk["sch_mat"], uk["orientation"], uk["sch_subj"])}


def weighted_r2(y, yrec, w):
    """Squared weighted Pearson correlation (weights w, weighted means); 0 with fewer than two positive weights or a
    vanishing weighted variance.  For 0/1 weights: np.corrcoef over the kept rows."""
    if np.count_nonzero(w > 0) < 2:
        return 0.0
    sw = np.sum(w)
    my, mr = np.sum(w * y) / sw, np.sum(w * yrec) / sw
    cyy, crr, cyr = np.sum(w * (y - my) ** 2), np.sum(w * (yrec - mr) ** 2), np.sum(w * (y - my) * (yrec - mr))
    if not (cyy > 0 and crr > 0):
        return 0.0
    return float(np.clip(cyr / np.sqrt(cyy) / np.sqrt(crr), -1.0, 1.0) ** 2)


def scaled_problem(T, sch, y, w, dirs, csf, sig_csf):
    """(A unscaled [M x Ntot], s A, s y, dicsizes) of one voxel: oracle rotations, rows times s = sqrt(w)."""
    cols = [orc.interp(sch, d, T).reshape(sch.shape[0], -1) for d in dirs]
    if csf:
        cols.append(np.asarray(sig_csf, dtype=np.float64)[:, None])
    A = np.ascontiguousarray(np.hstack(cols))
    s = np.sqrt(np.asarray(w, dtype=np.float64))
    sizes = np.array([T["N"]] * len(dirs) + [1] * int(csf))
    return A, np.ascontiguousarray(s[:, None] * A), np.ascontiguousarray(s * y), sizes


def ref_row(T, sch, y, w, dirs, csf, sig_csf, maxfasc, csf_on, deleted=False):
    """The referee's params row of one voxel; deleted=True solves on the rows with w > 0 only (the row-deleted form)."""
    K = len(dirs)
    row = np.zeros(num_params(maxfasc, csf_on))
    if K + int(csf) == 0:
        return row
    w = np.asarray(w, dtype=np.float64)
    A, As, ys, sizes = scaled_problem(T, sch, y, w, dirs, csf, sig_csf)
    if deleted:
        keep = w > 0
        As, ys = np.ascontiguousarray(As[keep]), np.ascontiguousarray(ys[keep])
    wt, sub, tot, obj, _ = orc.solve_exhaustive_posweights(As, ys, sizes)
    M0 = np.sum(wt)
    nu = wt / M0 if np.abs(M0) > 0 else wt
    row[0] = M0
    row[1:K + 1] = nu[:K]
    row[1 + maxfasc:1 + maxfasc + K] = sub[:K]
    if csf:
        row[1 + 2 * maxfasc] = nu[K]
    row[-2] = obj / np.sum(w)
    row[-1] = weighted_r2(y, A[:, tot] @ wt, w)
    return row


def pair_gap(As, ys, N):
    """(best, runner-up) of min_{w >= 0} |ys - As[:, (i, N + j)] w|^2 over ALL pairs (i, j), by the closed form of the
    2 x 2 non-negative least squares: the unconstrained solution where it is positive, else the better single atom."""
    D0, D1 = As[:, :N], As[:, N:2 * N]
    a11, a22 = np.sum(D0 * D0, axis=0)[:, None], np.sum(D1 * D1, axis=0)[None, :]
    y1, y2 = (D0.T @ ys)[:, None], (D1.T @ ys)[None, :]
    a12 = D0.T @ D1
    d1, d2, det = a22 * y1 - a12 * y2, a11 * y2 - a12 * y1, a11 * a22 - a12 * a12
    both = (d1 > 0) & (d2 > 0) & (det > 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        sc2 = np.where(both, (y1 * d1 + y2 * d2) / det, 0.0)
    s1 = np.maximum(np.where(y1 > 0, y1 * y1 / a11, 0.0), np.where(y2 > 0, y2 * y2 / a22, 0.0))
    obj = np.sort((np.sum(ys * ys) - np.where(both, sc2, s1)).reshape(-1))
    return obj[0], obj[1]


def assert_rows(got, ref, maxfasc, what="", rtol=RTOL_W, atol=ATOL, r2_rtol=1e-9):
    """Atom indices equal; M0, nu, MSE within rtol (atol 1e-10); R2 within r2_rtol."""
    ids = slice(1 + maxfasc, 1 + 2 * maxfasc)
    assert got.shape == ref.shape, what
    assert np.all(np.isfinite(got)), what
    bad = np.flatnonzero(np.any(got[:, ids] != ref[:, ids], axis=1))
    assert bad.size == 0, "%s atom indices differ in voxels %s: %s vs %s" % (what, bad[:8], got[bad[:8], ids], ref[bad[:8], ids])
    err = np.abs(got[:, :-1] - ref[:, :-1]) - (atol + rtol * np.abs(ref[:, :-1]))
    assert np.all(err <= 0), "%s max excess %.3e at %s" % (what, err.max(), np.unravel_index(np.argmax(err), err.shape))
    e2 = np.abs(got[:, -1] - ref[:, -1]) - r2_rtol * np.abs(ref[:, -1])
    assert np.all(e2 <= 0), "%s R2 max excess %.3e in voxel %d" % (what, e2.max(), int(np.argmax(e2)))
