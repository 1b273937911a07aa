"""What the tests of measurement weights on 2-D protocols share (include/mfx_w2d.h): the synthetic voxels, their weights,
and the REFEREES of the GPU tests - for the fit the oracle's solver on sqrt(W)-scaled columns with the weighted row packing
of tests/_wfit_ref.py, for the profile and the posterior tests/_post_ref.py on the same scaled columns.  Nothing here
needs a GPU: the rotation is an argument (the GPU tests pass the library's own, T.rotate / T.rotate_cols, which the
kernels must see bit for bit; the seeds were checked on the CPU with the reference's).

Synthetic voxels: two crossing fascicles (|cos| <= 0.85), a Rician-noisy mixture (SNR 30) of two rotated atoms with
fractions in [0.3, 0.7]; then NBAD(M) = max(6, M // 8) random rows are multiplied by U(0.1, 0.5).  Weights: 'mask' is 0 on those rows
and 1 elsewhere; 'smooth' is 0.25 * 16^u (u the row's delta scaled to [0, 1]; 1 - u for odd voxels) and 1e-3 of it on
those rows."""
import numpy as np

import _wfit_ref as WR
from oracle import oracle as orc

GAP = 1e-8
CUT = 1e-8
# protocol, atoms, voxels, zmin, seed: 9 chunks with a 2-row tail and one block with a half-filled tile; a second block of
# one atom; 2 x 2 blocks
SHAPES = [("syn2", 72, 24, 0.1, 31), ("syn2", 129, 12, 0.1, 34), ("fix", 160, 6, 0.3, 33)]
IDS = ["%s-%d" % (s[0], s[1]) for s in SHAPES]


def nbad(M):
    return max(6, M // 8)


def random_dirs(rng, n, zmin):
    v = rng.standard_normal((8 * n + 8, 3))
    v /= np.sqrt(np.sum(v ** 2, axis=1, keepdims=True))
    return np.ascontiguousarray(v[np.abs(v[:, 2]) >= zmin][:n])


def make_voxels(rotate_cols, sch, N, V, zmin, seed):
    """(Y [V, M], peaks [V, 6], bad [V, nbad] the corrupted rows, W_mask [V, M], W_smooth [V, M]); rotate_cols(dirs [2, 3],
    ids [2]) -> [2, M] gives atom ids[k] rotated onto dirs[k]."""
    rng = np.random.default_rng(seed)
    M = sch.shape[0]
    nb = nbad(M)
    u = (sch[:, 5] - sch[:, 5].min()) / (sch[:, 5].max() - sch[:, 5].min())
    Y, peaks, bad = np.zeros((V, M)), np.zeros((V, 6)), np.zeros((V, nb), dtype=np.int64)
    Wm, Ws = np.ones((V, M)), np.zeros((V, M))
    for v in range(V):
        d = random_dirs(rng, 2, zmin)
        while abs(d[0] @ d[1]) > 0.85:
            d = random_dirs(rng, 2, zmin)
        ids = rng.integers(0, N, 2)
        f = rng.uniform(0.3, 0.7)
        cols = rotate_cols(d, ids)
        clean = f * cols[0] + (1.0 - f) * cols[1]
        s = 1.0 / 30.0
        y = np.sqrt((clean + s * rng.standard_normal(M)) ** 2 + (s * rng.standard_normal(M)) ** 2)
        bad[v] = rng.choice(M, nb, replace=False)
        y[bad[v]] *= rng.uniform(0.1, 0.5, nb)
        Y[v], peaks[v] = y, d.reshape(-1)
        Wm[v, bad[v]] = 0.0
        Ws[v] = 0.25 * 16.0 ** (u if v % 2 == 0 else 1.0 - u)
        Ws[v, bad[v]] *= 1e-3
    return Y, peaks, bad, Wm, Ws


def outlier_voxels(rotate_cols, M, N, V, seed):
    """The voxels of the end-to-end test: two crossing fascicles, fractions in [0.4, 0.6], Rician noise at SNR 100, and four
    rows per voxel raised by U(0.5, 1): (Y [V, M], peaks [V, 6], ids [V, 2] the planted atoms, planted [V, 4] the rows)."""
    rng = np.random.default_rng(seed)
    Y, peaks, ids = np.zeros((V, M)), np.zeros((V, 6)), np.zeros((V, 2), dtype=np.int64)
    planted = np.zeros((V, 4), dtype=np.int64)
    for v in range(V):
        d = random_dirs(rng, 2, 0.1)
        while abs(d[0] @ d[1]) > 0.85:
            d = random_dirs(rng, 2, 0.1)
        ids[v] = rng.integers(0, N, 2)
        f = rng.uniform(0.4, 0.6)
        cols = rotate_cols(d, ids[v])
        clean = f * cols[0] + (1.0 - f) * cols[1]
        Y[v] = np.sqrt((clean + rng.standard_normal(M) / 100.0) ** 2 + (rng.standard_normal(M) / 100.0) ** 2)
        planted[v] = rng.choice(M, 4, replace=False)
        Y[v, planted[v]] += rng.uniform(0.5, 1.0, 4)
        peaks[v] = d.reshape(-1)
    return Y, peaks, ids, planted


def mad_mask(res, k=4.0):
    """True where a residual lies within k robust standard deviations (1.4826 MAD) of its voxel's median"""
    dev = np.abs(res - np.median(res, axis=1, keepdims=True))
    return dev <= k * 1.4826 * np.median(dev, axis=1, keepdims=True)


def ref_row(D, y, w, csf, sig_csf, maxfasc, csf_on, deleted=False):
    """The fit's referee for one voxel: D [K, M, N] the rotated dictionaries; the oracle's solver on (s A, s y) and the
    weighted packing.  deleted=True solves on the rows with w > 0 only (the row-deleted form)."""
    K = len(D)
    row = np.zeros(WR.num_params(maxfasc, csf_on))
    if K + int(csf) == 0:
        return row
    N = D[0].shape[1] if K else 0
    w = np.asarray(w, dtype=np.float64)
    cols = [np.asarray(Dk) for Dk in D] + ([np.asarray(sig_csf, dtype=np.float64)[:, None]] if csf else [])
    A = np.ascontiguousarray(np.hstack(cols))
    s = np.sqrt(w)
    As, ys = np.ascontiguousarray(s[:, None] * A), np.ascontiguousarray(s * y)
    if deleted:
        keep = w > 0
        As, ys = np.ascontiguousarray(As[keep]), np.ascontiguousarray(ys[keep])
    wt, sub, tot, obj, _ = orc.solve_exhaustive_posweights(As, ys, np.array([N] * K + [1] * int(csf)))
    M0 = np.sum(wt)
    nu = wt / M0 if np.abs(M0) > 0 else wt
    row[0] = M0
    row[1:K + 1] = nu[:K]
    row[1 + maxfasc:1 + maxfasc + K] = sub[:K]
    if csf:
        row[1 + 2 * maxfasc] = nu[K]
    row[-2] = obj / np.sum(w)
    row[-1] = WR.weighted_r2(y, A[:, tot] @ wt, w)
    return row


def gap(D, y, w):
    """top-2 gap of a K = 2 voxel relative to |y'|^2, and the arg-min pair"""
    s = np.sqrt(np.asarray(w, dtype=np.float64))
    As, ys = np.hstack([s[:, None] * D[0], s[:, None] * D[1]]), s * y
    o = WR.pair_gap(As, ys, D[0].shape[1])
    return (o[1] - o[0]) / np.sum(ys * ys)


def pair_ref(D, y, w):
    """long-double F_W of every pair of a K = 2 voxel on the scaled columns (tests/_post_ref.py), the 1 - c^2 of the bar,
    the input condition (no pair near the cut)"""
    import _post_ref as R
    s = np.sqrt(np.asarray(w, dtype=np.float64))
    g = R.gram(s * y, s[:, None] * D[0], s[:, None] * D[1])
    F, c2bar, c2s, below = R.pair_values(g, False, CUT)
    return {"F": F, "c2bar": c2bar, "clear": R.clear_of_the_cut(c2s, CUT), "ysq": float(g["ysq"])}


def single_ref(D0, y, w):
    """long-double F_W(i) of a one-fascicle voxel as an [N x 1] matrix for _post_ref.posterior (c2bar = 1)"""
    import _post_ref as R
    s = np.sqrt(np.asarray(w, dtype=np.float64))
    Dl, yl = (s[:, None] * D0).astype(R.LD), (s * y).astype(R.LD)
    A, Yv = (Dl * Dl).sum(0), Dl.T @ yl
    ysq = yl @ yl
    return {"F": (ysq - np.maximum(Yv, 0) ** 2 / A)[:, None], "c2bar": np.ones((D0.shape[1], 1)), "ysq": float(ysq), "clear": True}
