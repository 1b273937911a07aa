"""Measurement weights for the tests of the weighted bootstrap of 2-D protocols (include/mfx_wboot2d.h).  Nothing here needs
a GPU.  Three kinds: 'smooth' per-voxel weights in [0.25, 4]; 'mask' a per-voxel 0/1 mask that drops about 15 % of the rows,
among them a run of rows across the seam between the Gram kernel's first two chunks of MC rows; 'shared' one [M] vector
for all voxels.  Every voxel keeps more rows of positive weight than a fit has active compartments (checked here)."""
import numpy as np

MC = 8            # protocol rows per chunk of the cross-Gram's loop (F2_MC of csrc/fit2d_shared.h)
KINDS = ("smooth", "mask", "shared")


def smooth(rng, V, M):
    """[V, M] in [0.25, 4]: 0.25 * 16^u, u a slow wave over the rows with a phase per voxel."""
    m = np.arange(M)[None, :] / float(M)
    u = 0.5 * (1.0 + np.sin(2.0 * np.pi * (m + rng.uniform(0.0, 1.0, (V, 1)))))
    W = 0.25 * 16.0 ** u
    assert W.min() >= 0.25 and W.max() <= 4.0
    return np.ascontiguousarray(W)


def mask(rng, V, M, n_act=3):
    """[V, M] of 0 / 1: about 15 % of the rows dropped per voxel, rows MC - 2 .. MC + 1 (across a chunk seam) among them."""
    W = np.ones((V, M))
    for v in range(V):
        W[v, rng.choice(M, int(round(0.15 * M)), replace=False)] = 0.0
        W[v, MC - 2:MC + 2] = 0.0
    assert np.all(np.count_nonzero(W > 0, axis=1) > n_act)
    assert 0.1 < 1.0 - W.mean() < 0.3
    return W


def shared(rng, M):
    """One [M] vector in [0.25, 4] for all voxels, two rows dropped."""
    W = smooth(rng, 1, M)[0]
    W[[3, M - 2]] = 0.0
    return np.ascontiguousarray(W)


def weights(kind, V, M, seed, n_act=3):
    rng = np.random.default_rng(seed)
    if kind == "smooth":
        return smooth(rng, V, M)
    if kind == "mask":
        return mask(rng, V, M, n_act)
    if kind == "shared":
        return shared(rng, M)
    raise ValueError(kind)


def rows_of(W, V):
    """[V, M] view of weights of either shape."""
    return np.broadcast_to(W, (V, W.shape[-1]))
