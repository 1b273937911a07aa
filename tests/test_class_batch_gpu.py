"""The mixed-batch host entry points keep every voxel's rows with its voxel (csrc/class_batch.h: binning by class,
gather, scatter): mfx_fit2d_batch, mfx_wfit2d_batch, mfx_wfit_batch, mfx_rfit_batch and mfx_rfit2d_batch fit a batch, then
the same batch with its voxels in a fixed shuffled order; every output array of the second call must be the first call's
rows in that order, bit for bit.  Nothing here knows how the library bins: a row that lands on another voxel shows.

Models: N = 20 atoms on M = 22 measurements (neither a multiple of 16 or 8: padded columns and rows are in play) - for the
plans the recipe of test_robust_gpu.model (2 b0 + 2 shells of 10 directions), for the 2-D protocols the first
(Delta, delta) pair of syn2 (2 b0 + 5 gradient strengths x 4 directions) with the atoms of test_fit2d_gpu.atoms.  Voxels: 13
with K = 2, 0, 1, 2, 1, 0, 2, 1, 2, 0, 1, 2, 1 (maxfasc = 2), CSF flagged on one voxel of each K; the recipes of
test_robust_gpu.make_voxels and _robust2d_ref.make_voxels; weights as in their mixed batches.  Robust: Huber, n_iter = 2."""
import os

import numpy as np
import pytest

import _robust2d_ref as R2
from test_fit2d_gpu import DIFF, Z, atoms, csf_signal
from microstructure_fingerprinting_amd import engine, synth
from microstructure_fingerprinting_amd import mf_utils as U
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
N, M, V = 20, 22, 13
K = np.array([2, 0, 1, 2, 1, 0, 2, 1, 2, 0, 1, 2, 1])
CSF = np.zeros(V, dtype=bool)
CSF[[1, 4, 6]] = True                      # K = 0, 1, 2
PERM = np.random.default_rng(7).permutation(V)
_cache = {}


def weights(Y, seed):
    rng = np.random.default_rng(seed)
    W = rng.uniform(0.5, 2.0, Y.shape)
    for v in range(Y.shape[0]):
        W[v, rng.choice(Y.shape[1], 1 + v % 2, replace=False)] = 0.0
    return W


def plan_case():
    """the plan's model and its voxels, made once"""
    if "plan" not in _cache:
        rng = np.random.default_rng(1)
        sch = synth.make_scheme(rng, 2, [1000, 2000], [10, 10])
        dic = synth.make_dictionary(rng, sch, N)
        assert dic.shape == (M, N)
        T = orc.init_tables(dic, sch, Z)
        b = (orc.GAMMA_H * sch[:, 3] * sch[:, 5]) ** 2 * (sch[:, 4] - sch[:, 5] / 3)
        sig_csf = np.exp(-sch[:, 6] / 2.0) * np.exp(-b * 3.0e-9)
        rng = np.random.default_rng(61)
        peaks, Y = np.zeros((V, 6)), np.zeros((V, M))
        for v in range(V):
            d = synth.unit_vectors(rng, 2)
            ids = rng.integers(0, N, 2)
            f = rng.uniform(0.3, 0.7)
            y = 500.0 * (f * orc.interp(sch, d[0], T)[:, ids[0]] + (1.0 - f) * orc.interp(sch, d[1], T)[:, ids[1]])
            y += rng.normal(0, 500.0 / 30.0, M)
            bad = rng.choice(M, 4, replace=False)
            y[bad] *= rng.uniform(0.1, 0.5, 4)
            peaks[v], Y[v] = d.reshape(-1), y
        Y[CSF] = 0.8 * Y[CSF] + 100.0 * sig_csf
        plan = U.init_PGSE_multishell_interp(dic, sch, Z).plan_for(sch)
        _cache["plan"] = dict(h=plan, sig_csf=sig_csf, peaks=peaks, Y=Y, W=weights(Y, 62))
    return _cache["plan"]


def tables_case():
    """the 2-D protocol's tables and their voxels, made once"""
    if "tables" not in _cache:
        sch = np.load(os.path.join(G, "rot2d_cases.npz"))["syn2_sch"][:M]
        assert sch.shape[0] == M and np.unique(sch[:, 4:6], axis=0).shape[0] == 1
        T = U.RotateAtom2DTables(atoms(sch, N, 11), sch, Z, DIFF)
        sig_csf = csf_signal(sch)
        peaks, Y = R2.make_voxels(T, V, 61, 0.1)
        Y[CSF] = 0.8 * Y[CSF] + 100.0 * sig_csf
        _cache["tables"] = dict(h=T, sig_csf=sig_csf, peaks=peaks, Y=Y, W=weights(Y, 62))
    return _cache["tables"]


def outputs(entry, c, ix):
    """name -> array of every output of one entry point on the voxels ix of case c; per-voxel arrays first, then whole-batch ones"""
    Y, W, pk, k, cf, h, sc = c["Y"][ix], c["W"][ix], c["peaks"][ix], K[ix], CSF[ix], c["h"], c["sig_csf"]
    if entry == "mfx_fit2d_batch":
        p, st = engine.fit2d(h, Y, k, cf, pk, 2, True, sc)
        return dict(params=p, status=st), {}
    if entry == "mfx_wfit2d_batch":
        p, st, wst = engine.fit2d_weighted(h, Y, W, k, cf, pk, 2, True, sc)
        return dict(params=p, status=st, wstatus=wst), {}
    if entry == "mfx_wfit_batch":
        p, st = engine.fit_weighted(h, Y, W, k, cf, pk, 2, True, sc)
        return dict(params=p, status=st), {}
    fit = engine.fit_robust if entry == "mfx_rfit_batch" else engine.fit2d_robust
    p, Wout, info = fit(h, Y, k, cf, pk, 2, True, sc, W0=W, loss="huber", c=4.45, n_iter=2)
    per_voxel = dict(params=p, weights=Wout, scale=info["scale"], state=info["state"], status=info["status"])
    if "dir_status" in info:
        per_voxel["dir_status"] = info["dir_status"]
    return per_voxel, dict(n_changed=np.asarray(info["n_changed"]), n_iter_used=np.asarray(info["n_iter_used"]))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("entry", ["mfx_fit2d_batch", "mfx_wfit2d_batch", "mfx_wfit_batch", "mfx_rfit_batch", "mfx_rfit2d_batch"])
def test_shuffled_batch_gives_shuffled_rows(entry):
    c = tables_case() if "2d" in entry else plan_case()
    for k in range(3):
        assert np.count_nonzero((K == k) & CSF) == 1 and np.count_nonzero((K == k) & ~CSF) > 1
    assert not np.array_equal(PERM, np.arange(V))
    rows, whole = outputs(entry, c, np.arange(V))
    rows_p, whole_p = outputs(entry, c, PERM)
    # the batch is a real one: every class fitted something, and no two voxels share a parameter row
    assert np.all(np.isfinite(rows["params"])) and np.all(rows["status"] == 0)
    fitted = (K > 0) | CSF
    assert np.all(rows["params"][fitted, 0] > 0) and np.all(rows["params"][~fitted] == 0)
    assert np.unique(rows["params"][fitted], axis=0).shape[0] == np.count_nonzero(fitted)
    for name in rows:
        differ = [int(v) for v in range(V) if not same_bits(rows_p[name][v], rows[name][PERM[v]])]
        print("%s %s: %d of %d shuffled rows differ" % (entry, name, len(differ), V))
        assert same_bits(rows_p[name], rows[name][PERM]), "%s %s: rows %s" % (entry, name, differ)
    for name in whole:
        print("%s %s: %s, shuffled %s" % (entry, name, whole[name], whole_p[name]))
        assert same_bits(whole_p[name], whole[name]), "%s %s" % (entry, name)
