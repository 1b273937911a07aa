"""Bootstrap of 2-D (AxCaliber-like) protocols on the device (include/mfx_boot2d.h, csrc/boot2d.hip).

The replicate fit shares a voxel's directions among its B signals; its referee is the plain fit of the same signals with
the directions repeated (engine.fit2d), bit for bit.  The bootstrap around it is compared with the loop written by hand
from tests/_boot_ref.py and T.fit, bit for bit, and with the CPU oracle at test_fit2d_gpu's bar (atoms equal, rtol 1e-5,
atol 1e-12)."""
import json
import os

import numpy as np
import pytest

import _boot_ref as R
import _twin2d_cases as t2
import test_fit2d_gpu as F2
from microstructure_fingerprinting_amd import _lib, engine
from microstructure_fingerprinting_amd import mf_utils as U

pytestmark = pytest.mark.gpu

Q = (0.025, 0.5, 0.975)
_cache = {}


def rot_npz():
    if "rot" not in _cache:
        _cache["rot"] = np.load(os.path.join(F2.G, "rot2d_cases.npz"))
    return _cache["rot"]


def tables(name, N, seed):
    key = ("T", name, N, seed)
    if key not in _cache:
        sch = rot_npz()[name + "_sch"]
        _cache[key] = U.RotateAtom2DTables(F2.atoms(sch, N, seed), sch, F2.Z, F2.DIFF)
    return _cache[key]


def rep_tile():
    return _lib.lib().mfx_boot2d_rep_tile()


def replicate_signals(T, rng, V, B, zmin):
    """V two-fascicle voxels of test_fit2d_gpu and B noise realisations of each: (Ystar [V, B, M], peaks [V, 6])."""
    Y, peaks = F2.two_fascicle_voxels(T, rng, V, zmin)
    Ys = np.abs(Y[:, None, :] + rng.standard_normal((V, B, T.M)) / 30.0)
    return np.ascontiguousarray(Ys), peaks


def replicates_dev(T, Ys, peaks, k):
    import torch
    out, st = engine.fit2d_replicates_dev(T, torch.from_numpy(np.ascontiguousarray(Ys)).cuda(),
                                          torch.from_numpy(np.ascontiguousarray(peaks[:, :3 * k])).cuda(), k)
    torch.cuda.synchronize()
    return out.cpu().numpy(), st.cpu().numpy()


# ---- 1. the replicate fit against the plain fit of the same rows
@pytest.mark.parametrize("name,N,V,k,zmin", [("syn2", 72, 6, 2, 0.1),      # one block, ragged tile, NP = 80; 8 chunks + 2 rows
                                            ("fix", 160, 3, 2, 0.3),      # 2 x 2 blocks, 1776 rows
                                            ("syn2", 72, 6, 1, 0.1),
                                            ("syn2", 300, 6, 1, 0.1)])    # beyond one pass of 256 threads
def test_replicates_equal_plain_fit(name, N, V, k, zmin):
    lib = _lib.lib()
    T = tables(name, N, 6)
    assert k != 2 or N <= lib.mfx_fit2d_max_atoms(T.handle(), 2)
    Rt = rep_tile()
    Bs = sorted({1, Rt - 1, Rt, Rt + 1, 37})
    rng = np.random.default_rng(7 + N)
    Ys, peaks = replicate_signals(T, rng, V, max(Bs), zmin)
    pk = peaks[:, :3 * k]
    np_ = engine.num_params(k, False, False)
    plain, st = engine.fit2d(T, Ys.reshape(-1, T.M), np.full(V * max(Bs), k), None, np.repeat(pk, max(Bs), axis=0), k, False)
    assert np.all(st == 0) and np.all(np.isfinite(plain))
    plain = plain.reshape(V, max(Bs), np_)
    assert np.all(np.any(plain[:, 1:] != plain[:, :1], axis=(1, 2)))          # the replicates of a voxel are not copies of one row
    for B in Bs:
        got, vst = replicates_dev(T, Ys[:, :B], peaks, k)
        assert got.shape == (V, B, np_) and np.all(vst == 0)
        assert np.array_equal(got, plain[:, :B]), "B = %d" % B
        try:
            lib.mfx_boot2d_debug_set_force_plain(1)
            got2, vst2 = replicates_dev(T, Ys[:, :B], peaks, k)
        finally:
            lib.mfx_boot2d_debug_set_force_plain(0)
        assert np.array_equal(got2, plain[:, :B]) and np.all(vst2 == 0), "plain path, B = %d" % B


# ---- 2., 3., 5. the bootstrap of a mixed batch against the loop written by hand
def hand_loop(T, Y, peaks, K, csf, sig_csf, B, kind, seed, vox=None):
    """(Ystar, replicate rows [V, B, np], the own fit) from _boot_ref.resample and T.fit."""
    F = peaks.shape[1] // 3
    csf_on = csf is not None
    fit = T.fit(Y, peaks, K, csf_mask=csf, sig_csf=sig_csf)
    pred = T.predict(fit, peaks, sig_csf)
    groups = np.unique(T._arrays['sch'][:, 3:6], axis=0, return_inverse=True)[1].reshape(-1)
    Ys, st = R.resample(Y, pred, fit.params, F, csf_on, False, B, {'wild': 0, 'residual': 1}[kind], seed, True, groups=groups, vox=vox)
    assert not st.any()
    reps = np.stack([T.fit(np.ascontiguousarray(Ys[:, b]), peaks, K, csf_mask=csf, sig_csf=sig_csf).params for b in range(B)], axis=1)
    return Ys, reps, fit


def mixed_batch():
    """test_fit2d_gpu.test_mixed_batch's 30 voxels: K = 0..2, with and without CSF."""
    if "mixed" not in _cache:
        T = tables("syn2", 32, 12)
        sch = rot_npz()["syn2_sch"]
        sig_csf = F2.csf_signal(sch)
        rng = np.random.default_rng(13)
        V = 30
        Y, peaks = F2.two_fascicle_voxels(T, rng, V, 0.1)
        K = np.arange(V) % 3
        csf = (np.arange(V) % 5) < 2
        Y[csf] = 0.8 * Y[csf] + 0.2 * sig_csf
        props = {'rad': np.linspace(0.5, 4.0, T.N), 'fin': np.cos(np.arange(T.N))}
        _cache["mixed"] = (T, Y, peaks, K, csf, sig_csf, props)
    return _cache["mixed"]


def mixed_result(kind):
    key = ("mixed_result", kind)
    if key not in _cache:
        T, Y, peaks, K, csf, sig_csf, props = mixed_batch()
        r = T.bootstrap(Y, peaks, K, csf_mask=csf, sig_csf=sig_csf, B=5, kind=kind, seed=11, q=Q, props=props, keep=True)
        _cache[key] = (r, hand_loop(T, Y, peaks, K, csf, sig_csf, 5, kind, 11))
    return _cache[key]


def three_fascicle_batch():
    if "k3" not in _cache:
        T = tables("syn2", 12, 21)
        rng = np.random.default_rng(22)
        V = 4
        Y, peaks = np.zeros((V, T.M)), np.zeros((V, 9))
        for v in range(V):
            while True:
                d = F2.random_dirs(rng, 3, 0.1)
                if all(abs(d[a] @ d[b]) <= 0.85 for a in range(3) for b in range(a)):
                    break
            cols = T.rotate_cols(d, rng.integers(0, T.N, 3))
            Y[v] = F2.rician(rng, 0.4 * cols[0] + 0.35 * cols[1] + 0.25 * cols[2])
            peaks[v] = d.reshape(-1)
        _cache["k3"] = (T, Y, peaks, np.full(V, 3))
    return _cache["k3"]


def k3_result(kind):
    key = ("k3_result", kind)
    if key not in _cache:
        T, Y, peaks, K = three_fascicle_batch()
        r = T.bootstrap(Y, peaks, K, B=5, kind=kind, seed=11, q=Q, props={'rad': np.linspace(0.5, 4.0, T.N)}, keep=True)
        _cache[key] = (r, hand_loop(T, Y, peaks, K, None, None, 5, kind, 11))
    return _cache[key]


@pytest.mark.parametrize("kind", ["wild", "residual"])
def test_bootstrap_replicates_equal_hand_loop(kind):
    T, Y, peaks, K, csf, sig_csf, props = mixed_batch()
    r, (_, reps, fit) = mixed_result(kind)
    assert r.replicates.shape == (30, 5, 8) and np.all(r.status == 0) and np.all(r.dir_status == 0)
    assert np.array_equal(r.replicates, reps)
    none = (K == 0) & ~csf
    assert none.any() and np.all(r.replicates[none] == 0)
    for k in range(3):
        for c in (False, True):
            assert ((K == k) & (csf == c)).any()
    assert np.any(r.replicates[:, 1:, 3:5] != r.replicates[:, :1, 3:5])          # the replicates are not copies of one row
    # the own fit may be passed in: the same bits
    r2 = T.bootstrap(Y, peaks, K, fit=fit, csf_mask=csf, sig_csf=sig_csf, B=5, kind=kind, seed=11, q=Q, props=props, keep=True)
    assert np.array_equal(r2.replicates, r.replicates) and np.array_equal(r2.stats, r.stats, equal_nan=True)
    r3, (_, reps3, _) = k3_result(kind)
    assert r3.replicates.shape == (4, 5, 9) and np.all(r3.status == 0)
    assert np.array_equal(r3.replicates, reps3)


@pytest.mark.parametrize("kind", ["wild", "residual"])
def test_statistics_equal_restatement(kind):
    T, Y, peaks, K, csf, sig_csf, props = mixed_batch()
    for (r, (_, _, fit)), F, c, pr in ((mixed_result(kind), 2, True, np.stack([props['rad'], props['fin']])),
                                       (k3_result(kind), 3, False, np.linspace(0.5, 4.0, 12)[None, :])):
        X, valid, agree = R.gather(r.replicates, fit.params, F, c, False, pr, pr.shape[1])
        ref = R.reduce(X, valid, Q)
        assert r.stats.shape == ref.shape and r.columns == engine.boot_columns(F, c, False, pr.shape[0])
        assert np.array_equal(r.stats, ref, equal_nan=True)
        assert np.array_equal(r.agreement, agree / 5.0)
        assert np.array_equal(r.mean('rad'), ref[:, [r.columns.index(('prop', k, 0)) for k in range(F)], 1], equal_nan=True)
        assert np.array_equal(r.quantile('M0', 0.5), ref[:, 0, 6]) and np.array_equal(r.n_valid('frac'), np.full((len(ref), F), 5))


def test_oracle_on_replicates():
    T, Y, peaks, K, csf, sig_csf, props = mixed_batch()
    r, (Ys, _, _) = mixed_result("wild")
    seen = 0
    for k in range(3):
        for c in (False, True):
            if k == 0 and not c:
                continue
            v = int(np.flatnonzero((K == k) & (csf == c))[0])
            ref = np.array([F2.oracle_row(T, np.ascontiguousarray(Ys[v, b]), peaks[v, :3 * k].reshape(k, 3), c, sig_csf, 2, True)
                            for b in range(3)])
            F2.assert_rows(r.replicates[v, :3], ref, 2, "class K=%d csf=%d" % (k, c))
            seen += 1
    T3, Y3, peaks3, _ = three_fascicle_batch()
    r3, (Ys3, _, _) = k3_result("wild")
    ref = np.array([F2.oracle_row(T3, np.ascontiguousarray(Ys3[0, b]), peaks3[0].reshape(3, 3), False, None, 3, False) for b in range(3)])
    F2.assert_rows(r3.replicates[0, :3], ref, 3, "class K=3")
    assert seen == 5


# ---- 4. ties
def test_exact_ties_take_the_first_pair():
    sch = rot_npz()["syn2_sch"]
    half = F2.atoms(sch, 20, 8)
    T = U.RotateAtom2DTables(np.hstack([half, half]), sch, F2.Z, F2.DIFF)      # atoms i and i + 20 are bit-identical columns
    rng = np.random.default_rng(9)
    V = 8
    Y, peaks = F2.two_fascicle_voxels(T, rng, V, 0.1)
    r = T.bootstrap(Y, peaks, np.full(V, 2), B=rep_tile() + 1, seed=3, keep=True)
    assert np.all(r.status == 0) and np.all(np.isfinite(r.replicates))
    assert np.all(r.replicates[:, :, 3:5] < 20)                               # the lowest (i1, i2) of every tied group
    _, reps, _ = hand_loop(T, Y, peaks, np.full(V, 2), None, None, rep_tile() + 1, 'wild', 3)
    assert np.array_equal(r.replicates, reps)


@pytest.mark.parametrize("case", [("syn2", 32, 2, "margin"), ("syn2", 1, 64, "window")], ids=t2.case_id)
def test_near_twin_atoms(case):
    T = U.RotateAtom2DTables(t2.dictionary(case)[0], t2.scheme(case[0]), F2.Z, F2.DIFF)
    Y, peaks, _ = t2.voxels(case, t2.Rotation(T, "boot2d"), nv=6)
    K = np.full(Y.shape[0], 2)
    r = T.bootstrap(Y, peaks, K, B=5, seed=5, keep=True)
    _, reps, _ = hand_loop(T, np.array(Y), np.array(peaks), K, None, None, 5, 'wild', 5)
    assert np.all(r.status == 0) and np.array_equal(r.replicates, reps)


# ---- 6. invariance: subsets and chunks
def test_subsets_and_chunks_give_the_same_bits():
    T, Y, peaks, K, csf, sig_csf, props = mixed_batch()
    r, _ = mixed_result("residual")
    sub = np.array([3, 7, 8, 20, 29])
    rs = T.bootstrap(Y, peaks, K, csf_mask=csf, sig_csf=sig_csf, B=5, kind='residual', seed=11, q=Q, props=props, keep=True, voxels=sub)
    assert list(rs.voxels) == list(sub)
    assert np.array_equal(rs.replicates, r.replicates[sub]) and np.array_equal(rs.stats, r.stats[sub], equal_nan=True)
    assert np.array_equal(rs.agreement, r.agreement[sub]) and np.array_equal(rs.status, r.status[sub])
    groups = np.unique(T._arrays['sch'][:, 3:6], axis=0, return_inverse=True)[1].reshape(-1)
    pr = np.stack([props['rad'], props['fin']])
    one = engine.fit2d_bootstrap(T, Y, K, csf, peaks, 2, True, sig_csf, B=5, kind='residual', seed=11, q=Q, props=pr, groups=groups,
                                 keep=True, max_bytes=1)           # one voxel per chunk, of the bootstrap and of the replicate fit
    assert np.array_equal(one['replicates'], r.replicates) and np.array_equal(one['stats'], r.stats, equal_nan=True)
    assert np.array_equal(one['agree'], np.rint(r.agreement * 5).astype(np.int32)) and np.array_equal(one['status'], r.status)
    # the replicate fit alone in several chunks of voxels: the device entry point of one class
    import torch
    two = np.flatnonzero((K == 2) & ~csf)
    d = engine.fit2d_bootstrap_dev(T, torch.from_numpy(np.ascontiguousarray(Y[two])).cuda(), torch.from_numpy(np.ascontiguousarray(peaks[two])).cuda(),
                                   2, B=5, kind='residual', seed=11, q=Q, d_props=torch.from_numpy(pr).cuda(),
                                   d_groups=torch.from_numpy(groups.astype(np.int32)).cuda(), d_vox=torch.from_numpy(two).cuda(), keep=True,
                                   max_bytes=3 * 5 * T.M * 8)
    torch.cuda.synchronize()
    assert np.array_equal(d['replicates'].cpu().numpy(), r.replicates[two][:, :, [0, 1, 2, 3, 4, 6, 7]])
    assert np.all(d['status'].cpu().numpy() == 0) and np.all(d['dir_status'].cpu().numpy() == 0)


# ---- 7. failures
def test_failing_directions_and_unusable_rows():
    rot = rot_npz()
    errs = {e["why"]: e for e in json.loads(str(rot["errors_json"]))}
    e_plane = errs["in-plane new fascicle: 4 pairs"]
    T = U.RotateAtom2DTables(rot["fix_sig"], rot["fix_sch"], F2.Z, F2.DIFF)
    rng = np.random.default_rng(14)
    V, B = 8, 4
    Y, peaks = F2.two_fascicle_voxels(T, rng, V, 0.3)
    K = np.full(V, 2)
    K[1] = 1
    good = T.bootstrap(Y, peaks, K, B=B, seed=2, keep=True, on_error="nan")
    assert np.all(good.status == 0) and np.all(good.dir_status == 0) and np.all(np.isfinite(good.replicates))
    bad, Yb = peaks.copy(), Y.copy()
    bad[5, 3:6] = e_plane["newdir"]            # voxel 5, fascicle 1: a direction in the protocol's plane
    Yb[3, 10] = np.nan                          # voxel 3: a measurement that is not finite
    Yb[1, 0] = np.inf                           # voxel 1 (one fascicle) likewise
    r = T.bootstrap(Yb, bad, K, B=B, seed=2, keep=True, on_error="nan")
    assert tuple(r.dir_status[5]) == (U.ROT2D_NEW_PAIRS, 0, 4, 0, 1) and not np.any(np.delete(r.dir_status, 5, axis=0))
    assert list(r.status) == [0, 2, 0, 2, 0, 2, 0, 0]
    for v in (1, 3, 5):
        assert np.all(r.stats[v, :, 0] == 0) and np.all(np.isnan(r.stats[v, :, 1:])) and np.all(np.isnan(r.replicates[v]))
        assert np.all(r.agreement[v] == 0)
    keep = np.array([0, 2, 4, 6, 7])
    assert np.array_equal(r.replicates[keep], good.replicates[keep]) and np.array_equal(r.stats[keep], good.stats[keep], equal_nan=True)
    with pytest.raises(Exception) as ei:
        T.bootstrap(Y, bad, K, B=B, seed=2)
    assert (type(ei.value).__name__, str(ei.value)) == (e_plane["type"], e_plane["msg"])
    # the same through the plain path
    try:
        _lib.lib().mfx_boot2d_debug_set_force_plain(1)
        rp = T.bootstrap(Yb, bad, K, B=B, seed=2, keep=True, on_error="nan")
    finally:
        _lib.lib().mfx_boot2d_debug_set_force_plain(0)
    assert np.array_equal(rp.dir_status, r.dir_status) and np.array_equal(rp.status, r.status)
    assert np.array_equal(rp.replicates, r.replicates, equal_nan=True) and np.array_equal(rp.stats, r.stats, equal_nan=True)
