"""Bootstrap of 2-D (AxCaliber-like) protocols conditional on measurement weights, on the device (include/mfx_wboot2d.h,
csrc/wboot2d.hip).

The weighted replicate fit shares a voxel's weights and directions among its B signals; its referee is the weighted fit of
the same signals with weights and directions repeated (engine.fit2d_weighted), bit for bit, on the shared path and on the
plain one.  The bootstrap around it is compared with the loop written by hand from tests/_wboot_ref.py, tests/_boot_ref.py
and T.fit(weights=), bit for bit, and with the CPU oracle on sqrt(W)-scaled columns (tests/_w2d_ref.py) at
test_fit2d_gpu's bar (atoms equal, rtol 1e-5, atol 1e-12).  Shapes are test_boot2d_gpu's seam shapes."""
import json

import numpy as np
import pytest

import _boot_ref as R
import _w2d_ref as W2
import _wboot2d_cases as C
import _wboot_ref as WB
import test_boot2d_gpu as B2
import test_fit2d_gpu as F2
from microstructure_fingerprinting_amd import _lib, engine
from microstructure_fingerprinting_amd import mf_utils as U

pytestmark = pytest.mark.gpu

Q = (0.025, 0.5, 0.975)
KIND = {'wild': 0, 'residual': 1}
_cache = {}


def t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def rep_tile():
    return _lib.lib().mfx_wboot2d_rep_tile()


class force_plain:
    def __enter__(self):
        _lib.lib().mfx_wboot2d_debug_set_force_plain(1)

    def __exit__(self, *exc):
        _lib.lib().mfx_wboot2d_debug_set_force_plain(0)


def wreplicates_dev(T, Ys, W, peaks, k):
    import torch
    out, st, wst = engine.fit2d_weighted_replicates_dev(T, t(Ys), t(W), t(peaks[:, :3 * k]), k)
    torch.cuda.synchronize()
    return out.cpu().numpy(), st.cpu().numpy(), wst.cpu().numpy()


def weighted_rows(T, Ys, W, peaks, k):
    """The referee: engine.fit2d_weighted on the V B rows, weights and directions repeated -> [V, B, np]."""
    V, B, M = Ys.shape
    Wr = W if W.ndim == 1 else np.repeat(W, B, axis=0)
    rows, st, wst = engine.fit2d_weighted(T, Ys.reshape(-1, M), Wr, np.full(V * B, k), None, np.repeat(peaks[:, :3 * k], B, axis=0), k, False)
    assert not st.any() and not wst.any() and np.all(np.isfinite(rows))
    return rows.reshape(V, B, -1)


def groups_of(T):
    return np.unique(T._arrays['sch'][:, 3:6], axis=0, return_inverse=True)[1].reshape(-1)


# ---- 1. the weighted replicate fit against the weighted fit of the same rows
@pytest.mark.parametrize("wkind", C.KINDS)
@pytest.mark.parametrize("name,N,V,k,zmin", [("syn2", 72, 6, 2, 0.1),      # one block, ragged tile, NP = 80; chunk remainder rows
                                            ("fix", 160, 3, 2, 0.3),      # 2 x 2 blocks, 1776 rows
                                            ("syn2", 72, 6, 1, 0.1),
                                            ("syn2", 300, 6, 1, 0.1)])    # beyond one pass of 256 threads
def test_replicates_equal_weighted_fit(name, N, V, k, zmin, wkind):
    lib = _lib.lib()
    T = B2.tables(name, N, 6)
    assert k != 2 or N <= lib.mfx_wboot2d_max_atoms(T.handle())
    Rt = rep_tile()
    Bs = sorted({1, Rt - 1, Rt, Rt + 1, 37})
    rng = np.random.default_rng(7 + N)
    Ys, peaks = B2.replicate_signals(T, rng, V, max(Bs), zmin)
    W = C.weights(wkind, V, T.M, 100 + N + k, n_act=k)
    assert W.shape == ((T.M,) if wkind == "shared" else (V, T.M))
    ref = weighted_rows(T, Ys, W, peaks, k)
    assert np.all(np.any(ref[:, 1:] != ref[:, :1], axis=(1, 2)))              # the replicates of a voxel are not copies of one row
    for B in Bs:
        got, vst, wst = wreplicates_dev(T, Ys[:, :B], W, peaks, k)
        assert got.shape == ref[:, :B].shape and not vst.any() and not wst.any()
        assert np.array_equal(got, ref[:, :B]), "B = %d" % B
        with force_plain():
            got2, vst2, wst2 = wreplicates_dev(T, Ys[:, :B], W, peaks, k)
        assert np.array_equal(got2, ref[:, :B]) and not vst2.any() and not wst2.any(), "plain path, B = %d" % B


# ---- 2. unit weights
@pytest.mark.parametrize("k", [1, 2])
def test_unit_weights_give_the_unweighted_replicate_rows(k):
    T = B2.tables("syn2", 72, 6)
    V, B = 6, rep_tile() + 1
    Ys, peaks = B2.replicate_signals(T, np.random.default_rng(41), V, B, 0.1)
    plain, st = B2.replicates_dev(T, Ys, peaks, k)
    assert not st.any()
    for W in (np.ones((V, T.M)), np.ones(T.M)):
        got, vst, wst = wreplicates_dev(T, Ys, W, peaks, k)
        assert not vst.any() and not wst.any()
        assert np.array_equal(got, plain)


def test_unit_weights_give_the_unweighted_bootstrap():
    T, Y, peaks, K, csf, sig_csf, props = B2.mixed_batch()
    r, _ = B2.mixed_result("wild")
    for ones in (np.ones((30, T.M)), np.ones(T.M)):
        w = T.bootstrap(Y, peaks, K, csf_mask=csf, sig_csf=sig_csf, B=5, kind='wild', seed=11, q=Q, props=props, keep=True,
                        weights=ones, fixed_weights=True)
        assert np.array_equal(w.weights, ones) and np.all(w.status == 0) and np.all(w.dir_status == 0)
        fused = ~csf                                                          # K = 0, 1, 2 without a CSF column
        assert np.array_equal(w.replicates[fused], r.replicates[fused])
        # CSF classes go through the explicit solver: every column but R2 is equal, R2 agrees to rounding (the identity of
        # include/mfx_w2d.h: the weighted moments are summed by another routine; 1e-12 is test_w2d_gpu's bar for it)
        assert np.array_equal(w.replicates[..., :-1], r.replicates[..., :-1])
        assert np.allclose(w.replicates[..., -1], r.replicates[..., -1], rtol=1e-12, atol=0.0)
        assert np.array_equal(w.stats, r.stats, equal_nan=True) and np.array_equal(w.agreement, r.agreement)
    T3, Y3, peaks3, K3 = B2.three_fascicle_batch()
    r3, _ = B2.k3_result("wild")
    w3 = T3.bootstrap(Y3, peaks3, K3, B=5, kind='wild', seed=11, q=Q, props={'rad': np.linspace(0.5, 4.0, T3.N)}, keep=True,
                      weights=np.ones(T3.M), fixed_weights=True)
    assert np.array_equal(w3.replicates[..., :-1], r3.replicates[..., :-1])
    assert np.allclose(w3.replicates[..., -1], r3.replicates[..., -1], rtol=1e-12, atol=0.0)
    assert np.array_equal(w3.stats, r3.stats, equal_nan=True)


# ---- 3. the bootstrap of a mixed batch against the loop written by hand
def whand_loop(T, Y, W, peaks, K, csf, sig_csf, B, kind, seed, fit=None, vox=None):
    """(Ystar, replicate rows [V, B, np], the own weighted fit) from _wboot_ref.resample and T.fit(weights=)."""
    F = peaks.shape[1] // 3
    if fit is None:
        fit = T.fit(Y, peaks, K, csf_mask=csf, sig_csf=sig_csf, weights=W)
    pred = T.predict(fit, peaks, sig_csf)
    Ys, st = WB.resample(Y, pred, W, fit.params, F, csf is not None, B, KIND[kind], seed, True, groups=groups_of(T), vox=vox)
    assert not st.any()
    reps = np.stack([T.fit(np.ascontiguousarray(Ys[:, b]), peaks, K, csf_mask=csf, sig_csf=sig_csf, weights=W).params for b in range(B)],
                    axis=1)
    return Ys, reps, fit


def mixed_weights():
    """Per-voxel weights of the mixed batch: smooth for even voxels, a 0/1 mask for odd ones."""
    if "W" not in _cache:
        T = B2.mixed_batch()[0]
        W = C.weights("smooth", 30, T.M, 5)
        W[1::2] = C.weights("mask", 30, T.M, 6)[1::2]
        _cache["W"] = W
    return _cache["W"]


def wmixed_result(kind):
    key = ("mixed", kind)
    if key not in _cache:
        T, Y, peaks, K, csf, sig_csf, props = B2.mixed_batch()
        W = mixed_weights()
        Ys, reps, fit = whand_loop(T, Y, W, peaks, K, csf, sig_csf, 5, kind, 11)
        r = T.bootstrap(Y, peaks, K, fit=fit, csf_mask=csf, sig_csf=sig_csf, B=5, kind=kind, seed=11, q=Q, props=props, keep=True,
                        fixed_weights=True)
        _cache[key] = (r, (Ys, reps, fit))
    return _cache[key]


def wk3_result(kind):
    key = ("k3", kind)
    if key not in _cache:
        T, Y, peaks, K = B2.three_fascicle_batch()
        W = C.weights("shared", 4, T.M, 8)
        Ys, reps, fit = whand_loop(T, Y, W, peaks, K, None, None, 5, kind, 11)
        r = T.bootstrap(Y, peaks, K, fit=fit, B=5, kind=kind, seed=11, q=Q, props={'rad': np.linspace(0.5, 4.0, T.N)}, keep=True,
                        fixed_weights=True)
        _cache[key] = (r, (Ys, reps, fit), W)
    return _cache[key]


@pytest.mark.parametrize("kind", ["wild", "residual"])
def test_bootstrap_equals_hand_loop(kind):
    T, Y, peaks, K, csf, sig_csf, props = B2.mixed_batch()
    W = mixed_weights()
    r, (_, reps, fit) = wmixed_result(kind)
    assert r.replicates.shape == (30, 5, 8) and np.all(r.status == 0) and np.all(r.dir_status == 0)
    assert np.array_equal(r.weights, W) and fit.weights is not None
    assert np.array_equal(r.replicates, reps)
    none = (K == 0) & ~csf
    assert none.any() and np.all(r.replicates[none] == 0)
    assert np.any(r.replicates[:, 1:, 3:5] != r.replicates[:, :1, 3:5])          # the replicates are not copies of one row
    pr = np.stack([props['rad'], props['fin']])
    X, valid, agree = R.gather(r.replicates, fit.params, 2, True, False, pr, T.N)
    ref = R.reduce(X, valid, Q)
    assert r.columns == engine.boot_columns(2, True, False, 2)
    assert np.array_equal(r.stats, ref, equal_nan=True) and np.array_equal(r.agreement, agree / 5.0)
    # the own weighted fit made here (weights= without a fit): the same bits
    r2 = T.bootstrap(Y, peaks, K, csf_mask=csf, sig_csf=sig_csf, B=5, kind=kind, seed=11, q=Q, props=props, keep=True, weights=W,
                     fixed_weights=True)
    assert np.array_equal(r2.replicates, r.replicates) and np.array_equal(r2.stats, r.stats, equal_nan=True)
    # a small three-fascicle batch on one shared weight vector
    T3 = B2.three_fascicle_batch()[0]
    r3, (_, reps3, fit3), W3 = wk3_result(kind)
    assert r3.replicates.shape == (4, 5, 9) and np.all(r3.status == 0) and np.array_equal(r3.weights, W3)
    assert np.array_equal(r3.replicates, reps3)
    pr3 = np.linspace(0.5, 4.0, T3.N)[None, :]
    X3, valid3, agree3 = R.gather(r3.replicates, fit3.params, 3, False, False, pr3, T3.N)
    assert np.array_equal(r3.stats, R.reduce(X3, valid3, Q), equal_nan=True) and np.array_equal(r3.agreement, agree3 / 5.0)


# ---- 4. the CPU oracle on sqrt(W)-scaled columns
def test_oracle_on_replicates():
    T, Y, peaks, K, csf, sig_csf, props = B2.mixed_batch()
    W = mixed_weights()
    r, (Ys, _, _) = wmixed_result("wild")
    seen = 0
    for k in range(3):
        for c in (False, True):
            if k == 0 and not c:
                continue
            for v in np.flatnonzero((K == k) & (csf == c))[:2]:              # a smooth and a masked voxel of the class
                D = T.rotate(peaks[v, :3 * k].reshape(k, 3)) if k else []
                ref = np.array([W2.ref_row(D, Ys[v, b], W[v], c, sig_csf, 2, True) for b in range(2)])
                F2.assert_rows(r.replicates[v, :2], ref, 2, "class K=%d csf=%d voxel %d" % (k, c, v))
                seen += 1
    assert seen == 10
    T3, Y3, peaks3, _ = B2.three_fascicle_batch()
    r3, (Ys3, _, _), W3 = wk3_result("wild")
    D3 = T3.rotate(peaks3[0].reshape(3, 3))
    ref = np.array([W2.ref_row(D3, Ys3[0, b], W3, False, None, 3, False) for b in range(2)])
    F2.assert_rows(r3.replicates[0, :2], ref, 3, "class K=3")


# ---- 5. a robust fit end to end
def test_robust_fit_end_to_end():
    import torch
    T = B2.tables("syn2", 32, 12)
    V, B = 6, 5
    Y, peaks, _, planted = W2.outlier_voxels(T.rotate_cols, T.M, T.N, V, 17)
    K = np.full(V, 2)
    r = T.fit(Y, peaks, K, robust={'n_iter': 1})
    assert r.robust_info is not None and np.any(r.weights == 0) and r.weights.shape == (V, T.M)
    with pytest.raises(NotImplementedError, match="bootstrap of a weighted or robust fit is not served"):
        T.bootstrap(Y, peaks, K, fit=r, B=B)
    bs = T.bootstrap(Y, peaks, K, fit=r, B=B, seed=4, keep=True, fixed_weights=True)
    assert np.array_equal(bs.weights, r.weights) and np.all(bs.status == 0)
    _, reps, _ = whand_loop(T, Y, r.weights, peaks, K, None, None, B, 'wild', 4, fit=r)
    assert np.array_equal(bs.replicates, reps)
    # the rejected rows are left as measured in every replicate: nothing re-runs the rejection
    pred = T.predict(r, peaks)
    Ys, _, st = engine.wboot_resample_dev(t(Y), t(pred), t(r.weights), t(r.params), 2, B=B, seed=4)
    torch.cuda.synchronize()
    Ys = Ys.cpu().numpy()
    zero = r.weights == 0
    assert not st.cpu().numpy().any()
    for b in range(B):
        assert np.array_equal(Ys[:, b][zero], Y[zero])
    assert np.any(Ys[:, 0][~zero] != Y[~zero])


# ---- 6. invariance: subsets, chunks, the voxel's position
def test_subsets_chunks_and_permutations_give_the_same_bits():
    T, Y, peaks, K, csf, sig_csf, props = B2.mixed_batch()
    W = mixed_weights()
    r, (_, _, fit) = wmixed_result("residual")
    kw = dict(csf_mask=csf, sig_csf=sig_csf, B=5, kind='residual', seed=11, q=Q, props=props, keep=True, fixed_weights=True)
    sub = np.array([3, 7, 8, 20, 29])
    rs = T.bootstrap(Y, peaks, K, fit=fit, voxels=sub, **kw)
    assert list(rs.voxels) == list(sub) and np.array_equal(rs.weights, W[sub])
    assert np.array_equal(rs.replicates, r.replicates[sub]) and np.array_equal(rs.stats, r.stats[sub], equal_nan=True)
    assert np.array_equal(rs.agreement, r.agreement[sub]) and np.array_equal(rs.status, r.status[sub])
    groups = groups_of(T)
    pr = np.stack([props['rad'], props['fin']])
    ekw = dict(B=5, kind='residual', seed=11, q=Q, props=pr, groups=groups, keep=True)
    one = engine.fit2d_weighted_bootstrap(T, Y, W, K, csf, peaks, 2, True, sig_csf, max_bytes=1, **ekw)   # one voxel per chunk
    assert np.array_equal(one['replicates'], r.replicates) and np.array_equal(one['stats'], r.stats, equal_nan=True)
    assert np.array_equal(one['agree'], np.rint(r.agreement * 5).astype(np.int32)) and np.array_equal(one['status'], r.status)
    perm = np.random.default_rng(3).permutation(30)
    pm = engine.fit2d_weighted_bootstrap(T, Y[perm], W[perm], K[perm], csf[perm], peaks[perm], 2, True, sig_csf, vox=perm, **ekw)
    assert np.array_equal(pm['replicates'], r.replicates[perm]) and np.array_equal(pm['stats'], r.stats[perm], equal_nan=True)
    # the device entry point of one class in several chunks of voxels, a shared weight vector among them
    import torch
    two = np.flatnonzero((K == 2) & ~csf)
    for Wd, rr in ((W[two], r.replicates[two]), (None, None)):
        if Wd is None:
            Wd = C.weights("shared", 30, T.M, 9)
            rr = T.bootstrap(Y, peaks, K, weights=Wd, **kw).replicates[two]
        d = engine.fit2d_weighted_bootstrap_dev(T, t(Y[two]), t(Wd), t(peaks[two]), 2, B=5, kind='residual', seed=11, q=Q, d_props=t(pr),
                                                d_groups=t(groups.astype(np.int32)), d_vox=t(two), keep=True, max_bytes=3 * 5 * T.M * 8)
        torch.cuda.synchronize()
        assert np.array_equal(d['replicates'].cpu().numpy(), rr[:, :, [0, 1, 2, 3, 4, 6, 7]])
        assert np.all(d['status'].cpu().numpy() == 0) and np.all(d['dir_status'].cpu().numpy() == 0)


# ---- 7. statuses
def test_failing_directions_come_first():
    rot = B2.rot_npz()
    errs = {e["why"]: e for e in json.loads(str(rot["errors_json"]))}
    e_plane = errs["in-plane new fascicle: 4 pairs"]
    T = U.RotateAtom2DTables(rot["fix_sig"], rot["fix_sch"], F2.Z, F2.DIFF)
    rng = np.random.default_rng(14)
    V, B = 8, 4
    Y, peaks = F2.two_fascicle_voxels(T, rng, V, 0.3)
    W = C.weights("smooth", V, T.M, 15)
    K = np.full(V, 2)
    K[1] = 1
    kw = dict(B=B, seed=2, keep=True, weights=W, fixed_weights=True)
    good = T.bootstrap(Y, peaks, K, on_error="nan", **kw)
    assert np.all(good.status == 0) and np.all(good.dir_status == 0) and np.all(np.isfinite(good.replicates))
    bad, Yb = peaks.copy(), Y.copy()
    bad[5, 3:6] = e_plane["newdir"]            # voxel 5, fascicle 1: a direction in the protocol's plane
    Yb[3, 10] = np.nan                          # voxel 3: a measurement that is not finite
    r = T.bootstrap(Yb, bad, K, on_error="nan", **kw)
    assert tuple(r.dir_status[5]) == (U.ROT2D_NEW_PAIRS, 0, 4, 0, 1) and not np.any(np.delete(r.dir_status, 5, axis=0))
    assert list(r.status) == [0, 0, 0, 2, 0, 2, 0, 0]
    for v in (3, 5):
        assert np.all(r.stats[v, :, 0] == 0) and np.all(np.isnan(r.stats[v, :, 1:])) and np.all(np.isnan(r.replicates[v]))
        assert np.all(r.agreement[v] == 0)
    keep = np.array([0, 1, 2, 4, 6, 7])
    assert np.array_equal(r.replicates[keep], good.replicates[keep]) and np.array_equal(r.stats[keep], good.stats[keep], equal_nan=True)
    with pytest.raises(Exception) as ei:
        T.bootstrap(Y, bad, K, **kw)
    assert (type(ei.value).__name__, str(ei.value)) == (e_plane["type"], e_plane["msg"])
    with force_plain():
        rp = T.bootstrap(Yb, bad, K, on_error="nan", **kw)
    assert np.array_equal(rp.dir_status, r.dir_status) and np.array_equal(rp.status, r.status)
    assert np.array_equal(rp.replicates, r.replicates, equal_nan=True) and np.array_equal(rp.stats, r.stats, equal_nan=True)


def test_weight_statuses_and_their_neighbours():
    T = B2.tables("syn2", 32, 12)
    rng = np.random.default_rng(19)
    V, B = 7, 4
    Y, peaks = F2.two_fascicle_voxels(T, rng, V, 0.1)
    K = np.full(V, 2)
    K[6] = 1
    W = C.weights("smooth", V, T.M, 20)
    Wb = W.copy()
    Wb[1, 5] = -1.0                            # a negative weight: 3
    Wb[2] = 0.0                                # no positive weight: 4
    Wb[4] = 0.0
    Wb[4, 9] = 1.0                             # one row of positive weight, one active atom at the least: M+ <= n_act, 1
    Wb[6, 7] = np.inf                          # not finite: 3 (a one-fascicle voxel)
    flagged = np.array([1, 2, 4, 6])
    keep = np.array([0, 3, 5])
    ekw = dict(B=B, seed=6, q=Q, keep=True)
    for plain in (False, True):
        if plain:
            _lib.lib().mfx_wboot2d_debug_set_force_plain(1)
        try:
            r = engine.fit2d_weighted_bootstrap(T, Y, Wb, K, None, peaks, 2, False, **ekw)
            ref = engine.fit2d_weighted_bootstrap(T, Y[keep], W[keep], K[keep], None, peaks[keep], 2, False, vox=keep, **ekw)
        finally:
            _lib.lib().mfx_wboot2d_debug_set_force_plain(0)
        assert list(r['status']) == [0, 3, 4, 0, 1, 0, 3] and not r['dir_status'].any()
        for v in flagged:
            assert np.all(r['stats'][v, :, 0] == 0) and np.all(np.isnan(r['stats'][v, :, 1:])) and np.all(np.isnan(r['replicates'][v]))
            assert not r['agree'][v].any()
        assert not ref['status'].any() and np.all(np.isfinite(ref['replicates']))
        assert np.array_equal(r['replicates'][keep], ref['replicates']) and np.array_equal(r['stats'][keep], ref['stats'], equal_nan=True)
        assert np.array_equal(r['agree'][keep], ref['agree'])


# ---- 8. ties
def test_duplicated_atom_takes_the_first_pair_in_every_replicate():
    sch = B2.rot_npz()["syn2_sch"]
    half = F2.atoms(sch, 20, 8)
    T = U.RotateAtom2DTables(np.hstack([half, half]), sch, F2.Z, F2.DIFF)      # atoms i and i + 20 are bit-identical columns
    rng = np.random.default_rng(9)
    V, B, M = 4, rep_tile() + 1, T.M
    peaks, Y = np.zeros((V, 6)), np.zeros((V, M))
    W = rng.uniform(0.05, 2.0, (V, M))
    for v in range(V):
        d = F2.random_dirs(rng, 2, 0.1)
        while abs(d[0] @ d[1]) > 0.85:
            d = F2.random_dirs(rng, 2, 0.1)
        cols = T.rotate_cols(d, np.array([3 + v, 11 + v]))
        Y[v] = 0.5 * cols[0] + 0.5 * cols[1]
        W[v, rng.choice(M, 12, replace=False)] = 0.0
        peaks[v] = d.reshape(-1)
    Ys = np.ascontiguousarray(Y[:, None, :] * (1.0 + 0.01 * rng.standard_normal((V, B, M))))
    Ys[:, 0] = Y                                                              # replicate 0: the exact mixture, the twins tie exactly
    got, st, wst = wreplicates_dev(T, Ys, W, peaks, 2)
    with force_plain():
        got2, _, _ = wreplicates_dev(T, Ys, W, peaks, 2)
    assert not st.any() and not wst.any() and np.array_equal(got, got2)
    assert np.array_equal(got, weighted_rows(T, Ys, W, peaks, 2))
    atoms = got[:, :, 3:5]
    assert np.all(atoms < 20)                                                 # the lowest (i1, i2) of every tied group
    for v in range(V):
        assert tuple(atoms[v, 0]) == (3 + v, 11 + v), (v, atoms[v, 0])        # the exact tie: the first of the four tied pairs


# ---- 9. the limit of the shared path
def test_limit_is_reported_and_held():
    lib = _lib.lib()
    T = B2.tables("syn2", 72, 6)
    lim = lib.mfx_wboot2d_max_atoms(T.handle())
    assert lib.mfx_wboot2d_max_atoms(None) == 0
    # the plain weighted two-fascicle kernel, whose arithmetic the shared path repeats, must serve the dictionary too
    assert 160 <= lim <= lib.mfx_w2d_max_atoms(T.handle(), 0) and lim % 16 == 0


def test_one_atom_above_the_limit_takes_the_plain_path():
    lib = _lib.lib()
    lim = lib.mfx_wboot2d_max_atoms(B2.tables("syn2", 72, 6).handle())
    if lim > 1024:
        # the limit is set by the LDS of the two-fascicle kernels (some 3600 atoms): a dictionary one atom above it has
        # 13 million pairs per replicate row in the explicit solver of the plain path, far beyond a test of a few seconds
        pytest.skip("mfx_wboot2d_max_atoms = %d: one atom above it is out of a quick test's reach" % lim)
    T = B2.tables("syn2", lim + 1, 6)
    Ys, peaks = B2.replicate_signals(T, np.random.default_rng(2), 2, 3, 0.1)
    W = C.weights("smooth", 2, T.M, 3)
    got, st, wst = wreplicates_dev(T, Ys, W, peaks, 2)
    assert not st.any() and not wst.any() and np.array_equal(got, weighted_rows(T, Ys, W, peaks, 2))
