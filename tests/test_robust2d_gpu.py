"""Robust fits of 2-D (AxCaliber-like) protocols on the GPU (include/mfx_robust2d.h, csrc/robust2d.hip):
engine.fit2d_robust / fit2d_robust_dev / RotateAtom2DTables.fit(robust=...) against the loop a user writes by hand from
engine.fit2d, engine.fit2d_weighted, engine.predict2d and the NumPy rule of tests/_robust_ref.py - bit for bit - and
against a referee loop that shares no kernel with the fits (tests/_robust2d_ref.referee_backend).

Protocols: syn2 (M = 66, N = 24 atoms; N = 8 for the three-fascicle class; N = 72 for the referee, where the fused K = 2
kernel matters) and fix (M = 1776, N = 8).  Each test prints what it measures before it asserts."""
import os

import numpy as np
import pytest

import _post_ref as R
import _robust2d_ref as R2
import _robust_ref as RR
import _w2d_ref as W2
import _wfit_ref as WR
from test_fit2d_gpu import DIFF, Z, atoms, csf_signal, random_dirs
from microstructure_fingerprinting_amd import _lib, engine
from microstructure_fingerprinting_amd import mf_utils as U

pytestmark = pytest.mark.gpu

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
EPS = R.EPS
_cache = {}


def tables(name, N, seed):
    key = ("T", name, N, seed)
    if key not in _cache:
        sch = np.load(os.path.join(G, "rot2d_cases.npz"))[name + "_sch"]
        _cache[key] = (U.RotateAtom2DTables(atoms(sch, N, seed), sch, Z, DIFF), csf_signal(sch))
    return _cache[key]


def mixed():
    """A mixed batch on syn2: K in {0, 1, 2}, two CSF voxels per K (the CSF classes take the explicit solver)."""
    if "mixed" not in _cache:
        T, sig_csf = tables("syn2", 24, 11)
        V = 24
        peaks, Y = R2.make_voxels(T, V, 61, 0.1)
        K = np.arange(V) % 3
        csf = (np.arange(V) % 4) == 0
        Y[csf] = 0.8 * Y[csf] + 100.0 * sig_csf
        rng = np.random.default_rng(62)
        W0 = rng.uniform(0.5, 2.0, Y.shape)             # noise levels, and rows excluded for good
        for v in range(V):
            W0[v, rng.choice(Y.shape[1], 1 + v % 2, replace=False)] = 0.0
        for k in range(3):
            assert np.count_nonzero((K == k) & csf) == 2 and np.count_nonzero((K == k) & ~csf) > 0
        _cache["mixed"] = dict(T=T, sig_csf=sig_csf, V=V, peaks=peaks, Y=Y, K=K, csf=csf, W0=W0)
    return _cache["mixed"]


def loop_trace(base, loss, n_iter, c=4.45):
    """The hand-made loop's results after 0 .. n_iter iterations on the mixed batch, and the fits' direction records"""
    key = ("trace", base, loss, n_iter, c)
    if key not in _cache:
        b = mixed()
        be = R2.engine2d_backend(b["T"])
        W0 = {"none": None, "full": b["W0"], "shared": b["W0"][0]}[base]
        tr = RR.loop_ref(be, b["Y"], b["K"], b["csf"], b["peaks"], 2, True, b["sig_csf"], W0, loss, c, n_iter, trace=True)
        _cache[key] = (tr, be.dir_status)
    return _cache[key]


def same(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.int64), np.ascontiguousarray(b).view(np.int64))


def assert_equal_loop(got, ref, ref_dstat, what, n_changed=True):
    p, W, info = got
    rp, rW, ri = ref
    assert same(p, rp), what
    assert same(W, rW), what
    assert same(info["scale"], ri["scale"]) and np.array_equal(info["state"], ri["state"]), what
    assert np.array_equal(info["dir_status"], ref_dstat), what
    assert np.array_equal(info["status"], ri["status"]), what
    if n_changed:
        assert np.array_equal(np.asarray(info["n_changed"]), ri["n_changed"]), what


# ---- 7. the loop equals the hand-made loop, bit for bit
@pytest.mark.parametrize("loss", RR.LOSSES)
@pytest.mark.parametrize("base", ["none", "full", "shared"])
def test_fit2d_robust_equals_hand_made_loop(base, loss):
    b = mixed()
    T = b["T"]
    W0 = {"none": None, "full": b["W0"], "shared": b["W0"][0]}[base]
    trace, dstat = loop_trace(base, loss, 3)
    for n_iter in (0, 1, 2, 3):
        got = engine.fit2d_robust(T, b["Y"], b["K"], b["csf"], b["peaks"], 2, True, b["sig_csf"], W0=W0, loss=loss, c=4.45, n_iter=n_iter)
        what = "base=%s loss=%s n_iter=%d" % (base, loss, n_iter)
        assert_equal_loop(got, trace[n_iter], dstat, what)
        assert np.all(got[2]["status"] == 0) and np.all(got[2]["dir_status"] == 0), what
        assert got[2]["n_changed"].dtype == np.int64 and 0 <= got[2]["n_iter_used"] <= n_iter
        if n_iter == 0:
            assert np.array_equal(got[1], np.broadcast_to(np.ones(T.M) if W0 is None else W0, got[1].shape))
    none = (b["K"] == 0) & ~b["csf"]
    assert none.any() and np.all(got[0][none] == 0)
    # the reweighting did something: rows went out, and the fit moved
    if loss == "cutoff":
        assert np.count_nonzero(trace[3][1] == 0) > (0 if W0 is None else np.count_nonzero(np.broadcast_to(W0, trace[3][1].shape) == 0))
    assert not same(trace[3][0], trace[0][0])


def test_long_protocol_and_three_fascicles():
    # fix: M = 1776, V = 6, K = 2, cutoff
    T, _ = tables("fix", 8, 12)
    V = 6
    peaks, Y = R2.make_voxels(T, V, 63, 0.3)
    K = np.full(V, 2)
    be = R2.engine2d_backend(T)
    ref = RR.loop_ref(be, Y, K, None, peaks, 2, False, None, None, "cutoff", 4.45, 2)
    got = engine.fit2d_robust(T, Y, K, None, peaks, 2, False, n_iter=2)
    print("fix: n_changed %s, rejected rows per voxel %s" % (got[2]["n_changed"], np.count_nonzero(got[1] == 0, axis=1)))
    assert_equal_loop(got, ref, be.dir_status, "fix")
    assert np.count_nonzero(got[1] == 0) > 0
    # maxfasc = 3, three K = 3 voxels at N = 8: the explicit solver
    T3, _ = tables("syn2", 8, 5)
    rng = np.random.default_rng(64)
    V = 3
    peaks, Y = np.zeros((V, 9)), np.zeros((V, T3.M))
    for v in range(V):
        d = random_dirs(rng, 3, 0.1)
        ids = rng.integers(0, T3.N, 3)
        f = rng.uniform(0.2, 0.5, 3)
        y = 500.0 * (T3.rotate_cols(d, ids).T @ (f / f.sum())) + rng.normal(0, 500.0 / 30.0, T3.M)
        bad = rng.choice(T3.M, 4, replace=False)
        y[bad] *= rng.uniform(0.1, 0.5, 4)
        peaks[v], Y[v] = d.reshape(-1), y
    K = np.full(V, 3)
    be = R2.engine2d_backend(T3)
    ref = RR.loop_ref(be, Y, K, None, peaks, 3, False, None, None, "cutoff", 4.45, 2)
    got = engine.fit2d_robust(T3, Y, K, None, peaks, 3, False, n_iter=2)
    assert_equal_loop(got, ref, be.dir_status, "K = 3")
    assert np.all(np.isfinite(got[0])) and np.all(got[0][:, 0] > 0)


# ---- 8. early stop is invisible
def test_early_stop_is_invisible():
    b = mixed()
    T = b["T"]
    a = (b["Y"], b["K"], b["csf"], b["peaks"], 2, True, b["sig_csf"])
    trace, dstat = loop_trace("none", "cutoff", 8)
    got = engine.fit2d_robust(T, *a, n_iter=8)
    print("n_changed %s, reference %s, n_iter_used %d of 8" % (got[2]["n_changed"], trace[8][2]["n_changed"], got[2]["n_iter_used"]))
    assert_equal_loop(got, trace[8], dstat, "n_iter = 8")
    assert 1 <= got[2]["n_iter_used"] < 8
    # with a cutoff no residual reaches, iteration 0 changes no weight: the loop stops there and keeps the parameters of the
    # fit on the shared [M] base weights, where the hand-made loop refits on their [V, M] spread - the same bits
    w0 = b["W0"][0]
    be = R2.engine2d_backend(T)
    ref = RR.loop_ref(be, *a, w0, "cutoff", 1e6, 2)
    assert np.array_equal(ref[2]["n_changed"], [0, 0])
    got = engine.fit2d_robust(T, *a, W0=w0, loss="cutoff", c=1e6, n_iter=2)
    assert got[2]["n_iter_used"] == 1 and np.array_equal(got[2]["n_changed"], [0, 0])
    assert_equal_loop(got, ref, be.dir_status, "shared base weights")
    assert same(got[1], np.ascontiguousarray(np.broadcast_to(w0, got[1].shape)))
    # without base weights the parameters after iteration 0 have to be the weighted kernels': the loop goes on once
    ref = RR.loop_ref(be, *a, None, "cutoff", 1e6, 3)
    got = engine.fit2d_robust(T, *a, loss="cutoff", c=1e6, n_iter=3)
    assert got[2]["n_iter_used"] == 2 and np.array_equal(got[2]["n_changed"], [0, 0, 0])
    assert_equal_loop(got, ref, be.dir_status, "no base weights")
    assert np.all(got[1] == 1)


# ---- 9. the device-resident path on a stream of its own;  10. the plan is made once
def test_fit2d_robust_dev_equals_fit2d_robust_and_plans_once():
    import torch
    T, _ = tables("syn2", 24, 11)
    V = 21
    peaks, Y = R2.make_voxels(T, V, 71, 0.1)
    W0 = mixed()["W0"][:V]
    s = torch.cuda.Stream()
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()   # noqa: E731
    lib = _lib.lib()
    for k in (1, 2):
        for w0, loss in ((None, "cutoff"), (W0[1], "huber"), (W0, "tukey")):
            pk = np.ascontiguousarray(peaks[:, :3 * k])
            hp, hW, hi = engine.fit2d_robust(T, Y, np.full(V, k), None, pk, k, False, W0=w0, loss=loss, n_iter=3)
            n_host = lib.mfx_robust2d_debug_last_plan_directions()
            dY, dp, dW0 = t(Y), t(pk), (t(w0) if w0 is not None else None)
            torch.cuda.synchronize()
            with torch.cuda.stream(s):
                p, W, info = engine.fit2d_robust_dev(T, dY, dp, k, d_W0=dW0, loss=loss, n_iter=3)
            n_dev = lib.mfx_robust2d_debug_last_plan_directions()
            torch.cuda.synchronize()
            what = "K=%d loss=%s" % (k, loss)
            print("%s: directions planned: host form %d, device form %d (V = %d, 3 iterations)" % (what, n_host, n_dev, V))
            assert n_host == k * V and n_dev == k * V, what             # not (1 + 2 * 3) k V
            assert same(p.cpu().numpy(), hp) and same(W.cpu().numpy(), hW), what
            assert same(info["scale"].cpu().numpy(), hi["scale"]) and np.array_equal(info["state"].cpu().numpy(), hi["state"]), what
            assert np.array_equal(info["status"].cpu().numpy(), hi["status"]), what
            assert np.array_equal(info["dir_status"].cpu().numpy(), hi["dir_status"]), what
            assert np.array_equal(info["n_changed"].cpu().numpy(), hi["n_changed"]), what
    p0, W0_, i0 = engine.fit2d_robust_dev(T, t(Y), t(peaks), 2, n_iter=0)
    torch.cuda.synchronize()
    plain, _ = engine.fit2d(T, Y, np.full(V, 2), None, peaks, 2, False)
    assert same(p0.cpu().numpy(), plain) and np.all(W0_.cpu().numpy() == 1) and i0["n_changed"].numel() == 0


# ---- 11. bad voxels
def test_failing_direction_and_unusable_base_weights():
    b = mixed()
    T = b["T"]
    V = b["V"]
    vd, vw = 5, 7                                   # K = 2 and K = 1, no CSF
    assert b["K"][vd] == 2 and b["K"][vw] == 1 and not b["csf"][vd] and not b["csf"][vw]
    peaks, W0 = b["peaks"].copy(), b["W0"].copy()
    peaks[vd, 3:6] = [0.0, 0.0, 2.0]
    W0[vw, 3] = -1.0
    p, W, info = engine.fit2d_robust(T, b["Y"], b["K"], b["csf"], peaks, 2, True, b["sig_csf"], W0=W0, n_iter=2)
    assert np.all(np.isnan(p[vd])) and info["state"][vd] == 1 and np.isnan(info["scale"][vd]) and same(W[vd], W0[vd])
    assert np.array_equal(info["dir_status"][vd, [0, 4]], [U.ROT2D_NEWDIR_NORM, 1]) and info["status"][vd] == 0
    assert np.all(np.isnan(p[vw])) and info["state"][vw] == 3 and info["status"][vw] == 1 and same(W[vw], W0[vw])
    assert np.all(info["dir_status"][vw] == 0)
    ok = np.ones(V, bool)
    ok[[vd, vw]] = False
    good = engine.fit2d_robust(T, b["Y"][ok], b["K"][ok], b["csf"][ok], b["peaks"][ok], 2, True, b["sig_csf"], W0=b["W0"][ok], n_iter=2)
    assert same(p[ok], good[0]) and same(W[ok], good[1]) and same(info["scale"][ok], good[2]["scale"])
    assert np.array_equal(info["state"][ok], good[2]["state"]) and np.all(info["dir_status"][ok] == 0) and np.all(info["status"][ok] == 0)
    be = R2.engine2d_backend(T)
    ref = RR.loop_ref(be, b["Y"], b["K"], b["csf"], peaks, 2, True, b["sig_csf"], W0, "cutoff", 4.45, 2)
    assert_equal_loop((p, W, info), ref, be.dir_status, "bad voxels", n_changed=True)
    # the tables API: 'raise' raises the direction's exception, 'nan' returns the rows
    with pytest.raises(ValueError, match="unit norm"):
        T.fit(b["Y"], peaks, b["K"], b["csf"], b["sig_csf"], robust={"n_iter": 1})
    r = T.fit(b["Y"], peaks, b["K"], b["csf"], b["sig_csf"], on_error="nan", robust={"n_iter": 1})
    assert np.array_equal(r.failed, [vd]) and np.all(np.isnan(r.params[vd])) and r.robust_info["state"][vd] == 1


# ---- 12. the tables API
def test_tables_api():
    sch = np.load(os.path.join(G, "rot2d_cases.npz"))["syn2_sch"]
    N, V = 48, 16
    dic = atoms(sch, N, 101)
    T = U.RotateAtom2DTables(dic, sch, Z, DIFF)
    rad = np.linspace(0.5, 4.0, N)[np.random.default_rng(103).permutation(N)]
    Y, peaks, ids, planted = W2.outlier_voxels(T.rotate_cols, T.M, N, V, 102)
    K = np.full(V, 2)
    # the recipe
    plain = T.fit(Y, peaks, K)
    res = T.residuals(Y, plain, peaks)
    a = np.abs(res)
    Wk = a <= 4.45 * np.median(a, axis=1, keepdims=True)
    by_hand = T.fit(Y, peaks, K, weights=Wk)
    r = T.fit(Y, peaks, K, robust={"n_iter": 1})
    assert same(r.params, by_hand.params) and np.array_equal(r.status, by_hand.status)
    assert r.weights.dtype == np.float64 and np.array_equal(r.weights, Wk.astype(np.float64))
    assert np.array_equal(r.outlier_mask(), ~Wk) and np.array_equal(r.n_rejected, np.count_nonzero(~Wk, axis=1))
    assert np.array_equal(r.outlier_mask(), r.weights == 0) and r.outlier_mask().dtype == np.bool_
    assert same(r.robust_scale, np.median(a, axis=1)) and np.all(r.robust_info["state"] == 0)
    caught = np.array([np.all(r.outlier_mask()[v, planted[v]]) for v in range(V)])
    hit_plain = int(np.count_nonzero(np.all(plain.atoms == ids, axis=1)))
    hit = int(np.count_nonzero(np.all(r.atoms == ids, axis=1)))
    print("planted outliers rejected in %d of %d voxels; planted atoms recovered: plain fit %d, robust fit %d" % (caught.sum(), V, hit_plain, hit))
    assert plain.robust_info is None and plain.weights is None
    # robust=True is three iterations of the same; base weights stay out
    r3 = T.fit(Y, peaks, K, robust=True)
    e3 = engine.fit2d_robust(T, Y, K, None, peaks, 2, False, n_iter=3)
    assert same(r3.params, e3[0]) and same(r3.weights, e3[1]) and r3.robust_info["n_changed"].shape == (3,)
    w0 = np.ones(T.M)
    w0[:3] = 0.0
    rb = T.fit(Y, peaks, K, weights=w0, robust={"n_iter": 1, "loss": "huber"})
    assert np.all(rb.weights[:, :3] == 0) and not np.any(rb.outlier_mask()[:, :3]) and np.all(rb.weights[:, 3:] > 0)
    r2 = U.fit_2Dprotocol(dic, sch, Z, DIFF, Y, peaks, K, robust={"n_iter": 1})
    assert same(r2.params, r.params) and same(r2.weights, r.weights)
    # the posterior and the profile answer for the final weighted objective
    post = T.posterior(Y, peaks, K, fit=r, props={"rad": rad})
    post_w = T.posterior(Y, peaks, K, weights=r.weights, props={"rad": rad})
    assert np.all(post.status == 0)
    assert np.array_equal(post.weights, post_w.weights) and np.array_equal(post.log_sum, post_w.log_sum)
    prof = T.profile(Y, peaks, K, partner=True, weights=r.weights)
    sw = r.weights.sum(-1)
    for v in range(V):
        D = T.rotate(peaks[v].reshape(2, 3))
        ref = W2.pair_ref(D, Y[v], r.weights[v])
        B = 16 * T.M * EPS * ref["ysq"] / float(ref["c2bar"][r.atoms[v, 0], r.atoms[v, 1]])
        assert abs(prof.obj[v].min() - r.MSE[v] * sw[v]) <= 2 * B             # min obj = MSE * sum W (tests/test_w2d_gpu.py)
        assert prof.partner[v, 0, r.atoms[v, 0]] == r.atoms[v, 1]
    m, s = T.posterior_moments(Y, peaks, K, rad, weights=r.weights)
    assert np.array_equal(m, post.mean("rad")) and np.array_equal(s, post.std("rad"))


# ---- 13. a referee that shares no kernel with the loop's fits
REFEREE_SEED = 203         # chosen on the CPU with the reference's own rotate_atom_2Dprotocol (DESIGN.md 4.20 has the gaps)
REFEREE_CAUGHT = 12        # voxels in which the referee loop itself, run on the CPU on the reference's rotation, rejects all planted rows
REFEREE_GAP = 1e-8


def test_referee_loop():
    """_robust_ref.loop_ref with the CPU solver on sqrt(W) * T.rotate(dirs) as its fits and the NumPy sum over T.rotate's
    columns as its prediction: equal atom indices and W, the other columns at _wfit_ref.assert_rows' tolerances - given that
    at every fit of the referee loop the smallest top-2 gap is >= 1e-8 |y'|^2."""
    N, V = 72, 12
    T, _ = tables("syn2", N, REFEREE_SEED)
    Y, peaks, ids, planted = W2.outlier_voxels(T.rotate_cols, T.M, N, V, REFEREE_SEED + 1)
    K = np.full(V, 2)
    be = R2.referee_backend(T, peaks)
    rp, rW, ri = RR.loop_ref(be, Y, K, None, peaks, 2, False, None, None, "cutoff", 4.45, 2)
    print("smallest top-2 gap / |y'|^2 at the referee's fits 0, 1, 2: %s" % ", ".join("%.2e" % g for g in be.gaps))
    assert len(be.gaps) == 3 and min(be.gaps) >= REFEREE_GAP
    p, W, info = engine.fit2d_robust(T, Y, K, None, peaks, 2, False, n_iter=2)
    plain, _ = engine.fit2d(T, Y, K, None, peaks, 2, False)
    hit_plain = int(np.count_nonzero(np.all(plain[:, 3:5] == ids, axis=1)))
    hit = int(np.count_nonzero(np.all(p[:, 3:5] == ids, axis=1)))
    caught = int(np.count_nonzero([np.all(W[v, planted[v]] == 0) for v in range(V)]))
    ref_caught = int(np.count_nonzero([np.all(rW[v, planted[v]] == 0) for v in range(V)]))
    print("both planted atoms recovered in %d of %d voxels without robust, %d with; planted rows all rejected in %d voxels "
          "(referee loop here %d, on the CPU %d)" % (hit_plain, V, hit, caught, ref_caught, REFEREE_CAUGHT))
    assert np.array_equal(p[:, 3:5], rp[:, 3:5])
    assert np.array_equal(W, rW)
    WR.assert_rows(p, rp, 2, "robust 2-D against the referee loop")
    assert np.array_equal(info["state"], ri["state"]) and np.array_equal(info["n_changed"], ri["n_changed"])
    assert np.allclose(info["scale"], ri["scale"], rtol=WR.RTOL_W, atol=0)
    assert hit >= hit_plain and caught >= REFEREE_CAUGHT
