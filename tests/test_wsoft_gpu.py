"""Profiles and soft fits of a weighted fit on the GPU (include/mfx_wsoft.h): engine.posterior / profile /
pair_objectives with measurement weights, their device forms, and MFModelFit.profile / interval / posterior /
posterior_moments after MFModel.fit(weights=...).

The referee of a weighted voxel is the long-double referee of tests/_post_ref.py on rows scaled by s = sqrt(W):
gram(s y, s D_0, s D_1, s x) from the oracle's rotation, pair_values with the kernel's cut, posterior.  The bars are its
derived ones, B = 16 M eps ||s y||^2 / (1 - c^2) per pair propagated as that file documents; for the profile the bar is B
at the voxel's worst conditioned pair, as in tests/test_profile_gpu.py.  One fascicle: F(i) from the same Gram
quantities (with CSF the best support of the two unknowns), B = 16 M eps ||s y||^2.  Nothing is measured on the code
under test.  Every comparison asserts as a condition on its inputs that no pair has 1 - c^2 within [cut / 4, 4 cut]; the
seeds below were chosen on the host so that it holds for every voxel.

Each test prints what it measures before it asserts; the figures seen on the MI355X are in DESIGN.md 4.16.
"""
import numpy as np
import pytest

import _post_ref as R
import _wfit_ref  # noqa: F401  (the weighted fit's packing rules: MSE = objective / sum W)
from _post_ref import TP

pytestmark = pytest.mark.gpu

EPS, LD = R.EPS, R.LD
SIGMA = 500.0 / 30.0      # the synthetic voxels' noise: M0 / SNR of synth.make_voxels
KINDS = ["small", "c2", "synth300", "ukbb"]
SEEDS = {"small": 4101, "c2": 4102, "synth300": 4103, "ukbb": 4104}
_cases, _refs = {}, {}


def _weights(rng, V, M):
    """real-valued weights in [0, 4], about 15 % exact zeros, another zero pattern in every voxel"""
    W = rng.uniform(0.0, 4.0, (V, M))
    W[rng.random((V, M)) < 0.15] = 0.0
    return np.ascontiguousarray(W)


def _case(kind):
    """peaks [V x 6], Y [V x M], W [V x M] of a model: 3 voxels (2 at 986 atoms)"""
    if kind not in _cases:
        rng = np.random.default_rng(SEEDS[kind])
        if kind == "ukbb":
            d = TP._load("real_ukbb_fit_k2")
            peaks, Y = np.ascontiguousarray(d["peaks"][:2, :6]), np.ascontiguousarray(d["Y"][:2])
        else:
            peaks, Y = TP._synth_voxels(kind, 3, 2, seed=SEEDS[kind] + 50)
        _cases[kind] = (peaks, Y, _weights(rng, Y.shape[0], Y.shape[1]))
    return _cases[kind]


def _scaled(kind, y, w, pk, K, csf):
    s = np.sqrt(np.asarray(w, dtype=np.float64))
    D0 = TP._rot(kind, pk[:3])
    D1 = TP._rot(kind, pk[3:6]) if K == 2 else None
    x = TP._sig_csf(kind) if csf else None
    return s, s * y, s[:, None] * D0, (s[:, None] * D1 if K == 2 else None), (s * x if csf else None)


def _F(kind, y, w, pk, K, csf, rows=None):
    """the referee's values of one voxel, computed once: dict(F, c2bar, c2s, ysq, M, clear); K = 1: F [N x 1].
    rows: the protocol with the other rows deleted (unit weights on the kept ones)."""
    key = (kind, y.tobytes(), np.asarray(w).tobytes(), K, bool(csf), None if rows is None else rows.tobytes())
    if key in _refs:
        return _refs[key]
    cut = TP._cut()
    s, ys, D0, D1, xs = _scaled(kind, y, w, pk, K, csf)
    if rows is not None:
        ys, D0, D1, xs = ys[rows], D0[rows], (D1[rows] if K == 2 else None), (xs[rows] if csf else None)
    M = ys.shape[0]
    if K == 2:
        g = R.gram(ys, D0, D1, xs)
        F, c2bar, c2s, _ = R.pair_values(g, csf, cut)
    else:
        g = R.gram(ys, D0, D0[:, :1], xs)
        A, Yv, ysq = g["A11"], g["Y1"], g["ysq"]
        sc = TP._single(Yv, A)
        c2s = []
        if csf:
            X, xx, xy = g["X1"], g["xx"], g["xy"]
            c2 = 1 - X * X / (A * xx)
            both = np.where(c2 > cut, TP._pair_inner(A, xx, X, Yv, xy), -np.inf)
            sc = np.maximum(np.maximum(sc, TP._single(xy, xx)), both)
            c2s = [c2]
        F, c2bar = ysq - sc, np.ones_like(sc)
    out = {"F": F, "c2bar": c2bar, "c2s": c2s, "ysq": float(g["ysq"]), "M": M, "clear": R.clear_of_the_cut(c2s, cut)}
    _refs[key] = out
    return out


def _post_ref(f, T):
    return R.posterior(f["F"], f["c2bar"], f["ysq"], f["M"], T)


def _post_ratio(w, log_sum, ref, K):
    r = max(float(np.max(np.abs(np.asarray(w[k]).astype(LD) - ref["w"][k]) / ref["bar_w"][k])) for k in range(K))
    return max(r, float(abs(LD(log_sum) - ref["log_sum"]) / ref["bar_log_sum"]))


def _prof_bar(f):
    return 16 * f["M"] * EPS * f["ysq"] / float(np.min(f["c2bar"]))


def _sigma(kind, f, w, K, csf):
    """the noise level of a voxel: the synthetic one, or for the UKBB data the referee's residual variance"""
    if kind != "ukbb":
        return SIGMA
    return float(np.sqrt(float(f["F"].min()) / (np.count_nonzero(w > 0) - K - int(csf))))


def _check_voxel(tag, kind, y, w, pk, K, csf, T, got_w, got_ls, got_st, obj, par, f=None):
    """posterior and profile of one voxel against the referee; returns the two worst error / bar ratios"""
    f = f if f is not None else _F(kind, y, w, pk, K, csf)
    assert f["clear"], "%s: a pair near the cut: this input was chosen to have none" % tag
    ref = _post_ref(f, T)
    rp = _post_ratio(got_w, got_ls, ref, K)
    F, bar = f["F"], _prof_bar(f)
    refobj = [F.min(axis=1), F.min(axis=0)][:K]
    ro = max(float(np.max(np.abs(obj[k].astype(LD) - refobj[k]))) / bar for k in range(K))
    print("%s K=%d csf=%d: posterior %.3g of the bar (log_sum %.6f), profile %.3g of the bar %.3g"
          % (tag, K, csf, rp, float(got_ls), ro, bar))
    assert got_st == 0
    assert rp <= 1.0, "%s: posterior at %.3g of the bar" % (tag, rp)
    assert ro <= 1.0, "%s: profile at %.3g of the bar" % (tag, ro)
    if K == 1:
        assert np.all(par[0] == -1)
    else:
        for k in range(2):
            Fk = F if k == 0 else F.T
            at = Fk[np.arange(Fk.shape[0]), par[k]] - Fk.min(axis=1)
            assert np.all(at <= bar), "%s slot %d: a partner that is not a minimiser" % (tag, k)
    return rp, ro


def _run(kind, Y, W, peaks, K, csf, sigma, shift):
    """engine.posterior and engine.profile (with partner) of one class"""
    from microstructure_fingerprinting_amd import engine
    V = Y.shape[0]
    plan, x = TP._plan(kind), (TP._sig_csf(kind) if csf else None)
    pk = np.ascontiguousarray(peaks[:, :3 * K])
    post = engine.posterior(plan, Y, np.full(V, K), np.full(V, csf), pk, K, csf, x, sigma, shift=shift, W=W)
    prof = engine.profile(plan, Y, np.full(V, K), np.full(V, csf), pk, K, csf, x, partner=True, W=W)
    assert post[3] == 0 and prof[2] == 0
    return post, prof


# ------------------------------------------------------------------------------------------------
# 1. the referee at the smallest shapes that can go wrong
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("csf", [False, True])
@pytest.mark.parametrize("K", [2, 1])
@pytest.mark.parametrize("kind", KINDS)
def test_against_the_referee(kind, K, csf):
    """14 atoms (less than a tile), 48 (fewer tiles than waves), 300 (19 tiles: a second sweep, a padded last tile), 986
    with G-bracketed rows: posterior weights, log_sum, profile values and partners of every voxel."""
    peaks, Y, W = _case(kind)
    V = Y.shape[0]
    fs = [_F(kind, Y[v], W[v], peaks[v], K, csf) for v in range(V)]
    sigma = np.array([_sigma(kind, fs[v], W[v], K, csf) for v in range(V)])
    shift = np.array([float(f["F"].min()) for f in fs])
    (w, ls, st, _), (obj, par, _) = _run(kind, Y, W, peaks, K, csf, sigma, shift)
    worst = [0.0, 0.0]
    for v in range(V):
        r = _check_voxel("%s/%d" % (kind, v), kind, Y[v], W[v], peaks[v], K, csf, 2.0 * sigma[v] ** 2, w[v], ls[v], st[v], obj[v],
                         par[v], fs[v])
        worst = [max(a, b) for a, b in zip(worst, r)]
    print("%s K=%d csf=%d: worst posterior %.3g, worst profile %.3g of their bars over %d voxels" % (kind, K, csf, worst[0], worst[1], V))


@pytest.mark.parametrize("csf", [False, True])
def test_shared_weight_vector_and_default_shift(csf):
    """one [M] vector for all voxels (w_stride = 0), and the shift engine.posterior takes by default: the weighted fit's
    MSE * sum W, which equals the referee's minimum within the profile bar"""
    from microstructure_fingerprinting_amd import engine
    kind = "c2"
    peaks, Y, W = _case(kind)
    w1 = np.ascontiguousarray(W[1])
    V = Y.shape[0]
    (w, ls, st, _), (obj, par, _) = _run(kind, Y, w1, peaks, 2, csf, SIGMA, None)
    for v in range(V):
        _check_voxel("c2 shared/%d" % v, kind, Y[v], w1, peaks[v], 2, csf, 2.0 * SIGMA ** 2, w[v], ls[v], st[v], obj[v], par[v])
    fit, fst = engine.fit_weighted(TP._plan(kind), Y, w1, np.full(V, 2), np.full(V, csf), peaks, 2, csf, TP._sig_csf(kind) if csf else None)
    for v in range(V):
        f = _F(kind, Y[v], w1, peaks[v], 2, csf)
        assert fst[v] == 0 and abs(fit[v, -2] * w1.sum() - float(f["F"].min())) <= _prof_bar(f)


@pytest.mark.parametrize("csf", [False, True])
@pytest.mark.parametrize("kind", ["small", "c2"])
def test_pair_objectives_entrywise(kind, csf):
    from microstructure_fingerprinting_amd import engine
    peaks, Y, W = _case(kind)
    got = engine.pair_objectives(TP._plan(kind), Y, peaks, csf, TP._sig_csf(kind) if csf else None, W=W)
    for v in range(Y.shape[0]):
        f = _F(kind, Y[v], W[v], peaks[v], 2, csf)
        assert f["clear"], "a pair near the cut: this input was chosen to have none"
        bar = 16 * f["M"] * EPS * f["ysq"] / f["c2bar"].astype(LD)
        err = np.abs(got[v].astype(LD) - f["F"])
        print("%s csf=%d voxel %d: worst |F_W - referee| / bar = %.3g" % (kind, csf, v, float(np.max(err / bar))))
        assert np.all(err <= bar)


@pytest.mark.parametrize("csf", [False, True])
@pytest.mark.parametrize("K", [2, 1])
def test_302_row_protocol(K, csf):
    """M > 200 takes the KSTEPS = 140 instantiations (and 4 480 more bytes of LDS): two voxels of the 302-row, 64-atom
    model of tests/test_post_gpu.py against the referee, and unit weights against the unweighted call bit for bit."""
    from microstructure_fingerprinting_amd import engine
    import test_post_gpu as TPG
    kind = TPG._long_model()
    peaks, Y = TP._synth_voxels(kind, 2, 2, seed=4105)
    V, M = Y.shape
    assert M == 302
    W = _weights(np.random.default_rng(4106), V, M)
    fs = [_F(kind, Y[v], W[v], peaks[v], K, csf) for v in range(V)]
    shift = np.array([float(f["F"].min()) for f in fs])
    (w, ls, st, _), (obj, par, _) = _run(kind, Y, W, peaks, K, csf, SIGMA, shift)
    for v in range(V):
        _check_voxel("long302/%d" % v, kind, Y[v], W[v], peaks[v], K, csf, 2.0 * SIGMA ** 2, w[v], ls[v], st[v], obj[v], par[v], fs[v])
    plan, x = TP._plan(kind), (TP._sig_csf(kind) if csf else None)
    pk = np.ascontiguousarray(peaks[:, :3 * K])
    Kv, cv = np.full(V, K), np.full(V, csf)
    a = engine.posterior(plan, Y, Kv, cv, pk, K, csf, x, SIGMA, shift=shift)
    b = engine.posterior(plan, Y, Kv, cv, pk, K, csf, x, SIGMA, shift=shift, W=np.ones(M))
    for p, q in zip(a[:3], b[:3]):
        assert np.array_equal(p, q)
    a = engine.profile(plan, Y, Kv, cv, pk, K, csf, x, partner=True)
    b = engine.profile(plan, Y, Kv, cv, pk, K, csf, x, partner=True, W=np.ones((V, M)))
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


# ------------------------------------------------------------------------------------------------
# 2. W = 1 is the unweighted entry point, bit for bit
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("csf", [False, True])
@pytest.mark.parametrize("K", [2, 1])
@pytest.mark.parametrize("kind", ["small", "c2", "synth300"])
def test_unit_weights_equal_the_unweighted_entry_points_bit_for_bit(kind, K, csf):
    """At 14, 48 and 300 atoms (M <= 200) the extra [MP] doubles of LDS are far from moving the configuration: without
    CSF (8, 2, 2) holds up to 816 atoms in the weighted profile (848 unweighted; posterior 1 024 and 1 056), with CSF
    (4, 1, 2) up to 1 472, so both calls run the same (NW, TILES, NBUF, KS)."""
    from microstructure_fingerprinting_amd import engine
    peaks, Y, _ = _case(kind)
    V, M = Y.shape
    plan, x = TP._plan(kind), (TP._sig_csf(kind) if csf else None)
    pk = np.ascontiguousarray(peaks[:, :3 * K])
    Kv, cv = np.full(V, K), np.full(V, csf)
    shift = engine.profile(plan, Y, Kv, cv, pk, K, csf, x)[0][:, 0].min(axis=1)
    for ones in (np.ones((V, M)), np.ones(M)):
        a = engine.posterior(plan, Y, Kv, cv, pk, K, csf, x, SIGMA, shift=shift)
        b = engine.posterior(plan, Y, Kv, cv, pk, K, csf, x, SIGMA, shift=shift, W=ones)
        assert (a[2] == 0).all()
        for p, q in zip(a[:3], b[:3]):
            assert np.array_equal(p, q)
        a = engine.profile(plan, Y, Kv, cv, pk, K, csf, x, partner=True)
        b = engine.profile(plan, Y, Kv, cv, pk, K, csf, x, partner=True, W=ones)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    if K == 2 and kind != "synth300":
        assert np.array_equal(engine.pair_objectives(plan, Y, pk, csf, x), engine.pair_objectives(plan, Y, pk, csf, x, W=np.ones(M)))


# ------------------------------------------------------------------------------------------------
# 3. a 0/1 mask is the protocol with those rows deleted
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("csf", [False, True])
@pytest.mark.parametrize("K", [2, 1])
def test_mask_equals_the_protocol_with_the_rows_deleted(K, csf):
    """the weighted call on the full plan against the unweighted call on plan_for(sch[keep]) with y[keep]: within the sum
    of the two referees' bars (they differ in M only).  The mask keeps a b0 row and most of the others."""
    from microstructure_fingerprinting_amd import engine
    kind = "c2"
    peaks, Y, _ = _case(kind)
    V, M = Y.shape
    sch = TP._sch(kind)
    rng = np.random.default_rng(4200)
    keep = rng.random(M) > 0.25
    b0 = np.flatnonzero(sch[:, 3] == 0)
    keep[b0[0]] = True
    assert keep[b0].sum() >= 1 and K + int(csf) + 2 <= keep.sum() < M
    rows = np.flatnonzero(keep)
    mask = keep.astype(np.float64)
    model = TP._model(kind)
    plan_d = model.ms_interpolator.plan_for(np.ascontiguousarray(sch[rows]))
    x = TP._sig_csf(kind) if csf else None
    xd = np.ascontiguousarray(x[rows]) if csf else None
    pk = np.ascontiguousarray(peaks[:, :3 * K])
    Kv, cv = np.full(V, K), np.full(V, csf)
    fw = [_F(kind, Y[v], mask, peaks[v], K, csf) for v in range(V)]
    fd = [_F(kind, Y[v], mask, peaks[v], K, csf, rows=rows) for v in range(V)]
    shift = np.array([float(f["F"].min()) for f in fd])
    Yd = np.ascontiguousarray(Y[:, rows])
    a = engine.posterior(TP._plan(kind), Y, Kv, cv, pk, K, csf, x, SIGMA, shift=shift, W=mask)
    b = engine.posterior(plan_d, Yd, Kv, cv, pk, K, csf, xd, SIGMA, shift=shift)
    oa = engine.profile(TP._plan(kind), Y, Kv, cv, pk, K, csf, x, W=mask)[0]
    ob = engine.profile(plan_d, Yd, Kv, cv, pk, K, csf, xd)[0]
    T = 2.0 * SIGMA ** 2
    for v in range(V):
        assert fw[v]["clear"] and fd[v]["clear"], "a pair near the cut: this input was chosen to have none"
        assert a[2][v] == 0 and b[2][v] == 0
        rw, rd = _post_ref(fw[v], T), _post_ref(fd[v], T)
        worst = 0.0
        for k in range(K):
            bar = rw["bar_w"][k] + rd["bar_w"][k]
            worst = max(worst, float(np.max(np.abs(a[0][v, k].astype(LD) - b[0][v, k].astype(LD)) / bar)))
        worst = max(worst, float(abs(LD(a[1][v]) - LD(b[1][v])) / (rw["bar_log_sum"] + rd["bar_log_sum"])))
        pbar = _prof_bar(fw[v]) + _prof_bar(fd[v])
        po = float(np.max(np.abs(oa[v, :K] - ob[v, :K]))) / pbar
        print("voxel %d K=%d csf=%d (%d of %d rows kept): posterior %.3g, profile %.3g of the summed bars" % (v, K, csf, rows.size, M, worst, po))
        assert worst <= 1.0 and po <= 1.0
        # and each against its own referee
        assert _post_ratio(a[0][v], a[1][v], rw, K) <= 1.0 and _post_ratio(b[0][v], b[1][v], rd, K) <= 1.0


# ------------------------------------------------------------------------------------------------
# 4. status codes and launch independence
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,csf", [(2, False), (2, True), (1, False)])
def test_unusable_weights_are_flagged_and_the_neighbours_untouched(K, csf):
    from microstructure_fingerprinting_amd import engine
    kind = "c2"
    peaks, Y, W = _case(kind)
    N = 48
    order = [0, 1, 2, 0, 1, 2, 0]
    Y7, pk7, W7 = np.ascontiguousarray(Y[order]), np.ascontiguousarray(peaks[order, :3 * K]), np.ascontiguousarray(W[order])
    W7[1, 7], W7[2, 0], W7[4, Y.shape[1] // 2] = -1e-300, np.nan, np.inf
    W7[5] = 0.0
    plan, x = TP._plan(kind), (TP._sig_csf(kind) if csf else None)
    good = [0, 3, 6]
    shift7 = np.array([float(_F(kind, Y[v], W[v], peaks[v], K, csf)["F"].min()) for v in order])
    run = lambda ix: (engine.posterior(plan, Y7[ix], np.full(len(ix), K), np.full(len(ix), csf), pk7[ix], K, csf, x, SIGMA,   # noqa: E731
                                       shift=shift7[ix], W=W7[ix]),
                      engine.profile(plan, Y7[ix], np.full(len(ix), K), np.full(len(ix), csf), pk7[ix], K, csf, x, partner=True, W=W7[ix]))
    (w, ls, st, n), (obj, par, _) = run(np.arange(7))
    (wg, lg, sg, _), (og, pg, _) = run(np.array(good))
    print("K=%d csf=%d: status %s" % (K, csf, st))
    assert n == 0 and np.array_equal(st, [0, 3, 3, 0, 3, 4, 0]) and (sg == 0).all()
    bad = st != 0
    assert np.isnan(w[bad]).all() and np.isnan(ls[bad]).all() and np.isnan(obj[bad]).all() and (par[bad] == -1).all()
    assert np.isfinite(w[good]).all() and w.shape == (7, K, N)
    for p, q in ((w, wg), (ls, lg), (obj, og), (par, pg)):
        assert np.array_equal(p[good], q), "a neighbour of an unusable voxel differs from the run without it"
    # the default shift (the weighted fit's objective) leaves the codes as they are
    st2 = engine.posterior(plan, Y7, np.full(7, K), np.full(7, csf), pk7, K, csf, x, SIGMA, W=W7)[2]
    assert np.array_equal(st2, st)
    if K == 2:
        land = engine.pair_objectives(plan, Y7, pk7, csf, x, W=W7)
        assert np.isnan(land[bad]).all() and np.isfinite(land[good]).all()
        assert np.array_equal(land[good], engine.pair_objectives(plan, Y7[good], pk7[good], csf, x, W=W7[good]))
    # a shared vector with a bad entry flags every voxel; status 1 (the temperature) comes first
    assert (engine.posterior(plan, Y7, np.full(7, K), np.full(7, csf), pk7, K, csf, x, SIGMA, shift=shift7, W=W7[1])[2] == 3).all()
    sig = np.full(7, SIGMA)
    sig[5] = 0.0
    assert engine.posterior(plan, Y7, np.full(7, K), np.full(7, csf), pk7, K, csf, x, sig, shift=shift7, W=W7)[2][5] == 1


# ------------------------------------------------------------------------------------------------
# 5. scaling
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,csf", [(2, False), (2, True), (1, True)])
def test_scaling_weights_temperature_and_shift_together(K, csf):
    """(4 W, 4 T, 4 shift): s doubles exactly, so every product scales by a power of two; within 2 x the bar"""
    from microstructure_fingerprinting_amd import _lib as L
    kind = "synth300"
    peaks, Y, W = _case(kind)
    V, N = Y.shape[0], 300
    plan, x = TP._plan(kind), (TP._sig_csf(kind) if csf else None)
    pk = np.ascontiguousarray(peaks[:, :3 * K])
    fs = [_F(kind, Y[v], W[v], peaks[v], K, csf) for v in range(V)]
    T = np.full(V, 2.0 * SIGMA ** 2)
    shift = np.array([float(f["F"].min()) for f in fs])
    out = []
    for c in (1.0, 4.0):
        w, ls, st = np.zeros((V, K, N)), np.zeros(V), np.zeros(V, dtype=np.int32)
        Wc, Tc, sc = np.ascontiguousarray(c * W), np.ascontiguousarray(c * T), np.ascontiguousarray(c * shift)
        L.check(L.lib().mfx_wpost(plan.handle(), L.dptr(Y), L.dptr(Wc), Y.shape[1], L.dptr(pk), K, int(csf), L.dptr(x) if csf else None,
                                  L.dptr(Tc), L.dptr(sc), V, L.dptr(w), L.dptr(ls), L.iptr(st)))
        assert (st == 0).all()
        out.append((w, ls))
    for v in range(V):
        assert fs[v]["clear"], "a pair near the cut: this input was chosen to have none"
        ref = _post_ref(fs[v], T[v])
        r = max(float(np.max(np.abs(out[0][0][v, k].astype(LD) - out[1][0][v, k].astype(LD)) / (2 * ref["bar_w"][k]))) for k in range(K))
        r = max(r, float(abs(LD(out[0][1][v]) - LD(out[1][1][v])) / (2 * ref["bar_log_sum"])))
        print("voxel %d K=%d csf=%d: (4 W, 4 T, 4 shift) against (W, T, shift): %.3g of twice the bar; identical: %s"
              % (v, K, csf, r, np.array_equal(out[0][0][v], out[1][0][v])))
        assert r <= 1.0


# ------------------------------------------------------------------------------------------------
# 6. end to end: the robust refit, then the soft answers and the landscape of that fit
# ------------------------------------------------------------------------------------------------
def test_robust_refit_then_posterior_interval_and_profile():
    from microstructure_fingerprinting_amd import synth
    from microstructure_fingerprinting_amd import mf_utils as U
    import microstructure_fingerprinting_amd.mf as mfmod
    kind = "small"      # the dictionary with EAR entries that make_phantom needs; the weighted fit takes none (p_ear = 0)
    model = TP._model(kind)
    rng = np.random.default_rng(77)
    ph = synth.make_phantom(model, (9, 8, 7), rng, p_ear=0.0)
    sch = np.ascontiguousarray(model.dic["sch_mat"], dtype=np.float64)
    N, M = int(model.dic["num_atom"]), sch.shape[0]
    roi = np.flatnonzero(ph["mask"].reshape(-1))
    R_ = roi.size
    # planted outliers: 6 measurements of every third ROI voxel
    data = np.ascontiguousarray(ph["data"], dtype=np.float64)
    rows = data.reshape(-1, M)
    assert np.shares_memory(rows, data)
    hit = roi[::3]
    for v in hit:
        rows[v, rng.choice(M, 6, replace=False)] += 400.0
    kw = dict(peaks=ph["peaks"], pgse_scheme=sch, csf_mask=ph["csf_mask"], verbose=0)
    fit0 = model.fit(data, ph["mask"], ph["numfasc"], **kw)
    r = fit0.residuals(data)
    W = np.abs(r) <= 4.45 * np.median(np.abs(r), axis=-1, keepdims=True)
    W[ph["mask"] == 0] = True
    fit = model.fit(data, ph["mask"], ph["numfasc"], weights=W, **kw)
    Wr = np.asarray(fit.weights_roi, dtype=np.float64)
    K = ph["numfasc"].reshape(-1)[roi].astype(int)
    csf = ph["csf_mask"].reshape(-1)[roi] > 0
    pk = ph["peaks"].reshape(-1, 6)[roi]
    Yr = np.ascontiguousarray(rows[roi])
    scope = K >= 1
    dropped = M - Wr.sum(axis=1)
    print("phantom: %d ROI voxels (%d with planted outliers), %d in scope; rows dropped per voxel: mean %.2f, max %d"
          % (R_, hit.size, int(scope.sum()), dropped.mean(), int(dropped.max())))
    assert 200 <= R_ <= 400 and dropped.max() >= 6
    # profile: its minimum is the weighted fit's objective
    prof = fit.profile(data, partner=True)
    assert prof.obj.shape == (R_, 2, N) and prof.n_unsupported == int((~scope).sum())
    sse = fit.params_in_mask[:, -2] * Wr.sum(axis=1)
    worst = 0.0
    for v in np.flatnonzero(scope):
        mn = prof.obj[v, 0].min()
        bar = _prof_bar(_F(kind, Yr[v], Wr[v], pk[v], int(K[v]), bool(csf[v])))
        worst = max(worst, abs(mn - sse[v]) / bar)
        assert abs(mn - sse[v]) <= bar, "voxel %d: min of the profile %.17g, MSE * sum W %.17g, bar %.3g" % (v, mn, sse[v], bar)
        if K[v] == 2:
            assert abs(prof.obj[v, 1].min() - mn) <= bar
    print("min of the weighted profile against MSE * sum W: worst %.3g of the bar over %d voxels" % (worst, int(scope.sum())))
    first = np.arange(R_)[::3][:8]      # voxels with planted outliers: the unweighted landscape is another one
    assert not np.allclose(fit0.profile(data, voxels=first).obj, prof.obj[first], equal_nan=True)
    # posterior: status counts, the sub-selection, the cold limit
    post = fit.posterior(data)
    counts = {int(s): int((post.status == s).sum()) for s in np.unique(post.status)}
    print("posterior status counts: %s" % counts)
    assert post.n_unsupported == int((~scope).sum()) and (post.status[scope] == 0).all() and (post.status[~scope] == -1).all()
    sub = fit.posterior(data, voxels=[5, 2, 11])
    assert np.array_equal(sub.weights, post.weights[[5, 2, 11]], equal_nan=True) and np.array_equal(sub.status, post.status[[5, 2, 11]])
    le = post.log_evidence()
    npos = (Wr > 0).sum(axis=1)
    T = 2.0 * sse / (npos - K - csf)
    ok = post.status == 0
    assert np.allclose(le[ok], (post.log_sum - K * np.log(N) - 0.5 * npos * np.log(np.pi * T))[ok], rtol=1e-13) and np.isnan(le[~ok]).all()
    ids = fit.params_in_mask[:, 3:5].astype(int)
    nu = fit.params_in_mask[:, 1:3]
    cold, ncold = fit.posterior(data, sigma=1e-3 * np.sqrt(np.maximum(sse, 1e-300) / M)), 0
    for v in np.flatnonzero(scope & (cold.status == 0)):
        for k in range(int(K[v])):
            if nu[v, k] > 0:    # a fascicle the fit gave no weight to has no fitted atom
                top = np.sort(prof.obj[v, k])[:2]
                if top[1] - top[0] > 1e-6 * sse[v]:      # a distinct optimum: the arg-max is the fitted atom
                    assert cold.weights[v, k].argmax() == ids[v, k], "voxel %d fascicle %d" % (v, k)
                    ncold += 1
    print("cold limit: the arg-max atom is the fitted one in all %d (voxel, fascicle) pairs with a distinct optimum" % ncold)
    assert ncold >= scope.sum() // 2
    # posterior_moments and interval run their chunked device loops with the voxels' weight rows
    old = mfmod.MFModelFit.PROFILE_BYTES
    mfmod.MFModelFit.PROFILE_BYTES = 16 * N * 50
    try:
        vals = np.asarray(model.dic["rad"], dtype=np.float64).reshape(-1)
        mean, std = fit.posterior_moments(data, "rad")
        rm, rs = U.posterior_moments(post.weights, vals)
        gm = mean.reshape(-1, 2)[roi]
        assert np.array_equal(np.isnan(gm), np.isnan(rm))
        have = ~np.isnan(rm)
        assert np.max(np.abs(gm[have] - rm[have]) / np.abs(rm[have])) <= 1e-12
        lo, hi, cnt = fit.interval(data, "rad", rel=0.05)
        l, h, n = (a.reshape(-1, 2)[roi] for a in (lo, hi, cnt))
        for v in np.flatnonzero(scope)[::7]:
            for k in range(int(K[v])):
                sel = prof.obj[v, k] <= prof.obj[v, k].min() * 1.05
                assert n[v, k] == sel.sum() and l[v, k] == vals[sel].min() and h[v, k] == vals[sel].max()
    finally:
        mfmod.MFModelFit.PROFILE_BYTES = old
    # the shared [M] form goes through the same calls
    w1 = np.ones(M)
    w1[::11] = 0.0
    fit1 = model.fit(data, ph["mask"], ph["numfasc"], weights=w1, **kw)
    five = np.flatnonzero(scope)[:5]
    p1 = fit1.profile(data, voxels=five)
    for q, v in enumerate(five):
        bar = _prof_bar(_F(kind, Yr[v], w1, pk[v], int(K[v]), bool(csf[v])))
        assert abs(p1.obj[q, 0].min() - fit1.params_in_mask[v, -2] * w1.sum()) <= bar
    m1, _ = fit1.posterior_moments(data, "rad")
    assert np.isfinite(m1.reshape(-1, 2)[roi][scope, 0]).all()


# ------------------------------------------------------------------------------------------------
# 7. the _dev entry points only enqueue
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,csf", [(2, False), (1, True)])
def test_dev_entry_points_enqueue_on_the_callers_stream(K, csf):
    import torch
    from microstructure_fingerprinting_amd import engine
    kind = "synth300"
    peaks, Y, W = _case(kind)
    V = Y.shape[0]
    plan, x = TP._plan(kind), (TP._sig_csf(kind) if csf else None)
    pk = np.ascontiguousarray(peaks[:, :3 * K])
    Kv, cv = np.full(V, K), np.full(V, csf)
    shift = np.array([float(_F(kind, Y[v], W[v], peaks[v], K, csf)["F"].min()) for v in range(V)])
    host = engine.posterior(plan, Y, Kv, cv, pk, K, csf, x, SIGMA, shift=shift, W=W)
    hprof = engine.profile(plan, Y, Kv, cv, pk, K, csf, x, partner=True, W=W)
    hland = engine.pair_objectives(plan, Y, pk, csf, x, W=W) if K == 2 else None
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()   # noqa: E731
    dY, dW, dp, dT, dsh = t(Y), t(W), t(pk), t(np.full(V, 2.0 * SIGMA ** 2)), t(shift)
    dx = t(x) if csf else None
    big = torch.ones((4096, 4096), dtype=torch.float64, device="cuda")
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        for _ in range(40):                      # work ahead of the calls on their stream
            big2 = big @ big
        w, ls, st = engine.posterior_dev(plan, dY, dp, K, dT, dsh, csf, dx, d_W=dW)
        obj, par = engine.profile_dev(plan, dY, dp, K, csf, dx, partner=True, d_W=dW)
        land = engine.pair_objectives_dev(plan, dY, dp, csf, dx, d_W=dW) if K == 2 else None
        pending = not s.query()                  # the calls came back with the stream still busy
    torch.cuda.synchronize()
    del big2
    assert pending, "a _dev entry point waited for its stream"
    assert np.array_equal(w.cpu().numpy(), host[0]) and np.array_equal(ls.cpu().numpy(), host[1]) and np.array_equal(st.cpu().numpy(), host[2])
    assert np.array_equal(obj.cpu().numpy(), hprof[0]) and np.array_equal(par.cpu().numpy(), hprof[1])
    if K == 2:
        assert np.array_equal(land.cpu().numpy(), hland)
    # the shared vector on the device
    w1, _, st1 = engine.posterior_dev(plan, dY, dp, K, dT, dsh, csf, dx, d_W=t(W[0]))
    torch.cuda.synchronize()
    assert np.array_equal(w1.cpu().numpy()[0], host[0][0]) and (st1.cpu().numpy()[0] == 0)
