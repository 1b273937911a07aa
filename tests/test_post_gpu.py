"""Soft fits on the GPU: engine.posterior / posterior_dev, MFModelFit.posterior / posterior_moments.

The referee and the bar are those of tests/_post_ref.py: the value of every atom pair restated in long double from the
oracle's rotation (without CSF the two-variable closed form, with CSF all eight supports), the kernel's cut applied,
long-double exp with the shift at the referee's own minimum; a weight may differ by 2 (E_k[i] + w_ref E) +
(N^2 + 4096) eps and log_sum by 2 E + (N^2 + 4096) eps, E the sums of t_ref expm1(B / T) / Z_ref with
B = 16 M eps ||y||^2 / (1 - c^2) per pair.  Each comparison asserts as a condition on its inputs that no pair has
1 - c^2 within [cut / 4, 4 cut].

Each test prints what it measures before it asserts; the figures seen on the MI355X are in DESIGN.md 4.15.
"""
import numpy as np
import pytest

import _post_ref as R
from _post_ref import TP

pytestmark = pytest.mark.gpu

EPS = R.EPS
SIGMA = 500.0 / 30.0      # the synthetic voxels' noise: M0 / SNR of synth.make_voxels
_refs = {}


def _T(sigma):
    return 2.0 * float(sigma) ** 2


def _ref(tag, kind, y, pk, csf, T):
    """the referee of one voxel, computed once per (tag, csf, T)"""
    key = (tag, bool(csf), float(T))
    if key not in _refs:
        _refs[key] = R.voxel(kind, y, pk, csf, T, TP._cut())
    return _refs[key]


def _compare(tag, kind, Y, peaks, csf, sigma, w, log_sum, status):
    """every voxel of a two-fascicle set against the referee; returns the worst error / bar"""
    worst = 0.0
    sig = np.broadcast_to(np.asarray(sigma, dtype=np.float64), (Y.shape[0],))
    for v in range(Y.shape[0]):
        ref = _ref("%s/%d" % (tag, v), kind, Y[v], peaks[v], csf, _T(sig[v]))
        assert ref["clear"], "%s voxel %d: a pair near the cut: this input was chosen to have none" % (tag, v)
        ratio = R.worst_ratio(w[v], log_sum[v], ref)
        worst = max(worst, ratio)
        print("%s csf=%d voxel %d: worst |got - referee| / bar = %.3g (bars on weights %.3g .. %.3g, on log_sum %.3g; log_sum "
              "%.6f; %.0f effective pairs, %d pairs under the cut, smallest 1 - c^2 above it %.3g)"
              % (tag, csf, v, ratio, float(min(ref["bar_w"][0].min(), ref["bar_w"][1].min())),
                 float(max(ref["bar_w"][0].max(), ref["bar_w"][1].max())), float(ref["bar_log_sum"]), float(log_sum[v]),
                 ref["neff"], ref["ncut"], ref["c2min"]))
        assert status[v] == 0
        assert ratio <= 1.0, "%s voxel %d: %.3g of the bar" % (tag, v, ratio)
    return worst


def _run2(kind, Y, peaks, csf, sigma, shift=None):
    from microstructure_fingerprinting_amd import engine
    V = Y.shape[0]
    return engine.posterior(TP._plan(kind), Y, np.full(V, 2), np.full(V, csf), peaks, 2, csf, TP._sig_csf(kind) if csf else None,
                            sigma, shift=shift)


# ------------------------------------------------------------------------------------------------
# 1. the mixed set of fit_cases (14 atoms: less than one tile)
# ------------------------------------------------------------------------------------------------
def test_mixed_set_of_fit_cases():
    """K = 1 and K = 2, with and without CSF, EAR voxels and voxels without a fascicle through engine.posterior: the
    binning (every class against a call of its own on the device entry point), NaN rows and the count of the voxels out
    of scope, weights of each present fascicle summing to 1 within N eps; one-fascicle weights against the soft-min of
    the profile's values (obj = F for K = 1) within 4 w expm1(B / T) + (N^2 + 4096) eps, B = 16 M eps ||y||^2."""
    import torch
    from microstructure_fingerprinting_amd import engine
    d = TP._load("fit_cases")
    Y = np.ascontiguousarray(d["Y"])
    V, M = Y.shape
    K, csf, ear = d["numfasc"].astype(int), d["csf"] > 0, d["ear"] > 0
    peaks = np.ascontiguousarray(d["peaks"][:, :6])
    plan, x = TP._plan("small"), TP._sig_csf("small")
    N = 14
    rng = np.random.default_rng(3)
    sigma = rng.uniform(10.0, 25.0, V)
    w, ls, st, n_uns = engine.posterior(plan, Y, K, csf, peaks, 2, True, x, sigma, ear=ear)
    scope = (K >= 1) & (K <= 2) & ~ear
    print("fit_cases: %d voxels, %d out of scope; classes (K, csf): %s" % (V, int((~scope).sum()),
          sorted(set(zip(K[scope].tolist(), csf[scope].tolist())))))
    assert w.shape == (V, 2, N) and n_uns == int((~scope).sum()) and 0 < n_uns < V
    assert np.isnan(w[~scope]).all() and np.isnan(ls[~scope]).all() and (st[~scope] == -1).all()
    assert (st[scope] == 0).all() and np.isfinite(ls[scope]).all()
    for v in np.flatnonzero(scope):
        k = int(K[v])
        assert np.isnan(w[v, k:]).all() and np.isfinite(w[v, :k]).all() and (w[v, :k] >= 0).all()
        dev = np.abs(w[v, :k].sum(axis=1) - 1.0).max()
        assert dev <= N * EPS, "voxel %d: weights sum to 1 + %.3g" % (v, dev)
    print("largest |sum of a fascicle's weights - 1| = %.3g (N eps = %.3g)"
          % (max(np.abs(w[v, :int(K[v])].sum(axis=1) - 1.0).max() for v in np.flatnonzero(scope)), N * EPS))
    # every class on its own through the device entry point, shift from the fit as engine.posterior takes it
    dev_ = torch.device("cuda", 0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev_)   # noqa: E731
    seen = set()
    for k in (1, 2):
        for c in (False, True):
            ix = np.flatnonzero(scope & (K == k) & (csf == c))
            if not ix.size:
                continue
            seen.add((k, c))
            fit = engine.fit_batch(plan, Y[ix], np.full(ix.size, k), np.full(ix.size, c), None, peaks[ix, :3 * k], k, c, False,
                                   x if c else None)
            wd, ld, sd = engine.posterior_dev(plan, t(Y[ix]), t(peaks[ix, :3 * k]), k, t(2.0 * sigma[ix] ** 2), t(fit[:, -2] * M),
                                              c, t(x) if c else None)
            assert np.array_equal(wd.cpu().numpy(), w[ix, :k]) and np.array_equal(ld.cpu().numpy(), ls[ix])
            assert (sd.cpu().numpy() == 0).all()
    assert len(seen) == 4
    # one fascicle: the profile's values are F itself
    obj, _, _ = engine.profile(plan, Y, K, csf, peaks, 2, True, x, ear=ear)
    worst = 0.0
    for v in np.flatnonzero(scope & (K == 1) & ~csf):
        T = R.LD(_T(sigma[v]))
        F = obj[v, 0].astype(R.LD)
        tt = np.exp(-(F - F.min()) / T)
        wr, lr = tt / tt.sum(), np.log(tt.sum()) - F.min() / T
        rel = np.expm1(16 * M * EPS * R.LD(Y[v] @ Y[v]) / T)
        tail = (N * N + 4096) * EPS
        ratio = max(float(np.max(np.abs(w[v, 0] - wr) / (4 * wr * rel + tail))), float(abs(ls[v] - lr) / (2 * rel + tail)))
        worst = max(worst, ratio)
        assert ratio <= 1.0, "voxel %d: %.3g of the bar" % (v, ratio)
    print("one fascicle against the soft-min of the profile: worst error / bar = %.3g" % worst)


# ------------------------------------------------------------------------------------------------
# 2. fit_c2_small: every voxel against the referee, and the cold limit against the reference's fit
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("csf", [False, True])
def test_fit_c2_small_against_the_referee(csf):
    d = TP._load("fit_c2_small")
    Y, peaks = np.ascontiguousarray(d["Y"]), np.ascontiguousarray(d["peaks"])
    sigma = d["map_M0"] / 30.0
    w, ls, st, n = _run2("c2", Y, peaks, csf, sigma)
    assert n == 0
    worst = _compare("c2", "c2", Y, peaks, csf, sigma, w, ls, st)
    print("fit_c2_small csf=%d: worst error / bar over %d voxels = %.3g" % (csf, Y.shape[0], worst))


def test_fit_c2_small_cold_limit_finds_the_fitted_atoms():
    """T = gap / 50 (gap: the referee's distance of the two smallest pair values): the sum is its largest term, and the
    arg-max of each fascicle's weights is the atom the reference fitted (golden file), with a weight above 0.999."""
    d = TP._load("fit_c2_small")
    Y, peaks = np.ascontiguousarray(d["Y"]), np.ascontiguousarray(d["peaks"])
    V = Y.shape[0]
    refs = [_ref("c2/%d" % v, "c2", Y[v], peaks[v], False, _T(d["map_M0"][v] / 30.0)) for v in range(V)]
    gap = np.array([r["gap"] for r in refs])
    ysq = np.array([r["ysq"] for r in refs])
    print("gap / ||y||^2 = %s" % np.array2string(gap / ysq, precision=3))
    assert np.all(gap > 1e-8 * ysq), "an input without a distinct optimum"
    w, ls, st, _ = _run2("c2", Y, peaks, False, np.sqrt(gap / 50.0 / 2.0))
    assert (st == 0).all()
    for k in range(2):
        best = w[:, k].argmax(axis=1)
        print("fascicle %d: arg-max atoms %s, their weights %s" % (k, best, np.array2string(w[np.arange(V), k, best], precision=6)))
        assert np.array_equal(d["rad"][best], d["map_rad_f%d" % k]) and np.array_equal(d["fin"][best], d["map_fin_f%d" % k])
        assert np.all(w[np.arange(V), k, best] > 0.999)
        for v in range(V):   # the referee's minimiser is that atom too
            i, j = np.unravel_index(np.argmin(refs[v]["F"]), refs[v]["F"].shape)
            assert best[v] == (i, j)[k]


# ------------------------------------------------------------------------------------------------
# 3. / 4. synthetic dictionaries: 300 atoms (a last sweep with partly idle waves), 782 atoms (the benchmark's shape)
# ------------------------------------------------------------------------------------------------
def _six_voxels(csf):
    """four ordinary voxels, one with d_1 = d_0 (diagonal pairs under the cut), one fitted at a quarter of its noise"""
    kind = "synth300"
    peaks, Y = TP._synth_voxels(kind, 6, 2, seed=909)
    peaks, Y = peaks.copy(), Y.copy()
    rng = np.random.default_rng(910)
    D0 = TP._rot(kind, peaks[4, :3])
    peaks[4, 3:] = peaks[4, :3]
    Y[4] = 300.0 * D0[:, 17] + 200.0 * D0[:, 140] + rng.normal(0, SIGMA, D0.shape[0])
    if csf:      # voxels with and without CSF signal: both signs of w_x
        x = TP._sig_csf(kind)
        Y[[0, 1, 4]] += 150.0 * x[None, :]
    sigma = np.full(6, SIGMA)
    sigma[5] = SIGMA / 4
    return kind, np.ascontiguousarray(peaks), np.ascontiguousarray(Y), sigma


@pytest.mark.parametrize("csf", [False, True])
def test_300_atoms_against_the_referee(csf):
    """300 = 18 tiles + 12 atoms: the last tile is partly padding and the last sweep has idle waves."""
    kind, peaks, Y, sigma = _six_voxels(csf)
    w, ls, st, n = _run2(kind, Y, peaks, csf, sigma)
    assert n == 0 and w.shape == (6, 2, 300)
    worst = _compare("synth300", kind, Y, peaks, csf, sigma, w, ls, st)
    ref4 = _ref("synth300/4", kind, Y[4], peaks[4], csf, _T(sigma[4]))
    assert ref4["ncut"] >= 300, "the voxel with d_1 = d_0 should have its diagonal under the cut"
    neff = [_ref("synth300/%d" % v, kind, Y[v], peaks[v], csf, _T(sigma[v]))["neff"] for v in range(6)]
    print("synthetic N = 300 csf=%d: worst error / bar = %.3g; effective pairs per voxel %s" % (csf, worst, np.round(neff, 1)))
    assert neff[5] < min(neff[:4]), "a quarter of the noise should concentrate the sum"
    if csf:
        # both branches of the sign of w_x were taken: the CSF value differs from the plain one for some pairs only
        plain = R.voxel(kind, Y[2], peaks[2], False, _T(sigma[2]), TP._cut())["F"]
        same = np.mean(np.abs(plain - _ref("synth300/2", kind, Y[2], peaks[2], True, _T(sigma[2]))["F"]) <= 1e-9 * plain)
        print("voxel 2 (no CSF signal): %.1f %% of the pairs have w_x = 0" % (100 * same))
        assert 0.01 < same < 0.99


@pytest.mark.parametrize("csf", [False, True])
def test_782_atoms_against_the_referee(csf):
    """the benchmark's instantiation: 49 tiles, the seventh sweep of the 8-wave form has one valid wave"""
    peaks, Y = TP._synth_voxels("synth", 2, 2, seed=911)
    w, ls, st, n = _run2("synth", Y, peaks, csf, SIGMA)
    assert n == 0 and w.shape == (2, 2, 782)
    worst = _compare("synth782", "synth", Y, peaks, csf, SIGMA, w, ls, st)
    print("synthetic N = 782 csf=%d: worst error / bar = %.3g" % (csf, worst))


# ------------------------------------------------------------------------------------------------
# 5. G-bracketed rows (the UKBB fixture), 6. a 302-row protocol
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("csf", [False, True])
def test_ukbb_bracketed_rows_against_the_referee(csf):
    d = TP._load("real_ukbb_fit_k2")
    peaks, Y = np.ascontiguousarray(d["peaks"][:2, :6]), np.ascontiguousarray(d["Y"][:2])
    M = Y.shape[1]
    # the noise level from the referee's own minimum: sigma^2 = min F / (M - 2)
    sigma = np.array([np.sqrt(_ref("ukbb/%d" % v, "ukbb", Y[v], peaks[v], False, 1.0)["Fmin"] / (M - 2)) for v in range(2)])
    w, ls, st, n = _run2("ukbb", Y, peaks, csf, sigma)
    assert n == 0 and w.shape == (2, 2, 986)
    worst = _compare("ukbb", "ukbb", Y, peaks, csf, sigma, w, ls, st)
    print("UKBB (986 atoms, %d bracketed rows) csf=%d: worst error / bar = %.3g" % (M, csf, worst))


def _long_model():
    """2 b0 + 3 x 100 directions, 64 atoms: the KSTEPS = 140 instantiation"""
    import microstructure_fingerprinting_amd as mf
    from microstructure_fingerprinting_amd import synth
    if "long302" not in TP._cache:
        rng = np.random.default_rng(21)
        sch = synth.make_scheme(rng, 2, [1000, 2000, 3000], [100, 100, 100])
        dic = synth.make_dictionary(rng, sch, 64)
        md = {"dictionary": dic, "sch_mat": sch, "num_atom": 64, "num_ear": 0, "T2_csf": 2.0, "DIFF_csf": 3.0e-9, "T2_ear": 0.08,
              "DIFF_ear": np.zeros(0), "rad": np.round(rng.uniform(0.2, 2.0, 64), 1) * 1e-6,
              "fin": np.round(rng.uniform(0.3, 0.9, 64), 1), "orientation": TP.Z, "fasc_propnames": ["rad", "fin"]}
        TP._cache["long302"] = mf.MFModel(md)
    return "long302"


@pytest.mark.parametrize("csf", [False, True])
def test_302_row_protocol_against_the_referee(csf):
    kind = _long_model()
    peaks, Y = TP._synth_voxels(kind, 2, 2, seed=912)
    assert Y.shape == (2, 302)
    w, ls, st, n = _run2(kind, Y, peaks, csf, SIGMA)
    assert n == 0 and w.shape == (2, 2, 64)
    worst = _compare("long302", kind, Y, peaks, csf, SIGMA, w, ls, st)
    print("302 rows, 64 atoms csf=%d: worst error / bar = %.3g" % (csf, worst))


# ------------------------------------------------------------------------------------------------
# 7. launch independence
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,csf", [(2, False), (2, True), (1, False)])
def test_launch_independence(K, csf):
    """five voxels in one call equal five single-voxel calls bit for bit; two runs are bit-identical"""
    import torch
    from microstructure_fingerprinting_amd import engine
    kind = "synth300"
    peaks, Y = TP._synth_voxels(kind, 5, K, seed=913)
    plan = TP._plan(kind)
    dev = torch.device("cuda", 0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)   # noqa: E731
    d_x = t(TP._sig_csf(kind)) if csf else None
    T, sh = t(np.full(5, _T(SIGMA))), t(np.full(5, Y.shape[1] * SIGMA ** 2))   # the shift: the expected residual
    run = lambda sl: [o.cpu().numpy() for o in engine.posterior_dev(plan, t(Y[sl]), t(peaks[sl]), K, T[sl].contiguous(),   # noqa: E731
                                                                     sh[sl].contiguous(), csf, d_x)]
    a, b = run(slice(0, 5)), run(slice(0, 5))
    assert (a[2] == 0).all() and np.isfinite(a[0]).all()
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    for v in range(5):
        one = run(slice(v, v + 1))
        for x, y in zip(a, one):
            assert np.array_equal(x[v:v + 1], y), "voxel %d differs between a call of five and a call of its own" % v


# ------------------------------------------------------------------------------------------------
# 8. shift and temperature
# ------------------------------------------------------------------------------------------------
def test_shift_cancels_and_bad_inputs_are_flagged():
    from microstructure_fingerprinting_amd import engine
    d = TP._load("fit_c2_small")
    Y, peaks = np.ascontiguousarray(d["Y"]), np.ascontiguousarray(d["peaks"])
    V, N = Y.shape[0], 48
    sigma = d["map_M0"] / 30.0
    T = 2.0 * sigma ** 2
    Fmin = np.array([_ref("c2/%d" % v, "c2", Y[v], peaks[v], False, T[v])["Fmin"] for v in range(V)])
    for off in (-500.0, 500.0):
        w, ls, st, _ = _run2("c2", Y, peaks, False, sigma, shift=Fmin + off * T)
        worst = _compare("c2", "c2", Y, peaks, False, sigma, w, ls, st)
        print("shift = min F %+g T: worst error / bar = %.3g" % (off, worst))
    good = _run2("c2", Y, peaks, False, sigma, shift=Fmin)
    # unusable temperatures and shifts: status 1, NaN rows, the neighbours untouched
    plan = TP._plan("c2")
    Tb, sb = T.copy(), Fmin.copy()
    Tb[1], Tb[3], sb[4] = 0.0, np.nan, np.inf
    w, ls, st = np.zeros((V, 2, N)), np.zeros(V), np.zeros(V, dtype=np.int32)
    from microstructure_fingerprinting_amd import _lib as L
    L.check(L.lib().mfx_post(plan.handle(), L.dptr(Y), L.dptr(peaks), 2, 0, None, L.dptr(Tb), L.dptr(sb), V, L.dptr(w), L.dptr(ls),
                             L.iptr(st)))
    print("status with T = 0, T = NaN, shift = inf at voxels 1, 3, 4: %s" % st)
    assert np.array_equal(st, [0, 1, 0, 1, 1, 0])
    bad = st != 0
    assert np.isnan(w[bad]).all() and np.isnan(ls[bad]).all()
    assert np.array_equal(w[~bad], good[0][~bad]) and np.array_equal(ls[~bad], good[1][~bad])
    # negative and infinite temperatures likewise (through engine.posterior sigma is squared: use the ABI)
    Tb = T.copy()
    Tb[0], Tb[5] = -1.0, np.inf
    L.check(L.lib().mfx_post(plan.handle(), L.dptr(Y), L.dptr(peaks), 2, 0, None, L.dptr(Tb), L.dptr(Fmin.copy()), V, L.dptr(w),
                             L.dptr(ls), L.iptr(st)))
    assert np.array_equal(st, [1, 0, 0, 0, 0, 1])
    # a shift far above the minimum: exponents above 700, status 2
    sh = Fmin.copy()
    sh[2] = Fmin[2] + 2000.0 * T[2]
    w, ls, st, _ = _run2("c2", Y, peaks, False, sigma, shift=sh)
    print("status with shift = min F + 2000 T at voxel 2: %s" % st)
    assert np.array_equal(st, [0, 0, 2, 0, 0, 0]) and np.isnan(w[2]).all() and np.isnan(ls[2])
    keep = np.arange(V) != 2
    assert np.array_equal(w[keep], good[0][keep]) and np.array_equal(ls[keep], good[1][keep])
    # a shift far below it: every term underflows, Z = 0, status 2; one fascicle takes the same checks
    sh[2] = Fmin[2] - 2000.0 * T[2]
    assert _run2("c2", Y, peaks, False, sigma, shift=sh)[2][2] == 2
    sh1 = engine.profile(plan, Y, np.ones(V, int), None, peaks[:, :3], 1, False, None)[0][:, 0].min(axis=1)   # min F, one fascicle
    sh1[1:4] = [np.nan, 1e300, -1e300]
    k1 = engine.posterior(plan, Y, np.ones(V, int), None, peaks[:, :3], 1, False, None, sigma, shift=sh1)
    print("one fascicle, shifts min F, NaN, 1e300, -1e300, min F, min F: status %s" % k1[2])
    assert np.array_equal(k1[2][:4], [0, 1, 2, 2]) and np.isnan(k1[0][1:4]).all() and np.isfinite(k1[0][[0, 4, 5]]).all()


# ------------------------------------------------------------------------------------------------
# 9. limits
# ------------------------------------------------------------------------------------------------
def test_limits_are_reported_and_held():
    """mfx_post_max_atoms is never below the profile's; a dictionary at the limit is served, one tile over it raises
    NotImplementedError with the limit in the message (M = 200 without CSF: the last configuration tried)."""
    import microstructure_fingerprinting_amd as mf
    from microstructure_fingerprinting_amd import _lib as L
    from microstructure_fingerprinting_amd import engine, synth
    lib = L.lib()
    for kind in ("synth", "ukbb", _long_model()):
        h = TP._plan(kind).handle()
        for c in (0, 1):
            n, npf = lib.mfx_post_max_atoms(h, c), lib.mfx_profile_max_atoms(h, c, 0)
            print("%s csf=%d: largest dictionary %d (profile: %d)" % (kind, c, n, npf))
            assert n >= npf > 0 and n % 16 == 0
    limit = lib.mfx_post_max_atoms(TP._plan("synth").handle(), 0)
    sch, dic, rng = synth.make_model("C2", N=limit + 16)
    y = 300.0 * dic[:, 5] + 200.0 * dic[:, 9]
    pk = np.array([[0.0, 0.0, 1.0, 0.0, 0.0, 1.0]])
    for N in (limit, limit + 16):
        md = {"dictionary": dic[:, :N], "sch_mat": sch, "num_atom": N, "num_ear": 0, "T2_csf": 2.0, "DIFF_csf": 3.0e-9,
              "T2_ear": 0.08, "DIFF_ear": np.zeros(0), "rad": np.ones(N), "fin": np.ones(N), "orientation": TP.Z,
              "fasc_propnames": ["rad", "fin"]}
        plan = mf.MFModel(md).ms_interpolator.plan_for(np.ascontiguousarray(sch))
        assert lib.mfx_post_max_atoms(plan.handle(), 0) == limit
        if N == limit:
            # the sum arrays lie at the top of the workgroup's LDS here.  The landscape mode of the profile reaches this
            # size (it keeps no column arrays): weights against the soft-min of its pair values on the host.  Both score
            # a pair alike, so what differs is the rounding of F = ||y||^2 - score and of the exponent's argument, each
            # eps ||y||^2 / T relative in t, in numerator and denominator: 4 eps (||y||^2 / T) w + (N^2 + 4096) eps
            assert lib.mfx_profile_max_atoms(plan.handle(), 0, 1) >= N
            w, ls, st, _ = engine.posterior(plan, y[None, :], np.array([2]), None, pk, 2, False, None, SIGMA, shift=np.zeros(1))
            assert st[0] == 0 and w.shape == (1, 2, N) and abs(w[0, 0].sum() - 1) < N * EPS and abs(w[0, 1].sum() - 1) < N * EPS
            F = engine.pair_objectives(plan, y[None, :], pk)[0].astype(R.LD)
            T = R.LD(_T(SIGMA))
            t = np.exp(-(F - F.min()) / T)
            rel = 4 * EPS * float(y @ y) / float(T)
            tail = (N * N + 4096) * EPS
            for k in range(2):
                wr = t.sum(1 - k) / t.sum()
                ratio = float(np.max(np.abs(w[0, k] - wr) / (rel * wr + tail)))
                print("N = %d (the limit), fascicle %d: worst |w - soft-min of the landscape| / bar = %.3g" % (N, k, ratio))
                assert ratio <= 1.0
            lr = np.log(t.sum()) - F.min() / T
            print("log_sum %.9f against %.9f" % (ls[0], float(lr)))
            assert abs(ls[0] - lr) <= rel + tail
        else:
            with pytest.raises(NotImplementedError, match=r"exceed the %d that fit" % limit):
                engine.posterior(plan, y[None, :], np.array([2]), None, pk, 2, False, None, SIGMA, shift=np.zeros(1))


# ------------------------------------------------------------------------------------------------
# 10. a mixed volume through MFModelFit.posterior / posterior_moments
# ------------------------------------------------------------------------------------------------
def test_posterior_over_a_mixed_phantom():
    from microstructure_fingerprinting_amd import synth
    from microstructure_fingerprinting_amd import mf_utils as U
    import microstructure_fingerprinting_amd.mf as mfmod
    model = TP._model("small")
    rng = np.random.default_rng(55)
    ph = synth.make_phantom(model, (7, 6, 5), rng)
    sch = np.ascontiguousarray(model.dic["sch_mat"], dtype=np.float64)
    fit = model.fit(ph["data"], ph["mask"], ph["numfasc"], peaks=ph["peaks"], pgse_scheme=sch, csf_mask=ph["csf_mask"],
                    ear_mask=ph["ear_mask"], verbose=0)
    N, M = int(model.dic["num_atom"]), sch.shape[0]
    roi = np.flatnonzero(ph["mask"].reshape(-1))
    R_ = roi.size
    K = ph["numfasc"].reshape(-1)[roi].astype(int)
    csf, ear = ph["csf_mask"].reshape(-1)[roi] > 0, ph["ear_mask"].reshape(-1)[roi] > 0
    scope = (K >= 1) & ~ear
    post = fit.posterior(ph["data"])
    assert post.weights.shape == (R_, 2, N) and post.n_unsupported == int((~scope).sum()) and 0 < post.n_unsupported < R_
    assert np.array_equal(post.voxels, np.arange(R_))
    assert (post.status[~scope] == -1).all() and np.isnan(post.weights[~scope]).all() and np.isnan(post.log_sum[~scope]).all()
    ok = post.status == 0
    print("phantom: %d ROI voxels, %d out of scope, status counts %s" % (R_, post.n_unsupported,
          {int(s): int((post.status == s).sum()) for s in np.unique(post.status)}))
    assert ok[scope].all()
    le = post.log_evidence()
    assert np.isfinite(le[ok]).all() and np.isnan(le[~ok]).all()
    mse = fit.params_in_mask[:, -2]
    T = np.where(ok, 2.0 * mse * M / (M - K - csf), 1.0)   # voxels out of scope: any positive value, not compared
    assert np.allclose(le[ok], (post.log_sum - K * np.log(N) - 0.5 * M * np.log(np.pi * T))[ok], rtol=1e-13)
    for v in np.flatnonzero(scope):
        k = int(K[v])
        assert np.isnan(post.weights[v, k:]).all() and np.all(np.abs(post.weights[v, :k].sum(axis=1) - 1.0) <= N * EPS)
    sub = fit.posterior(ph["data"], voxels=[5, 2, 11])
    assert np.array_equal(sub.weights, post.weights[[5, 2, 11]], equal_nan=True) and np.array_equal(sub.status, post.status[[5, 2, 11]])
    fixed = fit.posterior(ph["data"], sigma=20.0, voxels=np.flatnonzero(scope)[:4])
    assert (fixed.status == 0).all() and not np.array_equal(fixed.weights, post.weights[np.flatnonzero(scope)[:4]], equal_nan=True)
    old = mfmod.MFModelFit.PROFILE_BYTES
    mfmod.MFModelFit.PROFILE_BYTES = 16 * N * 7     # 7 voxels per chunk: several chunks per class
    try:
        for name in ("rad", "fin"):
            vals = np.asarray(model.dic[name], dtype=np.float64).reshape(-1)
            mean, std = fit.posterior_moments(ph["data"], name)
            assert mean.shape == ph["mask"].shape + (2,) and std.shape == mean.shape
            rm, rs = U.posterior_moments(post.weights, vals)
            assert np.array_equal(post.mean(name), rm, equal_nan=True) and np.array_equal(post.std(name), rs, equal_nan=True)
            flat = lambda a: a.reshape(-1, 2)[roi]   # noqa: E731
            gm, gs = flat(mean), flat(std)
            assert np.array_equal(np.isnan(gm), np.isnan(rm)) and np.array_equal(np.isnan(gs), np.isnan(rs))
            have = ~np.isnan(rm)
            dm = np.max(np.abs(gm[have] - rm[have]) / np.abs(rm[have]))
            # the standard deviation: 1e-12 relative wherever it is well conditioned, std > 1e-3 max|v|.  Below that floor
            # the posterior sits on one property value and std is a root of rounding-level terms: two summation orders
            # move the mean by some eps max|v|, hence every (v - mean) by that much and - by Cauchy-Schwarz,
            # sum w |v - mean| <= std - the standard deviation by the same absolute amount: 1e-12 max|v| there
            vmax = np.abs(vals).max()
            err, big = np.abs(gs[have] - rs[have]), rs[have] > 1e-3 * vmax
            ds = float(np.max(err[big] / rs[have][big])) if big.any() else 0.0
            dsmall = float(np.max(err[~big] / vmax)) if (~big).any() else 0.0
            print("posterior_moments(%s): device against host reduction: mean %.3g relative; std %.3g relative in %d rows above "
                  "the floor 1e-3 max|v|, %.3g of max|v| in the %d rows below it" % (name, dm, ds, int(big.sum()), dsmall, int((~big).sum())))
            assert big.any()
            assert dm <= 1e-12 and ds <= 1e-12 and dsmall <= 1e-12
            assert np.all(rm[have] >= vals.min()) and np.all(rm[have] <= vals.max()) and np.all(rs[have] >= 0)
            outside = np.setdiff1d(np.arange(ph["mask"].size), roi)
            assert np.all(np.isnan(mean.reshape(-1, 2)[outside])) and np.all(np.isnan(std.reshape(-1, 2)[outside]))
            assert np.all(np.isnan(gm[~scope])) and np.all(np.isnan(gm[scope & (K == 1), 1])) and not np.isnan(gm[scope, 0]).any()
            q10, q90 = post.quantile(name, 0.1), post.quantile(name, 0.9)
            assert np.all(q10[have] <= q90[have]) and np.all(np.isin(q10[have], vals))
            lv, by = post.by_property(name)
            assert by.shape == (R_, 2, lv.size) and np.allclose(by[have].sum(-1), 1.0, atol=N * EPS)
    finally:
        mfmod.MFModelFit.PROFILE_BYTES = old
    with pytest.raises(ValueError, match="unknown fascicle property"):
        post.mean("nope")
    with pytest.raises(ValueError, match="sigma should be a scalar"):
        fit.posterior(ph["data"], sigma=np.ones(3))
