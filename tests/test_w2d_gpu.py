"""Measurement weights for 2-D (AxCaliber-like) protocols on the GPU (include/mfx_w2d.h, csrc/w2d.hip):
engine.fit2d_weighted / posterior2d(W=) / profile2d(W=), their _dev forms, and RotateAtom2DTables.fit / .posterior /
.profile / .interval with weights=.

Referees (tests/_w2d_ref.py): the reference's own chain on sqrt(W)-scaled reference rotations
(tests/golden/wfit2d_cases.npz); for the fit the oracle's solver on sqrt(W) * T.rotate(dirs) with the weighted row
packing of tests/_wfit_ref.py; for the profile and the posterior tests/_post_ref.py on the same scaled columns, with its
derived bars taking the protocol's M.  Fit rows: atom indices equal, the other columns within RTOL 1e-5 / ATOL 1e-10, R2
within 1e-9 (_wfit_ref.assert_rows).  Every voxel is compared.  Every synthetic set asserts its smallest top-2 gap
>= 1e-8 |y'|^2 (the seeds were chosen on the CPU with the reference's own rotation; DESIGN.md 4.18 has the gaps).
Each test prints what it measures before it asserts."""
import os

import numpy as np
import pytest

import _post_ref as R
import _w2d_ref as W2
import _wfit_ref as WR
from test_fit2d_gpu import DIFF, Z, atoms, csf_signal
from test_soft2d_gpu import check_posterior, check_profile
from microstructure_fingerprinting_amd import _lib, engine
from microstructure_fingerprinting_amd import mf_utils as U

pytestmark = pytest.mark.gpu

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GAP, CUT, EPS, LD = W2.GAP, W2.CUT, R.EPS, R.LD
KINDS = ("mask", "smooth")
_cases, _rot = {}, []


def rot():
    if not _rot:
        _rot.append(np.load(os.path.join(G, "rot2d_cases.npz")))
    return _rot[0]


def case(shape):
    """tables, voxels, weights and the rotated dictionaries of one shape, computed once"""
    if shape not in _cases:
        name, N, V, zmin, seed = shape
        sch = rot()[name + "_sch"]
        T = U.RotateAtom2DTables(atoms(sch, N, seed), sch, Z, DIFF)
        Y, peaks, bad, Wm, Ws = W2.make_voxels(T.rotate_cols, sch, N, V, zmin, seed)
        D = [T.rotate(peaks[v].reshape(2, 3)) for v in range(V)]
        _cases[shape] = {"T": T, "Y": Y, "peaks": peaks, "bad": bad, "W": {"mask": Wm, "smooth": Ws}, "D": D, "V": V, "refs": {}}
    return _cases[shape]


def fit_refs(c, kind):
    """the fit's referee rows and the smallest top-2 gap of (shape, kind), computed once"""
    key = ("fit", kind)
    if key not in c["refs"]:
        W = c["W"][kind]
        rows = np.array([W2.ref_row(c["D"][v], c["Y"][v], W[v], False, None, 2, False) for v in range(c["V"])])
        gap = min(W2.gap(c["D"][v], c["Y"][v], W[v]) for v in range(c["V"]))
        c["refs"][key] = (rows, gap)
    return c["refs"][key]


def pair_refs(c, kind):
    key = ("pair", kind)
    if key not in c["refs"]:
        c["refs"][key] = [W2.pair_ref(c["D"][v], c["Y"][v], c["W"][kind][v]) for v in range(c["V"])]
    return c["refs"][key]


def wfit(T, Y, W, peaks, K=2):
    V = Y.shape[0]
    got, st, wst = engine.fit2d_weighted(T, Y, W, np.full(V, K), None, np.ascontiguousarray(peaks[:, :3 * K]), K, False)
    assert np.all(st == 0) and np.all(wst == 0)
    return got


# ---- 1. the reference's goldens
def test_reference_goldens():
    gold, base = np.load(os.path.join(G, "wfit2d_cases.npz")), np.load(os.path.join(G, "fit2d_cases.npz"))
    for name in ("syn2", "fix"):
        T = U.RotateAtom2DTables(base[name + "_dic"], rot()[name + "_sch"], Z, float(base["DIFF"]))
        K, csf = base[name + "_K"], base[name + "_csf"].astype(bool)
        Y, peaks = base[name + "_Y"], base[name + "_peaks"]
        for kind in ("mask", "smooth", "shared"):
            Wk = gold["%s_W_%s" % (name, kind)]
            r = T.fit(Y, peaks, K, csf_mask=csf, sig_csf=base[name + "_sig_csf"], weights=Wk)
            ref = gold["%s_params_%s" % (name, kind)]
            assert r.params.shape == ref.shape and np.all(r.status == 0)      # every stored voxel is compared
            WR.assert_rows(r.params, ref, 2, "%s %s" % (name, kind))
            assert r.weights.dtype == np.float64 and r.weights.shape == Wk.shape
            if name != "syn2":
                continue
            # F_W of every pair from the reference's lsqnonneg_2var_opt: the profile within the derived bar plus the stored dF
            vox = gold["syn2_vox2"]
            Wv = Wk[vox].astype(np.float64) if Wk.ndim == 2 else Wk.astype(np.float64)
            obj, par, ds, n = engine.profile2d(T, Y[vox], np.full(vox.size, 2), peaks[vox, :6], 2, partner=True, W=Wv)
            assert n == 0 and np.all(ds == 0)
            c2 = gold["syn2_c2_" + kind]
            refs = [{"F": gold["syn2_FW_" + kind][q].astype(LD), "c2bar": np.where(c2[q] <= CUT, 1.0, c2[q]), "clear": True,
                     "ysq": float(gold["syn2_ysq_" + kind][vox[q]])} for q in range(vox.size)]
            check_profile("golden F_W %s" % kind, refs, T.M, obj, par, extra=[gold["syn2_dFW_" + kind][q] for q in range(vox.size)])


# ---- 2. the referees on the library's own rotation, every shape
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", W2.SHAPES, ids=W2.IDS)
def test_fit_referee(shape, kind):
    c = case(shape)
    T, V = c["T"], c["V"]
    assert shape[1] <= _lib.lib().mfx_w2d_max_atoms(T.handle(), 0)            # the fused kernel serves it
    ref, gap = fit_refs(c, kind)
    print("%s N=%d %s: smallest top-2 gap %.2e |y'|^2 over %d voxels" % (shape[0], shape[1], kind, gap, V))
    assert gap >= GAP, "pick another seed: gap %.2e" % gap
    got = wfit(T, c["Y"], c["W"][kind], c["peaks"])
    WR.assert_rows(got, ref, 2, "%s %s" % (W2.IDS[W2.SHAPES.index(shape)], kind))
    # ignoring W cannot pass: the unweighted fit picks another pair in at least half of the voxels
    plain, _ = engine.fit2d(T, c["Y"], np.full(V, 2), None, c["peaks"], 2, False)
    differ = int(np.count_nonzero(np.any(plain[:, 3:5] != ref[:, 3:5], axis=1)))
    print("the unweighted fit picks another pair in %d of %d voxels" % (differ, V))
    assert 2 * differ >= V


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", W2.SHAPES, ids=W2.IDS)
def test_profile_and_posterior_referee(shape, kind):
    c = case(shape)
    T, V, Wk = c["T"], c["V"], c["W"][kind]
    lib = _lib.lib()
    assert shape[1] <= min(lib.mfx_w2d_max_atoms(T.handle(), 1), lib.mfx_w2d_max_atoms(T.handle(), 2))
    refs = pair_refs(c, kind)
    obj, par, ds, n = engine.profile2d(T, c["Y"], np.full(V, 2), c["peaks"], 2, partner=True, W=Wk)
    assert n == 0 and np.all(ds == 0) and obj.shape == (V, 2, T.N)
    check_profile("%s N=%d %s" % (shape[0], shape[1], kind), refs, T.M, obj, par)
    fit = wfit(T, c["Y"], Wk, c["peaks"])
    sse = fit[:, -2] * Wk.sum(axis=1)
    n_pos = np.count_nonzero(Wk > 0, axis=1)
    for v in range(V):                                                        # min obj = MSE * sum W, at the fitted atoms
        B = 16 * T.M * EPS * refs[v]["ysq"] / float(refs[v]["c2bar"][int(fit[v, 3]), int(fit[v, 4])])
        assert abs(obj[v].min() - sse[v]) <= 2 * B and abs(obj[v, 0, int(fit[v, 3])] - sse[v]) <= 2 * B
    for scale in (0.25, 4.0):
        sigma = np.sqrt(scale * sse / (n_pos - 2))
        w, ls, st, ds, n = engine.posterior2d(T, c["Y"], np.full(V, 2), c["peaks"], 2, sigma, shift=sse, W=Wk)
        assert n == 0 and np.all(ds == 0)
        check_posterior("%s N=%d %s sigma^2 x %g" % (shape[0], shape[1], kind, scale), refs, T.M, 2.0 * sigma ** 2, w, ls, st)
    wd, lsd, _, _, _ = engine.posterior2d(T, c["Y"], np.full(V, 2), c["peaks"], 2, sigma, W=Wk)       # the default shift
    assert np.array_equal(wd, w) and np.array_equal(lsd, ls)
    if shape == W2.SHAPES[0]:                                                  # one fascicle
        pk1 = np.ascontiguousarray(c["peaks"][:, :3])
        refs1 = [W2.single_ref(c["D"][v][0], c["Y"][v], Wk[v]) for v in range(V)]
        o1, p1, _, _ = engine.profile2d(T, c["Y"], np.full(V, 1), pk1, 1, partner=True, W=Wk)
        f1 = wfit(T, c["Y"], Wk, pk1, K=1)
        for v in range(V):
            F = refs1[v]["F"][:, 0]
            assert np.all(np.abs(o1[v, 0] - F) <= 16 * T.M * EPS * refs1[v]["ysq"]) and int(f1[v, 2]) == int(np.argmin(F))
        assert np.all(p1 == -1)
        sse1 = f1[:, -2] * Wk.sum(axis=1)
        s1 = np.sqrt(sse1 / (n_pos - 1))
        w1, ls1, st1, _, _ = engine.posterior2d(T, c["Y"], np.full(V, 1), pk1, 1, s1, shift=sse1, W=Wk)
        check_posterior("K = 1 %s" % kind, refs1, T.M, 2.0 * s1 ** 2, w1, ls1, st1, K=1)


# ---- 3. W = 1 is the unweighted entry point, bit for bit
@pytest.mark.parametrize("shape", W2.SHAPES, ids=W2.IDS)
def test_unit_weights_bit_for_bit(shape):
    c = case(shape)
    T, V, Y, peaks = c["T"], c["V"], c["Y"], c["peaks"]
    for K in (2, 1):
        pk = np.ascontiguousarray(peaks[:, :3 * K])
        Kv = np.full(V, K)
        plain, _ = engine.fit2d(T, Y, Kv, None, pk, K, False)
        sse = plain[:, -2] * T.M
        sigma = np.sqrt(sse / (T.M - K))
        post = engine.posterior2d(T, Y, Kv, pk, K, sigma, shift=sse)
        prof = engine.profile2d(T, Y, Kv, pk, K, partner=True)
        for Wone in (np.ones((V, T.M)), np.ones(T.M)):
            assert np.array_equal(wfit(T, Y, Wone, pk, K), plain), "fit K = %d" % K
            pw = engine.posterior2d(T, Y, Kv, pk, K, sigma, shift=sse, W=Wone)
            ow = engine.profile2d(T, Y, Kv, pk, K, partner=True, W=Wone)
            for q in range(4):
                assert np.array_equal(pw[q], post[q]), "posterior K = %d output %d" % (K, q)
            for q in range(3):
                assert np.array_equal(ow[q], prof[q]), "profile K = %d output %d" % (K, q)


# ---- 4. a 0/1 mask is the referee on the deleted rows
def test_mask_equals_deleted_rows():
    """Three sets of rows - all b0 rows of one (Delta, delta) pair, scattered rows, one whole chunk of 8 - each dropped
    together with the voxel's own corrupted rows (without those the voxels' best pairs tie within rounding)."""
    c = case(W2.SHAPES[0])
    T, V = c["T"], 8
    Y, peaks, D, Wm = c["Y"][:V], c["peaks"][:V], c["D"][:V], c["W"]["mask"][:V]
    sch = rot()["syn2_sch"]
    M = T.M
    first = np.flatnonzero(sch[:, 3] == 0)[0]
    drops = {"b0 of one (Delta, delta)": (sch[:, 3] == 0) & (sch[:, 4] == sch[first, 4]) & (sch[:, 5] == sch[first, 5]),
             "scattered": np.isin(np.arange(M), np.random.default_rng(61).choice(M, 9, replace=False)),
             "chunk": np.isin(np.arange(M), np.arange(8, 16))}
    for what, drop in drops.items():
        assert 0 < drop.sum() < M
        keep = (Wm > 0) & ~drop[None, :]
        got = wfit(T, Y, keep.astype(np.float64), peaks)
        Dk = [[D[v][0][keep[v]], D[v][1][keep[v]]] for v in range(V)]
        nk = keep.sum(axis=1)
        ref = np.array([W2.ref_row(D[v], Y[v], keep[v].astype(float), False, None, 2, False, deleted=True) for v in range(V)])
        gap = min(W2.gap(Dk[v], Y[v][keep[v]], np.ones(nk[v])) for v in range(V))
        print("%s: %d rows dropped with the voxels' own, smallest top-2 gap %.2e" % (what, drop.sum(), gap))
        assert gap >= GAP
        WR.assert_rows(got, ref, 2, what)
        for v in range(V):                                                    # MSE and R2 over the kept rows
            yk = Y[v][keep[v]]
            yrec = Dk[v][0][:, int(got[v, 3])] * got[v, 0] * got[v, 1] + Dk[v][1][:, int(got[v, 4])] * got[v, 0] * got[v, 2]
            assert abs(got[v, -1] - np.corrcoef(yk, yrec)[0, 1] ** 2) <= 1e-9
            assert abs(got[v, -2] - np.sum((yk - yrec) ** 2) / nk[v]) <= 1e-9 * np.sum(yk ** 2) / nk[v]
        refs = [W2.pair_ref(Dk[v], Y[v][keep[v]], np.ones(nk[v])) for v in range(V)]
        obj, par, _, _ = engine.profile2d(T, Y, np.full(V, 2), peaks, 2, partner=True, W=keep)
        check_profile("profile, " + what, refs, int(nk.max()), obj, par)
        sse = got[:, -2] * nk
        sigma = np.sqrt(sse / (nk - 2))
        w, ls, st, _, _ = engine.posterior2d(T, Y, np.full(V, 2), peaks, 2, sigma, shift=sse, W=keep.astype(np.float64))
        check_posterior("posterior, " + what, refs, int(nk.max()), 2.0 * sigma ** 2, w, ls, st)


# ---- 5. the fused kernels against the materialise-and-solve path
@pytest.mark.parametrize("shape", [W2.SHAPES[0], W2.SHAPES[2]], ids=[W2.IDS[0], W2.IDS[2]])
def test_fused_equals_explicit(shape):
    lib = _lib.lib()
    c = case(shape)
    T, V = c["T"], min(c["V"], 12)
    Y, Wk, pk = c["Y"][:V], c["W"]["smooth"][:V], c["peaks"][:V]
    for k in (1, 2):
        fused = wfit(T, Y, Wk, pk, k)
        try:
            lib.mfx_w2d_debug_set_force_explicit(1)
            explicit = wfit(T, Y, Wk, pk, k)
        finally:
            lib.mfx_w2d_debug_set_force_explicit(0)
        WR.assert_rows(fused, explicit, k, "%s K = %d" % (shape[0], k), rtol=1e-12, atol=0.0, r2_rtol=1e-12)


# ---- 6. scale invariance, extreme weights, (cW, cT, c shift)
def test_scale_and_extremes():
    c = case(W2.SHAPES[0])
    T, V, Y, peaks, Wk = c["T"], c["V"], c["Y"], c["peaks"], c["W"]["smooth"]
    base = wfit(T, Y, Wk, peaks)
    for f in (1e-6, 1e6):
        got = wfit(T, Y, f * Wk, peaks)
        assert np.array_equal(got[:, 3:5], base[:, 3:5])
        assert np.allclose(got[:, :3], base[:, :3], rtol=1e-9, atol=0) and np.allclose(got[:, 5:], base[:, 5:], rtol=1e-9, atol=0)
    # weights spanning 1e-6 .. 1e6 inside one voxel, against the referee: on the 1 776 rows (of 66 rows so spread a handful
    # carry the whole fit, and the best pairs tie)
    cx = case(W2.SHAPES[2])
    rng = np.random.default_rng(71)
    Wx = 10.0 ** rng.uniform(-6, 6, cx["Y"].shape)
    Wx[:, 0], Wx[:, 1] = 1e-6, 1e6
    ref = np.array([W2.ref_row(cx["D"][v], cx["Y"][v], Wx[v], False, None, 2, False) for v in range(cx["V"])])
    gap = min(W2.gap(cx["D"][v], cx["Y"][v], Wx[v]) for v in range(cx["V"]))
    print("1e-6 .. 1e6: smallest top-2 gap %.2e |y'|^2" % gap)
    assert gap >= GAP
    WR.assert_rows(wfit(cx["T"], cx["Y"], Wx, cx["peaks"]), ref, 2, "1e-6 .. 1e6")
    # (4 W, 4 T, 4 shift) is exact: every product and sum scales by a power of two
    sse = base[:, -2] * Wk.sum(axis=1)
    sigma = np.sqrt(sse / (T.M - 2))
    a = engine.posterior2d(T, Y, np.full(V, 2), peaks, 2, sigma, shift=sse, W=Wk)
    b = engine.posterior2d(T, Y, np.full(V, 2), peaks, 2, 2.0 * sigma, shift=4.0 * sse, W=4.0 * Wk)
    assert np.all(a[2] == 0) and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    o4, p4, _, _ = engine.profile2d(T, Y, np.full(V, 2), peaks, 2, partner=True, W=4.0 * Wk)
    o1, p1, _, _ = engine.profile2d(T, Y, np.full(V, 2), peaks, 2, partner=True, W=Wk)
    assert np.array_equal(o4, 4.0 * o1) and np.array_equal(p4, p1)


# ---- 7. identical directions under a non-trivial W
def test_identical_directions():
    c = case(W2.SHAPES[0])
    T, V = c["T"], 8
    peaks = c["peaks"][:V].copy()
    peaks[:, 3:] = peaks[:, :3]
    Y, Wk = c["Y"][:V], c["W"]["smooth"][:V]
    D = [T.rotate(peaks[v].reshape(2, 3)) for v in range(V)]
    assert np.array_equal(D[0][0], D[0][1])                                   # Det = 0 on the diagonal
    ref = np.array([W2.ref_row(D[v], Y[v], Wk[v], False, None, 2, False) for v in range(V)])
    WR.assert_rows(wfit(T, Y, Wk, peaks), ref, 2, "identical directions")
    refs = [W2.pair_ref(D[v], Y[v], Wk[v]) for v in range(V)]
    obj, par, _, _ = engine.profile2d(T, Y, np.full(V, 2), peaks, 2, partner=True, W=Wk)
    check_profile("identical directions", refs, T.M, obj, par)


# ---- 8. a mixed host batch with planted statuses
def test_mixed_host_batch():
    sch = rot()["syn2_sch"]
    N, V = 24, 30
    T = U.RotateAtom2DTables(atoms(sch, N, 81), sch, Z, DIFF)
    sig_csf = csf_signal(sch)
    Y, pk2, bad, Wm, Ws = W2.make_voxels(T.rotate_cols, sch, N, V, 0.1, 82)
    rng = np.random.default_rng(83)
    peaks = np.hstack([pk2, np.array([W2.random_dirs(rng, 1, 0.1)[0] for _ in range(V)])])
    K = np.arange(V) % 4
    csf = (np.arange(V) % 5) < 2
    Y[csf] = 0.8 * Y[csf] + 0.2 * sig_csf
    Wk = np.where((np.arange(V) % 2 == 0)[:, None], Ws, Wm)
    good, st, wst = engine.fit2d_weighted(T, Y, Wk, K, csf, peaks, 3, True, sig_csf)
    assert np.all(st == 0) and np.all(wst == 0) and good.shape == (V, 10)
    for k in range(4):
        assert ((K == k) & csf).any() and ((K == k) & ~csf).any()
    ref = np.array([W2.ref_row(list(T.rotate(peaks[v, :3 * K[v]].reshape(K[v], 3))) if K[v] else [], Y[v], Wk[v], bool(csf[v]), sig_csf,
                               3, True) for v in range(V)])
    WR.assert_rows(good, ref, 3, "mixed")
    assert np.all(good[(K == 0) & ~csf] == 0)
    # planted: a NaN weight, a negative weight, all-zero weights, a failing direction
    Wb, pb = Wk.copy(), peaks.copy()
    Wb[5, 0] = np.nan         # K = 1, CSF
    Wb[6, 7] = -1e-3          # K = 2, CSF
    Wb[9] = 0.0               # K = 1
    Wb[14] = 0.0              # K = 2
    Wb[3, 2] = np.inf         # K = 3
    pb[10, 3:6] = [0.0, 0.6, 0.6]     # K = 2: not a unit vector
    pb[13, 0:3] = [0.0, 0.6, 0.6]     # K = 1
    Wb[13, 1] = -1.0          # ... and a bad weight: the direction is reported, the weight status stays 0
    want = np.zeros(V, dtype=np.int32)
    want[[5, 6, 3]], want[[9, 14]] = 1, 2
    got, st, wst = engine.fit2d_weighted(T, Y, Wb, K, csf, pb, 3, True, sig_csf)
    assert np.array_equal(wst, want)
    assert np.array_equal(np.flatnonzero(st[:, 0]), [10, 13]) and st[10, 0] == U.ROT2D_NEWDIR_NORM and st[10, 4] == 1 and st[13, 4] == 0
    flagged = (want > 0) | (st[:, 0] != 0)
    assert np.all(np.isnan(got[flagged])) and np.array_equal(got[~flagged], good[~flagged])
    for v in np.flatnonzero(~flagged):                                        # every neighbour: the same voxel fitted alone
        alone, s1, w1 = engine.fit2d_weighted(T, Y[v:v + 1], Wb[v:v + 1], K[v:v + 1], csf[v:v + 1], pb[v:v + 1], 3, True, sig_csf)
        assert np.array_equal(alone[0], got[v]) and not s1.any() and not w1.any()
    # posterior and profile statuses in their order: 5 (direction), 1 (T), 3, 4 (weights)
    two = np.arange(8)                # as two-fascicle voxels, whatever their class above
    Y2, p2, W2b = Y[two], np.ascontiguousarray(peaks[two, :6]), Wk[two].copy()
    fit2 = wfit(T, Y2, W2b, p2)
    sse = fit2[:, -2] * W2b.sum(axis=1)
    sig = np.sqrt(sse / (np.count_nonzero(W2b > 0, axis=1) - 2))
    gw = engine.posterior2d(T, Y2, np.full(two.size, 2), p2, 2, sig, shift=sse, W=W2b)
    go = engine.profile2d(T, Y2, np.full(two.size, 2), p2, 2, partner=True, W=W2b)
    assert np.all(gw[2] == 0)
    W2b[0, 3], W2b[1] = -2.0, 0.0
    p2b, sigb = p2.copy(), sig.copy()
    p2b[2, 0:3] = [0.0, 0.6, 0.6]
    W2b[2, 0] = np.nan                # direction first
    sigb[3] = 0.0
    W2b[3, 5] = -1.0                  # T before the weights
    bw = engine.posterior2d(T, Y2, np.full(two.size, 2), p2b, 2, sigb, shift=sse, W=W2b)
    bo = engine.profile2d(T, Y2, np.full(two.size, 2), p2b, 2, partner=True, W=W2b)
    wantp = np.zeros(two.size, dtype=np.int32)
    wantp[:4] = [3, 4, 5, 1]
    assert np.array_equal(bw[2], wantp) and bw[3][2, 0] == U.ROT2D_NEWDIR_NORM
    assert np.all(np.isnan(bw[0][:4])) and np.all(np.isnan(bw[1][:4])) and np.all(np.isnan(bo[0][:4])) and np.all(bo[1][:4] == -1)
    assert np.array_equal(bw[0][4:], gw[0][4:]) and np.array_equal(bw[1][4:], gw[1][4:])
    assert np.array_equal(bo[0][4:], go[0][4:]) and np.array_equal(bo[1][4:], go[1][4:])
    # RotateAtom2DTables refuses such weights before any device call, whatever on_error says
    with pytest.raises(ValueError, match="Detected 4 of 30 voxel.s. with negative or non-finite weights"):
        T.fit(Y, pb, K, csf_mask=csf, sig_csf=sig_csf, on_error="nan", weights=Wb)


# ---- 9. the device-resident forms on a stream of their own
def test_dev_forms_equal_host_forms():
    import torch
    c = case(W2.SHAPES[0])
    T, V, Y, Wk = c["T"], c["V"], c["Y"], c["W"]["smooth"].copy()
    peaks = c["peaks"].copy()
    peaks[3, 3:6] = [0.0, 0.6, 0.6]
    Wk[5, 2], Wk[6] = -1.0, 0.0
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()   # noqa: E731
    stream = torch.cuda.Stream()
    for k in (2, 1):
        pk = np.ascontiguousarray(peaks[:, :3 * k])
        host = engine.fit2d_weighted(T, Y, Wk, np.full(V, k), None, pk, k, False)
        sse = np.where(np.isfinite(host[0][:, -2]), host[0][:, -2], 1.0) * np.abs(Wk).sum(axis=1)
        sigma = np.sqrt(np.where(sse > 0, sse, 1.0) / (T.M - k))
        hpost = engine.posterior2d(T, Y, np.full(V, k), pk, k, sigma, shift=sse, W=Wk)
        hprof = engine.profile2d(T, Y, np.full(V, k), pk, k, partner=True, W=Wk)
        dY, dW, dp, dT, dsh = t(Y), t(Wk), t(pk), t(2.0 * sigma ** 2), t(sse)
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            out, st, wst = engine.fit2d_weighted_dev(T, dY, dW, dp, k)
            w, ls, pst, ds = engine.posterior2d_dev(T, dY, dp, k, dT, dsh, d_W=dW)
            obj, par, ds2 = engine.profile2d_dev(T, dY, dp, k, partner=True, d_W=dW)
            after = (dY * 2.0).sum()                        # the caller's stream is still usable behind the calls
        stream.synchronize()
        assert np.array_equal(out.cpu().numpy(), host[0], equal_nan=True) and np.array_equal(st.cpu().numpy(), host[1])
        assert np.array_equal(wst.cpu().numpy(), host[2]) and host[2][5] == 1 and host[2][6] == 2
        assert np.array_equal(w.cpu().numpy(), hpost[0], equal_nan=True) and np.array_equal(ls.cpu().numpy(), hpost[1], equal_nan=True)
        assert np.array_equal(pst.cpu().numpy(), hpost[2]) and np.array_equal(ds.cpu().numpy(), hpost[3])
        assert np.array_equal(obj.cpu().numpy(), hprof[0], equal_nan=True) and np.array_equal(par.cpu().numpy(), hprof[1])
        assert np.array_equal(ds2.cpu().numpy(), hprof[2]) and abs(float(after) - 2.0 * Y.sum()) <= 1e-9 * Y.sum()
        assert hpost[2][5] == 3 and hpost[2][6] == 4 and (hpost[2][3] == 5) == (k == 2)
        # the shared vector on the device: stride 0
        shared = c["W"]["smooth"][0]
        o2, _, _ = engine.fit2d_weighted_dev(T, dY, t(shared), dp, k)
        torch.cuda.synchronize()
        assert np.array_equal(o2.cpu().numpy(), engine.fit2d_weighted(T, Y, shared, np.full(V, k), None, pk, k, False)[0], equal_nan=True)


# ---- 10. the LDS limits
def test_max_atoms_is_held():
    sch = rot()["syn2_sch"]
    lib = _lib.lib()
    T0 = U.RotateAtom2DTables(atoms(sch, 16, 91), sch, Z, DIFF)
    lim = [lib.mfx_w2d_max_atoms(T0.handle(), what) for what in range(3)]
    print("largest dictionaries of the weighted K = 2 kernels: fit %d, posterior %d, profile %d" % tuple(lim))
    rng = np.random.default_rng(92)
    for what in (1, 2, 0):
        for N, ok in ((lim[what], True), (lim[what] + 1, False)):
            T = U.RotateAtom2DTables(atoms(sch, N, 91), sch, Z, DIFF)
            d = W2.random_dirs(rng, 2, 0.1)
            ids = rng.integers(0, N, 2)
            cols = T.rotate_cols(d, ids)
            Y, peaks, Wk = (0.5 * cols[0] + 0.5 * cols[1])[None, :] + 0.01, d.reshape(1, 6), rng.uniform(0.5, 2.0, (1, T.M))
            if what == 0:                                       # the fit: beyond the limit the materialise-and-solve path
                got = wfit(T, Y, Wk, peaks)
                assert np.all(np.isfinite(got)) and got[0, -1] > 0.9
                continue
            call = (lambda: engine.posterior2d(T, Y, np.full(1, 2), peaks, 2, 0.05, shift=np.zeros(1) + 0.05, W=Wk)) if what == 1 else \
                   (lambda: engine.profile2d(T, Y, np.full(1, 2), peaks, 2, W=Wk))
            if ok:
                assert np.all(np.isfinite(call()[0]))
            else:
                with pytest.raises(NotImplementedError, match=str(lim[what])):
                    call()
                engine.profile2d(T, Y, np.full(1, 1), peaks[:, :3], 1, W=Wk)      # one fascicle has no limit of its own


# ---- 11. end to end: fit, a MAD mask from the residuals, the refit, its posterior, interval and profile
def test_robust_refit_end_to_end():
    sch = rot()["syn2_sch"]
    N, V = 48, 16
    dic = atoms(sch, N, 101)
    T = U.RotateAtom2DTables(dic, sch, Z, DIFF)
    rad = np.linspace(0.5, 4.0, N)[np.random.default_rng(103).permutation(N)]
    Y, peaks, ids, planted = W2.outlier_voxels(T.rotate_cols, T.M, N, V, 102)
    K = np.full(V, 2)
    plain = T.fit(Y, peaks, K)
    pred = np.array([T.rotate_cols(peaks[v].reshape(2, 3), plain.atoms[v]).T @ (plain.M0[v] * plain.frac[v]) for v in range(V)])
    Wk = W2.mad_mask(Y - pred)
    caught = np.array([np.all(~Wk[v, planted[v]]) for v in range(V)])
    r = T.fit(Y, peaks, K, weights=Wk)
    hit_plain = int(np.count_nonzero(np.all(plain.atoms == ids, axis=1)))
    hit = int(np.count_nonzero(np.all(r.atoms == ids, axis=1)))
    print("planted outliers masked in %d of %d voxels; planted atoms recovered: plain fit %d, refit %d" % (caught.sum(), V, hit_plain, hit))
    assert caught.sum() >= V - 2 and 4 * hit_plain <= V and 4 * hit >= 3 * V
    assert r.weights.dtype == np.float64 and np.array_equal(r.weights, Wk.astype(np.float64))
    post = T.posterior(Y, peaks, K, fit=r, props={"rad": rad})
    assert np.all(post.status == 0) and np.all(np.isfinite(post.log_evidence()))
    post_w = T.posterior(Y, peaks, K, weights=Wk, props={"rad": rad})
    assert np.array_equal(post.weights, post_w.weights) and np.array_equal(post.log_sum, post_w.log_sum)
    prof = T.profile(Y, peaks, K, partner=True, weights=Wk)
    sw = Wk.sum(axis=1)
    for v in range(V):
        D = T.rotate(peaks[v].reshape(2, 3))
        ref = W2.pair_ref(D, Y[v], Wk[v].astype(np.float64))
        B = 16 * T.M * EPS * ref["ysq"] / float(ref["c2bar"][r.atoms[v, 0], r.atoms[v, 1]])
        assert abs(prof.obj[v].min() - r.MSE[v] * sw[v]) <= 2 * B             # min obj = MSE * sum W
        assert prof.partner[v, 0, r.atoms[v, 0]] == r.atoms[v, 1]
    lo, hi, cnt = T.interval(Y, peaks, K, rad, rel=0.05, weights=Wk)
    rl, rh, rc = U.profile_interval(prof.obj, rad, 0.05, 0.0)
    assert np.array_equal(lo, rl) and np.array_equal(hi, rh) and np.array_equal(cnt, rc) and np.all(cnt >= 1)
    for v in range(V):
        assert lo[v, 0] <= rad[r.atoms[v, 0]] <= hi[v, 0] and lo[v, 1] <= rad[r.atoms[v, 1]] <= hi[v, 1]
    m, s = T.posterior_moments(Y, peaks, K, rad, weights=Wk)
    assert np.array_equal(m, post.mean("rad")) and np.array_equal(s, post.std("rad"))
    # the cold limit: all posterior weight on the fitted atoms
    cold = T.posterior(Y, peaks, K, sigma=1e-4 * np.sqrt(r.MSE), fit=r)
    for v in range(V):
        assert cold.status[v] == 0
        assert abs(cold.weights[v, 0, r.atoms[v, 0]] - 1.0) <= 1e-9 and abs(cold.weights[v, 1, r.atoms[v, 1]] - 1.0) <= 1e-9
    # fit_2Dprotocol is the same fit
    r2 = U.fit_2Dprotocol(dic, sch, Z, DIFF, Y, peaks, K, weights=Wk)
    assert np.array_equal(r2.params, r.params)
