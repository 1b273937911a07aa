"""Soft fits and objective profiles of 2-D (AxCaliber-like) protocols on the GPU (include/mfx_soft2d.h,
csrc/soft2d.hip): engine.posterior2d / profile2d and their _dev forms, RotateAtom2DTables.posterior / .profile /
.interval / .posterior_moments.

The referee is tests/_post_ref.py on the dictionaries the library's own rotation returns (T.rotate), which the kernels
must see bit for bit: the value F of every atom pair in long double (gram, pair_values with the kernel's cut), the
weights and log-sum with long-double exp (posterior), the comparison by worst_ratio.  The bars are derived there, not
measured, and take the protocol's M: a pair's F carries at most B = 16 M eps ||y||^2 / (1 - c^2); a weight may differ by
2 (E_k[i] + w_ref E) + (N^2 + 4096) eps and log_sum by 2 E + (N^2 + 4096) eps.  For the profile every computed pair value
lies within B of F, hence a row's minimum within [min_j (F - B), min_j (F + B)], and the referee's value at the kernel's
partner is at most min_j (F + B) + B there.  The golden comparison (the reference's own lsqnonneg_2var_opt on
reference-rotated dictionaries, tests/golden/soft2d_cases.npz) adds the stored dF to B.  Every comparison asserts its
input condition: no pair with 1 - c^2 within [cut / 4, 4 cut].

Each test prints what it measures before it asserts; the figures seen on the MI355X are in DESIGN.md 4.17.
"""
import json
import os

import numpy as np
import pytest

import _post_ref as R
from test_fit2d_gpu import DIFF, Z, atoms, random_dirs, rician, two_fascicle_voxels
from microstructure_fingerprinting_amd import _lib, engine
from microstructure_fingerprinting_amd import mf_utils as U

pytestmark = pytest.mark.gpu

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
LD, EPS = R.LD, R.EPS
CUT = 1e-8
# protocol, atoms, voxels, zmin, seed: one block with a ragged 16-atom tile; a second block of one atom; 2 x 2 blocks and
# the row and column sums across them; exactly one block
SHAPES = [("syn2", 72, 12, 0.1, 21), ("syn2", 129, 12, 0.1, 22), ("fix", 160, 6, 0.3, 23), ("fix", 128, 4, 0.3, 24)]
IDS = ["%s-%d" % (s[0], s[1]) for s in SHAPES]
_cases, _rot = {}, []


def rot():
    if not _rot:
        _rot.append(np.load(os.path.join(G, "rot2d_cases.npz")))
    return _rot[0]


def pair_ref(T, y, dirs):
    """long-double F of every pair on the library's own rotation, the 1 - c^2 of the bar, the input condition"""
    D = T.rotate(np.asarray(dirs).reshape(2, 3))
    g = R.gram(y, D[0], D[1])
    F, c2bar, c2s, below = R.pair_values(g, False, CUT)
    return {"F": F, "c2bar": c2bar, "clear": R.clear_of_the_cut(c2s, CUT), "ysq": float(g["ysq"]), "ncut": int(below.sum()),
            "c2min": float(c2s[0].min())}


def single_ref(T, y, d):
    """long-double F(i) of a one-fascicle voxel as an [N x 1] matrix for R.posterior (B = 16 M eps ||y||^2: c2bar = 1)"""
    D = T.rotate(np.asarray(d).reshape(1, 3))[0].astype(LD)
    yl = y.astype(LD)
    A, Yv = (D * D).sum(0), D.T @ yl
    ysq = yl @ yl
    return {"F": (ysq - np.maximum(Yv, 0) ** 2 / A)[:, None], "c2bar": np.ones((T.N, 1)), "ysq": float(ysq)}


def case(shape):
    """tables, voxels, their fit and the referee's pair values of one shape, computed once"""
    if shape not in _cases:
        name, N, V, zmin, seed = shape
        sch = rot()[name + "_sch"]
        T = U.RotateAtom2DTables(atoms(sch, N, seed), sch, Z, DIFF)
        Y, peaks = two_fascicle_voxels(T, np.random.default_rng(100 + seed), V, zmin)
        fit, st = engine.fit2d(T, Y, np.full(V, 2), None, peaks, 2, False)
        assert np.all(st == 0)
        _cases[shape] = {"T": T, "Y": Y, "peaks": peaks, "fit": fit, "sse": fit[:, -2] * T.M,
                         "ref": [pair_ref(T, Y[v], peaks[v]) for v in range(V)]}
    return _cases[shape]


def check_posterior(tag, refs, M, Tv, w, log_sum, status, K=2):
    """every voxel against the referee at its own temperature; returns the worst error / bar"""
    worst = 0.0
    for v, r in enumerate(refs):
        assert r.get("clear", True), "%s voxel %d: a pair near the cut: this input was chosen to have none" % (tag, v)
        ref = R.posterior(r["F"], r["c2bar"], r["ysq"], M, Tv[v])
        got = [w[v, 0], w[v, 1]] if K == 2 else [w[v, 0], np.ones(1)]
        ratio = R.worst_ratio(got, log_sum[v], ref)
        worst = max(worst, ratio)
        print("%s voxel %d: worst |got - referee| / bar = %.3g (bars on weights %.3g .. %.3g, on log_sum %.3g; %.1f effective "
              "pairs)" % (tag, v, ratio, float(ref["bar_w"][0].min()), float(ref["bar_w"][0].max()), float(ref["bar_log_sum"]),
                          ref["neff"]))
        assert status[v] == 0
        assert ratio <= 1.0, "%s voxel %d: %.3g of the bar" % (tag, v, ratio)
    return worst


def check_profile(tag, refs, M, obj, par, extra=None):
    """rows and columns of every voxel within [min (F - B), min (F + B)], the partner a minimiser within the bar"""
    worst = 0.0
    for v, r in enumerate(refs):
        assert r["clear"], "%s voxel %d: a pair near the cut: this input was chosen to have none" % (tag, v)
        F = r["F"]
        B = 16 * M * EPS * LD(r["ysq"]) / r["c2bar"].astype(LD) + (0 if extra is None else extra[v])
        for s, ax in ((0, 1), (1, 0)):
            lo, hi = (F - B).min(axis=ax), (F + B).min(axis=ax)
            o = obj[v, s].astype(LD)
            mid, half = (lo + hi) / 2, (hi - lo) / 2
            worst = max(worst, float(np.max(np.abs(o - mid) / half)))
            assert np.all(o >= lo) and np.all(o <= hi), "%s voxel %d slot %d: %.3g of the bar" % (tag, v, s, worst)
            if par is not None:
                p = par[v, s]
                assert p.min() >= 0 and p.max() < F.shape[0]
                ix = (np.arange(F.shape[0]), p) if s == 0 else (p, np.arange(F.shape[0]))
                assert np.all(F[ix] - B[ix] <= hi), "%s voxel %d slot %d: a partner that is not a minimiser" % (tag, v, s)
    print("%s: worst |obj - centre of the referee's interval| / its half width = %.3g" % (tag, worst))
    return worst


# ---- 1. the shapes: posterior at three noise levels, profile
@pytest.mark.parametrize("scale", [0.25, 1.0, 4.0])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_posterior_shapes(shape, scale):
    c = case(shape)
    T, V = c["T"], c["Y"].shape[0]
    assert shape[1] <= _lib.lib().mfx_soft2d_max_atoms(T.handle(), 0)
    sigma = np.sqrt(scale * c["sse"] / (T.M - 2))
    w, ls, st, ds, n = engine.posterior2d(T, c["Y"], np.full(V, 2), c["peaks"], 2, sigma, shift=c["sse"])
    assert n == 0 and np.all(ds == 0) and w.shape == (V, 2, T.N)
    check_posterior("%s N=%d sigma^2 x %g" % (shape[0], shape[1], scale), c["ref"], T.M, 2.0 * sigma ** 2, w, ls, st)
    assert np.all(np.abs(w.sum(axis=2) - 1.0) <= T.N * EPS)


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_profile_shapes(shape):
    c = case(shape)
    T, V = c["T"], c["Y"].shape[0]
    assert shape[1] <= _lib.lib().mfx_soft2d_max_atoms(T.handle(), 1)
    obj, par, ds, n = engine.profile2d(T, c["Y"], np.full(V, 2), c["peaks"], 2, partner=True)
    assert n == 0 and np.all(ds == 0) and obj.shape == (V, 2, T.N) and par.dtype == np.int32
    check_profile("%s N=%d" % (shape[0], shape[1]), c["ref"], T.M, obj, par)
    # against the fit, which has its own referees: the smallest value is the fit's objective, at the fitted atoms
    for v in range(V):
        r = c["ref"][v]
        i, j = int(c["fit"][v, 3]), int(c["fit"][v, 4])
        bar = 16 * T.M * EPS * r["ysq"] / float(r["c2bar"][i, j])
        assert abs(obj[v, 0].min() - c["sse"][v]) <= bar and abs(obj[v, 1].min() - c["sse"][v]) <= bar
        two = np.partition(r["F"].reshape(-1), 1)[:2]
        if float(two[1] - two[0]) > 2 * float((16 * T.M * EPS * r["ysq"] / r["c2bar"]).max()):     # a unique optimum
            assert (int(obj[v, 0].argmin()), int(obj[v, 1].argmin())) == (i, j)
            assert (int(par[v, 0, i]), int(par[v, 1, j])) == (j, i)


@pytest.mark.parametrize("name,N,V,zmin", [("syn2", 72, 12, 0.1), ("fix", 160, 6, 0.3)])
def test_one_fascicle(name, N, V, zmin):
    sch = rot()[name + "_sch"]
    T = U.RotateAtom2DTables(atoms(sch, N, 31), sch, Z, DIFF)
    Y, peaks = two_fascicle_voxels(T, np.random.default_rng(32), V, zmin, fmin=0.45)
    pk = np.ascontiguousarray(peaks[:, :3])
    fit, st = engine.fit2d(T, Y, np.full(V, 1), None, pk, 1, False)
    sse = fit[:, -2] * T.M
    refs = [single_ref(T, Y[v], pk[v]) for v in range(V)]
    obj, par, ds, n = engine.profile2d(T, Y, np.full(V, 1), pk, 1, partner=True)
    assert n == 0 and np.all(ds == 0) and np.all(par == -1)
    for v in range(V):
        bar = 16 * T.M * EPS * refs[v]["ysq"]
        err = np.abs(obj[v, 0].astype(LD) - refs[v]["F"][:, 0])
        print("%s K=1 voxel %d: max |obj - F| / bar = %.3g" % (name, v, float(err.max() / bar)))
        assert np.all(err <= bar)
        assert abs(obj[v, 0].min() - sse[v]) <= bar and int(obj[v, 0].argmin()) == int(fit[v, 2])
    for scale in (0.25, 1.0, 4.0):
        sigma = np.sqrt(scale * sse / (T.M - 1))
        w, ls, pst, ds, n = engine.posterior2d(T, Y, np.full(V, 1), pk, 1, sigma, shift=sse)
        check_posterior("%s K=1 sigma^2 x %g" % (name, scale), refs, T.M, 2.0 * sigma ** 2, w, ls, pst, K=1)
        assert np.all(np.abs(w.sum(axis=2) - 1.0) <= T.N * EPS)


# ---- 2. the reference's goldens
def test_reference_goldens():
    gold, g = np.load(os.path.join(G, "fit2d_cases.npz")), np.load(os.path.join(G, "soft2d_cases.npz"))
    cut = float(g["cut"])
    assert cut == _lib.lib().mfx_profile_cut() == CUT
    for name in ("syn2", "fix"):
        T = U.RotateAtom2DTables(gold[name + "_dic"], rot()[name + "_sch"], Z, float(gold["DIFF"]))
        v2, v1 = g[name + "_vox2"], g[name + "_vox1"]
        assert v2.size and v1.size
        refs = []
        for r, v in enumerate(v2):
            c2 = g[name + "_c2"][r]
            assert not np.any((c2 >= cut / 4) & (c2 <= 4 * cut))
            refs.append({"F": g[name + "_F2"][r].astype(LD), "c2bar": np.where(c2 <= cut, 1.0, c2), "clear": True,
                         "ysq": float(g[name + "_ysq2"][r])})
        obj, par, ds, n = engine.profile2d(T, gold[name + "_Y"][v2], np.full(v2.size, 2), gold[name + "_peaks"][v2], 2, partner=True)
        assert n == 0 and np.all(ds == 0)
        check_profile("golden " + name, refs, T.M, obj, par, extra=[g[name + "_dF2"][r].astype(LD) for r in range(v2.size)])
        obj1, par1, ds, n = engine.profile2d(T, gold[name + "_Y"][v1], np.full(v1.size, 1), gold[name + "_peaks"][v1, :3], 1, partner=True)
        for r in range(v1.size):
            bar = 16 * T.M * EPS * float(g[name + "_ysq1"][r]) + g[name + "_dF1"][r]
            err = np.abs(obj1[r, 0] - g[name + "_F1"][r])
            print("golden %s K=1 voxel %d: %.3g of the bar" % (name, v1[r], float(np.max(err / bar))))
            assert np.all(err <= bar) and np.all(par1[r] == -1)


# ---- 3. the cold limit: the posterior collapses onto the fitted atoms
def test_cold_limit_is_the_fit():
    c = case(SHAPES[0])
    T, V = c["T"], c["Y"].shape[0]
    sigma = np.sqrt(c["sse"] / (T.M - 2) / 1e4)
    w, ls, st, ds, n = engine.posterior2d(T, c["Y"], np.full(V, 2), c["peaks"], 2, sigma, shift=c["sse"])
    assert np.all(st == 0)
    for v in range(V):
        i, j = int(c["fit"][v, 3]), int(c["fit"][v, 4])
        print("cold voxel %d: weights of the fitted atoms %.6f %.6f" % (v, w[v, 0, i], w[v, 1, j]))
        assert w[v, 0, i] > 0.99 and w[v, 1, j] > 0.99


# ---- 4. identical directions: the diagonal is scored as single atoms, both fascicles see the same problem
def test_identical_directions():
    sch = rot()["syn2_sch"]
    T = U.RotateAtom2DTables(atoms(sch, 48, 41), sch, Z, DIFF)
    rng = np.random.default_rng(42)
    V = 6
    Y, peaks = two_fascicle_voxels(T, rng, V, 0.3)
    peaks[:, 3:6] = peaks[:, 0:3]
    D = T.rotate(peaks[0].reshape(2, 3))
    assert np.array_equal(D[0], D[1])
    refs = [pair_ref(T, Y[v], peaks[v]) for v in range(V)]
    fit, _ = engine.fit2d(T, Y, np.full(V, 2), None, peaks, 2, False)
    sse = fit[:, -2] * T.M
    obj, par, ds, n = engine.profile2d(T, Y, np.full(V, 2), peaks, 2, partner=True)
    for v in range(V):
        r = refs[v]
        assert r["clear"] and r["ncut"] >= T.N           # the diagonal at least lies under the cut
        yl = Y[v].astype(LD)
        Dl = T.rotate(peaks[v, :3].reshape(1, 3))[0].astype(LD)
        alone = yl @ yl - np.maximum(Dl.T @ yl, 0) ** 2 / (Dl * Dl).sum(0)
        assert np.all(np.abs(np.diag(r["F"]) - alone) <= 16 * T.M * EPS * r["ysq"])     # the referee's diagonal: single atoms
    check_profile("identical directions", refs, T.M, obj, par)
    sigma = np.sqrt(sse / (T.M - 2))
    w, ls, st, ds, n = engine.posterior2d(T, Y, np.full(V, 2), peaks, 2, sigma, shift=sse)
    check_posterior("identical directions", refs, T.M, 2.0 * sigma ** 2, w, ls, st)
    for v in range(V):
        ref = R.posterior(refs[v]["F"], refs[v]["c2bar"], refs[v]["ysq"], T.M, 2.0 * sigma[v] ** 2)
        assert np.all(np.abs(w[v, 0] - w[v, 1]) <= ref["bar_w"][0] + ref["bar_w"][1])
    assert np.all(np.abs(w.sum(axis=2) - 1.0) <= T.N * EPS)


# ---- 5. launch independence, the device path, shift
def test_launch_independence_and_dev_path():
    import torch
    c = case(SHAPES[1])
    T, Y, peaks = c["T"], c["Y"], c["peaks"]
    V = Y.shape[0]
    sigma = np.sqrt(c["sse"] / (T.M - 2))
    host = engine.posterior2d(T, Y, np.full(V, 2), peaks, 2, sigma, shift=c["sse"])
    hobj = engine.profile2d(T, Y, np.full(V, 2), peaks, 2, partner=True)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()   # noqa: E731
    dT, dsh = t(2.0 * sigma ** 2), t(c["sse"])
    w, ls, st, ds = engine.posterior2d_dev(T, t(Y), t(peaks), 2, dT, dsh)
    obj, par, ds2 = engine.profile2d_dev(T, t(Y), t(peaks), 2, partner=True)
    after = (t(Y) * 2.0).sum()                              # torch's stream is still usable behind the calls
    torch.cuda.synchronize()
    assert np.array_equal(w.cpu().numpy(), host[0]) and np.array_equal(ls.cpu().numpy(), host[1])
    assert np.array_equal(st.cpu().numpy(), host[2]) and np.array_equal(ds.cpu().numpy(), host[3])
    assert np.array_equal(obj.cpu().numpy(), hobj[0]) and np.array_equal(par.cpu().numpy(), hobj[1])
    assert np.array_equal(ds2.cpu().numpy(), hobj[2]) and abs(float(after) - 2.0 * Y.sum()) <= 1e-9 * Y.sum()
    # voxel 3 alone, and at two positions of a batch among other voxels
    order = np.array([5, 3, 0, 7, 1, 3, 9])
    alone = engine.posterior2d(T, Y[3:4], np.full(1, 2), peaks[3:4], 2, sigma[3:4], shift=c["sse"][3:4])
    batch = engine.posterior2d(T, Y[order], np.full(order.size, 2), peaks[order], 2, sigma[order], shift=c["sse"][order])
    for q in (0, 1):
        assert np.array_equal(alone[q][0], batch[q][1]) and np.array_equal(alone[q][0], batch[q][5])
        assert np.array_equal(alone[q][0], host[q][3])
    aobj = engine.profile2d(T, Y[3:4], np.full(1, 2), peaks[3:4], 2, partner=True)
    bobj = engine.profile2d(T, Y[order], np.full(order.size, 2), peaks[order], 2, partner=True)
    for q in (0, 1):
        assert np.array_equal(aobj[q][0], bobj[q][1]) and np.array_equal(aobj[q][0], bobj[q][5]) and np.array_equal(aobj[q][0], hobj[q][3])
    # the one-fascicle class likewise
    pk1 = np.ascontiguousarray(peaks[:, :3])
    h1 = engine.posterior2d(T, Y, np.full(V, 1), pk1, 1, sigma, shift=c["sse"] * 4)
    w1, ls1, st1, _ = engine.posterior2d_dev(T, t(Y), t(pk1), 1, dT, t(c["sse"] * 4))
    o1, p1, _ = engine.profile2d_dev(T, t(Y), t(pk1), 1, partner=True)
    torch.cuda.synchronize()
    assert np.array_equal(w1.cpu().numpy(), h1[0]) and np.array_equal(ls1.cpu().numpy(), h1[1]) and np.all(st1.cpu().numpy() == h1[2])
    assert np.array_equal(o1.cpu().numpy(), engine.profile2d(T, Y, np.full(V, 1), pk1, 1)[0]) and np.all(p1.cpu().numpy() == -1)


def test_shift_cancels_and_status_codes():
    c = case(SHAPES[0])
    T, Y, peaks = c["T"], c["Y"], c["peaks"]
    V = Y.shape[0]
    sigma = np.sqrt(c["sse"] / (T.M - 2))
    Tv = 2.0 * sigma ** 2
    w, ls, st, _, _ = engine.posterior2d(T, Y, np.full(V, 2), peaks, 2, sigma, shift=c["sse"])
    w2, ls2, st2, _, _ = engine.posterior2d(T, Y, np.full(V, 2), peaks, 2, sigma, shift=c["sse"] - 20.0 * Tv)
    check_posterior("shifted by 20 T", c["ref"], T.M, Tv, w2, ls2, st2)
    for v in range(V):
        ref = R.posterior(c["ref"][v]["F"], c["ref"][v]["c2bar"], c["ref"][v]["ysq"], T.M, Tv[v])
        assert np.all(np.abs(w[v, 0] - w2[v, 0]) <= 2 * ref["bar_w"][0]) and abs(ls[v] - ls2[v]) <= 2 * ref["bar_log_sum"]
    # default shift: the fit's own objective
    wd, lsd, std, _, _ = engine.posterior2d(T, Y, np.full(V, 2), peaks, 2, sigma)
    assert np.array_equal(wd, w) and np.array_equal(lsd, ls)
    # status 1: T or shift unusable; status 2: the shift far above the smallest objective, or so far below that Z vanishes
    sig = sigma.copy()
    sig[1], sig[4] = 0.0, np.inf
    sh = c["sse"].copy()
    sh[2], sh[6] = np.nan, np.inf
    sh[7] = c["sse"][7] + 800.0 * Tv[7]
    sh[8] = c["sse"][8] - 800.0 * Tv[8]
    wb, lsb, stb, dsb, _ = engine.posterior2d(T, Y, np.full(V, 2), peaks, 2, sig, shift=sh)
    want = np.zeros(V, dtype=np.int32)
    want[[1, 2, 4, 6]], want[[7, 8]] = 1, 2
    assert np.array_equal(stb, want) and np.all(dsb == 0)
    bad = want != 0
    assert np.all(np.isnan(wb[bad])) and np.all(np.isnan(lsb[bad]))
    assert np.array_equal(wb[~bad], w[~bad]) and np.array_equal(lsb[~bad], ls[~bad])      # the neighbours are untouched
    pk1 = np.ascontiguousarray(peaks[:, :3])
    _, _, st1, _, _ = engine.posterior2d(T, Y, np.full(V, 1), pk1, 1, sig, shift=sh)
    assert np.all(st1[[1, 2, 4, 6]] == 1) and st1[8] == 2


# ---- 6. a failing direction in a batch
def test_failing_direction_in_a_batch():
    errs = {e["why"]: e for e in json.loads(str(rot()["errors_json"]))}
    T = U.RotateAtom2DTables(rot()["fix_sig"], rot()["fix_sch"], Z, DIFF)
    V = 8
    Y, peaks = two_fascicle_voxels(T, np.random.default_rng(51), V, 0.3)
    K = np.full(V, 2)
    fit, fst = engine.fit2d(T, Y, K, None, peaks, 2, False)
    sigma = np.sqrt(fit[:, -2] * T.M / (T.M - 2))
    good = engine.posterior2d(T, Y, K, peaks, 2, sigma)
    gobj = engine.profile2d(T, Y, K, peaks, 2, partner=True)
    assert np.all(good[2] == 0) and np.all(good[3] == 0)
    bad = peaks.copy()
    bad[5, 3:6] = errs["in-plane new fascicle: 4 pairs"]["newdir"]
    _, bst = engine.fit2d(T, Y, K, None, bad, 2, False)
    w, ls, st, ds, n = engine.posterior2d(T, Y, K, bad, 2, sigma)
    obj, par, ds2, _ = engine.profile2d(T, Y, K, bad, 2, partner=True)
    assert st[5] == 5 and np.all(np.delete(st, 5) == 0) and n == 0
    assert np.array_equal(ds, bst) and np.array_equal(ds2, bst) and tuple(ds[5]) == (U.ROT2D_NEW_PAIRS, 0, 4, 0, 1)
    assert np.all(np.isnan(w[5])) and np.isnan(ls[5]) and np.all(np.isnan(obj[5])) and np.all(par[5] == -1)
    keep = np.delete(np.arange(V), 5)
    assert np.array_equal(w[keep], good[0][keep]) and np.array_equal(ls[keep], good[1][keep])
    assert np.array_equal(obj[keep], gobj[0][keep]) and np.array_equal(par[keep], gobj[1][keep])
    # through the tables: 'nan' returns the record, 'raise' the reference's exception
    post = T.posterior(Y, bad, K, on_error="nan")
    assert post.status[5] == 5 and np.array_equal(post.dir_status, bst)
    with pytest.raises(Exception) as ei:
        T.profile(Y, bad, K)
    e = errs["in-plane new fascicle: 4 pairs"]
    assert (type(ei.value).__name__, str(ei.value)) == (e["type"], e["msg"])


# ---- 7. the LDS limit
@pytest.mark.parametrize("what", [0, 1])
def test_max_atoms_is_held(what):
    sch = rot()["syn2_sch"]
    T0 = U.RotateAtom2DTables(atoms(sch, 16, 61), sch, Z, DIFF)
    nmax = _lib.lib().mfx_soft2d_max_atoms(T0.handle(), what)
    assert nmax > 1024 and nmax % 16 == 0
    rng = np.random.default_rng(62)
    for N, ok in ((nmax, True), (nmax + 1, False)):
        T = U.RotateAtom2DTables(atoms(sch, N, 61), sch, Z, DIFF)
        Y, peaks = two_fascicle_voxels(T, rng, 1, 0.1)
        call = (lambda: engine.posterior2d(T, Y, np.full(1, 2), peaks, 2, 0.05, shift=np.zeros(1) + 0.05)) if what == 0 else \
               (lambda: engine.profile2d(T, Y, np.full(1, 2), peaks, 2))
        if ok:
            out = call()
            assert np.all(np.isfinite(out[0]))
        else:
            with pytest.raises(NotImplementedError, match=str(nmax)):
                call()
            engine.profile2d(T, Y, np.full(1, 1), peaks[:, :3], 1)       # one fascicle has no limit of its own


# ---- 8. RotateAtom2DTables on a mixed set
def test_tables_methods_on_a_mixed_set():
    sch = rot()["syn2_sch"]
    N = 40
    T = U.RotateAtom2DTables(atoms(sch, N, 71), sch, Z, DIFF)
    rng = np.random.default_rng(72)
    V = 12
    Y, peaks = two_fascicle_voxels(T, rng, V, 0.1, fmin=0.4)
    K = np.where(np.arange(V) % 3 == 0, 1, 2)
    K[7] = 0
    rad = np.linspace(0.5, 4.0, N)[np.random.default_rng(73).permutation(N)]
    fit = T.fit(Y, peaks, K)
    post = T.posterior(Y, peaks, K, props={"rad": rad})
    assert post.n_unsupported == 1 and post.status[7] == -1 and np.all(np.delete(post.status, 7) == 0)
    assert np.all(np.isnan(post.weights[7])) and np.all(np.isnan(post.weights[K == 1, 1])) and post.weights.shape == (V, 2, N)
    post2 = T.posterior(Y, peaks, K, fit=fit, props={"rad": rad})
    assert np.array_equal(post.weights, post2.weights, equal_nan=True)
    sse = fit.MSE * T.M
    w, ls, st, _, _ = engine.posterior2d(T, Y, K, peaks, 2, np.sqrt(sse / (T.M - K)), shift=sse)
    assert np.array_equal(post.weights, w, equal_nan=True) and np.array_equal(post.log_sum, ls, equal_nan=True)
    m, s = U.posterior_moments(post.weights, rad)
    assert np.array_equal(post.mean("rad"), m, equal_nan=True) and np.array_equal(post.std("rad"), s, equal_nan=True)
    m2, s2 = T.posterior_moments(Y, peaks, K, rad)
    assert np.array_equal(m2, m, equal_nan=True) and np.array_equal(s2, s, equal_nan=True)
    assert post.quantile("rad", 0.5).shape == (V, 2) and post.by_property("rad")[1].shape == (V, 2, N)
    assert np.all(np.isfinite(post.log_evidence()[K > 0]))
    prof = T.profile(Y, peaks, K, partner=True, props={"rad": rad})
    obj, par, _, n = engine.profile2d(T, Y, K, peaks, 2, partner=True)
    assert np.array_equal(prof.obj, obj, equal_nan=True) and np.array_equal(prof.partner, par) and prof.n_unsupported == n == 1
    assert prof.by_property("rad")[1].shape == (V, 2, N)
    lo, hi, cnt = T.interval(Y, peaks, K, rad, rel=0.05)
    rl, rh, rc = U.profile_interval(obj, rad, 0.05, 0.0)
    assert np.array_equal(lo, rl, equal_nan=True) and np.array_equal(hi, rh, equal_nan=True) and np.array_equal(cnt, rc)
    assert np.all(cnt[K == 2] >= 1) and np.all(cnt[7] == 0)
    # MSE = 0 (no signal at all): the default sigma is 0, status 1
    Yz = Y.copy()
    Yz[0] = 0.0
    pz = T.posterior(Yz, peaks, K)
    assert pz.status[0] == 1 and np.all(np.isnan(pz.weights[0])) and np.all(np.delete(pz.status, [0, 7]) == 0)
    # a two-fascicle phantom voxel: the evidence prefers two fascicles to one
    two = np.flatnonzero(K == 2)
    e2 = T.posterior(Y[two], peaks[two], np.full(two.size, 2), sigma=1.0 / 30).log_evidence()
    e1 = T.posterior(Y[two], peaks[two], np.full(two.size, 1), sigma=1.0 / 30).log_evidence()
    print("log evidence K=2 minus K=1:", e2 - e1)
    assert np.all(e2 > e1)
