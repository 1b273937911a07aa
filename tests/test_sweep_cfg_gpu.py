"""Every kernel of csrc/profile.hip and csrc/posterior.hip on the GPU, against the long-double referee.

The rows of tests/_sweep_cfg_cases.py reach each of the 78 K = 2 forms (configuration x bracketed rows x CSF x family x
weights) and the 8 K = 1 kernels; tests/test_sweep_cfg_host.py guards their input conditions without a GPU.  After each
K = 2 call the library's debug hook (mfx_profile_debug_last_config, mfx_post_debug_last_config) must report exactly the
row's form: the tests assert which kernel they ran, they do not predict it.

No tolerance is new.  Landscape: every pair within 16 M eps ||y||^2 / (1 - c^2) of the referee (tests/test_profile_gpu.py).
Profile: values within that bar at the voxel's worst conditioned pair; partner the referee's arg-min or a minimiser
within the bar; all N atoms of both slots.  Posterior: tests/_post_ref.py's worst_ratio <= 1 on weights and log_sum with
the shift at the referee's minimum, status 0, each fascicle's weights summing to 1 within N eps.  Weighted forms: the
referee on rows scaled by sqrt(W).  Every bar comes from the referee, never from the code under test.

Each test prints its worst error / bar before it asserts; the figures seen on the MI355X are in DESIGN.md 4.16b.
"""
import numpy as np
import pytest

import _post_ref as R
import _sweep_cfg_cases as S

pytestmark = pytest.mark.gpu

LD, EPS = R.LD, R.EPS
T = 2.0 * S.SIGMA ** 2


def _lib():
    from microstructure_fingerprinting_amd import _lib as L
    return L.lib()


def _plan(proto, N):
    return S.interpolator(S.base(proto), N).plan_for(S.scheme(proto))


def _form(family):
    """the hook's record of the calling thread's last K = 2 launch of the family ('post' or 'profile'), or None"""
    from microstructure_fingerprinting_amd import _lib as L
    buf = np.full(8, -1, dtype=np.int32)
    ok = getattr(L.lib(), "mfx_%s_debug_last_config" % family)(L.iptr(buf))
    return tuple(int(v) for v in buf) if ok else None


def _call(kind, proto, N, Y, pk, csf, W=None, partner=True, shift=None):
    """the family's host entry point on V voxels of one class; returns (outputs, the form the hook reports)"""
    from microstructure_fingerprinting_amd import engine
    plan, V = _plan(proto, N), Y.shape[0]
    x = S.sig_csf(proto) if csf else None
    K, c = np.full(V, 2), np.full(V, csf)
    if kind == "land":
        return engine.pair_objectives(plan, Y, pk, csf, x, W=W), _form("profile")
    if kind == "prof":
        obj, par, n_uns = engine.profile(plan, Y, K, c, pk, 2, csf, x, partner=partner, W=W)
        assert n_uns == 0
        return (obj, par), _form("profile")
    w, ls, st, n_uns = engine.posterior(plan, Y, K, c, pk, 2, csf, x, S.SIGMA, shift=shift, W=W)
    assert n_uns == 0
    return (w, ls, st), _form("post")


def _limit(kind, proto, N, csf, wgt):
    """the library's own limit for the row's plan, family and flags"""
    lib, h = _lib(), _plan(proto, N).handle()
    if wgt:
        return lib.mfx_wsoft_max_atoms(h, int(csf), {"post": 0, "prof": 1, "land": 2}[kind])
    if kind == "post":
        return lib.mfx_post_max_atoms(h, int(csf))
    return lib.mfx_profile_max_atoms(h, int(csf), int(kind == "land"))


def test_the_cut_is_the_cases_cut():
    assert float(_lib().mfx_profile_cut()) == S.CUT


# ------------------------------------------------------------------------------------------------
# 1. one row per form, and the rows at the limits
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", S.rows(), ids=lambda r: r["id"])
def test_form_against_the_referee(row):
    kind, proto, N, csf = row["kind"], row["proto"], row["N"], row["csf"]
    y = S.signal(proto, N, row["seed"])
    pk = S.peaks(proto)[None, :]
    W = S.weights(proto)[None, :] if row["wgt"] else None
    f = S.referee(row, y=y)
    assert not f["below"].any(), "a pair at or below the cut: this input was chosen to have none"
    F, M, ysq = f["F"], f["M"], f["ysq"]
    out, form = _call(kind, proto, N, y[None, :], pk, csf, W, shift=np.array([float(F.min())]))
    print("%s: the hook reports %s" % (row["id"], form))
    assert form == row["form"], "%s ran %s, the row is meant for %s" % (row["id"], form, row["form"])
    if row["limit"]:
        assert _limit(kind, proto, N, csf, row["wgt"]) == N
    if kind == "land":
        assert out.shape == (1, N, N)
        ratio = np.abs(out[0].astype(LD) - F) / (16 * M * EPS * ysq / f["c2bar"])
        worst = float(ratio.max())
        print("%s: worst |F - referee| / bar = %.3g over %d pairs (smallest 1 - c^2 = %.3g)" % (row["id"], worst, N * N, float(f["c2bar"].min())))
        assert np.all(ratio <= 1.0)
    elif kind == "prof":
        obj, par = out
        bar = 16 * M * EPS * ysq / float(f["c2bar"].min())
        assert obj.shape == (1, 2, N) and par.shape == (1, 2, N)
        worst, nmis = 0.0, 0
        for k in range(2):
            Fk = F if k == 0 else F.T
            worst = max(worst, float(np.max(np.abs(obj[0, k].astype(LD) - Fk.min(axis=1)))) / bar)
            assert (par[0, k] >= 0).all() and (par[0, k] < N).all()
            nmis += int((par[0, k] != Fk.argmin(axis=1)).sum())
            at = Fk[np.arange(N), par[0, k]] - Fk.min(axis=1)
            assert np.all(at <= bar), "%s slot %d: a partner that is not a minimiser" % (row["id"], k)
        print("%s: worst |obj - referee| / bar = %.3g over 2 x %d atoms, %d partners differ (ties within the bar)" % (row["id"], worst, N, nmis))
        assert worst <= 1.0
    else:
        w, ls, st = out
        ref = R.posterior(F, f["c2bar"], ysq, M, T)
        worst = R.worst_ratio(w[0], ls[0], ref)
        sums = [abs(float(w[0, k].sum()) - 1.0) for k in range(2)]
        print("%s: posterior at %.3g of the bar (log_sum %.6f, %.1f effective pairs), |sum w - 1| = %.3g, %.3g"
              % (row["id"], worst, float(ls[0]), ref["neff"], sums[0], sums[1]))
        assert st[0] == 0 and w.shape == (1, 2, N)
        assert worst <= 1.0
        assert max(sums) < N * EPS


# ------------------------------------------------------------------------------------------------
# 2. the K = 1 kernels
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", S.k1_rows(), ids=lambda r: r["id"])
def test_k1_against_the_referee(row):
    """One fascicle, the whole pool: F(i) = ||y||^2 - max(Y_i, 0)^2 / A_ii, with CSF the best support of the two unknowns;
    B = 16 M eps ||y||^2 (tests/test_wsoft_gpu.py's referee of K = 1)."""
    from microstructure_fingerprinting_amd import engine
    kind, proto, N, csf, wgt = row["kind"], row["proto"], row["N"], row["csf"], row["wgt"]
    rng = np.random.default_rng(row["seed"])
    b = S.block(proto, wgt)
    y = 500.0 * S.rotated(proto)[0][:, int(rng.integers(0, N))]
    y = np.ascontiguousarray(y + rng.normal(0, S.SIGMA, y.shape))
    ys = (b["s"] * y).astype(LD)
    A, Yv, ysq = b["A11"][:N], b["D0"][:, :N].astype(LD).T @ ys, ys @ ys
    sc = R.TP._single(Yv, A)
    if csf:
        X, xx, xy = b["X1"][:N], b["xx"], b["x"].astype(LD) @ ys
        c2 = 1 - X * X / (A * xx)
        assert R.clear_of_the_cut([c2], S.CUT) and c2.min() > S.CUT
        sc = np.maximum(np.maximum(sc, R.TP._single(xy, xx)), R.TP._pair_inner(A, xx, X, Yv, xy))
    F = (ysq - sc)[:, None]
    M, ysq = S.M_of(proto), float(ysq)
    plan, x = _plan(proto, N), (S.sig_csf(proto) if csf else None)
    pk, W = S.peaks(proto)[None, :3], (S.weights(proto)[None, :] if wgt else None)
    one, c = np.full(1, 1), np.full(1, csf)
    if kind == "prof":
        obj, par, n_uns = engine.profile(plan, y[None, :], one, c, pk, 1, csf, x, partner=True, W=W)
        worst = float(np.max(np.abs(obj[0, 0].astype(LD) - F[:, 0]))) / (16 * M * EPS * ysq)
        print("%s: worst |obj - referee| / bar = %.3g over %d atoms" % (row["id"], worst, N))
        assert n_uns == 0 and np.all(par == -1) and worst <= 1.0
    else:
        w, ls, st, n_uns = engine.posterior(plan, y[None, :], one, c, pk, 1, csf, x, S.SIGMA, shift=np.array([float(F.min())]), W=W)
        ref = R.posterior(F, np.ones_like(F), ysq, M, T)
        worst = max(float(np.max(np.abs(w[0, 0].astype(LD) - ref["w"][0]) / ref["bar_w"][0])),
                    float(abs(LD(ls[0]) - ref["log_sum"]) / ref["bar_log_sum"]))
        print("%s: posterior at %.3g of the bar over %d atoms (log_sum %.6f)" % (row["id"], worst, N, float(ls[0])))
        assert n_uns == 0 and st[0] == 0 and worst <= 1.0 and abs(float(w[0, 0].sum()) - 1.0) < N * EPS


# ------------------------------------------------------------------------------------------------
# 3. unit weights give the bits of the unweighted call, in every configuration
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", [0, 1, 2, 3])
@pytest.mark.parametrize("kind", S.KINDS)
def test_unit_weights_reproduce_the_unweighted_call(kind, cfg):
    """At the weighted form's limit for the configuration, where the unweighted call takes the same configuration: the
    hook reports forms that differ in WGT alone, and the outputs are equal bit for bit."""
    proto = "long" if cfg == 3 else "short"
    M = S.M_of(proto)
    N = S.interval(kind, M, False, False, True, cfg)[1] - 5
    NP = N + 5
    assert S.pick(kind, M, False, False, False, NP) == S.pick(kind, M, False, False, True, NP) == cfg
    y = S.signal(proto, N, 9700 + cfg)[None, :]
    pk = S.peaks(proto)[None, :]
    shift = np.zeros(1)
    plain, f0 = _call(kind, proto, N, y, pk, False, None, shift=shift)
    ones, f1 = _call(kind, proto, N, y, pk, False, np.ones((1, M)), shift=shift)
    want = S.SWEEP_CFG[cfg] + (0, 0, int(kind == "land"))
    print("%s cfg %d, N = %d: %s and %s" % (kind, cfg, N, f0, f1))
    assert f0 == want + (0,) and f1 == want + (1,)
    plain, ones = (plain,) if kind == "land" else plain, (ones,) if kind == "land" else ones
    for a, b in zip(plain, ones):
        assert np.array_equal(a, b)
    if kind == "post":
        assert plain[2][0] == 0


# ------------------------------------------------------------------------------------------------
# 4. a pair's value does not depend on the configuration
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("csf", [False, True])
def test_landscape_is_the_same_in_every_configuration(csf):
    """A pair's score depends on its own five sums (with CSF eight).  Column statistics are summed over the rows in index
    order by one thread, and the cross term is one chain of KSTEPS = 50 MFMAs over k-steps 0 .. 49 in every (50, ...)
    configuration (the chunk loop differs only in which columns share a chunk and a buffer), so the first 300 rows and
    columns of the landscape are bit-equal between a 300-atom dictionary and one large enough for every later
    configuration of the path."""
    proto, M = "short", S.M_of("short")
    y = S.signal(proto, 300, 9800)[None, :]
    pk = S.peaks(proto)[None, :]
    small, f0 = _call("land", proto, 300, y, pk, csf)
    seen = [f0]
    for c in S.path(M, False, csf)[1:]:
        N = S.interval("land", M, False, csf, False, c)[0] + 11
        big, f = _call("land", proto, N, y, pk, csf)
        seen.append(f)
        sub = big[0, :300, :300]
        ndiff = int((sub != small[0]).sum())
        print("csf=%d: %s at 300 atoms against %s at %d atoms: %d of 90000 pairs differ, max |diff| = %.3g"
              % (csf, f0, f, N, ndiff, float(np.abs(sub - small[0]).max())))
        assert f[:4] == S.SWEEP_CFG[c]
        assert np.array_equal(sub, small[0])
    assert seen[0][:4] == S.SWEEP_CFG[S.path(M, False, csf)[0]] and len(set(seen)) == len(seen)


# ------------------------------------------------------------------------------------------------
# 5. a voxel's result does not depend on the other voxels of the launch
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,proto,cfg", [("post", "short", 2), ("prof", "short", 2), ("post", "long_br", 3), ("prof", "long_br", 3),
                                            ("land", "long_br", 3)])
def test_five_voxels_in_one_launch(kind, proto, cfg):
    """Five voxels with directions of their own in one launch against five single calls, bit for bit, in a (50, 4, 1, 1)
    form and in a bracketed (140, 4, 1, 1) form."""
    from microstructure_fingerprinting_amd import synth
    M, br = S.M_of(proto), S.is_br(proto)
    lo, hi = S.interval(kind, M, br, False, False, cfg)
    N = 293 if lo == 16 else lo + 11
    rng = np.random.default_rng(9600 + cfg)
    pk = np.ascontiguousarray(np.concatenate([synth.unit_vectors(rng, 5), synth.unit_vectors(rng, 5)], axis=1))
    Y = np.stack([S.signal(proto, N, 9610 + v) for v in range(5)])
    shift = np.zeros(5)
    want = S.SWEEP_CFG[cfg] + (int(br), 0, int(kind == "land"), 0)
    together, f = _call(kind, proto, N, Y, pk, False, shift=shift)
    assert f == want
    together = (together,) if kind == "land" else together
    for v in range(5):
        alone, f = _call(kind, proto, N, Y[v:v + 1], pk[v:v + 1], False, shift=shift[:1])
        assert f == want
        alone = (alone,) if kind == "land" else alone
        for a, b in zip(together, alone):
            assert np.array_equal(a[v:v + 1], b), "voxel %d" % v
    if kind == "post":
        assert (together[2] == 0).all()
    print("%s %s N = %d: 5 voxels in one launch equal 5 single calls bit for bit (%s)" % (kind, proto, N, f))


# ------------------------------------------------------------------------------------------------
# 6. one tile above the limit
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("csf", [False, True])
@pytest.mark.parametrize("proto", ["long", "long_br"])
@pytest.mark.parametrize("wgt", [False, True])
@pytest.mark.parametrize("kind", S.KINDS)
def test_one_tile_above_the_limit_raises(kind, wgt, proto, csf):
    M, br = S.M_of(proto), S.is_br(proto)
    limit = S.max_atoms(kind, M, br, csf, wgt)
    N = limit + 16
    assert _limit(kind, proto, N, csf, wgt) == limit
    y = S.pool(S.base(proto))[:, 3][None, :] * 300.0
    before = _form("post" if kind == "post" else "profile")
    with pytest.raises(NotImplementedError, match=r"\b%d\b" % limit):
        _call(kind, proto, N, y, S.peaks(proto)[None, :], csf, np.ones((1, M)) if wgt else None, shift=np.zeros(1))
    assert _form("post" if kind == "post" else "profile") == before   # a refused call launches nothing and records nothing
