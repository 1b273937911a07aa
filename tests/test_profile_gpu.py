"""Objective profiles on the GPU: engine.profile / profile_dev / pair_objectives, MFModelFit.profile / interval.

Referees: (1) a long-double restatement on the host, from the oracle's rotation (orc.interp), of the value of every atom
pair - without CSF the two-variable closed form, with CSF an enumeration of all eight supports of the three unknowns
(independent of the projection the kernel uses); (2) the solver itself on dictionaries restricted to one atom per slot:
the reference's own in tests/golden/profile_cases.npz (tests/golden/gen_golden_profile.py), the oracle's at full size.

The bar.  A Gram quantity summed over M products carries at most M eps |a||b|; carried through the two-atom form
(z1^2 - 2 c z1 z2 + z2^2) / (1 - c^2) (z = d.y / |d|, c the cosine of the atom pair; with CSF of the atoms with the
CSF column projected out) and doubled this bounds a pair's error by 16 M eps ||y||^2 / (1 - c^2).  It is a derived
bound: the float64 NumPy restatement stays below 0.0025 of it on these inputs.

Each test prints what it measures before it asserts; the figures seen on the MI355X are in DESIGN.md 4.12.
"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
Z = np.array([0.0, 0.0, 1.0])
EPS = float(np.finfo(np.float64).eps)
LD = np.longdouble
_cache = {}


def _load(name):
    return np.load(os.path.join(G, name + ".npz"))


def _model(kind):
    """kind: 'small' (fit_cases' 14 atoms), 'c2' (fit_c2_small's 48 atoms), 'ukbb' (986 atoms), 'synth' (782 atoms),
    'synth300' (300 atoms)"""
    import microstructure_fingerprinting_amd as mf
    from microstructure_fingerprinting_amd import synth
    if kind not in _cache:
        if kind == "small":
            d = _load("fit_cases")
            md = {"dictionary": d["dictionary"], "sch_mat": d["sch_ms"], "num_atom": int(d["N"]), "num_ear": int(d["E"]),
                  "T2_csf": float(d["T2_csf"]), "DIFF_csf": float(d["DIFF_csf"]), "T2_ear": float(d["T2_ear"]),
                  "DIFF_ear": d["DIFF_ear"], "rad": d["rad"], "fin": d["fin"]}
        elif kind == "c2":
            d = _load("fit_c2_small")
            md = {"dictionary": d["dictionary"], "sch_mat": d["sch_ms"], "num_atom": d["dictionary"].shape[1], "num_ear": 0,
                  "T2_csf": 2.0, "DIFF_csf": 3.0e-9, "T2_ear": 0.08, "DIFF_ear": np.zeros(0), "rad": d["rad"], "fin": d["fin"]}
        elif kind == "ukbb":
            d = _load("real_ukbb")
            md = {k: d[k] for k in ("dictionary", "sch_mat", "DIFF_ear", "rad", "fin")}
            md.update(num_atom=int(d["num_atom"]), num_ear=int(d["num_ear"]), T2_csf=float(d["T2_csf"]),
                      DIFF_csf=float(d["DIFF_csf"]), T2_ear=float(d["T2_ear"]))
        else:
            N = 300 if kind == "synth300" else 782
            sch, dic, rng = synth.make_model("C2", N=N)
            md = {"dictionary": dic, "sch_mat": sch, "num_atom": N, "num_ear": 3, "T2_csf": 2.0, "DIFF_csf": 3.0e-9,
                  "T2_ear": 0.08, "DIFF_ear": np.array([0.5e-9, 1.0e-9, 1.5e-9]),
                  "rad": np.round(rng.uniform(0.2, 2.0, N), 1) * 1e-6, "fin": np.round(rng.uniform(0.3, 0.9, N), 1)}
        md.update(orientation=Z, fasc_propnames=["rad", "fin"])
        _cache[kind] = mf.MFModel(md)
    return _cache[kind]


def _sch(kind):
    if kind == "small":
        return np.ascontiguousarray(_load("fit_cases")["sch"])
    if kind == "ukbb":
        return np.ascontiguousarray(_load("real_ukbb")["sch_subj"])
    return np.ascontiguousarray(_model(kind).dic["sch_mat"], dtype=np.float64)


def _plan(kind):
    return _model(kind).ms_interpolator.plan_for(_sch(kind))


def _sig_csf(kind):
    return _model(kind)._extra_signals(_sch(kind), True, False)[0]


def _rot(kind, d):
    """the oracle's rotated dictionary [M x N] for one direction"""
    from oracle import oracle as orc
    ms = _model(kind).ms_interpolator
    T = {"S": ms.S, "N": ms.num_subs, "G_un": ms.Gms_un, "off": ms.off, "x": ms.x_flat, "Y": ms.Y_flat,
         "scheme_DeldelTE": ms["scheme_DeldelTE"]}
    out = orc.interp(_sch(kind), d, T)
    return out.reshape(out.shape[0], -1)


def _synth_voxels(kind, V, K, seed, snr=30.0):
    """peaks [V x 3K], Y [V x M] of the synthetic models, through the oracle's rotation"""
    from microstructure_fingerprinting_amd import synth
    rng = np.random.default_rng(seed)
    N = int(_model(kind).dic["num_atom"])
    peaks, Y, _, _ = synth.make_voxels(rng, V, K, lambda d: np.stack([_rot(kind, x) for x in d]), N, snr=snr)
    return np.ascontiguousarray(peaks), np.ascontiguousarray(Y)


# ------------------------------------------------------------------------------------------------
# the long-double referee
# ------------------------------------------------------------------------------------------------
def _gram(y, D0, D1, x=None):
    y, D0, D1 = y.astype(LD), D0.astype(LD), D1.astype(LD)
    g = {"ysq": y @ y, "A11": (D0 * D0).sum(0)[:, None], "A22": (D1 * D1).sum(0)[None, :], "A12": D0.T @ D1,
         "Y1": (D0.T @ y)[:, None], "Y2": (D1.T @ y)[None, :]}
    if x is not None:
        x = x.astype(LD)
        g.update(X1=(D0.T @ x)[:, None], X2=(D1.T @ x)[None, :], xx=x @ x, xy=x @ y)
    return g


def _single(Yv, A):
    return np.maximum(Yv, 0) ** 2 / A


def _pair_inner(A11, A22, A12, Y1, Y2):
    """score of the unconstrained two-atom optimum where both weights are positive, else -inf"""
    d1, d2, Det = A22 * Y1 - A12 * Y2, A11 * Y2 - A12 * Y1, A11 * A22 - A12 * A12
    ok = (d1 > 0) & (d2 > 0) & (Det > 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(ok, (Y1 * d1 + Y2 * d2) / Det, -np.inf)


def _F2(g):
    """(F [N x N], 1 - c^2 [N x N]) of the two-variable problem"""
    s = np.maximum(_pair_inner(g["A11"], g["A22"], g["A12"], g["Y1"], g["Y2"]),
                   np.maximum(_single(g["Y1"], g["A11"]), _single(g["Y2"], g["A22"])))
    return g["ysq"] - s, 1 - g["A12"] ** 2 / (g["A11"] * g["A22"])


def _F3(g):
    """(F [N x N], 1 - c'^2) with the CSF weight as a third unknown: the best of all eight supports whose unconstrained
    optimum has positive weights (a feasible point each, the NNLS optimum among them)."""
    A11, A22, A12, Y1, Y2, X1, X2, xx, xy = (g[k] for k in ("A11", "A22", "A12", "Y1", "Y2", "X1", "X2", "xx", "xy"))
    s = np.maximum(_single(Y1, A11), _single(Y2, A22))
    s = np.maximum(s, _single(xy, xx))
    s = np.maximum(s, _pair_inner(A11, A22, A12, Y1, Y2))
    s = np.maximum(s, _pair_inner(A11, xx, X1, Y1, xy))
    s = np.maximum(s, _pair_inner(A22, xx, X2, Y2, xy))
    # all three: Cramer's rule on [[A11 A12 X1] [A12 A22 X2] [X1 X2 xx]] w = [Y1 Y2 xy]
    c00, c01, c02 = A22 * xx - X2 * X2, X1 * X2 - A12 * xx, A12 * X2 - A22 * X1
    c11, c12, c22 = A11 * xx - X1 * X1, A12 * X1 - A11 * X2, A11 * A22 - A12 * A12
    det = A11 * c00 + A12 * c01 + X1 * c02
    w1 = c00 * Y1 + c01 * Y2 + c02 * xy
    w2 = c01 * Y1 + c11 * Y2 + c12 * xy
    w3 = c02 * Y1 + c12 * Y2 + c22 * xy
    ok = (det > 0) & (w1 > 0) & (w2 > 0) & (w3 > 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        s = np.maximum(s, np.where(ok, (Y1 * w1 + Y2 * w2 + xy * w3) / det, -np.inf))
    A11p, A22p, A12p = A11 - X1 * X1 / xx, A22 - X2 * X2 / xx, A12 - X1 * X2 / xx
    return g["ysq"] - s, 1 - A12p ** 2 / (A11p * A22p)


def _referee(kind, y, pk, csf):
    """(F [N x N] long double, 1 - c^2 [N x N], ||y||^2) of one two-fascicle voxel"""
    g = _gram(y, _rot(kind, pk[:3]), _rot(kind, pk[3:6]), _sig_csf(kind) if csf else None)
    F, c2 = _F3(g) if csf else _F2(g)
    return F, c2, float(g["ysq"])


def _cut():
    from microstructure_fingerprinting_amd import _lib
    cut = float(_lib.lib().mfx_profile_cut())
    assert 0 < cut <= 1e-6
    return cut


def _two_fascicle_voxels(kind):
    if kind == "c2":
        d = _load("fit_c2_small")
        return np.ascontiguousarray(d["peaks"]), np.ascontiguousarray(d["Y"])
    if kind == "ukbb":
        d = _load("real_ukbb_fit_k2")
        return np.ascontiguousarray(d["peaks"][:3]), np.ascontiguousarray(d["Y"][:3])
    return _synth_voxels("synth", 3, 2, seed=101)


# ------------------------------------------------------------------------------------------------
# 1. every pair against the referee (landscape mode)
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("csf", [False, True])
@pytest.mark.parametrize("kind", ["c2", "synth", "ukbb"])
def test_every_pair_against_the_referee(kind, csf):
    """|F_kernel - F_referee| <= 16 M eps ||y||^2 / (1 - c^2) for every atom pair; none of these inputs has a pair below
    the cut.  Measured on the MI355X: see DESIGN.md 4.12."""
    from microstructure_fingerprinting_amd import engine
    peaks, Y = _two_fascicle_voxels(kind)
    M = Y.shape[1]
    got = engine.pair_objectives(_plan(kind), Y, peaks, csf, _sig_csf(kind) if csf else None)
    cut, worst, c2min = _cut(), 0.0, 1.0
    for v in range(Y.shape[0]):
        F, c2, ysq = _referee(kind, Y[v], peaks[v], csf)
        bar = 16 * M * EPS * ysq / c2
        err = np.abs(got[v].astype(LD) - F)
        worst, c2min = max(worst, float(np.max(err / bar))), min(c2min, float(c2.min()))
        print("%s csf=%d voxel %d: max |F - F_ref| = %.3g ||y||^2, worst err / bar = %.3g, smallest 1 - c^2 = %.3g"
              % (kind, csf, v, float(err.max() / ysq), float(np.max(err / bar)), float(c2.min())))
        assert c2.min() > cut, "a pair below the cut: this input was chosen to have none"
        assert np.all(err <= bar)
    print("%s csf=%d: worst err / bar over all voxels = %.3g (smallest 1 - c^2 = %.3g)" % (kind, csf, worst, c2min))


# ------------------------------------------------------------------------------------------------
# 2. profiles against the solver
# ------------------------------------------------------------------------------------------------
def _voxel_bar(kind, y, pk, K, csf):
    """(16 M eps ||y||^2 / min(1 - c^2) of the voxel, referee F or None)"""
    ysq = float(y @ y)
    if K == 1:
        return 16 * y.shape[0] * EPS * ysq, None
    F, c2, _ = _referee(kind, y, pk, csf)
    return 16 * y.shape[0] * EPS * ysq / float(c2.min()), F


@pytest.mark.parametrize("cname", ["fit_c2_small", "fit_cases_k1", "fit_cases"])
def test_profile_reproduces_the_reference_solver(cname):
    """obj and partner against the reference's solve_exhaustive_posweights on [a_i | D_other (| x)] (golden file), every
    entry: values within 16 M eps ||y||^2 / min(1 - c^2); partner equal, or the referee's value at the kernel's partner
    within the same bar of the row's minimum."""
    from microstructure_fingerprinting_amd import engine
    g = _load("profile_cases")
    kind = "c2" if cname == "fit_c2_small" else "small"
    d = _load(cname)
    vox, K, csf = g[cname + "_vox"], g[cname + "_K"], g[cname + "_csf"]
    maxfasc = g[cname + "_obj"].shape[1]
    Y = np.ascontiguousarray(d["Y"][vox])
    peaks = np.ascontiguousarray(d["peaks"][vox][:, :3 * maxfasc])
    obj, par, n_uns = engine.profile(_plan(kind), Y, K, csf, peaks, maxfasc, bool(csf.any()), _sig_csf(kind) if csf.any() else None,
                                     partner=True)
    assert n_uns == 0 and obj.shape == g[cname + "_obj"].shape
    worst, nmis = 0.0, 0
    for r in range(vox.size):
        k = int(K[r])
        bar, F = _voxel_bar(kind, Y[r], peaks[r], k, bool(csf[r]))
        ref, rpar = g[cname + "_obj"][r, :k], g[cname + "_partner"][r, :k]
        err = np.abs(obj[r, :k] - ref)
        worst = max(worst, float(err.max() / bar))
        assert np.all(err <= bar), "voxel %d: %.3g of the bar" % (vox[r], float(err.max() / bar))
        assert np.all(np.isnan(obj[r, k:])) and np.all(par[r, k:] == -1)
        if k == 1:
            assert np.all(par[r, 0] == -1)
            continue
        for s in range(2):
            Fs = F if s == 0 else F.T
            mis = np.flatnonzero(par[r, s] != rpar[s])
            nmis += mis.size
            at = Fs[mis, par[r, s, mis]] - Fs[mis].min(axis=1)
            assert np.all(at <= bar), "voxel %d slot %d: a partner that is not a minimiser" % (vox[r], s)
    print("%s: worst |obj - reference| / bar = %.3g over %d voxels; %d partners differ (all tie within the bar)"
          % (cname, worst, vox.size, nmis))


@pytest.mark.parametrize("csf", [False, True])
@pytest.mark.parametrize("K", [1, 2])
@pytest.mark.parametrize("kind", ["synth", "ukbb"])
def test_profile_against_the_oracle_solver_at_full_size(kind, K, csf):
    """64 sampled (voxel, slot, atom) triples per class at 782 and 986 atoms: the oracle's solve_exhaustive_posweights
    on the dictionary restricted to that atom against obj / partner."""
    from microstructure_fingerprinting_amd import engine
    from oracle import oracle as orc
    if kind == "ukbb":
        d = _load("real_ukbb_fit_k2")
        peaks, Y = np.ascontiguousarray(d["peaks"][:, :3 * K]), np.ascontiguousarray(d["Y"])
    else:
        peaks, Y = _synth_voxels("synth", 4, K, seed=202 + K)
    V, M = Y.shape
    x = _sig_csf(kind) if csf else None
    obj, par, n_uns = engine.profile(_plan(kind), Y, np.full(V, K), np.full(V, csf), peaks, K, csf, x, partner=True)
    N = obj.shape[2]
    assert n_uns == 0 and obj.shape == (V, K, N)
    rng = np.random.default_rng(7)
    worst, nmis = 0.0, 0
    bars, Fs, Ds = {}, {}, {}
    for _ in range(64):
        v, s, i = int(rng.integers(V)), int(rng.integers(K)), int(rng.integers(N))
        if v not in bars:
            bars[v], Fs[v] = _voxel_bar(kind, Y[v], peaks[v], K, csf)
            Ds[v] = [_rot(kind, peaks[v, 3 * k:3 * k + 3]) for k in range(K)]
        cols, sizes = [None] * K, [N] * K
        cols[s], sizes[s] = Ds[v][s][:, i:i + 1], 1
        if K == 2:
            cols[1 - s] = Ds[v][1 - s]
        A = np.ascontiguousarray(np.concatenate(cols + ([x[:, None]] if csf else []), axis=1))
        w, sub, tot, mo, yrec = orc.solve_exhaustive_posweights(A, Y[v], np.array(sizes + [1] * int(csf)))
        err = abs(obj[v, s, i] - mo)
        worst = max(worst, err / bars[v])
        assert err <= bars[v], "voxel %d slot %d atom %d: |obj - oracle| = %.3g of the bar" % (v, s, i, err / bars[v])
        if K == 2 and par[v, s, i] != sub[1 - s]:
            nmis += 1
            F = Fs[v] if s == 0 else Fs[v].T
            assert F[i, par[v, s, i]] - F[i].min() <= bars[v]
        if K == 1:
            assert par[v, s, i] == -1
    print("%s K=%d csf=%d: worst |obj - oracle| / bar = %.3g over 64 triples; %d partners differ (ties within the bar)"
          % (kind, K, csf, worst, nmis))


# ------------------------------------------------------------------------------------------------
# 3. near-parallel fascicles
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("deg", [0.0, 0.05, 0.5, 3.0])
def test_near_parallel_fascicles(deg):
    """Crossing angles down to 0 with the same atom in both slots among the candidates: pairs below the cut are scored
    as single atoms, an upper bound.  lo - bar <= obj <= hi + bar with lo the long-double minimum over all pairs of the
    row and hi the one over the pairs above the cut and the atom alone; the bar is the pair bound at the worst
    conditioned pair that is above the cut."""
    from microstructure_fingerprinting_amd import engine, synth
    kind, cut = "synth300", _cut()
    rng = np.random.default_rng(31)
    p1 = synth.unit_vectors(rng, 1)[0]
    ax = np.cross(p1, [0.3, -0.5, 0.8])
    ax /= np.linalg.norm(ax)
    th = np.deg2rad(deg)
    p2 = p1 * np.cos(th) + ax * np.sin(th)
    D0, D1 = _rot(kind, p1), _rot(kind, p2)
    M, N = D0.shape
    Y = np.stack([300.0 * D0[:, 17] + 200.0 * D1[:, 17] + rng.normal(0, 10, M),      # the same atom in both slots
                  250.0 * D0[:, 5] + 250.0 * D1[:, 140] + rng.normal(0, 10, M),
                  400.0 * D0[:, 77]])                                                   # one atom, no noise
    peaks = np.tile(np.concatenate([p1, p2]), (3, 1))
    obj, par, _ = engine.profile(_plan(kind), Y, np.full(3, 2), None, peaks, 2, False, None, partner=True)
    nbelow = 0
    for v in range(3):
        g = _gram(Y[v], D0, D1)
        F, c2 = _F2(g)
        ysq = float(g["ysq"])
        above = c2 > cut
        nbelow += int((~above).sum())
        bar = 16 * M * EPS * ysq / float(c2[above].min())
        alone0, alone1 = (g["ysq"] - _single(g["Y1"], g["A11"]))[:, 0], (g["ysq"] - _single(g["Y2"], g["A22"]))[0]
        Fa = np.where(above, F, np.inf)
        for s, (lo, hi) in enumerate(((F.min(1), np.minimum(Fa.min(1), alone0)), (F.min(0), np.minimum(Fa.min(0), alone1)))):
            o = obj[v, s].astype(LD)
            print("%.2f deg voxel %d slot %d: max (lo - obj) / bar = %.3g, max (obj - hi) / bar = %.3g, max (hi - lo) = %.3g "
                  "||y||^2, bar = %.3g ||y||^2" % (deg, v, s, float(np.max(lo - o) / bar), float(np.max(o - hi) / bar),
                                                    float(np.max(hi - lo) / ysq), bar / ysq))
            assert np.all(lo - bar <= o) and np.all(o <= hi + bar)
    print("%.2f deg: %d of %d pairs below the cut %.1g" % (deg, nbelow, 3 * N * N, cut))
    if deg == 0.0:
        assert nbelow >= 3 * N      # the diagonal at least


# ------------------------------------------------------------------------------------------------
# 4. agreement with the fit
# ------------------------------------------------------------------------------------------------
def _min_c2_dev(plan, d_pk, N):
    """smallest 1 - c^2 over the atom pairs of every two-fascicle voxel, on the device (float64; for the bar only)"""
    import torch
    from microstructure_fingerprinting_amd import _lib as L
    V, M = d_pk.shape[0], plan.M
    out = torch.empty(V, dtype=torch.float64, device=d_pk.device)
    st = torch.cuda.current_stream(d_pk.device).cuda_stream
    for i0 in range(0, V, 64):
        pk = d_pk[i0:i0 + 64]
        D = []
        for k in range(2):
            d = pk[:, 3 * k:3 * k + 3].contiguous()
            o = torch.empty((d.shape[0], M, N), dtype=torch.float64, device=d_pk.device)
            L.check(L.lib().mfx_rotate_dev(plan.handle(), d.data_ptr(), d.shape[0], 0, o.data_ptr(), st))
            D.append(o / o.norm(dim=1, keepdim=True))
        c = torch.bmm(D[0].transpose(1, 2), D[1])
        out[i0:i0 + 64] = (1 - c * c).amin(dim=(1, 2))
    return out.cpu().numpy()


def _check_against_fit(tag, obj, params, K, M, bars, ysq):
    """argmin obj[k] == fitted ID where the runner-up is further than the bar away; min obj == MSE * M within the bar"""
    V, nf = obj.shape[:2]
    nid = ntie = 0
    worst = 0.0
    for v in range(V):
        for k in range(int(K[v])):
            o = obj[v, k]
            order = np.argsort(o, kind="stable")
            dev = abs(o[order[0]] - params[v, -2] * M)
            worst = max(worst, dev / bars[v])
            assert dev <= bars[v], "%s voxel %d: |min obj - MSE M| = %.3g of the bar" % (tag, v, dev / bars[v])
            if o.size > 1 and o[order[1]] - o[order[0]] <= bars[v]:
                ntie += 1
                continue
            nid += 1
            assert order[0] == int(params[v, 1 + nf + k]), "%s voxel %d fascicle %d" % (tag, v, k)
    print("%s: worst |min obj - MSE M| / bar = %.3g; %d fitted IDs equal the profile's arg-min, %d rows with a runner-up "
          "within the bar left out" % (tag, worst, nid, ntie))
    return nid


@pytest.mark.parametrize("cname", ["fit_c2_small", "fit_cases_k1", "fit_cases", "real_ukbb_fit_k2", "real_ukbb_fit_k2csf"])
def test_profile_agrees_with_the_fit_on_the_fixtures(cname):
    """Every fixture class in scope: arg-min and minimum against the fit; profile mode against the row and column minima
    of landscape mode; EAR and fascicle-free voxels give NaN rows and are counted."""
    from microstructure_fingerprinting_amd import engine
    kind = {"fit_c2_small": "c2", "fit_cases_k1": "small", "fit_cases": "small"}.get(cname, "ukbb")
    d = _load(cname)
    Y = np.ascontiguousarray(d["Y"])
    V, M = Y.shape
    if cname == "fit_cases":
        K, csf, ear, maxfasc = d["numfasc"].astype(int), d["csf"] > 0, d["ear"] > 0, 2
    elif cname == "fit_cases_k1":
        K, csf, ear, maxfasc = np.ones(V, int), np.zeros(V, bool), np.zeros(V, bool), 1
    else:
        c = bool(int(d["csf"])) if "csf" in d.files else False
        K, csf, ear, maxfasc = np.full(V, 2), np.full(V, c), np.zeros(V, bool), 2
    peaks = np.ascontiguousarray(d["peaks"][:, :3 * maxfasc])
    csf_on, ear_on = bool(csf.any()), bool(ear.any())
    model, sch = _model(kind), _sch(kind)
    plan = _plan(kind)
    sig_csf, sig_ear, E = model._extra_signals(sch, csf_on, ear_on)
    params = engine.fit_batch(plan, Y, K, csf, ear, peaks, maxfasc, csf_on, ear_on, sig_csf, sig_ear, E)
    obj, par, n_uns = engine.profile(plan, Y, K, csf, peaks, maxfasc, csf_on, sig_csf, partner=True, ear=ear)
    scope = (K >= 1) & ~ear
    print("%s: %d voxels, %d out of scope" % (cname, V, int((~scope).sum())))
    assert n_uns == int((~scope).sum())
    assert np.all(np.isnan(obj[~scope])) and np.all(par[~scope] == -1)
    assert not np.isnan(obj[scope, 0]).any()
    bars, ysq = np.zeros(V), np.sum(Y * Y, axis=1)
    for v in np.flatnonzero(scope):
        bars[v], _ = _voxel_bar(kind, Y[v], peaks[v], int(K[v]), bool(csf[v]))
    # the fit's parameter rows of the voxels in scope have the layout of the whole class (EAR columns included)
    idx = np.flatnonzero(scope)
    _check_against_fit(cname, obj[idx], params[idx][:, list(range(1 + 2 * maxfasc)) + [-2, -1]], K[idx], M, bars[idx], ysq[idx])
    two = np.flatnonzero(scope & (K == 2))
    for c in (False, True):
        sel = two[csf[two] == c][:3]
        if not sel.size:
            continue
        land = engine.pair_objectives(plan, Y[sel], peaks[sel], c, sig_csf if c else None)
        for r, v in enumerate(sel):
            d0 = np.abs(land[r].min(axis=1) - obj[v, 0]).max()
            d1 = np.abs(land[r].min(axis=0) - obj[v, 1]).max()
            print("%s voxel %d csf=%d: profile vs landscape minima: %.3g, %.3g of the bar" % (cname, v, c, d0 / bars[v], d1 / bars[v]))
            assert d0 <= bars[v] and d1 <= bars[v]


@pytest.mark.parametrize("csf", [False, True])
def test_profile_agrees_with_the_fit_on_2000_synthetic_voxels(csf):
    import torch
    from microstructure_fingerprinting_amd import engine
    kind = "synth"
    plan, N = _plan(kind), 782
    rng = np.random.default_rng(404)
    V, M = 2000, plan.M
    from microstructure_fingerprinting_amd import synth
    dev = torch.device("cuda", 0)
    peaks = np.concatenate([synth.unit_vectors(rng, V), synth.unit_vectors(rng, V)], axis=1)
    atoms = rng.integers(0, N, (V, 2)).astype(np.int32)
    nu = rng.dirichlet(np.ones(3 if csf else 2), V)
    d_pk = torch.from_numpy(peaks).to(dev)
    d_Y = torch.zeros((V, M), dtype=torch.float64, device=dev)
    for k in range(2):
        col = engine.rotate_columns_dev(plan, d_pk[:, 3 * k:3 * k + 3].contiguous(), torch.from_numpy(atoms[:, k].copy()).to(dev))
        d_Y += 500.0 * torch.from_numpy(nu[:, k:k + 1].copy()).to(dev) * col
    d_x = torch.from_numpy(np.ascontiguousarray(_sig_csf(kind))).to(dev)
    if csf:
        d_Y += 500.0 * torch.from_numpy(nu[:, 2:3].copy()).to(dev) * d_x[None, :]
    d_Y += torch.from_numpy(rng.normal(0, 500.0 / 30.0, (V, M))).to(dev)
    d_Y = d_Y.contiguous()
    params = engine.fit_batch_dev(plan, d_Y, d_pk, 2, csf_on=csf, d_sig_csf=d_x if csf else None).cpu().numpy()
    obj, par = engine.profile_dev(plan, d_Y, d_pk, 2, csf, d_x if csf else None, partner=True)
    torch.cuda.synchronize()
    assert tuple(obj.shape) == (V, 2, N) and par.dtype == torch.int32
    ysq = (d_Y * d_Y).sum(dim=1).cpu().numpy()
    bars = 16 * M * EPS * ysq / _min_c2_dev(plan, d_pk, N)
    o, p = obj.cpu().numpy(), par.cpu().numpy()
    nid = _check_against_fit("synthetic csf=%d" % csf, o, params[:, [0, 1, 2, 3, 4, -2, -1]], np.full(V, 2), M, bars, ysq)
    assert nid >= 0.9 * 2 * V
    # the partner of the best atom of slot 0 is the best atom of slot 1 (and back) wherever the optimum is unique
    b0 = o[:, 0].argmin(axis=1)
    b1 = o[:, 1].argmin(axis=1)
    uniq = (np.partition(o[:, 0], 1, axis=1)[:, 1] - o[:, 0].min(axis=1) > bars) & \
           (np.partition(o[:, 1], 1, axis=1)[:, 1] - o[:, 1].min(axis=1) > bars)
    assert np.array_equal(p[uniq, 0, b0[uniq]], b1[uniq]) and np.array_equal(p[uniq, 1, b1[uniq]], b0[uniq])
    assert (p >= 0).all() and (p < N).all()


# ------------------------------------------------------------------------------------------------
# 5. a mixed volume through MFModelFit.interval
# ------------------------------------------------------------------------------------------------
def test_interval_over_a_mixed_phantom():
    from microstructure_fingerprinting_amd import engine, synth
    from microstructure_fingerprinting_amd import mf_utils as U
    import microstructure_fingerprinting_amd.mf as mfmod
    model = _model("small")
    rng = np.random.default_rng(55)
    ph = synth.make_phantom(model, (7, 6, 5), rng)
    sch = np.ascontiguousarray(model.dic["sch_mat"], dtype=np.float64)
    fit = model.fit(ph["data"], ph["mask"], ph["numfasc"], peaks=ph["peaks"], pgse_scheme=sch, csf_mask=ph["csf_mask"],
                    ear_mask=ph["ear_mask"], verbose=0)
    N = int(model.dic["num_atom"])
    roi = np.flatnonzero(ph["mask"].reshape(-1))
    R = roi.size
    Y = np.asarray(ph["data"].reshape(-1, sch.shape[0])[roi], dtype=np.float64)
    K = ph["numfasc"].reshape(-1)[roi].astype(int)
    csf, ear = ph["csf_mask"].reshape(-1)[roi] > 0, ph["ear_mask"].reshape(-1)[roi] > 0
    pk = ph["peaks"].reshape(-1, 6)[roi]
    plan = model.ms_interpolator.plan_for(sch)
    sig_csf = model._extra_signals(sch, True, False)[0]
    obj, _, n_uns = engine.profile(plan, Y, K, csf, pk, 2, True, sig_csf, ear=ear)
    scope = (K >= 1) & ~ear
    assert n_uns == int((~scope).sum()) and 0 < n_uns < R
    prof = fit.profile(ph["data"], partner=True)
    assert prof.n_unsupported == n_uns and np.array_equal(prof.obj, obj, equal_nan=True)
    lv, by = prof.by_property("rad")
    assert by.shape == (R, 2, lv.size) and np.array_equal(by, U.profile_by_property(obj, model.dic["rad"])[1], equal_nan=True)
    sub = fit.profile(ph["data"], voxels=[5, 2, 11])
    assert np.array_equal(sub.obj, obj[[5, 2, 11]], equal_nan=True) and sub.partner is None
    old = mfmod.MFModelFit.PROFILE_BYTES
    mfmod.MFModelFit.PROFILE_BYTES = 16 * N * 7     # 7 voxels per chunk: several chunks per class
    try:
        for name, rel, delta in (("rad", 0.0, 0.0), ("fin", 0.05, 0.0), ("rad", 0.0, 25.0)):
            lo, hi, cnt = fit.interval(ph["data"], name, rel=rel, delta=delta)
            assert lo.shape == ph["mask"].shape + (2,) and cnt.dtype.kind == "i"
            rl, rh, rc = U.profile_interval(obj, model.dic[name], rel, delta)
            flat = lambda a: a.reshape(-1, 2)[roi]   # noqa: E731
            assert np.array_equal(flat(lo), rl, equal_nan=True) and np.array_equal(flat(hi), rh, equal_nan=True)
            assert np.array_equal(flat(cnt), rc)
            outside = np.setdiff1d(np.arange(ph["mask"].size), roi)
            assert np.all(np.isnan(lo.reshape(-1, 2)[outside])) and np.all(cnt.reshape(-1, 2)[outside] == 0)
            print("interval(%s, rel=%g, delta=%g): %d voxels, mean count %.2f" % (name, rel, delta, R, rc[scope, 0].mean()))
            if rel == 0.0 and delta == 0.0:
                # where the optimum is unique beyond rounding, the range collapses onto the fitted property map
                ysq = np.sum(Y * Y, axis=1)
                nchk = 0
                for k in range(2):
                    fmap = getattr(fit, "%s_f%d" % (name, k)).reshape(-1)[roi]
                    frac = getattr(fit, "frac_f%d" % k).reshape(-1)[roi]
                    for v in np.flatnonzero(scope & (K > k) & (frac > 0)):
                        bar, _ = _voxel_bar("small", Y[v], pk[v], int(K[v]), bool(csf[v]))
                        o = np.sort(obj[v, k])
                        if o[1] - o[0] > bar:
                            nchk += 1
                            assert rc[v, k] == 1 and rl[v, k] == rh[v, k] == fmap[v]
                print("rel = 0: lo == hi == fitted %s in %d (voxel, fascicle) rows with a unique optimum" % (name, nchk))
                assert nchk > 0
    finally:
        mfmod.MFModelFit.PROFILE_BYTES = old


# ------------------------------------------------------------------------------------------------
# 6. the device entry point
# ------------------------------------------------------------------------------------------------
def test_dev_entry_only_enqueues_streams_and_threads():
    """Four mfx_profile_dev calls on one stream return long before the first has finished and give the bits of a call
    made alone; so does a call on a non-default torch stream, and two host threads on one device."""
    import threading
    import time
    import torch
    from microstructure_fingerprinting_amd import _lib as L
    from microstructure_fingerprinting_amd import engine
    kind = "synth"
    plan, N = _plan(kind), 782
    dev = torch.device("cuda", 0)
    V = 6000
    pk0, Y0 = _synth_voxels("synth", 8, 2, seed=66)
    rng = np.random.default_rng(67)
    rep = V // 8
    Y = np.tile(Y0, (rep, 1)) + rng.normal(0, 5.0, (V, Y0.shape[1]))
    d_Y, d_pk = torch.from_numpy(Y).to(dev), torch.from_numpy(np.tile(pk0, (rep, 1))).to(dev)
    alone = engine.profile_dev(plan, d_Y, d_pk, 2)
    torch.cuda.synchronize()
    outs = [torch.zeros_like(alone) for _ in range(4)]
    lib, st = L.lib(), torch.cuda.current_stream(dev).cuda_stream
    t0 = time.perf_counter()
    for o in outs:
        L.check(lib.mfx_profile_dev(plan.handle(), d_Y.data_ptr(), d_pk.data_ptr(), 2, 0, None, V, o.data_ptr(), None, st))
    t_host = time.perf_counter() - t0
    torch.cuda.synchronize()
    t_all = time.perf_counter() - t0
    print("4 calls enqueued in %.2f ms, finished after %.1f ms" % (t_host * 1e3, t_all * 1e3))
    assert t_host < 0.25 * t_all, "the device entry point blocked: %.1f ms of %.1f ms on the host" % (t_host * 1e3, t_all * 1e3)
    for o in outs:
        assert torch.equal(o, alone)
    s = torch.cuda.Stream(device=dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        other, opar = engine.profile_dev(plan, d_Y[:500].contiguous(), d_pk[:500].contiguous(), 2, partner=True)
    s.synchronize()
    assert torch.equal(other, alone[:500])
    host = engine.profile(plan, Y[:40], np.full(40, 2), None, d_pk[:40].cpu().numpy(), 2, False, None, partner=True)
    assert np.array_equal(host[0], alone[:40].cpu().numpy()) and np.array_equal(host[1], opar[:40].cpu().numpy())
    got, errs = [None, None], []

    def work(t):
        try:
            got[t] = engine.profile(plan, Y[:300], np.full(300, 2), None, d_pk[:300].cpu().numpy(), 2, False, None)[0]
        except Exception as e:   # noqa: BLE001 (reported below)
            errs.append(e)
    th = [threading.Thread(target=work, args=(t,)) for t in range(2)]
    for x in th:
        x.start()
    for x in th:
        x.join()
    assert not errs, errs
    ref = alone[:300].cpu().numpy()
    assert np.array_equal(got[0], ref) and np.array_equal(got[1], ref)


def test_limits_are_reported():
    from microstructure_fingerprinting_amd import _lib as L
    plan = _plan("synth")
    lib = L.lib()
    n = [lib.mfx_profile_max_atoms(plan.handle(), c, l) for c in (0, 1) for l in (0, 1)]
    print("largest dictionary for M = 200 (profile, landscape, CSF profile, CSF landscape): %s" % n)
    assert min(n) >= 986
    bad = np.array([[0.0, 0.0, 1.3, 1.0, 0.0, 0.0]])
    pk0, Y0 = _synth_voxels("synth", 1, 2, seed=5)
    from microstructure_fingerprinting_amd import engine
    with pytest.raises(ValueError):
        engine.profile(plan, Y0, np.array([2]), None, bad, 2, False, None)
    assert np.isfinite(engine.profile(plan, Y0, np.array([2]), None, pk0, 2, False, None)[0]).all()
