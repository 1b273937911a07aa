"""Bootstrap on the GPU (include/mfx_boot.h) against its NumPy restatement (tests/_boot_ref.py), the plain fit and the
CPU oracle, on the dictionary and protocol of tests/golden/fit_cases.npz (14 atoms, 64 measurements - exactly one wave's
worth of rows, so the resampling kernel is also run on rows of 101 and 37 entries, which needs no protocol).  Seven
voxels of every class: K = 0 + CSF, K = 1 + EAR, three plain K = 2 (one class with several voxels, so that it can be cut
into chunks), K = 2 + CSF + EAR, K = 3.  That the replicates do move the fit is checked on the CPU in
tests/test_boot_host.py (the power condition)."""
import numpy as np
import pytest

import _boot_ref as R

pytestmark = pytest.mark.gpu

SEED = 1
Q = (0.0, 0.025, 0.5, 0.975, 1.0)


class Case:
    pass


@pytest.fixture(scope="module")
def case():
    from microstructure_fingerprinting_amd import engine
    from microstructure_fingerprinting_amd import mf_utils as mfu
    from oracle import oracle as orc
    c = Case()
    c.d, c.sch, c.sig_csf, c.sig_ear = R.golden_model()
    d = c.d
    c.E, c.N, c.M, c.F = int(d["E"]), int(d["N"]), c.sch.shape[0], 3
    c.T = orc.init_tables(d["dictionary"], d["sch_ms"], R.Z)
    c.ms = mfu.init_PGSE_multishell_interp(d["dictionary"], d["sch_ms"], R.Z)
    c.plan = c.ms.plan_for(c.sch)
    idx = np.array([18, 13, 0, 7, 8, 2, 4])
    c.K = np.array([0, 1, 2, 2, 2, 2, 3], dtype=np.int32)
    assert np.array_equal(d["numfasc"][idx[:6]], c.K[:6]) and d["numfasc"][4] == 2
    c.csf, c.ear = d["csf"][idx].copy(), d["ear"][idx].copy()
    assert list(c.csf) == [True, False, False, False, False, True, False] and list(c.ear) == [False, True, False, False, False, True, False]
    c.V = idx.size
    c.Y = np.ascontiguousarray(d["Y"][idx])
    c.peaks = np.zeros((c.V, 9))
    c.peaks[:, :6] = d["peaks"][idx]
    third = np.cross(c.peaks[6, :3], c.peaks[6, 3:6])
    c.peaks[6, 6:] = third / np.linalg.norm(third)
    c.props = np.stack([d["rad"], d["fin"]])
    c.args = (c.K, c.csf, c.ear, c.peaks, 3, True, True, c.sig_csf, c.sig_ear, c.E)
    c.P0 = engine.fit_batch(c.plan, c.Y, *c.args)
    c.pred = engine.predict(c.plan, c.P0, c.peaks, 3, True, True, c.sig_csf, c.sig_ear, c.E)
    c.groups = engine.boot_groups(c.sch)
    assert len(np.unique(c.groups)) > 1
    c._ref = {}
    return c


def ref_ystar(c, B, kind, inflate, offset=0, groups=None):
    """The restatement's replicates of the seven voxels, computed once per setting and never changed."""
    key = (B, kind, inflate, offset, None if groups is None else groups.tobytes())
    if key not in c._ref:
        g = (c.groups if groups is None else groups) if kind == 1 else None
        Ys, st = R.resample(c.Y, c.pred, c.P0, 3, True, True, B, kind, SEED, inflate, offset, g)
        Ys.setflags(write=False)
        c._ref[key] = (Ys, st)
    return c._ref[key]


def same(a, b):
    return np.array_equal(a, b, equal_nan=True)


@pytest.mark.parametrize("B", [1, 5, 65])
@pytest.mark.parametrize("kind", ["wild", "residual"])
def test_resample_equals_the_restatement(case, B, kind):
    """mfx_boot_resample_dev bit for bit: inflate on and off, the default groups and a hand-made vector with a group of
    one row, an index that crosses into its high word, the peaks copied to every replicate row, a NaN prediction row."""
    import torch
    from microstructure_fingerprinting_amd import engine
    c = case
    dev = torch.device("cuda", 0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    code = engine.BOOT_KINDS[kind]
    hand = (np.arange(c.M) % 5).astype(np.int32)
    hand[17] = -3                                           # a group of one row
    settings = [(True, 0, None), (False, 0, None)]
    if code == 1:
        settings.append((True, 0, hand))
    if B == 5:
        settings.append((True, 2 ** 32 - 3, None))          # idx = offset + v M + m crosses 2^32 in the first voxel
    for inflate, offset, groups in settings:
        g = (c.groups if groups is None else groups) if code == 1 else None
        Ys, pk, st = engine.boot_resample_dev(t(c.Y), t(c.pred), t(c.P0), 3, True, True, B, kind, SEED, inflate, offset,
                                              t(g) if g is not None else None, t(c.peaks))
        want, wst = ref_ystar(c, B, code, inflate, offset, groups)
        assert np.array_equal(st.cpu().numpy(), wst) and not wst.any()
        got = Ys.cpu().numpy()
        bad = np.argwhere(got != want)
        assert bad.size == 0, (inflate, offset, bad[:5])
        assert np.array_equal(pk.cpu().numpy(), np.repeat(c.peaks, B, axis=0))
    if B == 5:
        assert not same(ref_ystar(c, B, code, True)[0], ref_ystar(c, B, code, False)[0])     # the scale does something
        P = c.pred.copy()
        P[3, 11] = np.nan
        Ys, _, st = engine.boot_resample_dev(t(c.Y), t(P), t(c.P0), 3, True, True, B, kind, SEED, True,
                                             d_groups=t(c.groups) if code == 1 else None)
        got, want = Ys.cpu().numpy(), ref_ystar(c, B, code, True)[0]
        assert list(st.cpu().numpy()) == [0, 0, 0, 2, 0, 0, 0] and np.all(np.isnan(got[3])) and np.array_equal(np.delete(got, 3, 0), np.delete(want, 3, 0))
        # a subset with its batch indices gives the whole batch's replicates
        sub = np.array([5, 1, 6])
        Ys, _, _ = engine.boot_resample_dev(t(c.Y[sub]), t(c.pred[sub]), t(c.P0[sub]), 3, True, True, B, kind, SEED, True,
                                            d_groups=t(c.groups) if code == 1 else None, d_vox=t(sub.astype(np.int64)))
        assert np.array_equal(Ys.cpu().numpy(), want[sub])
        # rows that are no multiple of the wave: 101 entries (two passes, the second ragged) and 37 (less than a wave)
        for Mr in (101, 37):
            Yr = np.ascontiguousarray(np.concatenate([c.Y, c.Y[:, ::-1]], axis=1)[:, :Mr])
            Pr = np.ascontiguousarray(np.concatenate([c.pred, c.pred[:, ::-1]], axis=1)[:, :Mr])
            gr = (np.arange(Mr) % 7).astype(np.int32)
            gr[Mr - 1] = 99
            Ys, _, st = engine.boot_resample_dev(t(Yr), t(Pr), t(c.P0), 3, True, True, B, kind, SEED, True, 2 ** 32 - 50,
                                                 d_groups=t(gr) if code == 1 else None)
            wr, wst = R.resample(Yr, Pr, c.P0, 3, True, True, B, code, SEED, True, 2 ** 32 - 50, gr if code == 1 else None)
            assert np.array_equal(Ys.cpu().numpy(), wr) and np.array_equal(st.cpu().numpy(), wst), Mr


def fit_rows(c, Ys, B):
    """engine.fit_batch on replicate signals [V, B, M] with replicated peaks: rows [V, B, np]."""
    from microstructure_fingerprinting_amd import engine
    rep = lambda a: np.repeat(a, B, axis=0)
    out = engine.fit_batch(c.plan, np.ascontiguousarray(Ys.reshape(c.V * B, c.M)), rep(c.K), rep(c.csf), rep(c.ear), rep(c.peaks), 3, True,
                           True, c.sig_csf, c.sig_ear, c.E)
    return out.reshape(c.V, B, -1)


@pytest.mark.parametrize("B,kind", [(1, "wild"), (5, "wild"), (5, "residual"), (65, "wild")])
def test_replicate_rows_equal_the_plain_fit_on_the_restatements_signals(case, B, kind):
    """engine.fit_bootstrap(keep=True) bit for bit: row order, peak replication, class binning, the batch-index counter;
    the voxels' own fit made inside or handed in; three chunks of the K = 2 class; a subset; the device entry point."""
    import torch
    from microstructure_fingerprinting_amd import engine
    c = case
    code = engine.BOOT_KINDS[kind]
    want = fit_rows(c, ref_ystar(c, B, code, True)[0], B)
    kw = dict(B=B, kind=kind, seed=SEED, inflate=True, q=Q, props=c.props, keep=True)
    res = engine.fit_bootstrap(c.plan, c.Y, *c.args, **kw)
    assert not res["status"].any()
    bad = np.argwhere(res["replicates"] != want)
    assert bad.size == 0, bad[:5]
    if B != 5:
        return
    given = engine.fit_bootstrap(c.plan, c.Y, *c.args, params=c.P0, **kw)
    chunks = engine.fit_bootstrap(c.plan, c.Y, *c.args, max_bytes=B * c.M * 8, **kw)     # one voxel per chunk
    for other in (given, chunks):
        for k in ("replicates", "stats", "agree", "status"):
            assert same(other[k], res[k]), k
    sub = np.array([4, 0, 6, 2])
    part = engine.fit_bootstrap(c.plan, c.Y[sub], c.K[sub], c.csf[sub], c.ear[sub], c.peaks[sub], *c.args[4:], vox=sub, **kw)
    for k in ("replicates", "stats", "agree", "status"):
        assert same(part[k], res[k][sub]), k
    if kind == "wild":
        off = 2 ** 32 - 3
        res_o = engine.fit_bootstrap(c.plan, c.Y, *c.args, offset=off, **kw)
        assert same(res_o["replicates"], fit_rows(c, ref_ystar(c, B, code, True, off)[0], B)) and not same(res_o["replicates"], want)
    # the device entry point on the plain K = 2 class, keyed by the batch indices
    dev = torch.device("cuda", 0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    k2 = np.array([2, 3, 4])
    out = engine.fit_bootstrap_dev(c.plan, t(c.Y[k2]), t(c.peaks[k2, :6]), 2, B=B, kind=kind, seed=SEED, q=Q, d_props=t(c.props),
                                   d_vox=t(k2.astype(np.int64)), keep=True, max_bytes=2 * B * c.M * 8)
    torch.cuda.synchronize(dev)
    cols2 = [0, 1, 2, 4, 5, 10, 11]                     # (maxfasc 2, no CSF, no EAR) inside the batch's layout
    assert same(out["replicates"].cpu().numpy(), want[k2][:, :, cols2])
    names = res["columns"]
    pick = [names.index(n) for n in out["columns"]]
    assert same(out["stats"].cpu().numpy(), res["stats"][k2][:, pick]) and same(out["agree"].cpu().numpy(), res["agree"][k2, :2])


def test_statistics_of_the_replicates(case):
    """The table engine.fit_bootstrap returns is the restatement's gather and reduce of its own replicate rows, bit for
    bit; columns a voxel's class lacks are weights that are 0 in every replicate and properties that are never valid."""
    from microstructure_fingerprinting_amd import engine
    c, B = case, 65
    res = engine.fit_bootstrap(c.plan, c.Y, *c.args, B=B, kind="wild", seed=SEED, q=Q, props=c.props, keep=True)
    X, valid, agree = R.gather(res["replicates"], c.P0, 3, True, True, c.props, c.N)
    want = R.reduce(X, valid, Q)
    assert res["columns"] == engine.boot_columns(3, True, True, 2) and res["stats"].shape == want.shape
    bad = np.argwhere(~((res["stats"] == want) | (np.isnan(res["stats"]) & np.isnan(want))))
    assert bad.size == 0, [(tuple(b), res["stats"][tuple(b)], want[tuple(b)]) for b in bad[:5]]
    assert np.array_equal(res["agree"], agree) and agree.max() <= B
    nv = res["stats"][:, :, 0]
    assert np.all(nv[:, :7] == B)                                         # M0, the weights and MSE ignore nothing
    for v in range(c.V):
        for k in range(3):
            cols = [7 + 2 * k, 8 + 2 * k]
            assert np.all(nv[v, cols] == np.count_nonzero(res["replicates"][v, :, 1 + k] > 0))
            if k >= c.K[v]:
                assert np.all(nv[v, cols] == 0) and np.all(res["stats"][v, 1 + k, [1, 3, 4]] == 0) and agree[v, k] == 0
    assert np.any((nv[:, 7:] > 0) & (nv[:, 7:] < B))                      # the validity rule is at work somewhere
    assert np.any(res["stats"][:, 7:, 2] > 0)                             # and a property does spread


def test_cpu_oracle_agrees_on_three_replicates_per_class(case):
    """The CPU oracle on the restatement's signals: atoms equal (those of compartments with a weight), other columns
    within the tolerances tests/test_fit_gpu.py uses for mixed classes (rtol 1e-7, atol 1e-9); the three-fascicle voxel,
    which that file does not have, against the oracle's exhaustive solver as tests/test_parity_stress_gpu.py does (1e-6)."""
    from microstructure_fingerprinting_amd import engine
    from oracle import oracle as orc
    c, B, n = case, 5, 3
    Ys = ref_ystar(c, B, 0, True)[0]
    res = engine.fit_bootstrap(c.plan, c.Y, *c.args, B=B, kind="wild", seed=SEED, keep=True)
    rows = res["replicates"]
    to2 = [0, 1, 2, 4, 5, 7, 8, 9, 10, 11]                # the batch's layout -> (maxfasc 2, CSF, EAR)
    for v in range(6):
        ref = orc.fit_batch(c.T, c.sch, Ys[v, :n], np.full(n, c.K[v]), np.full(n, c.csf[v]), np.full(n, c.ear[v]),
                            np.tile(c.peaks[v, :6], (n, 1)), 2, True, True, c.sig_csf, c.sig_ear, c.E)
        got = rows[v, :n][:, to2].copy()
        for col_nu, col_id in ((1, 3), (2, 4), (6, 7)):
            off = ref[:, col_nu] <= 1e-9
            got[off, col_id] = 0; ref[off, col_id] = 0
        assert np.array_equal(got[:, [3, 4, 7]], ref[:, [3, 4, 7]]), v
        assert np.allclose(got, ref, rtol=1e-7, atol=1e-9), v
    v = 6
    for b in range(n):
        A = np.concatenate([orc.interp(c.sch, c.peaks[v, 3 * k:3 * k + 3], c.T) for k in range(3)], axis=1)
        w, sub, tot, mo, yrec = orc.solve_exhaustive_posweights(np.ascontiguousarray(A), np.ascontiguousarray(Ys[v, b]), np.array([c.N] * 3))
        got = rows[v, b]
        act = w > 1e-9
        assert np.array_equal(got[4:7][act], sub[act].astype(float)), (b, got, sub, w)
        assert np.allclose(got[0], w.sum(), rtol=1e-6) and np.allclose(got[1:4], w / w.sum(), rtol=1e-6, atol=1e-9)
        assert np.isclose(got[-2], mo / c.M, rtol=1e-6)


@pytest.mark.parametrize("B", [1, 5, 65, 2500, 4096])
def test_reduce_equals_the_restatement(B):
    """mfx_boot_reduce_dev on hand-made tables, bit for bit: a column with no valid entry, one with exactly one, exact
    ties, full and ragged columns; B = 2500 and 4096 are the sizes at which three and one wave share a workgroup's LDS; quantiles also within 2 ulp of numpy's linear rule (positive values: numpy interpolates
    from the nearer end, which is the same number up to the rounding of the result)."""
    import torch
    from microstructure_fingerprinting_amd import engine
    rng = np.random.default_rng(40 + B)
    V, C = 3, 6
    X = rng.uniform(1.0, 2.0, (V, B, C))
    valid = np.ones((V, B, C), dtype=bool)
    valid[:, :, 1] = False                                               # nothing valid
    valid[:, :, 2] = False
    valid[np.arange(V), rng.integers(0, B, V), 2] = True                 # exactly one
    X[:, :, 3] = rng.integers(1, 4, (V, B)).astype(float)                # exact ties
    valid[:, :, 4] = rng.random((V, B)) < 0.6                            # ragged
    X[:, :, 5] = rng.uniform(1e-3, 1e3, (V, B)) ** 2
    X[~valid] = np.nan                                                   # an entry that is not valid is never looked at
    dev = torch.device("cuda", 0)
    got = engine.boot_reduce_dev(torch.from_numpy(X).to(dev), torch.from_numpy(valid).to(dev), Q).cpu().numpy()
    want = R.reduce(X, valid, Q)
    bad = np.argwhere(~((got == want) | (np.isnan(got) & np.isnan(want))))
    assert bad.size == 0, [(tuple(b), got[tuple(b)], want[tuple(b)]) for b in bad[:5]]
    assert np.all(got[:, 1, 0] == 0) and np.all(np.isnan(got[:, 1, 1:])) and np.all(got[:, 2, 0] == 1) and np.all(np.isnan(got[:, 2, 2]))
    for v in range(V):
        for col in range(C):
            x = X[v, valid[v, :, col], col]
            if x.size == 0:
                continue
            qn = np.quantile(x, Q, method="linear")
            assert np.all(np.abs(got[v, col, 5:] - qn) <= 2 * np.spacing(np.abs(qn))), (v, col, got[v, col, 5:], qn)
            assert np.isclose(got[v, col, 1], x.mean(), rtol=1e-14) and got[v, col, 3] == x.min() and got[v, col, 4] == x.max()
            if x.size > 1:
                assert np.isclose(got[v, col, 2], x.std(ddof=1), rtol=1e-12, atol=1e-300)
    assert engine.boot_reduce_dev(torch.from_numpy(X).to(dev), torch.from_numpy(valid).to(dev), ()).shape == (V, C, 5)


def test_mfmodelfit_bootstrap():
    import microstructure_fingerprinting_amd as mf
    d, sch, _, _ = R.golden_model()
    M = sch.shape[0]
    model = mf.MFModel({"dictionary": d["dictionary"], "sch_mat": d["sch_ms"], "orientation": R.Z, "num_atom": int(d["N"]),
                        "num_ear": int(d["E"]), "T2_csf": float(d["T2_csf"]), "DIFF_csf": float(d["DIFF_csf"]),
                        "T2_ear": float(d["T2_ear"]), "DIFF_ear": d["DIFF_ear"], "fasc_propnames": ["rad ", "fin"],
                        "rad": d["rad"], "fin": d["fin"]})
    grid = (4, 6)
    data = np.ascontiguousarray(d["Y"].reshape(grid + (M,)))
    mask = np.ones(grid); mask[0, 1] = 0; mask[3, 5] = 0
    fkw = dict(peaks=d["peaks"].reshape(grid + (6,)), pgse_scheme=sch, verbose=0)
    fit = model.fit(data, mask, d["numfasc"].reshape(grid), csf_mask=d["csf"].reshape(grid), ear_mask=d["ear"].reshape(grid), **fkw)
    B = 5
    bs = fit.bootstrap(data, B, seed=SEED, keep=True)
    roi = mask.reshape(-1) > 0
    n = int(roi.sum())
    assert bs.B == B and bs.seed == SEED and bs.replicates.shape == (n, B, fit.params_in_mask.shape[1])
    assert np.array_equal(bs.status.reshape(-1)[roi], np.zeros(n)) and np.all(bs.status.reshape(-1)[~roi] == -1)
    for name, shp in (("rad", grid + (2,)), ("fin", grid + (2,)), ("frac", grid + (2,)), ("M0", grid), ("frac_csf", grid),
                      ("frac_ear", grid), ("MSE", grid)):
        for f in (bs.mean, bs.std, bs.n_valid, lambda nm: bs.quantile(nm, 0.025), lambda nm: bs.quantile(nm, 0.975)):
            a = f(name)
            assert a.shape == shp, name
            out = a.reshape((24,) + shp[2:])[~roi]
            assert np.all(np.isnan(out)) if a.dtype.kind == "f" else np.all(out == 0)
    assert bs.agreement.shape == grid + (2,) and np.all(np.isnan(bs.agreement.reshape(24, 2)[~roi]))
    ag = bs.agreement.reshape(24, 2)[roi]
    rep, P = bs.replicates, fit.params_in_mask
    count = np.stack([np.count_nonzero((rep[:, :, 1 + k] > 0) & (rep[:, :, 3 + k] == P[:, None, 3 + k]), axis=1) for k in range(2)], axis=1)
    assert np.all((ag >= 0) & (ag <= 1)) and np.array_equal(ag, count / B)
    # 'frac' ignores nothing; a property honours nu_k > 0
    assert np.all(bs.n_valid("frac").reshape(24, 2)[roi] == B) and np.all(bs.n_valid("M0").reshape(-1)[roi] == B)
    nv = bs.n_valid("rad").reshape(24, 2)[roi]
    assert np.array_equal(nv, np.count_nonzero(rep[:, :, 1:3] > 0, axis=1)) and np.any(nv < B)
    mean_rad = bs.mean("rad").reshape(24, 2)[roi]
    for v in range(n):
        for k in range(2):
            ok = rep[v, :, 1 + k] > 0
            if ok.any():
                assert np.isclose(mean_rad[v, k], d["rad"][rep[v, ok, 3 + k].astype(int)].mean(), rtol=1e-14)
            else:
                assert np.isnan(mean_rad[v, k])
    assert np.allclose(bs.mean("frac").reshape(24, 2)[roi], rep[:, :, 1:3].mean(axis=1), rtol=1e-14, atol=1e-300)
    assert np.all(bs.quantile("MSE", 0.025).reshape(-1)[roi] <= bs.quantile("MSE", 0.975).reshape(-1)[roi])
    with pytest.raises(ValueError, match="was not asked for"):
        bs.quantile("MSE", 0.5)
    with pytest.raises(ValueError, match="unknown bootstrap statistic"):
        bs.mean("R2")
    # the same seed gives the same bits, another seed other replicates; a subset gives the whole ROI's
    again = fit.bootstrap(data, B, seed=SEED, keep=True)
    assert same(again.replicates, rep) and same(again.stats, bs.stats)
    assert not same(fit.bootstrap(data, B, seed=SEED + 1, keep=True).replicates, rep)
    vox = np.array([20, 3, 11])
    part = fit.bootstrap(data, B, seed=SEED, keep=True, voxels=vox)
    assert same(part.replicates, rep[vox]) and same(part.mean("rad").reshape(24, 2)[np.flatnonzero(roi)[vox]], mean_rad[vox])
    assert np.count_nonzero(part.status >= 0) == 3
    res = fit.bootstrap(data, B, kind="residual", seed=SEED)
    assert res.replicates is None and np.all(res.status.reshape(-1)[roi] == 0)
    # not served / beyond the limit
    fit_w = model.fit(data, mask, np.minimum(d["numfasc"].reshape(grid), 1), weights=np.ones(M), **fkw)
    with pytest.raises(NotImplementedError, match="bootstrap of a weighted or robust fit is not served"):
        fit_w.bootstrap(data, B)
    with pytest.raises(NotImplementedError, match="4096"):
        fit.bootstrap(data, 4097)
