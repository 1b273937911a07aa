"""Bootstrap conditional on measurement weights on the GPU (include/mfx_wboot.h, csrc/wboot.hip): the replicate weighted
fit against the weighted fit row by row, the resampling kernel against its NumPy restatement (tests/_wboot_ref.py), the
whole bootstrap against the loop a user writes by hand, the CPU oracle on replicate signals, and MFModelFit.bootstrap(
fixed_weights=True).

Models are synth.make_model("C2", N) with the scheme trimmed to M rows and voxels the recipe of tests/test_wfit_gpu.py
(make_voxels: even voxels general weights, odd voxels a 0/1 mask of 12 rows), imported from there.  "Equal" is
np.array_equal (NaN where both are NaN for the tables), no row left out."""
import numpy as np
import pytest

import _boot_ref as R
import _wboot_ref as WR
import _wfit_ref as WF
import _ties_cases as TC
import test_wfit_gpu as TW
from microstructure_fingerprinting_amd import _lib, engine
from oracle import oracle as orc

pytestmark = pytest.mark.gpu
SEED = 3
Q = (0.0, 0.025, 0.5, 0.975, 1.0)
_cache = {}


def same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def dev():
    import torch
    return torch.device("cuda", 0)


def t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def setup(N, M, V, seed):
    """(sch, plan, T, peaks [V, 6], Y, W) of V two-fascicle voxels on the first M rows of the C2 scheme."""
    key = ("setup", N, M, V, seed)
    if key not in _cache:
        sch, ms, T = TW.model(N)
        sch = np.ascontiguousarray(sch[:M])
        peaks, Y, W = TW.make_voxels(T, sch, V, np.random.default_rng(seed))
        _cache[key] = dict(sch=sch, plan=ms.plan_for(sch), T=T, peaks=peaks, Y=Y, W=W, N=N, M=M, V=V)
    return _cache[key]


def replicate_signals(c, B, seed):
    """Signals that move the fit: the voxel's row with every entry scaled by U(0.9, 1.1), B times."""
    rng = np.random.default_rng(seed)
    return np.ascontiguousarray(c["Y"][:, None, :] * rng.uniform(0.9, 1.1, (c["V"], B, c["M"])))


def plain_rows(c, Ys, W, K):
    """engine.fit_weighted_dev on the V B rows with the weights and peaks repeated: rows [V, B, np]."""
    import torch
    V, B, M = Ys.shape
    Wr = W if W.ndim == 1 else np.repeat(W, B, axis=0)
    out, st = engine.fit_weighted_dev(c["plan"], t(Ys.reshape(V * B, M)), t(Wr), t(np.repeat(c["peaks"][:, :3 * K], B, axis=0)), K)
    torch.cuda.synchronize()
    assert not st.cpu().numpy().any()
    return out.cpu().numpy().reshape(V, B, -1)


# ---- 1. the replicate fit is the weighted fit, row by row
@pytest.mark.parametrize("N,M,K", [(72, 45, 2), (144, 48, 2), (48, 197, 1)])
def test_replicates_equal_the_weighted_fit(N, M, K):
    """N = 72: one 128-block with a ragged 16-tile, M no multiple of the row chunk of 8; N = 144: two blocks, the second
    ragged; K = 1 on 197 rows.  B at and around the replicate tile Rt = mfx_wboot_rep_tile() (counts below 1 do not
    exist); general and 0/1 weights per voxel, one shared vector, and all of it again on the plain path."""
    import torch
    lib = _lib.lib()
    c = setup(N, M, 6, 31)
    assert M % 8 != 0 or N == 144
    if K == 2:
        assert N <= lib.mfx_wfit_max_atoms(c["plan"].handle(), 2)       # the shared path serves it
    Rt = lib.mfx_wboot_rep_tile()
    Bs = sorted({b for b in (1, Rt - 1, Rt, Rt + 1, 2 * Rt + 3) if b >= 1})
    Ys_all = replicate_signals(c, max(Bs), 7)
    for W in (c["W"], np.ascontiguousarray(c["W"][0])):
        want_all = plain_rows(c, Ys_all, W, K)
        assert len({r.tobytes() for r in want_all.reshape(-1, want_all.shape[-1])}) == want_all.shape[0] * want_all.shape[1]
        for B in Bs:
            Ys = np.ascontiguousarray(Ys_all[:, :B])
            for force in (0, 1):
                lib.mfx_wboot_debug_set_force_plain(force)
                try:
                    got, st = engine.fit_weighted_replicates_dev(c["plan"], t(Ys), t(W), t(c["peaks"][:, :3 * K]), K)
                    torch.cuda.synchronize()
                finally:
                    lib.mfx_wboot_debug_set_force_plain(0)
                assert not st.cpu().numpy().any()
                bad = np.argwhere(got.cpu().numpy() != want_all[:, :B])
                assert bad.size == 0, (W.ndim, B, force, bad[:5])


# ---- 2. the resampling kernel against the restatement
def fitted(c, K=2):
    """The voxels' own weighted fit and its prediction, once."""
    if "P0" not in c:
        V = c["V"]
        c["P0"], st = engine.fit_weighted(c["plan"], c["Y"], c["W"], np.full(V, K), None, c["peaks"], K, False)
        assert not st.any()
        c["pred"] = engine.predict(c["plan"], c["P0"], c["peaks"], K)
        c["groups"] = engine.boot_groups(c["sch"])
        assert len(np.unique(c["groups"])) > 1
    return c


@pytest.mark.parametrize("kind", ["wild", "residual"])
def test_resample_equals_the_restatement(kind):
    import torch
    c = fitted(setup(48, 197, 6, 32))
    code = engine.BOOT_KINDS[kind]
    g = c["groups"] if code == 1 else None
    B = 5
    for W in (c["W"], np.ascontiguousarray(c["W"][1])):            # per voxel; one shared 0/1 mask
        for inflate, offset in ((True, 0), (False, 0), (True, 2 ** 32 - 100)):
            Ys, pk, st = engine.wboot_resample_dev(t(c["Y"]), t(c["pred"]), t(W), t(c["P0"]), 2, False, B, kind, SEED, inflate, offset,
                                                   t(g) if g is not None else None, t(c["peaks"]))
            torch.cuda.synchronize()
            want, wst = WR.resample(c["Y"], c["pred"], W, c["P0"], 2, False, B, code, SEED, inflate, offset, g)
            assert np.array_equal(st.cpu().numpy(), wst) and not wst.any()
            bad = np.argwhere(Ys.cpu().numpy() != want)
            assert bad.size == 0, (W.ndim, inflate, offset, bad[:5])
            assert np.array_equal(pk.cpu().numpy(), np.repeat(c["peaks"], B, axis=0))
            zero = np.broadcast_to(W == 0, c["Y"].shape)
            assert zero.any() and np.array_equal(want[:, 0][zero], c["Y"][zero])
        # a subset with its batch indices gives the whole batch's replicates
        sub = np.array([4, 1, 5])
        want, _ = WR.resample(c["Y"], c["pred"], W, c["P0"], 2, False, B, code, SEED, True, 9, g)
        Ws = W if W.ndim == 1 else W[sub]
        Ys, _, _ = engine.wboot_resample_dev(t(c["Y"][sub]), t(c["pred"][sub]), t(Ws), t(c["P0"][sub]), 2, False, B, kind, SEED, True, 9,
                                             t(g) if g is not None else None, d_vox=t(sub.astype(np.int64)))
        assert np.array_equal(Ys.cpu().numpy(), want[sub])
    # W = 1 is mfx_boot_resample_dev, bit for bit
    for W in (np.ones(c["Y"].shape), np.ones(c["M"])):
        a, _, sa = engine.wboot_resample_dev(t(c["Y"]), t(c["pred"]), t(W), t(c["P0"]), 2, False, B, kind, SEED, True, 9,
                                             t(g) if g is not None else None)
        b, _, sb = engine.boot_resample_dev(t(c["Y"]), t(c["pred"]), t(c["P0"]), 2, False, False, B, kind, SEED, True, 9,
                                            t(g) if g is not None else None)
        assert torch.equal(a, b) and torch.equal(sa, sb)


# ---- 3. the bootstrap of a mixed batch is the hand loop
def mixed():
    """12 voxels on 48 atoms: K in {0, 1, 2}, every third voxel flagged CSF (with CSF signal mixed in)."""
    if "mixed" not in _cache:
        c = dict(setup(48, 200, 12, 33))
        c["K"] = np.array([2, 1, 0, 2, 2, 0, 2, 2, 1, 0, 2, 1], dtype=np.int32)
        c["csf"] = (np.arange(12) % 3) == 0
        c["sig_csf"] = TC.c2_model(48)[3]
        assert c["sig_csf"].shape == (200,)
        c["Y"] = c["Y"].copy()
        c["Y"][c["csf"]] = 0.8 * c["Y"][c["csf"]] + 100.0 * c["sig_csf"]
        c["props"] = np.stack([np.linspace(0.5, 5.0, 48), np.linspace(0.9, 0.3, 48)])
        c["args"] = (c["K"], c["csf"], c["peaks"], 2, True, c["sig_csf"])
        c["P0"], st = engine.fit_weighted(c["plan"], c["Y"], c["W"], *c["args"])
        assert not st.any()
        c["pred"] = engine.predict(c["plan"], c["P0"], c["peaks"], 2, True, False, c["sig_csf"])
        c["groups"] = engine.boot_groups(c["sch"])
        _cache["mixed"] = c
    return _cache["mixed"]


def hand_loop(c, B, kind, W=None, Y=None):
    """(replicate rows [V, B, np], stats, agree, status) of the loop written by hand: engine.fit_weighted, engine.predict,
    the restatement's rule, engine.fit_weighted on the replicates, the gather and reduce of tests/_boot_ref.py."""
    key = ("hand", B, kind)
    if W is None and Y is None and key in c:
        return c[key]
    W0 = c["W"] if W is None else W
    Y0 = c["Y"] if Y is None else Y
    V, M = Y0.shape
    P0, pred = c["P0"], c["pred"]
    if W is not None or Y is not None:
        P0, _ = engine.fit_weighted(c["plan"], Y0, W0, *c["args"])
        fin = np.all(np.isfinite(P0), axis=1)                           # (the host's predict refuses a NaN row: NaN by hand)
        pred = np.full(Y0.shape, np.nan)
        pred[fin] = engine.predict(c["plan"], P0[fin], c["peaks"][fin], 2, True, False, c["sig_csf"])
    code = engine.BOOT_KINDS[kind]
    Ys, st = WR.resample(Y0, pred, W0, P0, 2, True, B, code, SEED, True, 0, c["groups"] if code == 1 else None)
    Yz = np.where(np.isnan(Ys), 0.0, Ys)
    rep = lambda a: np.repeat(a, B, axis=0)
    ok = np.isin(st, (0, 1, 2))                                     # usable weights: those rows can be fitted
    rows = np.full((V, B, P0.shape[1]), np.nan)
    if ok.any():
        Wr = W0 if W0.ndim == 1 else rep(W0[ok])
        got, fst = engine.fit_weighted(c["plan"], Yz[ok].reshape(-1, M), Wr, rep(c["K"][ok]), rep(c["csf"][ok]), rep(c["peaks"][ok]), 2, True,
                                       c["sig_csf"])
        assert not fst.any()
        rows[ok] = got.reshape(-1, B, P0.shape[1])
    rows[st != 0] = np.nan
    X, valid, agree = R.gather(np.where(np.isnan(rows), 0.0, rows), P0, 2, True, False, c["props"], c["N"])
    X[st != 0], valid[st != 0], agree[st != 0] = np.nan, False, 0
    out = (rows, R.reduce(X, valid, Q), agree, st)
    if W is None and Y is None:
        c[key] = out
    return out


@pytest.mark.parametrize("kind", ["wild", "residual"])
def test_bootstrap_equals_the_hand_loop(kind):
    c, B = mixed(), 9
    rows, stats, agree, st = hand_loop(c, B, kind)
    assert not st.any()
    res = engine.fit_weighted_bootstrap(c["plan"], c["Y"], c["W"], *c["args"], B=B, kind=kind, seed=SEED, q=Q, props=c["props"], keep=True)
    assert not res["status"].any() and res["columns"] == engine.boot_columns(2, True, False, 2)
    bad = np.argwhere(res["replicates"] != rows)
    assert bad.size == 0, bad[:5]
    assert np.array_equal(res["agree"], agree) and agree.max() <= B
    assert res["stats"].shape == stats.shape
    bad = np.argwhere(~((res["stats"] == stats) | (np.isnan(res["stats"]) & np.isnan(stats))))
    assert bad.size == 0, [(tuple(b), res["stats"][tuple(b)], stats[tuple(b)]) for b in bad[:5]]
    assert np.any(res["stats"][:, 1:3, 2] > 0)                         # the replicates do move the fit
    # the own fit handed in is the own fit made inside
    given = engine.fit_weighted_bootstrap(c["plan"], c["Y"], c["W"], *c["args"], B=B, kind=kind, seed=SEED, q=Q, props=c["props"],
                                          params=c["P0"], keep=True)
    for k in ("replicates", "stats", "agree", "status"):
        assert same(given[k], res[k]), k


# ---- 4. the CPU oracle on replicate signals
ORACLE_SEED = 41


def oracle_case():
    """8 voxels, B = 4, on 48 atoms and 200 rows, all from the oracle: its weighted fit, the prediction of that, the
    restatement's replicates, the referee's row of every replicate and the smallest top-2 gap among them."""
    if "oracle" not in _cache:
        c = dict(setup(48, 200, 8, ORACLE_SEED))
        V, B, N = 8, 4, 48
        P0, _ = TW.referee(c["T"], c["sch"], c["Y"], c["W"], c["peaks"], 2)
        pred = np.zeros_like(c["Y"])
        for v in range(V):
            A = WF.scaled_problem(c["T"], c["sch"], c["Y"][v], c["W"][v], c["peaks"][v].reshape(2, 3), False, None)[0]
            pred[v] = (P0[v, 0] * P0[v, 1]) * A[:, int(P0[v, 3])] + (P0[v, 0] * P0[v, 2]) * A[:, N + int(P0[v, 4])]
        Ys, st = WR.resample(c["Y"], pred, c["W"], P0, 2, False, B, 0, SEED, True)
        assert not st.any()
        ref, gap = TW.referee(c["T"], c["sch"], Ys.reshape(V * B, -1), np.repeat(c["W"], B, axis=0), np.repeat(c["peaks"], B, axis=0), 2,
                              gaps=True)
        print("replicates: smallest top-2 gap %.2e |y'|^2 over %d rows" % (gap, V * B))
        assert gap >= TW.GAP, "pick another ORACLE_SEED: gap %.2e" % gap
        c.update(Ys=Ys, ref=ref.reshape(V, B, -1))
        _cache["oracle"] = c
    return _cache["oracle"]


def test_oracle_referee_on_replicates():
    import torch
    c = oracle_case()
    lib = _lib.lib()
    for force in (0, 1):
        lib.mfx_wboot_debug_set_force_plain(force)
        try:
            got, st = engine.fit_weighted_replicates_dev(c["plan"], t(c["Ys"]), t(c["W"]), t(c["peaks"]), 2)
            torch.cuda.synchronize()
        finally:
            lib.mfx_wboot_debug_set_force_plain(0)
        assert not st.cpu().numpy().any()
        got = got.cpu().numpy()
        assert got.shape == c["ref"].shape                              # no replicate is excluded
        WF.assert_rows(got.reshape(-1, got.shape[-1]), c["ref"].reshape(-1, got.shape[-1]), 2, "replicates, force_plain=%d" % force)


# ---- 5. W = 1
def test_unit_weights_against_the_unweighted_bootstrap():
    """What the headers promise for W = 1: the replicate SIGNALS are those of mfx_boot.h bit for bit (asserted on the
    device in test_resample_equals_the_restatement and here through the value the two bootstraps agree on), the weighted
    kernels see the unweighted dictionary columns bit for bit, and MSE = min_obj / M.  The two fits are different
    kernels, so their rows are compared as tests/test_wfit_gpu.py compares them for W = 1 (K = 1, 2 without CSF): atoms
    equal, every other column within rtol 1e-12.  Shared and per-voxel unit weights give the same bits."""
    c, B = mixed(), 6
    V, M = c["Y"].shape
    kw = dict(B=B, kind="wild", seed=SEED, q=Q, props=c["props"], keep=True)
    plain = engine.fit_bootstrap(c["plan"], c["Y"], c["K"], c["csf"], None, c["peaks"], 2, True, False, c["sig_csf"], **kw)
    full = engine.fit_weighted_bootstrap(c["plan"], c["Y"], np.ones((V, M)), *c["args"], **kw)
    shared = engine.fit_weighted_bootstrap(c["plan"], c["Y"], np.ones(M), *c["args"], **kw)
    for k in ("replicates", "stats", "agree", "status"):
        assert same(full[k], shared[k]), k
    assert not plain["status"].any() and not full["status"].any()
    nocsf = ~c["csf"]
    a, b = full["replicates"], plain["replicates"]
    WF.assert_rows(a[nocsf].reshape(-1, a.shape[-1]), b[nocsf].reshape(-1, a.shape[-1]), 2, "W = 1", rtol=1e-12, atol=0.0)
    # a CSF column: the weighted fit goes through the explicit solver, the plain fit through its fused kernels - two
    # float64 solvers of one problem, compared at the referee tolerance of tests/_wfit_ref.py (RTOL_W)
    WF.assert_rows(a[~nocsf].reshape(-1, a.shape[-1]), b[~nocsf].reshape(-1, a.shape[-1]), 2, "W = 1, CSF")
    assert np.array_equal(full["agree"], plain["agree"])


# ---- 6. invariance
def test_invariance_under_subsets_chunks_and_order():
    c, B = mixed(), 9
    V, M = c["Y"].shape
    kw = dict(B=B, kind="residual", seed=SEED, q=Q, props=c["props"], keep=True)
    res = engine.fit_weighted_bootstrap(c["plan"], c["Y"], c["W"], *c["args"], **kw)
    keys = ("replicates", "stats", "agree", "status")
    chunks = engine.fit_weighted_bootstrap(c["plan"], c["Y"], c["W"], *c["args"], max_bytes=B * M * 8, **kw)     # one voxel per chunk
    for k in keys:
        assert same(chunks[k], res[k]), k
    for sub in (np.array([4, 0, 6, 3]), np.random.default_rng(1).permutation(V)):
        part = engine.fit_weighted_bootstrap(c["plan"], c["Y"][sub], c["W"][sub], c["K"][sub], c["csf"][sub], c["peaks"][sub], 2, True,
                                             c["sig_csf"], vox=sub, **kw)
        for k in keys:
            assert same(part[k], res[k][sub]), k
    # the device entry point on the K = 2 class without CSF, keyed by the batch indices, in small chunks and whole
    import torch
    k2 = np.flatnonzero((c["K"] == 2) & ~c["csf"])
    assert k2.size >= 3
    cols2 = [0, 1, 2, 3, 4, 6, 7]                       # (maxfasc 2, no CSF) inside the batch's layout
    for mb in (B * M * 8, engine.BOOT_DEFAULT_BYTES):
        out = engine.fit_weighted_bootstrap_dev(c["plan"], t(c["Y"][k2]), t(c["W"][k2]), t(c["peaks"][k2]), 2, B=B, kind="residual",
                                                seed=SEED, q=Q, d_props=t(c["props"]), d_vox=t(k2.astype(np.int64)), keep=True,
                                                max_bytes=mb)
        torch.cuda.synchronize()
        assert same(out["replicates"].cpu().numpy(), res["replicates"][k2][:, :, cols2])
        pick = [res["columns"].index(n) for n in out["columns"]]
        assert same(out["stats"].cpu().numpy(), res["stats"][k2][:, pick]) and same(out["agree"].cpu().numpy(), res["agree"][k2])


# ---- 7. unusable rows
def test_unusable_voxels_get_their_status_and_nan_statistics():
    c, B = mixed(), 9
    W, Y = c["W"].copy(), c["Y"].copy()
    W[0, 5] = -1.0                                                      # 3 (a K = 2 + CSF voxel)
    W[1] = 0.0                                                          # 4 (K = 1)
    Y[10, 17] = np.nan                                                  # 2 (K = 2)
    W[7] = 0.0
    W[7, 90] = 1.0                                                      # 1 (K = 2): M+ = 1 row, and it has a weight to explain it
    kw = dict(B=B, kind="wild", seed=SEED, q=Q, props=c["props"], keep=True)
    res = engine.fit_weighted_bootstrap(c["plan"], Y, W, *c["args"], **kw)
    rows, stats, agree, st = hand_loop(c, B, "wild", W=W, Y=Y)
    assert list(st[[0, 1, 10, 7]]) == [3, 4, 2, 1] and np.count_nonzero(st) == 4
    assert np.array_equal(res["status"], st)
    bad_v = st != 0
    assert np.all(np.isnan(res["replicates"][bad_v])) and np.all(np.isnan(res["stats"][bad_v][:, :, 1:])) and not res["stats"][bad_v][:, :, 0].any()
    assert not res["agree"][bad_v].any()
    # the neighbours are untouched: theirs are the bits of the clean batch
    clean = engine.fit_weighted_bootstrap(c["plan"], c["Y"], c["W"], *c["args"], **kw)
    for k in ("replicates", "stats", "agree", "status"):
        assert same(res[k][~bad_v], clean[k][~bad_v]), k
    assert same(res["replicates"], rows) and same(res["stats"], stats)


# ---- 8. exact ties
def test_duplicated_atom_takes_the_first_pair_in_every_replicate():
    import torch
    from microstructure_fingerprinting_amd import mf_utils as mfu
    from microstructure_fingerprinting_amd import synth
    sch, dic, T, _ = TC.c2_model(16)
    dic = dic.copy()
    src, dup = 3, 11
    dic[:, dup] = dic[:, src]                                           # atom 11 is atom 3 again
    T2 = orc.init_tables(dic, sch, TW.Z)
    plan = mfu.init_PGSE_multishell_interp(dic, sch, TW.Z).plan_for(sch)
    rng = np.random.default_rng(5)
    V, B, M = 4, 5, sch.shape[0]
    peaks, Y, W = np.zeros((V, 6)), np.zeros((V, M)), np.ones((V, M))
    for v in range(V):
        d = synth.unit_vectors(rng, 2)
        other = [0, 7, 9, 14][v]
        cols = (src, other) if v % 2 == 0 else (other, src)             # the twin in the first, then in the second dictionary
        Y[v] = 500.0 * (0.5 * orc.interp(sch, d[0], T2)[:, cols[0]] + 0.5 * orc.interp(sch, d[1], T2)[:, cols[1]])
        W[v] = rng.uniform(0.05, 2.0, M)
        W[v, rng.choice(M, 12, replace=False)] = 0.0
        peaks[v] = d.reshape(-1)
    Ys = np.ascontiguousarray(Y[:, None, :] * (1.0 + 0.01 * rng.standard_normal((V, B, M))))
    Ys[:, 0] = Y                                                        # replicate 0: the exact mixture, the twins tie exactly
    lib = _lib.lib()
    rows = {}
    for force in (0, 1):
        lib.mfx_wboot_debug_set_force_plain(force)
        try:
            got, st = engine.fit_weighted_replicates_dev(plan, t(Ys), t(W), t(peaks), 2)
            torch.cuda.synchronize()
        finally:
            lib.mfx_wboot_debug_set_force_plain(0)
        assert not st.cpu().numpy().any()
        rows[force] = got.cpu().numpy()
    assert np.array_equal(rows[0], rows[1])
    atoms = rows[0][:, :, 3:5]
    assert not np.any((atoms == dup) & (rows[0][:, :, 1:3] > 0))        # never the later twin
    for v in range(V):
        assert atoms[v, 0, v % 2] == src, (v, atoms[v])                 # the exact tie: the first of the tied pairs
    print("the earlier twin is chosen in %d of %d replicate rows" % (np.count_nonzero(np.any(atoms == src, axis=2)), V * B))


# ---- 9. end to end
def test_mfmodelfit_bootstrap_with_fixed_weights():
    import test_profile_gpu as TP
    from microstructure_fingerprinting_amd import synth
    model = TP._model("small")
    rng = np.random.default_rng(78)
    ph = synth.make_phantom(model, (6, 5, 4), rng, p_ear=0.0)
    sch = np.ascontiguousarray(model.dic["sch_mat"], dtype=np.float64)
    M = sch.shape[0]
    roi = np.flatnonzero(ph["mask"].reshape(-1))
    data = np.ascontiguousarray(ph["data"], dtype=np.float64)
    rows = data.reshape(-1, M)
    for v in roi[::3]:
        rows[v, rng.choice(M, 6, replace=False)] += 400.0               # planted outliers
    kw = dict(peaks=ph["peaks"], pgse_scheme=sch, csf_mask=ph["csf_mask"], verbose=0)
    a = (data, ph["mask"], ph["numfasc"])
    fit = model.fit(*a, robust={"n_iter": 1}, **kw)
    Wr = np.asarray(fit.weights_roi)
    assert Wr.shape == (roi.size, M) and np.any(Wr == 0)
    with pytest.raises(NotImplementedError, match="bootstrap of a weighted or robust fit is not served"):
        fit.bootstrap(data, B=8, keep=True)
    bs = fit.bootstrap(data, B=8, fixed_weights=True, keep=True, seed=SEED)
    K = ph["numfasc"].reshape(-1)[roi].astype(int)
    csf = ph["csf_mask"].reshape(-1)[roi] > 0
    pk = ph["peaks"].reshape(-1, 6)[roi]
    plan = model.ms_interpolator.plan_for(sch)
    names = list(fit._props)
    props = np.stack([fit._props[n] for n in names])
    csf_on = bool(csf.any())
    res = engine.fit_weighted_bootstrap(plan, np.ascontiguousarray(rows[roi]), Wr, K, csf, pk, 2, csf_on,
                                        model._extra_signals(sch, csf_on, False)[0], B=8, kind="wild", seed=SEED, props=props,
                                        params=fit.params_in_mask, keep=True)
    assert same(bs.replicates, res["replicates"]) and same(bs.stats, res["stats"]) and bs.columns == res["columns"]
    assert bs.weights is Wr or np.array_equal(bs.weights, Wr)
    assert np.array_equal(bs.status.reshape(-1)[roi], res["status"]) and np.all(bs.status.reshape(-1)[ph["mask"].reshape(-1) == 0] == -1)
    assert "rad" in names and fit._nf == 2 and bs.std("rad").shape == ph["mask"].shape + (2,)
    assert np.any(bs.std("frac")[np.isfinite(bs.std("frac"))] > 0)
    # a subset gives the whole ROI's replicates
    sub = np.array([5, 2, 9])
    part = fit.bootstrap(data, B=8, fixed_weights=True, keep=True, seed=SEED, voxels=sub)
    assert same(part.replicates, bs.replicates[sub]) and np.array_equal(part.weights, Wr[sub])
    # one shared [M] vector of weights takes the shared-vector route
    fit1 = model.fit(*a, weights=np.ones(M), **kw)
    assert np.asarray(fit1.weights_roi).shape == (M,)
    b1 = fit1.bootstrap(data, B=8, fixed_weights=True, keep=True, seed=SEED)
    r1 = engine.fit_weighted_bootstrap(plan, np.ascontiguousarray(rows[roi]), np.ones(M), K, csf, pk, 2, csf_on,
                                       model._extra_signals(sch, csf_on, False)[0], B=8, kind="wild", seed=SEED, props=props,
                                       params=fit1.params_in_mask, keep=True)
    assert b1.weights.shape == (M,) and same(b1.replicates, r1["replicates"]) and same(b1.stats, r1["stats"])
    assert fit.bootstrap.__kwdefaults__["fixed_weights"] is False
