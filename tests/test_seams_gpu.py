"""Every launch and upload seam of the host code crossed at its smallest crossing shape (cases and method:
tests/_seam_cases.py; table and timings: DESIGN.md 4.28).

Per case: the distinct voxels are fitted in one small call `base`, which is held against the entry point's own referee (the
CPU oracle by test_units_gpu._compare, tests/_wfit_ref.py, _w2d_ref.py, _robust_ref.py, _solve_soft_cases.py,
test_fit2d_gpu.oracle_row) so that the tiled rows are right and not merely consistent; then the big call on V = L + r
voxels drawn from them returns base[idx] BIT FOR BIT on every output.  L comes from mfx_debug_seam, and every test asserts
V > L before it runs.  No tolerance is introduced here."""
import contextlib
import time

import numpy as np
import pytest

import _seam_cases as sc
import _units_cases as uc

pytestmark = pytest.mark.gpu

D = sc.D
_cache = {}


def _lib():
    from microstructure_fingerprinting_amd import _lib as L
    return L.lib()


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _case(name):
    """(case, L, V, idx): V > L asserted here, for every test, before anything runs"""
    c = sc.CASES[name]
    L, V, cuts = sc.sizes(name)
    assert V > L >= 1 and cuts, "%s does not cross its seam: V = %d, L = %d" % (name, V, L)
    idx, _ = sc.indices(name)
    assert np.all(idx[np.array(cuts) - 1] != idx[np.array(cuts)])
    return c, L, V, idx


@contextlib.contextmanager
def _timed(name, L, V, extra=""):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    yield
    torch.cuda.synchronize()
    print("%s: V = %d, L = %d, %d pieces, big call %.2f s%s" % (name, V, L, -(-V // L), time.perf_counter() - t0, extra))


@contextlib.contextmanager
def _hooks(*pairs):
    """(name of a debug switch, value while the block runs, value restored behind it)"""
    lib = _lib()
    try:
        for name, on, _ in pairs:
            getattr(lib, name)(on)
        yield lib
    finally:
        for name, _, off in pairs:
            getattr(lib, name)(off)


def _same(a, b):
    """bit equality, NaN patterns included"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype == np.float64 and b.dtype == np.float64:
        return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))
    return a.shape == b.shape and np.array_equal(a, b)


def _first_bad(got, want):
    bad = np.flatnonzero(np.any(np.atleast_2d(got.reshape(got.shape[0], -1) != want.reshape(want.shape[0], -1)), axis=1))
    return "%d rows differ, the first at %s" % (bad.size, bad[:4])


def _pgse_plan(mdl):
    from microstructure_fingerprinting_amd import mf_utils as mfu
    key = ("plan", mdl["key"])
    if key not in _cache:
        ms = mfu.init_PGSE_multishell_interp(mdl["dic"], mdl["sch"], uc.Z)
        _cache[key] = (ms, ms.plan_for(mdl["sch"]))
    return _cache[key][1]


# ---------------------------------------------------------------------------------------------------------------------
# seam 1: rotation, directions per launch
def test_rotation_directions_per_launch():
    """mfx_rotate (default stream) and mfx_rotate_dev on a stream of its own at B = L + 37 random directions: against
    orc.interp bit for bit on the directions around every boundary, and the whole second piece against the same call on
    dirs[L:] alone; mfx_rotate_cols (no seam) at the same B from the same fixtures."""
    import torch
    from microstructure_fingerprinting_amd import _lib as L_, synth
    from oracle import oracle as orc
    c, L, B, _ = _case("rotate")
    mdl = uc.model(c["dirs"], c["N"])
    M, N = mdl["M"], mdl["N"]
    assert M <= 16 and N == 4
    plan, T, sch = _pgse_plan(mdl), uc.tables(mdl, 1.0), mdl["sch"]
    lib = _lib()
    d = np.ascontiguousarray(synth.unit_vectors(np.random.default_rng(c["seed"]), B))
    out = np.full((B, M, N), np.nan)
    with _timed("rotate", L, B):
        L_.check(lib.mfx_rotate(plan.handle(), L_.dptr(d), B, 0, L_.dptr(out)))
    near = sorted(set(range(0, 8)) | set(range(L - 32, L + 32)) | set(range(B - 70, B)))
    assert len(near) >= 64 and L - 1 in near and L in near and B - 1 in near
    ref = {b: orc.interp(sch, d[b], T) for b in near}
    for b in near:
        assert np.array_equal(out[b], ref[b]), "mfx_rotate: direction %d (L = %d) differs from the oracle" % (b, L)
    tail = np.full((B - L, M, N), np.nan)
    L_.check(lib.mfx_rotate(plan.handle(), L_.dptr(np.ascontiguousarray(d[L:])), B - L, 0, L_.dptr(tail)))
    assert np.array_equal(out[L:], tail), "mfx_rotate: the second launch's rows " + _first_bad(out[L:], tail)
    assert np.all(np.isfinite(out))
    # the device entry point on a non-default stream
    s = torch.cuda.Stream()
    dd = _t(d)
    dout = torch.full((B, M, N), float("nan"), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        L_.check(lib.mfx_rotate_dev(plan.handle(), dd.data_ptr(), B, 0, dout.data_ptr(), s.cuda_stream))
    s.synchronize()
    assert np.array_equal(dout.cpu().numpy(), out), "mfx_rotate_dev: " + _first_bad(dout.cpu().numpy(), out)
    # one atom per direction: no seam, same fixtures
    cols = np.random.default_rng(c["seed"] + 1).integers(0, N, B).astype(np.int32)
    oc = np.full((B, M), np.nan)
    L_.check(lib.mfx_rotate_cols(plan.handle(), L_.dptr(d), L_.iptr(cols), B, 0, L_.dptr(oc)))
    assert np.array_equal(oc, out[np.arange(B), :, cols]), "mfx_rotate_cols: " + _first_bad(oc, out[np.arange(B), :, cols])
    for b in near:
        assert np.array_equal(oc[b], ref[b][:, cols[b]])


# ---------------------------------------------------------------------------------------------------------------------
# seams 2 and 3: the two-fascicle + CSF/EAR launchers (one class on the device: the host entry point's own chunks grow
# from V / 8 and never hand these launchers more than V / 2 voxels, so V = L + r reaches them only through mfx_fit_batch_dev)
def _fit_dev(mdl, cls, Y, peaks):
    import torch
    from microstructure_fingerprinting_amd import engine
    K, cs, e = uc.CLASSES[cls]
    out = engine.fit_batch_dev(_pgse_plan(mdl), _t(Y), _t(peaks), K, bool(cs), bool(e), _t(mdl["sig_csf"]) if cs else None,
                               _t(mdl["sig_ear"]) if e else None, uc.E if e else 0)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _pgse_base(name, hooks=()):
    """(mdl, cls, peaks, Y, base rows) of a PGSE case: the D distinct voxels in one call, held against the CPU oracle"""
    import test_units_gpu as UG
    c = sc.CASES[name]
    mdl, cls = uc.model(c["dirs"], c["N"]), c["cls"]
    peaks, Y = uc.voxels(mdl, cls, D)
    with _hooks(*hooks):
        base = _fit_dev(mdl, cls, Y, peaks)
    UG._compare(base, uc.oracle_rows(mdl, cls, 1.0, 1.0, D), cls, "%s: the distinct voxels against the oracle" % name)
    return mdl, cls, peaks, Y, base


# Ring entries of the screening kernel in the pipeline test.  With the built-in 2 048 none of the 61 distinct voxels is handed
# back; with 8 the voxels that list more than 8 pairs are (8 of the 61 when this was written: the absent fascicle's ties,
# the identical peaks, ...), about 4 500 of the big call's voxels, so that the hand-back pass crosses its own launches too.
K2S_CAP = 8


@pytest.mark.parametrize("name", ["k2x-NN_E-M62", "k2x-NN_1_E-M62", "k2x-NN_1-M68-screen-off"])
def test_plain_k2x_launch_chunks(name):
    """launch_k2x_t: a.vox_base and the per-workgroup slab across its launches of 2 048 voxels"""
    hooks = [("mfx_debug_set_k2x_screen", 0, 1)] if name.endswith("screen-off") else []
    c, L, V, idx = _case(name)
    mdl, cls, peaks, Y, base = _pgse_base(name, hooks)
    with _hooks(*hooks), _timed(name, L, V):
        big = _fit_dev(mdl, cls, Y[idx], peaks[idx])
    assert _same(big, base[idx]), "%s: %s" % (name, _first_bad(big, base[idx]))


def test_k2sx_pipeline_big_launches_and_hand_back_pass():
    """launch_k2sx_pipeline at 32 768 + 2 048 + 5 voxels: vox_base of the screening and of the list-mode kernel, the
    per-launch list arrays re-used by the second big launch, and the hand-back pass over the device-side list, with voxels
    handed back in both pieces.  Whether a voxel near the ring's size is handed back depends on the order in which its
    waves append (the rows do not): the pieces are therefore judged by the voxels that are handed back even with a ring
    four times as large - what a ring of 4 n overwrites, a ring of n overwrites too."""
    name = "k2sx-NN_1-M68"
    hooks = [("mfx_debug_set_k2x_screen", 1, 1), ("mfx_debug_set_k2s_cap", K2S_CAP, 0)]
    c, L, V, idx = _case(name)
    assert V == L + sc.seam(sc.K2X_CHUNK) + 5
    mdl, cls, peaks, Y, base = _pgse_base(name, hooks)
    assert mdl["M"] == 68

    def alone(cap):
        """counters 4 and 5 of every distinct voxel in a call of its own"""
        own = np.zeros((D, 2), dtype=np.int64)
        with _hooks(hooks[0], ("mfx_debug_set_k2s_cap", cap, 0)) as lib:
            for v in range(D):
                one = _fit_dev(mdl, cls, Y[v:v + 1], peaks[v:v + 1])
                own[v] = lib.mfx_debug_last_counter(4), lib.mfx_debug_last_counter(5)
                assert _same(one, base[v:v + 1]), "voxel %d alone (ring of %d) differs from its row in the small call" % (v, cap)
        return own
    sure, own = alone(4 * K2S_CAP)[:, 0] > 0, alone(K2S_CAP)
    with _hooks(*hooks) as lib, _timed(name, L, V):
        big = _fit_dev(mdl, cls, Y[idx], peaks[idx])
        back, by_bound = lib.mfx_debug_last_counter(4), lib.mfx_debug_last_counter(5)
    print("%s: of %d distinct voxels %d are handed back alone with a ring of %d (%d by the bound check), %d with a ring of %d; big "
          "call: %d voxels handed back, %d by the bound check; surely handed back: %d in the first piece, %d in the second"
          % (name, D, (own[:, 0] > 0).sum(), K2S_CAP, (own[:, 1] > 0).sum(), sure.sum(), 4 * K2S_CAP, back, by_bound,
             sure[idx[:L]].sum(), sure[idx[L:]].sum()))
    assert _same(big, base[idx]), "%s: %s" % (name, _first_bad(big, base[idx]))
    assert sure[idx[:L]].any() and sure[idx[L:]].any(), "no voxel is surely handed back in one of the pieces"
    assert sure[idx].sum() <= back < V, "the big call hands back %d voxels" % back
    assert back > sc.seam(sc.K2X_CHUNK), "the hand-back pass does not reach its second launch"


# ---------------------------------------------------------------------------------------------------------------------
# the weights of seams 4 to 6: per distinct voxel, a 0/1 mask with two zeroed rows for every third voxel, U(0.5, 1.5) otherwise
def _weights(V, M, seed):
    rng = np.random.default_rng(seed)
    W = rng.uniform(0.5, 1.5, (V, M))
    for v in range(0, V, 3):
        W[v] = 1.0
        W[v, rng.choice(M, 2, replace=False)] = 0.0
    return W


# seam 4: mfx_solve_dense_chunks behind the weighted fit
@pytest.mark.parametrize("name", ["dense-wfit-NN_1-M260", "dense-wfit-NN-M260-explicit"])
def test_dense_chunks_behind_fit_weighted(name):
    """engine.fit_weighted on a class its fused kernels do not take ([N, N, 1]; [N, N] with the explicit path forced): the
    block of min(free / 4, 1 GiB) holds fewer than V voxels, so the callbacks' v0, d_params + (v0 + q) np and ok + v0 + q
    run with v0 > 0."""
    import _wfit_ref as R
    from microstructure_fingerprinting_amd import engine
    c, L, V, idx = _case(name)
    mdl, cls = uc.model(c["dirs"], c["N"]), c["cls"]
    K, cs, _ = uc.CLASSES[cls]
    assert mdl["M"] == c["M"] and c["per_vox"] == 8 * mdl["M"] * (K * mdl["N"] + cs + 1)
    peaks, Y = uc.voxels(mdl, cls, D)
    W = _weights(D, mdl["M"], c["seed"])
    plan, T = _pgse_plan(mdl), uc.tables(mdl, 1.0)
    sig_csf = mdl["sig_csf"] if cs else None
    hooks = [("mfx_wfit_debug_set_force_explicit", 1, 0)] if name.endswith("explicit") else []

    def fit(ix):
        n = len(ix)
        return engine.fit_weighted(plan, Y[ix], W[ix], np.full(n, K), np.full(n, bool(cs)), peaks[ix], K, bool(cs), sig_csf)
    with _hooks(*hooks):
        base, bst = fit(np.arange(D))
        assert not bst.any()
        ref = np.array([R.ref_row(T, mdl["sch"], Y[v], W[v], peaks[v].reshape(K, 3), bool(cs), sig_csf, K, bool(cs)) for v in range(D)])
        R.assert_rows(base, ref, K, name)
        with _timed(name, L, V):
            big, st = fit(idx)
    assert not st.any() and _same(big, base[idx]), "%s: %s" % (name, _first_bad(big, base[idx]))


def _tables2d(sch_name, N, seed):
    import test_fit2d_gpu as F2
    from microstructure_fingerprinting_amd import mf_utils as U
    key = ("T2", sch_name, N, seed)
    if key not in _cache:
        rot = np.load(F2.G + "/rot2d_cases.npz")
        if sch_name == "syn2-44":       # the first two (Delta, delta) series of the 66-row protocol
            full = rot["syn2_sch"]
            pairs = np.unique(full[:, 4:6], axis=0)
            sch = np.ascontiguousarray(full[np.any(np.all(full[:, None, 4:6] == pairs[None, :2], axis=2), axis=1)])
        else:
            sch = rot[sch_name + "_sch"]
        _cache[key] = (U.RotateAtom2DTables(F2.atoms(sch, N, seed), sch, F2.Z, F2.DIFF), sch)
    return _cache[key]


@pytest.mark.parametrize("name", ["dense-fit2d-NN_1-fix", "dense-w2d-NN_1-fix"])
def test_dense_chunks_behind_the_2d_fits(name):
    """The same seam through engine.fit2d and engine.fit2d_weighted: two fascicles + CSF on the 1 776-row protocol."""
    import _w2d_ref as W2
    import _wfit_ref as R
    import test_fit2d_gpu as F2
    from microstructure_fingerprinting_amd import engine
    c, L, V, idx = _case(name)
    T, sch = _tables2d(c["sch"], c["N"], 6)
    assert T.M == c["M"] and c["per_vox"] == 8 * T.M * (2 * T.N + 1)
    sig_csf = F2.csf_signal(sch)
    Y, peaks = F2.two_fascicle_voxels(T, np.random.default_rng(c["seed"]), D, 0.3)
    Y = 0.8 * Y + 0.2 * sig_csf
    weighted = "w2d" in name
    W = _weights(D, T.M, c["seed"])

    def fit(ix):
        n = len(ix)
        if weighted:
            return engine.fit2d_weighted(T, Y[ix], W[ix], np.full(n, 2), np.ones(n, bool), peaks[ix], 2, True, sig_csf)
        return engine.fit2d(T, Y[ix], np.full(n, 2), np.ones(n, bool), peaks[ix], 2, True, sig_csf)
    base = fit(np.arange(D))
    assert all(not s.any() for s in base[1:])
    if weighted:
        ref = np.array([W2.ref_row(T.rotate(peaks[v].reshape(2, 3)), Y[v], W[v], True, sig_csf, 2, True) for v in range(D)])
        R.assert_rows(base[0], ref, 2, name)
    else:
        ref = np.array([F2.oracle_row(T, Y[v], peaks[v].reshape(2, 3), True, sig_csf, 2, True) for v in range(D)])
        F2.assert_rows(base[0], ref, 2, name)
    assert np.median(base[0][:, 5]) > 0.1, "the CSF column carries no weight: the class is not exercised"
    with _timed(name, L, V):
        big = fit(idx)
    for k, (b, a) in enumerate(zip(big, base)):
        assert _same(b, a[idx]), "%s output %d: %s" % (name, k, _first_bad(b, a[idx]))


# ---------------------------------------------------------------------------------------------------------------------
# seams 5 and 6: upload chunks of the host entry points, mixed batches
def _mixed_pgse(name):
    """The distinct voxels of classes N, NN, NN_1 (D each, small batch: class-major) and the big batch: the NN bin of
    L + 70 voxels drawn from its distinct ones, the other classes' voxels scattered among them.  -> (mdl, small, big, src)
    with small / big dicts of Y, W, K, csf, peaks and src [V] the row of the small batch every big voxel repeats."""
    c, L, Vnn, idx = _case(name)
    mdl = uc.model(c["dirs"], c["N"])
    M = mdl["M"]
    assert M == c["M"]
    classes = ("NN",) + sc.MIXED_OTHERS
    small = dict(Y=np.zeros((3 * D, M)), peaks=np.zeros((3 * D, 6)), K=np.zeros(3 * D, dtype=np.int32), csf=np.zeros(3 * D, bool))
    for i, cls in enumerate(classes):
        K, cs, _ = uc.CLASSES[cls]
        pk, Y = uc.voxels(mdl, cls, D)
        rows = slice(i * D, (i + 1) * D)
        small["Y"][rows], small["peaks"][rows, :3 * K], small["K"][rows], small["csf"][rows] = Y, pk, K, bool(cs)
    small["W"] = _weights(3 * D, M, c["seed"])
    labels = sc.mixed_layout(Vnn, c["seed"])
    src = np.zeros(labels.size, dtype=np.int64)
    src[labels == "NN"] = idx
    for i, cls in enumerate(classes[1:], start=1):
        src[labels == cls] = i * D + np.arange(D)
    big = {k: a[src] for k, a in small.items()}
    assert big["Y"].nbytes < sc.MAX_HOST_BYTES and np.count_nonzero(big["K"] == 2) == Vnn + D
    return mdl, small, big, src, L, Vnn


def test_wfit_upload_chunks():
    """mfx_wfit_batch: the [N, N] bin of a mixed batch in two uploads (gather_rows / scatter_rows from the bin's second
    chunk on)"""
    import _wfit_ref as R
    from microstructure_fingerprinting_amd import engine
    name = "upload-wfit-M260"
    mdl, small, big, src, L, Vnn = _mixed_pgse(name)
    plan, T = _pgse_plan(mdl), uc.tables(mdl, 1.0)

    def fit(b):
        return engine.fit_weighted(plan, b["Y"], b["W"], b["K"], b["csf"], b["peaks"], 2, True, mdl["sig_csf"])
    base, bst = fit(small)
    assert not bst.any()
    ref = np.array([R.ref_row(T, mdl["sch"], small["Y"][v], small["W"][v], small["peaks"][v, :3 * small["K"][v]].reshape(-1, 3),
                              bool(small["csf"][v]), mdl["sig_csf"], 2, True) for v in range(3 * D)])
    R.assert_rows(base, ref, 2, name)
    with _timed(name, L, Vnn, ", %.0f MB of signals" % (big["Y"].nbytes / 1e6)):
        got, st = fit(big)
    del big
    assert not st.any() and _same(got, base[src]), "%s: %s" % (name, _first_bad(got, base[src]))


def test_rfit_upload_chunks():
    """mfx_rfit_batch (cutoff, three iterations): rows, weights, scale, state and status of the [N, N] bin across its two
    uploads; the small call is the loop written by hand (tests/_robust_ref.py), bit for bit"""
    import _robust_ref as RR
    from microstructure_fingerprinting_amd import engine
    name = "upload-rfit-M260"
    mdl, small, big, src, L, Vnn = _mixed_pgse(name)
    plan = _pgse_plan(mdl)

    def fit(b):
        return engine.fit_robust(plan, b["Y"], b["K"], b["csf"], b["peaks"], 2, True, mdl["sig_csf"], W0=b["W"], loss="cutoff",
                                 c=4.45, n_iter=3)
    bp, bW, bi = fit(small)
    rp, rW, ri = RR.loop_ref(RR.engine_backend(plan), small["Y"], small["K"], small["csf"], small["peaks"], 2, True, mdl["sig_csf"],
                             small["W"], "cutoff", 4.45, 3)
    assert _same(bp, rp) and _same(bW, rW) and _same(bi["scale"], ri["scale"]) and np.array_equal(bi["state"], ri["state"])
    assert not bi["status"].any() and np.count_nonzero(bW == 0) > np.count_nonzero(small["W"] == 0)
    with _timed(name, L, Vnn, ", %.0f MB of signals" % (big["Y"].nbytes / 1e6)):
        p, W, info = fit(big)
    del big
    assert _same(p, bp[src]), "%s rows: %s" % (name, _first_bad(p, bp[src]))
    assert _same(W, bW[src]), "%s weights: %s" % (name, _first_bad(W, bW[src]))
    for k in ("scale", "state", "status"):
        assert _same(info[k], bi[k][src]), "%s %s: %s" % (name, k, _first_bad(info[k], bi[k][src]))


def test_rfit2d_upload_chunks():
    """mfx_rfit2d_batch's chunk_of(K): the two-fascicle bin of a mixed batch (K = 1, K = 2, K = 2 + CSF) on the 1 776-row
    protocol in two uploads; the small call is the hand-made loop on engine.fit2d / predict2d / fit2d_weighted, bit for bit"""
    import _robust2d_ref as R2
    import _robust_ref as RR
    import test_fit2d_gpu as F2
    from microstructure_fingerprinting_amd import engine
    name = "upload-rfit2d-fix"
    c, L, V2, idx = _case(name)
    T, sch = _tables2d(c["sch"], c["N"], 6)
    assert T.M == c["M"] and c["per_vox"] == 2
    sig_csf = F2.csf_signal(sch)
    pk, Y = R2.make_voxels(T, 3 * D, c["seed"], 0.3)
    K = np.repeat([2, 1, 2], D).astype(np.int32)
    csf = np.repeat([False, False, True], D)
    Y[csf] = 0.8 * Y[csf] + 100.0 * sig_csf
    small = dict(Y=Y, peaks=pk, K=K, csf=csf, W=_weights(3 * D, T.M, c["seed"]))
    labels = np.array(["a"] * V2 + ["b"] * D + ["c"] * D)[np.random.default_rng(c["seed"]).permutation(V2 + 2 * D)]
    src = np.zeros(labels.size, dtype=np.int64)
    src[labels == "a"], src[labels == "b"], src[labels == "c"] = idx, D + np.arange(D), 2 * D + np.arange(D)
    big = {k: a[src] for k, a in small.items()}

    def fit(b):
        return engine.fit2d_robust(T, b["Y"], b["K"], b["csf"], b["peaks"], 2, True, sig_csf, W0=b["W"], loss="cutoff", c=4.45, n_iter=3)
    bp, bW, bi = fit(small)
    rp, rW, ri = RR.loop_ref(R2.engine2d_backend(T), Y, K, csf, pk, 2, True, sig_csf, small["W"], "cutoff", 4.45, 3)
    assert _same(bp, rp) and _same(bW, rW) and _same(bi["scale"], ri["scale"]) and np.array_equal(bi["state"], ri["state"])
    assert not bi["status"].any() and not bi["state"].any() and not bi["dir_status"].any()
    with _timed(name, L, V2, ", %.0f MB of signals" % (big["Y"].nbytes / 1e6)):
        p, W, info = fit(big)
    assert _same(p, bp[src]), "%s rows: %s" % (name, _first_bad(p, bp[src]))
    assert _same(W, bW[src]), "%s weights: %s" % (name, _first_bad(W, bW[src]))
    for k in ("scale", "state", "status", "dir_status"):
        assert _same(info[k], bi[k][src]), "%s %s: %s" % (name, k, _first_bad(info[k], bi[k][src]))


# ---------------------------------------------------------------------------------------------------------------------
# seam 7: the 65 535-signal clamp of the solver's soft answers
@pytest.mark.parametrize("name", ["solve-soft-8x8", "solve-soft-8x8x1"])
def test_solve_soft_clamp(name):
    """engine.solve_profile_dev (with partners) and engine.solve_posterior_dev with max_bytes at its default: the byte
    budget would allow more than 65 535 signals, so the clamp is what cuts.  T and shift per signal, tiled with them."""
    import _solve_soft_cases as SC
    import torch
    from microstructure_fingerprinting_amd import engine
    from microstructure_fingerprinting_amd import mf_utils as mfu
    c, L, V, idx = _case(name)
    sizes, M = c["sizes"], c["M"]
    A, Y, sz = SC.problem(sizes, M)
    assert Y.shape[0] == c["D"]
    ref = SC.referee(sizes, M)
    sig = SC.sigmas(sizes, M)
    T = np.array([2.0 * sig[v % 2] ** 2 for v in range(c["D"])])
    shift = np.array([float(ref[v]["prof"][0][0].min()) for v in range(c["D"])])
    with mfu.ExhaustiveSolver(np.array(A), np.array(sz)) as S:
        for what in ("profile", "posterior"):
            assert sc.DEFAULT_BYTES // S.soft_bytes_per_signal(what) > L, "the byte budget cuts before the clamp"

        def run(ix):
            dY = _t(Y[ix])
            obj, par, st = engine.solve_profile_dev(S, dY, partner=True)
            w, ls, mo, st2 = engine.solve_posterior_dev(S, dY, _t(T[ix]), _t(shift[ix]))
            torch.cuda.synchronize()
            return [x.cpu().numpy() for x in list(obj) + list(par) + list(w) + [ls, mo, st, st2]]
        base = run(np.arange(c["D"]))
        nk = len(sizes[:2])
        assert not base[-1].any() and not base[-2].any()
        for v in range(c["D"]):
            SC.check_profile("%s signal %d" % (name, v), [o[v] for o in base[:nk]], [p[v] for p in base[nk:2 * nk]], ref[v]["prof"])
            r = SC.worst_ratio([w[v] for w in base[2 * nk:3 * nk]], base[3 * nk][v], ref[v]["post"][sig[v % 2]])
            assert r <= 1.0, "%s signal %d: %.3g of the referee's bar" % (name, v, r)
        with _timed(name, L, V):
            big = run(idx)
    for k, (b, a) in enumerate(zip(big, base)):
        assert _same(b, a[idx]), "%s output %d: %s" % (name, k, _first_bad(b, a[idx]))


# ---------------------------------------------------------------------------------------------------------------------
# seam 8: the 65 535-voxel clamp (gridDim.z) of the shared-fit bootstrap kernels
@pytest.mark.parametrize("name", ["boot2d-K1", "boot2d-K2", "wboot2d-K1", "wboot2d-K2"])
def test_bootstrap_shared_fit_clamp(name):
    """engine.fit2d_replicates_dev / fit2d_weighted_replicates_dev with B = 2 replicates a voxel (the signal itself and the
    signal times a fixed U(0.9, 1.1) row): rec + v0 K M, Y + v0 B M, vstat + 5 v0, params + v0 B np and the weights' rows in
    the second launch.  The replicates are given, so nothing random depends on a voxel's position."""
    import _w2d_ref as W2
    import _wfit_ref as R
    import test_fit2d_gpu as F2
    import torch
    from microstructure_fingerprinting_amd import engine
    c, L, V, idx = _case(name)
    K, B, weighted = c["K"], c["B"], name.startswith("w")
    T, sch = _tables2d(c["sch"], c["N"], 6)
    lib = _lib()
    assert T.M == c["M"] == 44 and B == 2
    # the shared-fit route serves the case (b2_shared_serves / wb2_shared_serves: K = 1 always, K = 2 up to the limit; no
    # force-plain switch is set), and its bytes per voxel leave the clamp as what cuts
    assert K == 1 or T.N <= (lib.mfx_wboot2d_max_atoms(T.handle()) if weighted else lib.mfx_fit2d_max_atoms(T.handle(), 2))
    assert sc.DEFAULT_BYTES // sc.boot2d_shared_bytes(K, T.N, T.M, B, weighted) > L
    rng = np.random.default_rng(c["seed"])
    Y, peaks = F2.two_fascicle_voxels(T, rng, D, 0.1)
    pk = np.ascontiguousarray(peaks[:, :3 * K])
    Ys = np.ascontiguousarray(np.stack([Y, Y * rng.uniform(0.9, 1.1, T.M)], axis=1))
    W = _weights(D, T.M, c["seed"])

    def run(ix):
        if weighted:
            out = engine.fit2d_weighted_replicates_dev(T, _t(Ys[ix]), _t(W[ix]), _t(pk[ix]), K)
        else:
            out = engine.fit2d_replicates_dev(T, _t(Ys[ix]), _t(pk[ix]), K)
        torch.cuda.synchronize()
        return [x.cpu().numpy() for x in out]
    base = run(np.arange(D))
    assert all(not s.any() for s in base[1:])
    for b in range(B):
        if weighted:
            ref = np.array([W2.ref_row(T.rotate(pk[v].reshape(K, 3)), Ys[v, b], W[v], False, None, K, False) for v in range(D)])
            R.assert_rows(base[0][:, b], ref, K, "%s replicate %d" % (name, b))
        else:
            ref = np.array([F2.oracle_row(T, Ys[v, b], pk[v].reshape(K, 3), False, None, K, False) for v in range(D)])
            F2.assert_rows(base[0][:, b], ref, K, "%s replicate %d" % (name, b))
    assert np.all(np.any(base[0][:, 0] != base[0][:, 1], axis=1))
    with _timed(name, L, V):
        big = run(idx)
    for k, (b, a) in enumerate(zip(big, base)):
        assert _same(b, a[idx]), "%s output %d: %s" % (name, k, _first_bad(b, a[idx]))
