"""Soft answers of the batched explicit solver on the device (include/mfx_solve_soft.h, csrc/solve_soft.hip): objective
profiles and posterior weights of many signals against one dictionary.

Referee, bars and inputs: tests/_solve_soft_cases.py (the long-double referee of tests/_post_ref.py on the explicit
dictionary; bars derived from B = 16 M eps ||y||^2 / (1 - c^2), nothing measured).  Every posterior comparison runs at a
peaked and at a broad noise level; tests/test_solve_soft_host.py shows that only the broad one can see a wrong sum.
The tile is 64 x 64: [64, 64] fills one, [65, 63] / [63, 65] add a tile of one row / one column, [150, 149] has seams
inside both sub-dictionaries, [1, 90] and [70, 1] are a single row and a single column."""
import functools

import numpy as np
import pytest

import _solve_soft_cases as SC

pytestmark = pytest.mark.gpu

EPS = SC.EPS
V = SC.V


def _mfu():
    from microstructure_fingerprinting_amd import mf_utils as mfu
    return mfu


def _solver(sizes, M):
    A, Y, sz = SC.problem(sizes, M)
    return _mfu().ExhaustiveSolver(np.array(A), np.array(sz)), np.array(Y)


def _rows(x, v):
    return [a[v] for a in x]


def _check_posterior(tag, Q, ref, s, signals=range(V)):
    worst = 0.0
    for v in signals:
        assert Q.status[v] == 0, "%s signal %d" % (tag, v)
        r = SC.worst_ratio(_rows(Q.weights, v), Q.log_sum[v], ref[v]["post"][s])
        worst = max(worst, r)
        assert r <= 1.0, "%s signal %d sigma %g: %.3g of the bar" % (tag, v, s, r)
    print("%s sigma %g: worst |got - referee| / bar = %.3g" % (tag, s, worst))


# ---- 1. shapes, against the referee, on the host route and the torch route
@pytest.mark.parametrize("sizes,M", SC.CASES, ids=SC.IDS)
def test_profile_and_posterior_against_the_referee(sizes, M):
    import torch
    from microstructure_fingerprinting_amd import engine
    ref = SC.referee(sizes, M)
    S, Y = _solver(sizes, M)
    with S:
        nk = len(sizes[:2])
        P = S.profile(Y, partner=True)
        assert len(P.obj) == nk and len(P.partner) == nk and np.all(P.status == 0)
        assert all(o.shape == (V, n) and o.dtype == np.float64 for o, n in zip(P.obj, sizes))
        assert all(p.shape == (V, n) and p.dtype == np.int32 for p, n in zip(P.partner, sizes))
        for v in range(V):
            SC.check_profile("host signal %d" % v, _rows(P.obj, v), _rows(P.partner, v), ref[v]["prof"])
        P2 = S.profile(Y)
        assert P2.partner is None and all(np.array_equal(a, b) for a, b in zip(P.obj, P2.obj))
        dY = torch.from_numpy(Y).cuda()
        dobj, dpar, dst = engine.solve_profile_dev(S, dY, partner=True)
        assert all(np.array_equal(a, b.cpu().numpy()) for a, b in zip(P.obj, dobj))
        assert all(np.array_equal(a, b.cpu().numpy()) for a, b in zip(P.partner, dpar))
        assert dst.dtype == torch.int32 and not dst.cpu().numpy().any()
        for v in range(V):
            SC.check_profile("torch signal %d" % v, [o[v].cpu().numpy() for o in dobj], [p[v].cpu().numpy() for p in dpar], ref[v]["prof"])
        if nk == 1:
            assert np.all(P.partner[0] == -1)
        for s in SC.sigmas(sizes, M):
            Q = S.posterior(Y, sigma=s)
            assert len(Q.weights) == nk and np.array_equal(Q.T, np.full(V, 2.0 * s * s))
            _check_posterior("host", Q, ref, s)
            dT = torch.full((V,), 2.0 * s * s, dtype=torch.float64, device="cuda")
            dw, dls, dmin, dst = engine.solve_posterior_dev(S, dY, dT)
            Qd = _mfu().SolverPosterior([w.cpu().numpy() for w in dw], dls.cpu().numpy(), dmin.cpu().numpy(), dst.cpu().numpy(),
                                        Q.T, M, {})
            _check_posterior("torch", Qd, ref, s)
            assert all(np.array_equal(a, b) for a, b in zip(Q.weights, Qd.weights))
            assert np.array_equal(Q.log_sum, Qd.log_sum) and np.array_equal(Q.min_obj, Qd.min_obj)
            # the evidence: log_sum - sum log n_k - (M / 2) log(pi T)
            assert np.allclose(Q.log_evidence(), Q.log_sum - sum(np.log(n) for n in sizes[:2]) - 0.5 * M * np.log(np.pi * 2.0 * s * s),
                               rtol=0, atol=1e-12)


# ---- 2. determinism
@functools.lru_cache(maxsize=None)
def _big(sizes):
    """V = 500 (9 tiles, gridDim.y = 228: three trips of 228, 228 and 44 signals): the 37 signals repeated"""
    M = 17
    S, Y = _solver(sizes, M)
    ix = np.arange(500) % V
    Y500 = np.ascontiguousarray(Y[ix])
    s = SC.broad_sigma(sizes, M)
    with S:
        P = S.profile(Y500, partner=True)
        Q = S.posterior(Y500, sigma=s)
    out = P.obj + P.partner + Q.weights + [Q.log_sum, Q.min_obj, P.status, Q.status]
    for a in out:
        a.setflags(write=False)
    return Y500, ix, s, out


def _all_outputs(S, Y, s, **kw):
    P = S.profile(Y, partner=True, **kw)
    Q = S.posterior(Y, sigma=s, **kw)
    return P.obj + P.partner + Q.weights + [Q.log_sum, Q.min_obj, P.status, Q.status]


@pytest.mark.parametrize("sizes", [(150, 149), (150, 149, 1)], ids=["150x149", "150x149x1"])
def test_identical_signals_give_identical_rows_at_every_position(sizes):
    Y500, ix, s, out = _big(sizes)
    for a in out:
        assert np.array_equal(a, a[:V][ix])
    assert not out[-1].any() and not out[-2].any()


@pytest.mark.parametrize("sizes", [(150, 149), (150, 149, 1)], ids=["150x149", "150x149x1"])
def test_chunking_and_batch_size_do_not_change_a_bit(sizes):
    Y500, ix, s, out = _big(sizes)
    S, Y = _solver(sizes, 17)
    with S:
        bp, bq = S.soft_bytes_per_signal('profile'), S.soft_bytes_per_signal('posterior')
        n1, n2 = sizes[0], sizes[1]
        Pn = 3 * n1 + 3 * n2
        assert bp == 8 * (sum(sizes) + 8) + 12 * Pn and bq == 8 * (sum(sizes) + 8) + 8 * Pn
        for nsig in (300, 1):     # 300 + 200 signals, and one signal a chunk
            P = S.profile(Y500, partner=True, max_bytes=nsig * bp)
            Q = S.posterior(Y500, sigma=s, max_bytes=nsig * bq)
            got = P.obj + P.partner + Q.weights + [Q.log_sum, Q.min_obj, P.status, Q.status]
            for a, b in zip(out, got):
                assert np.array_equal(a, b), "chunks of %d" % nsig
        for v in range(V):        # V = 1 calls
            got = _all_outputs(S, Y[v], s)
            for a, b in zip(out, got):
                assert np.array_equal(a[v:v + 1], b), "single signal %d" % v


@pytest.mark.parametrize("sizes", [(150, 149), (150, 149, 1)], ids=["150x149", "150x149x1"])
def test_non_finite_rows_leave_their_neighbours_untouched(sizes):
    Y500, ix, s, out = _big(sizes)
    S, _ = _solver(sizes, 17)
    Yb = Y500.copy()
    bad = [3, 230, 499]           # one in each trip of the sweep
    Yb[3, 0], Yb[230, 5], Yb[499, 16] = np.nan, np.inf, -np.inf
    with S:
        got = _all_outputs(S, Yb, s)
    keep = np.setdiff1d(np.arange(500), bad)
    for a, b in zip(out, got):
        assert np.array_equal(a[keep], b[keep])
    nk = 2
    obj, par, w = got[:nk], got[nk:2 * nk], got[2 * nk:3 * nk]
    log_sum, min_obj, pst, qst = got[3 * nk:]
    assert np.all(pst[bad] == 5) and np.all(qst[bad] == 5)
    assert all(np.isnan(a[bad]).all() for a in obj + w) and all((p[bad] == -1).all() for p in par)
    assert np.isnan(log_sum[bad]).all() and np.isnan(min_obj[bad]).all()


# ---- 3. consistency with the solver
@pytest.mark.parametrize("sizes,M", [((150, 149), 17), ((150, 149, 1), 17), ((65, 63), 30), ((33, 31, 1), 30)],
                         ids=["150x149-M17", "150x149x1-M17", "65x63-M30", "33x31x1-M30"])
def test_consistent_with_the_solver(sizes, M):
    ref = SC.referee(sizes, M)
    S, Y = _solver(sizes, M)
    s = SC.broad_sigma(sizes, M)
    with S:
        w, sub, tot, obj, yrec, status = S.solve(Y)
        P = S.profile(Y, partner=True)
        Q = S.posterior(Y, sigma=s)
        Q2 = S.posterior(Y, sigma=s, shift=Q.min_obj)
    assert np.array_equal(P.obj[0].min(axis=1), Q.min_obj) and np.array_equal(P.obj[1].min(axis=1), Q.min_obj)
    assert all(np.array_equal(a, b) for a, b in zip(Q.weights, Q2.weights))
    assert np.array_equal(Q.log_sum, Q2.log_sum) and np.array_equal(Q.min_obj, Q2.min_obj) and not Q2.status.any()
    sure = 0
    for v in range(V):
        i = int(np.argmin(P.obj[0][v]))
        robj, rarg, bar, _ = ref[v]["prof"][0]
        B = float(bar[int(np.argmin(robj))])       # of the referee's arg-min pair
        assert abs(Q.min_obj[v] - obj[v]) <= B, "signal %d: |%g - %g| > %g" % (v, Q.min_obj[v], obj[v], B)
        if ref[v]["post"][s]["gap"] > 2 * B:
            sure += 1
            assert (i, int(P.partner[0][v, i])) == (int(sub[v, 0]), int(sub[v, 1])), "signal %d" % v
            j = int(np.argmin(P.obj[1][v]))
            assert (int(P.partner[1][v, j]), j) == (i, int(sub[v, 1])), "signal %d" % v
    print("%d of %d signals have a decided arg-min" % (sure, V))
    assert sure >= 30
    for k, n in enumerate(sizes[:2]):
        assert np.all(np.abs(Q.weights[k].sum(axis=1) - 1.0) <= (n + 64) * EPS)


# ---- 4. consistency with the per-voxel path
@pytest.mark.parametrize("csf", [False, True], ids=["plain", "csf"])
def test_consistent_with_the_per_voxel_kernels(csf):
    """One multi-shell model rotated onto two fixed directions is an explicit dictionary: the solver's answers and the
    per-voxel kernels' (engine.posterior / engine.profile on the plan, the peaks repeated) each lie within their bar of
    the same long-double referee."""
    from microstructure_fingerprinting_amd import engine
    PR, TP = SC.PR, SC.TP
    kind = "c2"
    d0 = np.array([0.3, 0.2, 0.93]); d0 /= np.linalg.norm(d0)
    d1 = np.array([0.8, -0.5, 0.33]); d1 /= np.linalg.norm(d1)
    D0, D1 = TP._rot(kind, d0), TP._rot(kind, d1)
    x = np.asarray(TP._sig_csf(kind), dtype=np.float64) if csf else None
    M, N = D0.shape
    rng = np.random.default_rng(2024)
    nv = 8
    Y = np.stack([0.6 * D0[:, rng.integers(N)] + 0.3 * D1[:, rng.integers(N)] + (0.1 * x if csf else 0.0)
                  + 0.01 * np.abs(D0).mean() * rng.standard_normal(M) for _ in range(nv)])
    A = np.ascontiguousarray(np.concatenate([D0, D1] + ([x[:, None]] if csf else []), axis=1))
    sizes = np.array([N, N, 1] if csf else [N, N])
    pk = np.tile(np.concatenate([d0, d1]), (nv, 1))
    sigma = 0.05 * float(np.sqrt((Y ** 2).mean()))
    T = 2.0 * sigma * sigma
    cut = SC.cut()
    with _mfu().ExhaustiveSolver(A, sizes) as S:
        Q = S.posterior(Y, sigma=sigma)
        P = S.profile(Y)
    plan = TP._plan(kind)
    K, flags = np.full(nv, 2), (np.full(nv, True) if csf else None)
    w, log_sum, status, n_uns = engine.posterior(plan, Y, K, flags, pk, 2, csf, x, sigma)
    obj, _, _ = engine.profile(plan, Y, K, flags, pk, 2, csf, x)
    assert n_uns == 0 and not status.any() and not Q.status.any()
    for v in range(nv):
        r = PR.voxel(kind, Y[v], pk[v], csf, T, cut)
        assert r["clear"]
        mine = PR.worst_ratio(_rows(Q.weights, v), Q.log_sum[v], r)
        theirs = PR.worst_ratio([w[v, 0], w[v, 1]], log_sum[v], r)
        print("voxel %d: solver %.3g, per-voxel kernel %.3g of the bar" % (v, mine, theirs))
        assert mine <= 1.0 and theirs <= 1.0
        g = PR.gram(Y[v], D0, D1, x)
        F, c2bar, _, _ = PR.pair_values(g, csf, cut)
        for k, (Fa, ca) in enumerate(((F, c2bar), (F.T, c2bar.T))):
            arg = np.argmin(Fa, axis=1)
            rows = np.arange(N)
            B = 16 * M * EPS * r["ysq"] / np.asarray(ca[rows, arg], dtype=np.float64)
            assert np.all(np.abs(P.obj[k][v].astype(SC.LD) - Fa[rows, arg]) <= B)
            assert np.all(np.abs(obj[v, k].astype(SC.LD) - Fa[rows, arg]) <= B)
            assert np.all(np.abs(P.obj[k][v] - obj[v, k]) <= 2 * B)


# ---- 5. statuses and errors
def test_statuses():
    sizes, M = (65, 63), 17
    S, Y = _solver(sizes, M)
    n1, n2 = sizes
    with S:
        base = S.posterior(Y, sigma=2.0)
        sig = np.full(V, 2.0)
        sig[4], sig[9] = 0.0, np.nan
        sh = base.min_obj.copy()
        sh[12] = np.inf
        sh[20] = base.min_obj[20] + 701.0 * 8.0      # the best pair's exponent is 701
        sh[21] = base.min_obj[21] + 600.0 * 8.0      # in range: only the normalisation moves
        Q = S.posterior(Y, sigma=sig, shift=sh)
        expect = np.zeros(V, dtype=np.int32)
        expect[[4, 9, 12]] = 1
        expect[20] = 2
        assert np.array_equal(Q.status, expect)
        for v in np.flatnonzero(expect):
            assert np.isnan(Q.weights[0][v]).all() and np.isnan(Q.weights[1][v]).all() and np.isnan(Q.log_sum[v])
        ok = np.flatnonzero((expect == 0) & (np.arange(V) != 21))
        assert all(np.array_equal(a[ok], b[ok]) for a, b in zip(Q.weights, base.weights)) and np.array_equal(Q.log_sum[ok], base.log_sum[ok])
        assert np.array_equal(Q.min_obj, base.min_obj)
        assert np.allclose(Q.weights[0][21], base.weights[0][21], rtol=1e-12, atol=0) and abs(Q.log_sum[21] - base.log_sum[21]) < 1e-9
        # the all-zero signal: every pair has F = 0
        assert Q.status[0] == 0 and Q.min_obj[0] == 0.0 and abs(Q.log_sum[0] - np.log(n1 * n2)) <= 4 * EPS * np.log(n1 * n2)
        assert np.allclose(Q.weights[0][0], 1.0 / n1, rtol=(n2 + 64) * EPS, atol=0)
        assert np.allclose(Q.weights[1][0], 1.0 / n2, rtol=(n1 + 64) * EPS, atol=0)
        # sigma from the residual: the noiseless planted row has min F <= 0 or no meaning; the zero row has min F = 0
        R = S.posterior(Y)
        assert R.status[0] == 1 and np.isnan(R.T[0])
        good = np.flatnonzero(R.status == 0)
        assert good.size >= V - 2 and np.allclose(R.T[good], 2.0 * R.min_obj[good] / (M - 2), rtol=1e-14, atol=0)
        m, sd = S.posterior_moments(Y, np.arange(n1, dtype=np.float64), sigma=2.0)
        assert np.allclose(m, (base.weights[0] * np.arange(n1)).sum(axis=1), rtol=1e-13) and np.all(sd >= 0)
    # a planted row without noise on a dictionary of small integers, where every product and sum is exact: the pairs that
    # hold the planted atom have F = 0 exactly, so min F <= 0 and the residual gives no noise level
    rng = np.random.default_rng(5)
    Ai = rng.integers(1, 5, size=(M, 11)).astype(np.float64)
    with _mfu().ExhaustiveSolver(Ai, np.array([6, 5])) as S2:
        R = S2.posterior(np.array(Ai[:, 0]))
        assert R.min_obj[0] <= 0.0 and R.status[0] == 1 and np.isnan(R.weights[0]).all() and np.isnan(R.log_sum[0])
        assert S2.profile(np.array(Ai[:, 0])).obj[0][0, 0] == 0.0


def test_unserved_classes_and_argument_errors():
    import torch
    from microstructure_fingerprinting_amd import engine
    mfu = _mfu()
    for sizes in ((40, 40, 40), (6, 5, 4, 3)):
        A, Y, sz = SC.SB.make_problem(sizes, 17)
        with mfu.ExhaustiveSolver(A, sz) as S:
            dY = torch.from_numpy(Y).cuda()
            for call in (lambda: S.profile(Y), lambda: S.posterior(Y, sigma=1.0), lambda: engine.solve_profile_dev(S, dY),
                         lambda: engine.solve_posterior_dev(S, dY, torch.ones(V, dtype=torch.float64, device="cuda"))):
                with pytest.raises(NotImplementedError, match=r"\[%s\] are not served" % ", ".join(str(n) for n in sizes)):
                    call()
            assert S.soft_bytes_per_signal('profile') == -1
            assert S.solve(Y)[5].sum() == 0     # the solver itself serves them
    S, Y = _solver((37, 5), 17)
    with S:
        dY = torch.from_numpy(Y).cuda()
        dT = torch.ones(V, dtype=torch.float64, device="cuda")
        for bad in (torch.zeros((4, 5), dtype=torch.float64, device="cuda"), torch.zeros((2, 3, 17), dtype=torch.float64, device="cuda")):
            with pytest.raises(ValueError, match=r"\(17, 42\)"):
                engine.solve_profile_dev(S, bad)
            with pytest.raises(ValueError, match=r"\(17, 42\)"):
                engine.solve_posterior_dev(S, bad, dT)
        for bad in (dY.float(), dY.cpu(), dY.t()):
            with pytest.raises(AssertionError):
                engine.solve_profile_dev(S, bad)
            with pytest.raises(AssertionError):
                engine.solve_posterior_dev(S, bad, dT)
        with pytest.raises(AssertionError):
            engine.solve_posterior_dev(S, dY, dT.float())
        with pytest.raises(ValueError, match=r"T should have one entry per signal \(37\)"):
            engine.solve_posterior_dev(S, dY, dT[:5].contiguous())
        with pytest.raises(ValueError, match="out may hold 'obj0', 'obj1', 'partner0', 'partner1', 'status', got \\['w'\\]"):
            engine.solve_profile_dev(S, dY, out={'w': dT})
        with pytest.raises(ValueError, match="out\\['obj1'\\] should be"):
            engine.solve_profile_dev(S, dY, out={'obj1': torch.empty((V, 6), dtype=torch.float64, device="cuda")})
        with pytest.raises(ValueError, match="out\\['status'\\] should be"):
            engine.solve_posterior_dev(S, dY, dT, out={'status': torch.empty(V, dtype=torch.int64, device="cuda")})
        S.device = 1            # (as if the handle lived elsewhere: the check comes before any call)
        try:
            with pytest.raises(ValueError, match="signals live on cuda:0, the solver on device 1"):
                engine.solve_profile_dev(S, dY)
            with pytest.raises(ValueError, match="signals live on cuda:0, the solver on device 1"):
                engine.solve_posterior_dev(S, dY, dT)
        finally:
            S.device = 0
        # out tensors are written in place
        o0 = torch.empty((V, 37), dtype=torch.float64, device="cuda")
        obj, par, st = engine.solve_profile_dev(S, dY, out={'obj0': o0})
        assert obj[0] is o0 and par is None and torch.equal(o0, engine.solve_profile_dev(S, dY)[0][0])
        # no signal: empty outputs, no launch
        P = S.profile(np.zeros((0, 17)), partner=True)
        assert P.obj[0].shape == (0, 37) and P.partner[1].shape == (0, 5) and P.status.shape == (0,)
        assert S.posterior(np.zeros((0, 17)), sigma=1.0).weights[1].shape == (0, 5)
    from microstructure_fingerprinting_amd import _lib
    L = _lib.lib()
    with mfu.ExhaustiveSolver(np.ones((3, 2)), np.array([2])) as S1:
        h = S1.handle()
        o = np.zeros((1, 2))
        stt = np.zeros(1, dtype=np.int32)
        y = np.ones((1, 3))
        assert L.mfx_solve_profile(h, _lib.dptr(y), 1, 0, _lib.dptr(o), _lib.dptr(o), None, None, _lib.iptr(stt)) == _lib.MFX_ERR_ARG
        assert "no second set of outputs" in L.mfx_last_error().decode()
        assert L.mfx_solve_profile(h, _lib.dptr(y), 1, 0, None, None, None, None, _lib.iptr(stt)) == _lib.MFX_ERR_ARG


def test_two_handles_and_a_side_stream():
    import torch
    from microstructure_fingerprinting_amd import engine
    Sa, Ya = _solver((65, 63), 17)
    Sb, Yb = _solver((33, 31, 1), 30)
    with Sa, Sb:
        Pa, Pb = Sa.profile(Ya, partner=True), Sb.profile(Yb, partner=True)
        Qa, Qb = Sa.posterior(Ya, sigma=2.0), Sb.posterior(Yb, sigma=4.0)
        dYa, dYb = torch.from_numpy(Ya).cuda(), torch.from_numpy(Yb).cuda()
        dTa = torch.full((V,), 8.0, dtype=torch.float64, device="cuda")
        dTb = torch.full((V,), 32.0, dtype=torch.float64, device="cuda")
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        res = []
        with torch.cuda.stream(side):
            for _ in range(3):      # alternating handles, repeated calls: the arena's scratch is reused in stream order
                res.append((engine.solve_profile_dev(Sa, dYa, partner=True), engine.solve_posterior_dev(Sb, dYb, dTb),
                            engine.solve_posterior_dev(Sa, dYa, dTa), engine.solve_profile_dev(Sb, dYb, partner=True)))
        side.synchronize()
        for pa, qb, qa, pb in res:
            for (obj, par, st), P in ((pa, Pa), (pb, Pb)):
                assert all(np.array_equal(a.cpu().numpy(), b) for a, b in zip(obj, P.obj))
                assert all(np.array_equal(a.cpu().numpy(), b) for a, b in zip(par, P.partner))
            for (w, ls, mo, st), Q in ((qa, Qa), (qb, Qb)):
                assert all(np.array_equal(a.cpu().numpy(), b) for a, b in zip(w, Q.weights))
                assert np.array_equal(ls.cpu().numpy(), Q.log_sum) and np.array_equal(mo.cpu().numpy(), Q.min_obj)


# ---- 6. the cut
def test_a_pair_below_the_cut_is_scored_as_its_better_single_atom():
    M = 17
    rng = np.random.default_rng(606)
    A = np.abs(rng.standard_normal((M, 12)))
    A[:, 6 + 4] = A[:, 2]             # atom 2 of the first and atom 4 of the second sub-dictionary: 1 - c^2 = 0
    sizes = np.array([6, 6])
    Y = np.stack([0.7 * A[:, 2] + 0.01 * rng.standard_normal(M), 0.5 * A[:, 2] + 0.3 * A[:, 7] + 0.01 * rng.standard_normal(M),
                  0.4 * A[:, 1] + 0.4 * A[:, 10] + 0.01 * rng.standard_normal(M)])
    with _mfu().ExhaustiveSolver(A, sizes) as S:
        P = S.profile(Y, partner=True)
        for s in (0.05, 2.0):
            Q = S.posterior(Y, sigma=s)
            for v in range(3):
                F, c2bar, c2s, ysq = SC.pair_F(A, (6, 6), Y[v])
                assert SC.PR.clear_of_the_cut(c2s, SC.cut()) and c2s[0][2, 4] <= SC.cut() and c2bar[2, 4] == 1.0
                single = ysq - max(SC.TP._single(SC.LD(A[:, 2] @ Y[v]), SC.LD(A[:, 2] @ A[:, 2])), 0)
                assert abs(float(F[2, 4] - single)) <= 16 * M * EPS * ysq     # the referee's `below` branch
                r = SC.posterior_ref(F, c2bar, ysq, M, 2.0 * s * s)
                assert SC.worst_ratio(_rows(Q.weights, v), Q.log_sum[v], r) <= 1.0 and Q.status[v] == 0
                SC.check_profile("cut signal %d" % v, _rows(P.obj, v), _rows(P.partner, v), SC.profile_ref(F, c2bar, ysq, M))
