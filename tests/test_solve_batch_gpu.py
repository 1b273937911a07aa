"""Batched explicit-dictionary solver on the device (include/mfx_solve.h, csrc/solve_batch.hip).

The contract: row v of a batch equals, bit for bit, what solve_exhaustive_posweights(A, Y[v], dicsizes) returns, on the
tiled route (two sub-dictionaries, three with a last one of one column), on the generic route, forced or not, and
whatever the chunking.  The loop of one-problem solves of a case is made once and shared by the tests of that case.
The tile of the tiled route is 64 x 64: [64, 64] fills one exactly, [65, 63] and [63, 65] add a tile of one row and of
one column, [150, 149] has seams inside both sub-dictionaries."""
import contextlib
import functools
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

V = 37
SHAPES2 = [[37, 5], [1, 90], [150, 149], [64, 64], [65, 63], [63, 65]]
SHAPES3 = [[33, 31, 1], [40, 40, 40], [12, 9, 7]]
SHAPES_OTHER = [[50], [6, 5, 4, 3], [3, 3, 2, 2, 2]]
CASES = [(tuple(s), M) for s in SHAPES2 + SHAPES3 + SHAPES_OTHER for M in (17, 30)]
IDS = ["%s-M%d" % ("x".join(str(n) for n in s), M) for s, M in CASES]


def _mfu():
    from microstructure_fingerprinting_amd import mf_utils as mfu
    return mfu


@contextlib.contextmanager
def forced_generic():
    from microstructure_fingerprinting_amd import _lib
    _lib.lib().mfx_solve_debug_set_force_generic(1)
    try:
        yield
    finally:
        _lib.lib().mfx_solve_debug_set_force_generic(0)


def make_problem(sizes, M, seed=77):
    """|randn| dictionary; signals as in test_solver_vs_oracle_two_dictionaries_ragged (0.7 of an atom of the first
    sub-dictionary, 0.2 of one of every other, noise of 0.01), the atoms drawn per signal; signal 0 is all zero and
    signal 1 exactly 2 a_0 + a_{n1 + 3}."""
    sizes = np.asarray(sizes)
    rng = np.random.default_rng([seed, M] + [int(s) for s in sizes])
    starts = np.concatenate(([0], np.cumsum(sizes)[:-1]))
    A = np.abs(rng.standard_normal((M, int(sizes.sum()))))
    Y = np.zeros((V, M))
    for v in range(2, V):
        for k, (s0, n) in enumerate(zip(starts, sizes)):
            Y[v] += (0.7 if k == 0 else 0.2) * A[:, s0 + rng.integers(n)]
        Y[v] += 0.01 * rng.standard_normal(M)
    Y[1] = 2.0 * A[:, 0]
    if sizes.size > 1:
        Y[1] = 2.0 * A[:, 0] + A[:, starts[1] + min(3, sizes[1] - 1)]
    return A, Y, sizes


@functools.lru_cache(maxsize=None)
def reference(sizes, M):
    """The problem of a case and the loop of one-problem solves on it (read-only)."""
    A, Y, sz = make_problem(sizes, M)
    rows = [_mfu().solve_exhaustive_posweights(A, Y[v].copy(), sz) for v in range(V)]
    for a in (A, Y):
        a.setflags(write=False)
    return A, Y, sz, rows


def assert_rows_equal(got, rows, what=""):
    """Bit equality of a batch result with a list of one-problem results, dtypes included."""
    w, sub, tot, obj, yrec, status = got
    assert w.shape[0] == len(rows)
    for v, (rw, rsub, rtot, robj, ryrec) in enumerate(rows):
        tag = "%s signal %d" % (what, v)
        assert status[v] == 0, tag
        assert np.array_equal(sub[v], rsub) and np.array_equal(tot[v], rtot), tag
        assert sub.dtype == rsub.dtype and tot.dtype == rtot.dtype, tag
        assert np.array_equal(w[v], rw), tag
        assert obj[v] == robj, tag
        if yrec is not None:
            assert np.array_equal(yrec[v], ryrec), tag
    assert w.dtype == np.float64 and obj.dtype == np.float64 and status.dtype == np.int32


@pytest.mark.parametrize("sizes,M", CASES, ids=IDS)
def test_bit_equal_to_the_single_solver(sizes, M):
    mfu = _mfu()
    A, Y, sz, rows = reference(sizes, M)
    with mfu.ExhaustiveSolver(A, sz) as S:
        assert (S.M, S.num_columns) == (M, int(sz.sum())) and np.array_equal(S.dicsizes, sz)
        assert_rows_equal(S.solve(Y), rows, "one chunk")
        assert_rows_equal(S.solve(Y, max_bytes=15 * S.bytes_per_signal), rows, "chunks of 15, 15, 7")
        assert_rows_equal(S.solve(Y, max_bytes=1), rows[:V], "chunks of one")
        with forced_generic():
            assert_rows_equal(S.solve(Y), rows, "generic route")
            assert_rows_equal(S.solve(Y, max_bytes=15 * S.bytes_per_signal), rows, "generic route, chunks of 15, 15, 7")
        one = S.solve(Y[5])                                   # a single [M] vector
        assert_rows_equal(one, rows[5:6], "one vector")
        assert S.solve(Y, recons=False)[4] is None
    assert_rows_equal(mfu.solve_exhaustive_posweights_batch(A, Y[:3], sz), rows[:3], "one-shot")


@pytest.mark.parametrize("sizes,M", CASES, ids=IDS)
def test_oracle_parity(sizes, M):
    """Up to three sub-dictionaries: the oracle's arithmetic, so indices, weights and objective exact, ties included.
    Four and more: the oracle is a third-party NNLS compared at 1e-5, and an index can only be claimed where the minimiser
    is unique.  A sub-dictionary whose weight is 0 at the optimum has none: every one of its atoms gives the same
    objective in exact arithmetic (the all-zero signal, the signal made of two atoms exactly), and the last bits of two
    different NNLS algorithms pick among them - the oracle returns weights of 1e-16 there, objectives of 1e-30.  The
    index is compared where the oracle's weight exceeds 1e-10, the absolute tolerance the weights are compared at: a
    weight below it is not told from 0."""
    from oracle import oracle as orc
    A, Y, sz, _ = reference(sizes, M)
    w, sub, tot, obj, yrec, status = _mfu().solve_exhaustive_posweights_batch(A, Y, sz)
    for v in range(V):
        ref = orc.solve_exhaustive_posweights(A, Y[v].copy(), sz)
        if sz.size <= 3:
            assert np.array_equal(sub[v], ref[1]) and np.array_equal(tot[v], ref[2]), v
            assert np.array_equal(w[v], ref[0]) and obj[v] == ref[3], v
        else:
            unique = ref[0] > 1e-10
            assert np.array_equal(sub[v][unique], ref[1][unique]) and np.array_equal(tot[v][unique], ref[2][unique]), v
            assert np.allclose(w[v], ref[0], rtol=1e-5, atol=1e-10), v
            assert np.isclose(obj[v], ref[3], rtol=1e-5, atol=1e-10), v
            assert np.allclose(yrec[v], ref[4], rtol=1e-5, atol=1e-10), v


def test_reference_golden_problems_through_the_batch():
    """tests/golden/solver_cases.npz, V = 1 each: the assertions of test_solver_gpu.test_reference_golden_problems."""
    mfu = _mfu()
    d = np.load(os.path.join(G, "solver_cases.npz"))
    for nm in d["names"]:
        sizes = d[nm + "_sizes"]
        w, sub, tot, obj, yrec, status = mfu.solve_exhaustive_posweights_batch(d[nm + "_A"], d[nm + "_y"], sizes)
        assert w.shape == (1, sizes.size) and status[0] == 0
        w, sub, tot, obj, yrec = w[0], sub[0], tot[0], obj[0], yrec[0]
        assert np.array_equal(sub, d[nm + "_sub"]), nm
        assert np.array_equal(tot, d[nm + "_tot"]), nm
        if sizes.size <= 3:
            assert np.array_equal(w, d[nm + "_w"]), nm
            assert obj == float(d[nm + "_obj"]), nm
            assert sub.dtype == np.int32
        else:
            assert np.allclose(w, d[nm + "_w"], rtol=1e-5, atol=1e-10), nm
            assert np.isclose(obj, float(d[nm + "_obj"]), rtol=1e-5, atol=1e-10), nm
        assert np.allclose(yrec, d[nm + "_yrec"], rtol=1e-5, atol=1e-10), nm


def test_three_large_dictionaries_against_the_oracle():
    """[72, 72, 72]: 373 248 tuples, where the one-problem path switches to its matrix-pipe screen and the batch does
    not: indices against the oracle only."""
    from oracle import oracle as orc
    rng = np.random.default_rng(72)
    sz = np.array([72, 72, 72])
    A = np.abs(rng.standard_normal((30, 216)))
    Y = np.stack([0.7 * A[:, 5] + 0.2 * A[:, 72 + 40] + 0.2 * A[:, 144 + 71] + 0.01 * rng.standard_normal(30),
                  0.5 * A[:, 71] + 0.4 * A[:, 72] + 0.01 * rng.standard_normal(30)])
    got = _mfu().solve_exhaustive_posweights_batch(A, Y, sz)
    for v in range(2):
        ref = orc.solve_exhaustive_posweights(A, Y[v].copy(), sz)
        assert np.array_equal(got[1][v], ref[1]) and np.array_equal(got[2][v], ref[2]) and got[5][v] == 0


def test_ties_duplicate_columns():
    """Duplicated columns -> exact ties -> first hit in scan order (test_solver_gpu.py:127-133), on both routes."""
    from oracle import oracle as orc
    mfu = _mfu()
    rng = np.random.default_rng(77)
    A = np.abs(rng.standard_normal((12, 6)))
    A[:, 4] = A[:, 3]
    sz = np.array([3, 3])
    Y = np.stack([2.0 * A[:, 0] + 1.0 * A[:, 3], 1.0 * A[:, 2] + 0.5 * A[:, 4], 3.0 * A[:, 4]])
    rows = [mfu.solve_exhaustive_posweights(A, y.copy(), sz) for y in Y]
    with mfu.ExhaustiveSolver(A, sz) as S:
        for route in (contextlib.nullcontext, forced_generic):
            with route():
                got = S.solve(Y)
            assert_rows_equal(got, rows, route.__name__)
            for v in range(3):
                assert np.array_equal(got[1][v], orc.solve_exhaustive_posweights(A, Y[v].copy(), sz)[1])


def test_candidate_list_overflow():
    """[140, 140] with every column identical: 19600 tied tuples, more than the candidate list holds; the overflow rule
    runs on the one-problem path's block partition, so the result is that path's, bit for bit, on both routes."""
    mfu = _mfu()
    rng = np.random.default_rng(140)
    M = 12
    col = np.abs(rng.standard_normal(M))
    A = np.tile(col[:, None], (1, 280))
    sz = np.array([140, 140])
    Y = np.stack([1.5 * col, col + 0.01 * rng.standard_normal(M), 0.3 * col + 0.05 * np.abs(rng.standard_normal(M))])
    rows = [mfu.solve_exhaustive_posweights(A, y.copy(), sz) for y in Y]
    with mfu.ExhaustiveSolver(A, sz) as S:
        assert_rows_equal(S.solve(Y), rows, "tiled route")
        with forced_generic():
            assert_rows_equal(S.solve(Y), rows, "generic route")


@pytest.mark.parametrize("sizes", [(65, 63), (33, 31, 1), (6, 5, 4, 3)], ids=["65x63", "33x31x1", "6x5x4x3"])
def test_non_finite_signal(sizes):
    mfu = _mfu()
    A, Y, sz, rows = reference(sizes, 17)
    Yb = np.array(Y[:9])
    Yb[4, 3] = np.nan
    Yb[7, 0] = np.inf
    with mfu.ExhaustiveSolver(A, sz) as S:
        clean = S.solve(Y[:9])
        w, sub, tot, obj, yrec, status = S.solve(Yb)
    assert list(status) == [0, 0, 0, 0, 1, 0, 0, 1, 0]
    for v in (4, 7):
        assert np.all(np.isnan(w[v])) and np.isnan(obj[v]) and np.all(np.isnan(yrec[v]))
        assert np.all(sub[v] == -1) and np.all(tot[v] == -1)
    keep = [0, 1, 2, 3, 5, 6, 8]
    for got, ref in zip((w, sub, tot, obj, yrec, status), clean):
        assert np.array_equal(got[keep], ref[keep])
    assert_rows_equal(tuple(x[keep] for x in (w, sub, tot, obj, yrec, status)), [rows[v] for v in keep])


def test_device_route():
    """engine.solve_batch_dev on torch tensors equals .solve bit for bit; recons=False writes nothing; a handle's calls
    are independent of each other; two handles live side by side."""
    import torch
    from microstructure_fingerprinting_amd import engine
    mfu = _mfu()
    A, Y, sz, rows = reference((65, 63), 17)
    A3, Y3, sz3, rows3 = reference((33, 31, 1), 17)
    with mfu.ExhaustiveSolver(A, sz) as S, mfu.ExhaustiveSolver(A3, sz3) as S3:
        host = S.solve(Y)
        dY = torch.from_numpy(np.array(Y)).cuda()
        w, sub, tot, obj, yrec, status = engine.solve_batch_dev(S, dY)
        assert sub.dtype == torch.int64 and tot.dtype == torch.int64 and status.dtype == torch.int32
        for got, ref in zip((w, sub, tot, obj, yrec, status), host):
            assert np.array_equal(got.cpu().numpy(), ref)
        # recons=False: None, and a buffer offered for it is left alone; the other outputs land in the caller's tensors
        keep = torch.full((V, 17), -7.0, dtype=torch.float64, device='cuda')
        out = {'w': torch.empty((V, 2), dtype=torch.float64, device='cuda'), 'yrec': keep}
        r = engine.solve_batch_dev(S, dY, out=out, recons=False)
        assert r[4] is None and r[0] is out['w'] and bool(torch.all(keep == -7.0))
        assert np.array_equal(r[0].cpu().numpy(), host[0]) and np.array_equal(r[3].cpu().numpy(), host[3])
        # the other handle in between, then other signals on the first one: every call stands alone
        assert_rows_equal(S3.solve(Y3), rows3, "second handle")
        perm = np.arange(V)[::-1].copy()
        assert_rows_equal(S.solve(np.array(Y)[perm]), [rows[v] for v in perm], "second call")
        assert_rows_equal(S.solve(Y), rows, "third call")
        one = engine.solve_batch_dev(S, dY[3])
        assert np.array_equal(one[0].cpu().numpy(), host[0][3:4]) and tuple(one[4].shape) == (1, 17)
        for bad in (dY[:, :-1].contiguous(), dY.reshape(1, V, 17)):
            with pytest.raises(ValueError, match=r"\(17, 128\)"):
                engine.solve_batch_dev(S, bad)
        with pytest.raises(ValueError, match="out\\['obj'\\] should be"):
            engine.solve_batch_dev(S, dY, out={'obj': torch.empty(V + 1, dtype=torch.float64, device='cuda')})
