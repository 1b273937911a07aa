"""The batched explicit-dictionary solver (include/mfx_solve.h, csrc/solve_batch.hip) where its first suite,
test_solve_batch_gpu.py, does not go: sweeps of more than one trip, batches that mix overflowed, ordinary, all-zero and
non-finite signals, the edges of the candidate list, the tie cases of the one-problem solver across the seams of the
64 x 64 tiles, near-twin atoms, signals of very different magnitudes, a row stride, a side stream.

The referee is the contract everywhere: row v equals solve_exhaustive_posweights(A, Y[v], dicsizes), bit for bit, dtypes
included.  Where a test says so, the CPU oracle is asked as well - exact in indices, weights and objective - so that
both solvers cannot be wrong together.  No comparison has a tolerance.  The fixtures are tests/_solve_batch_cases.py; what
makes them meaningful (how many pairs tie, straddle a seam, lie inside the window) is asserted without a GPU in
test_solve_batch_referee_host.py.  The loop of one-problem solves of a fixture is made once per process.

THE SWEEP.  On the tiled route mfx_solve_batch_dev launches sb_tile_kernel on dim3(ntiles, ny) with
ntiles = ceil(n1 / 64) ceil(n2 / 64) and ny = max(1, min(nv, ceil(2048 / ntiles))) for a chunk of nv signals; workgroup
(tile, y) handles the signals y, y + ny, ..: ceil(nv / ny) trips.  A chunk holds min(V, 65 535, max_bytes /
bytes_per_signal) signals.  On the generic route the grid is dim3(nblocks, nv), one signal a row of the grid.
  A1  [150, 149] (, 1), V = 500: ntiles = 3 x 3 = 9, ny = ceil(2048 / 9) = 228: three trips of 228 / 228 / 44 signals.
      With max_bytes = 300 bytes_per_signal: a chunk of 300 (ny = 228: two trips, 228 / 72), then a chunk of 200
      (ny = min(200, 228) = 200: one trip).  Rows 3, 230 and 499 - one per trip - are non-finite, row 229 is all zero.
  A2  [1500, 1500], V = 9: ntiles = 24 x 24 = 576, ny = ceil(2048 / 576) = 4: three trips of 4 / 4 / 1 signals.
      sb_overflow_kernel: min(8192, ceil(2 250 000 / 256)) = 8192 blocks loop over the 9 signals.
  A3  [2, 2], V = 65 541: ntiles = 1; a chunk of 65 535 (ny = min(65 535, 2048) = 2048: 32 trips, 31 of 2048 signals and
      one of 2047), then a chunk of 6 (ny = 6: one trip).  Generic route: gridDim.y = 65 535, then 6."""
import contextlib
import ctypes as ct

import numpy as np
import pytest

import _solve_batch_cases as B
import _ties_cases as TC
from test_solve_batch_gpu import assert_rows_equal, forced_generic, reference

pytestmark = pytest.mark.gpu

ROUTES = {"tiled": contextlib.nullcontext, "generic": forced_generic}
_loops = {}


def _mfu():
    from microstructure_fingerprinting_amd import mf_utils as mfu
    return mfu


def loop(key, A, Y, sz, keep=None):
    """The one-problem solves of the rows `keep` (all of them by default) of a fixture, made once per process."""
    if key not in _loops:
        _loops[key] = [_mfu().solve_exhaustive_posweights(A, Y[v].copy(), sz) for v in (range(Y.shape[0]) if keep is None else keep)]
    return _loops[key]


def rows_of(got, keep):
    return tuple(x[keep] if x is not None else None for x in got)


def assert_bad_rows(got, bad):
    w, sub, tot, obj, yrec, status = got
    for v in bad:
        assert status[v] == 1, v
        assert np.all(np.isnan(w[v])) and np.isnan(obj[v]) and np.all(np.isnan(yrec[v])), v
        assert np.all(sub[v] == -1) and np.all(tot[v] == -1), v
    assert np.count_nonzero(status) == len(bad)


def assert_oracle_exact(got, A, Y, sz, keep=None, what=""):
    """indices, weights and objective of the CPU oracle, exact (up to three sub-dictionaries: the oracle's arithmetic)"""
    from oracle import oracle as orc
    for v in (range(Y.shape[0]) if keep is None else keep):
        ref = orc.solve_exhaustive_posweights(A, Y[v].copy(), sz)
        tag = "%s signal %d: %s, oracle %s" % (what, v, got[1][v], ref[1])
        assert np.array_equal(got[1][v], ref[1]) and np.array_equal(got[2][v], ref[2]), tag
        assert np.array_equal(got[0][v], ref[0]) and got[3][v] == ref[3], tag


# ---- A. sweeps of more than one trip
@pytest.mark.parametrize("route", sorted(ROUTES))
@pytest.mark.parametrize("sizes", B.SWEEP_SHAPES, ids=TC.shape_id)
def test_sweep_of_three_trips(sizes, route):
    """A1.  500 signals over 9 tiles: trips of 228 / 228 / 44; in chunks of 300 + 200: trips of 228 / 72, then one."""
    A, Y, sz = B.sweep_problem(sizes)
    keep = [v for v in range(B.SWEEP_V) if v not in B.SWEEP_BAD]
    rows = loop(("sweep", sizes), A, Y, sz, keep)
    with _mfu().ExhaustiveSolver(A, sz) as S, ROUTES[route]():
        for what, max_bytes in (("one chunk", 0), ("chunks of 300 + 200", 300 * S.bytes_per_signal)):
            got = S.solve(Y, max_bytes=max_bytes)
            assert_bad_rows(got, B.SWEEP_BAD)
            assert_rows_equal(rows_of(got, keep), rows, "%s, %s" % (route, what))


@pytest.mark.parametrize("route", sorted(ROUTES))
def test_sweep_over_576_tiles_planted(route):
    """A2.  [1500, 1500], nine signals planted in nine tiles (the first, the ragged last, both sides of a seam): trips of
    4 / 4 / 1.  The loop, and the oracle's exact answer."""
    A, Y, sz = B.planted_problem()
    rows = loop("planted", A, Y, sz)
    with _mfu().ExhaustiveSolver(A, sz) as S, ROUTES[route]():
        got = S.solve(Y)
    assert [tuple(int(i) for i in s) for s in got[1]] == B.PLANTED9
    assert_rows_equal(got, rows, route)
    assert_oracle_exact(got, A, Y, sz, what=route)


@pytest.mark.parametrize("route", sorted(ROUTES))
def test_sweep_over_576_tiles_every_signal_overflows(route):
    """A2.  2 250 000 exact ties in each of nine signals: the tiled collect breaks out of its rows in every trip and
    sb_overflow_kernel loops over the nine signals on 8192 blocks.  The loop; the oracle's indices (0, 0)."""
    A, Y, sz = B.all_tied_batch()
    rows = loop("all tied", A, Y, sz)
    with _mfu().ExhaustiveSolver(A, sz) as S, ROUTES[route]():
        got = S.solve(Y)
    assert_rows_equal(got, rows, route)
    assert np.all(got[1] == 0) and np.all(got[0][:, 1] == 0.0)
    assert_oracle_exact(got, A, Y, sz, what=route)


@pytest.mark.parametrize("sizes,route", [((2, 2), "tiled"), ((2, 2), "generic"), ((3,), "generic")],
                         ids=["2x2-tiled", "2x2-generic", "3-generic"])
def test_chunk_clamp_at_65535_signals(sizes, route):
    """A3.  65 541 signals, 37 distinct: chunks of 65 535 + 6.  Tiled: 32 trips; generic: gridDim.y = 65 535.  The whole
    arrays at once against the 37 one-problem results."""
    A, base, sz = B.clamp_problem(sizes)
    rows = loop(("clamp", sizes), A, base, sz)
    idx = np.arange(B.CLAMP_V) % B.CLAMP_DISTINCT
    Y = np.ascontiguousarray(base[idx])
    with _mfu().ExhaustiveSolver(A, sz) as S, ROUTES[route]():
        assert B.CLAMP_V * S.bytes_per_signal < (256 << 20)       # the byte budget does not cut the chunk first
        w, sub, tot, obj, yrec, status = S.solve(Y)
    ew, esub, etot, eobj, eyrec = (np.stack([np.asarray(r[k]) for r in rows])[idx] for k in range(5))
    assert not status.any() and status.shape == (B.CLAMP_V,)
    assert np.array_equal(sub, esub) and np.array_equal(tot, etot) and sub.dtype == esub.dtype and tot.dtype == etot.dtype
    assert np.array_equal(w, ew) and np.array_equal(obj, eobj) and np.array_equal(yrec, eyrec)
    assert w.dtype == np.float64 and obj.dtype == np.float64 and status.dtype == np.int32


# ---- B. overflowed and ordinary signals in one batch; the edges of the candidate list
@pytest.mark.parametrize("route", sorted(ROUTES))
def test_overflowed_and_ordinary_signals_in_one_batch(route):
    """Twelve signals: four overflow (19 500 exact ties), four have a unique optimum, one ties 130-fold, one is all zero,
    two are non-finite.  In one chunk and in chunks of 5 + 5 + 2.  The loop on every finite row, and the oracle's
    indices on every finite row (the host test finds no rounding-level partner in any of them)."""
    A, Y, sz, _, _ = B.mixed_problem()
    bad = [v for v, k in enumerate(B.MIXED_KINDS) if k in ("nan", "inf")]
    keep = [v for v in range(len(B.MIXED_KINDS)) if v not in bad]
    rows = loop("mixed", A, Y, sz, keep)
    with _mfu().ExhaustiveSolver(A, sz) as S, ROUTES[route]():
        for what, max_bytes in (("one chunk", 0), ("chunks of 5", 5 * S.bytes_per_signal)):
            got = S.solve(Y, max_bytes=max_bytes)
            assert_bad_rows(got, bad)
            assert_rows_equal(rows_of(got, keep), rows, "%s, %s" % (route, what))
            assert_oracle_exact(got, A, Y, sz, keep, "%s, %s" % (route, what))


@pytest.mark.parametrize("sizes,what", B.CAP_EDGES, ids=[TC.shape_id(s) for s, _ in B.CAP_EDGES])
def test_candidate_list_edges(sizes, what):
    """Identical columns: 16 384 ties fill the list exactly and nothing overflows; 16 512 overflow by 128; 16 383 leave one
    entry free."""
    A, Y, sz = B.cap_edge_problem(sizes)
    rows = loop(("cap", sizes), A, Y, sz)
    with _mfu().ExhaustiveSolver(A, sz) as S:
        for route in sorted(ROUTES):
            with ROUTES[route]():
                assert_rows_equal(S.solve(Y), rows, "%s, %s" % (what, route))


# ---- C. the tie cases of the one-problem solver, through the batch
@pytest.mark.parametrize("sizes", B.MIRROR_SHAPES, ids=TC.shape_id)
def test_mirrored_subdictionaries_across_a_tile_seam(sizes):
    """Two bit-identical sub-dictionaries of 70 atoms: (i, j) and (j, i) hold the same columns and, for a pair that straddles
    column 64, lie in the tiles (0, 1) and (1, 0).  The loop bit for bit and the oracle exact, on both routes and in
    chunks of 7."""
    A, Y, sz, _ = B.mirror_problem(sizes)
    rows = loop(("mirror", sizes), A, Y, sz)
    with _mfu().ExhaustiveSolver(A, sz) as S:
        for route in sorted(ROUTES):
            with ROUTES[route]():
                for what, max_bytes in (("one chunk", 0), ("chunks of 7", 7 * S.bytes_per_signal)):
                    got = S.solve(Y, max_bytes=max_bytes)
                    assert_rows_equal(got, rows, "%s, %s" % (route, what))
                    assert_oracle_exact(got, A, Y, sz, what="%s, %s" % (route, what))


def test_tie_across_column_tiles_and_waves():
    """[3, 300]: the tied tuples (0, 5), (0, 290), (2, 5), (2, 290) lie in column tiles 0 and 4 and in the rows of waves 0
    and 2; three signals made of those two vectors.  The oracle's first hit, (0, 5), on both routes."""
    A, Y, sz = B.two_block_batch()
    rows = loop("two block", A, Y, sz)
    with _mfu().ExhaustiveSolver(A, sz) as S:
        for route in sorted(ROUTES):
            with ROUTES[route]():
                got = S.solve(Y)
            assert [tuple(int(i) for i in s) for s in got[1]] == [(0, 5)] * 3, route
            assert_rows_equal(got, rows, route)
            assert_oracle_exact(got, A, Y, sz, what=route)


@pytest.mark.parametrize("kind", ["within", "cross", "tiled twin"])
def test_k3_ties_follow_the_reference_order(kind):
    """[4, 3, 4], a generic class: the reference's i3 -> i1 -> i2 order decides exact ties in sb_finalize_kernel; and a twin of
    the tiled class, [4, 3, 1] with a duplicated column in the first sub-dictionary.  V = 1, seeds 0 .. 7."""
    mfu = _mfu()
    for seed in range(8):
        A, y, sz = B.k3_tiled_twin(seed) if kind == "tiled twin" else TC.k3_order_problem(kind, seed)
        row = [mfu.solve_exhaustive_posweights(A, y.copy(), sz)]
        with mfu.ExhaustiveSolver(A, sz) as S:
            for route in sorted(ROUTES):
                with ROUTES[route]():
                    got = S.solve(y)
                assert_rows_equal(got, row, "%s %d, %s" % (kind, seed, route))
                assert_oracle_exact(got, A, y[None, :], sz, what="%s %d, %s" % (kind, seed, route))


# ---- D. near-twin atoms; magnitudes
@pytest.mark.parametrize("csf", [False, True], ids=["96x96", "96x96x1"])
@pytest.mark.parametrize("ladder", sorted(B.TWIN_FLOOR))
def test_near_twin_atoms(ladder, csf):
    """Families of 8 near copies per atom in both sub-dictionaries: runners-up inside 1e-9 |y|^2 in 14 of 48 signals
    (margin ladder) and in all 48, up to 64 pairs (window ladder) - where the error bound MFX_SCORE_ERR ysq / rel with
    sb_rel_kernel's tabulated rel decides what is listed.  The loop bit for bit and the oracle exact, on both routes."""
    A, Y, sz = B.twin_problem(ladder, csf)
    rows = loop(("twin", ladder, csf), A, Y, sz)
    with _mfu().ExhaustiveSolver(A, sz) as S:
        for route in sorted(ROUTES):
            with ROUTES[route]():
                got = S.solve(Y)
            assert_rows_equal(got, rows, "%s, %s" % (ladder, route))
            assert_oracle_exact(got, A, Y, sz, what="%s, %s" % (ladder, route))


@pytest.mark.parametrize("sizes", [(65, 63), (33, 31, 1)], ids=TC.shape_id)
def test_magnitudes_of_600_binades_in_one_batch(sizes):
    """The rows of a test_solve_batch_gpu problem times 2^k, k cycling through -300, -40, 0, 40, 300: smax, the tie
    threshold and the error bound are per signal.  The loop on every scaled row; the indices of the unscaled row wherever
    the one-problem solver itself returns them for both (the count is printed: a covariance the one-problem solver does
    not have is not asked of the batch)."""
    A, Y, sz, rows = reference(sizes, 17)
    Ys = np.ascontiguousarray(Y * B.magnitude_scales(Y.shape[0])[:, None])
    assert np.all(np.isfinite(Ys)) and np.all(np.isfinite(np.sum(Ys * Ys, axis=1)))
    scaled = loop(("magnitudes", sizes), A, Ys, sz)
    same = [v for v in range(Y.shape[0]) if np.array_equal(scaled[v][1], rows[v][1])]
    print("%s: the one-problem solver returns the unscaled row's indices in %d of %d scaled rows" % (sizes, len(same), Y.shape[0]))
    with _mfu().ExhaustiveSolver(A, sz) as S:
        for route in sorted(ROUTES):
            with ROUTES[route]():
                got = S.solve(Ys)
            assert_rows_equal(got, scaled, route)
            for v in same:
                assert np.array_equal(got[1][v], rows[v][1]), (route, v)


# ---- E. plumbing
def test_create_with_a_row_stride_larger_than_the_columns():
    """mfx_solve_create with lda = Ntot + 8 and a pointer 3 columns into the row: the rows of the compact dictionary."""
    from microstructure_fingerprinting_amd import _lib
    mfu = _mfu()
    rng = np.random.default_rng(150)
    off, extra = 3, 8

    class Strided(mfu.ExhaustiveSolver):
        def __init__(self, wide, sizes):
            self._wide = wide
            super().__init__(np.ascontiguousarray(wide[:, off:off + int(sizes.sum())]), sizes)

        def handle(self):
            if self._h is None:
                h = ct.c_void_p()
                ptr = ct.cast(self._wide.ctypes.data + 8 * off, ct.POINTER(ct.c_double))
                _lib.check(_lib.lib().mfx_solve_create(ptr, self._wide.shape[1], self.M, _lib.lptr(self.dicsizes), self.Kp, self.device,
                                                       ct.byref(h)))
                self._h = h
            return self._h

    for sizes in ([9, 7, 1], [70, 5], [6, 5, 4]):
        sz = np.array(sizes, dtype=np.int64)
        Ntot, M = int(sz.sum()), 14
        wide = np.abs(rng.standard_normal((M, Ntot + extra))) + 0.2
        Ac = np.ascontiguousarray(wide[:, off:off + Ntot])
        starts = np.concatenate(([0], np.cumsum(sz)[:-1]))
        Y = np.stack([Ac[:, starts + rng.integers(sz)] @ np.linspace(0.6, 0.2, sz.size) + 0.01 * rng.standard_normal(M) for _ in range(9)])
        rows = [mfu.solve_exhaustive_posweights(Ac, y.copy(), sz) for y in Y]
        with Strided(wide, sz) as S, mfu.ExhaustiveSolver(Ac, sz) as Sc:
            strided, compact = S.solve(Y), Sc.solve(Y)
            for s, c in zip(strided, compact):
                assert np.array_equal(s, c)
            assert_rows_equal(strided, rows, "lda %d, %s" % (Ntot + extra, sizes))
            with forced_generic():
                assert_rows_equal(S.solve(Y), rows, "lda %d, %s, generic route" % (Ntot + extra, sizes))


def test_device_route_on_a_side_stream():
    """engine.solve_batch_dev inside torch.cuda.stream(side): the signals are produced on that stream, behind work that
    keeps it busy, and go through in two chunks; after the stream is synchronised the rows are those of .solve.  Then a
    call on the default stream with the same handle."""
    import torch
    from microstructure_fingerprinting_amd import engine
    mfu = _mfu()
    A, Y, sz, rows = reference((65, 63), 17)
    Y2 = np.ascontiguousarray(np.concatenate([Y, Y[::-1]]))
    rows2 = rows + rows[::-1]
    with mfu.ExhaustiveSolver(A, sz) as S:
        budget = 40 * S.bytes_per_signal                      # 74 signals: chunks of 40 + 34
        host = S.solve(Y2, max_bytes=budget)
        assert_rows_equal(host, rows2, "host")
        half = torch.from_numpy(0.5 * Y2).cuda()
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            busy = torch.ones((2048, 2048), device="cuda")
            for _ in range(4):
                busy = busy @ busy * 1e-4
            dY = half + half                                  # exact: the signals, written on the side stream
            out = engine.solve_batch_dev(S, dY, max_bytes=budget)
        side.synchronize()
        for got, ref in zip(out, host):
            assert np.array_equal(got.cpu().numpy(), ref)
        assert torch.cuda.current_stream() == torch.cuda.default_stream()
        again = engine.solve_batch_dev(S, dY[:37].contiguous())
        torch.cuda.synchronize()
        for got, ref in zip(again, host):
            assert np.array_equal(got.cpu().numpy(), ref[:37])
        assert bool(torch.isfinite(busy).all())
