"""Guards of tests/test_solve_batch_referee_gpu.py that need no GPU: the fixtures of tests/_solve_batch_cases.py still are
the batches that test is about - judged on the CPU oracle and on numpy alone (pairs_in_window: the closed-form objective
of every pair), never on the library.  Every test prints the populations it measured (pytest -s)."""
import numpy as np
import pytest

import _solve_batch_cases as B
import _ties_cases as TC
from oracle import oracle as orc


def _oracle_rows(A, Y, sz):
    return [orc.solve_exhaustive_posweights(A, Y[v].copy(), sz) for v in range(Y.shape[0])]


def test_pairs_in_window_is_the_oracles_objective():
    """The helper's best objective is the oracle's min_obj, bit for bit, and its first best pair in scan order the
    oracle's pair: on a plain problem, on exact ties and on the all-zero signal."""
    A, Y, sz, _, _ = B.mixed_problem()
    for v, kind in enumerate(B.MIXED_KINDS):
        if kind in ("nan", "inf"):
            continue
        res, ysq = B.pair_objectives(A[:, :140], A[:, 140:], Y[v])
        w, sub, _, obj, _ = orc.solve_exhaustive_posweights(A, Y[v].copy(), sz)
        assert res.min() == obj, (v, kind)
        assert np.unravel_index(np.argmin(res), res.shape) == tuple(sub), (v, kind)
    assert B.pairs_in_window(A[:, :140], A[:, 140:], Y[4]) == (19600, 19600)      # all zero: every objective is 0


def test_sweep_batches_have_their_special_rows():
    """A1: 500 rows, exactly three of them non-finite - one in each trip of 228 / 228 / 44, row 230 next to the all-zero
    row 229 right behind the first trip's end - and every other row a finite non-zero signal."""
    for sizes in B.SWEEP_SHAPES:
        A, Y, sz = B.sweep_problem(sizes)
        assert Y.shape == (B.SWEEP_V, B.SWEEP_M) and A.shape == (B.SWEEP_M, sum(sizes))
        bad = np.flatnonzero(~np.all(np.isfinite(Y), axis=1))
        assert tuple(bad) == B.SWEEP_BAD and sorted({int(v) // 228 for v in bad}) == [0, 1, 2]
        zero = np.flatnonzero(np.all(Y == 0, axis=1))
        assert tuple(zero) == (B.SWEEP_ZERO,) and B.SWEEP_ZERO == 228 + 1
        assert np.isnan(Y[3]).any() and np.isposinf(Y[230]).any() and np.isneginf(Y[499]).any()


def test_planted_signals_sit_in_nine_different_tiles():
    """A2: the oracle returns every planted pair; the pairs lie in nine different 64 x 64 tiles, among them the first, the
    ragged last one (28 x 28) and the scan's second grid-stride trip; every signal of the all-tied batch ties everywhere
    and the oracle answers (0, 0)."""
    A, Y, sz = B.planted_problem()
    tiles = {(i // 64, j // 64) for i, j in B.PLANTED9}
    assert len(tiles) == 9 and (0, 0) in tiles and (23, 23) in tiles and TC.PLANTED in B.PLANTED9
    assert 1500 - 23 * 64 == 28 and (1499, 1499) in B.PLANTED9
    for (i, j), ref in zip(B.PLANTED9, _oracle_rows(A, Y, sz)):
        assert tuple(ref[1]) == (i, j)
    A, Y, sz = B.all_tied_batch()
    assert np.all(A == A[:, :1])          # one vector in all 3000 columns: every pair's Gram and A^T y are the same bits
    for ref in _oracle_rows(A, Y, sz):
        assert tuple(ref[1]) == (0, 0) and ref[0][0] > 0.25 and ref[0][1] == 0.0
    print("A2: 9 planted pairs in 9 tiles recovered by the oracle; 9 signals of 2 250 000 exact ties each")


def test_clamp_batch_crosses_the_chunk_limit():
    assert B.CLAMP_V == 65535 + 6
    for sizes in ((2, 2), (3,)):
        A, base, sz = B.clamp_problem(sizes)
        assert base.shape == (B.CLAMP_DISTINCT, 3) and len({tuple(b) for b in base}) == B.CLAMP_DISTINCT
        idx = np.arange(B.CLAMP_V) % B.CLAMP_DISTINCT
        assert idx[65535] != idx[0]       # the second chunk does not start on the first chunk's first signal


def test_mixed_batch_populations():
    """B: more than 16 384 exact ties in every "overflow" row, at most 130 in every other finite non-zero row (the all-zero
    row ties everywhere at objective 0 and lists nothing: its score is not positive); r . d_k <= -1.01 for the 20
    distinct columns; the oracle's answers - (0, 0) with weights (a, 0) for the overflow rows, the planted pairs for the
    unique rows.  No finite row has a rounding-level partner: the window holds the exact ties and nothing else."""
    A, Y, sz, c, r = B.mixed_problem()
    assert len(B.MIXED_KINDS) == 12 and Y.shape == (12, 12)
    D = A[:, np.concatenate((B.MIXED_DISTINCT, 140 + B.MIXED_DISTINCT))]
    assert D.shape[1] == 20 and not np.any(np.all(D == c[:, None], axis=0))
    assert np.count_nonzero(np.all(A == c[:, None], axis=0)) == 260
    print("B: max r . d_k = %.4f" % (r @ D).max())
    assert (r @ D).max() <= -1.01
    amps = iter((1.2, 0.4, 0.8, 2.0))
    for v, kind in enumerate(B.MIXED_KINDS):
        if kind in ("nan", "inf"):
            assert not np.all(np.isfinite(Y[v]))
            continue
        assert np.all(np.isfinite(Y[v]))
        if kind == "zero":
            assert not Y[v].any()
            continue
        near, exact = B.pairs_in_window(A[:, :140], A[:, 140:], Y[v])
        w, sub, _, _, _ = orc.solve_exhaustive_posweights(A, Y[v].copy(), sz)
        print("B: row %2d %-8s %5d exact ties, %5d pairs in the window, oracle %s w %s" % (v, kind, exact, near, sub, w))
        assert near == exact, "a rounding-level partner in row %d: do not use it" % v
        if kind == "overflow":
            assert exact == 19500 > B.SCAN_CAP
            assert tuple(sub) == (0, 0) and abs(w[0] - next(amps)) < 1e-12 and w[1] == 0.0
        else:
            assert exact <= 130
            assert exact == (130 if kind == "ties130" else 1)
            assert tuple(sub) == (B.MIXED_PLANTED[v] if kind == "unique" else (0, 34))


def test_cap_edges_tie_exactly_at_the_list_size():
    for sizes, what in B.CAP_EDGES:
        A, Y, sz = B.cap_edge_problem(sizes)
        n = sizes[0] * sizes[1]
        for y in Y:
            assert B.pairs_in_window(A[:, :sizes[0]], A[:, sizes[0]:], y) == (n, n)
        print("cap edge %s: %d exact ties (%s)" % (sizes, n, what))
    assert [s[0] * s[1] - B.SCAN_CAP for s, _ in B.CAP_EDGES] == [0, 128, -1]


@pytest.mark.parametrize("sizes", B.MIRROR_SHAPES, ids=TC.shape_id)
def test_mirror_batch_keeps_its_power(sizes):
    """C: at least 10 of the 60 pairs straddle the seam between columns 63 and 64, and in at least 5 signals the oracle
    returns sub[0] > sub[1], the second of the two mirrored tuples in tuple-number order; in at least 3 signals it does so
    for a straddling pair, where the mirror tuple lies in the other tile (measured: 15 straddling; swapped 9 on (70, 70)
    and 26 on (70, 70, 1), 5 and 7 of them straddling)."""
    A, Y, sz, pairs = B.mirror_problem(sizes)
    assert np.array_equal(A[:, :70], A[:, 70:140])
    rows = _oracle_rows(A, Y, sz)
    swapped = sum(1 for ref in rows if ref[1][0] > ref[1][1])
    swapped_straddling = sum(1 for ref in rows if ref[1][0] > ref[1][1] and B.straddling(ref[1][None, :2]))
    print("C: %s: %d of %d pairs straddle the seam, the oracle returns sub[0] > sub[1] in %d signals (%d of them straddling)"
          % (sizes, B.straddling(pairs), B.MIRROR_V, swapped, swapped_straddling))
    assert B.straddling(pairs) >= 10 and swapped >= 5 and swapped_straddling >= 3
    for ref, p in zip(rows, pairs):
        assert set(ref[1][:2]) == set(p)       # the planted atoms, in one order or the other


def test_tie_problems_have_the_oracles_first_hit():
    """C: [3, 300] - all three signals are made of the same two vectors and the oracle's first hit is (0, 5); the tied
    tuples 5, 290, 605, 890 lie in column tiles 0 and 4 and in rows of waves 0 and 2.  [4, 3, 1]: (0, 1, 0) before
    (3, 1, 0)."""
    A, Y, sz = B.two_block_batch()
    assert np.array_equal(A[:, 2], A[:, 0]) and np.array_equal(A[:, 3 + 290], A[:, 3 + 5])
    assert (5 // 64, 290 // 64) == (0, 4) and (0 % 4, 2 % 4) == (0, 2)
    for ref in _oracle_rows(A, Y, sz):
        assert tuple(ref[1]) == (0, 5)
    for seed in range(8):
        A, y, sz = B.k3_tiled_twin(seed)
        assert np.array_equal(A[:, 3], A[:, 0])
        w, sub, _, _, _ = orc.solve_exhaustive_posweights(A, y, sz)
        assert tuple(sub) == (0, 1, 0) and np.all(w > 0.05)


@pytest.mark.parametrize("ladder", sorted(B.TWIN_FLOOR))
def test_twin_batches_populate_the_window(ladder):
    """D: the number of signals in which a runner-up lies within 1e-9 |y|^2 of the best pair, by pairs_in_window (measured:
    14 of 48 on the margin ladder, at most 23 pairs; 48 of 48 on the window ladder, at most 64 pairs).  The floors, 10
    and 40, are the test's power."""
    A, Y, sz = B.twin_problem(ladder, False)
    near = [B.pairs_in_window(A[:, :96], A[:, 96:], Y[v])[0] for v in range(B.TWIN_V)]
    populated = sum(1 for n in near if n > 1)
    print("D: %s ladder: a runner-up inside the window in %d of %d signals, at most %d pairs" % (ladder, populated, B.TWIN_V, max(near)))
    assert populated >= B.TWIN_FLOOR[ladder]
    A3, Y3, sz3 = B.twin_problem(ladder, True)
    assert np.array_equal(A3[:, :192], A) and np.array_equal(Y3, Y) and tuple(sz3) == (96, 96, 1)


def test_magnitude_scales_are_exact_and_normal():
    s = B.magnitude_scales(37)
    assert set(np.log2(s)) == set(B.MAGNITUDES) and np.all(np.isfinite(s * s)) and np.all(s * s >= np.finfo(float).tiny)
    y = np.random.default_rng(0).standard_normal(17)
    for k in s[:5]:
        assert np.array_equal((y * k) / k, y)
