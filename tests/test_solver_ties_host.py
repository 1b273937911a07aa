"""Guards of tests/test_solver_ties_gpu.py that need no GPU: the generators of tests/_ties_cases.py still produce
the problems that test is about, judged on the CPU oracle's answers alone."""
import numpy as np
import pytest

import _ties_cases as C
from oracle import oracle as orc


@pytest.mark.parametrize("sizes,M", C.ONE_BLOCK, ids=C.shape_id)
def test_symmetric_problems_keep_their_power(sizes, M):
    """In at least 5 of the 60 problems of every one-block shape the oracle returns sub[0] > sub[1]: the second of
    the two mirrored tuples in tuple-number order (measured: 7, 6, 25, 32)."""
    n = C.swapped(C.symmetric_reference(sizes, M))
    print("%s: sub[0] > sub[1] in %d of %d problems" % (sizes, n, len(C.SEEDS)))
    assert n >= 5


@pytest.mark.parametrize("sizes,M", C.FOUR, ids=C.shape_id)
def test_four_dictionary_mirrors_tie_exactly_in_the_oracle(sizes, M):
    """K' = 4 with two identical sub-dictionaries: in every problem the two atoms differ and carry weight, the
    mirrored tuple's objective equals the winner's bit for bit, and the oracle returns the first of the two
    (sub[0] < sub[1]) - so the GPU test may ask for the oracle's fascicle indices exactly (the EAR index where the EAR
    compartment is active, as everywhere for K' >= 4)."""
    N = sizes[0]
    for A, y, ds, (w, sub, tot, obj, yrec) in C.symmetric_reference_four(sizes, M):
        assert sub[0] < sub[1] and w[0] > 0.1 and w[1] > 0.1
        pick = lambda s0, s1: np.ascontiguousarray(A[:, [s0, N + s1, 2 * N, 2 * N + 1 + sub[3]]])
        one = np.ones(4, dtype=np.int64)
        assert orc.solve_exhaustive_posweights(pick(sub[1], sub[0]), y, one)[3] == orc.solve_exhaustive_posweights(pick(sub[0], sub[1]), y, one)[3] == obj


def test_fit_path_voxels_keep_their_power():
    """The identical-peak voxels of the fit-path tests: the two atoms differ in every voxel, and in at least 5 of 24
    the oracle returns them as (larger, smaller) (measured: 8 without and 13 with the CSF column)."""
    sch, _, T, sig_csf = C.c2_model(16)
    V = 24
    for csf in (None, sig_csf):
        peaks, Y = C.identical_peak_voxels(sch, T, V, 3, csf)
        on = csf is not None
        ref = orc.fit_batch(T, sch, Y, np.full(V, 2), np.full(V, on), np.zeros(V, bool), peaks, 2, on, False, csf, None, 0, nthreads=4)
        assert np.all(ref[:, 3] != ref[:, 4])
        assert np.count_nonzero(ref[:, 3] > ref[:, 4]) >= 5


def test_order_problems_tell_the_two_orders_apart():
    """'cross' problems: the oracle returns (0, 1, 3) - first in tuple-number order - for some seeds and (3, 1, 0) -
    first in its own i3 -> i1 -> i2 order - for others; 'within': always the first of the four tied triples."""
    got = {tuple(orc.solve_exhaustive_posweights(*C.k3_order_problem("cross", s))[1]) for s in range(8)}
    assert got == {(0, 1, 3), (3, 1, 0)}
    assert all(tuple(orc.solve_exhaustive_posweights(*C.k3_order_problem("within", s))[1]) == (0, 1, 0) for s in range(8))


def test_large_problems_have_the_planted_answers():
    w, sub, _, _, _ = orc.solve_exhaustive_posweights(*C.all_tied_problem())
    assert tuple(sub) == (0, 0) and abs(w[0] - 2.0) < 0.05 and w[1] == 0.0
    w, sub, _, _, _ = orc.solve_exhaustive_posweights(*C.all_tied_triples_problem())
    assert tuple(sub) == (1, 0, 0) and np.all(w > 0.1)
    _, sub, _, _, _ = orc.solve_exhaustive_posweights(*C.grid_stride_problem())
    assert tuple(sub) == C.PLANTED and C.PLANTED[0] * 1500 + C.PLANTED[1] >= 8192 * 256
    _, sub, _, _, _ = orc.solve_exhaustive_posweights(*C.two_block_tie_problem())
    assert tuple(sub) == (0, 5)


@pytest.mark.parametrize("Kp", [6, 7, 8])
def test_many_dictionaries_have_a_clear_optimum(Kp):
    """The oracle recovers the last atom of every sub-dictionary, and the runner-up over all tuples is more than
    1e-6 |y|^2 away (so the GPU test compares indices in every case)."""
    A, y, sizes = C.many_dictionaries_problem(Kp)
    gap, best = C.top2_gap(A, y, sizes)
    assert gap > 1e-6
    _, sub, _, _, _ = orc.solve_exhaustive_posweights(A, y, sizes)
    assert tuple(sub) == tuple(sizes - 1) == best
