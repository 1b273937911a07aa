"""The power of the near-twin population (tests/_twin_cases.py), on the CPU oracle alone: tests/test_twin_gpu.py referees
every fit path on it, and says something about a margin only while the population holds runners-up inside the margin,
scanned before the optimum.  These are conditions on the fixtures, not measurements of the library: the seeds in
_twin_cases.py are chosen so that they hold, and the measured values are printed."""
import numpy as np
import pytest

import _twin_cases as tc
import _units_cases as uc
import test_units_gpu as UG      # the dispatch table only: nothing of that module runs here

POPULATIONS = tc.populations(UG.PATHS)


def _ceil_div(a, b):
    return -(-a // b)


@pytest.mark.parametrize("pop", POPULATIONS, ids=tc.pop_id)
def test_population_has_power(pop):
    """Margin ladder: at least one voxel in six with a gap in (1e-9, 1e-6], one in six below 1e-9, one in four runner-up
    first.  Window ladder with 8 copies: the median number of family tuples within 1e-9 |y|^2 is at least 16 (one
    fascicle: a family has 7 other members, more than half of them, 4).  Both: 1 - c^2 >= 1e-6 between columns of
    different sub-dictionaries in every voxel (not the near-collinear regime, which begins at 1e-8), every oracle weight
    non-negative (the Cramer tolerance is inert)."""
    cls, dirs, nbase, copies, ladder = pop
    mdl = tc.model(dirs, nbase, copies, ladder)
    g = tc.gap_and_order(mdl, cls)
    rows = tc.oracle_rows(mdl, cls)
    V = rows.shape[0]
    gap = g["gap"]
    mid, low, high = int(np.sum((gap > 1e-9) & (gap <= 1e-6))), int(np.sum(gap <= 1e-9)), int(np.sum(gap > 1e-6))
    first = int(np.sum(g["first"]))
    wmin = float(rows[:, uc.weight_columns(cls)].min())
    print("%s: %d voxels; gap < 1e-9: %d, 1e-9 .. 1e-6: %d, > 1e-6: %d; runner-up first %d; tuples within 1e-9 median %g "
          "max %g; min 1 - c^2 %.2e; min oracle weight %.3e; max inconsistency %.2e"
          % (tc.pop_id(pop), V, low, mid, high, first, np.median(g["within"]), g["within"].max(), g["mincc"].min(), wmin,
             g["incons"].max()))
    if ladder == "margin":
        assert mid >= _ceil_div(V, 6) and low >= _ceil_div(V, 6) and first >= _ceil_div(V, 4), (low, mid, high, first)
    elif copies == 8:
        assert np.median(g["within"]) >= (16 if uc.CLASSES[cls][0] >= 2 else 4)
    assert g["mincc"].min() >= 1e-6
    assert wmin >= 0.0


def test_oracle_inconsistency_is_what_the_gpu_test_assumes():
    """max |orc.nnls re-score of the oracle's own tuple - min_obj| / |y|^2 over the whole population, and over the classes
    that the reference solves through an NNLS per tuple: not above the figures recorded in _twin_cases.py, from which
    test_twin_gpu's bound below the tie window is taken."""
    worst, worst4, n = 0.0, 0.0, 0
    for cls, dirs, nbase, copies, ladder in POPULATIONS:
        g = tc.gap_and_order(tc.model(dirs, nbase, copies, ladder), cls)
        n += g["incons"].size
        worst = max(worst, float(g["incons"].max()))
        if sum(uc.CLASSES[cls]) >= 4:
            worst4 = max(worst4, float(g["incons"].max()))
    print("oracle inconsistency over %d voxels: %.3e (four and more sub-dictionaries: %.3e); recorded %.3e, bound %.3e"
          % (n, worst, worst4, tc.INCONSISTENCY_MEASURED, tc.INCONSISTENCY))
    assert worst <= tc.INCONSISTENCY_MEASURED
