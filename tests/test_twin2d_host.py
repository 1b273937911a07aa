"""The power of the near-twin populations of the 2-D protocol fits (tests/_twin2d_cases.py), on the CPU alone: the
rotation is tests/_rot2d_ref.Referee, the solver the oracle.  tests/test_twin2d_gpu.py referees the kernels on these
populations and says something about an interval, a bound, a list or the overflow pass only while the populations reach
them.  These are conditions on the fixtures, not measurements of the library: the seeds in _twin2d_cases.py are chosen so
that they hold, no voxel is dropped to meet one, and the measured values are printed."""
import numpy as np
import pytest

import _twin2d_cases as t2

ALL = t2.CASES + [t2.FIX_CASE]


def _ceil_div(a, b):
    return -(-a // b)


@pytest.mark.parametrize("case", ALL, ids=t2.case_id)
def test_population_has_power(case):
    """Every direction rotates; 1 - c^2 >= 1e-6 between the two dictionaries' columns outside the identical-direction
    voxels; margin ladder: a third of the voxels with a gap < 1e-6 |y|^2 and one above 1e-4; window ladder: every gap
    <= 1e-9 |y|^2; the runner-up precedes the optimum in a quarter to three quarters of the voxels.

    1 x 64 on the margin ladder cannot hold a gap above 1e-4: all 4 095 other pairs are built from copies of the chosen
    atoms, 63 values of eps share 6.5 decades, and the optimum's nearest copy is never a whole 1e-4 |y|^2 away (largest
    gap over 8 dictionary seeds x 30 voxel seeds: 1.8e-5).  There the largest gap must exceed 1e-6 (measured 9.5e-6), so
    that the case still holds clearly decided voxels beside the undecided ones."""
    rot = t2.ref_rotation(case)
    Y, peaks, kind = t2.voxels(case, rot)              # (RefRotation asserts that every direction rotates)
    g = t2.gap_and_order(case, rot)
    V = Y.shape[0]
    gap, first = g["gap"], int(np.sum(g["first"]))
    tagged = kind == t2.SAME
    print("%s: %d voxels (%d one fascicle, %d identical directions); gap min %.2e median %.2e max %.2e; < 1e-9: %d, < 1e-6: %d, "
          "> 1e-4: %d; runner-up first %d; pairs within 1e-9 median %g max %g; min 1 - c^2 %.2e (identical directions %s)"
          % (t2.case_id(case), V, np.sum(kind == t2.ONE), tagged.sum(), gap.min(), np.median(gap), gap.max(), np.sum(gap <= 1e-9),
             np.sum(gap < 1e-6), np.sum(gap > 1e-4), first, np.median(g["within"]), g["within"].max(), g["mincc"][~tagged].min(),
             " ".join("%.1e" % x for x in g["mincc"][tagged])))
    assert g["mincc"][~tagged].min() >= 1e-6
    if case[3] == "margin":
        assert np.sum(gap < 1e-6) >= _ceil_div(V, 3)
        if case[2] < 64:
            assert np.sum(gap > 1e-4) >= 1
        else:
            assert gap.max() > 1e-6
    else:
        assert gap.max() <= 1e-9
    assert _ceil_div(V, 4) <= first <= (3 * V) // 4, first


@pytest.mark.parametrize("case", t2.FLOOD_CASES, ids=t2.case_id)
def test_flood_cases_overflow_the_list(case):
    """A slot of mfx_fit2d_k2_kernel is row i with the columns j' = j (mod 16) of one wave's 64-column half of a block.
    In every two-fascicle voxel every slot holds a pair with two positive weights, 1 - c^2 > 1e-6 and a float64
    objective within 0.5e-9 |y|^2 of the minimum: the slot's best pair is listed under any rounding (the window is
    1e-9 |y|^2), at least 16 N > 512 slots."""
    rot = t2.ref_rotation(case)
    Y, peaks, kind = t2.voxels(case, rot)
    N = rot.N
    slot_of_col = (np.arange(N) // 64) * 16 + np.arange(N) % 16
    nslots = np.unique(slot_of_col).size
    assert N * nslots >= 16 * N > 512
    worst = 0.0
    for v in np.flatnonzero(kind == t2.TWO):
        obj, both, cc = t2.pairs(case, rot, v)
        ysq = float(Y[v] @ Y[v])
        good = both & (cc > 1e-6)
        rel = np.where(good, (obj - obj.min()) / ysq, np.inf)
        per_slot = np.array([rel[:, slot_of_col == s].min(axis=1) for s in range(nslots)])
        worst = max(worst, float(per_slot.max()))
        assert per_slot.max() <= 0.5e-9, (v, per_slot.max())
    print("%s: %d slots of up to %d pairs; the worst slot's best pair lies %.2e |y|^2 above the minimum"
          % (t2.case_id(case), N * nslots, _ceil_div(N, 16), worst))


def test_the_8x8_window_case_stays_on_the_list():
    """At most 256 pairs within 2e-9 |y|^2 of the minimum in every voxel: the list (512), not the overflow pass."""
    case = ("syn2", 8, 8, "window")
    rot = t2.ref_rotation(case)
    Y, peaks, kind = t2.voxels(case, rot)
    n = np.array([np.count_nonzero(t2.pairs(case, rot, v)[0] - t2.pairs(case, rot, v)[0].min() <= 2e-9 * float(Y[v] @ Y[v]))
                  for v in range(Y.shape[0])])
    print("8x8 window: pairs within 2e-9 |y|^2 per voxel: %s" % n.tolist())
    assert n.max() <= 256 and n[kind == t2.TWO].min() >= 64


@pytest.mark.parametrize("case", t2.CASES, ids=t2.case_id)
def test_csf_population_has_power(case):
    """The same voxels with a fifth of the CSF signal mixed in, fitted with a CSF column: 1 - c^2 >= 1e-6 between any two
    sub-dictionaries' columns (the CSF column included) outside the identical-direction voxels; window ladder: every family
    gap <= 1e-9 |y|^2; margin ladder: a third of the voxels with a gap < 1e-6 |y|^2.  The relative determinant of the
    oracle's triple (two atoms + CSF) is printed: it is what the explicit solver's score error scales with."""
    rot = t2.ref_rotation(case)
    Y, peaks, kind = t2.csf_voxels(case, rot)
    g = t2.gap_and_order(case, rot, csf=True)
    rows = t2.oracle_rows(case, rot, 2, True)
    tagged = kind == t2.SAME
    gap, V = g["gap"], Y.shape[0]
    print("%s + CSF: gap min %.2e median %.2e max %.2e; < 1e-6: %d; runner-up first %d of %d; min 1 - c^2 %.2e; oracle CSF fraction "
          "%.2f .. %.2f" % (t2.case_id(case), gap.min(), np.median(gap), gap.max(), np.sum(gap < 1e-6), int(np.sum(g["first"])), V,
                            g["mincc"][~tagged].min(), rows[:, 5].min(), rows[:, 5].max()))
    assert g["mincc"][~tagged].min() >= 1e-6
    if case[3] == "window":
        assert gap.max() <= 1e-9
    else:
        assert np.sum(gap < 1e-6) >= _ceil_div(V, 3)


@pytest.mark.parametrize("case", t2.EXPANSION_CASES, ids=t2.case_id)
def test_expansion_voxels_reach_the_family_expansions(case):
    """The noise-free voxels: the oracle's smaller weight is positive and at most 1e-7 of the other one - the second
    weight in even voxels (row expansion), the first in odd ones (column expansion)."""
    from test_fit2d_gpu import oracle_row
    rot = t2.ref_rotation(case)
    Y, peaks = t2.expansion_voxels(case, rot)
    ref = np.array([oracle_row(rot, Y[v], peaks[v].reshape(2, 3), False, None, 2, False) for v in range(Y.shape[0])])
    even = np.arange(Y.shape[0]) % 2 == 0
    ratio = np.where(even, ref[:, 2] / ref[:, 1], ref[:, 1] / ref[:, 2])
    print("%s: smaller weight over the other: %s" % (t2.case_id(case), " ".join("%.1e" % r for r in ratio)))
    assert np.all(ratio > 0) and np.all(ratio <= 1e-7)


@pytest.mark.parametrize("unit", t2.UNITS, ids=[u[0] for u in t2.UNITS])
def test_units_stay_inside_the_equivariant_region(unit):
    """q = log2(cy) + 5 log2(c), counted from these signals' size, stays >= -16.6; at the power-of-two pairs
    the oracle's rows on the referee's rotation of the rescaled dictionary are its baseline rows rescaled, bit for bit
    (two fascicles, two fascicles + CSF, one fascicle)."""
    name, c, cy, pow2 = unit
    q = t2.Q_SIGNALS + np.log2(cy) + 5.0 * np.log2(c)
    print("%s: q = %.1f" % (name, q))
    assert q >= -16.6
    if not pow2:
        return
    for case in t2.UNIT_CASES:
        base, rot = t2.ref_rotation(case), t2.ref_rotation(case, c)
        for K, csf in ((2, False), (2, True), (1, False)):
            ref = t2.oracle_rows(case, base, K, csf)
            got = t2.to_baseline(t2.oracle_rows(case, rot, K, csf, c=c, cy=cy, base=base), c, cy)
            assert np.array_equal(got, ref), (t2.case_id(case), K, csf)
