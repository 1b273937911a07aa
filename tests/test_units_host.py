"""Dictionaries and signals stored in other units, without a GPU: the precondition of tests/test_units_gpu.py.

The CPU oracle referees the GPU at the units of tests/_units_cases.py.  Here the oracle itself is pinned to the reference
at other units (tests/golden/units_cases.npz, bit for bit, the tolerance regime's negative weights included), shown to be
exactly equivariant at every unit pair the GPU tests use, and the boundary of that region - where the reference's
absolute Cramer tolerance takes over - is measured and kept at a distance ("Units", records the table)."""
import os

import numpy as np
import pytest

import _units_cases as uc
from oracle import oracle as orc

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def test_oracle_equals_reference_at_other_units():
    """solve_exhaustive_posweights(A c, y cy, sizes) as executed by the reference at eight unit pairs - five in the inert
    region, three in the tolerance regime (q = -50, -70, -100), where some of the reference's rows carry negative weights:
    sub-indices equal, w and min_obj bit for bit for up to three sub-dictionaries (as test_oracle_golden requires at
    S0 ~ 1), to rounding for the class that goes through scipy.optimize.nnls in the reference."""
    d = np.load(os.path.join(G, "units_cases.npz"))
    nneg = 0
    for nm in d["names"]:
        A, Y, sizes = d[nm + "_A"], d[nm + "_Y"], d[nm + "_sizes"]
        for u, (c, cy) in enumerate(d["units"]):
            for i in range(Y.shape[0]):
                w, sub, tot, obj, yrec = orc.solve_exhaustive_posweights(A * c, Y[i] * cy, sizes)
                what = (str(nm), c, cy, i)
                w_ref, obj_ref = d[nm + "_w"][u, i], float(d[nm + "_obj"][u, i])
                nneg += bool(np.any(w_ref < 0))
                assert np.array_equal(sub, d[nm + "_sub"][u, i]), what
                if sizes.size <= 3:
                    assert np.array_equal(w, w_ref), what
                    assert obj == obj_ref, what
                else:
                    assert np.allclose(w, w_ref, rtol=1e-9, atol=1e-12 * np.abs(w_ref).max()), what
                    assert np.isclose(obj, obj_ref, rtol=1e-9, atol=0), what
                yr = d[nm + "_yrec"][u, i]
                assert np.allclose(yrec, yr, rtol=1e-12, atol=1e-13 * np.abs(yr).max()), what
    assert nneg >= 2     # the fixture does hold rows of the tolerance regime


@pytest.mark.parametrize("cls", sorted(uc.CLASSES))
def test_oracle_is_equivariant_at_the_gpu_tests_units(cls):
    """Every class of the GPU tests, their voxels (M = 62, N = 64; three fascicles + CSF: N = 40), every power-of-two unit
    pair of theirs: the oracle's row, brought back to baseline units, is the baseline row bit for bit, and no weight is
    negative at any pair (non-power-of-two pairs included) - the reference's tolerance is inert there."""
    mdl = uc.model(20, 40 if cls == "NNN_1" else 64)
    base = uc.oracle_rows(mdl, cls, 1.0, 1.0)
    wc = uc.weight_columns(cls)
    assert np.all(base[:, wc] >= 0) and np.all(base[:, 0] > 0)
    for name, c, cy, pow2 in uc.UNITS:
        rows = uc.oracle_rows(mdl, cls, c, cy)
        assert np.all(np.isfinite(rows)), name
        assert np.all(rows[:, wc] >= 0), name
        if pow2:
            back = uc.to_baseline(rows, c, cy)
            bad = np.where(np.any(back != base, axis=1))[0]
            assert bad.size == 0, "%s at %s: rows %s differ from the baseline" % (cls, name, bad)


SWEEP_CLASSES = ["N", "N_1", "N_1_E", "NN", "NN_1", "NN_E", "NN_1_E", "NNN"]


def test_tolerance_boundary_is_far_from_the_gpu_tests_units(capsys):
    """The boundary, measured: q = ey + 5 ec downward in steps of 2 on two ladders, one from signal units 2^0 (even q) and
    one from 2^-9 (odd q): dictionary units 2^ec, ec = 0, -2 .. -20, and between two of them the signal unit lowered by
    2^-2 .. 2^-8; per class the largest q at which any row of the oracle departs from the rescaled baseline (a class
    is followed down to its first departure).  Every unit pair of the GPU tests must stay at least 15 binary
    orders above the worst of them.  Measured here (the GPU tests' voxels, M = 62, N = 64): DESIGN.md, "Units"."""
    mdl = uc.model(20, 64)
    pairs = sorted(((ey - dy + 5 * ec, ec, ey - dy) for ec in range(0, -21, -2) for ey in (0, -9) for dy in range(0, 10, 2)),
                   reverse=True)
    boundary = {}
    for cls in SWEEP_CLASSES:
        base = uc.oracle_rows(mdl, cls, 1.0, 1.0)
        for q, ec, ey in pairs:
            c, cy = 2.0 ** ec, 2.0 ** ey
            rows = uc.oracle_rows(mdl, cls, c, cy)
            if np.any(uc.to_baseline(rows, c, cy) != base):
                boundary[cls] = (q, ec, ey, int(np.sum(np.any(rows[:, uc.weight_columns(cls)] < 0, axis=1))))
                break
    with capsys.disabled():
        print("\nclass      first departure (largest q)   (ec, ey)   rows with a negative weight there")
        for cls in SWEEP_CLASSES:
            if cls in boundary:
                print("%-10s q = %4d                      (%d, %d)   %d" % ((cls,) + boundary[cls][:3] + boundary[cls][3:]))
            else:
                print("%-10s none down to q = %d" % (cls, pairs[-1][0]))
    worst = max(v[0] for v in boundary.values())
    lowest = min(uc.q_of(c, cy) for _, c, cy, _ in uc.UNITS)
    print("worst boundary q = %d, lowest q of the GPU tests' units = %.1f" % (worst, lowest))
    assert lowest >= worst + 15
    assert uc.q_of(*uc.TOLERANCE_REGIME[1:3]) < worst    # the pair of the tolerance-regime test lies below the boundary
