"""The fits of 2-D (AxCaliber-like) protocols on dictionaries of near-twin atoms and in other units
(tests/_twin2d_cases.py; tests/test_twin2d_host.py guards the populations' power on the CPU alone).

mfx_fit2d_k2_kernel<WGT> ranks pairs on an MFMA-summed cross-Gram and protects a slot's arg-min with a 4 M eps interval and
the 1e-9 |y|^2 window; a lower bound runs across its 128 x 128 blocks; up to 512 listed slots are decided in the
reference's arithmetic, near-collinear pairs are handed over unranked, a vanishing weight expands the winner's row or
column, and an overflowing list sends every pair through the exact stage.  On the margin ladder a runner-up within the
interval is scanned first in about half of the voxels; on the window ladder whole families lie inside the window: 8 x 8
fills the list, 1 x 64 and 1 x 48 overflow it in every two-fascicle voxel, 72 x 2 carries the bound across blocks.

The referee is always the oracle's solve_exhaustive_posweights on the columns the library's own T.rotate returns (the
rotation is refereed elsewhere; the kernels must see its output bit for bit): test_fit2d_gpu.oracle_row, and
_w2d_ref.ref_row on sqrt(W)-scaled columns for weighted fits.  EVERY voxel of every case is compared, every status must
be 0, atom indices must be equal in every voxel (all classes have K + csf <= 3, where the reference's order is defined),
and the other columns are held to the existing bars, test_fit2d_gpu.assert_rows and _wfit_ref.assert_rows."""
import numpy as np
import pytest

import _twin2d_cases as t2
import _w2d_ref as W2
import _wfit_ref as WR
import test_fit2d_gpu as F2
from microstructure_fingerprinting_amd import _lib, engine
from microstructure_fingerprinting_amd import mf_utils as U

pytestmark = pytest.mark.gpu

ALL = t2.CASES + [t2.FIX_CASE]
WINDOW = [c for c in t2.CASES if c[3] == "window"]
WKINDS = ("smooth", "mask")
CLASSES = {"k2": (2, False), "k1": (1, False), "k2csf": (2, True)}
K3_VOXELS = 8
_rot, _rows = {}, {}


def rotation(case, c=1.0):
    """the library's rotation of a case's dictionary in units of c, every rotated dictionary kept (rot.rot: the tables)"""
    key = (case, c)
    if key not in _rot:
        T = U.RotateAtom2DTables(t2.dictionary(case)[0] * c, t2.scheme(case[0]), F2.Z, F2.DIFF)
        _rot[key] = t2.Rotation(T, "lib%g" % c)
    return _rot[key]


def sig_csf(case, c=1.0):
    return F2.csf_signal(t2.scheme(case[0])) * c


def class_voxels(case, K, csf):
    """(Y, peaks [V, 3 K]) of a case as voxels of K fascicles (+ CSF): built on the library's rotation in units of 1"""
    base = rotation(case)
    Y, peaks, _ = t2.csf_voxels(case, base) if csf else t2.voxels(case, base, max(K, 2))
    if K == 3:
        Y, peaks = Y[:K3_VOXELS], peaks[:K3_VOXELS]
    return Y, np.ascontiguousarray(peaks[:, :3 * K])


def fit(case, K, csf, c=1.0, cy=1.0, wkind=None):
    """engine.fit2d / fit2d_weighted (wkind: the weights of _twin2d_cases.weights) on the case's voxels at units (c, cy),
    computed once; every status 0"""
    key = (case, K, csf, c, cy, wkind)
    if key in _rows:
        return _rows[key]
    T = rotation(case, c).rot
    Y, pk = class_voxels(case, K, csf)
    V = Y.shape[0]
    args = (np.full(V, K), np.full(V, True) if csf else None, pk, K, csf, sig_csf(case, c) if csf else None)
    if wkind is None:
        got, st = engine.fit2d(T, Y * cy, *args)
    else:
        got, st, wst = engine.fit2d_weighted(T, Y * cy, t2.weights(case, wkind, *Y.shape), *args)
        assert np.all(wst == 0)
    assert np.all(st == 0) and got.shape[0] == V
    _rows[key] = got
    return got


def fused(case, K):
    """rows of the fused kernels (paths 1 and 2)"""
    return fit(case, K, False)


def reference(case, K, csf, c=1.0, cy=1.0, wkind=None):
    W = t2.weights(case, wkind, *class_voxels(case, K, csf)[0].shape) if wkind else None
    return t2.oracle_rows(case, rotation(case, c), K, csf, W=W, wkind=wkind, c=c, cy=cy, base=rotation(case),
                          nmax=K3_VOXELS if K == 3 else None)


# ---- 1, 2. the fused kernels
@pytest.mark.parametrize("case", ALL, ids=t2.case_id)
def test_k2_fused(case):
    T = rotation(case).rot
    assert T.N <= _lib.lib().mfx_fit2d_max_atoms(T.handle(), 2)
    F2.assert_rows(fused(case, 2), reference(case, 2, False), 2, t2.case_id(case))


@pytest.mark.parametrize("case", t2.CASES, ids=t2.case_id)
def test_k1_first_twin_wins(case):
    """mfx_fit2d_k1_kernel: twins of one atom tie to rounding, and the first index in the reference's order must win"""
    F2.assert_rows(fused(case, 1), reference(case, 1, False), 1, t2.case_id(case))


# ---- 3. the materialise-and-solve route on the same voxels
@pytest.mark.parametrize("case", ALL, ids=t2.case_id)
def test_explicit_equals_oracle_and_fused(case):
    lib = _lib.lib()
    for K in (2, 1):
        try:
            lib.mfx_fit2d_debug_set_force_explicit(1)
            _rows.pop((case, K, False, 1.0, 1.0, None), None)
            explicit = fit(case, K, False)
        finally:
            _rows.pop((case, K, False, 1.0, 1.0, None), None)
            lib.mfx_fit2d_debug_set_force_explicit(0)
        F2.assert_rows(explicit, reference(case, K, False), K, "%s explicit K = %d" % (t2.case_id(case), K))
        got = fused(case, K)
        bad = np.flatnonzero(np.any(got != explicit, axis=1))
        assert bad.size == 0, "%s K = %d: fused and explicit rows differ in voxels %s: %s vs %s" % (t2.case_id(case), K, bad[:4],
                                                                                                    got[bad[:4]], explicit[bad[:4]])


# ---- 4. a CSF column, three fascicles, a mixed batch
@pytest.mark.parametrize("case", t2.CASES, ids=t2.case_id)
def test_k2_csf(case):
    F2.assert_rows(fit(case, 2, True), reference(case, 2, True), 2, t2.case_id(case))


@pytest.mark.parametrize("case", t2.K3_CASES, ids=t2.case_id)
def test_k3(case):
    F2.assert_rows(fit(case, 3, False), reference(case, 3, False), 3, t2.case_id(case))


@pytest.mark.parametrize("case", t2.K3_CASES, ids=t2.case_id)
def test_mixed_batch(case):
    """K = 0 / 1 / 2 / 3 with a CSF mask (never beside three fascicles) through RotateAtom2DTables.fit: 28 voxels, four of
    each class with fascicles and CSF"""
    rot = rotation(case)
    Y, peaks, _ = t2.voxels(case, rot, 3, nv=28)
    V = Y.shape[0]
    K = np.arange(V) % 4
    csf = ((np.arange(V) // 4) % 2 == 0) & (K < 3)
    sc = sig_csf(case)
    Y = np.where(csf[:, None], 0.8 * Y + 0.2 * sc, Y)
    r = rot.rot.fit(Y, peaks, K, csf_mask=csf, sig_csf=sc)
    assert np.all(r.status == 0) and r.params.shape == (V, 10)
    ref = np.array([F2.oracle_row(rot, Y[v], peaks[v, :3 * K[v]].reshape(K[v], 3), bool(csf[v]), sc, 3, True) for v in range(V)])
    F2.assert_rows(r.params, ref, 3, t2.case_id(case))
    assert np.all(r.params[(K == 0) & ~csf] == 0)


# ---- the family expansions: noise-free voxels whose second (first) weight lies in (0, 1e-7] of the other
@pytest.mark.parametrize("case", t2.EXPANSION_CASES, ids=t2.case_id)
def test_family_expansion(case):
    rot = rotation(case)
    T = rot.rot
    Y, peaks = t2.expansion_voxels(case, rot)
    V = Y.shape[0]
    ref = np.array([F2.oracle_row(rot, Y[v], peaks[v].reshape(2, 3), False, None, 2, False) for v in range(V)])
    ratio = np.where(np.arange(V) % 2 == 0, ref[:, 2] / ref[:, 1], ref[:, 1] / ref[:, 2])
    # the range in which the kernel expands.  tests/test_twin2d_host.py guards it in every voxel on the referee's rotation; on
    # the library's, whose last bits differ, a twin of the planted atom may take a voxel with a weight of exactly 0
    inside = (ratio > 0) & (ratio <= 1e-7)
    print("%s: %d of %d voxels with the smaller weight in (0, 1e-7] of the other" % (t2.case_id(case), inside.sum(), V))
    assert inside.sum() >= V - 2 and np.all(ratio <= 1e-7), ratio
    got, st = engine.fit2d(T, Y, np.full(V, 2), None, peaks, 2, False)
    assert np.all(st == 0)
    F2.assert_rows(got, ref, 2, t2.case_id(case) + " expansion")
    W = t2.weights(case, "smooth", V, T.M)
    wgot, st, wst = engine.fit2d_weighted(T, Y, W, np.full(V, 2), None, peaks, 2, False)
    assert np.all(st == 0) and np.all(wst == 0)
    wref = np.array([W2.ref_row(rot.rotate(peaks[v].reshape(2, 3)), Y[v], W[v], False, None, 2, False) for v in range(V)])
    WR.assert_rows(wgot, wref, 2, t2.case_id(case) + " expansion, weighted")


# ---- 5. measurement weights
@pytest.mark.parametrize("wkind", WKINDS)
@pytest.mark.parametrize("cls", sorted(CLASSES))
@pytest.mark.parametrize("case", t2.CASES, ids=t2.case_id)
def test_weighted(case, cls, wkind):
    K, csf = CLASSES[cls]
    got = fit(case, K, csf, wkind=wkind)
    WR.assert_rows(got, reference(case, K, csf, wkind=wkind), K, "%s %s %s" % (t2.case_id(case), cls, wkind))


@pytest.mark.parametrize("case", WINDOW, ids=t2.case_id)
def test_unit_weights_bit_for_bit(case):
    for K in (2, 1):
        assert np.array_equal(fit(case, K, False, wkind="ones"), fused(case, K)), "K = %d" % K


# ---- 6. the device-resident forms
def test_dev_forms_equal_host_forms():
    import torch
    case = ("syn2", 8, 8, "window")
    T = rotation(case).rot
    Y, pk = class_voxels(case, 2, False)
    W = t2.weights(case, "smooth", *Y.shape)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()   # noqa: E731
    out, st = engine.fit2d_dev(T, t(Y), t(pk), 2)
    wout, wst, wwst = engine.fit2d_weighted_dev(T, t(Y), t(W), t(pk), 2)
    torch.cuda.synchronize()
    assert not st.cpu().numpy().any() and not wst.cpu().numpy().any() and not wwst.cpu().numpy().any()
    assert np.array_equal(out.cpu().numpy(), fused(case, 2))
    assert np.array_equal(wout.cpu().numpy(), fit(case, 2, False, wkind="smooth"))


# ---- 7. other units
PATHS = [(cls, None) for cls in sorted(CLASSES)] + [("k3", None)] + [(cls, w) for cls in sorted(CLASSES) for w in WKINDS]


@pytest.mark.parametrize("unit", t2.UNITS, ids=[u[0] for u in t2.UNITS])
@pytest.mark.parametrize("path", PATHS, ids=lambda p: p[0] + ("-" + p[1] if p[1] else ""))
@pytest.mark.parametrize("case", t2.UNIT_CASES, ids=t2.case_id)
def test_units(case, path, unit):
    """The dictionary and the CSF column in units of c, the signals in units of cy: against the oracle at the same units,
    and at the power-of-two pairs against the path's own baseline rows - indices identical, M0 cy / c, the fractions,
    MSE cy^2 and R2 equal bit for bit (every product and sum of the fit scales by a power of two)."""
    name, c, cy, pow2 = unit
    cls, wkind = path
    K, csf = (3, False) if cls == "k3" else CLASSES[cls]
    what = "%s %s %s at %s" % (t2.case_id(case), cls, wkind or "", name)
    got = t2.to_baseline(fit(case, K, csf, c, cy, wkind), c, cy)
    ref = t2.to_baseline(reference(case, K, csf, c, cy, wkind), c, cy)
    if wkind:
        WR.assert_rows(got, ref, K, what + " against the oracle")
    else:
        F2.assert_rows(got, ref, K, what + " against the oracle")
    if pow2:
        base = fit(case, K, csf, wkind=wkind)
        bad = np.argwhere(got != base)
        assert bad.size == 0, "%s against its own baseline rows: %d entries differ, first %s: %r vs %r" % (
            what, bad.shape[0], bad[0], got[tuple(bad[0])], base[tuple(bad[0])])
