"""Bootstrap of 2-D protocols conditional on measurement weights (include/mfx_wboot2d.h), the parts that need no GPU: the
C ABI, every argument check of the new entry points (each must fire before any device call) and the public interface's
rules for ``weights=`` and ``fixed_weights=``."""
import os
import re

import numpy as np
import pytest

import _wboot2d_cases as C
from microstructure_fingerprinting_amd import _lib, engine
from microstructure_fingerprinting_amd import mf_utils as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Z = np.array([0.0, 0.0, 1.0])


class NoDeviceTables:
    """Stands for a RotateAtom2DTables in the argument checks: asking it for its handle is a device call."""
    def __init__(self, M, N):
        self.M, self.N = M, N

    def handle(self):
        raise AssertionError("the device was touched before the arguments were checked")


def _header(name):
    return open(os.path.join(ROOT, "include", name)).read()


def _declared():
    src = re.sub(r"/\*.*?\*/", "", _header("mfx_wboot2d.h"), flags=re.S)
    return sorted(set(re.findall(r"\b(mfx_[a-z_0-9]+)\s*\(", src)))


def test_wboot2d_abi_symbols():
    lib = _lib.lib()
    assert sorted(_lib.WBOOT2D_EXPORTS) == _declared()
    assert sorted(_lib.WBOOT2D_EXPORTS) == sorted(["mfx_wboot2d_abi_version", "mfx_wboot2d_rep_tile", "mfx_wboot2d_max_atoms",
                                                    "mfx_wboot2d_debug_set_force_plain", "mfx_wboot2d_fit_rows_dev",
                                                    "mfx_wboot2d_fit_dev", "mfx_wboot2d_fit"])
    for name in _lib.WBOOT2D_EXPORTS:
        assert hasattr(lib, name)
        assert name not in _lib.EXPORTS and name not in _lib.BOOT2D_EXPORTS and name not in _lib.WBOOT_EXPORTS and name not in _lib.W2D_EXPORTS
    assert lib.mfx_wboot2d_abi_version() == 1
    # the headers it stands on keep their versions: only their "Not served" sentences changed
    assert lib.mfx_boot2d_abi_version() == 1 and lib.mfx_wboot_abi_version() == 1 and lib.mfx_w2d_abi_version() == 1
    assert lib.mfx_boot_abi_version() == 1
    assert lib.mfx_wboot2d_rep_tile() == lib.mfx_boot2d_rep_tile() >= 2
    assert lib.mfx_wboot2d_max_atoms(None) == 0
    for f in ("fit2d_weighted_replicates_dev", "fit2d_weighted_bootstrap_dev", "fit2d_weighted_bootstrap"):
        assert callable(getattr(engine, f))
    for h in ("mfx_boot2d.h", "mfx_wboot.h"):
        src = _header(h)
        assert "mfx_wboot2d.h" in src
        left_out = src.split("Not served:")[1].split("*/")[0]
        assert "weights" not in left_out and "robust fits" not in left_out
    own = _header("mfx_wboot2d.h")
    assert "held fixed" in own and "conditional on the rows that were rejected" in " ".join(own.split()).replace("* ", "")


def test_entry_points_without_device():
    lib = _lib.lib()
    M = 16
    Y, W, pk = np.ones((1, M)), np.ones((1, M)), np.array([[0.0, 0.0, 1.0]])
    K = np.ones(1, dtype=np.int32)
    st, ag, ds = np.zeros(1, dtype=np.int32), np.zeros(1, dtype=np.int32), np.zeros(5, dtype=np.int32)
    stats = np.zeros((1, 3, 5))
    calls = [lambda: lib.mfx_wboot2d_fit_rows_dev(None, None, None, M, None, 1, -1, 4, None, None, None, None),
             lambda: lib.mfx_wboot2d_fit_dev(None, None, None, M, None, 1, 0, None, None, None, None, None, 1, 4, 0, 1, 0, 0, None, 0, None,
                                             0, 0, None, None, None, None, None, None),
             lambda: lib.mfx_wboot2d_fit(None, _lib.dptr(Y), _lib.dptr(W), M, _lib.iptr(K), None, _lib.dptr(pk), 1, 0, None, None, None,
                                         None, 1, 4, 0, 1, 0, 0, None, 0, None, 0, 0, _lib.dptr(stats), _lib.iptr(ag), _lib.iptr(st),
                                         _lib.iptr(ds), None)]
    for c in calls:
        if lib.mfx_device_count() > 0:             # with a device the null handle is what is wrong
            assert c() == _lib.MFX_ERR_ARG
            continue
        assert c() == _lib.MFX_ERR_NO_DEVICE
        assert "no CPU path" in lib.mfx_last_error().decode()


def test_engine_argument_checks_come_before_the_device():
    M, N = 20, 8
    T = NoDeviceTables(M, N)
    Y = np.ones((3, M))
    W = np.ones((3, M))
    pk = np.tile([0.0, 0.0, 1.0, 0.0, 0.6, 0.8], (3, 1))
    K = np.array([1, 2, 0])
    sc = np.ones(M)
    base = (Y, W, K, None, pk, 2, False)
    for args, kw, exc, msg in [
            (base, dict(B=0), ValueError, "B should be an integer >= 1"),
            (base, dict(B=2.5), ValueError, "B should be an integer"),
            (base, dict(B=True), ValueError, "B should be an integer"),
            (base, dict(kind='pairs'), ValueError, "kind should be one of"),
            (base, dict(q=(0.5, 1.5)), ValueError, r"q should lie in \[0, 1\]"),
            (base, dict(q='median'), ValueError, "q should be numbers"),
            (base, dict(seed=1.5), ValueError, "seed should be an integer"),
            (base, dict(offset=0.5), ValueError, "offset should be an integer"),
            (base, dict(B=4097), NotImplementedError, "at most 4096"),
            (base, dict(q=np.linspace(0, 1, 33)), NotImplementedError, "at most 32 bootstrap quantiles"),
            ((Y[:, :-1],) + base[1:], {}, ValueError, "protocol has 20 measurements"),
            ((Y, W[:2]) + base[2:], {}, ValueError, r"weights should have shape \(3, 20\) or \(20,\)"),
            ((Y, W[0, :-1]) + base[2:], {}, ValueError, r"weights should have shape \(3, 20\) or \(20,\)"),
            ((Y, W, K[:2]) + base[3:], {}, ValueError, "K should have one entry"),
            ((Y, W, np.array([1, 2, 3])) + base[3:], {}, ValueError, "K should lie in"),
            ((Y, W, K, np.array([1, 0, 0]), pk, 2, False), {}, ValueError, "flagged CSF need csf_on"),
            ((Y, W, K, np.array([1, 0]), pk, 2, True, sc), {}, ValueError, "csf should have one entry"),
            ((Y, W, K, None, pk[:, :3], 2, False), {}, ValueError, "peaks should have shape"),
            ((Y, W, K, None, pk, 2, True), {}, ValueError, "csf_on needs sig_csf"),
            ((Y, W, K, None, pk, 2, True, sc[:-1]), {}, ValueError, "sig_csf has 19 entries"),
            ((Y, W, K, None, np.tile(pk, (1, 2)), 4, False), {}, NotImplementedError, "0 to 3 fascicles"),
            (base, dict(params=np.zeros((3, 6))), ValueError, r"params should have shape \(3, 7\)"),
            (base, dict(vox=np.arange(2)), ValueError, "vox should have one entry"),
            (base, dict(props=np.zeros((2, N + 1))), ValueError, r"props should have shape \(nprop, 8\)"),
            (base, dict(kind='residual'), ValueError, "needs groups"),
            (base, dict(kind='residual', groups=np.zeros(M - 1, dtype=int)), ValueError, "groups should be 20 integers"),
            (base, dict(kind='residual', groups=np.zeros(M)), ValueError, "groups should be 20 integers")]:
        with pytest.raises(exc, match=msg):
            engine.fit2d_weighted_bootstrap(T, *args, **kw)
    # a shared [M] vector passes the shape check: the call gets as far as the handle
    with pytest.raises(AssertionError, match="the device was touched"):
        engine.fit2d_weighted_bootstrap(T, Y, W[0], K, None, pk, 2, False, B=4)


def _tables():
    rot = np.load(os.path.join(ROOT, "tests", "golden", "rot2d_cases.npz"))
    sch = rot["syn2_sch"]
    rng = np.random.default_rng(3)
    b = (2 * np.pi * 42.577480e6 * sch[:, 3] * sch[:, 5]) ** 2 * (sch[:, 4] - sch[:, 5] / 3)
    sig = np.exp(-np.outer(b, rng.uniform(0.3e-9, 2.5e-9, 6)))
    return U.RotateAtom2DTables(sig, sch, Z, 2.2e-9), sch


def test_tables_bootstrap_rules_for_weights_come_before_the_device():
    T, sch = _tables()
    M, V = T.M, 3
    Y = np.ones((V, M))
    pk = np.tile([0.0, 0.0, 1.0, 0.0, 0.6, 0.8], (V, 1))
    K = np.array([1, 2, 0])
    Wv = C.weights("smooth", V, M, 1)
    plain = U.Fit2DResult(np.zeros((V, 7)), np.zeros((V, 5)), 2, False)
    weighted = U.Fit2DResult(np.zeros((V, 7)), np.zeros((V, 5)), 2, False, weights=Wv)
    shared = U.Fit2DResult(np.zeros((V, 7)), np.zeros((V, 5)), 2, False, weights=np.ones(M))
    robust = U.Fit2DResult(np.zeros((V, 7)), np.zeros((V, 5)), 2, False, weights=np.ones((V, M)))
    robust._set_robust({'scale': np.ones(V)}, None)
    for kw, exc, msg in [
            (dict(fixed_weights=1), ValueError, "fixed_weights should be True or False, got 1"),
            (dict(fixed_weights='yes'), ValueError, "fixed_weights should be True or False"),
            (dict(fixed_weights=None), ValueError, "fixed_weights should be True or False"),
            (dict(weights=Wv), ValueError, "fixed_weights"),
            (dict(weights=Wv, fit=weighted), ValueError, "fixed_weights"),
            (dict(fixed_weights=True), ValueError, "fixed_weights=True needs a fit made with weights= or robust=: "),
            (dict(fixed_weights=True, fit=plain), ValueError, "fixed_weights=True needs a fit made with weights= or robust=: this fit"),
            (dict(fixed_weights=True, fit=weighted, weights=2.0 * Wv), ValueError, r"weights differ from those of fit \(3 voxels\)"),
            (dict(fixed_weights=True, fit=plain, weights=Wv), ValueError, r"weights differ from those of fit \(3 voxels\)"),
            (dict(fixed_weights=True, fit=shared, weights=Wv), ValueError, r"weights differ from those of fit \(3 voxels\)"),
            (dict(fixed_weights=True, weights=Wv[:, :-1]), ValueError, "weights not compatible with the data of 3 voxel"),
            (dict(fixed_weights=True, weights=-Wv), ValueError, "negative or non-finite weights"),
            (dict(fixed_weights=True, weights=np.zeros(M)), ValueError, "without a positive weight"),
            (dict(fixed_weights=True, weights=Wv, B=4097), NotImplementedError, "at most 4096"),
            (dict(fixed_weights=True, weights=Wv, q=np.linspace(0, 1, 33)), NotImplementedError, "at most 32 bootstrap quantiles"),
            (dict(fixed_weights=True, weights=Wv, kind='block'), ValueError, "kind should be one of"),
            (dict(fixed_weights=True, weights=Wv, voxels=[3]), ValueError, "positions in the batch"),
            (dict(fixed_weights=True, fit=U.Fit2DResult(np.zeros((V + 1, 7)), np.zeros((V + 1, 5)), 2, False, weights=np.ones(M))),
             ValueError, "the same 3 voxels")]:
        with pytest.raises(exc, match=msg):
            T.bootstrap(Y, pk, K, **kw)
    # the default is what it was: a weighted or robust fit is refused
    for fit in (weighted, shared, robust):
        for kw in ({}, dict(fixed_weights=False)):
            with pytest.raises(NotImplementedError, match="bootstrap of a weighted or robust fit is not served"):
                T.bootstrap(Y, pk, K, fit=fit, B=4, **kw)
    assert T._h is None                                 # nothing was created on a device
    if _lib.lib().mfx_device_count() == 0:              # valid arguments get as far as the device, and no further
        for kw in (dict(fit=weighted), dict(fit=robust), dict(weights=Wv), dict(weights=np.ones(M)), dict(fit=weighted, weights=Wv),
                   dict(fit=shared, weights=np.ones((V, M)))):
            with pytest.raises(_lib.MfxError, match="no CPU path"):
                T.bootstrap(Y, pk, K, B=4, kind='residual', fixed_weights=True, **kw)
    doc = " ".join(U.RotateAtom2DTables.bootstrap.__doc__.split())
    assert "fixed_weights=True" in doc and "include/mfx_wboot2d.h" in doc
    assert "conditional on the rows that were rejected" in doc.lower() and "No replicate re-runs the rejection" in doc
    assert "conditional on the rows that were rejected" in " ".join(U.Bootstrap2DResult.__doc__.split())


def test_result_keeps_the_weights():
    V, B, F = 2, 4, 2
    cols = engine.boot_columns(F, False, False, 0)
    res = {'stats': np.zeros((V, len(cols), 5)), 'columns': cols, 'replicates': None, 'status': np.zeros(V, dtype=np.int32),
           'dir_status': np.zeros((V, 5), dtype=np.int32), 'agree': np.zeros((V, F), dtype=np.int32)}
    assert U.Bootstrap2DResult(res, [], (), np.arange(V), F, False, B, 0).weights is None
    W = np.ones((V, 7))
    assert U.Bootstrap2DResult(res, [], (), np.arange(V), F, False, B, 0, weights=W).weights is W


def test_weight_cases_keep_a_degree_of_freedom():
    for M in (66, 1776):
        for kind in C.KINDS:
            W = C.rows_of(C.weights(kind, 6, M, 11), 6)
            assert np.all(np.isfinite(W)) and np.all(W >= 0) and W.max() <= 4.0
            assert np.all(np.count_nonzero(W > 0, axis=1) > 3)
        m = C.weights("mask", 6, M, 11)
        assert set(np.unique(m)) == {0.0, 1.0} and not m[:, C.MC - 2:C.MC + 2].any()
