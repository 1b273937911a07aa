"""Robust fits of 2-D protocols (include/mfx_robust2d.h), the parts that need no GPU: the C ABI, the entry points without a
device, the argument checks of engine.fit2d_robust and RotateAtom2DTables.fit(robust=...), which come before the tables are
asked for their device handle, and robust=None / False taking the path that was there."""
import os
import re

import numpy as np
import pytest

from test_fit2d_gpu import DIFF, Z, atoms
from test_predict2d_host import OTHER_VERSIONS, NoDeviceTables, other_versions
from microstructure_fingerprinting_amd import _lib, engine
from microstructure_fingerprinting_amd import mf_utils as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")


def _declared(header):
    src = open(os.path.join(ROOT, "include", header)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(mfx_[a-z_0-9]+)\s*\(", src)))


def test_robust2d_abi_symbols():
    lib = _lib.lib()
    assert sorted(_lib.ROBUST2D_EXPORTS) == _declared("mfx_robust2d.h")
    older = (_lib.EXPORTS + _lib.ROT2D_EXPORTS + _lib.FIT2D_EXPORTS + _lib.W2D_EXPORTS + _lib.ROBUST_EXPORTS + _lib.PREDICT2D_EXPORTS)
    for name in _lib.ROBUST2D_EXPORTS:
        assert hasattr(lib, name) and name not in older
    assert lib.mfx_robust2d_abi_version() == 1 and lib.mfx_predict2d_abi_version() == 1
    assert other_versions(lib) == OTHER_VERSIONS
    assert sorted(_lib.ROBUST_EXPORTS) == _declared("mfx_robust.h") and sorted(_lib.W2D_EXPORTS) == _declared("mfx_w2d.h")
    for f in (engine.fit2d_robust, engine.fit2d_robust_dev):
        assert callable(f)
    assert lib.mfx_robust2d_debug_last_plan_directions() >= 0


def test_entry_points_without_device():
    lib = _lib.lib()
    M = 16
    Y, pk = np.ones((1, M)), np.array([[0.0, 0.0, 1.0]])
    K = np.ones(1, dtype=np.int32)
    prm, W, sc = np.zeros((1, 5)), np.zeros((1, M)), np.zeros(1)
    ds, ws, stt, used = (np.zeros((1, 5), dtype=np.int32), np.zeros(1, dtype=np.int32), np.zeros(1, dtype=np.int32),
                         np.zeros(1, dtype=np.int32))
    nch = np.zeros(2, dtype=np.int64)

    def host(maxfasc=1, c=4.45):
        return lib.mfx_rfit2d_batch(None, _lib.dptr(Y), None, 0, _lib.iptr(K), None, _lib.dptr(pk), maxfasc, 0, None, 0, c, 2, 1,
                                    _lib.dptr(prm), _lib.dptr(W), _lib.dptr(sc), _lib.iptr(stt), _lib.iptr(ds), _lib.iptr(ws),
                                    _lib.lptr(nch), _lib.iptr(used))
    calls = [host, lambda: host(maxfasc=4), lambda: host(c=0.5),
             lambda: lib.mfx_rfit2d_batch_dev(None, None, None, 0, None, 1, 0, 4.45, 1, 1, None, None, None, None, None, None, None, None)]
    for c in calls:
        if lib.mfx_device_count() > 0:             # with a device the null pointers are what is wrong
            assert c() in (_lib.MFX_ERR_ARG, _lib.MFX_ERR_UNSUPPORTED)
            continue
        assert c() == _lib.MFX_ERR_NO_DEVICE
        assert "no CPU path" in lib.mfx_last_error().decode()


def test_engine_argument_checks_come_before_the_device():
    M = 20
    t = NoDeviceTables(M, 6)
    Y = np.ones((3, M))
    pk = np.tile([0.0, 0.0, 1.0, 0.0, 0.6, 0.8], (3, 1))
    K = np.array([1, 2, 0])
    sc = np.ones(M)
    ok = (Y, K, None, pk, 2, False)
    for args, kw, exc, msg in [(ok, dict(c=0.99), ValueError, "c should be a finite number >= 1"),
                               (ok, dict(c=np.nan), ValueError, "c should be a finite number >= 1"),
                               (ok, dict(loss="l2"), ValueError, "loss should be one of 'cutoff', 'huber', 'tukey'"),
                               (ok, dict(n_iter=-1), ValueError, "n_iter should be a non-negative integer"),
                               (ok, dict(n_iter=1.5), ValueError, "n_iter should be a non-negative integer"),
                               ((Y[:, :-1], K, None, pk, 2, False), {}, ValueError, "measurements"),
                               (ok, dict(W0=np.ones((3, M - 1))), ValueError, r"weights should have shape .*\(3 voxels\)"),
                               (ok, dict(W0=np.ones((2, M))), ValueError, "weights should have shape"),
                               (ok, dict(W0=np.ones(M + 1)), ValueError, "weights should have shape"),
                               ((Y, K, None, pk[:, :3], 2, False), {}, ValueError, "peaks should have shape"),
                               ((Y, K[:2], None, pk, 2, False), {}, ValueError, "K should have one entry"),
                               ((Y, np.array([1, 2, 3]), None, pk, 2, False), {}, ValueError, "K should lie in"),
                               ((Y, K, np.array([1, 0, 0]), pk, 2, False, sc), {}, ValueError, "need csf_on"),
                               ((Y, K, np.array([1, 0, 0]), pk, 2, True), {}, ValueError, "need csf_on and sig_csf"),
                               ((Y, K, np.array([1, 0]), pk, 2, True, sc), {}, ValueError, "csf should have one entry"),
                               ((Y, K, None, pk, 2, True), {}, ValueError, "csf_on needs sig_csf"),
                               ((Y, K, None, np.tile(pk, (1, 2)), 4, False), {}, NotImplementedError, "0 to 3 fascicles")]:
        with pytest.raises(exc, match=msg):
            engine.fit2d_robust(t, *args, **kw)


@pytest.fixture()
def T(monkeypatch):
    sch = np.load(os.path.join(G, "rot2d_cases.npz"))["syn2_sch"]
    t = U.RotateAtom2DTables(atoms(sch, 6, 3), sch, Z, DIFF)

    def no_handle(self):
        raise AssertionError("the device was touched before the arguments were checked")
    monkeypatch.setattr(U.RotateAtom2DTables, "handle", no_handle)
    return t


def test_tables_robust_checks_come_before_the_device(T):
    V, M = 3, T.M
    data = np.ones((V, M))
    pk = np.tile([0.0, 0.0, 1.0, 0.0, 0.6, 0.8], (V, 1))
    K = np.array([1, 2, 0])
    for r, msg in [({"c": 0.5}, "c should be a finite number >= 1"), ({"loss": "lorentz"}, "loss should be one of"),
                   ({"n_iter": -1}, "n_iter should be a non-negative integer"), (3, "robust should be None, a bool or a dict"),
                   ("yes", "robust should be None, a bool or a dict"), ({"cc": 3}, "unknown key.*'cc'")]:
        with pytest.raises(ValueError, match=msg):
            T.fit(data, pk, K, robust=r)
    for kw, msg in [(dict(weights=np.zeros(M)), "without a positive weight"), (dict(weights=-np.ones((V, M))), "negative or non-finite"),
                    (dict(weights=np.ones((V, M + 1))), "weights not compatible"), (dict(on_error="skip"), "on_error should be")]:
        with pytest.raises(ValueError, match=msg):
            T.fit(data, pk, K, robust=True, **kw)
    with pytest.raises(ValueError, match="data has shape"):
        T.fit(data[:, :-1], pk, K, robust=True)
    with pytest.raises(ValueError, match="numfasc should lie in"):
        T.fit(data, pk, np.array([1, 2, 3]), robust={"n_iter": 1})
    with pytest.raises(TypeError):
        T.fit(data, pk, K, None, None, "raise", None, True)            # keyword only
    with pytest.raises(AssertionError, match="the device was touched"):   # a valid request gets as far as the handle
        T.fit(data, pk, K, robust=True)
    r = U.Fit2DResult(np.zeros((V, 7)), np.zeros((V, 5)), 2, False)
    assert r.robust_info is None and r.robust_scale is None and r.n_rejected is None
    with pytest.raises(RuntimeError, match="not a robust fit"):
        r.outlier_mask()


@pytest.mark.parametrize("robust", [None, False])
def test_robust_off_is_the_existing_path(monkeypatch, T, robust):
    """robust=None / False never reach engine.fit2d_robust: the plain fit goes to engine.fit2d, the weighted one to
    engine.fit2d_weighted, with the arguments they get without the keyword."""
    V, M = 3, T.M
    data = np.ones((V, M))
    pk = np.tile([0.0, 0.0, 1.0, 0.0, 0.6, 0.8], (V, 1))
    K = np.array([1, 2, 0])
    seen = []

    class Reached(Exception):
        pass

    def sentinel(*a, **k):
        raise AssertionError("engine.fit2d_robust was reached with robust=%r" % (robust,))

    def plain(tables, Y, *a, **k):
        seen.append(("fit2d", len(a), sorted(k)))
        raise Reached

    def weighted(tables, Y, W, *a, **k):
        seen.append(("fit2d_weighted", W.shape, len(a), sorted(k)))
        raise Reached
    monkeypatch.setattr(engine, "fit2d_robust", sentinel)
    monkeypatch.setattr(engine, "fit2d", plain)
    monkeypatch.setattr(engine, "fit2d_weighted", weighted)
    with pytest.raises(Reached):
        T.fit(data, pk, K, robust=robust)
    with pytest.raises(Reached):
        T.fit(data, pk, K, weights=np.ones(M), robust=robust)
    with pytest.raises(Reached):
        U.RotateAtom2DTables.fit(T, data, pk, K)                      # without the keyword: the same calls
    with pytest.raises(Reached):
        U.RotateAtom2DTables.fit(T, data, pk, K, weights=np.ones(M))
    assert seen[:2] == seen[2:] == [("fit2d", 6, []), ("fit2d_weighted", (M,), 6, [])]
