"""The forward model of 2-D protocols (include/mfx_predict2d.h), the parts that need no GPU: the C ABI, the entry points
without a device, and the argument checks of engine.predict2d and RotateAtom2DTables.predict / residuals / simulate, which
all come before the tables are asked for their device handle."""
import os
import re

import numpy as np
import pytest

from test_fit2d_gpu import DIFF, Z, atoms
from microstructure_fingerprinting_amd import _lib, engine
from microstructure_fingerprinting_amd import mf_utils as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")


def _declared(header):
    src = open(os.path.join(ROOT, "include", header)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(mfx_[a-z_0-9]+)\s*\(", src)))


def other_versions(lib):
    """the version calls of every header that was there before"""
    return {n: getattr(lib, n)() for n in ("mfx_abi_version", "mfx_mcf_abi_version", "mfx_rot2d_abi_version", "mfx_fit2d_abi_version",
                                           "mfx_wfit_abi_version", "mfx_predict_abi_version", "mfx_profile_abi_version",
                                           "mfx_post_abi_version", "mfx_wsoft_abi_version", "mfx_soft2d_abi_version",
                                           "mfx_w2d_abi_version", "mfx_robust_abi_version")}


OTHER_VERSIONS = {"mfx_abi_version": 3, "mfx_mcf_abi_version": 1, "mfx_rot2d_abi_version": 1, "mfx_fit2d_abi_version": 1,
                  "mfx_wfit_abi_version": 1, "mfx_predict_abi_version": 1, "mfx_profile_abi_version": 2, "mfx_post_abi_version": 2,
                  "mfx_wsoft_abi_version": 1, "mfx_soft2d_abi_version": 1, "mfx_w2d_abi_version": 1, "mfx_robust_abi_version": 1}


def test_predict2d_abi_symbols():
    lib = _lib.lib()
    assert sorted(_lib.PREDICT2D_EXPORTS) == _declared("mfx_predict2d.h")
    older = (_lib.EXPORTS + _lib.ROT2D_EXPORTS + _lib.FIT2D_EXPORTS + _lib.PREDICT_EXPORTS + _lib.W2D_EXPORTS + _lib.ROBUST_EXPORTS)
    for name in _lib.PREDICT2D_EXPORTS:
        assert hasattr(lib, name) and name not in older
    assert lib.mfx_predict2d_abi_version() == 1
    assert other_versions(lib) == OTHER_VERSIONS
    # the symbol lists of the older headers are what they were
    assert sorted(_lib.PREDICT_EXPORTS) == _declared("mfx_predict.h") and sorted(_lib.FIT2D_EXPORTS) == _declared("mfx_fit2d.h")
    assert sorted(_lib.W2D_EXPORTS) == _declared("mfx_w2d.h") and sorted(_lib.ROT2D_EXPORTS) == _declared("mfx_rot2d.h")
    for f in (engine.predict2d, engine.predict2d_dev, U.RotateAtom2DTables.predict, U.RotateAtom2DTables.residuals,
              U.RotateAtom2DTables.simulate):
        assert callable(f)


def test_entry_points_without_device():
    lib = _lib.lib()
    M = 16
    prm, pk, out = np.zeros((1, 5)), np.array([[0.0, 0.0, 1.0]]), np.zeros((1, M))
    ds = np.zeros((1, 5), dtype=np.int32)

    def host(maxfasc=1):
        return lib.mfx_predict2d(None, _lib.dptr(prm), _lib.dptr(pk), maxfasc, 0, None, 1, None, None, 0, 0, 0, 0, _lib.dptr(out), None,
                                 _lib.iptr(ds))
    calls = [host, lambda: host(maxfasc=4),
             lambda: lib.mfx_predict2d_dev(None, None, None, 1, 0, None, 1, None, None, 0, 0, 0, 0, None, None, None, None, None)]
    for c in calls:
        if lib.mfx_device_count() > 0:             # with a device the null handle is what is wrong
            assert c() in (_lib.MFX_ERR_ARG, _lib.MFX_ERR_UNSUPPORTED)
            continue
        assert c() == _lib.MFX_ERR_NO_DEVICE
        assert "no CPU path" in lib.mfx_last_error().decode()


class NoDeviceTables:
    """Stands for a RotateAtom2DTables in engine's argument checks: asking it for its handle is a device call."""
    def __init__(self, M, N):
        self.M, self.N = M, N

    def handle(self):
        raise AssertionError("the device was touched before the arguments were checked")


@pytest.fixture()
def T(monkeypatch):
    sch = np.load(os.path.join(G, "rot2d_cases.npz"))["syn2_sch"]
    t = U.RotateAtom2DTables(atoms(sch, 6, 3), sch, Z, DIFF)

    def no_handle(self):
        raise AssertionError("the device was touched before the arguments were checked")
    monkeypatch.setattr(U.RotateAtom2DTables, "handle", no_handle)
    return t


def test_engine_argument_checks_come_before_the_device():
    M, N = 20, 6
    t = NoDeviceTables(M, N)
    prm = np.zeros((3, 7))
    pk = np.tile([0.0, 0.0, 1.0, 0.0, 0.6, 0.8], (3, 1))
    for args, kw, exc, msg in [((prm[:, :6], pk, 2), {}, ValueError, "params should have 7 columns"),
                               ((prm, pk, 2), dict(csf_on=True, sig_csf=np.ones(M)), ValueError, "params should have 8 columns"),
                               ((prm, pk[:, :3], 2), {}, ValueError, "peaks should have shape"),
                               ((prm, pk[:2], 2), {}, ValueError, "peaks should have shape"),
                               ((np.zeros((3, 11)), np.tile(pk, (1, 2)), 4), {}, NotImplementedError, "0 to 3 fascicles"),
                               ((np.zeros((3, 8)), pk, 2), dict(csf_on=True, sig_csf=np.ones(M - 1)), ValueError, "sig_csf has"),
                               ((prm, pk, 2), dict(Y=np.ones((3, M + 1))), ValueError, "data has shape"),
                               ((prm, pk, 2), dict(ncoils=1), ValueError, "needs sigma_g"),
                               ((prm, pk, 2), dict(ncoils=1, sigma_g=np.ones(2)), ValueError, "sigma_g should be a scalar")]:
        with pytest.raises(exc, match=msg):
            engine.predict2d(t, *args, **kw)


def test_tables_argument_checks_come_before_the_device(T):
    M = T.M
    V = 3
    prm = np.zeros((V, 7)); prm[:, 0] = 1.0; prm[:, 1] = 0.5
    pk = np.tile([0.0, 0.0, 1.0, 0.0, 0.6, 0.8], (V, 1))
    data = np.ones((V, M))
    for call, exc, msg in [
            (lambda: T.predict(prm[0], pk), ValueError, "params should be a 2-D array"),
            (lambda: T.predict(prm, pk[:, :5]), ValueError, "peaks should have shape"),
            (lambda: T.predict(prm, pk[:2]), ValueError, "peaks should have shape"),
            (lambda: T.predict(prm[:, :6], pk), ValueError, "params should have 1 \\+ 2 maxfasc"),
            (lambda: T.predict(np.zeros((V, 8)), pk), ValueError, "sig_csf is needed"),
            (lambda: T.predict(np.zeros((V, 8)), pk, np.ones(M + 2)), ValueError, "sig_csf has"),
            (lambda: T.predict(np.zeros((V, 15)), np.tile(pk, (1, 2))), NotImplementedError, "at most 3 fascicles"),
            (lambda: T.predict(prm, pk, on_error="ignore"), ValueError, "on_error should be"),
            (lambda: T.residuals(data[:, :-1], prm, pk), ValueError, "data has shape"),
            (lambda: T.residuals(data[:2], prm, pk), ValueError, "data has shape"),
            (lambda: T.simulate(prm, pk), ValueError, "exactly one of SNR and sigma_g"),
            (lambda: T.simulate(prm, pk, SNR=20.0, sigma_g=0.1), ValueError, "exactly one of SNR and sigma_g"),
            (lambda: T.simulate(prm, pk, sigma_g=0.1, N=0), ValueError, "N should be a positive integer"),
            (lambda: T.simulate(prm, pk, sigma_g=0.1, N=1.5), ValueError, "N should be a positive integer"),
            (lambda: T.simulate(prm, pk, sigma_g=np.ones((V, M + 1))), ValueError, "sigma_g should be a scalar"),
            (lambda: T.simulate(prm, pk[:, :4], SNR=10.0), ValueError, "peaks should have shape")]:
        with pytest.raises(exc, match=msg):
            call()
    # a valid request gets as far as the handle, and no further
    for call in (lambda: T.predict(prm, pk), lambda: T.residuals(data, prm, pk), lambda: T.simulate(prm, pk, SNR=20.0, seed=1)):
        with pytest.raises(AssertionError, match="the device was touched"):
            call()
