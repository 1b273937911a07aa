"""Bootstrap of 2-D protocols (include/mfx_boot2d.h), the parts that need no GPU: the C ABI, every argument check of the
new entry points (each must fire before any device call) and the result object's name lookup."""
import os
import re

import numpy as np
import pytest

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


def _declared():
    src = open(os.path.join(ROOT, "include", "mfx_boot2d.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(mfx_[a-z_0-9]+)\s*\(", src)))


def test_boot2d_abi_symbols():
    lib = _lib.lib()
    assert sorted(_lib.BOOT2D_EXPORTS) == _declared()
    for name in _lib.BOOT2D_EXPORTS:
        assert hasattr(lib, name)
        assert name not in _lib.EXPORTS and name not in _lib.BOOT_EXPORTS and name not in _lib.FIT2D_EXPORTS
    assert lib.mfx_boot2d_abi_version() == 1
    assert lib.mfx_boot_abi_version() == 1 and lib.mfx_fit2d_abi_version() == 1 and lib.mfx_predict2d_abi_version() == 1
    assert lib.mfx_boot2d_rep_tile() >= 2
    for f in ("fit2d_replicates_dev", "fit2d_bootstrap_dev", "fit2d_bootstrap"):
        assert callable(getattr(engine, f))
    assert "2-D protocols" not in open(os.path.join(ROOT, "include", "mfx_boot.h")).read().split("Not served:")[1].split(".")[0]


def test_entry_points_without_device():
    lib = _lib.lib()
    M = 16
    Y, pk = np.ones((1, M)), np.array([[0.0, 0.0, 1.0]])
    K = np.ones(1, dtype=np.int32)
    st, ag, ds = np.zeros(1, dtype=np.int32), np.zeros(1, dtype=np.int32), np.zeros(5, dtype=np.int32)
    stats = np.zeros((1, 3, 5))
    calls = [lambda: lib.mfx_boot2d_fit_rows_dev(None, None, None, 1, -1, 4, None, None, None),
             lambda: lib.mfx_boot2d_fit_dev(None, None, None, 1, 0, None, None, None, None, None, 1, 4, 0, 1, 0, 0, None, 0, None, 0, 0,
                                            None, None, None, None, None, None),
             lambda: lib.mfx_boot2d_fit(None, _lib.dptr(Y), _lib.iptr(K), None, _lib.dptr(pk), 1, 0, None, None, None, None, 1, 4, 0, 1,
                                        0, 0, None, 0, None, 0, 0, _lib.dptr(stats), _lib.iptr(ag), _lib.iptr(st), _lib.iptr(ds), None)]
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
    pk = np.tile([0.0, 0.0, 1.0, 0.0, 0.6, 0.8], (3, 1))
    K = np.array([1, 2, 0])
    sc = np.ones(M)
    base = (Y, K, None, pk, 2, False)
    for args, kw, exc, msg in [
            (base, dict(B=0), ValueError, "B should be an integer >= 1"),
            (base, dict(B=2.5), ValueError, "B should be an integer"),
            (base, dict(B=True), ValueError, "B should be an integer"),
            (base, dict(kind='pairs'), ValueError, "kind should be one of"),
            (base, dict(q=(0.5, 1.5)), ValueError, r"q should lie in \[0, 1\]"),
            (base, dict(q=(np.nan,)), ValueError, r"q should lie in \[0, 1\]"),
            (base, dict(q='median'), ValueError, "q should be numbers"),
            (base, dict(seed=1.5), ValueError, "seed should be an integer"),
            (base, dict(offset=0.5), ValueError, "offset should be an integer"),
            (base, dict(B=4097), NotImplementedError, "at most 4096"),
            (base, dict(q=np.linspace(0, 1, 33)), NotImplementedError, "at most 32 bootstrap quantiles"),
            ((Y[:, :-1],) + base[1:], {}, ValueError, "protocol has 20 measurements"),
            ((Y, K[:2]) + base[2:], {}, ValueError, "K should have one entry"),
            ((Y, np.array([1, 2, 3])) + base[2:], {}, ValueError, "K should lie in"),
            ((Y, K, np.array([1, 0, 0]), pk, 2, False), {}, ValueError, "flagged CSF need csf_on"),
            ((Y, K, np.array([1, 0]), pk, 2, True, sc), {}, ValueError, "csf should have one entry"),
            ((Y, K, None, pk[:, :3], 2, False), {}, ValueError, "peaks should have shape"),
            ((Y, K, None, pk, 2, True), {}, ValueError, "csf_on needs sig_csf"),
            ((Y, K, None, pk, 2, True, sc[:-1]), {}, ValueError, "sig_csf has 19 entries"),
            ((Y, K, None, np.tile(pk, (1, 2)), 4, False), {}, NotImplementedError, "0 to 3 fascicles"),
            (base, dict(params=np.zeros((3, 6))), ValueError, r"params should have shape \(3, 7\)"),
            (base, dict(vox=np.arange(2)), ValueError, "vox should have one entry"),
            (base, dict(props=np.zeros((2, N + 1))), ValueError, r"props should have shape \(nprop, 8\)"),
            (base, dict(kind='residual'), ValueError, "needs groups"),
            (base, dict(kind='residual', groups=np.zeros(M - 1, dtype=int)), ValueError, "groups should be 20 integers"),
            (base, dict(kind='residual', groups=np.zeros(M)), ValueError, "groups should be 20 integers")]:
        with pytest.raises(exc, match=msg):
            engine.fit2d_bootstrap(T, *args, **kw)
    assert engine.boot_columns(2, True, False, 1) == ['M0', 'nu_0', 'nu_1', 'nu_csf', 'MSE', ('prop', 0, 0), ('prop', 1, 0)]


def _tables():
    rot = np.load(os.path.join(ROOT, "tests", "golden", "rot2d_cases.npz"))
    sch = rot["syn2_sch"]
    rng = np.random.default_rng(3)
    b = (2 * np.pi * 42.577480e6 * sch[:, 3] * sch[:, 5]) ** 2 * (sch[:, 4] - sch[:, 5] / 3)
    sig = np.exp(-np.outer(b, rng.uniform(0.3e-9, 2.5e-9, 6)))
    return U.RotateAtom2DTables(sig, sch, Z, 2.2e-9), sch


def test_tables_bootstrap_checks_come_before_the_device():
    T, sch = _tables()
    M, N, V = T.M, T.N, 3
    Y = np.ones((V, M))
    pk = np.tile([0.0, 0.0, 1.0, 0.0, 0.6, 0.8], (V, 1))
    K = np.array([1, 2, 0])
    for args, kw, exc, msg in [
            ((Y, pk, K), dict(B=0), ValueError, "B should be an integer >= 1"),
            ((Y, pk, K), dict(B=10.0), ValueError, "B should be an integer"),
            ((Y, pk, K), dict(B=4097), NotImplementedError, "at most 4096"),
            ((Y, pk, K), dict(kind='block'), ValueError, "kind should be one of"),
            ((Y, pk, K), dict(q=(0.1, 2.0)), ValueError, "q should lie in"),
            ((Y, pk, K), dict(on_error='ignore'), ValueError, "on_error should be"),
            ((Y[:, :-1], pk, K), {}, ValueError, "protocol has %d measurements" % M),
            ((Y, pk[:2], K), {}, ValueError, "peaks should have shape"),
            ((Y, pk, K[:2]), {}, ValueError, "numfasc should have one entry"),
            ((Y, pk, np.array([1, 2, 3])), {}, ValueError, "numfasc should lie in"),
            ((Y, np.tile(pk, (1, 2)), K), {}, NotImplementedError, "at most 3 fascicles"),
            ((Y, pk, K), dict(csf_mask=np.array([1, 0])), ValueError, "csf_mask should have one entry"),
            ((Y, pk, K), dict(csf_mask=np.array([1, 0, 0])), ValueError, "flagged CSF need sig_csf"),
            ((Y, pk, K), dict(sig_csf=np.ones(M - 1)), ValueError, "sig_csf has %d entries" % (M - 1)),
            ((Y, pk, K), dict(props={'rad': np.ones(N + 1)}), ValueError, "property rad has"),
            ((Y, pk, K), dict(voxels=[3]), ValueError, "positions in the batch"),
            ((Y, pk, K), dict(kind='residual', groups=np.zeros(3, dtype=int)), ValueError, "groups should be %d integers" % M),
            ((Y, pk, K), dict(kind='residual', groups=np.zeros(M)), ValueError, "groups should be %d integers" % M),
            ((Y, pk, K), dict(fit=np.zeros((V, 7))), ValueError, "fit should be the Fit2DResult"),
            ((Y, pk, K), dict(fit=U.Fit2DResult(np.zeros((V + 1, 7)), np.zeros((V + 1, 5)), 2, False)), ValueError, "the same 3 voxels"),
            ((Y, pk, K), dict(fit=U.Fit2DResult(np.zeros((V, 8)), np.zeros((V, 5)), 2, True)), ValueError, "the same 3 voxels")]:
        with pytest.raises(exc, match=msg):
            T.bootstrap(*args, **kw)
    weighted = U.Fit2DResult(np.zeros((V, 7)), np.zeros((V, 5)), 2, False, weights=np.ones(M))
    robust = U.Fit2DResult(np.zeros((V, 7)), np.zeros((V, 5)), 2, False, weights=np.ones((V, M)))
    robust._set_robust({'scale': np.ones(V)}, None)
    for fit in (weighted, robust):
        with pytest.raises(NotImplementedError, match="bootstrap of a weighted or robust fit is not served"):
            T.bootstrap(Y, pk, K, fit=fit, B=4)
    assert T._h is None                                 # nothing was created on a device
    # the default groups of the residual bootstrap: rows sharing (G, Delta, delta)
    g = np.unique(sch[:, 3:6], axis=0, return_inverse=True)[1].reshape(-1)
    if sch.shape[1] == 7:
        assert np.array_equal(g, engine.boot_groups(sch))
    if _lib.lib().mfx_device_count() == 0:              # valid arguments get as far as the device, and no further
        with pytest.raises(_lib.MfxError, match="no CPU path"):
            T.bootstrap(Y, pk, K, B=4, kind='residual')
    assert 'redraws its own' in U.RotateAtom2DTables.bootstrap.__doc__


def test_result_name_lookup():
    V, B, F = 2, 4, 2
    cols = engine.boot_columns(F, True, False, 2)
    rng = np.random.default_rng(1)
    res = {'stats': rng.normal(size=(V, len(cols), 7)), 'columns': cols, 'replicates': None, 'status': np.zeros(V, dtype=np.int32),
           'dir_status': np.zeros((V, 5), dtype=np.int32), 'agree': np.array([[4, 2], [0, 1]], dtype=np.int32)}
    r = U.Bootstrap2DResult(res, ['rad', 'fin'], (0.025, 0.975), np.arange(V), F, True, B, 7)
    s = res['stats']
    assert np.array_equal(r.mean('rad'), s[:, [5, 7], 1]) and np.array_equal(r.std('fin'), s[:, [6, 8], 2])
    assert np.array_equal(r.mean('frac'), s[:, 1:3, 1]) and r.mean('frac').shape == (V, F)
    assert np.array_equal(r.min('M0'), s[:, 0, 3]) and np.array_equal(r.max('MSE'), s[:, 4, 4])
    assert np.array_equal(r.mean('frac_csf'), s[:, 3, 1]) and r.mean('frac_csf').shape == (V,)
    assert np.array_equal(r.quantile('rad', 0.975), s[:, [5, 7], 6]) and np.array_equal(r.quantile('M0', 0.025), s[:, 0, 5])
    assert r.n_valid('rad').dtype == np.int64 and r.n_valid('rad').shape == (V, F)
    assert np.array_equal(r.agreement, [[1.0, 0.5], [0.0, 0.25]])
    assert r.B == B and r.seed == 7 and list(r.q) == [0.025, 0.975] and list(r.voxels) == [0, 1] and r.replicates is None
    with pytest.raises(ValueError, match="quantile 0.5 was not asked for"):
        r.quantile('rad', 0.5)
    with pytest.raises(ValueError, match="unknown bootstrap statistic radius"):
        r.mean('radius')
    with pytest.raises(ValueError, match="unknown bootstrap statistic frac_ear"):
        r.mean('frac_ear')
    r2 = U.Bootstrap2DResult(dict(res, columns=engine.boot_columns(F, False, False, 2), stats=s[:, :8]), ['rad', 'fin'], (), np.arange(V),
                             F, False, B, 0)
    with pytest.raises(ValueError, match="unknown bootstrap statistic frac_csf"):
        r2.mean('frac_csf')
