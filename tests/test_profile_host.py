"""Objective profiles, host side: the C ABI of include/mfx_profile.h, the argument errors raised before any device
call, mf_utils.profile_by_property / profile_interval, and the golden file's own consistency.  No GPU needed."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from microstructure_fingerprinting_amd import _lib, engine
from microstructure_fingerprinting_amd import mf_utils as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")


def _declared(header):
    src = open(os.path.join(ROOT, "include", header)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(mfx_[a-z_0-9]+)\s*\(", src)))


def test_header_declares_the_bound_symbols():
    lib = _lib.lib()
    decl = _declared("mfx_profile.h")
    assert decl == sorted(_lib.PROFILE_EXPORTS)
    for name in decl:
        assert hasattr(lib, name), "libmfx.so lacks %s declared in include/mfx_profile.h" % name
    assert lib.mfx_profile_abi_version() == 2
    assert 0.0 < lib.mfx_profile_cut() <= 1e-6
    # mfx.h, its binding list and its version are as they were
    assert _declared("mfx.h") == sorted(_lib.EXPORTS)
    for other in (_lib.EXPORTS, _lib.PREDICT_EXPORTS, _lib.MCF_EXPORTS, _lib.ROT2D_EXPORTS):
        assert not set(_lib.PROFILE_EXPORTS) & set(other)
    assert lib.mfx_abi_version() == 3


def test_header_states_the_definitions():
    src = open(os.path.join(ROOT, "include", "mfx_profile.h")).read()
    for word in ("lsqnonneg_2var_opt", "mfx_profile_cut", "NaN", "MFX_ERR_UNSUPPORTED", "not clamped", "560"):
        assert word.lower() in src.lower(), word


def test_without_a_device_the_entry_points_say_so():
    lib = _lib.lib()
    if lib.mfx_device_count() > 0:
        pytest.skip("a GPU is present")
    fake = C.c_void_p(8)   # never dereferenced: the device check comes first
    assert lib.mfx_profile_dev(fake, fake, fake, 2, 0, None, 1, fake, None, None) == _lib.MFX_ERR_NO_DEVICE
    assert lib.mfx_pair_objectives_dev(fake, fake, fake, 0, None, 1, fake, None) == _lib.MFX_ERR_NO_DEVICE
    assert b"no HIP device" in lib.mfx_last_error()


class _Tables:
    N = 14


class _Plan:
    """Stands for an engine.Plan of M rows; the argument checks must be done before its handle is asked for."""
    M = 64
    tables = _Tables()

    def handle(self):
        raise AssertionError("the device plan was touched before the arguments were checked")


def test_engine_profile_argument_errors():
    P = _Plan()
    V = 5
    Y, pk, K = np.zeros((V, 64)), np.zeros((V, 6)), np.full(V, 2)
    with pytest.raises(ValueError, match="protocol has 64"):
        engine.profile(P, np.zeros((V, 63)), K, None, pk, 2, False, None)
    with pytest.raises(ValueError, match="one entry per voxel"):
        engine.profile(P, Y, np.full(V + 1, 2), None, pk, 2, False, None)
    with pytest.raises(ValueError, match="peaks should have 6 columns"):
        engine.profile(P, Y, K, None, np.zeros((V, 3)), 2, False, None)
    with pytest.raises(ValueError, match="csf_on and sig_csf"):
        engine.profile(P, Y, K, np.ones(V, bool), pk, 2, False, None)
    with pytest.raises(ValueError, match="sig_csf has 60"):
        engine.profile(P, Y, K, np.ones(V, bool), pk, 2, True, np.ones(60))
    with pytest.raises(ValueError, match="exceeds maxfasc"):
        engine.profile(P, Y, np.full(V, 3), None, pk, 2, False, None)
    with pytest.raises(ValueError, match=r"peaks should have shape \(5, 6\)"):
        engine.pair_objectives(P, Y, np.zeros((V, 3)))
    with pytest.raises(ValueError, match="protocol has 64"):
        engine.pair_objectives(P, np.zeros((V, 10)), pk)
    with pytest.raises(ValueError, match="sig_csf"):
        engine.pair_objectives(P, Y, pk, True, None)


def test_profile_classes_bins_and_counts():
    K = np.array([0, 1, 2, 2, 1, 2, 3, 2])
    csf = np.array([1, 0, 0, 1, 1, 0, 0, 0], bool)
    ear = np.array([0, 0, 0, 0, 0, 1, 0, 0], bool)
    with pytest.raises(ValueError, match="exceeds maxfasc"):
        engine.profile_classes(K, csf, ear, 2)
    bins, n_uns = engine.profile_classes(K, csf, ear, 3)
    assert n_uns == 3    # no fascicle, EAR, three fascicles
    assert [(k, c, list(ix)) for k, c, ix in bins] == [(1, False, [1]), (1, True, [4]), (2, False, [2, 7]), (2, True, [3])]
    # a volume with nothing in scope needs no device: all rows NaN, all counted
    obj, par, n = engine.profile(_Plan(), np.zeros((2, 64)), np.array([0, 2]), None, np.zeros((2, 6)), 2, False, None,
                                 partner=True, ear=np.array([False, True]))
    assert n == 2 and obj.shape == (2, 2, 14) and np.isnan(obj).all() and (par == -1).all()


def test_profile_by_property_hand_made():
    vals = np.array([2.0, 1.0, 2.0, 3.0, 1.0])
    obj = np.array([[5.0, 4.0, 3.0, 9.0, 4.0],
                    [1.0, 1.0, 1.0, 1.0, 1.0],
                    [np.nan] * 5])
    lv, by = U.profile_by_property(obj, vals)
    assert np.array_equal(lv, [1.0, 2.0, 3.0])
    assert np.array_equal(by[:2], [[4.0, 3.0, 9.0], [1.0, 1.0, 1.0]]) and np.isnan(by[2]).all()
    lv3, by3 = U.profile_by_property(obj.reshape(3, 1, 5), vals)      # leading axes are kept
    assert by3.shape == (3, 1, 3) and np.array_equal(by3[:, 0], by, equal_nan=True)
    with pytest.raises(ValueError, match="atoms"):
        U.profile_by_property(obj, vals[:4])
    import torch
    lt, bt = U.profile_by_property(torch.from_numpy(obj), vals)
    assert torch.is_tensor(bt) and np.array_equal(bt.numpy(), by, equal_nan=True) and np.array_equal(lt.numpy(), lv)


def test_profile_interval_hand_made():
    vals = np.array([2.0, 1.0, 2.5, 3.0, 0.5])
    obj = np.array([[10.0, 10.0, 11.0, 10.5, 30.0],      # a tie at the minimum
                    [4.0, 2.0, 3.0, 2.0, 2.1],
                    [np.nan] * 5])
    lo, hi, n = U.profile_interval(obj, vals)
    assert np.array_equal(lo[:2], [1.0, 1.0]) and np.array_equal(hi[:2], [2.0, 3.0]) and np.array_equal(n, [2, 2, 0])
    assert np.isnan(lo[2]) and np.isnan(hi[2])
    lo, hi, n = U.profile_interval(obj, vals, rel=0.05)   # 10.5 and 2.1 come in
    assert np.array_equal(lo[:2], [1.0, 0.5]) and np.array_equal(hi[:2], [3.0, 3.0]) and np.array_equal(n, [3, 3, 0])
    lo, hi, n = U.profile_interval(obj, vals, delta=1.0)  # an absolute margin: 11 and 3 too
    assert np.array_equal(lo[:2], [1.0, 0.5]) and np.array_equal(hi[:2], [3.0, 3.0]) and np.array_equal(n, [4, 4, 0])
    lo, hi, n = U.profile_interval(obj, vals, rel=0.05, delta=0.5)
    assert np.array_equal(n, [4, 3, 0])
    with pytest.raises(ValueError, match="negative"):
        U.profile_interval(obj, vals, rel=-0.1)
    import torch
    tl, th, tn = U.profile_interval(torch.from_numpy(obj), vals, rel=0.05)
    assert np.array_equal(tl.numpy(), [1.0, 0.5, np.nan], equal_nan=True) and np.array_equal(tn.numpy(), [3, 3, 0])
    assert "profile_interval" in U.__all__ and "profile_by_property" in U.__all__


def test_golden_file_is_self_consistent():
    """Row minima of the reference's profiles equal the reference's own fit: map_MSE * M of fit_c2_small within
    4 M eps ||y||^2 (both come from its Gram arithmetic, MSE = SoS / M); the partner of a slot's best atom is the other
    slot's best atom; a single-fascicle profile has no partner."""
    g = np.load(os.path.join(G, "profile_cases.npz"))
    c2 = np.load(os.path.join(G, "fit_c2_small.npz"))
    M = c2["Y"].shape[1]
    obj, par, ysq = g["fit_c2_small_obj"], g["fit_c2_small_partner"], g["fit_c2_small_ysq"]
    assert obj.shape == (6, 2, 48) and np.allclose(ysq, np.sum(c2["Y"] ** 2, axis=1), rtol=1e-14)
    bar = 4 * M * np.finfo(float).eps * ysq
    for k in range(2):
        dev = np.abs(obj[:, k].min(axis=1) - c2["map_MSE"] * M)
        print("slot %d: max |min obj - MSE M| / ||y||^2 = %.3g" % (k, float(np.max(dev / ysq))))
        assert np.all(dev <= bar)
    assert float(g["fit_c2_small_min_vs_mse"]) <= 4 * M * np.finfo(float).eps
    b0, b1 = obj[:, 0].argmin(axis=1), obj[:, 1].argmin(axis=1)
    r = np.arange(6)
    assert np.array_equal(par[r, 0, b0], b1) and np.array_equal(par[r, 1, b1], b0)
    assert np.array_equal(c2["rad"][b0], c2["map_rad_f0"]) and np.array_equal(c2["rad"][b1], c2["map_rad_f1"])
    k1 = np.load(os.path.join(G, "fit_cases_k1.npz"))
    o1 = g["fit_cases_k1_obj"]
    assert o1.shape == (12, 1, 14) and (g["fit_cases_k1_partner"] == -1).all()
    assert np.all(np.abs(o1[:, 0].min(axis=1) - k1["map_MSE"] * 64) <= 4 * 64 * np.finfo(float).eps * g["fit_cases_k1_ysq"])
    fc = np.load(os.path.join(G, "fit_cases.npz"))
    vox = g["fit_cases_vox"]
    assert vox.size > 0 and np.all(fc["csf"][vox] > 0) and np.all(fc["ear"][vox] == 0) and g["fit_cases_csf"].all()
    for r, v in enumerate(vox):
        k = int(g["fit_cases_K"][r])
        assert np.isnan(g["fit_cases_obj"][r, k:]).all() and not np.isnan(g["fit_cases_obj"][r, :k]).any()
