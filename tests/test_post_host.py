"""Soft fits, host side: the C ABI of include/mfx_post.h, the argument errors raised before any device call,
mf_utils.posterior_moments / posterior_quantile / posterior_by_property on hand-computed values, and the referee of
tests/_post_ref.py restated in float64 against its long-double form.  No GPU needed."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _post_ref as R
from microstructure_fingerprinting_amd import _lib, engine
from microstructure_fingerprinting_amd import mf_utils as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")


def _declared(header):
    src = open(os.path.join(ROOT, "include", header)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(mfx_[a-z_0-9]+)\s*\(", src)))


def test_header_binding_and_library_are_in_step():
    lib = _lib.lib()
    decl = _declared("mfx_post.h")
    assert decl == sorted(_lib.POST_EXPORTS)
    for name in decl:
        assert hasattr(lib, name), "libmfx.so lacks %s declared in include/mfx_post.h" % name
    assert lib.mfx_post_abi_version() == 2
    # the other headers, their binding lists and versions are as they were
    assert _declared("mfx.h") == sorted(_lib.EXPORTS) and lib.mfx_abi_version() == 3
    assert _declared("mfx_profile.h") == sorted(_lib.PROFILE_EXPORTS) and lib.mfx_profile_abi_version() == 2
    for other in (_lib.EXPORTS, _lib.PREDICT_EXPORTS, _lib.MCF_EXPORTS, _lib.ROT2D_EXPORTS, _lib.PROFILE_EXPORTS,
                  _lib.FIT2D_EXPORTS, _lib.WFIT_EXPORTS):
        assert not set(_lib.POST_EXPORTS) & set(other)
    assert lib.mfx_post_max_atoms(None, 0) == 0


def test_header_states_the_definitions():
    src = open(os.path.join(ROOT, "include", "mfx_post.h")).read()
    for word in ("mfx_profile_cut", "log_sum", "shift", "NaN", "MFX_ERR_UNSUPPORTED", "fixed order", "above 700", "560"):
        assert word.lower() in src.lower(), word


def test_without_a_device_the_entry_points_say_so():
    lib = _lib.lib()
    if lib.mfx_device_count() > 0:
        pytest.skip("a GPU is present")
    fake = C.c_void_p(8)   # never dereferenced: the device check comes first
    assert lib.mfx_post_dev(fake, fake, fake, 2, 0, None, fake, fake, 1, fake, fake, fake, None) == _lib.MFX_ERR_NO_DEVICE
    assert b"no HIP device" in lib.mfx_last_error()
    one = np.ones(1)
    st = np.zeros(1, dtype=np.int32)
    assert lib.mfx_post(fake, _lib.dptr(one), _lib.dptr(one), 2, 0, None, _lib.dptr(one), _lib.dptr(one), 1, _lib.dptr(one),
                        _lib.dptr(one), _lib.iptr(st)) == _lib.MFX_ERR_NO_DEVICE
    assert b"no HIP device" in lib.mfx_last_error()


class _Tables:
    N = 14
    device = 0


class _Plan:
    """Stands for an engine.Plan of M rows; the argument checks must be done before its handle is asked for."""
    M = 64
    tables = _Tables()

    def handle(self):
        raise AssertionError("the device plan was touched before the arguments were checked")


def test_engine_posterior_argument_errors():
    import torch
    P = _Plan()
    V = 5
    Y, pk, K = np.zeros((V, 64)), np.zeros((V, 6)), np.full(V, 2)
    with pytest.raises(ValueError, match="protocol has 64"):
        engine.posterior(P, np.zeros((V, 63)), K, None, pk, 2, False, None, 1.0)
    with pytest.raises(ValueError, match="one entry per voxel"):
        engine.posterior(P, Y, np.full(V + 1, 2), None, pk, 2, False, None, 1.0)
    with pytest.raises(ValueError, match="peaks should have 6 columns"):
        engine.posterior(P, Y, K, None, np.zeros((V, 3)), 2, False, None, 1.0)
    with pytest.raises(ValueError, match="csf_on and sig_csf"):
        engine.posterior(P, Y, K, np.ones(V, bool), pk, 2, False, None, 1.0)
    with pytest.raises(ValueError, match="csf_on and sig_csf"):
        engine.posterior(P, Y, K, np.ones(V, bool), pk, 2, True, None, 1.0)
    with pytest.raises(ValueError, match="sig_csf has 60"):
        engine.posterior(P, Y, K, np.ones(V, bool), pk, 2, True, np.ones(60), 1.0)
    with pytest.raises(ValueError, match="exceeds maxfasc"):
        engine.posterior(P, Y, np.full(V, 3), None, pk, 2, False, None, 1.0)
    with pytest.raises(ValueError, match="sigma should be a scalar or have one entry per voxel"):
        engine.posterior(P, Y, K, None, pk, 2, False, None, np.ones(V + 1))
    with pytest.raises(ValueError, match="shift should be a scalar or have one entry per voxel"):
        engine.posterior(P, Y, K, None, pk, 2, False, None, 1.0, shift=np.ones((V, 2)))
    # a set with nothing in scope needs no device: all rows NaN, all counted, status -1
    w, ls, st, n = engine.posterior(P, np.zeros((3, 64)), np.array([0, 2, 3]), None, np.zeros((3, 9)), 3, False, None, 1.0,
                                    ear=np.array([False, True, False]))
    assert n == 3 and w.shape == (3, 3, 14) and np.isnan(w).all() and np.isnan(ls).all() and (st == -1).all()
    # the device entry point: shapes, K and the CSF column before the tensors' residence and the plan
    tY, tpk, tT = torch.zeros((V, 64), dtype=torch.float64), torch.zeros((V, 6), dtype=torch.float64), torch.ones(V, dtype=torch.float64)
    with pytest.raises(NotImplementedError, match="K = 1 or 2"):
        engine.posterior_dev(P, tY, torch.zeros((V, 9), dtype=torch.float64), 3, tT, tT)
    with pytest.raises(NotImplementedError, match="K = 1 or 2"):
        engine.posterior_dev(P, tY, torch.zeros((V, 0), dtype=torch.float64), 0, tT, tT)
    with pytest.raises(ValueError, match="protocol has 64"):
        engine.posterior_dev(P, tY[:, :60], tpk, 2, tT, tT)
    with pytest.raises(ValueError, match=r"peaks should have shape \(5, 3\)"):
        engine.posterior_dev(P, tY, tpk, 1, tT, tT)
    with pytest.raises(ValueError, match="csf_on without d_sig_csf"):
        engine.posterior_dev(P, tY, tpk, 2, tT, tT, csf_on=True)
    with pytest.raises(ValueError, match="sig_csf has 60"):
        engine.posterior_dev(P, tY, tpk, 2, tT, tT, csf_on=True, d_sig_csf=torch.ones(60, dtype=torch.float64))
    with pytest.raises(ValueError, match="T should be a tensor with one entry per voxel"):
        engine.posterior_dev(P, tY, tpk, 2, tT[:4], tT)
    with pytest.raises(ValueError, match="shift should be a tensor with one entry per voxel"):
        engine.posterior_dev(P, tY, tpk, 2, tT, 0.0)


def test_posterior_moments_hand_made():
    vals = np.array([2.0, 1.0, 2.0, 4.0])
    w = np.array([[0.25, 0.25, 0.25, 0.25],
                  [0.0, 1.0, 0.0, 0.0],
                  [np.nan] * 4,
                  [0.5, 0.0, 0.0, 0.5]])
    mean, std = U.posterior_moments(w, vals)
    # row 0: mean 9/4, E v^2 = 25/4, var = 25/4 - 81/16 = 19/16; row 3: mean 3, var 1
    assert np.allclose(mean[[0, 1, 3]], [2.25, 1.0, 3.0], rtol=1e-15) and np.isnan(mean[2])
    assert np.allclose(std[[0, 1, 3]], [np.sqrt(19.0) / 4, 0.0, 1.0], rtol=1e-15) and np.isnan(std[2])
    m3, s3 = U.posterior_moments(w.reshape(4, 1, 4), vals)      # leading axes are kept
    assert m3.shape == (4, 1) and np.array_equal(m3[:, 0], mean, equal_nan=True) and np.array_equal(s3[:, 0], std, equal_nan=True)
    with pytest.raises(ValueError, match="atoms"):
        U.posterior_moments(w, vals[:3])
    import torch
    mt, st = U.posterior_moments(torch.from_numpy(w), vals)
    assert torch.is_tensor(mt) and np.array_equal(mt.numpy(), mean, equal_nan=True) and np.allclose(st.numpy(), std, rtol=1e-15, equal_nan=True)
    for name in ("posterior_moments", "posterior_quantile", "posterior_by_property"):
        assert name in U.__all__


def test_posterior_quantile_hand_made():
    vals = np.array([3.0, 1.0, 2.0, 1.0, 5.0])     # sorted: 1 (atoms 1, 3), 2, 3, 5
    w = np.array([[0.25, 0.125, 0.25, 0.125, 0.25],   # cumulative over the sorted atoms: .125 .25 .5 .75 1
                  [0.0, 0.0, 0.0, 0.0, 1.0],
                  [np.nan] * 5])
    for q, want in ((0.0, 1.0), (0.2, 1.0), (0.25, 1.0), (0.3, 2.0), (0.5, 2.0), (0.51, 3.0), (0.75, 3.0), (0.9, 5.0), (1.0, 5.0)):
        got = U.posterior_quantile(w, vals, q)
        # q = 0: every value's cumulative weight reaches 0, the smallest value it is
        assert got[0] == want and got[1] == (1.0 if q == 0.0 else 5.0) and np.isnan(got[2]), (q, got)
    assert U.posterior_quantile(w.reshape(3, 1, 5), vals, 0.5).shape == (3, 1)
    with pytest.raises(ValueError, match=r"\[0, 1\]"):
        U.posterior_quantile(w, vals, 1.5)
    import torch
    gt = U.posterior_quantile(torch.from_numpy(w), vals, 0.51)
    assert torch.is_tensor(gt) and np.array_equal(gt.numpy(), [3.0, 5.0, np.nan], equal_nan=True)


def test_posterior_by_property_hand_made():
    vals = np.array([2.0, 1.0, 2.0, 3.0, 1.0])
    w = np.array([[0.125, 0.25, 0.125, 0.25, 0.25],
                  [0.0, 0.0, 1.0, 0.0, 0.0],
                  [np.nan] * 5])
    lv, by = U.posterior_by_property(w, vals)
    assert np.array_equal(lv, [1.0, 2.0, 3.0])
    assert np.array_equal(by[:2], [[0.5, 0.25, 0.25], [0.0, 1.0, 0.0]]) and np.isnan(by[2]).all()
    lv3, by3 = U.posterior_by_property(w.reshape(3, 1, 5), vals)
    assert by3.shape == (3, 1, 3) and np.array_equal(by3[:, 0], by, equal_nan=True)
    with pytest.raises(ValueError, match="atoms"):
        U.posterior_by_property(w, vals[:4])
    import torch
    lt, bt = U.posterior_by_property(torch.from_numpy(w), vals)
    assert torch.is_tensor(bt) and np.array_equal(bt.numpy(), by, equal_nan=True) and np.array_equal(lt.numpy(), lv)
    # the mean through the levels is the mean over the atoms
    assert np.allclose((by[:2] * lv).sum(-1), U.posterior_moments(w[:2], vals)[0], rtol=1e-15)


@pytest.mark.parametrize("csf", [False, True])
def test_float64_restatement_of_the_referee_stays_within_the_bar(csf):
    """The referee in float64 NumPy against its long-double form on fit_c2_small at sigma = M0 / 30: the bar has to
    hold for plain float64 arithmetic of the same formulas with a wide margin, or it is no bar for the kernel."""
    d = np.load(os.path.join(G, "fit_c2_small.npz"))
    Y, peaks = np.ascontiguousarray(d["Y"]), np.ascontiguousarray(d["peaks"])
    cut, worst = 1e-8, 0.0
    for v in range(Y.shape[0]):
        T = 2.0 * (float(d["map_M0"][v]) / 30.0) ** 2
        ref = R.voxel("c2", Y[v], peaks[v], csf, T, cut)
        f64 = R.voxel("c2", Y[v], peaks[v], csf, T, cut, dt=np.float64)
        assert ref["clear"], "a pair near the cut: this input was chosen to have none"
        ratio = R.worst_ratio(f64["w"], f64["log_sum"], ref)
        worst = max(worst, ratio)
        print("csf=%d voxel %d: float64 against long double: %.3g of the bar; bars on weights %.3g .. %.3g, on log_sum %.3g; "
              "%.0f effective pairs, smallest 1 - c^2 = %.3g" % (csf, v, ratio, float(ref["bar_w"][0].min()),
                                                                  float(max(ref["bar_w"][0].max(), ref["bar_w"][1].max())),
                                                                  float(ref["bar_log_sum"]), ref["neff"], ref["c2min"]))
        for k in range(2):
            assert abs(float(ref["w"][k].sum()) - 1.0) < 1e-15
    print("csf=%d: worst float64 / long double error = %.3g of the bar" % (csf, worst))
    assert worst <= 1.0
