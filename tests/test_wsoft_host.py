"""Profiles and soft fits of a weighted fit, host side: the C ABI of include/mfx_wsoft.h, the argument errors raised
before any device call, and Posterior.log_evidence with measurement weights on hand-made arrays.  No GPU needed."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from microstructure_fingerprinting_amd import _lib, engine
from microstructure_fingerprinting_amd import mf as mfmod

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared(header):
    src = open(os.path.join(ROOT, "include", header)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(mfx_[a-z_0-9]+)\s*\(", src)))


def test_header_binding_and_library_are_in_step():
    lib = _lib.lib()
    decl = _declared("mfx_wsoft.h")
    assert decl == sorted(_lib.WSOFT_EXPORTS) and len(decl) == 8
    for name in decl:
        assert hasattr(lib, name), "libmfx.so lacks %s declared in include/mfx_wsoft.h" % name
    assert lib.mfx_wsoft_abi_version() == 1
    # the other headers, their binding lists and versions are as they were
    others = {"mfx.h": (_lib.EXPORTS, "mfx_abi_version", 3), "mfx_profile.h": (_lib.PROFILE_EXPORTS, "mfx_profile_abi_version", 2),
              "mfx_post.h": (_lib.POST_EXPORTS, "mfx_post_abi_version", 2), "mfx_wfit.h": (_lib.WFIT_EXPORTS, "mfx_wfit_abi_version", 1),
              "mfx_predict.h": (_lib.PREDICT_EXPORTS, "mfx_predict_abi_version", 1), "mfx_mcf.h": (_lib.MCF_EXPORTS, "mfx_mcf_abi_version", 1),
              "mfx_rot2d.h": (_lib.ROT2D_EXPORTS, "mfx_rot2d_abi_version", 1), "mfx_fit2d.h": (_lib.FIT2D_EXPORTS, "mfx_fit2d_abi_version", 1)}
    for header, (exports, version, want) in others.items():
        assert _declared(header) == sorted(exports), header
        assert getattr(lib, version)() == want, header
        assert not set(_lib.WSOFT_EXPORTS) & set(exports), header
    assert _lib.POST_EXPORTS == ["mfx_post_abi_version", "mfx_post_max_atoms", "mfx_post_dev", "mfx_post",
                                 "mfx_post_debug_last_config"]
    assert _lib.PROFILE_EXPORTS == ["mfx_profile_abi_version", "mfx_profile_cut", "mfx_profile_max_atoms", "mfx_profile_dev",
                                    "mfx_profile", "mfx_pair_objectives_dev", "mfx_pair_objectives",
                                    "mfx_profile_debug_last_config"]
    for what in (0, 1, 2, 3):
        assert lib.mfx_wsoft_max_atoms(None, 0, what) == 0


def test_header_states_the_definitions():
    src = open(os.path.join(ROOT, "include", "mfx_wsoft.h")).read()
    for word in ("sqrt(W[v,m])", "correctly rounded", "fl(s_m * D_k[m,i])", "fl(s_m * y_m)", "fl(s_m * x_m)", "mfx_profile_cut",
                 "status 3", "status 4", "NaN", "partner -1", "bit for bit", "sigma^2 / W", "MFX_ERR_UNSUPPORTED", "560",
                 "w_stride = 0"):
        assert word.lower() in src.lower(), word


def test_without_a_device_the_entry_points_say_so():
    lib = _lib.lib()
    if lib.mfx_device_count() > 0:
        pytest.skip("a GPU is present")
    fake = C.c_void_p(8)   # never dereferenced: the device check comes first
    one, st = np.ones(1), np.zeros(1, dtype=np.int32)
    d, i = _lib.dptr(one), _lib.iptr(st)
    calls = [lambda: lib.mfx_wpost_dev(fake, fake, fake, 1, fake, 2, 0, None, fake, fake, 1, fake, fake, fake, None),
             lambda: lib.mfx_wpost(fake, d, d, 1, d, 2, 0, None, d, d, 1, d, d, i),
             lambda: lib.mfx_wprofile_dev(fake, fake, fake, 1, fake, 2, 0, None, 1, fake, None, None),
             lambda: lib.mfx_wprofile(fake, d, d, 1, d, 2, 0, None, 1, d, None),
             lambda: lib.mfx_wpair_objectives_dev(fake, fake, fake, 1, fake, 0, None, 1, fake, None),
             lambda: lib.mfx_wpair_objectives(fake, d, d, 1, d, 0, None, 1, d)]
    for call in calls:
        assert call() == _lib.MFX_ERR_NO_DEVICE
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


def test_weights_argument_errors_come_before_any_device_call():
    import torch
    P = _Plan()
    V = 5
    Y, pk, K = np.zeros((V, 64)), np.zeros((V, 6)), np.full(V, 2)
    for bad in (np.ones((V, 63)), np.ones(63), np.ones((V + 1, 64)), np.ones((64, V)), np.ones((1, 64)), np.float64(1.0)):
        with pytest.raises(ValueError, match=r"weights should have shape \(5, 64\) or \(64,\)"):
            engine.posterior(P, Y, K, None, pk, 2, False, None, 1.0, W=bad)
        with pytest.raises(ValueError, match=r"weights should have shape \(5, 64\) or \(64,\)"):
            engine.profile(P, Y, K, None, pk, 2, False, None, W=bad)
        with pytest.raises(ValueError, match=r"weights should have shape \(5, 64\) or \(64,\)"):
            engine.pair_objectives(P, Y, pk, W=bad)
    # the other checks are those of the unweighted calls, with weights given
    with pytest.raises(ValueError, match="protocol has 64"):
        engine.posterior(P, np.zeros((V, 63)), K, None, pk, 2, False, None, 1.0, W=np.ones(64))
    with pytest.raises(ValueError, match="exceeds maxfasc"):
        engine.profile(P, Y, np.full(V, 3), None, pk, 2, False, None, W=np.ones(64))
    with pytest.raises(ValueError, match=r"peaks should have shape \(5, 6\)"):
        engine.pair_objectives(P, Y, np.zeros((V, 9)), W=np.ones(64))
    # three fascicles and EAR-flagged voxels are out of scope with weights as without: NaN rows, counted, and a set with
    # nothing else in it needs no device.  The weights' shape is still checked.
    K3, ear = np.array([0, 2, 3]), np.array([False, True, False])
    w, ls, st, n = engine.posterior(P, np.zeros((3, 64)), K3, None, np.zeros((3, 9)), 3, False, None, 1.0, ear=ear, W=np.ones((3, 64)))
    assert n == 3 and w.shape == (3, 3, 14) and np.isnan(w).all() and np.isnan(ls).all() and (st == -1).all()
    obj, par, n = engine.profile(P, np.zeros((3, 64)), K3, None, np.zeros((3, 9)), 3, False, None, partner=True, ear=ear, W=np.ones(64))
    assert n == 3 and np.isnan(obj).all() and (par == -1).all()
    with pytest.raises(ValueError, match="weights should have shape"):
        engine.profile(P, np.zeros((3, 64)), K3, None, np.zeros((3, 9)), 3, False, None, ear=ear, W=np.ones((2, 64)))
    # the device entry points take one class: K = 3 with weights is refused like K = 3 without, shapes before residence
    tY, tpk, tT = torch.zeros((V, 64), dtype=torch.float64), torch.zeros((V, 6), dtype=torch.float64), torch.ones(V, dtype=torch.float64)
    tW = torch.ones((V, 64), dtype=torch.float64)
    with pytest.raises(NotImplementedError, match="K = 1 or 2"):
        engine.posterior_dev(P, tY, torch.zeros((V, 9), dtype=torch.float64), 3, tT, tT, d_W=tW)
    with pytest.raises(NotImplementedError, match="K = 1 or 2"):
        engine.profile_dev(P, tY, torch.zeros((V, 9), dtype=torch.float64), 3, d_W=tW)
    for call in (lambda w: engine.posterior_dev(P, tY, tpk, 2, tT, tT, d_W=w), lambda w: engine.profile_dev(P, tY, tpk, 2, d_W=w),
                 lambda w: engine.pair_objectives_dev(P, tY, tpk, d_W=w)):
        with pytest.raises(ValueError, match=r"weights should have shape \(5, 64\) or \(64,\)"):
            call(tW[:, :60])
        with pytest.raises(ValueError, match=r"weights should have shape \(5, 64\) or \(64,\)"):
            call(tW[:4])


def test_log_evidence_with_measurement_weights():
    """log_sum - K log N - (n_pos / 2) log(pi T) + (1 / 2) sum_{W > 0} log W_m on hand-made arrays; W = 1 gives the
    unweighted value exactly."""
    N, M = 8, 6
    w = np.full((3, 2, N), 1.0 / N)
    ls = np.array([-3.5, 2.25, np.nan])
    st = np.array([0, 0, 3], dtype=np.int32)
    K = np.array([2, 1, 2])
    T = np.array([2.0, 0.5, 1.0])
    plain = mfmod.Posterior(w, ls, st, 0, np.arange(3), {}, K, T, M).log_evidence()
    want = ls - K * np.log(N) - 0.5 * M * np.log(np.pi * T)
    assert np.array_equal(plain[:2], want[:2]) and np.isnan(plain[2])
    ones = mfmod.Posterior(w, ls, st, 0, np.arange(3), {}, K, T, M, W=np.ones((3, M))).log_evidence()
    assert np.array_equal(ones, plain, equal_nan=True)
    ones1 = mfmod.Posterior(w, ls, st, 0, np.arange(3), {}, K, T, M, W=np.ones(M)).log_evidence()
    assert np.array_equal(ones1, plain, equal_nan=True)
    W = np.array([[4.0, 0.0, 0.25, 1.0, 2.0, 0.0],
                  [1.0, 1.0, 0.0, 8.0, 0.5, 1.0],
                  [1.0, 1.0, 1.0, 1.0, 1.0, 1.0]])
    got = mfmod.Posterior(w, ls, st, 0, np.arange(3), {}, K, T, M, W=W).log_evidence()
    # voxel 0: 4 positive weights, log(4 * 0.25 * 1 * 2) = log 2; voxel 1: 5 positive, log(8 * 0.5) = log 4
    hand = np.array([-3.5 - 2 * np.log(8.0) - 2.0 * np.log(np.pi * 2.0) + 0.5 * np.log(2.0),
                     2.25 - np.log(8.0) - 2.5 * np.log(np.pi * 0.5) + 0.5 * np.log(4.0)])
    assert np.allclose(got[:2], hand, rtol=1e-15, atol=0) and np.isnan(got[2])
    shared = mfmod.Posterior(w, ls, st, 0, np.arange(3), {}, K, T, M, W=W[0]).log_evidence()
    assert np.allclose(shared[:2], ls[:2] - K[:2] * np.log(N) - 2.0 * np.log(np.pi * T[:2]) + 0.5 * np.log(2.0), rtol=1e-15)
    # a Gaussian check of the formula: one measurement of weight W and residual r has density sqrt(W / (pi T)) exp(-W r^2 / T)
    r, Wm, Tm = 0.3, 2.5, 0.7
    dens = np.sqrt(Wm / (np.pi * Tm)) * np.exp(-Wm * r * r / Tm)
    one = mfmod.Posterior(np.ones((1, 1, 1)), np.array([-Wm * r * r / Tm]), np.zeros(1, dtype=np.int32), 0, np.arange(1), {},
                          np.array([1]), np.array([Tm]), 1, W=np.array([[Wm]])).log_evidence()
    assert abs(one[0] - np.log(dens)) <= 4 * np.finfo(float).eps * abs(np.log(dens))
    assert "3" in mfmod.Posterior.__doc__ and "4" in mfmod.Posterior.__doc__ and "not finite" in mfmod.Posterior.__doc__
