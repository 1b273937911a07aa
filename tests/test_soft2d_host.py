"""Soft fits and objective profiles of 2-D protocols, the parts that need no GPU: the C ABI of include/mfx_soft2d.h,
the argument checks that come before any device call, the result objects, and the float64 restatement of the referee of
tests/_post_ref.py against its long-double form on the reference's pair values (tests/golden/soft2d_cases.npz, written by
gen_golden_soft2d.py)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _post_ref as R
from microstructure_fingerprinting_amd import _lib, engine
from microstructure_fingerprinting_amd import mf as mfmod
from microstructure_fingerprinting_amd import mf_utils as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
Z = np.array([0.0, 0.0, 1.0])
EPS = R.EPS


@pytest.fixture(scope="module")
def rot():
    return np.load(os.path.join(G, "rot2d_cases.npz"))


def _declared(header):
    src = open(os.path.join(ROOT, "include", header)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(mfx_[a-z_0-9]+)\s*\(", src)))


def test_header_binding_and_library_are_in_step():
    lib = _lib.lib()
    decl = _declared("mfx_soft2d.h")
    assert decl == sorted(_lib.SOFT2D_EXPORTS)
    for name in decl:
        assert hasattr(lib, name), "libmfx.so lacks %s declared in include/mfx_soft2d.h" % name
    assert lib.mfx_soft2d_abi_version() == 1
    for other in (_lib.EXPORTS, _lib.MCF_EXPORTS, _lib.ROT2D_EXPORTS, _lib.FIT2D_EXPORTS, _lib.WFIT_EXPORTS, _lib.PREDICT_EXPORTS,
                  _lib.PROFILE_EXPORTS, _lib.POST_EXPORTS, _lib.WSOFT_EXPORTS):
        assert not set(_lib.SOFT2D_EXPORTS) & set(other)
    # the other headers, their binding lists and versions are as they were
    for header, lst, version in (("mfx.h", _lib.EXPORTS, (lib.mfx_abi_version, 3)),
                                 ("mfx_fit2d.h", _lib.FIT2D_EXPORTS, (lib.mfx_fit2d_abi_version, 1)),
                                 ("mfx_post.h", _lib.POST_EXPORTS, (lib.mfx_post_abi_version, 2)),
                                 ("mfx_profile.h", _lib.PROFILE_EXPORTS, (lib.mfx_profile_abi_version, 2)),
                                 ("mfx_rot2d.h", _lib.ROT2D_EXPORTS, (lib.mfx_rot2d_abi_version, 1)),
                                 ("mfx_wsoft.h", _lib.WSOFT_EXPORTS, (lib.mfx_wsoft_abi_version, 1))):
        assert _declared(header) == sorted(lst), header
        assert version[0]() == version[1], header
    assert len(_lib.EXPORTS) == 42 and len(_lib.FIT2D_EXPORTS) == 5 and len(_lib.POST_EXPORTS) == 5 and len(_lib.PROFILE_EXPORTS) == 8


def test_header_states_the_definitions():
    src = open(os.path.join(ROOT, "include", "mfx_soft2d.h")).read()
    for word in ("mfx_profile_cut", "mfx_rot2d_rotate", "bit for bit", "log_sum", "shift", "NaN", "MFX_ERR_UNSUPPORTED",
                 "fixed order", "above 700", "dir_status", "lowest index", "launch nothing"):
        assert word.lower() in src.lower(), word


def test_max_atoms_needs_no_device():
    lib = _lib.lib()
    assert lib.mfx_soft2d_max_atoms(None, 0) == 0
    h = 1                                      # any non-null handle: the limits do not depend on the protocol
    n_post, n_prof = lib.mfx_soft2d_max_atoms(h, 0), lib.mfx_soft2d_max_atoms(h, 1)
    assert n_post >= n_prof >= 1024 and n_post % 16 == 0 and n_prof % 16 == 0      # the largest measured size fits both
    assert lib.mfx_soft2d_max_atoms(h, 2) == 0 and lib.mfx_soft2d_max_atoms(h, -1) == 0


def test_without_a_device_the_entry_points_say_so(rot):
    lib = _lib.lib()
    if lib.mfx_device_count() > 0:
        pytest.skip("a GPU is present")
    fake = C.c_void_p(8)   # never dereferenced: the device check comes first
    one = np.ones(1)
    st, ds = np.zeros(1, dtype=np.int32), np.zeros(5, dtype=np.int32)
    calls = [lambda: lib.mfx_post2d_dev(fake, fake, fake, 2, fake, fake, 1, fake, fake, fake, fake, None),
             lambda: lib.mfx_post2d(fake, _lib.dptr(one), _lib.dptr(one), 2, _lib.dptr(one), _lib.dptr(one), 1, _lib.dptr(one),
                                    _lib.dptr(one), _lib.iptr(st), _lib.iptr(ds)),
             lambda: lib.mfx_profile2d_dev(fake, fake, fake, 2, 1, fake, None, fake, None),
             lambda: lib.mfx_profile2d(fake, _lib.dptr(one), _lib.dptr(one), 1, 1, _lib.dptr(one), None, _lib.iptr(ds))]
    for c in calls:
        assert c() == _lib.MFX_ERR_NO_DEVICE
        assert b"no HIP device" in lib.mfx_last_error()
    T = U.RotateAtom2DTables(rot["syn2_sig"], rot["syn2_sch"], Z, 2.2e-9)
    pk, K = np.array([[0.0, 0.0, 1.0]]), np.ones(1, dtype=np.int32)
    with pytest.raises(_lib.MfxError, match="no CPU path"):
        T.posterior(np.ones((1, T.M)), pk, K, sigma=0.1)
    with pytest.raises(_lib.MfxError, match="no CPU path"):
        T.profile(np.ones((1, T.M)), pk, K)


class _Tables:
    """Stands for a RotateAtom2DTables of M rows; the argument checks must be done before its handle is asked for."""
    M, N, device = 66, 14, 0

    def handle(self):
        raise AssertionError("the device handle was touched before the arguments were checked")


def test_engine_argument_errors_come_before_the_device():
    import torch
    T = _Tables()
    V = 5
    Y, pk, K = np.zeros((V, 66)), np.zeros((V, 6)), np.full(V, 2)
    for call in (lambda *a, **k: engine.posterior2d(T, *a, 1.0, **k), lambda *a, **k: engine.profile2d(T, *a, **k)):
        with pytest.raises(ValueError, match="protocol has 66"):
            call(np.zeros((V, 63)), K, pk, 2)
        with pytest.raises(ValueError, match="one entry per voxel"):
            call(Y, np.full(V + 1, 2), pk, 2)
        with pytest.raises(ValueError, match="peaks should have 6 columns"):
            call(Y, K, np.zeros((V, 3)), 2)
        with pytest.raises(ValueError, match=r"0\.\.maxfasc"):
            call(Y, np.full(V, 3), pk, 2)
        with pytest.raises(ValueError, match="csf should have one entry per voxel"):
            call(Y, K, pk, 2, csf=np.zeros(V + 1, bool))
    with pytest.raises(ValueError, match="sigma should be a scalar or have one entry per voxel"):
        engine.posterior2d(T, Y, K, pk, 2, np.ones(V + 1))
    with pytest.raises(ValueError, match="shift should be a scalar or have one entry per voxel"):
        engine.posterior2d(T, Y, K, pk, 2, 1.0, shift=np.ones((V, 2)))
    # a set with nothing in scope needs no device: all rows NaN, all counted, status -1
    w, ls, st, ds, n = engine.posterior2d(T, np.zeros((3, 66)), np.array([0, 2, 3]), np.zeros((3, 9)), 3, 1.0,
                                          csf=np.array([False, True, False]))
    assert n == 3 and w.shape == (3, 3, 14) and np.isnan(w).all() and np.isnan(ls).all() and (st == -1).all() and (ds == 0).all()
    obj, par, ds, n = engine.profile2d(T, np.zeros((3, 66)), np.array([0, 2, 3]), np.zeros((3, 9)), 3, partner=True,
                                       csf=np.array([False, True, False]))
    assert n == 3 and obj.shape == (3, 3, 14) and np.isnan(obj).all() and (par == -1).all()
    # the device entry points: shapes and K before the tensors' residence and the handle
    tY, tpk, tT = torch.zeros((V, 66), dtype=torch.float64), torch.zeros((V, 6), dtype=torch.float64), torch.ones(V, dtype=torch.float64)
    for call in (lambda y, p, k: engine.posterior2d_dev(T, y, p, k, tT, tT), lambda y, p, k: engine.profile2d_dev(T, y, p, k)):
        with pytest.raises(NotImplementedError, match="K = 1 or 2"):
            call(tY, torch.zeros((V, 9), dtype=torch.float64), 3)
        with pytest.raises(NotImplementedError, match="K = 1 or 2"):
            call(tY, torch.zeros((V, 0), dtype=torch.float64), 0)
        with pytest.raises(ValueError, match="protocol has 66"):
            call(tY[:, :60], tpk, 2)
        with pytest.raises(ValueError, match=r"peaks should have shape \(5, 3\)"):
            call(tY, tpk, 1)
    with pytest.raises(ValueError, match="T should be a tensor with one entry per voxel"):
        engine.posterior2d_dev(T, tY, tpk, 2, tT[:4], tT)
    with pytest.raises(ValueError, match="shift should be a tensor with one entry per voxel"):
        engine.posterior2d_dev(T, tY, tpk, 2, tT, 0.0)


def test_tables_argument_errors_come_before_the_device(rot):
    T = U.RotateAtom2DTables(rot["syn2_sig"], rot["syn2_sch"], Z, 2.2e-9)
    T.handle = _Tables().handle
    V = 4
    Y, pk, K = np.ones((V, T.M)), np.tile([0.0, 0.0, 1.0, 1.0, 0.0, 0.0], (V, 1)), np.full(V, 2)
    for m in (T.posterior, T.profile):
        with pytest.raises(ValueError, match="on_error"):
            m(Y, pk, K, on_error="ignore")
        with pytest.raises(ValueError, match="protocol has 66"):
            m(Y[:, :60], pk, K)
        with pytest.raises(ValueError, match="numfasc should have one entry"):
            m(Y, pk, K[:3])
        with pytest.raises(ValueError, match="3 maxfasc"):
            m(Y, pk[:, :5], K)
        with pytest.raises(ValueError, match=r"numfasc should lie in 0\.\.2"):
            m(Y, pk, np.full(V, 3))
        with pytest.raises(ValueError, match="property rad has 2 entries"):
            m(Y, pk, K, props={"rad": np.ones(2)})
    with pytest.raises(ValueError, match="rel and delta"):
        U.profile_interval(np.zeros((1, 2, T.N)), np.ones(T.N), rel=-1.0)
    for name in ("posterior", "profile", "interval", "posterior_moments"):
        assert callable(getattr(U.RotateAtom2DTables, name))
    for name in ("posterior2d", "posterior2d_dev", "profile2d", "profile2d_dev"):
        assert callable(getattr(engine, name))


def test_result_objects_behave_as_specified():
    """The classes RotateAtom2DTables.posterior / .profile return, on hand-made values with a props dict."""
    rad = np.array([2.0, 1.0, 2.0, 4.0])
    w = np.array([[[0.25, 0.25, 0.25, 0.25], [0.5, 0.0, 0.0, 0.5]],
                  [[0.0, 1.0, 0.0, 0.0], [np.nan] * 4]])
    T, M = np.array([0.02, 0.08]), 66
    p = mfmod.Posterior(w, np.array([-3.0, -7.0]), np.zeros(2, dtype=np.int32), 0, np.arange(2), {"rad": rad}, np.array([2, 1]), T, M)
    assert np.allclose(p.mean("rad")[[0, 0, 1], [0, 1, 0]], [2.25, 3.0, 1.0], rtol=1e-15) and np.isnan(p.mean("rad")[1, 1])
    assert np.allclose(p.std("rad")[[0, 0, 1], [0, 1, 0]], [np.sqrt(19.0) / 4, 1.0, 0.0], rtol=1e-15)
    assert np.array_equal(p.quantile("rad", 0.5)[0], [2.0, 2.0])
    lv, by = p.by_property("rad")
    assert np.array_equal(lv, [1.0, 2.0, 4.0]) and np.array_equal(by[0], [[0.25, 0.5, 0.25], [0.0, 0.5, 0.5]])
    want = np.array([-3.0, -7.0]) - np.array([2, 1]) * np.log(4) - 0.5 * M * np.log(np.pi * T)
    assert np.allclose(p.log_evidence(), want, rtol=1e-15)
    with pytest.raises(ValueError, match="unknown fascicle property"):
        p.mean("fin")
    obj = np.array([[[3.0, 1.0, 2.0, 5.0], [np.nan] * 4]])
    o = mfmod.ObjectiveProfile(obj, None, 0, np.arange(1), {"rad": rad})
    lv, by = o.by_property("rad")
    assert np.array_equal(by[0, 0], [1.0, 2.0, 5.0]) and np.isnan(by[0, 1]).all() and o.partner is None
    lo, hi, cnt = U.profile_interval(obj, rad, rel=1.0)
    assert (lo[0, 0], hi[0, 0], cnt[0, 0]) == (1.0, 2.0, 2) and np.isnan(lo[0, 1]) and cnt[0, 1] == 0


def test_float64_restatement_of_the_referee_stays_within_the_bar(rot):
    """The referee's posterior in float64 NumPy against its long-double form on the golden F (the reference's own
    lsqnonneg_2var_opt values) at sigma^2 = MSE M / (M - 2): the bar has to hold for plain float64 arithmetic of the same
    formulas, or it is no bar for the kernel.  Along the way the stored file is checked against the golden fit: the same
    voxels, min F the fit's objective within B at the fitted pair, no pair near the cut, dF small."""
    gold, g = np.load(os.path.join(G, "fit2d_cases.npz")), np.load(os.path.join(G, "soft2d_cases.npz"))
    cut = float(g["cut"])
    assert cut == 1e-8
    assert os.path.getsize(os.path.join(G, "soft2d_cases.npz")) < os.path.getsize(os.path.join(G, "fit2d_cases.npz"))
    worst = 0.0
    for name in ("syn2", "fix"):
        M = rot[name + "_sch"].shape[0]
        v2 = g[name + "_vox2"]
        K, csf = gold[name + "_K"], gold[name + "_csf"].astype(bool)
        assert np.array_equal(v2, np.flatnonzero((K == 2) & ~csf)) and np.array_equal(g[name + "_vox1"], np.flatnonzero((K == 1) & ~csf))
        for r, v in enumerate(v2):
            F, c2, ysq = g[name + "_F2"][r], g[name + "_c2"][r], float(g[name + "_ysq2"][r])
            assert R.clear_of_the_cut([c2], cut), "a pair near the cut: the generator asserts there is none"
            c2bar = np.where(c2 <= cut, 1.0, c2)
            sse = float(gold[name + "_params"][v, -2]) * M
            i, j = np.unravel_index(np.argmin(F), F.shape)
            assert abs(F.min() - sse) <= 16 * M * EPS * ysq / c2bar[i, j]
            assert (i, j) == tuple(gold[name + "_params"][v, 3:5].astype(int))
            assert np.all(g[name + "_dF2"][r] >= 0) and g[name + "_dF2"][r].max() <= 1e-9 * ysq
            Tv = 2.0 * sse / (M - 2)
            ref = R.posterior(F.astype(R.LD), c2bar, ysq, M, Tv)
            f64 = R.posterior(F, c2bar, ysq, M, Tv, dt=np.float64)
            ratio = R.worst_ratio(f64["w"], f64["log_sum"], ref)
            worst = max(worst, ratio)
            print("%s voxel %d: float64 against long double: %.3g of the bar (bar on log_sum %.3g, %.1f effective pairs)"
                  % (name, v, ratio, float(ref["bar_log_sum"]), ref["neff"]))
            for k in range(2):
                assert abs(float(ref["w"][k].sum()) - 1.0) < 1e-15
        for r, v in enumerate(g[name + "_vox1"]):
            F = g[name + "_F1"][r]
            assert abs(F.min() - float(gold[name + "_params"][v, -2]) * M) <= 16 * M * EPS * float(g[name + "_ysq1"][r])
            assert int(np.argmin(F)) == int(gold[name + "_params"][v, 3])
    print("worst float64 / long double error = %.3g of the bar" % worst)
    assert worst <= 1.0
