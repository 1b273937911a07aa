"""Soft answers of the batched explicit solver (include/mfx_solve_soft.h), the parts that need no GPU: the C ABI, that
nothing is computed without a device, that the argument checks come before the device is touched, and that the inputs of
tests/test_solve_soft_gpu.py can tell a right kernel from a wrong one: every case is clear of the cut, the broad noise
level spreads the posterior over at least NEFF_FLOOR pairs, and there a float64 restatement that drops ONE pair from the
sums misses the referee's bar a thousandfold (at the peaked level it is invisible: neff is 1)."""
import os
import re

import numpy as np
import pytest

import _solve_soft_cases as SC
from microstructure_fingerprinting_amd import _lib, engine
from microstructure_fingerprinting_amd import mf_utils as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    src = open(os.path.join(ROOT, "include", "mfx_solve_soft.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(mfx_[a-z_0-9]+)\s*\(", src)))


def test_solve_soft_abi_symbols():
    lib = _lib.lib()
    assert sorted(_lib.SOLVE_SOFT_EXPORTS) == _declared()
    for name in ("mfx_solve_soft_abi_version", "mfx_solve_soft_bytes_per_signal", "mfx_solve_profile_dev", "mfx_solve_profile",
                 "mfx_solve_post_dev", "mfx_solve_post"):
        assert name in _lib.SOLVE_SOFT_EXPORTS
    for name in _lib.SOLVE_SOFT_EXPORTS:
        assert hasattr(lib, name)
        assert name not in _lib.EXPORTS and name not in _lib.SOLVE_EXPORTS
    assert lib.mfx_solve_soft_abi_version() == 1
    assert lib.mfx_solve_abi_version() == 1   # the solver's own header is as it was
    assert lib.mfx_solve_soft_bytes_per_signal(None, 0) == -1 and lib.mfx_solve_soft_bytes_per_signal(None, 1) == -1
    assert lib.mfx_solve_soft_served(None) == _lib.MFX_ERR_ARG
    assert callable(engine.solve_profile_dev) and callable(engine.solve_posterior_dev)
    for name in ("profile", "posterior", "posterior_moments"):
        assert callable(getattr(U.ExhaustiveSolver, name))


def test_no_host_computation_without_a_device():
    lib = _lib.lib()
    if lib.mfx_device_count() > 0:      # with a device the same calls are served, on the device
        A = np.abs(np.random.default_rng(2).standard_normal((6, 5)))
        with U.ExhaustiveSolver(A, np.array([3, 2])) as S:
            assert np.array_equal(S.profile(np.ones((2, 6))).status, [0, 0])
            assert np.array_equal(S.posterior(np.ones((2, 6)), sigma=1.0).status, [0, 0])
        assert lib.mfx_solve_profile_dev(None, None, 1, 0, None, None, None, None, None, None) == _lib.MFX_ERR_ARG
        return
    assert lib.mfx_solve_profile_dev(None, None, 1, 0, None, None, None, None, None, None) == _lib.MFX_ERR_NO_DEVICE
    assert lib.mfx_solve_profile(None, None, 1, 0, None, None, None, None, None) == _lib.MFX_ERR_NO_DEVICE
    assert lib.mfx_solve_post_dev(None, None, 1, None, None, 0, None, None, None, None, None, None) == _lib.MFX_ERR_NO_DEVICE
    assert lib.mfx_solve_post(None, None, 1, None, None, 0, None, None, None, None, None) == _lib.MFX_ERR_NO_DEVICE
    assert "no CPU path" in lib.mfx_last_error().decode()
    A = np.abs(np.random.default_rng(2).standard_normal((6, 5)))
    for call in (lambda S: S.profile(np.ones((2, 6))), lambda S: S.posterior(np.ones((2, 6)), sigma=1.0),
                 lambda S: S.posterior_moments(np.ones((2, 6)), np.arange(3.0), sigma=1.0)):
        with pytest.raises((_lib.MfxError, NotImplementedError), match="no CPU path"):
            call(U.ExhaustiveSolver(A, np.array([3, 2])))


class _NoHandle(U.ExhaustiveSolver):
    def handle(self):
        raise AssertionError("the device was touched before the arguments were checked")


def test_argument_checks_come_before_the_device():
    A = np.abs(np.random.default_rng(1).standard_normal((6, 5)))
    S = _NoHandle(A, np.array([3, 2]))
    for Y in (np.ones((4, 5)), np.ones(5), np.ones((2, 3, 6)), np.ones((6, 1)), np.array(1.0)):
        for call in (S.profile, lambda y: S.posterior(y, sigma=1.0), lambda y: S.posterior_moments(y, np.arange(3.0), sigma=1.0)):
            with pytest.raises(ValueError) as e:
                call(Y)
            assert "(6, 5)" in str(e.value) and str(tuple(Y.shape)) in str(e.value)
    for call in (S.profile, S.posterior):
        with pytest.raises(AssertionError, match="y should be a NumPy ndarray"):
            call(np.ones((2, 6)).tolist())
    Y = np.ones((4, 6))
    with pytest.raises(ValueError, match=r"sigma should be a scalar or have one entry per voxel \(4\)"):
        S.posterior(Y, sigma=np.ones(3))
    with pytest.raises(ValueError, match=r"shift should be a scalar or have one entry per voxel \(4\)"):
        S.posterior(Y, sigma=1.0, shift=np.ones((4, 1)))
    with pytest.raises(ValueError, match="property 'rad' of sub-dictionary 1 should have 2 values"):
        S.profile(Y, props={"rad": np.arange(3.0)})
    with pytest.raises(ValueError, match="property 'rad' of sub-dictionary 0 should have 3 values"):
        S.posterior(Y, sigma=1.0, props={"rad": [np.arange(2.0), np.arange(2.0)]})
    assert S._h is None
    # the torch route: what solve_batch_dev asserts and says, before the handle is asked for
    import torch
    for fn in (engine.solve_profile_dev, lambda s, y: engine.solve_posterior_dev(s, y, y)):
        with pytest.raises(AssertionError):
            fn(S, torch.ones((4, 6), dtype=torch.float64))        # not a CUDA tensor
    assert S._h is None


def test_result_objects_on_host_arrays():
    """SolverProfile / SolverPosterior are thin views on the existing helpers of mf_utils"""
    obj = [np.array([[3.0, 1.0, 2.0]]), np.array([[5.0, 1.0]])]
    P = U.SolverProfile(obj, None, np.zeros(1, np.int32), {"rad": [np.array([1.0, 2.0, 2.0]), np.array([7.0, 8.0])]})
    lev, by = P.by_property("rad")
    assert np.array_equal(lev, [1.0, 2.0]) and np.array_equal(by, [[3.0, 1.0]])
    lo, hi, cnt = P.interval("rad", delta=1.0)
    assert (lo[0], hi[0], cnt[0]) == (2.0, 2.0, 2)
    lo, hi, cnt = P.interval("rad", k=1)
    assert (lo[0], hi[0], cnt[0]) == (8.0, 8.0, 1)
    with pytest.raises(KeyError):
        P.by_property("fin")
    w = [np.array([[0.25, 0.75]]), np.array([[1.0]])]
    Q = U.SolverPosterior(w, np.array([-3.0]), np.array([0.5]), np.zeros(1, np.int32), np.array([2.0]), 10, {"rad": [np.array([1.0, 3.0]), np.array([4.0])]})
    assert Q.mean("rad")[0] == 2.5 and abs(Q.std("rad")[0] - np.sqrt(0.75)) < 1e-15 and Q.mean("rad", k=1)[0] == 4.0
    assert Q.quantile("rad", 0.5)[0] == 3.0 and np.array_equal(Q.by_property("rad")[1], [[0.25, 0.75]])
    assert abs(Q.log_evidence()[0] - (-3.0 - np.log(2) - np.log(1) - 5 * np.log(2 * np.pi))) < 1e-14


@pytest.mark.parametrize("sizes,M", SC.CASES, ids=SC.IDS)
def test_inputs_are_clear_of_the_cut_and_the_broad_leg_is_broad(sizes, M):
    ref = SC.referee(sizes, M)
    bs = SC.broad_sigma(sizes, M)
    assert bs >= 2.0
    for v, r in enumerate(ref):
        assert r["clear"], "signal %d" % v
        if v > 0:
            assert r["post"][bs]["neff"] >= SC.NEFF_FLOOR, "signal %d: neff %.1f at sigma %g" % (v, r["post"][bs]["neff"], bs)
    assert ref[1]["post"][SC.SIGMA_PEAKED]["neff"] < 1.5   # the peaked leg: one pair carries the sum


@pytest.mark.parametrize("sizes", [(150, 149), (65, 63), (33, 31, 1), (150, 149, 1)], ids=lambda s: "x".join(map(str, s)))
def test_one_dropped_pair_is_seen_on_the_broad_leg(sizes):
    """Power.  A float64 restatement agrees with the referee far inside the bar; the same restatement without the single
    pair (n1 - 1, n2 - 1) in its sums misses the bar by more than 1e3 at the broad noise level."""
    M = 17
    A, Y, _ = SC.problem(sizes, M)
    ref = SC.referee(sizes, M)
    bs = SC.broad_sigma(sizes, M)
    for v in (1, 2, 5, 20, 36):
        F, c2bar, _, ysq = SC.pair_F(A, sizes, Y[v], dt=np.float64)
        ok = SC.posterior_ref(F, c2bar, ysq, M, 2.0 * bs * bs, dt=np.float64)
        assert SC.worst_ratio(ok["w"], ok["log_sum"], ref[v]["post"][bs]) < 0.1
        Fd = F.copy()
        Fd[-1, -1] = np.inf                         # exp(-inf) = 0: the pair is absent from every sum
        bad = SC.posterior_ref(Fd, c2bar, ysq, M, 2.0 * bs * bs, dt=np.float64)
        miss = SC.worst_ratio(bad["w"], bad["log_sum"], ref[v]["post"][bs])
        print("%s signal %d: the dropped pair misses the bar by %.3g" % (sizes, v, miss))
        assert miss > 1e3
