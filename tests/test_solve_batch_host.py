"""Batched explicit-dictionary solver (include/mfx_solve.h), the parts that need no GPU: the C ABI, the assertions of the
one-problem wrapper on the dictionary, the shape errors (each before any device call), and that nothing is computed on
the host without a device."""
import os
import re

import numpy as np
import pytest

from microstructure_fingerprinting_amd import _lib, engine
from microstructure_fingerprinting_amd import mf_utils as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    src = open(os.path.join(ROOT, "include", "mfx_solve.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(mfx_[a-z_0-9]+)\s*\(", src)))


def test_solve_abi_symbols():
    lib = _lib.lib()
    assert sorted(_lib.SOLVE_EXPORTS) == _declared()
    for name in ("mfx_solve_abi_version", "mfx_solve_create", "mfx_solve_destroy", "mfx_solve_num_columns", "mfx_solve_batch_dev",
                 "mfx_solve_batch", "mfx_solve_debug_set_force_generic"):
        assert name in _lib.SOLVE_EXPORTS
    for name in _lib.SOLVE_EXPORTS:
        assert hasattr(lib, name)
        assert name not in _lib.EXPORTS
    assert lib.mfx_solve_abi_version() == 1
    assert lib.mfx_solve_num_columns(None) == -1 and lib.mfx_solve_bytes_per_signal(None) == -1
    lib.mfx_solve_destroy(None)
    assert callable(engine.solve_batch_dev) and callable(U.solve_exhaustive_posweights_batch)


class _NoHandle(U.ExhaustiveSolver):
    def handle(self):
        raise AssertionError("the device was touched before the arguments were checked")


def test_dictionary_assertions_are_those_of_the_single_wrapper():
    A = np.abs(np.random.default_rng(0).standard_normal((6, 5)))
    y = np.ones(6)
    sizes = np.array([3, 2])
    Z = A.copy(); Z[:, 1] = 0
    for a, s, msg in [
            (A.tolist(), sizes, "A should be a NumPy ndarray"),
            (A[:, 0], sizes, "A should be a 2D array"),
            (Z, sizes, "All-zero columns detected in A"),
            (np.zeros((6, 0)), sizes, "A and y should not be empty arrays"),
            (A, [3, 2], "dicsizes should be a NumPy ndarray"),
            (A, np.array([5, 0]), "All entries of dicsizes should be > 0"),
            (A, np.array([3, 3]), r"Number of columns of A \(5\) does not equal sum of size of sub-matrices in diclengths array \(6\)")]:
        with pytest.raises(AssertionError, match=msg):
            _NoHandle(a, s)
        if isinstance(a, np.ndarray) and a.ndim == 2 and a.shape[0] == 6:   # the single wrapper: the same text
            with pytest.raises(AssertionError, match=msg):
                U.solve_exhaustive_posweights(a, y, s)
        with pytest.raises(AssertionError, match=msg):
            U.solve_exhaustive_posweights_batch(a, y[None, :], s)
    with pytest.raises(AssertionError, match="y should be a NumPy ndarray"):
        _NoHandle(A, sizes).solve(y.tolist())


def test_shape_errors_name_both_shapes_and_come_before_the_device():
    A = np.abs(np.random.default_rng(1).standard_normal((6, 5)))
    S = _NoHandle(A, np.array([3, 2]))
    assert (S.M, S.num_columns, S.Kp) == (6, 5, 2) and list(S.dicsizes) == [3, 2] and list(S.starts) == [0, 3]
    for Y in (np.ones((4, 5)), np.ones(5), np.ones((2, 3, 6)), np.ones((6, 1)), np.array(1.0)):
        with pytest.raises(ValueError) as e:
            S.solve(Y)
        assert "(6, 5)" in str(e.value) and str(tuple(Y.shape)) in str(e.value)
    assert S.signal_rows((6,)) == 1 and S.signal_rows((0, 6)) == 0 and S.signal_rows((9, 6)) == 9
    assert S._h is None
    # no signal: empty arrays, no launch (the handle is never asked for)
    w, sub, tot, obj, yrec, status = S.solve(np.zeros((0, 6)))
    assert w.shape == (0, 2) and sub.shape == (0, 2) and tot.shape == (0, 2) and obj.shape == (0,) and yrec.shape == (0, 6)
    assert status.shape == (0,) and status.dtype == np.int32 and sub.dtype == np.int32 and tot.dtype == np.int32
    assert S.solve(np.zeros((0, 6)), recons=False)[4] is None
    assert _NoHandle(np.ones((3, 4)), np.array([1, 1, 1, 1])).solve(np.zeros((0, 3)))[1].dtype == np.int64
    with S as T:
        assert T is S
    S.close()


def test_no_host_computation_without_a_device():
    lib = _lib.lib()
    A = np.abs(np.random.default_rng(2).standard_normal((6, 5)))
    sizes = np.array([3, 2], dtype=np.int64)
    if lib.mfx_device_count() > 0:      # with a device the same calls are served, on the device
        assert np.array_equal(U.ExhaustiveSolver(A, sizes).solve(np.ones((2, 6)))[5], [0, 0])
        assert lib.mfx_solve_batch_dev(None, None, 1, 0, None, None, None, None, None, None) == _lib.MFX_ERR_ARG
        return
    with pytest.raises((_lib.MfxError, NotImplementedError), match="no CPU path"):
        U.ExhaustiveSolver(A, sizes).solve(np.ones((2, 6)))
    with pytest.raises((_lib.MfxError, NotImplementedError), match="no CPU path"):
        U.solve_exhaustive_posweights_batch(A, np.ones(6), sizes)
    h = _lib.C.c_void_p()
    assert lib.mfx_solve_create(_lib.dptr(A), 5, 6, _lib.lptr(sizes), 2, 0, _lib.C.byref(h)) == _lib.MFX_ERR_NO_DEVICE
    assert not h.value
    assert lib.mfx_solve_batch_dev(None, None, 1, 0, None, None, None, None, None, None) == _lib.MFX_ERR_NO_DEVICE
    assert lib.mfx_solve_batch(None, None, 1, 0, None, None, None, None, None) == _lib.MFX_ERR_NO_DEVICE
    assert "no CPU path" in lib.mfx_last_error().decode()


def test_create_limits_and_messages():
    """The limits of mfx_solve_exhaustive, with its messages; the checks that come before the device look are the same
    with and without one."""
    lib = _lib.lib()
    A = np.ones((2, 9))
    h = _lib.C.c_void_p()
    nine = np.ones(9, dtype=np.int64)
    assert lib.mfx_solve_create(_lib.dptr(A), 9, 2, _lib.lptr(nine), 9, 0, _lib.C.byref(h)) == _lib.MFX_ERR_UNSUPPORTED
    assert "at most 8 sub-dictionaries are supported (got 9)" in lib.mfx_last_error().decode()
    assert lib.mfx_solve_create(None, 9, 2, _lib.lptr(nine), 2, 0, _lib.C.byref(h)) == _lib.MFX_ERR_ARG
    assert not h.value
