"""The 2-D protocol rotation (mfx_rot2d_plan_kernel / mfx_rot2d_eval_kernel / mfx_rot2d_cols_kernel) against an
independent referee (tests/_rot2d_ref.py, pinned on the reference by tests/test_rot2d_ref_host.py) and against the
wide recording of the reference (tests/golden/rot2d_wide.npz): whole populations of directions with the failing ones
among them, (Delta, delta) pairs of more than 256 rows, rows of different pairs interleaved, repeated rows, atom
counts past one and two trips of the evaluation loops, and the row limit.

Everything goes through the C ABI as RotateAtom2DTables.rotate does, but reads the [B, 4] status array instead of
raising.  Bar: rtol 1e-10, atol 1e-13 (tests/test_rot2d_gpu.py).  A direction the referee calls unclear (a decision
within rounding of its threshold, see _rot2d_ref) is run, must give a status record and finite values or a NaN block,
and is left out of the value and status comparisons."""
import numpy as np
import pytest

import _rot2d_ref as ref2d
import _rot2d_wide as W

from microstructure_fingerprinting_amd import _lib as L
from microstructure_fingerprinting_amd import engine
from microstructure_fingerprinting_amd import mf_utils as U

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def wide():
    return W.Wide()


def _rotate(T, dirs):
    d = L.f64c(dirs).reshape(-1, 3)
    out = np.zeros((d.shape[0], T.M, T.N))
    status = np.full((d.shape[0], 4), -7, dtype=np.int32)
    L.check(L.lib().mfx_rot2d_rotate(T.handle(), L.dptr(d), d.shape[0], L.dptr(out), L.iptr(status)))
    return out, status


def _rotate_cols(T, dirs, cols):
    d = L.f64c(dirs).reshape(-1, 3)
    c = np.ascontiguousarray(cols, dtype=np.int32)
    out = np.zeros((d.shape[0], T.M))
    status = np.full((d.shape[0], 4), -7, dtype=np.int32)
    L.check(L.lib().mfx_rot2d_rotate_cols(T.handle(), L.dptr(d), L.iptr(c), d.shape[0], L.dptr(out), L.iptr(status)))
    return out, status


def _tables(wide, c):
    sch, sig = wide.protocol(c)
    return U.RotateAtom2DTables(sig, sch, np.array(c["refdir"]), wide.DIFF)


def _check_against(T, out, status, results, recorded=None):
    """every direction: a status record and finite values or a NaN block; every clear one: the referee's (and the
    recording's) outcome and the referee's values.  Returns the number of clear successes and of clear failures."""
    assert np.all((status[:, 0] >= 0) & (status[:, 0] <= U.ROT2D_NO_REF_LINE))
    n_ok = n_bad = 0
    for k, r in enumerate(results):
        if status[k, 0] == U.ROT2D_OK:
            assert np.all(np.isfinite(out[k])), k
        else:
            assert np.all(np.isnan(out[k])), k
        if not r.clear:
            continue
        if recorded is not None:
            assert r.error == recorded(k), k
        if r.error is None:
            assert status[k, 0] == U.ROT2D_OK, (k, status[k])
            assert W.worst_ratio(out[k], r.out) <= 1.0, (k, W.worst_ratio(out[k], r.out))
            n_ok += 1
        else:
            e = T.error_for(status[k])
            assert (type(e).__name__, str(e)) == r.error, (k, status[k])
            n_bad += 1
    return n_ok, n_bad


@pytest.mark.parametrize("key", W.keys())
def test_population_against_recording_and_referee(wide, key):
    c = wide.combo(key)
    T = _tables(wide, c)
    dirs = wide.w[key + "_dirs"]
    results = wide.results(c)
    out, status = _rotate(T, dirs)
    n_ok, n_bad = _check_against(T, out, status, results, lambda k: wide.recorded(c, k))
    assert n_ok >= 250 and n_bad >= 3
    vidx, vrows, val = wide.w[key + "_vidx"], wide.w[key + "_vrows"], wide.w[key + "_val"]
    for i, k in enumerate(vidx):
        if results[k].clear:
            assert W.worst_ratio(out[k][vrows[i]], val[i]) <= 1.0, (k, W.worst_ratio(out[k][vrows[i]], val[i]))
    # the failing directions of a batch do not touch the others
    good = status[:, 0] == U.ROT2D_OK
    out2, status2 = _rotate(T, dirs[good])
    assert np.all(status2 == 0) and np.array_equal(out2, out[good])


def _tiled_atoms(sig, N):
    n = np.arange(N)
    return np.ascontiguousarray(sig[:, n % sig.shape[1]] * (1.0 + 0.01 * n))


@pytest.mark.parametrize("N", [1, 2, 3, 255, 256, 257, 511, 512, 513, 782, 1025])
def test_atom_loop_trips(wide, N):
    """protocol A, reference direction o1: the evaluation kernel's atom loops (256 per trip, 512 with double2) before,
    at and past one and two trips, for a generic direction, one that makes a line vanish and one that extrapolates"""
    c = wide.combo("A_o1")
    sch, sig4 = wide.protocol(c)
    sig = _tiled_atoms(sig4, N)
    name = {n: k for k, n in enumerate(wide.edge_names)}
    dirs = wide.w["A_o1_dirs"][[c["n_edge"], name["line1"], name["+z"]]]
    R = ref2d.Referee(sig, sch, np.array(c["refdir"]), wide.DIFF)
    res = [R.rotate(d) for d in dirs]
    assert all(r.clear and r.error is None for r in res)
    assert res[0].margins["vanished"] == 0 and res[1].margins["vanished"] > 0 and res[2].margins["extrapolated"] > 0
    T = U.RotateAtom2DTables(sig, sch, np.array(c["refdir"]), wide.DIFF)
    out, status = _rotate(T, dirs)
    assert out.shape == (3, 352, N)
    assert _check_against(T, out, status, res) == (3, 0)
    cols = np.array([0, N - 1, N // 2])
    oc, sc = _rotate_cols(T, np.repeat(dirs, 3, axis=0), np.tile(cols, 3))
    assert np.all(sc == 0)
    for b in range(9):
        want = res[b // 3].out[:, cols[b % 3]]
        assert W.worst_ratio(oc[b], want) <= 1.0, (b, W.worst_ratio(oc[b], want))
        assert np.array_equal(oc[b], out[b // 3][:, cols[b % 3]])


def test_rows_sorted_by_pair_give_the_interleaved_result(wide):
    """the plan kernel indexes its LDS arrays by position in pair_rows and everything else by row: protocol A with
    its rows sorted by pair (pair_rows the identity) must give the interleaved result, rows permuted back"""
    c = wide.combo("A_o1")
    sch, sig = wide.protocol(c)
    dirs = wide.w["A_o1_dirs"]
    perm = np.lexsort((np.arange(sch.shape[0]), sch[:, 5], sch[:, 4]))      # stable: rows keep their order inside a pair
    assert not np.array_equal(perm, np.arange(sch.shape[0]))
    Ti = _tables(wide, c)
    Ts = U.RotateAtom2DTables(sig[perm], sch[perm], np.array(c["refdir"]), wide.DIFF)
    assert not np.array_equal(Ti._arrays["pair_rows"], np.arange(Ti.M))
    assert np.array_equal(Ts._arrays["pair_rows"], np.arange(Ts.M))
    oi, si = _rotate(Ti, dirs)
    os_, ss = _rotate(Ts, dirs)
    assert np.array_equal(si, ss)
    assert np.array_equal(os_, oi[:, perm, :], equal_nan=True)
    assert (si[:, 0] == 0).sum() >= 250


def test_row_limit(wide):
    """4000 rows fill the plan kernel's two LDS arrays (the C populations run there); 4001 are refused at creation"""
    c = wide.combo("C_z")
    sch, sig = wide.protocol(c)
    assert sch.shape[0] == 4000
    T = _tables(wide, c)
    out, status = _rotate(T, wide.w["C_z_dirs"][c["n_edge"]:c["n_edge"] + 2])
    assert np.all(status == 0) and np.all(np.isfinite(out))
    T1 = U.RotateAtom2DTables(np.vstack([sig, sig[:1]]), np.vstack([sch, sch[:1]]), np.array(c["refdir"]), wide.DIFF)
    assert T1.M == 4001
    with pytest.raises(NotImplementedError, match="more than 4000 protocol rows"):
        T1.handle()
    assert T1._h is None


def test_predict2d_stands_on_the_referee(wide):
    """one single-fascicle parameter row of protocol A: M0 nu times the referee's column"""
    c = wide.combo("A_o1")
    T = _tables(wide, c)
    k = c["n_edge"] + 1
    r = wide.results(c)[k]
    assert r.clear and r.error is None
    M0, nu, atom = 1.7, 0.625, 2
    params = np.array([[M0, nu, float(atom), 0.0, 0.0]])
    out, dstat = engine.predict2d(T, params, wide.w["A_o1_dirs"][k:k + 1], 1)
    assert np.all(dstat == 0)
    want = (M0 * nu) * r.out[:, atom]
    assert W.worst_ratio(out[0], want) <= 1.0, W.worst_ratio(out[0], want)
