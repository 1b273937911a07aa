"""rotate_atom_2Dprotocol on the device against the reference's outputs (tests/golden/rot2d_cases.npz,
written by gen_golden_rot2d.py).

Bit equality with the reference is not attainable: its rotated gradients come from a BLAS product (FMA,
blocked sums) and the device's acos / sin / cos / exp differ from the C library's in the last bit.  Every
step after the rotation follows the reference's operation order, so the bar is rtol 1e-10, atol 1e-13 (that
of rotate_atom).  Batches, single calls, the one-atom variant and the device-resident path are compared
with each other bit for bit."""
import json
import os

import numpy as np
import pytest

from microstructure_fingerprinting_amd import engine
from microstructure_fingerprinting_amd import mf_utils as U

pytestmark = pytest.mark.gpu

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
RTOL, ATOL = 1e-10, 1e-13


@pytest.fixture(scope="module")
def d():
    return np.load(os.path.join(G, "rot2d_cases.npz"))


def _groups(d):
    return list(enumerate(json.loads(str(d["values_json"]))))


def _close(out, ref):
    assert out.shape == ref.shape
    assert np.all(np.abs(out - ref) <= ATOL + RTOL * np.abs(ref)), np.max(np.abs(out - ref))


def _tables(d, v):
    return U.RotateAtom2DTables(d[v["sig"]], d[v["sch"]], np.array(v["refdir"]), v["DIFF"])


def test_value_cases_match_reference(d):
    for gi, v in _groups(d):
        dirs, ref = d["val%d_dirs" % gi], d["val%d_out" % gi]
        T = _tables(d, v)
        out = T.rotate(dirs)
        for k in range(v["n"]):
            _close(out[k].reshape(ref[k].shape), ref[k])
            single = U.rotate_atom_2Dprotocol(d[v["sig"]], d[v["sch"]], np.array(v["refdir"]), dirs[k], v["DIFF"])
            assert single.shape == ref[k].shape          # 1-D signals stay 1-D
            assert np.array_equal(single.reshape(out[k].shape), out[k])


def _device_errors(d):
    return [e for e in json.loads(str(d["errors_json"])) if not e["host"]]


def test_error_cases_match_reference(d):
    errs = _device_errors(d)
    assert len(errs) >= 4
    for e in errs:
        with pytest.raises(Exception) as ei:
            U.rotate_atom_2Dprotocol(d[e["sig"]], d[e["sch"]], np.array(e["refdir"]), np.array(e["newdir"]), e["DIFF"])
        assert (type(ei.value).__name__, str(ei.value)) == (e["type"], e["msg"]), e["why"]


def test_batch_raises_for_the_lowest_failing_direction(d):
    e = next(x for x in _device_errors(d) if "in-plane" in x["why"])
    T = U.RotateAtom2DTables(d[e["sig"]], d[e["sch"]], np.array(e["refdir"]), e["DIFF"])
    good = d["val0_dirs"][4:6]
    dirs = np.vstack([good, [e["newdir"]], [[0.0, 0.6, 0.6]]])
    with pytest.raises(AssertionError) as ei:
        T.rotate(dirs)
    assert str(ei.value) == e["msg"]
    with pytest.raises(ValueError, match="unit norm"):
        T.rotate(np.vstack([good, [[0.0, 0.6, 0.6]], [e["newdir"]]]))


def _random_dirs(rng, n, zmin=0.1):
    v = rng.standard_normal((4 * n, 3))
    v /= np.sqrt(np.sum(v ** 2, axis=1, keepdims=True))
    return np.ascontiguousarray(v[np.abs(v[:, 2]) >= zmin][:n])


def test_batch_equals_single_calls_bitwise(d):
    v = _groups(d)[1][1]
    T = _tables(d, v)
    dirs = _random_dirs(np.random.default_rng(1), 64)
    out = T.rotate(dirs)
    for k in range(64):
        assert np.array_equal(T.rotate(dirs[k:k + 1])[0], out[k])


def test_rotate_cols_equals_rotate_column(d):
    for gi in (0, 3):
        v = _groups(d)[gi][1]
        T = _tables(d, v)
        dirs = d["val%d_dirs" % gi]
        full = T.rotate(dirs)
        cols = np.arange(dirs.shape[0]) % T.N
        got = T.rotate_cols(dirs, cols)
        assert np.array_equal(got, full[np.arange(dirs.shape[0]), :, cols])


def test_dev_path_equals_host_path(d):
    import torch
    v = _groups(d)[0][1]
    T = _tables(d, v)
    dirs = d["val0_dirs"]
    host = T.rotate(dirs)
    dd = torch.from_numpy(dirs).cuda()
    out, st = engine.rotate2d_dev(T, dd)
    torch.cuda.synchronize()
    assert np.all(st.cpu().numpy() == 0)
    assert np.array_equal(out.cpu().numpy(), host)
    cols = torch.arange(dirs.shape[0], dtype=torch.int32, device="cuda") % T.N
    oc, sc = engine.rotate2d_dev(T, dd, cols)
    assert np.all(sc.cpu().numpy() == 0)
    assert np.array_equal(oc.cpu().numpy(), host[np.arange(dirs.shape[0]), :, cols.cpu().numpy()])
    # a failing direction: its status record, NaN output, the reference's exception
    bad = torch.from_numpy(np.vstack([dirs[:2], [[0.7071067811865476, 0.7071067811865476, 0.0]]])).cuda()
    ob, sb = engine.rotate2d_dev(T, bad)
    s = sb.cpu().numpy()
    assert np.all(s[:2] == 0) and s[2, 0] == U.ROT2D_NEW_PAIRS and s[2, 1] == 0 and s[2, 2] == 4
    assert np.all(np.isnan(ob[2].cpu().numpy())) and np.array_equal(ob[:2].cpu().numpy(), host[:2])
    with pytest.raises(AssertionError, match="found 4 instead of 2 pairs"):
        T.raise_for_status(s)


def test_large_batch(d):
    sig = d["fix_sig"][:, np.arange(64) % 3] * (1.0 + 0.01 * np.arange(64))
    T = U.RotateAtom2DTables(sig, d["fix_sch"], np.array([0.0, 0.0, 1.0]), 2.2e-9)
    dirs = _random_dirs(np.random.default_rng(2), 512)
    out = T.rotate(dirs)                                  # 512 x 1776 x 64 doubles, about 465 MB
    assert out.shape == (512, 1776, 64) and np.all(np.isfinite(out))
    for k in np.random.default_rng(3).choice(512, 8, replace=False):
        assert np.array_equal(T.rotate(dirs[k:k + 1])[0], out[k])
