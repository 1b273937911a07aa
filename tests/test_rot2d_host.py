"""2-D protocol rotation on the host: the helpers rotate_scheme_mat, vrrotvec2mat, rotate_vector,
get_perp_vector and project_PGSE_scheme_xy_plane against the reference's outputs, the validation that
raises before any device call (types and messages recorded in tests/golden/rot2d_cases.npz by
gen_golden_rot2d.py), the direction-independent tables, and the C ABI of include/mfx_rot2d.h.  No GPU needed."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

import microstructure_fingerprinting_amd as mf
from microstructure_fingerprinting_amd import _lib
from microstructure_fingerprinting_amd import mf_utils as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def d():
    return np.load(os.path.join(G, "rot2d_cases.npz"))


def test_names_are_exported():
    for name in ("rotate_atom_2Dprotocol", "RotateAtom2DTables", "rotate_scheme_mat", "vrrotvec2mat", "rotate_vector",
                 "get_perp_vector", "project_PGSE_scheme_xy_plane"):
        assert name in U.__all__
        assert getattr(mf.mf_utils, name) is getattr(U, name)


def test_rotate_scheme_mat_matches_reference(d):
    z = np.array([0.0, 0.0, 1.0])
    for nd, ref in zip(d["rsm_dirs"], d["rsm_out"]):
        out = U.rotate_scheme_mat(d["rsm_in"].copy(), z, nd)
        assert np.array_equal(out, ref)
    dirs = d["rsm_dirs"]
    assert np.array_equal(U.rotate_scheme_mat(d["rsm_in"].copy(), dirs[3], dirs[4]), d["rsm_pair_out"])


def test_rotate_scheme_mat_parallel_returns_input_object(d):
    sch = d["rsm_in"].copy()
    assert U.rotate_scheme_mat(sch, np.array([0, 0, 1]), np.array([0.0, 0.0, 1.0])) is sch
    assert U.rotate_scheme_mat(sch, np.array([0, 0, 1]), np.array([0.0, 0.0, -1.0])) is sch


def test_small_helpers_match_reference(d):
    for ax, th, ref in zip(d["vrm_axes"], d["vrm_theta"], d["vrm_out"]):
        assert np.array_equal(U.vrrotvec2mat(ax, th), ref)
    for v, ax, th, ref in zip(d["rv_v"], d["vrm_axes"], d["vrm_theta"], d["rv_out"]):
        assert np.array_equal(U.rotate_vector(v, ax, th), ref)
    assert np.array_equal(U.get_perp_vector(d["gpv_in"].copy()), d["gpv_out"])


def test_project_scheme_xy_plane(d, tmp_path):
    assert np.array_equal(U.project_PGSE_scheme_xy_plane(d["proj_in"].copy()), d["proj_out"])
    path = tmp_path / "proj.scheme"
    np.savetxt(str(path), d["proj_in"], header="VERSION: 1", comments="", fmt="%.17g")
    assert np.array_equal(U.project_PGSE_scheme_xy_plane(str(path)), d["proj_out"])
    one = U.project_PGSE_scheme_xy_plane(d["proj_in"][5].copy())
    assert np.array_equal(one, d["proj_out"][5:6])


def test_helper_errors_match_reference(d):
    for fn, args, etype, msg in json.loads(str(d["helper_errors_json"])):
        a = [d[v].copy() if isinstance(v, str) else (np.array(v) if isinstance(v, list) else v) for v in args]
        with pytest.raises(Exception) as ei:
            getattr(U, fn)(*a)
        assert type(ei.value).__name__ == etype
        assert str(ei.value) == msg


def _host_error_cases():
    dd = np.load(os.path.join(G, "rot2d_cases.npz"))
    return [(e["why"], e) for e in json.loads(str(dd["errors_json"])) if e["host"]]


@pytest.mark.parametrize("why,e", _host_error_cases())
def test_host_side_errors_raise_before_the_device(d, why, e):
    """Raised by the host before any device call: the same on a machine without a GPU."""
    with pytest.raises(Exception) as ei:
        U.rotate_atom_2Dprotocol(d[e["sig"]], d[e["sch"]], np.array(e["refdir"]), np.array(e["newdir"]), e["DIFF"])
    assert type(ei.value).__name__ == e["type"]
    assert str(ei.value) == e["msg"]


def test_error_cases_cover_the_reference_checks(d):
    errs = json.loads(str(d["errors_json"]))
    msgs = " ".join(e["msg"] for e in errs)
    for part in ("zeros for gz", "same number of elements", "should have unit norm", "found 4 unique",
                 "found 7 unique", "found 4 instead of 2 pairs", "trying to interpolate b0 sequences"):
        assert part in msgs


def test_tables_do_not_modify_the_scheme(d):
    sch = d["fix_sch"].copy()
    T = U.RotateAtom2DTables(d["fix_sig"], sch, np.array([0.0, 0.0, 1.0]), 2.2e-9)
    assert np.array_equal(sch, d["fix_sch"])
    # the new side sees the reference's in-place normalisation of the first two columns (refdir along z)
    g = d["fix_sch"][:, :2]
    n = np.sqrt(np.sum(g ** 2, axis=1))
    nz = n > 0
    assert np.array_equal(T._arrays["sch"][nz, :2], g[nz] / n[nz][:, None])


def test_fixture_tables(d):
    T = U.RotateAtom2DTables(d["fix_sig"], d["fix_sch"], np.array([0.0, 0.0, 1.0]), 2.2e-9)
    a = T._arrays
    assert (T.M, T.N, T.P) == (1776, 3, 9)
    assert np.all(a["ref_info"][:, 0] == 0) and np.all(a["ref_info"][:, 2] == 5)
    assert T.num_tables == 36 and np.all((a["ref_tab"] == -1) == (np.abs(a["ref_dirs"]).sum(axis=2) == 0))   # no line through 0
    for t in range(T.num_tables):
        x = a["kx"][a["tab_off"][t]:a["tab_off"][t + 1]]
        assert x.size >= 2 and np.all(np.diff(x) >= 0)
    assert sorted(a["pair_rows"].tolist()) == list(range(T.M))


def test_vanished_rows_take_the_pair_b0_value(d):
    T2 = U.RotateAtom2DTables(d["syn2_sig"], d["syn2_sch"], np.array([0.0, 0.0, 1.0]), 2.2e-9)
    sch, sig = d["syn2_sch"], d["syn2_sig"]
    for p, Del in enumerate(np.unique(sch[:, 4])):
        b0 = np.where((sch[:, 3] == 0) & (sch[:, 4] == Del))[0]
        assert b0.size == 2
        assert np.array_equal(T2._arrays["cst"][T2._arrays["van_const"][p]], np.mean(sig[b0, :], axis=0))
    T1 = U.RotateAtom2DTables(d["syn1_sig"], d["syn1_sch"], np.array([0.0, 0.0, 1.0]), 2.2e-9)
    for p in range(T1.P):
        c = T1._arrays["van_const"][p]
        assert c >= 0 and c in T1._arrays["row_const"]


def test_reference_side_failure_is_recorded_not_raised(d):
    errs = {e["why"]: e for e in json.loads(str(d["errors_json"]))}
    e = errs["pair without b0 rows: 4 unique"]
    T = U.RotateAtom2DTables(d[e["sig"]], d[e["sch"]], np.array(e["refdir"]), e["DIFF"])
    assert T._arrays["ref_info"][1, 0] == U.ROT2D_REF_UNIQUE and T._arrays["ref_info"][1, 1] == 4
    err = T.error_for([U.ROT2D_REF_UNIQUE, 1, 4, 0])
    assert type(err).__name__ == e["type"] and str(err) == e["msg"]


def _declared():
    src = open(os.path.join(ROOT, "include", "mfx_rot2d.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(mfx_[a-z_0-9]+)\s*\(", src)))


def test_rot2d_abi_symbols():
    lib = _lib.lib()
    assert sorted(_lib.ROT2D_EXPORTS) == _declared()
    for name in _lib.ROT2D_EXPORTS:
        assert hasattr(lib, name)
        assert name not in _lib.EXPORTS
    assert lib.mfx_rot2d_abi_version() == 1


def _create(T, **over):
    a = dict(T._arrays, **over)
    h = C.c_void_p()
    rc = _lib.lib().mfx_rot2d_create(
        _lib.dptr(a["sch"]), T.M, _lib.iptr(a["pair_off"]), _lib.iptr(a["pair_rows"]), T.P, _lib.iptr(a["ref_info"]),
        _lib.dptr(a["ref_dirs"]), _lib.iptr(a["ref_tab"]), _lib.iptr(a["row_const"]), _lib.iptr(a["van_const"]),
        _lib.dptr(a["cst"]), T.num_const, _lib.iptr(a["tab_off"]), _lib.dptr(a["kx"]), _lib.dptr(a["ky"]),
        T.num_tables, T.N, T.gamma, T.DIFF, 0, C.byref(h))
    return rc, _lib.lib().mfx_last_error().decode(), h


def test_create_checks_every_index(d):
    T = U.RotateAtom2DTables(d["syn2_sig"], d["syn2_sch"], np.array([0.0, 0.0, 1.0]), 2.2e-9)
    a = T._arrays
    bad = {"pair_off": a["pair_off"] + np.int32(1), "pair_rows": np.zeros_like(a["pair_rows"]),
           "ref_tab": a["ref_tab"] + np.int32(T.num_tables), "row_const": a["row_const"] + np.int32(T.num_const),
           "van_const": a["van_const"] + np.int32(T.num_const), "tab_off": np.zeros_like(a["tab_off"])}
    for k, v in bad.items():
        rc, msg, _ = _create(T, **{k: np.ascontiguousarray(v, dtype=np.int32)})
        assert rc == _lib.MFX_ERR_ARG, (k, msg)


def test_entry_points_without_device(d):
    lib = _lib.lib()
    T = U.RotateAtom2DTables(d["syn2_sig"], d["syn2_sch"], np.array([0.0, 0.0, 1.0]), 2.2e-9)
    dirs = np.array([[0.0, 0.0, 1.0]])
    cols = np.zeros(1, dtype=np.int32)
    out = np.zeros((1, T.M, T.N))
    st = np.zeros((1, 4), dtype=np.int32)
    rc, msg, h = _create(T)
    if lib.mfx_device_count() > 0:
        assert rc == 0
        assert lib.mfx_rot2d_rotate(h, _lib.dptr(dirs), 1, _lib.dptr(out), _lib.iptr(st)) == 0
        assert np.all(st == 0) and np.all(np.isfinite(out))
        lib.mfx_rot2d_destroy(h)
        return
    assert rc == _lib.MFX_ERR_NO_DEVICE and "no CPU path" in msg
    calls = [lambda: lib.mfx_rot2d_rotate(None, _lib.dptr(dirs), 1, _lib.dptr(out), _lib.iptr(st)),
             lambda: lib.mfx_rot2d_rotate_dev(None, None, 1, None, None, None),
             lambda: lib.mfx_rot2d_rotate_cols(None, _lib.dptr(dirs), _lib.iptr(cols), 1, _lib.dptr(out), _lib.iptr(st)),
             lambda: lib.mfx_rot2d_rotate_cols_dev(None, None, None, 1, None, None, None)]
    for c in calls:
        assert c() == _lib.MFX_ERR_NO_DEVICE
    lib.mfx_rot2d_destroy(None)
    with pytest.raises(_lib.MfxError, match="no CPU path"):
        U.rotate_atom_2Dprotocol(d["syn2_sig"], d["syn2_sch"], np.array([0.0, 0.0, 1.0]), np.array([1.0, 0.0, 0.0]),
                                 2.2e-9)
