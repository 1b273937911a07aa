"""mf.mcf on the host: generated eigenvalue / coupling tables against the reference's MCF_data files,
the reference's validation (exception types and messages recorded in tests/golden/mcf_cases.npz by
gen_golden_mcf.py), and the C ABI of include/mfx_mcf.h.  No GPU needed."""
import json
import os
import re

import numpy as np
import pytest

import microstructure_fingerprinting_amd as mf
from microstructure_fingerprinting_amd import _lib
from microstructure_fingerprinting_amd import mcf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def d():
    return np.load(os.path.join(G, "mcf_cases.npz"))


def test_mcf_is_exported():
    assert mf.mcf is mcf
    for name in ("import_DDE_scheme", "MCF_PGSE", "MCF_DDE", "MCF_PGSE_atoms", "mcf_tables"):
        assert callable(getattr(mf.mcf, name))


@pytest.mark.parametrize("M", [60, 20, 1])
def test_cylinder_tables_match_reference_files(d, M):
    lam, B = mcf.mcf_tables('cylinder', M)
    lref, Bref = d["Lcl"][:M], d["Bcl"][:M, :M]
    assert lam.shape == (M,) and B.shape == (M, M)
    assert lam[0] == 0.0 and np.all(np.diff(lam) > 0)
    assert np.all(np.abs(lam - lref) <= 1e-8 * np.abs(lref))
    assert np.max(np.abs(B - Bref)) <= 2e-6
    assert np.array_equal(B != 0, Bref != 0)
    assert np.all(B >= 0) and np.array_equal(B, B.T)


def test_sphere_and_planes_eigenvalues(d):
    lam_s, B_s = mcf.mcf_tables('sphere')
    lam_p, _ = mcf.mcf_tables('p')
    assert B_s is None
    assert np.all(np.abs(lam_s - d["Lsl"]) <= 1e-8 * np.maximum(np.abs(d["Lsl"]), 1e-300))
    assert np.all(np.abs(lam_p - d["Lpl"]) <= 1e-8 * np.maximum(np.abs(d["Lpl"]), 1e-300))
    assert abs(mcf.mcf_tables('c')[0][59] - 405.784) < 1e-3
    assert abs(lam_s[59] - 422.690) < 1e-3
    assert lam_p[59] == (59 * np.pi) ** 2


def test_tables_are_cached_and_read_only():
    a = mcf.mcf_tables('c', 30)
    assert mcf.mcf_tables('cylinder', 30)[1] is a[1]
    with pytest.raises(ValueError):
        a[0][0] = 1.0
    with pytest.raises(ValueError, match="Unknown domain"):
        mcf.mcf_tables('torus')


def _resolve(kw, d):
    named = {"sch_ukbb_2": d["sch_ukbb"][:2], "dde_2": d["sch_dde"][:2], "a_list": [1.0, 2.0]}
    out = dict(kw)
    for k, v in kw.items():
        if isinstance(v, str) and v in named:
            out[k] = named[v]
        elif isinstance(v, list):
            out[k] = np.array(v, dtype=float)
    return out


def _error_cases():
    dd = np.load(os.path.join(G, "mcf_cases.npz"))
    return [tuple(e) for e in json.loads(str(dd["errors_json"])) if e[2] is not None]


@pytest.mark.parametrize("fn,kw,etype,msg", _error_cases())
def test_validation_matches_reference(d, fn, kw, etype, msg):
    """Raised before any launch, so the same on a machine without a GPU."""
    with pytest.raises(Exception) as ei:
        getattr(mf.mcf, fn)(**_resolve(kw, d))
    assert type(ei.value).__name__ == etype
    assert str(ei.value) == msg


def test_error_cases_cover_every_branch(d):
    errs = [e for e in json.loads(str(d["errors_json"])) if e[2] is not None]
    kinds = {e[2] for e in errs}
    assert kinds == {"ValueError", "RuntimeError", "NotImplementedError", "TypeError"}
    assert sum("too small to ensure accuracy" in e[3] for e in errs) == 4


def test_no_gradient_rows_on_other_domains(d):
    # the reference returns ones for a sphere when no row has a gradient (its loop never reaches the domain)
    E = mf.mcf.MCF_PGSE('sphere', 2e-6, 2e-9, G=[0.0, 0.0], Delta=[0.03, 0.03], delta=[0.01, 0.01])
    assert np.array_equal(E, d["sphere_nograd"])
    with pytest.raises(NotImplementedError):
        mf.mcf.MCF_PGSE_atoms('s', [1e-6, 2e-6], [2e-9, 2e-9], scheme=d["sch_ukbb"])


def test_atoms_argument_shapes(d):
    with pytest.raises(ValueError, match="same length"):
        mf.mcf.MCF_PGSE_atoms('c', [1e-6, 2e-6], [2e-9], scheme=d["sch_ukbb"])
    with pytest.raises(ValueError, match="too small to ensure accuracy"):   # any atom failing the q/p check
        mf.mcf.MCF_PGSE_atoms('c', [1e-6, 40e-6], [2e-9, 0.5e-9], scheme=d["sch_ukbb"])


def _declared():
    src = open(os.path.join(ROOT, "include", "mfx_mcf.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(mfx_[a-z_0-9]+)\s*\(", src)))


def test_mcf_abi_symbols():
    lib = _lib.lib()
    assert sorted(_lib.MCF_EXPORTS) == _declared()
    for name in _lib.MCF_EXPORTS:
        assert hasattr(lib, name)
        assert name not in _lib.EXPORTS
    assert lib.mfx_mcf_abi_version() == 1


def _call(fn, seq, L=(2e-6,), D=(2e-9,), M=60, env=(0.0, 0.0, 1.0)):
    lib = _lib.lib()
    lam, B = mcf.mcf_tables('c', 60)
    lam, B = _lib.f64c(lam), _lib.f64c(B)
    seq, L, D, env = _lib.f64c(seq), _lib.f64c(L), _lib.f64c(D), _lib.f64c(env)
    E = np.full((seq.shape[0], L.size), -1.0)
    rc = getattr(lib, fn)(_lib.dptr(lam), _lib.dptr(B), M, _lib.dptr(seq), seq.shape[0], _lib.dptr(L), _lib.dptr(D),
                          L.size, _lib.dptr(env), 2.675e8, _lib.dptr(E))
    return rc, lib.mfx_last_error().decode(), E


def test_mcf_abi_argument_errors_and_device():
    seq7 = np.array([[1.0, 0.0, 0.0, 0.0, 0.03, 0.01, 0.05]])
    seq14 = np.zeros((1, 14))
    for fn, seq in (("mfx_mcf_pgse", seq7), ("mfx_mcf_dde", seq14)):
        rc, msg, _ = _call(fn, seq, M=65)
        assert rc == _lib.MFX_ERR_ARG and "M <=" in msg
        rc, msg, _ = _call(fn, seq, L=(-1e-6,))
        assert rc == _lib.MFX_ERR_ARG and "positive" in msg
        rc, msg, _ = _call(fn, seq, env=(0.0, 0.0, 0.0))
        assert rc == _lib.MFX_ERR_ARG and "envdir" in msg
        rc, msg, E = _call(fn, seq)
        if _lib.lib().mfx_device_count() < 1:
            assert rc == _lib.MFX_ERR_NO_DEVICE and "no CPU path" in msg
            with pytest.raises(_lib.MfxError):
                _lib.check(rc)
        else:
            assert rc == 0 and np.array_equal(E, np.ones((1, 1)))   # a row without gradient


def test_public_api_without_device_raises():
    if _lib.lib().mfx_device_count() > 0:
        E = mf.mcf.MCF_PGSE('c', 2e-6, 2e-9, G=[0.05], Delta=[0.03], delta=[0.01])
        assert E.shape == (1,) and 0.0 < E[0] < 1.0
        return
    with pytest.raises(_lib.MfxError, match="no CPU path"):
        mf.mcf.MCF_PGSE('c', 2e-6, 2e-9, G=[0.05], Delta=[0.03], delta=[0.01])
