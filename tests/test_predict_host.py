"""Forward model, host side: the C ABI of include/mfx_predict.h, gen_SoS_MRI's argument handling (the message of
its ValueError was recorded by running the reference: tests/golden/gen_golden_predict.py) and the argument errors of
engine.predict that are raised before any device call.  No GPU needed."""
import os
import re

import numpy as np
import pytest

import microstructure_fingerprinting_amd as mf
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
    decl = _declared("mfx_predict.h")
    assert decl == sorted(_lib.PREDICT_EXPORTS)
    for name in decl:
        assert hasattr(lib, name), "libmfx.so lacks %s declared in include/mfx_predict.h" % name
    assert lib.mfx_predict_abi_version() == 1
    # mfx.h, its binding list and its version are as they were
    assert _declared("mfx.h") == sorted(_lib.EXPORTS)
    assert not set(_lib.PREDICT_EXPORTS) & set(_lib.EXPORTS)
    assert lib.mfx_abi_version() == 3


def test_gen_SoS_MRI_is_exported():
    assert "gen_SoS_MRI" in U.__all__
    assert mf.mf_utils.gen_SoS_MRI is U.gen_SoS_MRI


@pytest.mark.parametrize("N", [1, 4])
def test_gen_SoS_MRI_without_noise_returns_sqrtN_S0(N):
    S0 = np.array([[1.0, -2.0, 0.0], [3.5, 4.0, 1e-3]])
    for sg in (0, 0.0, np.zeros(S0.shape), np.zeros((1, 1))):
        out = U.gen_SoS_MRI(S0, sg, N)
        assert out.shape == S0.shape and np.array_equal(out, np.sqrt(N) * S0)
    assert U.gen_SoS_MRI(2.0, 0, N) == np.sqrt(N) * 2.0


def test_gen_SoS_MRI_shape_mismatch_has_the_reference_message():
    d = np.load(os.path.join(G, "predict_cases.npz"))
    with pytest.raises(ValueError) as ei:
        U.gen_SoS_MRI(np.ones((3, 4)), np.ones((4, 3)), 1)
    assert str(ei.value) == str(d["sos_shape_error"])


def test_gen_SoS_MRI_refuses_complex_input():
    with pytest.raises(TypeError, match="real"):
        U.gen_SoS_MRI(np.ones(4) + 1j * np.ones(4), 0.1)
    with pytest.raises(TypeError, match="real"):
        U.gen_SoS_MRI(np.ones(4, dtype=np.complex64), 0.0)


def test_noisy_call_without_a_device_fails_loudly():
    if _lib.lib().mfx_device_count() > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(_lib.MfxError):
        U.gen_SoS_MRI(np.ones((2, 5)), 0.1, 2, seed=7)
    with pytest.raises(_lib.MfxError):
        engine.sos_noise(np.ones(8), np.full(8, 0.5), 1, seed=1)


def test_seed_none_draws_from_numpys_global_stream():
    np.random.seed(1234)
    a = [U._sos_seed(None) for _ in range(3)]
    np.random.seed(1234)
    b = [U._sos_seed(None) for _ in range(3)]
    assert a == b and len(set(a)) == 3 and all(0 <= s < 2 ** 64 for s in a)
    assert U._sos_seed(5) == 5 and U._sos_seed(-1) == 2 ** 64 - 1


class _Plan:
    """Stands for an engine.Plan of M rows; the argument checks must be done before its handle is asked for."""
    M = 64

    def handle(self):
        raise AssertionError("the device plan was touched before the arguments were checked")


def test_engine_predict_argument_errors():
    P = _Plan()
    V = 5
    ok = np.zeros((V, engine.num_params(2, True, False)))
    pk = np.zeros((V, 6))
    csf = np.ones(64)
    with pytest.raises(ValueError, match="params should have 8 columns"):
        engine.predict(P, np.zeros((V, 7)), pk, 2, True, False, csf)
    with pytest.raises(ValueError, match="params should have"):
        engine.predict(P, np.zeros(8), pk, 2, True, False, csf)
    with pytest.raises(ValueError, match=r"peaks should have shape \(5, 6\)"):
        engine.predict(P, ok, np.zeros((V, 3)), 2, True, False, csf)
    with pytest.raises(ValueError, match=r"peaks should have shape \(5, 6\)"):
        engine.predict(P, ok, np.zeros((V + 1, 6)), 2, True, False, csf)
    with pytest.raises(ValueError, match="protocol has 64"):
        engine.predict(P, ok, pk, 2, True, False, csf, Y=np.zeros((V, 63)))
    with pytest.raises(ValueError, match="protocol has 64"):
        engine.predict(P, ok, pk, 2, True, False, np.ones(60))
    with pytest.raises(ValueError, match="sig_ear"):
        engine.predict(P, np.zeros((V, 9)), pk, 2, False, True, None, np.ones((63, 3)), 3)
    with pytest.raises(ValueError, match="maxfasc"):
        engine.predict(P, ok, pk, 4, True, False, csf)
    with pytest.raises(ValueError, match="sigma_g"):
        engine.predict(P, ok, pk, 2, True, False, csf, ncoils=1)
    with pytest.raises(ValueError, match="sigma_g should be a scalar"):
        engine.predict(P, ok, pk, 2, True, False, csf, sigma_g=np.ones(V + 1), ncoils=1)
