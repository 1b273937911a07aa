"""Bootstrap conditional on measurement weights (include/mfx_wboot.h), the parts that need no GPU: the C ABI, the
restatement of the rule (tests/_wboot_ref.py) against the unweighted one for W = 1 and on its own properties, and the
argument checks of the engine's entry points and of MFModelFit.bootstrap(fixed_weights=...), which come before any
device call."""
import os
import re

import numpy as np
import pytest

import _boot_ref as R
import _wboot_ref as WR
from microstructure_fingerprinting_amd import _lib, engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 5


class NoDevicePlan:
    """Stands for an engine.Plan in the argument checks: asking it for its handle is a device call."""
    def __init__(self, M, scheme=None):
        self.M, self.scheme = M, scheme

    def handle(self):
        raise AssertionError("the device was touched before the arguments were checked")


def problem(V=5, M=37, F=2, seed=3):
    """Rows, predictions and parameter rows (two positive fascicle weights: n_act = 2) with no model behind them."""
    rng = np.random.default_rng(seed)
    P = rng.uniform(50.0, 500.0, (V, M))
    Y = P + rng.normal(0.0, 10.0, (V, M))
    params = np.zeros((V, R.num_params(F, False, False)))
    params[:, 0], params[:, 1], params[:, 2] = 400.0, 0.6, 0.4
    groups = (np.arange(M) % 4).astype(np.int32)
    groups[M - 1] = 77                                      # a group of one row
    return Y, P, params, groups


def test_wboot_abi_symbols():
    src = open(os.path.join(ROOT, "include", "mfx_wboot.h")).read()
    decl = sorted(set(re.findall(r"\b(mfx_[a-z_0-9]+)\s*\(", re.sub(r"/\*.*?\*/", "", src, flags=re.S))))
    lib = _lib.lib()
    assert sorted(_lib.WBOOT_EXPORTS) == decl and len(decl) == 7
    for name in _lib.WBOOT_EXPORTS:
        assert hasattr(lib, name)
        for other in (_lib.EXPORTS, _lib.BOOT_EXPORTS, _lib.BOOT2D_EXPORTS, _lib.WFIT_EXPORTS):
            assert name not in other
    assert lib.mfx_wboot_abi_version() == 1 and lib.mfx_boot_abi_version() == 1 and lib.mfx_wfit_abi_version() == 1
    assert lib.mfx_wboot_rep_tile() >= 1
    for f in ("wboot_resample_dev", "fit_weighted_replicates_dev", "fit_weighted_bootstrap_dev", "fit_weighted_bootstrap"):
        assert callable(getattr(engine, f))
    assert "mfx_wboot.h" in open(os.path.join(ROOT, "include", "mfx_boot.h")).read()


def test_entry_points_without_device():
    lib = _lib.lib()
    M = 16
    Y, W, pk = np.ones((1, M)), np.ones(M), np.array([[0.0, 0.0, 1.0]])
    K = np.ones(1, dtype=np.int32)
    st, ag = np.zeros(1, dtype=np.int32), np.zeros(1, dtype=np.int32)
    stats = np.zeros((1, 3, 5))
    calls = [lambda: lib.mfx_wboot_resample_dev(M, None, None, None, 0, None, 1, 0, None, None, None, -1, 4, 0, 1, 0, 0, None, None, None,
                                                None),
             lambda: lib.mfx_wboot_fit_rows_dev(None, None, None, 0, None, 1, 1, 4, None, None, None),
             lambda: lib.mfx_wboot_fit_dev(None, None, None, 0, None, 1, 0, None, None, None, None, None, 1, 4, 0, 1, 0, 0, None, 0, None, 0,
                                           0, None, None, None, None, None),
             lambda: lib.mfx_wboot_fit(None, _lib.dptr(Y), _lib.dptr(W), 0, _lib.iptr(K), None, _lib.dptr(pk), 1, 0, None, None, None, None,
                                       1, 4, 0, 1, 0, 0, None, 0, None, 0, 0, _lib.dptr(stats), _lib.iptr(ag), _lib.iptr(st), None)]
    for c in calls:
        if lib.mfx_device_count() > 0:             # with a device the null plan / the negative V is what is wrong
            assert c() == _lib.MFX_ERR_ARG
            continue
        assert c() == _lib.MFX_ERR_NO_DEVICE
        assert "no CPU path" in lib.mfx_last_error().decode()


@pytest.mark.parametrize("kind", [0, 1])
def test_unit_weights_reproduce_the_unweighted_rule(kind):
    Y, P, params, groups = problem()
    g = groups if kind == 1 else None
    for inflate in (True, False):
        want, wst = R.resample(Y, P, params, 2, False, False, 6, kind, SEED, inflate, 2 ** 32 - 9, g)
        for W in (np.ones(Y.shape), np.ones(Y.shape[1])):
            got, st = WR.resample(Y, P, W, params, 2, False, 6, kind, SEED, inflate, 2 ** 32 - 9, g)
            assert np.array_equal(got, want) and np.array_equal(st, wst) and not st.any()


@pytest.mark.parametrize("kind", [0, 1])
def test_zero_weight_rows_come_back_as_measured(kind):
    Y, P, params, groups = problem()
    rng = np.random.default_rng(8)
    W = rng.uniform(0.05, 2.0, Y.shape)
    zero = rng.random(Y.shape) < 0.3
    zero[:, -1] = False
    W[zero] = 0.0
    got, st = WR.resample(Y, P, W, params, 2, False, 7, kind, SEED, True, 0, groups if kind == 1 else None)
    assert not st.any()
    B = got.shape[1]
    assert np.array_equal(got[np.repeat(zero[:, None], B, 1)], np.repeat(Y[:, None], B, 1)[np.repeat(zero[:, None], B, 1)])
    moved = got != np.repeat(Y[:, None], B, 1)
    assert not np.any(moved & zero[:, None]) and np.mean(moved[np.repeat(~zero[:, None], B, 1)]) > 0.9
    # the scale counts the rows of positive weight: a = sqrt(M+ / (M+ - 2)), one division, one square root
    if kind == 0:
        v = 0
        Mp = int(np.count_nonzero(W[v] > 0))
        a = np.sqrt(float(Mp) / float(Mp - 2))
        r = Y[v] - P[v]
        keep = ~zero[v]
        ar = a * r
        assert np.all(((got[v, 0] == P[v] + ar) | (got[v, 0] == P[v] - ar))[keep])


def test_residual_kind_draws_only_rows_of_positive_weight():
    Y, P, params, groups = problem(V=4, M=41)
    rng = np.random.default_rng(9)
    W = rng.uniform(0.05, 2.0, Y.shape)
    zero = rng.random(Y.shape) < 0.4
    zero[:, -1] = False                                     # the group of one row keeps its row
    W[zero] = 0.0
    draws = []
    got, st = WR.resample(Y, P, W, params, 2, False, 50, 1, SEED, False, 0, groups, draws=draws)
    assert not st.any() and draws
    seen = {}
    for v, b, m, j in draws:
        assert W[v, m] > 0 and W[v, j] > 0 and groups[j] == groups[m]
        seen.setdefault((v, m), set()).add(j)
    # over 50 replicates a row of a group with n_g+ positive rows sees (nearly) all of them and never more
    for (v, m), js in seen.items():
        n_pos = int(np.count_nonzero((groups == groups[m]) & (W[v] > 0)))
        assert len(js) <= n_pos and (n_pos > 4 or len(js) == n_pos), (v, m, len(js), n_pos)
    assert seen[(0, Y.shape[1] - 1)] == {Y.shape[1] - 1}
    # in standardised units: y* = p + (s_j r_j) / s_m without the scale
    v, b, m, j = draws[0]
    assert got[v, b, m] == P[v, m] + (np.sqrt(W[v, j]) * (Y[v, j] - P[v, j])) / np.sqrt(W[v, m])


def test_status_order():
    Y, P, params, groups = problem(V=6, M=12)
    W = np.ones(Y.shape)
    W[0, 3] = -1.0; Y[0, 2] = np.nan                       # 3 before 2
    W[1] = 0.0; P[1, 0] = np.inf                            # 4 before 2
    Y[2, 5] = np.nan; W[2, 2:] = 0.0                        # 2 before 1 (M+ = 2 = n_act)
    W[3, 2:] = 0.0                                          # 1: M+ = 2 <= n_act = 2
    W[4, 7] = np.inf                                        # 3: not finite
    got, st = WR.resample(Y, P, W, params, 2, False, 3, 0, SEED, True)
    assert list(st) == [3, 4, 2, 1, 3, 0]
    assert np.all(np.isnan(got[:5])) and np.all(np.isfinite(got[5]))
    W[3, 2] = 1e-300                                        # M+ = 3 > n_act: fine, with a = sqrt(3 / 1)
    assert list(WR.resample(Y, P, W, params, 2, False, 3, 0, SEED, True)[1]) == [3, 4, 2, 0, 3, 0]
    assert WR.status_of(Y[5], P[5], np.full(12, np.nan), 2) == 3


@pytest.mark.parametrize("kind", [0, 1])
def test_a_subset_gives_the_whole_batchs_replicates(kind):
    Y, P, params, groups = problem()
    W = np.random.default_rng(4).uniform(0.1, 1.0, Y.shape)
    W[:, ::5] = 0.0
    g = groups if kind == 1 else None
    want, _ = WR.resample(Y, P, W, params, 2, False, 4, kind, SEED, True, 11, g)
    sub = np.array([3, 0, 4])
    got, _ = WR.resample(Y[sub], P[sub], W[sub], params[sub], 2, False, 4, kind, SEED, True, 11, g, vox=sub)
    assert np.array_equal(got, want[sub])
    assert not np.array_equal(WR.resample(Y[sub], P[sub], W[sub], params[sub], 2, False, 4, kind, SEED, True, 11, g)[0], want[sub])


def test_engine_argument_checks_come_before_the_device():
    M = 20
    sch = np.zeros((M, 7)); sch[:, 3] = np.repeat([0.0, 0.1, 0.2, 0.3], 5); sch[:, 4:7] = [0.03, 0.01, 0.07]
    plan = NoDevicePlan(M, sch)
    Y, W = np.ones((3, M)), np.ones((3, M))
    pk = np.tile([0.0, 0.0, 1.0, 0.0, 0.6, 0.8], (3, 1))
    K = np.array([1, 2, 0])
    base = (Y, W, K, None, pk, 2, False)
    for args, kw, exc, msg in [
            (base, dict(B=0), ValueError, "B should be an integer >= 1"),
            (base, dict(B=True), ValueError, "B should be an integer"),
            (base, dict(kind='pairs'), ValueError, "kind should be one of"),
            (base, dict(q=(0.5, 1.5)), ValueError, r"q should lie in \[0, 1\]"),
            (base, dict(seed=1.5), ValueError, "seed should be an integer"),
            (base, dict(offset=0.5), ValueError, "offset should be an integer"),
            (base, dict(B=4097), NotImplementedError, "at most 4096"),
            (base, dict(q=np.linspace(0, 1, 33)), NotImplementedError, "at most 32 bootstrap quantiles"),
            ((Y[:, :-1],) + base[1:], {}, ValueError, "protocol has 20 measurements"),
            ((Y, W[:2]) + base[2:], {}, ValueError, "weights should have shape"),
            ((Y, np.ones(M - 1)) + base[2:], {}, ValueError, "weights should have shape"),
            ((Y, W, K[:2]) + base[3:], {}, ValueError, "K should have one entry"),
            ((Y, W, np.array([1, 2, 3])) + base[3:], {}, ValueError, "K should lie in"),
            ((Y, W, K, np.array([1, 0, 0]), pk, 2, False), {}, ValueError, "flagged CSF need csf_on"),
            ((Y, W, K, None, pk[:, :3], 2, False), {}, ValueError, "peaks should have shape"),
            ((Y, W, K, None, pk, 2, True), {}, ValueError, "csf_on needs sig_csf"),
            ((Y, W, K, None, np.tile(pk, (1, 2)), 4, False), {}, ValueError, "not served for maxfasc = 4"),
            (base, dict(params=np.zeros((3, 6))), ValueError, r"params should have shape \(3, 7\)"),
            (base, dict(vox=np.arange(2)), ValueError, "vox should have one entry"),
            (base, dict(props=np.ones((2, 5, 1))), ValueError, "props should have shape"),
            (base, dict(kind='residual', groups=np.zeros(M - 1, dtype=int)), ValueError, "groups should be 20 integers")]:
        with pytest.raises(exc, match=msg):
            engine.fit_weighted_bootstrap(plan, *args, **kw)
    with pytest.raises(ValueError, match="knows no scheme"):
        engine.fit_weighted_bootstrap(NoDevicePlan(M), *base, kind='residual')


def test_device_entry_points_check_their_arguments_first():
    torch = pytest.importorskip("torch")

    class Fake:
        """Stands for a CUDA float64 tensor in the checks: asking it for its pointer is a device call."""
        is_cuda, dtype, device = True, torch.float64, None

        def __init__(self, *shape):
            self.shape = tuple(shape)

        def is_contiguous(self):
            return True

        def dim(self):
            return len(self.shape)

        def data_ptr(self):
            raise AssertionError("the device was touched before the arguments were checked")
    M = 20
    plan = NoDevicePlan(M)
    Y, P, W, par, pk = Fake(3, M), Fake(3, M), Fake(3, M), Fake(3, 7), Fake(3, 6)
    for args, kw, msg in [((Y, P, W, par, 2), dict(B=0), "B should be an integer >= 1"),
                          ((Y, P, W, par, 2), dict(kind='x'), "kind should be one of"),
                          ((Y, P, W, par, 4), {}, "maxfasc must be 0..3"),
                          ((Y, Fake(3, M - 1), W, par, 2), {}, "prediction should have the data's shape"),
                          ((Y, P, Fake(2, M), par, 2), {}, "weights should have shape"),
                          ((Y, P, W, Fake(3, 8), 2), {}, "params should have shape"),
                          ((Y, P, W, par, 2), dict(d_peaks=Fake(3, 3)), "peaks should have shape"),
                          ((Y, P, W, par, 2), dict(kind='residual'), "needs groups")]:
        with pytest.raises(ValueError, match=msg):
            engine.wboot_resample_dev(*args, **kw)
    for args, msg in [((Fake(3, M), W, pk, 2), "replicate signals should have shape"),
                      ((Fake(3, 4, M - 1), W, pk, 2), "protocol has 20 measurements"),
                      ((Fake(3, 4, M), Fake(M + 1), pk, 2), "weights should have shape"),
                      ((Fake(3, 4, M), W, Fake(3, 3), 2), "peaks should have shape"),
                      ((Fake(3, 4, M), W, Fake(3, 12), 4), "not served for maxfasc = 4")]:
        with pytest.raises(ValueError, match=msg):
            engine.fit_weighted_replicates_dev(plan, *args)
    for args, kw, exc, msg in [((Y, W, pk, 2), dict(B=4097), NotImplementedError, "at most 4096"),
                               ((Y, W, pk, 2), dict(q=(2.0,)), ValueError, "q should lie in"),
                               ((Fake(3, M + 1), W, pk, 2), {}, ValueError, "protocol has 20 measurements"),
                               ((Y, Fake(M - 1), pk, 2), {}, ValueError, "weights should have shape"),
                               ((Y, W, Fake(3, 3), 2), {}, ValueError, "peaks should have shape"),
                               ((Y, W, pk, 2), dict(csf_on=True), ValueError, "csf_on needs sig_csf"),
                               ((Y, W, pk, 2), dict(d_params=Fake(3, 6)), ValueError, "params should have shape"),
                               ((Y, W, pk, 2), dict(d_pred=Fake(3, M)), ValueError, "a prediction needs the parameters"),
                               ((Y, W, pk, 2), dict(kind='residual'), ValueError, "needs groups")]:
        with pytest.raises(exc, match=msg):
            engine.fit_weighted_bootstrap_dev(plan, *args, **kw)


def test_mfmodelfit_fixed_weights_checks_come_before_the_device():
    import microstructure_fingerprinting_amd as mf
    from microstructure_fingerprinting_amd.mf import MFModelFit
    d, sch, _, _ = R.golden_model()
    M = sch.shape[0]
    model = mf.MFModel({"dictionary": d["dictionary"], "sch_mat": d["sch_ms"], "orientation": R.Z, "num_atom": int(d["N"]),
                        "num_ear": int(d["E"]), "T2_csf": float(d["T2_csf"]), "DIFF_csf": float(d["DIFF_csf"]),
                        "T2_ear": float(d["T2_ear"]), "DIFF_ear": d["DIFF_ear"], "fasc_propnames": ["rad ", "fin"],
                        "rad": d["rad"], "fin": d["fin"]})
    mask = np.ones((2, 2)); mask[0, 0] = 0

    def fit_object(**extra):
        info = {'maxfasc': 1, 'csf_on': False, 'ear_on': False, 'affine': None, 'mask': mask, 'fasc_propnames': ['rad', 'fin'],
                'peaks_roi': np.tile([0.0, 0.0, 1.0], (3, 1)), 'roi_index': np.flatnonzero(mask.reshape(-1) > 0), 'model': model,
                'pgse_scheme': sch, 'numfasc_roi': np.ones(3, dtype=int), 'csf_roi': np.zeros(3, bool), 'ear_roi': np.zeros(3, bool),
                '_dict_rad': d['rad'], '_dict_fin': d['fin']}
        info.update(extra)
        P = np.zeros((3, 5)); P[:, 0] = 100.0; P[:, 1] = 1.0
        return MFModelFit(info, P)
    data = np.ones((2, 2, M))
    robust = dict(weights_roi=np.ones((3, M)), robust_base=None, robust_options={}, robust_info={'scale': np.ones(3)})
    with pytest.raises(ValueError, match="fixed_weights=True needs a fit made with weights= or robust="):
        fit_object().bootstrap(data, B=4, fixed_weights=True)
    for extra in (dict(weights_roi=np.ones(M)), robust):
        fit = fit_object(**extra)
        with pytest.raises(NotImplementedError, match="bootstrap of a weighted or robust fit is not served"):
            fit.bootstrap(data, B=4)                        # the default did not change
        with pytest.raises(NotImplementedError, match="bootstrap of a weighted or robust fit is not served"):
            fit.bootstrap(data, B=4, fixed_weights=False)
        with pytest.raises(ValueError, match="fixed_weights should be True or False"):
            fit.bootstrap(data, B=4, fixed_weights=1)
        with pytest.raises(TypeError):
            fit.bootstrap(data, 4, 'wild', True)            # keyword only
        for kw, exc, msg in [(dict(B=0), ValueError, "B should be an integer >= 1"), (dict(kind='block'), ValueError, "kind should be one of"),
                             (dict(q=(0.1, 2.0)), ValueError, "q should lie in"), (dict(B=4097), NotImplementedError, "at most 4096"),
                             (dict(voxels=[3]), ValueError, "positions in the ROI"),
                             (dict(kind='residual', groups=np.zeros(3, dtype=int)), ValueError, "groups should be %d integers" % M)]:
            with pytest.raises(exc, match=msg):
                fit.bootstrap(data, fixed_weights=True, **kw)
        with pytest.raises(ValueError, match="data should have shape"):
            fit.bootstrap(data[..., :-1], B=4, fixed_weights=True)
    doc = " ".join(MFModelFit.bootstrap.__doc__.lower().split())
    assert "conditional on the rows that were rejected" in doc
    assert model.ms_interpolator._tables is None        # nothing was created on a device
    if _lib.lib().mfx_device_count() == 0:              # valid arguments get as far as the device, and no further
        for extra in (dict(weights_roi=np.ones(M)), robust):
            with pytest.raises(_lib.MfxError, match="no CPU path"):
                fit_object(**extra).bootstrap(data, B=4, fixed_weights=True)
