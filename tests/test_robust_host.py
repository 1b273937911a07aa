"""Robust fits (include/mfx_robust.h), the parts that need no GPU: the C ABI, the NumPy statement of the weight rule
(tests/_robust_ref.py, the referee of tests/test_robust_gpu.py) on hand-computed cases, the argument checks that come
before any device call, and robust=None / False taking the path that was there."""
import os
import re

import numpy as np
import pytest

import _robust_ref as RR
from microstructure_fingerprinting_amd import _lib, engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
Z = np.array([0.0, 0.0, 1.0])


class NoDevicePlan:
    """Stands for an engine.Plan in the argument checks: asking it for its handle is a device call."""
    def __init__(self, M):
        self.M = M

    def handle(self):
        raise AssertionError("the device was touched before the arguments were checked")


def _declared():
    src = open(os.path.join(ROOT, "include", "mfx_robust.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(mfx_[a-z_0-9]+)\s*\(", src)))


def test_robust_abi_symbols():
    lib = _lib.lib()
    assert sorted(_lib.ROBUST_EXPORTS) == _declared()
    for name in _lib.ROBUST_EXPORTS:
        assert hasattr(lib, name)
        assert name not in _lib.EXPORTS and name not in _lib.WFIT_EXPORTS
    assert lib.mfx_robust_abi_version() == 1
    assert lib.mfx_abi_version() == 3 and lib.mfx_wfit_abi_version() == 1      # the other headers keep their versions
    assert engine.ROBUST_LOSSES == {"cutoff": 0, "huber": 1, "tukey": 2}
    for f in (engine.robust_weights_dev, engine.robust_weights, engine.fit_robust_dev, engine.fit_robust):
        assert callable(f)


def test_entry_points_without_device():
    lib = _lib.lib()
    M = 16
    Y, pk = np.ones((1, M)), np.array([[0.0, 0.0, 1.0]])
    K = np.ones(1, dtype=np.int32)
    prm, W, sc = np.zeros((1, 5)), np.zeros((1, M)), np.zeros(1)
    st, stt, used = np.zeros(1, dtype=np.int32), np.zeros(1, dtype=np.int32), np.zeros(1, dtype=np.int32)
    nch = np.zeros(2, dtype=np.int64)

    def host(maxfasc=1, c=4.45):
        return lib.mfx_rfit_batch(None, _lib.dptr(Y), None, 0, _lib.iptr(K), None, _lib.dptr(pk), maxfasc, 0, None, 0, c, 2, 1,
                                  _lib.dptr(prm), _lib.dptr(W), _lib.dptr(sc), _lib.iptr(stt), _lib.iptr(st), _lib.lptr(nch),
                                  _lib.iptr(used))
    calls = [lambda: lib.mfx_robust_weights_dev(M, None, None, None, 0, 0, 4.45, 1, None, None, None, None, None, None),
             lambda: lib.mfx_rfit_batch_dev(None, None, None, 0, None, 1, 0, 4.45, 1, 1, None, None, None, None, None, None, None),
             host, lambda: host(maxfasc=4), lambda: host(c=0.5)]
    for c in calls:
        if lib.mfx_device_count() > 0:             # with a device the null pointers are what is wrong
            assert c() == _lib.MFX_ERR_ARG or c() == _lib.MFX_ERR_UNSUPPORTED
            continue
        assert c() == _lib.MFX_ERR_NO_DEVICE
        assert "no CPU path" in lib.mfx_last_error().decode()


# ---- the rule, by hand
def _losses():
    """The referee's loss names are the engine's, in the order of their codes."""
    names = tuple(sorted(engine.ROBUST_LOSSES, key=engine.ROBUST_LOSSES.get))
    assert names == RR.LOSSES
    return names


def test_rule_odd_even_and_losses():
    assert _losses() == ("cutoff", "huber", "tukey")
    y = np.array([10.0, 10.0, 10.0, 10.0, 10.0])
    p = np.array([9.0, 12.0, 10.5, 6.0, 13.0])            # a = 1, 2, 0.5, 4, 3 -> odd n0: median 2
    W, s, st = RR.rule_one(y, p, None, "cutoff", 1.0)
    assert (s, st) == (2.0, 0) and np.array_equal(W, [1, 1, 1, 0, 0])
    W, s, st = RR.rule_one(y, p, None, "cutoff", 1.5)     # thr 3
    assert np.array_equal(W, [1, 1, 1, 0, 1])
    W, s, st = RR.rule_one(y, p, None, "huber", 1.0)      # thr 2: 1, 1, 1, 2/4, 2/3
    assert np.array_equal(W, [1.0, 1.0, 1.0, 0.5, 2.0 / 3.0])
    W, s, st = RR.rule_one(y, p, None, "tukey", 2.0)      # thr 4: u = .25, .5, .125, 1, .75
    u = np.array([0.25, 0.5, 0.125, 1.0, 0.75])
    assert np.array_equal(W, np.where(u < 1, (1 - u * u) * (1 - u * u), 0.0)) and W[3] == 0.0 and W[0] == 0.87890625
    # base weights: row 1 is out for good, n0 = 4 (even): a over B = 1, 0.5, 4, 3 -> median (1 + 3) / 2 = 2
    w0 = np.array([2.0, 0.0, 0.5, 1.0, 4.0])
    W, s, st = RR.rule_one(y, p, w0, "cutoff", 1.0)
    assert (s, st) == (2.0, 0) and np.array_equal(W, [2.0, 0.0, 0.5, 0.0, 0.0])
    W, s, st = RR.rule_one(y, p, w0, "huber", 1.0)
    assert np.array_equal(W, [2.0, 0.0, 0.5, 0.5, 4.0 * (2.0 / 3.0)])
    # even n0, the two roundings of the mean: a = 0.1, 0.2, 0.3, 0.7 -> fl(fl(0.2 + 0.3) / 2)
    y4, p4 = np.zeros(4), np.array([0.1, -0.3, 0.7, 0.2])
    W, s, st = RR.rule_one(y4, p4, None, "cutoff", 1.0)
    assert s == (0.2 + 0.3) / 2.0 and np.array_equal(W, [1, 0, 0, 1])
    assert RR.rule_one(np.array([3.0]), np.array([1.0]), None, "cutoff", 1.0)[1] == 2.0          # M = 1


def test_rule_ties_do_not_matter():
    rng = np.random.default_rng(5)
    for n in (2, 3, 6, 7, 62, 63):
        for _ in range(20):
            a = rng.integers(0, 3, n).astype(np.float64) * 0.1        # few distinct values: ties straddle the median
            assert RR.median_by_order(a) == np.median(a)
            assert RR.median_by_order(a[::-1]) == np.median(a)
    a = np.full(9, 0.3)
    W, s, st = RR.rule_one(a, np.zeros(9), None, "cutoff", 1.0)       # all residuals equal: everything is kept at c = 1
    assert s == 0.3 and st == 0 and np.all(W == 1)
    # c >= 1 keeps at least ceil(n0 / 2) rows
    for n in (1, 2, 5, 8):
        y = rng.normal(size=n)
        for loss in _losses()[:2]:
            W, s, st = RR.rule_one(y, np.zeros(n), None, loss, 1.0)
            assert st == 0 and np.count_nonzero(W > 0) >= (n + 1) // 2


def test_rule_states():
    assert len(_losses()) == 3
    y, p = np.arange(6.0), np.zeros(6)
    W, s, st = RR.rule_one(y, np.full(6, np.nan), None, "cutoff", 4.45)
    assert st == 1 and np.isnan(s) and np.all(W == 1)
    w0 = np.array([1.0, 0.0, 1.0, 1.0, 1.0, 1.0])
    pn = p.copy(); pn[1] = np.nan                          # a NaN outside B is not looked at
    assert RR.rule_one(y, pn, w0, "cutoff", 4.45)[2] == 0
    W, s, st = RR.rule_one(y, np.array([0, 1, 2, 3, 9.0, 9.0]), None, "tukey", 4.45)     # four of six fitted exactly
    assert st == 2 and s == 0.0 and np.all(W == 1)
    for bad in (np.array([1, -1e-3, 1, 1, 1, 1.0]), np.array([1, np.inf, 1, 1, 1, 1.0]), np.array([1, np.nan, 1, 1, 1, 1.0]),
                np.zeros(6)):
        W, s, st = RR.rule_one(y, p, bad, "huber", 4.45)
        assert st == 3 and np.isnan(s) and np.array_equal(W, bad, equal_nan=True)
    W, sc, stt, ch = RR.weights_ref(np.stack([y, y]), np.stack([p, np.full(6, np.nan)]), None, "cutoff", 1.0, Wprev=np.ones((2, 6)))
    assert np.array_equal(stt, [0, 1]) and np.array_equal(ch, [1, 0])


# ---- argument errors, all before the device
def test_engine_argument_checks_come_before_the_device():
    M = 20
    plan = NoDevicePlan(M)
    Y = np.ones((3, M))
    pk = np.tile([0.0, 0.0, 1.0, 0.0, 0.6, 0.8], (3, 1))
    K = np.array([1, 2, 0])
    sc = np.ones(M)
    ok = (Y, K, None, pk, 2, False)
    for args, kw, msg in [(ok, dict(c=0.99), "c should be a finite number >= 1"),
                          (ok, dict(c=np.nan), "c should be a finite number >= 1"),
                          (ok, dict(c="a"), "c should be a finite number >= 1"),
                          (ok, dict(loss="l2"), "loss should be one of 'cutoff', 'huber', 'tukey'"),
                          (ok, dict(loss=0), "loss should be one of"),
                          (ok, dict(n_iter=-1), "n_iter should be a non-negative integer"),
                          (ok, dict(n_iter=1.5), "n_iter should be a non-negative integer"),
                          ((Y[:, :-1], K, None, pk, 2, False), {}, "measurements"),
                          (ok, dict(W0=np.ones((3, M - 1))), r"weights should have shape .*\(3 voxels\)"),
                          (ok, dict(W0=np.ones((2, M))), "weights should have shape"),
                          (ok, dict(W0=np.ones(M + 1)), "weights should have shape"),
                          ((Y, K, None, pk[:, :3], 2, False), {}, "peaks should have shape"),
                          ((Y, K[:2], None, pk, 2, False), {}, "K should have one entry"),
                          ((Y, np.array([1, 2, 3]), None, pk, 2, False), {}, "K should lie in"),
                          ((Y, K, np.array([1, 0, 0]), pk, 2, False, sc), {}, "need csf_on"),
                          ((Y, K, np.array([1, 0, 0]), pk, 2, True), {}, "need csf_on and sig_csf"),
                          ((Y, K, np.array([1, 0]), pk, 2, True, sc), {}, "csf should have one entry"),
                          ((Y, K, None, np.tile(pk, (1, 2)), 4, False), {}, "not served for maxfasc = 4"),
                          (ok, dict(ear=np.array([0, 1, 0])), "not served for voxels with an EAR")]:
        with pytest.raises(ValueError, match=msg):
            engine.fit_robust(plan, *args, **kw)
    P = np.zeros((3, M))
    for args, kw, msg in [((Y, P), dict(c=0.5), "c should be a finite number >= 1"),
                          ((Y, P), dict(loss="bisquare"), "loss should be one of"),
                          ((Y, P[:, :-1]), {}, "prediction should have the data's shape"),
                          ((Y, P[:2]), {}, "prediction should have the data's shape"),
                          ((Y, P, np.ones((3, M + 1))), {}, "base weights should have shape"),
                          ((Y, P, np.ones(M - 1)), {}, "base weights should have shape"),
                          ((Y, P), dict(Wprev=np.ones((2, M))), "previous weights should have shape"),
                          ((np.ones(M), np.ones(M)), {}, "data should have shape")]:
        with pytest.raises(ValueError, match=msg):
            engine.robust_weights(*args, **kw)
    for r, msg in [("yes", "robust should be None, a bool or a dict"), ({"cc": 3}, "unknown key.*'cc'"),
                   ({"c": 0.2}, "c should be a finite number >= 1"), ({"loss": "L1"}, "loss should be one of"),
                   ({"n_iter": -2}, "n_iter should be a non-negative integer")]:
        with pytest.raises(ValueError, match=msg):
            engine.robust_options(r)
    assert engine.robust_options(None) is None and engine.robust_options(False) is None
    assert engine.robust_options(True) == {"loss": "cutoff", "c": 4.45, "n_iter": 3}
    assert engine.robust_options({"n_iter": 1, "loss": "tukey"}) == {"loss": "tukey", "c": 4.45, "n_iter": 1}


def _model():
    import microstructure_fingerprinting_amd as mf
    d = np.load(os.path.join(G, "fit_cases.npz"))
    model = mf.MFModel({"dictionary": d["dictionary"], "sch_mat": d["sch_ms"], "orientation": Z, "num_atom": int(d["N"]),
                        "num_ear": int(d["E"]), "T2_csf": float(d["T2_csf"]), "DIFF_csf": float(d["DIFF_csf"]),
                        "T2_ear": float(d["T2_ear"]), "DIFF_ear": d["DIFF_ear"], "fasc_propnames": ["rad ", "fin"],
                        "rad": d["rad"], "fin": d["fin"]})
    M = d["sch"].shape[0]
    data = np.ones((2, 3, M)); mask = np.ones((2, 3)); mask[0, 0] = 0
    pk = np.tile([0, 0, 1.0, 1, 0, 0], (2, 3, 1))
    return model, data, mask, dict(peaks=pk, pgse_scheme=d["sch"], verbose=0), M


def test_mfmodel_robust_checks_come_before_the_device():
    model, data, mask, kw, M = _model()
    for r, msg in [({"c": 0.5}, "c should be a finite number >= 1"), ({"loss": "lorentz"}, "loss should be one of"),
                   ({"n_iter": -1}, "n_iter should be a non-negative integer"), (3, "robust should be None, a bool or a dict")]:
        with pytest.raises(ValueError, match=msg):
            model.fit(data, mask, 1, robust=r, **kw)
    for r in (True, {"n_iter": 1}):                       # the ValueError of weights with ear_mask, with and without weights
        with pytest.raises(ValueError, match="not served together with ear_mask: 5 of 5 voxel"):
            model.fit(data, mask, 1, robust=r, ear_mask=np.ones((2, 3)), **kw)
        with pytest.raises(ValueError, match="not served together with ear_mask: 5 of 5 voxel"):
            model.fit(data, mask, 1, robust=r, weights=np.ones(M), ear_mask=np.ones((2, 3)), **kw)
    with pytest.raises(ValueError, match="without a positive weight"):
        model.fit(data, mask, 1, robust=True, weights=np.zeros(M), **kw)
    with pytest.raises(TypeError):
        model.fit(data, mask, 1, True, **kw)            # keyword only
    assert model.ms_interpolator._tables is None        # nothing was created on a device
    if _lib.lib().mfx_device_count() == 0:              # a valid request gets as far as the device, and no further
        with pytest.raises(_lib.MfxError, match="no CPU path"):
            model.fit(data, mask, 1, robust=True, **kw)


@pytest.mark.parametrize("robust", [None, False])
def test_robust_off_is_the_existing_path(monkeypatch, robust):
    """robust=None / False never reach engine.fit_robust: the plain fit goes to fit_batch, the weighted one to
    fit_weighted, with the arguments they get without the keyword."""
    model, data, mask, kw, M = _model()
    seen = []

    class Reached(Exception):
        pass

    def sentinel(*a, **k):
        raise AssertionError("engine.fit_robust was reached with robust=%r" % (robust,))

    def plain(plan, Y, *a, **k):
        seen.append(("fit_batch", len(a), sorted(k)))
        raise Reached

    def weighted(plan, Y, W, *a, **k):
        seen.append(("fit_weighted", W.shape))
        raise Reached
    monkeypatch.setattr(engine, "fit_robust", sentinel)
    monkeypatch.setattr(engine, "fit_batch", plain)
    monkeypatch.setattr(engine, "fit_weighted", weighted)
    monkeypatch.setattr(type(model.ms_interpolator), "plan_for", lambda self, sch: NoDevicePlan(sch.shape[0]))
    with pytest.raises(Reached):
        model.fit(data, mask, 1, robust=robust, **kw)
    with pytest.raises(Reached):
        model.fit(data, mask, 1, robust=robust, weights=np.ones(M), **kw)
    assert seen == [("fit_batch", 10, ["rows"]), ("fit_weighted", (M,))]
