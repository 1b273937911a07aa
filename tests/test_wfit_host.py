"""Weighted fit (include/mfx_wfit.h), the parts that need no GPU: the C ABI, the argument checks that come before any
device call, the gap condition of tests/golden/wfit_cases.npz (written by gen_golden_wfit.py from the reference's chain
on row-deleted protocols), and the referee of tests/test_wfit_gpu.py checked against those goldens."""
import os
import re

import numpy as np
import pytest

import _wfit_ref as R
from microstructure_fingerprinting_amd import _lib, engine
from oracle import oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(G, "wfit_cases.npz"))


class NoDevicePlan:
    """Stands for an engine.Plan in the argument checks: asking it for its handle is a device call."""
    def __init__(self, M):
        self.M = M

    def handle(self):
        raise AssertionError("the device was touched before the arguments were checked")


def _declared():
    src = open(os.path.join(ROOT, "include", "mfx_wfit.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(mfx_[a-z_0-9]+)\s*\(", src)))


def test_wfit_abi_symbols():
    lib = _lib.lib()
    assert sorted(_lib.WFIT_EXPORTS) == _declared()
    for name in _lib.WFIT_EXPORTS:
        assert hasattr(lib, name)
        assert name not in _lib.EXPORTS and name not in _lib.FIT2D_EXPORTS
    assert lib.mfx_wfit_abi_version() == 1
    assert lib.mfx_abi_version() == 3 and lib.mfx_fit2d_abi_version() == 1      # the other headers keep their versions
    assert lib.mfx_wfit_max_atoms(None, 2) == 0
    assert callable(engine.fit_weighted) and callable(engine.fit_weighted_dev)


def test_entry_points_without_device():
    lib = _lib.lib()
    M = 16
    Y, W, pk = np.ones((1, M)), np.ones((1, M)), np.array([[0.0, 0.0, 1.0]])
    K = np.ones(1, dtype=np.int32)
    prm = np.zeros((1, 5))
    st = np.zeros(1, dtype=np.int32)
    calls = [lambda: lib.mfx_wfit_batch_dev(None, None, None, M, None, 1, 1, None, None, None),
             lambda: lib.mfx_wfit_batch(None, _lib.dptr(Y), _lib.dptr(W), M, _lib.iptr(K), None, _lib.dptr(pk), 1, 0, None, 1,
                                        _lib.dptr(prm), _lib.iptr(st)),
             lambda: lib.mfx_wfit_batch(None, _lib.dptr(Y), _lib.dptr(W), M, _lib.iptr(K), None, _lib.dptr(pk), 4, 0, None, 1,
                                        _lib.dptr(prm), _lib.iptr(st))]
    for c in calls:
        if lib.mfx_device_count() > 0:             # with a device the null plan is what is wrong
            assert c() == _lib.MFX_ERR_ARG
            continue
        assert c() == _lib.MFX_ERR_NO_DEVICE
        assert "no CPU path" in lib.mfx_last_error().decode()
    lib.mfx_wfit_debug_set_force_explicit(1)
    lib.mfx_wfit_debug_set_force_explicit(0)


def test_engine_argument_checks_come_before_the_device():
    M = 20
    plan = NoDevicePlan(M)
    Y, W = np.ones((3, M)), np.ones((3, M))
    pk = np.tile([0.0, 0.0, 1.0, 0.0, 0.6, 0.8], (3, 1))
    K = np.array([1, 2, 0])
    sc = np.ones(M)
    for args, kw, msg in [((Y[:, :-1], W, K, None, pk, 2, False), {}, "measurements"),
                          ((Y, W[:, :-1], K, None, pk, 2, False), {}, r"weights should have shape .*\(3 voxels\)"),
                          ((Y, W[:2], K, None, pk, 2, False), {}, "weights should have shape"),
                          ((Y, np.ones(M + 1), K, None, pk, 2, False), {}, "weights should have shape"),
                          ((Y, W, K, None, pk[:, :3], 2, False), {}, "peaks should have shape"),
                          ((Y, W, K[:2], None, pk, 2, False), {}, "K should have one entry"),
                          ((Y, W, np.array([1, 2, 3]), None, pk, 2, False), {}, "K should lie in"),
                          ((Y, W, K, np.array([1, 0, 0]), pk, 2, False, sc), {}, "need csf_on"),
                          ((Y, W, K, np.array([1, 0, 0]), pk, 2, True), {}, "need csf_on and sig_csf"),
                          ((Y, W, K, np.array([1, 0]), pk, 2, True, sc), {}, "csf should have one entry"),
                          ((Y, W, K, None, np.tile(pk, (1, 2)), 4, False), {}, "not served for maxfasc = 4"),
                          ((Y, W, K, None, pk, 2, False), dict(ear=np.array([0, 1, 0])), "not served for voxels with an EAR")]:
        with pytest.raises(ValueError, match=msg):
            engine.fit_weighted(plan, *args, **kw)


def test_mfmodel_weight_checks_come_before_the_device(tmp_path):
    """Each failure is a ValueError that names the voxel count, raised before the model's device tables exist."""
    import microstructure_fingerprinting_amd as mf
    d = np.load(os.path.join(G, "fit_cases.npz"))
    model = mf.MFModel({"dictionary": d["dictionary"], "sch_mat": d["sch_ms"], "orientation": R.Z, "num_atom": int(d["N"]),
                        "num_ear": int(d["E"]), "T2_csf": float(d["T2_csf"]), "DIFF_csf": float(d["DIFF_csf"]),
                        "T2_ear": float(d["T2_ear"]), "DIFF_ear": d["DIFF_ear"], "fasc_propnames": ["rad ", "fin"],
                        "rad": d["rad"], "fin": d["fin"]})
    M = d["sch"].shape[0]
    data = np.ones((2, 3, M)); mask = np.ones((2, 3)); mask[0, 0] = 0
    pk = np.tile([0, 0, 1.0, 1, 0, 0], (2, 3, 1))
    kw = dict(peaks=pk, pgse_scheme=d["sch"], verbose=0)
    W = np.ones((2, 3, M))
    neg = W.copy(); neg[1, 1, 4] = -1.0; neg[1, 2, 0] = -0.5
    nan = W.copy(); nan[0, 1, 3] = np.nan
    inf = np.ones(M); inf[2] = np.inf
    none = W.copy(); none[1, 0] = 0.0
    outside = W.copy(); outside[0, 0] = -1.0            # a voxel outside the mask is never looked at
    for w, msg in [(np.ones((2, 3, M - 1)), "weights not compatible with the data of 5 voxel"),
                   (np.ones((3, 2, M)), "weights not compatible"), (np.ones(M + 2), "weights not compatible"),
                   (neg, "Detected 2 of 5 voxel"), (nan, "Detected 1 of 5 voxel.* negative or non-finite"),
                   (inf, "Detected 5 of 5 voxel"), (none, "Detected 1 of 5 voxel.* without a positive weight"),
                   (np.zeros(M, dtype=bool), "Detected 5 of 5 voxel.* without a positive weight"),
                   (np.array(["a"] * M), "boolean or numeric")]:
        with pytest.raises(ValueError, match=msg):
            model.fit(data, mask, 1, weights=w, **kw)
    with pytest.raises(ValueError, match="not served together with ear_mask: 5 of 5 voxel"):
        model.fit(data, mask, 1, weights=W, ear_mask=np.ones((2, 3)), **kw)
    assert model.ms_interpolator._tables is None        # nothing was created on a device
    if _lib.lib().mfx_device_count() == 0:              # valid weights get as far as the device, and no further
        for w in (outside, np.ones(M, dtype=bool), W.astype(np.int16)):
            with pytest.raises(_lib.MfxError, match="no CPU path"):
                model.fit(data, mask, 1, weights=w, **kw)


def test_golden_gap_condition(gold):
    """Best and runner-up objective over all index tuples of the row-deleted problem differ by at least 1e-8 |y'|^2 in
    every stored voxel, every voxel has its own mask, and every class is there."""
    assert float(gold["gap"]) == 1e-8
    models = R.golden_models()
    nvox = 0
    for name, nmask in (("fc", 8), ("uk", 12)):
        dic, _, _, sch = models[name]
        M = sch.shape[0]
        o, ysq, W, Y = gold[name + "_obj2"], gold[name + "_ysq"], gold[name + "_W"], gold[name + "_Y"]
        V = ysq.shape[0]
        nvox += V
        assert W.shape == (V, M) and W.dtype == np.uint8 and set(np.unique(W)) == {0, 1} and np.all(W.sum(axis=1) == M - nmask)
        assert len({w.tobytes() for w in W}) == V
        assert gold[name + "_params"].shape == (V, 8) and o.shape == (V, 2)
        K, csf = gold[name + "_K"], gold[name + "_csf"]
        fitted = (K + csf) > 0
        assert np.all(o[fitted, 1] - o[fitted, 0] >= 1e-8 * ysq[fitted])
        assert np.allclose(ysq, np.sum((W * Y) ** 2, axis=1), rtol=1e-13)
        assert np.allclose(gold[name + "_params"][:, -2] * (M - nmask), o[:, 0], rtol=0, atol=1e-9 * ysq.max())
        assert np.all(gold[name + "_params"][~fitted] == 0)
    assert nvox >= 24
    Kc = {(int(k), int(c)) for n in ("fc", "uk") for k, c in zip(gold[n + "_K"], gold[n + "_csf"])}
    assert Kc == {(0, 0), (0, 1), (1, 0), (1, 1), (2, 0), (2, 1)}
    assert sch.shape[0] % 8 != 0                        # the UKBB subject protocol: 105 rows, G-bracketed
    assert os.path.getsize(os.path.join(G, "wfit_cases.npz")) < 1 << 20


def test_referee_reproduces_the_reference(gold):
    """The GPU tests' referee - the oracle's solver on sqrt(W)-scaled oracle rotations plus the weighted row packing -
    against the reference's results on the row-deleted protocols; its masked-row and deleted-row forms agree bit for bit."""
    models = R.golden_models()
    for name in ("fc", "uk"):
        dic, sch_ms, ordir, sch = models[name]
        T = orc.init_tables(dic, sch_ms, ordir)
        ref = gold[name + "_params"]
        rows, rows_del = [], []
        for v in range(ref.shape[0]):
            K, csf = int(gold[name + "_K"][v]), bool(gold[name + "_csf"][v])
            a = (T, sch, gold[name + "_Y"][v], gold[name + "_W"][v], gold[name + "_peaks"][v, :3 * K].reshape(K, 3), csf,
                 gold[name + "_sig_csf"], 2, True)
            rows.append(R.ref_row(*a))
            rows_del.append(R.ref_row(*a, deleted=True))
        rows, rows_del = np.array(rows), np.array(rows_del)
        # a zero row adds +0.0 to every serial sum: bit for bit where the solver sums serially (two sub-dictionaries and
        # more); with one sub-dictionary it takes |y|^2 from np.sum, whose pairwise blocks move with the row count
        two = gold[name + "_K"] + gold[name + "_csf"] >= 2
        assert np.array_equal(rows[two], rows_del[two])
        assert np.array_equal(rows[:, 3:5], rows_del[:, 3:5]) and np.allclose(rows, rows_del, rtol=1e-12, atol=0)
        R.assert_rows(rows, ref, 2, name)


def test_weighted_r2_restatement():
    rng = np.random.default_rng(3)
    y, r = rng.normal(size=40), rng.normal(size=40)
    w = (rng.random(40) < 0.7).astype(float)
    k = w > 0
    assert np.isclose(R.weighted_r2(y, r, w), np.corrcoef(y[k], r[k])[0, 1] ** 2, rtol=1e-12)
    g = rng.uniform(0.1, 2, 40)
    assert np.isclose(R.weighted_r2(y, r, g), R.weighted_r2(y, r, 1e6 * g), rtol=1e-12)
    assert R.weighted_r2(y, r, np.eye(40)[0]) == 0.0 and R.weighted_r2(y, np.ones(40), g) == 0.0
