"""Bootstrap (include/mfx_boot.h), the parts that need no GPU: the C ABI, the argument checks that come before any
device call, the restatement's generator against the published known-answer vectors, and the power condition of
tests/test_boot_gpu.py checked on the CPU oracle."""
import os
import re

import numpy as np
import pytest

import _boot_ref as R
from microstructure_fingerprinting_amd import _lib, engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class NoDevicePlan:
    """Stands for an engine.Plan in the argument checks: asking it for its handle is a device call."""
    def __init__(self, M, scheme=None):
        self.M, self.scheme = M, scheme

    def handle(self):
        raise AssertionError("the device was touched before the arguments were checked")


def _declared():
    src = open(os.path.join(ROOT, "include", "mfx_boot.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(mfx_[a-z_0-9]+)\s*\(", src)))


def test_boot_abi_symbols():
    lib = _lib.lib()
    assert sorted(_lib.BOOT_EXPORTS) == _declared()
    for name in _lib.BOOT_EXPORTS:
        assert hasattr(lib, name)
        assert name not in _lib.EXPORTS and name not in _lib.ROBUST_EXPORTS and name not in _lib.PREDICT_EXPORTS
    assert lib.mfx_boot_abi_version() == 1
    assert lib.mfx_abi_version() == 3 and lib.mfx_predict_abi_version() == 1 and lib.mfx_robust_abi_version() == 1
    for f in ("boot_resample_dev", "boot_reduce_dev", "fit_bootstrap_dev", "fit_bootstrap"):
        assert callable(getattr(engine, f))
    src = open(os.path.join(ROOT, "include", "mfx_boot.h")).read()
    assert int(re.search(r"#define MFX_BOOT_STREAM (0x[0-9a-f]+)u", src).group(1), 16) == R.BOOT_STREAM != R.SOS_STREAM
    assert int(re.search(r"#define MFX_BOOT_MAX_B (\d+)", src).group(1)) == engine.BOOT_MAX_B == 4096
    assert int(re.search(r"#define MFX_BOOT_MAX_Q (\d+)", src).group(1)) == engine.BOOT_MAX_Q
    assert int(re.search(r"#define MFX_BOOT_NSTAT (\d+)", src).group(1)) == engine.BOOT_NSTAT


def test_entry_points_without_device():
    lib = _lib.lib()
    M = 16
    Y, pk = np.ones((1, M)), np.array([[0.0, 0.0, 1.0]])
    K = np.ones(1, dtype=np.int32)
    st, ag = np.zeros(1, dtype=np.int32), np.zeros(1, dtype=np.int32)
    stats = np.zeros((1, 3, 5))
    calls = [lambda: lib.mfx_boot_resample_dev(M, None, None, None, 1, 0, 0, None, None, None, -1, 4, 0, 1, 0, 0, None, None, None, None),
             lambda: lib.mfx_boot_gather_dev(None, None, 1, 0, 0, None, 0, 4, None, -1, 4, None, None, None, None),
             lambda: lib.mfx_boot_reduce_dev(None, None, -1, 4, 3, None, 0, None, None),
             lambda: lib.mfx_boot_fit_dev(None, None, None, 1, 0, 0, None, None, 0, None, None, None, None, 1, 4, 0, 1, 0, 0, None, 0,
                                          None, 0, 0, None, None, None, None, None),
             lambda: lib.mfx_boot_fit(None, _lib.dptr(Y), _lib.iptr(K), None, None, _lib.dptr(pk), 1, 0, 0, None, None, 0, None, None,
                                      None, 1, 4, 0, 1, 0, 0, None, 0, None, 0, 0, _lib.dptr(stats), _lib.iptr(ag), _lib.iptr(st), None)]
    for c in calls:
        if lib.mfx_device_count() > 0:             # with a device the null plan / the negative V is what is wrong
            assert c() == _lib.MFX_ERR_ARG
            continue
        assert c() == _lib.MFX_ERR_NO_DEVICE
        assert "no CPU path" in lib.mfx_last_error().decode()


def test_engine_argument_checks_come_before_the_device():
    M = 20
    sch = np.zeros((M, 7)); sch[:, 3] = np.repeat([0.0, 0.1, 0.2, 0.3], 5); sch[:, 4:7] = [0.03, 0.01, 0.07]
    plan = NoDevicePlan(M, sch)
    Y = np.ones((3, M))
    pk = np.tile([0.0, 0.0, 1.0, 0.0, 0.6, 0.8], (3, 1))
    K = np.array([1, 2, 0])
    sc, se = np.ones(M), np.ones((M, 2))
    base = (Y, K, None, None, pk, 2, False, False)
    for args, kw, exc, msg in [
            (base, dict(B=0), ValueError, "B should be an integer >= 1"),
            (base, dict(B=2.5), ValueError, "B should be an integer"),
            (base, dict(B=True), ValueError, "B should be an integer"),
            (base, dict(kind='pairs'), ValueError, "kind should be one of"),
            (base, dict(q=(0.5, 1.5)), ValueError, r"q should lie in \[0, 1\]"),
            (base, dict(q=(-0.1,)), ValueError, r"q should lie in \[0, 1\]"),
            (base, dict(q=(np.nan,)), ValueError, r"q should lie in \[0, 1\]"),
            (base, dict(q='median'), ValueError, "q should be numbers"),
            (base, dict(seed=1.5), ValueError, "seed should be an integer"),
            (base, dict(B=4097), NotImplementedError, "at most 4096"),
            (base, dict(q=np.linspace(0, 1, 33)), NotImplementedError, "at most 32 bootstrap quantiles"),
            ((Y[:, :-1],) + base[1:], {}, ValueError, "data should have shape"),
            ((Y, K[:2]) + base[2:], {}, ValueError, "K should have one entry"),
            ((Y, np.array([1, 2, 3])) + base[2:], {}, ValueError, "K should lie in"),
            ((Y, K, np.array([1, 0, 0]), None, pk, 2, False, False), {}, ValueError, "flagged CSF need csf_on"),
            ((Y, K, None, np.array([0, 0, 1]), pk, 2, False, False), {}, ValueError, "flagged EAR need ear_on"),
            ((Y, K, np.array([1, 0]), None, pk, 2, True, False, sc), {}, ValueError, "csf should have one entry"),
            ((Y, K, None, None, pk[:, :3], 2, False, False), {}, ValueError, "peaks should have shape"),
            ((Y, K, None, None, pk, 2, True, False), {}, ValueError, "csf_on needs sig_csf"),
            ((Y, K, None, None, pk, 2, False, True, None, se[:, :1], 2), {}, ValueError, "sig_ear should have shape"),
            ((Y, K, None, None, np.tile(pk, (1, 2)), 4, False, False), {}, ValueError, "maxfasc must be 0..3"),
            (base, dict(params=np.zeros((3, 6))), ValueError, r"params should have shape \(3, 7\)"),
            (base, dict(vox=np.arange(2)), ValueError, "vox should have one entry"),
            (base, dict(kind='residual', groups=np.zeros(M - 1, dtype=int)), ValueError, "groups should be 20 integers"),
            (base, dict(kind='residual', groups=np.zeros(M)), ValueError, "groups should be 20 integers")]:
        with pytest.raises(exc, match=msg):
            engine.fit_bootstrap(plan, *args, **kw)
    with pytest.raises(ValueError, match="knows no scheme"):
        engine.fit_bootstrap(NoDevicePlan(M), *base, kind='residual')
    # the default groups: rows sharing (G, Delta, delta)
    g = engine.boot_groups(sch)
    assert g.dtype == np.int32 and np.array_equal(g, np.repeat([0, 1, 2, 3], 5))
    assert engine.boot_columns(2, True, True, 2) == ['M0', 'nu_0', 'nu_1', 'nu_csf', 'nu_ear', 'MSE', ('prop', 0, 0), ('prop', 0, 1),
                                                     ('prop', 1, 0), ('prop', 1, 1)]
    assert len(engine.boot_columns(3, False, True, 1)) == R.columns(3, False, True, 1)


def test_mfmodelfit_bootstrap_checks_come_before_the_device():
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
    fit = fit_object()
    for kw, exc, msg in [(dict(B=0), ValueError, "B should be an integer >= 1"), (dict(B=10.0), ValueError, "B should be an integer"),
                         (dict(kind='block'), ValueError, "kind should be one of"), (dict(q=(0.1, 2.0)), ValueError, "q should lie in"),
                         (dict(B=4097), NotImplementedError, "at most 4096"),
                         (dict(voxels=[3]), ValueError, "positions in the ROI"),
                         (dict(kind='residual', groups=np.zeros(3, dtype=int)), ValueError, "groups should be %d integers" % M)]:
        with pytest.raises(exc, match=msg):
            fit.bootstrap(data, **kw)
    with pytest.raises(ValueError, match="data should have shape"):
        fit.bootstrap(data[..., :-1], B=4)
    for extra in (dict(weights_roi=np.ones(M)), dict(weights_roi=np.ones((3, M)), robust_base=None, robust_options={},
                                                     robust_info={'scale': np.ones(3)})):
        with pytest.raises(NotImplementedError, match="bootstrap of a weighted or robust fit is not served"):
            fit_object(**extra).bootstrap(data, B=4)
    assert model.ms_interpolator._tables is None        # nothing was created on a device
    if _lib.lib().mfx_device_count() == 0:              # valid arguments get as far as the device, and no further
        with pytest.raises(_lib.MfxError, match="no CPU path"):
            fit.bootstrap(data, B=4)


def test_philox_known_answers():
    """Philox4x32-10's published known-answer vectors (Random123's kat_vectors), the vectorised form against the plain one,
    and one counter of the sum-of-squares noise as tests/test_predict_gpu.py derives it."""
    assert R.philox4x32_10([0, 0, 0, 0], [0, 0]) == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    assert R.philox4x32_10([0xffffffff] * 4, [0xffffffff] * 2) == [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]
    assert R.philox4x32_10([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0]) == \
        [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]
    import test_predict_gpu as tpg
    seed, idx, j = 0x0123456789abcdef, (1 << 32) + 7, 2
    ctr, key = [idx & R.M32, idx >> 32, j, R.SOS_STREAM], [seed & R.M32, seed >> 32]
    assert R.philox4x32_10(ctr, key) == tpg._philox(ctr, key)
    idxs = np.array([0, 1, (1 << 32) - 1, 1 << 32, (1 << 64) - 1, 123456789012345], dtype=np.uint64)
    for b in (0, 3, 4095):
        u = R.philox_word0(idxs, b, seed)
        want = [R.philox4x32_10([int(i) & R.M32, int(i) >> 32, b, R.BOOT_STREAM], key)[0] for i in idxs]
        assert [int(x) for x in u] == want
    assert R.philox_word0(idxs, 0, seed, R.SOS_STREAM)[0] != R.philox_word0(idxs, 0, seed)[0]


def test_mulhi32_indexing_stays_inside_the_group():
    for n in (1, 2, 3, 7, 64, 8192):
        u = np.array([0, 1, (1 << 31) - 1, 1 << 31, (1 << 32) - 2, (1 << 32) - 1] + list(range(0, 1 << 32, (1 << 32) // 997)), dtype=np.uint64)
        j = R.mulhi32(u, n)
        assert j.max() < n and j.min() == 0 and int(R.mulhi32((1 << 32) - 1, n)) == n - 1
    # every row of a group can be drawn, and only rows of the group
    lists = R.group_lists([5, 5, -1, 5, 9, -1])
    assert [list(x) for x in lists] == [[0, 1, 3], [0, 1, 3], [2, 5], [0, 1, 3], [4], [2, 5]]


def test_restatement_of_the_rule():
    """The pieces of the restatement against their definitions: the scale, the sign flips, the group draws, the status."""
    rng = np.random.default_rng(5)
    V, M, B = 3, 12, 40
    Y, P = rng.normal(10, 1, (V, M)), rng.normal(10, 1, (V, M))
    prm = np.array([[100.0, 0.7, 0.3, 1, 2, 0.0, 3.0, 0.9], [100.0, 1.0, 0.0, 1, 2, 0.5, 3.0, 0.9], [100.0, 0.5, 0.5, 1, 2, 0.1, 3.0, 0.9]])
    assert [R.n_active(r, 2, True, False) for r in prm] == [2, 2, 3]
    assert R.scale(12, 3, True) == np.sqrt(12.0 / 9.0) and R.scale(12, 3, False) == 1.0
    P[2, 4] = np.nan
    Ys, st = R.resample(Y, P, prm, 2, True, False, B, 0, 9, True)
    assert list(st) == [0, 0, 2] and np.all(np.isnan(Ys[2]))
    a = np.sqrt(12.0 / 10.0)
    dev = (Ys[:2] - P[:2, None, :]) / (a * (Y[:2] - P[:2]))[:, None, :]
    assert np.allclose(np.abs(dev), 1.0, rtol=1e-12) and 0.35 < np.mean(dev > 0) < 0.65
    groups = np.array([0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 7])
    Yr, st = R.resample(Y[:2], P[:2], prm[:2], 2, True, False, B, 1, 9, False, groups=groups)
    r = Y[:2] - P[:2]
    for v in range(2):
        for m in range(M):
            pool = P[v, m] + r[v, groups == groups[m]]
            assert np.all(np.isin(Yr[v, :, m], pool))
        assert np.array_equal(Yr[v, :, 11], np.full(B, P[v, 11] + r[v, 11]))   # a group of one row keeps its residual
        assert len(np.unique(Yr[v, :, 0])) == 4                                   # every row of the group is drawn
    # keyed by the batch index: a subset with vox gives the whole batch's replicates
    Ysub, _ = R.resample(Y[1:2], P[1:2], prm[1:2], 2, True, False, B, 0, 9, True, vox=[1])
    assert np.array_equal(Ysub[0], Ys[1])
    # M <= n_act: status 1
    _, st1 = R.resample(Y[:1, :2], P[:1, :2], prm[:1], 2, True, False, 2, 0, 9, True)
    assert list(st1) == [1]


def test_restatement_of_the_statistics():
    x = np.array([3.0, 1.0, 2.0, 2.0, 10.0])
    s = R.reduce_column(x, [True] * 5, [0.0, 0.5, 0.25, 1.0])
    assert s[0] == 5 and s[1] == 18.0 / 5.0 and np.isclose(s[2], np.std(x, ddof=1), rtol=1e-15) and s[3] == 1 and s[4] == 10
    assert np.allclose(s[5:], np.quantile(x, [0.0, 0.5, 0.25, 1.0]), rtol=1e-15)
    s = R.reduce_column(x, [False, True, False, False, False], [0.3])
    assert s[0] == 1 and s[1] == 1.0 and np.isnan(s[2]) and s[3] == s[4] == s[5] == 1.0
    s = R.reduce_column(x, [False] * 5, [0.3])
    assert s[0] == 0 and np.all(np.isnan(s[1:]))
    # the value table: a property counts only with a positive weight and an atom inside the dictionary
    reps = np.array([[[100.0, 0.6, 0.4, 2, 5, 4.0, 0.9], [100.0, 1.0, 0.0, 2, 0, 5.0, 0.9], [90.0, 0.5, 0.5, 3, 5, 6.0, 0.8]]])
    p0 = np.array([[100.0, 0.6, 0.4, 2, 5, 4.0, 0.9]])
    props = np.arange(16.0).reshape(2, 8)
    X, valid, agree = R.gather(reps, p0, 2, False, False, props, 8)
    assert X.shape == (1, 3, R.columns(2, False, False, 2)) and list(agree[0]) == [2, 2]
    assert np.array_equal(valid[0, :, 4:], [[True] * 4, [True, True, False, False], [True] * 4]) and np.all(valid[0, :, :4])
    assert np.array_equal(X[0, 0], [100.0, 0.6, 0.4, 4.0, 2.0, 10.0, 5.0, 13.0]) and np.all(np.isnan(X[0, 1, 6:]))


def test_power_condition_on_the_cpu_oracle():
    """What keeps the GPU comparisons of tests/test_boot_gpu.py from passing on replicates that all equal the original:
    on tests/golden/fit_cases.npz as it is (its signals carry noise at SNR about 30; no noise is added), wild bootstrap,
    seed 1, B = 16, inflate on, fitted by the CPU oracle: in at least half of the two-fascicle voxels at least one
    replicate picks, with a positive weight, another atom than the original fit.  Measured share: 10 of 10."""
    from oracle import oracle as orc
    d, sch, sig_csf, sig_ear = R.golden_model()
    T = orc.init_tables(d["dictionary"], d["sch_ms"], R.Z)
    E, B = int(d["E"]), 16
    K, csf, ear, peaks, Y = d["numfasc"], d["csf"], d["ear"], d["peaks"], d["Y"]
    P = orc.fit_batch(T, sch, Y, K, csf, ear, peaks, 2, True, True, sig_csf, sig_ear, E)
    pred = R.oracle_predict(T, sch, P, peaks, 2, True, True, sig_csf, sig_ear)
    two = np.flatnonzero(K == 2)
    Ys, st = R.resample(Y[two], pred[two], P[two], 2, True, True, B, 0, 1, True, vox=two)
    assert not st.any()
    moved = 0
    for i, v in enumerate(two):
        rep = orc.fit_batch(T, sch, Ys[i], np.full(B, 2), np.full(B, csf[v]), np.full(B, ear[v]), np.tile(peaks[v], (B, 1)), 2, True,
                            True, sig_csf, sig_ear, E)
        moved += bool(np.any((rep[:, 3:5] != P[v, 3:5]) & (rep[:, 1:3] > 0)))
    print("power condition: %d of %d two-fascicle voxels have a replicate with another atom" % (moved, two.size))
    assert two.size == 10 and 2 * moved >= two.size
