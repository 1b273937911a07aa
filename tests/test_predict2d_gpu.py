"""The forward model of 2-D (AxCaliber-like) protocols on the GPU (include/mfx_predict2d.h, csrc/predict2d.hip).

Referees: a NumPy sum over the columns the library's own single-atom rotation returns (T.rotate_cols), which the kernel
must reproduce bit for bit, and the reference's own y_recons of every voxel of fit2d_cases.npz
(tests/golden/predict2d_cases.npz, written by gen_golden_predict2d.py), held to the rotation's 1e-10.

Protocols: syn2 (M = 66: one lane sweep and a 2-row tail, N = 24 atoms) and fix (M = 1776: 27 sweeps and 48 lanes, N = 8);
V in {1, 5, 37}: the last workgroup has idle waves."""
import os

import numpy as np
import pytest

from test_fit2d_gpu import DIFF, Z, atoms, csf_signal, random_dirs
from microstructure_fingerprinting_amd import engine
from microstructure_fingerprinting_amd import mf_utils as U

pytestmark = pytest.mark.gpu

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
RTOL_W = 1e-5   # tests/test_predict_gpu.py
PROTOCOLS = {"syn2": (24, 11, 0.1), "fix": (8, 12, 0.3)}     # atoms, seed, zmin (those of fit2d_cases.npz)
_cache = {}


def rot():
    if "rot" not in _cache:
        _cache["rot"] = np.load(os.path.join(G, "rot2d_cases.npz"))
    return _cache["rot"]


def gold():
    if "gold" not in _cache:
        _cache["gold"] = np.load(os.path.join(G, "fit2d_cases.npz"))
    return _cache["gold"]


def tables(name):
    """the tables of fit2d_cases.npz's dictionary of a protocol, made once"""
    if ("T", name) not in _cache:
        sch = rot()[name + "_sch"]
        N, seed, _ = PROTOCOLS[name]
        dic = atoms(sch, N, seed)
        assert np.array_equal(dic, gold()[name + "_dic"])
        _cache[("T", name)] = (U.RotateAtom2DTables(dic, sch, Z, DIFF), csf_signal(sch))
    return _cache[("T", name)]


def same(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def numpy_sum(T, params, peaks, maxfasc, csf_on, sig_csf):
    """P = 0; for k: if w_k > 0: P = P + w_k * T.rotate_cols(dir_k, id_k); if w_csf > 0: P = P + w_csf * sig_csf (w = M0 nu)"""
    V = params.shape[0]
    P = np.zeros((V, T.M))
    w = params[:, :1] * params[:, 1:1 + maxfasc]
    vk = [(v, k) for v in range(V) for k in range(maxfasc) if w[v, k] > 0]
    cols = T.rotate_cols(np.array([peaks[v, 3 * k:3 * k + 3] for v, k in vk]).reshape(-1, 3),
                         np.array([params[v, 1 + maxfasc + k] for v, k in vk], dtype=np.int64))
    for (v, k), col in zip(vk, cols):             # (v, k) ascending: f0, f1, f2 per voxel
        P[v] = P[v] + w[v, k] * col
    if csf_on:
        for v in range(V):
            wc = params[v, 0] * params[v, 1 + 2 * maxfasc]
            if wc > 0:
                P[v] = P[v] + wc * sig_csf
    return P


def hand_rows(T, V, maxfasc, csf_on, zmin, seed):
    """parameter rows with K mixed over 0..maxfasc; absent fascicles have fraction 0, atom 0 and a zero direction; voxel 0
    has nothing at all"""
    rng = np.random.default_rng(seed)
    params = np.zeros((V, engine.num_params(maxfasc, csf_on, False)))
    peaks = np.zeros((V, 3 * maxfasc))
    K = np.arange(V) % (maxfasc + 1)
    for v in range(V):
        params[v, 0] = rng.uniform(0.5, 2.0)
        nu = rng.uniform(0.1, 1.0, K[v] + 1)
        nu /= nu.sum()
        params[v, 1:1 + K[v]] = nu[:K[v]]
        params[v, 1 + maxfasc:1 + maxfasc + K[v]] = rng.integers(0, T.N, K[v])
        if K[v]:
            peaks[v, :3 * K[v]] = random_dirs(rng, K[v], zmin).reshape(-1)
        if csf_on and v % 2 == 1:
            params[v, 1 + 2 * maxfasc] = nu[K[v]]
        params[v, -2:] = rng.uniform(0, 1, 2)          # MSE, R2: ignored
    assert K[0] == 0
    return params, peaks, K


# ---- 1. bits
@pytest.mark.parametrize("V", [1, 5, 37])
@pytest.mark.parametrize("csf_on", [False, True])
@pytest.mark.parametrize("name", ["syn2", "fix"])
def test_hand_made_rows_bit_for_bit(name, csf_on, V):
    T, sig_csf = tables(name)
    params, peaks, K = hand_rows(T, V, 3, csf_on, PROTOCOLS[name][2], 7 + V)
    out, dstat = engine.predict2d(T, params, peaks, 3, csf_on, sig_csf if csf_on else None)
    ref = numpy_sum(T, params, peaks, 3, csf_on, sig_csf)
    assert same(out, ref)
    assert np.all(dstat == 0)                       # the zero directions of absent fascicles flag nothing
    assert np.all(out[0] == 0) and not np.any(np.signbit(out[0]))       # K = 0 without CSF: an exact zero row
    if V > 3:
        assert np.all(out[3, :8] > 0)


@pytest.mark.parametrize("name", ["syn2", "fix"])
def test_rows_of_the_fit_bit_for_bit(name):
    T, sig_csf = tables(name)
    g = gold()
    Y, peaks, K, csf = g[name + "_Y"], g[name + "_peaks"], g[name + "_K"], g[name + "_csf"]
    params, st = engine.fit2d(T, Y, K, csf, peaks, 2, True, sig_csf)
    assert np.all(st == 0)
    out, dstat = engine.predict2d(T, params, peaks, 2, True, sig_csf)
    assert same(out, numpy_sum(T, params, peaks, 2, True, sig_csf)) and np.all(dstat == 0)
    # without the CSF column, the fit's own classes
    nocsf = np.flatnonzero(csf == 0)
    p2, st2 = engine.fit2d(T, Y[nocsf], K[nocsf], None, peaks[nocsf], 2, False)
    out2, _ = engine.predict2d(T, p2, peaks[nocsf], 2, False)
    assert same(out2, numpy_sum(T, p2, peaks[nocsf], 2, False, None))
    assert same(out2, out[nocsf])


# ---- 2. the reference's y_recons
@pytest.mark.parametrize("name", ["syn2", "fix"])
def test_reproduces_the_reference_y_rec(name):
    T, sig_csf = tables(name)
    g = gold()
    y_rec = np.load(os.path.join(G, "predict2d_cases.npz"))[name + "_y_rec"]
    assert np.array_equal(sig_csf, g[name + "_sig_csf"]) and y_rec.shape == g[name + "_Y"].shape
    out, dstat = engine.predict2d(T, g[name + "_params"], g[name + "_peaks"], 2, True, sig_csf)
    assert np.all(dstat == 0)
    ratio = np.max(np.abs(out - y_rec), axis=1) / np.max(np.abs(y_rec), axis=1)
    print("%s: largest |out - y_rec| / max|y_rec| over %d voxels: %.3e" % (name, y_rec.shape[0], ratio.max()))
    assert np.all(ratio <= 1e-10)


# ---- 3. statuses
def test_directions_of_absent_and_present_fascicles():
    T, _ = tables("syn2")
    params, peaks, K = hand_rows(T, 9, 3, False, 0.1, 21)
    clean, _ = engine.predict2d(T, params, peaks, 3)
    pk = peaks.copy()
    v1 = int(np.flatnonzero(K == 1)[0])
    pk[v1, 3:6] = [0.0, 0.0, 2.0]                  # non-unit, fascicle 1 absent
    pk[v1, 6:9] = 0.0
    out, dstat = engine.predict2d(T, params, pk, 3)
    assert np.all(dstat == 0) and same(out, clean)
    # the same directions on present fascicles
    v3, v2 = int(np.flatnonzero(K == 3)[0]), int(np.flatnonzero(K == 2)[0])
    pk = peaks.copy()
    pk[v3, 3:6] = [0.0, 0.0, 2.0]                  # fascicle 1 of a K = 3 voxel
    pk[v3, 6:9] = 0.0                              # and fascicle 2: the lowest is reported
    pk[v2, 0:3] = 0.0                              # fascicle 0 of a K = 2 voxel
    out, dstat = engine.predict2d(T, params, pk, 3)
    badv = sorted([v2, v3])
    assert np.all(np.isnan(out[badv]))
    assert np.array_equal(dstat[v3, [0, 4]], [U.ROT2D_NEWDIR_NORM, 1]) and np.array_equal(dstat[v2, [0, 4]], [U.ROT2D_NEWDIR_NORM, 0])
    okv = np.setdiff1d(np.arange(9), badv)
    assert np.all(dstat[okv] == 0) and same(out[okv], clean[okv])
    with pytest.raises(ValueError, match="unit norm") as e:
        T.predict(params, pk)
    assert str(e.value) == str(T.error_for(dstat[badv[0], :4]))
    got = T.predict(params, pk, on_error='nan')
    assert np.all(np.isnan(got[badv])) and same(got[okv], clean[okv])
    assert same(T.predict(params, peaks), clean)
    # a voxel the fit could not serve: a NaN row in, a NaN row out, no direction looked at
    pn = params.copy()
    pn[v2] = np.nan
    got = T.predict(pn, pk[:, :], on_error='nan')
    assert np.all(np.isnan(got[v2])) and same(got[okv], clean[okv])


@pytest.mark.parametrize("what,value", [("id", -1.0), ("id", "N"), ("id", 1.5), ("id", np.nan), ("nu", -0.1), ("nu", np.inf),
                                        ("nu", np.nan), ("csf", -0.1), ("csf", np.inf)])
def test_bad_rows(what, value):
    import torch
    T, sig_csf = tables("syn2")
    params, peaks, K = hand_rows(T, 9, 3, True, 0.1, 22)
    clean, _ = engine.predict2d(T, params, peaks, 3, True, sig_csf)
    bad = params.copy()
    v = int(np.flatnonzero(K == 2)[0])
    col = {"id": 1 + 3 + 1, "nu": 1 + 1, "csf": 1 + 6}[what]
    bad[v, col] = T.N if value == "N" else value
    with pytest.raises(ValueError, match="atom index" if what == "id" else "weight M0 \\* nu"):
        engine.predict2d(T, bad, peaks, 3, True, sig_csf)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()   # noqa: E731
    out, stats, status, dstat = engine.predict2d_dev(T, t(bad), t(peaks), 3, True, t(sig_csf))
    out, status = out.cpu().numpy(), status.cpu().numpy()
    assert status[0] == (engine_bits()[what]) and status[1] == v
    assert np.all(np.isnan(out[v]))
    ok = np.arange(9) != v
    assert same(out[ok], clean[ok]) and np.all(dstat.cpu().numpy() == 0)


def engine_bits():
    return {"id": 1, "nu": 2, "csf": 2}          # MFX_PRED_ST_ID, MFX_PRED_ST_WEIGHT


# ---- 4. the residual
@pytest.mark.parametrize("name", ["syn2", "fix"])
def test_residual_and_r2(name):
    T, sig_csf = tables(name)
    g = gold()
    Y, peaks, K, csf = g[name + "_Y"], g[name + "_peaks"], g[name + "_K"], g[name + "_csf"]
    params, _ = engine.fit2d(T, Y, K, csf, peaks, 2, True, sig_csf)
    out, stats, dstat = engine.predict2d(T, params, peaks, 2, True, sig_csf, Y=Y)
    plain, _ = engine.predict2d(T, params, peaks, 2, True, sig_csf)
    assert same(out, plain)
    rss = np.sum((Y - out) ** 2, axis=1)
    assert np.all(np.abs(stats[:, 0] - rss) <= 1e-12 * rss)
    assert np.allclose(stats[:, 1], params[:, -1], rtol=RTOL_W, atol=1e-12)
    fit = T.fit(Y, peaks, K, csf.astype(bool), sig_csf)
    res = T.residuals(Y, fit, peaks, sig_csf)
    assert same(res, Y - T.predict(fit, peaks, sig_csf)) and same(res, Y - out)
    assert same(T.predict(fit.params, peaks, sig_csf), out)


# ---- 5. noise
def test_fused_noise():
    import torch
    T, sig_csf = tables("syn2")
    V, M = 37, T.M
    params, peaks, K = hand_rows(T, V, 3, True, 0.1, 23)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()   # noqa: E731
    dp, dk, dc = t(params), t(peaks), t(sig_csf)
    clean = engine.predict2d_dev(T, dp, dk, 3, True, dc)[0]
    rng = np.random.default_rng(24)
    sv, se = t(rng.uniform(0.01, 0.1, V)), t(rng.uniform(0.01, 0.1, (V, M)))
    for sigma, spread, ncoils in ((0.05, 0.05, 1), (sv, sv[:, None].expand(V, M).contiguous(), 4), (se, se, 2)):
        fused = engine.predict2d_dev(T, dp, dk, 3, True, dc, sigma_g=sigma, ncoils=ncoils, seed=99, offset=1000)[0]
        two = engine.sos_noise_dev(clean, spread, ncoils, seed=99, offset=1000)
        assert same(fused.cpu().numpy(), two.cpu().numpy())
        assert not same(fused.cpu().numpy(), clean.cpu().numpy())
    # a batch split into two calls
    V1 = 13
    whole = engine.predict2d_dev(T, dp, dk, 3, True, dc, sigma_g=se, ncoils=2, seed=5, offset=77)[0].cpu().numpy()
    a = engine.predict2d_dev(T, dp[:V1].contiguous(), dk[:V1].contiguous(), 3, True, dc, sigma_g=se[:V1].contiguous(), ncoils=2, seed=5,
                             offset=77)[0].cpu().numpy()
    b = engine.predict2d_dev(T, dp[V1:].contiguous(), dk[V1:].contiguous(), 3, True, dc, sigma_g=se[V1:].contiguous(), ncoils=2, seed=5,
                             offset=77 + V1 * M)[0].cpu().numpy()
    assert same(np.vstack([a, b]), whole)
    host, _ = engine.predict2d(T, params, peaks, 3, True, sig_csf, sigma_g=se.cpu().numpy(), ncoils=2, seed=5, offset=77)
    assert same(host, whole)
    # T.simulate
    s1 = T.simulate(params, peaks, sig_csf, SNR=20.0, seed=3)
    assert same(s1, T.simulate(params, peaks, sig_csf, SNR=20.0, seed=3))
    assert not same(s1, T.simulate(params, peaks, sig_csf, SNR=20.0, seed=4))
    assert same(s1, engine.predict2d(T, params, peaks, 3, True, sig_csf, sigma_g=params[:, 0] / 20.0, ncoils=1, seed=3)[0])
    assert s1.shape == (V, M) and np.all(np.isfinite(s1)) and np.all(s1 >= 0)


# ---- 6. host and device forms, a stream of its own
@pytest.mark.parametrize("name,V", [("syn2", 37), ("fix", 5)])
def test_dev_equals_host_on_a_stream(name, V):
    import torch
    T, sig_csf = tables(name)
    params, peaks, K = hand_rows(T, V, 3, True, PROTOCOLS[name][2], 25)
    rng = np.random.default_rng(26)
    Y = rng.uniform(0.0, 1.0, (V, T.M))
    host, hstats, hd = engine.predict2d(T, params, peaks, 3, True, sig_csf, Y=Y)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()   # noqa: E731
    dp, dk, dc, dY = t(params), t(peaks), t(sig_csf), t(Y)
    out, stats, status, dstat = engine.predict2d_dev(T, dp, dk, 3, True, dc, d_Y=dY)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        out_s, stats_s, status_s, dstat_s = engine.predict2d_dev(T, dp, dk, 3, True, dc, d_Y=dY)
    torch.cuda.synchronize()
    for o, q in ((out, stats), (out_s, stats_s)):
        assert same(o.cpu().numpy(), host) and same(q.cpu().numpy(), hstats)
    assert np.all(status.cpu().numpy() == 0) and np.all(status_s.cpu().numpy() == 0)
    assert np.array_equal(dstat.cpu().numpy(), hd) and np.array_equal(dstat_s.cpu().numpy(), hd)
