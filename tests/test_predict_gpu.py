"""Forward model on the GPU: engine.predict / predict_dev / sos_noise_dev, MFModel.predict / simulate,
MFModelFit.predict / residuals and mf_utils.gen_SoS_MRI.

The reference values (parameter rows and y_rec of the reference's own voxel routine) are in
tests/golden/predict_cases.npz, written by tests/golden/gen_golden_predict.py.

Each test prints what it measures before it asserts; the figures seen on the MI355X are in DESIGN.md 4.11.
"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
Z = np.array([0.0, 0.0, 1.0])
RTOL_W = 1e-5   # the project's tolerance for fitted weights (tests/test_fit_gpu.py)
CLASSES = ["fit_cases", "fit_cases_k1", "fit_c2_small", "real_ukbb_fit_k2", "real_ukbb_fit_k2csf", "real_ukbb_fit_k2csfear"]
_cache = {}


def _load(name):
    return np.load(os.path.join(G, name + ".npz"))


def _model(kind):
    """kind: 'small' (fit_cases' 14-atom model), 'c2' (fit_c2_small's 48 atoms), 'ukbb' (986 atoms)"""
    import microstructure_fingerprinting_amd as mf
    if kind not in _cache:
        if kind == "small":
            d = _load("fit_cases")
            md = {"dictionary": d["dictionary"], "sch_mat": d["sch_ms"], "num_atom": int(d["N"]), "num_ear": int(d["E"]),
                  "T2_csf": float(d["T2_csf"]), "DIFF_csf": float(d["DIFF_csf"]), "T2_ear": float(d["T2_ear"]),
                  "DIFF_ear": d["DIFF_ear"], "rad": d["rad"], "fin": d["fin"]}
        elif kind == "c2":
            d = _load("fit_c2_small")
            md = {"dictionary": d["dictionary"], "sch_mat": d["sch_ms"], "num_atom": d["dictionary"].shape[1], "num_ear": 0,
                  "T2_csf": 2.0, "DIFF_csf": 3.0e-9, "T2_ear": 0.08, "DIFF_ear": np.zeros(0), "rad": d["rad"], "fin": d["fin"]}
        else:
            d = _load("real_ukbb")
            md = {k: d[k] for k in ("dictionary", "sch_mat", "DIFF_ear", "rad", "fin")}
            md.update(num_atom=int(d["num_atom"]), num_ear=int(d["num_ear"]), T2_csf=float(d["T2_csf"]),
                      DIFF_csf=float(d["DIFF_csf"]), T2_ear=float(d["T2_ear"]))
        md.update(orientation=Z, fasc_propnames=["rad", "fin"])
        _cache[kind] = mf.MFModel(md)
    return _cache[kind]


def _case(cname):
    """-> dict(model, sch, Y, peaks [V x 3 maxfasc], numfasc, csf, ear, maxfasc, csf_on, ear_on, params, yrec)"""
    g = _load("predict_cases")
    if cname in ("fit_cases", "fit_cases_k1"):
        model, sch = _model("small"), _load("fit_cases")["sch"]
    elif cname == "fit_c2_small":
        model, sch = _model("c2"), _load("fit_c2_small")["sch_ms"]
    else:
        model, sch = _model("ukbb"), _load("real_ukbb")["sch_subj"]
    d = _load(cname)
    maxfasc, csf_on, ear_on = (int(x) for x in g[cname + "_flags"])
    return dict(model=model, sch=np.ascontiguousarray(sch), Y=d["Y"], peaks=np.ascontiguousarray(d["peaks"][:, :3 * maxfasc]),
                numfasc=g[cname + "_numfasc"], csf=g[cname + "_csf"], ear=g[cname + "_ear"], maxfasc=maxfasc,
                csf_on=bool(csf_on), ear_on=bool(ear_on), params=g[cname + "_params"], yrec=g[cname + "_yrec"])


def _engine_args(c):
    """(plan, params, peaks, maxfasc, csf_on, ear_on, sig_csf, sig_ear, E) for engine.predict"""
    m = c["model"]
    sig_csf, sig_ear, E = m._extra_signals(c["sch"], c["csf_on"], c["ear_on"])
    return (m.ms_interpolator.plan_for(c["sch"]), c["params"], c["peaks"], c["maxfasc"], c["csf_on"], c["ear_on"], sig_csf,
            sig_ear, E)


def _dev_args(c, params=None, peaks=None):
    import torch
    plan, P, pk, maxfasc, csf_on, ear_on, sig_csf, sig_ear, E = _engine_args(c)
    t = lambda a: None if a is None else torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda")  # noqa: E731
    return (plan, t(P if params is None else params), t(pk if peaks is None else peaks), maxfasc, csf_on, ear_on, t(sig_csf),
            t(sig_ear), E)


def _fit(c):
    V = c["Y"].shape[0]
    return c["model"].fit(c["Y"], np.ones(V), c["numfasc"], peaks=c["peaks"] if c["maxfasc"] else np.zeros((V, 3)),
                          pgse_scheme=c["sch"], csf_mask=c["csf"].astype(float) if c["csf_on"] else None,
                          ear_mask=c["ear"].astype(float) if c["ear_on"] else None, verbose=0)


# ------------------------------------------------------------------------------------------------
# against the reference
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cname", CLASSES)
def test_predict_reproduces_the_reference_y_rec(cname):
    """|out - y_rec| <= 1e-10 max|y_rec| per voxel (the bar of the HCP rotation test): beside the rotation's own
    error the weights add two roundings per compartment (M0 * nu here, the solver's w there)."""
    from microstructure_fingerprinting_amd import engine
    c = _case(cname)
    out = engine.predict(*_engine_args(c))
    assert out.shape == c["yrec"].shape
    scale = np.max(np.abs(c["yrec"]), axis=1)
    err = np.max(np.abs(out - c["yrec"]), axis=1)
    print("%s: max |out - y_rec| / max|y_rec| = %.3g" % (cname, float(np.max(err[scale > 0] / scale[scale > 0]))))
    assert np.all(err <= 1e-10 * scale)
    empty = (c["numfasc"] + c["csf"] + c["ear"]) == 0
    assert np.array_equal(out[empty], np.zeros((int(empty.sum()), out.shape[1])))
    if cname == "fit_cases":
        assert empty.sum() == 1   # voxel 21


# ------------------------------------------------------------------------------------------------
# against the fit
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cname", CLASSES)
def test_fit_predict_agrees_with_the_fits_own_MSE_and_R2(cname):
    """mean((Y - fit.predict())^2) against fit.MSE.  The solver gets its residual from Gram quantities and predict from
    the signal: they agree to cancellation error.  The reference's own y_rec against the reference's own MSE agree to
    1.2e-13 relative on fit_cases (recorded in the golden file); the bar is 100 times that; the noise-free voxel
    (voxel 9 of fit_cases, MSE of order 1e-12) alone has an absolute floor of 1e-12 mean(Y^2) beside it.  Voxels without any compartment are left out: the reference does not
    estimate there and reports MSE = 0 beside a zero prediction."""
    from microstructure_fingerprinting_amd import engine
    c = _case(cname)
    g = _load("predict_cases")
    assert float(g["fit_cases_ref_mse_rel"]) <= 1.2e-13
    fit = _fit(c)
    pred = fit.predict()
    V, M = c["Y"].shape
    assert pred.shape == (V, M)
    some = (c["numfasc"] + c["csf"] + c["ear"]) > 0
    mse = np.mean((c["Y"] - pred) ** 2, axis=1)
    floor = 1e-12 * np.mean(c["Y"] ** 2, axis=1)
    dev = np.abs(mse - fit.MSE)
    big = some & (fit.MSE > 1.0)
    print("%s: max |mean((Y - predict)^2) - MSE| / MSE = %.3g over %d voxels; noise-free voxels: max dev / mean(Y^2) = %.3g"
          % (cname, float(np.max(dev[big] / fit.MSE[big])) if big.any() else 0.0, int(big.sum()),
             float(np.max((dev / np.mean(c["Y"] ** 2, axis=1))[some & ~big])) if (some & ~big).any() else 0.0))
    assert np.all(dev[big] <= 1.2e-11 * fit.MSE[big])
    clean = some & ~big          # noise-free voxels (voxel 9 of fit_cases): only they get the absolute floor
    assert np.all(dev[clean] <= 1.2e-11 * np.abs(fit.MSE[clean]) + floor[clean])
    if cname == "fit_cases":
        assert list(np.flatnonzero(clean)) == [9]
    else:
        assert not clean.any()
    assert np.array_equal(fit.residuals(c["Y"]), c["Y"] - pred)
    # the fused residual: sum of squares against NumPy's on the returned signal, R2 against the fit's
    out, stats = engine.predict(*(_engine_args(c)[:1] + (fit.params_in_mask,) + _engine_args(c)[2:]), Y=c["Y"])
    assert np.array_equal(out, pred)
    rss = np.sum((c["Y"] - out) ** 2, axis=1)
    print("%s: max rel. deviation of the fused sum of squares from NumPy's = %.3g, of R2 from the fit's = %.3g"
          % (cname, float(np.max(np.abs(stats[:, 0] - rss) / rss)),
             float(np.max(np.abs(stats[some, 1] - fit.R2[some]) / np.maximum(fit.R2[some], 1e-300)))))
    assert np.all(np.abs(stats[:, 0] - rss) <= 1e-12 * rss)
    assert np.allclose(stats[some, 1], fit.R2[some], rtol=RTOL_W, atol=1e-12)


# ------------------------------------------------------------------------------------------------
# consistency, bit for bit
# ------------------------------------------------------------------------------------------------
def test_single_fascicle_voxel_equals_rotate_columns():
    import torch
    from microstructure_fingerprinting_amd import engine
    for cname in ("fit_cases_k1", "real_ukbb_fit_k2"):   # the second protocol has G-bracketed rows
        c = _case(cname)
        plan = c["model"].ms_interpolator.plan_for(c["sch"])
        N = c["model"].ms_interpolator.num_subs
        rng = np.random.default_rng(5)
        V = 37
        dirs = rng.normal(size=(V, 3))
        dirs /= np.linalg.norm(dirs, axis=1)[:, None]
        ids = rng.integers(0, N, V)
        P = np.zeros((V, engine.num_params(1, False, False)))
        P[:, 0], P[:, 1], P[:, 2] = 1.0, 1.0, ids
        out = engine.predict_dev(plan, torch.as_tensor(P, device="cuda"), torch.as_tensor(dirs, device="cuda"), 1)
        ref = engine.rotate_columns_dev(plan, torch.as_tensor(dirs, device="cuda"), torch.as_tensor(ids, device="cuda"))
        assert torch.equal(out, ref)


@pytest.mark.parametrize("cname", ["fit_cases", "real_ukbb_fit_k2csfear"])
def test_host_device_and_split_calls_agree(cname):
    import torch
    from microstructure_fingerprinting_amd import engine
    c = _case(cname)
    rep = 9 if cname != "fit_cases" else 1   # more voxels than one wave round
    params, peaks, Y = (np.tile(c[k], (rep, 1)) for k in ("params", "peaks", "Y"))
    a = _engine_args(c)
    host, hstats = engine.predict(a[0], params, peaks, *a[3:], Y=Y)
    d = _dev_args(c, params, peaks)
    dev, dstats = engine.predict_dev(*d, d_Y=torch.as_tensor(Y, device="cuda"))
    assert np.array_equal(dev.cpu().numpy(), host) and np.array_equal(dstats.cpu().numpy(), hstats)
    V = params.shape[0]
    cuts = [0, 1, max(2, V // 3 + 1), V]
    parts = [engine.predict_dev(d[0], d[1][i:j].contiguous(), d[2][i:j].contiguous(), *d[3:]) for i, j in zip(cuts, cuts[1:])]
    assert torch.equal(torch.cat(parts), dev)


def test_fit_object_predict_scatters_engine_predict():
    from microstructure_fingerprinting_amd import engine
    c = _case("fit_cases")
    mask = np.zeros((5, 6))
    mask.reshape(-1)[3:27] = 1     # 24 ROI voxels inside a 30-voxel grid
    roi = mask > 0

    def vol(a, fill=0.0):
        v = np.full(mask.shape + a.shape[1:], fill, dtype=a.dtype)
        v[roi] = a
        return v
    fit = c["model"].fit(vol(c["Y"], 7.0), mask, vol(c["numfasc"]), peaks=vol(c["peaks"]), pgse_scheme=c["sch"],
                         csf_mask=vol(c["csf"].astype(float)), ear_mask=vol(c["ear"].astype(float)), verbose=0)
    a = _engine_args(c)
    flat = engine.predict(a[0], fit.params_in_mask, *a[2:])
    want = np.zeros(mask.shape + (c["Y"].shape[1],))
    want[roi] = flat
    got = fit.predict()
    assert got.dtype == np.float64 and np.array_equal(got, want)
    assert np.array_equal(got[~roi], np.zeros_like(got[~roi]))
    g32 = fit.predict(dtype=np.float32)
    assert g32.dtype == np.float32 and np.array_equal(g32, want.astype(np.float32))
    buf = np.full(want.shape, 3.0, dtype=np.float32)
    assert fit.predict(out=buf) is buf and np.array_equal(buf, g32)
    res = fit.residuals(vol(c["Y"], 7.0))
    assert np.array_equal(res[roi], c["Y"] - flat) and not res[~roi].any()
    fit.PREDICT_CHUNK = 7            # several device calls give the same volume
    assert np.array_equal(fit.predict(), want)
    assert "predict" not in fit.param_names


# ------------------------------------------------------------------------------------------------
# errors
# ------------------------------------------------------------------------------------------------
def test_direction_norm_is_checked_only_for_present_fascicles():
    from microstructure_fingerprinting_amd import engine
    c = _case("fit_c2_small")
    a = _engine_args(c)
    peaks = c["peaks"].copy()
    peaks[2, 3:] *= 1.5
    with pytest.raises(ValueError, match="unit norm"):
        engine.predict(a[0], c["params"], peaks, *a[3:])
    params = c["params"].copy()
    params[2, 2] = 0.0               # that fascicle's weight is 0: its direction is not looked at
    params[2, 4] = 1e9               # nor its atom index
    out = engine.predict(a[0], params, peaks, *a[3:])
    assert np.all(np.isfinite(out))
    again = engine.predict(*a)       # the plan's status word is clear again
    assert np.all(np.isfinite(again))


@pytest.mark.parametrize("col,value", [(3, "N"), (3, -1.0), (4, 2.5), (1, -0.25), (0, np.inf), (3, np.nan)])
def test_bad_indices_and_weights_raise_and_leave_a_nan_row(col, value):
    import torch
    from microstructure_fingerprinting_amd import engine
    c = _case("fit_c2_small")
    a = _engine_args(c)
    value = float(c["model"].ms_interpolator.num_subs) if value == "N" else value
    params = c["params"].copy()
    params[4, col] = value
    with pytest.raises(ValueError):
        engine.predict(a[0], params, *a[2:])
    d = _dev_args(c, params)
    with pytest.raises(ValueError, match="voxel 4"):
        engine.predict_dev(*d)
    out = engine.predict_dev(*d, check=False).cpu().numpy()
    good = engine.predict(*a)
    assert np.all(np.isnan(out[4]))
    keep = np.arange(out.shape[0]) != 4
    assert np.array_equal(out[keep], good[keep])
    assert np.array_equal(engine.predict_dev(*_dev_args(c)).cpu().numpy(), good)   # a valid batch afterwards
    assert torch.cuda.is_available()


def test_bad_row_beside_a_bad_direction_leaves_the_plan_clean():
    """A batch with both faults raises for the bad row; the direction flag does not wait for the next call."""
    from microstructure_fingerprinting_amd import engine
    c = _case("fit_c2_small")
    params, peaks = c["params"].copy(), c["peaks"].copy()
    params[4, 3] = -1.0
    peaks[2, 3:] *= 1.5
    with pytest.raises(ValueError, match="voxel 4"):
        engine.predict_dev(*_dev_args(c, params, peaks))
    out = engine.predict_dev(*_dev_args(c))          # a valid batch on the same plan: no left-over ValueError
    assert np.array_equal(out.cpu().numpy(), engine.predict(*_engine_args(c)))


def test_fit_object_predict_gives_nan_for_a_voxel_without_valid_parameters():
    """One voxel whose parameters cannot be predicted (fitted from unusable data, say) costs its own row, not the volume."""
    c = _case("fit_c2_small")
    fit = _fit(c)
    good = fit.predict()
    fit.params_in_mask[1, 0] = np.nan      # M0
    fit.params_in_mask[3, 2] = -0.1        # nu_f1
    fit.params_in_mask[5, 3] = 48.0        # ID_f0 = N
    got = fit.predict()
    bad = np.array([False, True, False, True, False, True])
    assert np.all(np.isnan(got[bad])) and np.array_equal(got[~bad], good[~bad])
    res = fit.residuals(c["Y"])
    assert np.all(np.isnan(res[bad])) and np.array_equal(res[~bad], c["Y"][~bad] - good[~bad])
    with pytest.raises(ValueError):        # the model-level call on such rows still refuses them
        c["model"].predict(fit.params_in_mask, c["peaks"], pgse_scheme=c["sch"])


def test_model_predict_refuses_sigma_without_coils():
    c = _case("fit_c2_small")
    with pytest.raises(ValueError, match="N"):
        c["model"].predict(c["params"], c["peaks"], pgse_scheme=c["sch"], sigma_g=3.0)


def test_ear_index_out_of_range_raises():
    from microstructure_fingerprinting_amd import engine
    c = _case("fit_cases")
    a = _engine_args(c)
    params = c["params"].copy()
    v = int(np.flatnonzero(c["ear"] & (params[:, 6] > 0))[0])
    params[v, 7] = a[8]              # ID_ear = E
    with pytest.raises(ValueError):
        engine.predict(a[0], params, *a[2:])
    out = engine.predict_dev(*_dev_args(c, params), check=False).cpu().numpy()
    assert np.all(np.isnan(out[v])) and np.all(np.isfinite(np.delete(out, v, axis=0)))


# ------------------------------------------------------------------------------------------------
# noise: what is deterministic
# ------------------------------------------------------------------------------------------------
def _philox(ctr, key):
    c, k = list(ctr), list(key)
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & 0xffffffff, (p0 >> 32) ^ c[3] ^ k[1], p0 & 0xffffffff]
        k = [(k[0] + 0x9E3779B9) & 0xffffffff, (k[1] + 0xBB67AE85) & 0xffffffff]
    return c


def test_noise_follows_the_documented_counter_layout():
    """The generator written out on the host (Philox4x32-10, which reproduces the published known-answer vectors):
    key = seed, counter = (index lo, index hi, coil, 'SOSM').  The device's log / sin / cos may differ from NumPy's in
    the last bits: 1e-13 relative."""
    import torch
    from microstructure_fingerprinting_amd import engine
    assert _philox([0, 0, 0, 0], [0, 0]) == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    assert _philox([0xffffffff] * 4, [0xffffffff] * 2) == [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]
    seed, offset, ncoils, n = 0x0123456789abcdef, (1 << 32) - 5, 3, 40
    rng = np.random.default_rng(0)
    S0, sg = rng.uniform(0, 3, n), rng.uniform(0.1, 1, n)
    want = np.zeros(n)
    for i in range(n):
        idx, acc = offset + i, 0.0
        for j in range(ncoils):
            w = _philox([idx & 0xffffffff, idx >> 32, j, 0x534f534d], [seed & 0xffffffff, seed >> 32])
            u1 = ((((w[0] >> 5) << 26) | (w[1] >> 6)) + 1.0) * 2.0 ** -53
            u2 = (((w[2] >> 5) << 26) | (w[3] >> 6)) * 2.0 ** -53
            r = np.sqrt(-2.0 * np.log(u1))
            acc = (acc + (S0[i] + sg[i] * (r * np.cos(2 * np.pi * u2))) ** 2) + (sg[i] * (r * np.sin(2 * np.pi * u2))) ** 2
        want[i] = np.sqrt(acc)
    got = engine.sos_noise_dev(torch.as_tensor(S0, device="cuda"), torch.as_tensor(sg, device="cuda"), ncoils, seed, offset)
    assert np.allclose(got.cpu().numpy(), want, rtol=1e-13, atol=0)
    assert np.array_equal(engine.sos_noise(S0, sg, ncoils, seed, offset), got.cpu().numpy())   # host entry point


def test_noise_is_a_function_of_seed_and_index():
    import torch
    from microstructure_fingerprinting_amd import engine
    n, k = 100003, 4099        # k is not a multiple of the workgroup size (256)
    S0 = torch.linspace(0.0, 5.0, n, dtype=torch.float64, device="cuda")
    a = engine.sos_noise_dev(S0, 0.7, 2, seed=11)
    assert torch.equal(a, engine.sos_noise_dev(S0, 0.7, 2, seed=11))
    b = engine.sos_noise_dev(S0, 0.7, 2, seed=12)
    assert not torch.equal(a, b) and float((a != b).double().mean()) > 0.999
    lo = engine.sos_noise_dev(S0[:k].contiguous(), 0.7, 2, seed=11)
    hi = engine.sos_noise_dev(S0[k:].contiguous(), 0.7, 2, seed=11, offset=k)
    assert torch.equal(torch.cat([lo, hi]), a)
    assert torch.equal(engine.sos_noise_dev(S0.clone(), 0.7, 2, seed=11, offset=2 ** 40)[:5],
                       engine.sos_noise_dev(S0[:5].contiguous(), 0.7, 2, seed=11, offset=2 ** 40))
    sg = torch.full((n,), 0.7, dtype=torch.float64, device="cuda")
    sg[::7] = 0.0
    S = S0 - 2.0               # negative entries too
    c = engine.sos_noise_dev(S, sg, 3, seed=11)
    want = np.sqrt(3) * np.abs(S.cpu().numpy()[::7])
    assert np.array_equal(c.cpu().numpy()[::7], want)
    assert torch.equal(c[1:7], engine.sos_noise_dev(S, 0.7, 3, seed=11)[1:7])
    inplace = S0.clone()
    assert engine.sos_noise_dev(inplace, 0.7, 2, seed=11, out=inplace) is inplace and torch.equal(inplace, a)


@pytest.mark.parametrize("mode", ["scalar", "voxel", "element"])
def test_fused_noise_equals_predict_then_noise(mode):
    import torch
    from microstructure_fingerprinting_amd import engine
    c = _case("fit_cases")
    d = _dev_args(c)
    clean = engine.predict_dev(*d)
    V, M = clean.shape
    sg = {"scalar": 12.5, "voxel": d[1][:, 0] / 30.0 + 1.0,
          "element": torch.linspace(1.0, 20.0, V * M, dtype=torch.float64, device="cuda").reshape(V, M)}[mode]
    fused = engine.predict_dev(*d, sigma_g=sg, ncoils=4, seed=99, offset=123456789)
    sg_el = sg if mode != "voxel" else sg[:, None].expand(V, M).contiguous()
    two = engine.sos_noise_dev(clean, sg_el, 4, seed=99, offset=123456789)
    assert torch.equal(fused, two)
    assert not torch.equal(fused, clean)
    Y = torch.as_tensor(c["Y"], device="cuda")
    f2, stats = engine.predict_dev(*d, d_Y=Y, sigma_g=sg, ncoils=4, seed=99, offset=123456789)
    assert torch.equal(f2, fused)
    rss = ((Y - fused) ** 2).sum(dim=1)
    assert torch.allclose(stats[:, 0], rss, rtol=1e-12, atol=0)


def test_gen_SoS_MRI_on_the_device():
    import torch
    from microstructure_fingerprinting_amd import engine
    from microstructure_fingerprinting_amd import mf_utils as U
    S0 = np.linspace(0.5, 2.0, 24).reshape(2, 3, 4)
    a = U.gen_SoS_MRI(S0, 0.3, 2, seed=5)
    assert a.shape == S0.shape and a.dtype == np.float64 and np.array_equal(a, U.gen_SoS_MRI(S0, 0.3, 2, seed=5))
    assert np.array_equal(a, U.gen_SoS_MRI(S0, np.full((1, 1), 0.3), 2, seed=5))
    assert np.array_equal(a, U.gen_SoS_MRI(S0, np.full(S0.shape, 0.3), 2, seed=5))
    v = U.gen_SoS_MRI(S0[0, 0], np.full((1, 1), 0.3), 2, seed=5)      # (N,) beside (1, 1)
    assert v.shape == (4,) and np.array_equal(v, a[0, 0])
    t = U.gen_SoS_MRI(torch.as_tensor(S0, device="cuda"), 0.3, 2, seed=5)
    assert torch.is_tensor(t) and t.is_cuda and np.array_equal(t.cpu().numpy(), a)
    assert np.array_equal(a.reshape(-1), engine.sos_noise(S0.reshape(-1), 0.3, 2, seed=5))
    np.random.seed(77)
    r1 = U.gen_SoS_MRI(S0, 0.3)
    r2 = U.gen_SoS_MRI(S0, 0.3)
    np.random.seed(77)
    assert np.array_equal(U.gen_SoS_MRI(S0, 0.3), r1) and not np.array_equal(r1, r2)


# ------------------------------------------------------------------------------------------------
# noise: the distribution (fixed seeds: deterministic)
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S0,sigma,N", [(0.0, 1.0, 1), (1.0, 0.5, 1), (500.0, 500.0 / 30, 1), (3.0, 1.0, 4), (0.2, 1.0, 8)])
def test_noise_distribution(S0, sigma, N):
    """E[Y^2] = N (S0^2 + 2 sigma^2) with standard error sqrt(4 N sigma^2 (sigma^2 + S0^2) / n): |z| <= 5.
    (Y / sigma)^2 is non-central chi-square with 2N degrees of freedom and non-centrality N S0^2 / sigma^2:
    Kolmogorov-Smirnov D sqrt(n) <= 2.  Lag-1 correlation and the correlation between seeds s and s + 1:
    |r| sqrt(n) <= 5.  The reference's generator stays at |z| <= 1.4, D sqrt(n) <= 1.2, |r| sqrt(n) <= 2.8 on these cases."""
    import torch
    from scipy import stats
    from microstructure_fingerprinting_amd import engine
    n = 1 << 20
    seed = 1000 + 10 * N + int(S0)
    s0 = torch.full((n,), S0, dtype=torch.float64, device="cuda")
    y = engine.sos_noise_dev(s0, sigma, N, seed=seed).cpu().numpy()
    y1 = engine.sos_noise_dev(s0, sigma, N, seed=seed + 1).cpu().numpy()
    assert np.all(np.isfinite(y)) and np.all(y >= 0)
    z = (np.mean(y ** 2) - N * (S0 ** 2 + 2 * sigma ** 2)) / np.sqrt(4 * N * sigma ** 2 * (sigma ** 2 + S0 ** 2) / n)
    x = np.sort((y / sigma) ** 2)
    nc = N * S0 ** 2 / sigma ** 2
    cdf = stats.ncx2.cdf(x, 2 * N, nc) if nc > 0 else stats.chi2.cdf(x, 2 * N)
    i = np.arange(1, n + 1)
    D = max(np.max(i / n - cdf), np.max(cdf - (i - 1) / n))
    r_lag = np.corrcoef(y[:-1], y[1:])[0, 1]
    r_seed = np.corrcoef(y, y1)[0, 1]
    print("(S0, sigma, N) = (%g, %g, %d): z = %.2f, D sqrt(n) = %.2f, lag-1 r sqrt(n) = %.2f, seed r sqrt(n) = %.2f"
          % (S0, sigma, N, z, D * np.sqrt(n), r_lag * np.sqrt(n), r_seed * np.sqrt(n)))
    assert abs(z) <= 5
    assert D * np.sqrt(n) <= 2.0
    assert abs(r_lag) * np.sqrt(n) <= 5 and abs(r_seed) * np.sqrt(n) <= 5


# ------------------------------------------------------------------------------------------------
# the loop the feature is for: parameters -> signals -> fit -> parameters, on the device
# ------------------------------------------------------------------------------------------------
def test_predict_then_fit_returns_the_parameters():
    """The noise-free prediction of the recorded two-fascicle rows lies in the dictionary, so the optimum is the
    ground truth: atom indices exactly, M0 and the fractions within RTOL_W (the reference's solver, fed its own y_rec
    of these 6 voxels, returns the same index pairs and the weights to 1.5e-14 of M0)."""
    import torch
    from microstructure_fingerprinting_amd import _lib, engine
    c = _case("fit_c2_small")
    d = _dev_args(c)
    plan, d_params, d_peaks = d[0], d[1], d[2]
    assert d_params.shape[0] == 6
    sig = engine.predict_dev(*d)
    back = engine.fit_batch_dev(plan, sig, d_peaks, 2)
    assert torch.equal(back[:, 3:5], d_params[:, 3:5])
    dev = ((back[:, :3] - d_params[:, :3]).abs() / d_params[:, :3].abs()).max().item()
    print("noise-free refit: max rel. deviation of M0, nu_f0, nu_f1 = %.3g" % dev)
    assert torch.allclose(back[:, :3], d_params[:, :3], rtol=RTOL_W, atol=0)
    # 256 noisy draws per voxel at SNR 50, one fit call
    truth = d_params.repeat_interleave(256, dim=0).contiguous()
    pk = d_peaks.repeat_interleave(256, dim=0).contiguous()
    runs = []
    for _ in range(2):
        noisy = c["model"].simulate(truth, pk, SNR=50, seed=2024, pgse_scheme=c["sch"])
        assert torch.is_tensor(noisy) and noisy.is_cuda and tuple(noisy.shape) == (6 * 256, c["sch"].shape[0])
        est = engine.fit_batch_dev(plan, noisy, pk, 2, check=False)
        _lib.check(_lib.lib().mfx_plan_status(plan.handle(), torch.cuda.current_stream().cuda_stream))   # no status flag
        assert not torch.isnan(est).any() and not torch.isnan(noisy).any()
        runs.append((noisy, est))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    assert not torch.equal(runs[0][0][0], runs[0][0][1])      # the draws of one voxel differ from each other
    m0 = runs[0][1][:, 0].reshape(6, 256).mean(dim=1)
    print("noisy refit at SNR 50: mean M0 / truth = %s" % np.array2string((m0 / d_params[:, 0]).cpu().numpy(), precision=4))
