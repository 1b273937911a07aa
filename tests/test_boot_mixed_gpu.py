"""Where a class's numbers land in a mixed batch, for the four bootstrap entry points (mfx_boot_fit, mfx_wboot_fit,
mfx_boot2d_fit, mfx_wboot2d_fit): the mixed entry point runs once, every class then runs on its own through the device
entry point of its family keyed by the voxels' batch indices, and the mixed result must equal, bit for bit, what is
assembled here in NumPy from the per-class results - by the documented column names (engine.boot_columns for the
statistics, PARAM_NAMES below for the parameter rows: include/mfx.h's layout), not by index formulas.

The rule of the assembly (include/mfx_boot.h): a column the class does not have is, for a weight, 0 in every replicate
(n = B, mean, min, max and quantiles 0, std 0 or NaN for B = 1) and, for a property, never valid (n = 0, the rest NaN); a
voxel in a non-zero status has n = 0 and NaN everywhere; agree is 0 beyond the class's fascicles; the replicate rows are 0
(NaN for a non-zero status) outside the class's columns.

Batches: every class the family serves (K in 0..3, CSF, and EAR for the plain family), two classes of 5 voxels and the
others of 1 or 2, in a shuffled order; B = 3, two quantiles, one property table, keep = True, max_bytes = 1, so that a
chunk of the mixed entry point holds 4 voxels and the 5-voxel classes cross a chunk.  The plain and weighted families run
on the 14 atoms and 64 rows of tests/golden/fit_cases.npz, the 2-D families on the 12-atom tables of
tests/test_boot2d_gpu.py; weights are tests/_wboot2d_cases.py's (per voxel for one family, one shared vector for the
other).  Nothing here restates the resampling rule, so tests/_wboot_ref.py has nothing to give.  Every voxel of these
batches is fine (status 0, asserted): the fill of a voxel in a non-zero status is checked cell by cell without a device in
tests/boot_batch_check.cpp, and on the device by the unusable-voxel tests of the four families."""
import numpy as np
import pytest

import _boot_ref as R
import _wboot2d_cases as C

pytestmark = pytest.mark.gpu

B, Q, SEED, F = 3, (0.25, 0.9), 5, 3
FAMILIES = {            # family: (kind, the own fit handed in as params)
    "boot": ("residual", True),
    "wboot": ("wild", False),
    "boot2d": ("wild", True),
    "wboot2d": ("residual", False),
}
KEYS = ("replicates", "stats", "agree", "status", "dir_status")


def param_names(maxfasc, csf_on, ear_on):
    """The names of a parameter row's entries (include/mfx.h): M0, the fascicles' weights, their atoms, the CSF weight, the
    EAR weight and its atom, MSE, R2."""
    names = ["M0"] + ["nu_%d" % k for k in range(maxfasc)] + ["id_%d" % k for k in range(maxfasc)]
    names += ["nu_csf"] if csf_on else []
    names += ["nu_ear", "id_ear"] if ear_on else []
    return names + ["MSE", "R2"]


def t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def class_list(with_ear):
    """(K, csf, ear) per voxel: every class, (2, 0, 0) and (1, 1, 0) five times, the others once or twice, shuffled."""
    vox = []
    n = 0
    for k in range(F + 1):
        for c in (0, 1):
            for e in ((0, 1) if with_ear else (0,)):
                if (k, c, e) in ((2, 0, 0), (1, 1, 0)):
                    count = 5
                else:
                    n += 1
                    count = 1 + n % 2
                vox += [(k, c, e)] * count
    order = np.random.default_rng(17).permutation(len(vox))
    cls = np.array(vox)[order]
    return cls[:, 0].astype(np.int32), cls[:, 1].astype(bool), cls[:, 2].astype(bool)


def unit_dirs(rng, zmin=0.1):
    """Three unit directions away from the transverse plane and from each other."""
    while True:
        d = rng.standard_normal((3, 3))
        d /= np.sqrt(np.sum(d ** 2, axis=1, keepdims=True))
        if np.all(np.abs(d[:, 2]) >= zmin) and all(abs(d[a] @ d[b]) <= 0.85 for a in range(3) for b in range(a)):
            return d


def batch(family):
    """The mixed batch of a family: a dict of what its entry points take."""
    from microstructure_fingerprinting_amd import engine
    rng = np.random.default_rng(23)
    two_d = family.endswith("2d")
    K, csf, ear = class_list(family == "boot")
    V = K.size
    peaks = np.stack([unit_dirs(rng).reshape(-1) for _ in range(V)])
    c = dict(family=family, K=K, csf=csf, ear=ear, V=V, peaks=peaks, with_ear=family == "boot")
    if two_d:
        import test_boot2d_gpu as B2
        import test_fit2d_gpu as F2
        T = B2.tables("syn2", 12, 21)
        sch = B2.rot_npz()["syn2_sch"]
        c.update(T=T, M=T.M, N=T.N, sig_csf=F2.csf_signal(sch), sig_ear=None, E=0)
        c["groups"] = np.unique(sch[:, 3:6], axis=0, return_inverse=True)[1].reshape(-1).astype(np.int32)
        Y = np.zeros((V, T.M))
        for v in range(V):
            cols = T.rotate_cols(peaks[v].reshape(3, 3), rng.integers(0, T.N, 3))
            Y[v] = F2.rician(rng, 0.4 * cols[0] + 0.35 * cols[1] + 0.25 * cols[2])
        Y[csf] = 0.8 * Y[csf] + 0.2 * c["sig_csf"]
        c["props"] = np.linspace(0.5, 4.0, T.N)[None, :]
    else:
        from microstructure_fingerprinting_amd import mf_utils as mfu
        d, sch, sig_csf, sig_ear = R.golden_model()
        ms = mfu.init_PGSE_multishell_interp(d["dictionary"], d["sch_ms"], R.Z)
        c.update(ms=ms, T=ms.plan_for(sch), M=sch.shape[0], N=int(d["N"]), sig_csf=sig_csf,
                 sig_ear=np.ascontiguousarray(sig_ear), E=int(d["E"]))
        c["groups"] = engine.boot_groups(sch)
        Y = d["Y"][np.arange(V) % d["Y"].shape[0]] * rng.uniform(0.95, 1.05, (V, c["M"]))
        c["props"] = np.ascontiguousarray(d["rad"][None, :])
    c["Y"] = np.ascontiguousarray(Y)
    assert len(np.unique(c["groups"])) > 1
    if family == "wboot":
        c["W"] = C.weights("smooth", V, c["M"], 31)
    if family == "wboot2d":
        c["W"] = C.weights("shared", V, c["M"], 32)
    return c


def own_fit(c):
    """The voxels' own fit in the batch's layout (the families that hand it in are the unweighted ones)."""
    from microstructure_fingerprinting_amd import engine
    if c["family"] == "boot":
        return engine.fit_batch(c["T"], c["Y"], c["K"], c["csf"], c["ear"], c["peaks"], F, True, True, c["sig_csf"], c["sig_ear"], c["E"])
    assert c["family"] == "boot2d"
    rows, st = engine.fit2d(c["T"], c["Y"], c["K"], c["csf"], c["peaks"], F, True, c["sig_csf"])
    assert not st.any()
    return rows


def mixed(c, kind, params):
    from microstructure_fingerprinting_amd import engine
    kw = dict(B=B, kind=kind, seed=SEED, q=Q, props=c["props"], groups=c["groups"], params=params, max_bytes=1, keep=True)
    fam = c["family"]
    if fam == "boot":
        return engine.fit_bootstrap(c["T"], c["Y"], c["K"], c["csf"], c["ear"], c["peaks"], F, True, True, c["sig_csf"], c["sig_ear"],
                                    c["E"], **kw)
    if fam == "wboot":
        return engine.fit_weighted_bootstrap(c["T"], c["Y"], c["W"], c["K"], c["csf"], c["peaks"], F, True, c["sig_csf"], **kw)
    if fam == "boot2d":
        return engine.fit2d_bootstrap(c["T"], c["Y"], c["K"], c["csf"], c["peaks"], F, True, c["sig_csf"], **kw)
    return engine.fit2d_weighted_bootstrap(c["T"], c["Y"], c["W"], c["K"], c["csf"], c["peaks"], F, True, c["sig_csf"], **kw)


def one_class(c, kind, k, cf, e, ix, params):
    """The device entry point of the family on the voxels ix of class (k, cf, e): a dict of NumPy arrays."""
    import torch
    from microstructure_fingerprinting_amd import engine
    kw = dict(B=B, kind=kind, seed=SEED, q=Q, d_props=t(c["props"]), d_groups=t(c["groups"]), d_vox=t(ix.astype(np.int64)), keep=True,
              d_params=None if params is None else t(params))
    fam = c["family"]
    Y, pk = t(c["Y"][ix]), (t(c["peaks"][ix, :3 * k]) if k else None)
    sc = t(c["sig_csf"]) if cf else None
    if fam in ("wboot", "wboot2d"):
        W = t(c["W"] if c["W"].ndim == 1 else c["W"][ix])
    if fam == "boot":
        r = engine.fit_bootstrap_dev(c["T"], Y, pk, k, bool(cf), bool(e), sc, t(c["sig_ear"]) if e else None, c["E"] if e else 0, **kw)
    elif fam == "wboot":
        r = engine.fit_weighted_bootstrap_dev(c["T"], Y, W, pk, k, bool(cf), sc, **kw)
    elif fam == "boot2d":
        r = engine.fit2d_bootstrap_dev(c["T"], Y, pk, k, bool(cf), sc, **kw)
    else:
        r = engine.fit2d_weighted_bootstrap_dev(c["T"], Y, W, pk, k, bool(cf), sc, **kw)
    torch.cuda.synchronize()
    return {key: (val.cpu().numpy() if hasattr(val, "cpu") else val) for key, val in r.items()}


def run_case(family):
    """(the mixed entry point's result, the assembly of the per-class results), dicts over KEYS."""
    from microstructure_fingerprinting_amd import engine
    kind, give = FAMILIES[family]
    c = batch(family)
    V, e_on = c["V"], c["with_ear"]
    P0 = own_fit(c) if give else None
    got = mixed(c, kind, P0)
    names_F = param_names(F, True, e_on)
    cols_F = engine.boot_columns(F, True, e_on, 1)
    assert got["columns"] == cols_F and got["replicates"].shape == (V, B, len(names_F))
    NS = 5 + len(Q)
    want = dict(replicates=np.full((V, B, len(names_F)), -7.0), stats=np.full((V, len(cols_F), NS), -7.0),
                agree=np.full((V, F), -7, dtype=np.int32), status=np.full(V, -7, dtype=np.int32))
    if "dir_status" in got:
        want["dir_status"] = np.full((V, 5), -7, dtype=np.int32)
    absent_weight = np.array([float(B), 0.0, 0.0 if B > 1 else np.nan, 0.0, 0.0] + [0.0] * len(Q))
    never_valid = np.array([0.0] + [np.nan] * (NS - 1))
    sizes = []
    for k in range(F + 1):
        for cf in (0, 1):
            for e in ((0, 1) if e_on else (0,)):
                ix = np.flatnonzero((c["K"] == k) & (c["csf"] == bool(cf)) & (c["ear"] == bool(e)))
                sizes.append(ix.size)
                names = param_names(k, cf, e)
                pcols = [names_F.index(n) for n in names]
                r = one_class(c, kind, k, cf, e, ix, None if P0 is None else P0[np.ix_(ix, pcols)])
                ccols = [cols_F.index(n) for n in r["columns"]]
                ok = r["status"] == 0
                want["status"][ix] = r["status"]
                for j, name in enumerate(cols_F):
                    weight = not isinstance(name, tuple)
                    want["stats"][ix, j] = np.where(ok[:, None], absent_weight, never_valid) if weight else never_valid
                want["stats"][np.ix_(ix, ccols)] = r["stats"]
                want["agree"][ix] = 0
                want["agree"][ix, :k] = r["agree"]
                want["replicates"][ix] = np.where(ok, 0.0, np.nan)[:, None, None]
                want["replicates"][np.ix_(ix, np.arange(B), pcols)] = r["replicates"]
                if "dir_status" in want:
                    want["dir_status"][ix] = r["dir_status"]
    assert sorted(sizes)[-2:] == [5, 5] and min(sizes) >= 1 and max(sorted(sizes)[:-2]) <= 2 and sum(sizes) == V
    return got, want


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_mixed_batch_is_the_assembly_of_its_classes(family):
    got, want = run_case(family)
    assert np.any(got["replicates"][:, 1:] != got["replicates"][:, :1])          # the replicates are not copies of one row
    assert not got["status"].any()
    for key in KEYS:
        if key == "dir_status" and not family.endswith("2d"):
            assert key not in got
            continue
        assert got[key].shape == want[key].shape and got[key].dtype == want[key].dtype, key
        assert np.array_equal(got[key], want[key], equal_nan=(got[key].dtype.kind == "f")), key
