"""Every fit path on dictionaries and signals stored in other units (tests/_units_cases.py: UNITS).

The reference normalises neither a dictionary nor a signal.  Inside the region where its absolute Cramer tolerance is
inert ("Units"; tests/test_units_host.py measures the boundary and shows the CPU oracle exactly equivariant
at every unit pair used here) a fit at (c, cy) is the baseline fit with M0 -> M0 cy / c and MSE -> MSE cy^2.  The
kernels rank in FP32 / split FP16 and hold a few constants that are absolute in the dictionary's units; every path is
therefore run at every unit pair and compared
  (a) with the oracle at the SAME units - atom indices equal, the other columns within RTOL_W = 1e-5 (test_fit_gpu's
      _check; the classes that go through a Lawson-Hanson solve per tuple in the reference compare an atom index only
      where its compartment is active, as test_parity_stress_gpu does) - on rows brought back to baseline units, so
      that the absolute floors of those comparisons mean what they mean in the other modules;
  (b) for power-of-two units, with the same path's own baseline rows: indices equal, values within RTOL_W (the FP64
      exact stage makes bit-equality the expectation: the count is printed, not asserted).
Fixtures: 2 b0 + 3 shells of 20 / 22 / 43 / 86 directions (M = 62, 68, 131, 260), N = 64 atoms (the smallest
dictionary the batched three-fascicle path takes), E = 4, 16 voxels per class: generic mixtures at SNR 30, a
noise-free one, one with a fascicle absent (N-fold ties), two with a pair of identical peaks; tests/_units_cases.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

import _units_cases as uc
import test_fit_gpu as FG
import test_parity_stress_gpu as PS

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
RTOL_W = FG.RTOL_W
UNIT = {u[0]: u for u in uc.UNITS}

# path -> (class, directions per shell, atoms, [(debug hook, value while the path runs, value afterwards)])
# How each case reaches the kernel it names (dispatch read in csrc/mfx_api.hip and csrc/tu_k2x.hip):
#   small-*        K <= 1 -> fit_class_fused -> launch_small (fit_small.hip), whatever the extra columns.
#   k2s-M62        K = 2, no extra column -> launch_k2: screen on, M <= 256 -> KSm = 4 (M <= 64) -> fit_k2s.hip.
#   k2w-forced     mfx_debug_set_k2_wide(1) and 128 < M = 131 <= 208 -> mfx_launch_k2w_ks13 (fit_k2w.hip).
#   k2w-M260       256 < M = 260 <= 384 with the automatic setting -> mfx_launch_k2w_ks24.
#   k2-fp64        mfx_debug_set_k2_screen(0) -> mfx_launch_k2_f64 (fit_k2.hip).
#   k2x-M62        [N, N, 1] at M = 62: the screening pipeline needs 64 <= M, so either setting of
#                  mfx_debug_set_k2x_screen runs launch_k2x_t<16> (fit_k2x.hip): one case, the switch left alone;
#   k2sx-M68-*     [N, N, 1] at M = 68: screen on -> launch_k2sx_pipeline<50> (the FP32/FP16 pre-screen with its
#                  scr_scale'd tables), screen off -> launch_k2x_t<50>.
#   k2xc-M260      [N, N, 1], 200 < M = 260 < 560 -> launch_k2sx_pipeline<100, ., 4, 1> (the wide kernel's XC form).
#   k2x-NN_E, k2x-NN_1_E   E > 0 -> no pipeline -> launch_k2x_t<16> (fit_k2x.hip).
#   generic-NN_1   mfx_debug_set_force_generic(1): fit_class_dev skips the fused kernels -> fit_class_generic
#                  (materialised dictionary, solve_generic.hip's tuple scan).
#   k3b            K = 3, NX = 0, N = 64 >= 32, N^3 = 2^18 -> k3b_applies -> fit_k3_batched (fit_k3.hip).
#   k3-unscreened  mfx_debug_set_k3_screen(0) -> fit_class_generic with k3 = false: one thread per triple.
#   k3b-cap4       mfx_debug_set_k3_cap(4): a voxel that lists more than 4 triples (its threshold rises while the
#                  screen appends; the absent fascicle's atoms tie 64-fold) sets its overflow flag, and the gated
#                  launch_solver fallback (solve_k3.hip's screen, itself backed by the scan) redoes it.  The library
#                  counts those voxels (mfx_debug_last_counter(6)): the test requires one at least (9 of the 16 at
#                  every unit pair when this was written) and none in the plain k3b case (2^18 triples < the 4 M cap).
#   generic-NNN_1  NX = 1 -> k3b_applies false -> fit_class_generic, Kp = 4 -> plain tuple scan, _4up finalize.
# (MFX_K3_BATCH=0 is an environment switch read once per thread: test_three_fascicles_one_by_one_in_a_child.)
PATHS = {
    "small-N": ("N", 20, 64, []), "small-N_1": ("N_1", 20, 64, []), "small-N_E": ("N_E", 20, 64, []),
    "small-N_1_E": ("N_1_E", 20, 64, []),
    "k2s-M62": ("NN", 20, 64, []),
    "k2w-forced-M131": ("NN", 43, 64, [("mfx_debug_set_k2_wide", 1, -1)]),
    "k2w-M260": ("NN", 86, 64, []),
    "k2-fp64-M62": ("NN", 20, 64, [("mfx_debug_set_k2_screen", 0, 1)]),
    "k2x-M62": ("NN_1", 20, 64, []),
    "k2sx-M68-screen-on": ("NN_1", 22, 64, [("mfx_debug_set_k2x_screen", 1, 1)]),
    "k2sx-M68-screen-off": ("NN_1", 22, 64, [("mfx_debug_set_k2x_screen", 0, 1)]),
    "k2xc-M260": ("NN_1", 86, 64, []),
    "k2x-NN_E": ("NN_E", 20, 64, []),
    "k2x-NN_1_E": ("NN_1_E", 20, 64, []),
    "generic-NN_1": ("NN_1", 20, 64, [("mfx_debug_set_force_generic", 1, 0)]),
    "k3b": ("NNN", 20, 64, []),
    "k3-unscreened": ("NNN", 20, 64, [("mfx_debug_set_k3_screen", 0, 1)]),
    "k3b-cap4": ("NNN", 20, 64, [("mfx_debug_set_k3_cap", 4, 0)]),
    "generic-NNN_1": ("NNN_1", 20, 40, []),
}
_plans, _gpu, _redone = {}, {}, {}


def _plan(mdl, c):
    from microstructure_fingerprinting_amd import mf_utils as mfu
    key = (mdl["key"], c)
    if key not in _plans:
        ms = mfu.init_PGSE_multishell_interp(mdl["dic"] * c, mdl["sch"], uc.Z)
        _plans[key] = (ms, ms.plan_for(mdl["sch"]))
    return _plans[key][1]


def _fit(mdl, cls, c, cy):
    from microstructure_fingerprinting_amd import engine
    peaks, Y = uc.voxels(mdl, cls)
    Kv, cm, em, maxfasc, csf_on, ear_on, sc, se, ne = uc.fit_args(mdl, cls, Y.shape[0], c)
    return engine.fit_batch(_plan(mdl, c), Y * cy, Kv, cm, em, peaks, maxfasc, csf_on, ear_on, sc, se, ne)


def _gpu_rows(path, c, cy):
    """the library's rows of a path at (c, cy), its debug hooks set for the call and restored behind it"""
    from microstructure_fingerprinting_amd import _lib as L
    key = (path, c, cy)
    if key not in _gpu:
        cls, dirs, N, hooks = PATHS[path]
        lib = L.lib()
        try:
            for name, on, _ in hooks:
                getattr(lib, name)(on)
            _gpu[key] = _fit(uc.model(dirs, N), cls, c, cy)
            _redone[key] = lib.mfx_debug_last_counter(6)    # voxels of the batched K = 3 path redone after a list overflow
        finally:
            for name, _, off in hooks:
                getattr(lib, name)(off)
    return _gpu[key]


def _compare(got, ref, cls, what):
    """comparison (a) of the module docstring, on rows in baseline units"""
    K, c, e = uc.CLASSES[cls]
    maxfasc = max(K, 1)
    assert np.all(np.isfinite(got)), what
    if K + c + e >= 4:       # _4up in the reference
        ear = (2 * maxfasc + c + 1, 2 * maxfasc + c + 2) if e else None
        PS._assert_rows(got, ref, maxfasc, what, rtol=RTOL_W, ids_where_active=True, ear=ear)
        return
    try:
        FG._check(got, ref, maxfasc)
    except AssertionError as ex:
        ids = slice(1 + maxfasc, 1 + 2 * maxfasc)
        bad = np.where(np.any(got[:, ids] != ref[:, ids], axis=1) | ~np.all(np.isclose(got, ref, rtol=RTOL_W, atol=1e-10), axis=1))[0]
        raise AssertionError("%s: %s; voxels %s\ngot\n%s\nexpected\n%s" % (what, ex, bad[:6], got[bad[:3]], ref[bad[:3]]))
    if e:
        col = 2 * maxfasc + c + 2
        assert np.array_equal(got[:, col], ref[:, col]), "%s: EAR indices differ" % what


def _check_unit(path, cls, got_at, base_at, ref_at, unit):
    name, c, cy, pow2 = UNIT[unit]
    got = uc.to_baseline(got_at(c, cy), c, cy)
    _compare(got, uc.to_baseline(ref_at(c, cy), c, cy), cls, "%s at %s against the oracle" % (path, name))
    if pow2:
        base = base_at()
        _compare(got, base, cls, "%s at %s against its own baseline rows" % (path, name))
        print("%s at %s: %d of %d rows bit-equal to the baseline's" % (path, name, int(np.sum(np.all(got == base, axis=1))), got.shape[0]))


@pytest.mark.parametrize("unit", uc.UNIT_IDS)
@pytest.mark.parametrize("path", sorted(PATHS))
def test_fit_path_at_other_units(path, unit):
    """One fit path (PATHS: the comment above says how each case reaches its kernel) at one unit pair: (a) and (b)."""
    cls, dirs, N, _ = PATHS[path]
    mdl = uc.model(dirs, N)
    _check_unit(path, cls, lambda c, cy: _gpu_rows(path, c, cy), lambda: _gpu_rows(path, 1.0, 1.0),
                lambda c, cy: uc.oracle_rows(mdl, cls, c, cy), unit)
    if path in ("k3b", "k3b-cap4"):
        n = _redone[(path,) + UNIT[unit][1:3]]
        print("%s at %s: %d of %d voxels redone by the gated fallback" % (path, unit, n, uc.nvox(cls)))
        assert n >= 1 if path == "k3b-cap4" else n == 0


# ---- MFX_K3_BATCH=0: an environment switch, read once per thread - a fresh child process fits every unit pair
def _child_k3_nobatch(out):
    mdl = uc.model(20, 64)
    res = {"base": _fit(mdl, "NNN", 1.0, 1.0)}
    for name, c, cy, _ in uc.UNITS:
        res[name] = _fit(mdl, "NNN", c, cy)
    np.savez(out, **res)


@pytest.fixture(scope="module")
def k3_nobatch_rows(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("units") / "k3_nobatch.npz")
    code = "import sys; sys.path[:0] = [%r, %r]; import test_units_gpu as t; t._child_k3_nobatch(%r)" % (HERE, ROOT, out)
    p = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, MFX_K3_BATCH="0"), capture_output=True, text=True,
                       timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    return dict(np.load(out))


@pytest.mark.parametrize("unit", uc.UNIT_IDS)
def test_three_fascicles_one_by_one_in_a_child(k3_nobatch_rows, unit):
    """MFX_K3_BATCH=0: fit_class_fused sends K = 3 to fit_class_generic, where k3_applies holds (three sub-dictionaries
    of 64 >= 16 atoms, 64^3 = 2^18 triples) -> solve_k3.hip's FP32 relaxed-bound screen, voxel by voxel."""
    mdl = uc.model(20, 64)
    _check_unit("k3-one-by-one", "NNN", lambda c, cy: k3_nobatch_rows[unit], lambda: k3_nobatch_rows["base"],
                lambda c, cy: uc.oracle_rows(mdl, "NNN", c, cy), unit)


# ---- mf_utils.solve_exhaustive_posweights on explicit dictionaries
SOLVE = {"64x64": (64, [64, 64]), "64x64x1": (64, [64, 64, 1]), "64x64x64": (64, [64, 64, 64]), "16x16x16x2": (16, [16, 16, 16, 2])}
_solve = {}


def _solve_problem(name):
    """(A, Y [3, M], sizes) at baseline units: oracle rotations of the M = 62 model (+ the CSF column, + two EAR columns);
    a generic mixture at SNR 30, a noise-free one, one whose last fascicle is absent (its atoms tie)."""
    if name not in _solve:
        from microstructure_fingerprinting_amd import synth
        from oracle import oracle as orc
        N, sizes = SOLVE[name]
        mdl = uc.model(20, N)
        rng = np.random.default_rng(300 + len(sizes) + N)
        T = uc.tables(mdl, 1.0)
        cols = []
        for s in sizes:
            cols.append(orc.interp(mdl["sch"], synth.unit_vectors(rng, 1)[0], T) if s == N else
                        (mdl["sig_csf"][:, None] if s == 1 else mdl["sig_ear"][:, :2]))
        A = np.ascontiguousarray(np.concatenate(cols, axis=1))
        st = np.concatenate([[0], np.cumsum(sizes)[:-1]])
        Y = np.zeros((3, mdl["M"]))
        for i in range(3):
            nu = rng.dirichlet(2.0 * np.ones(len(sizes)))
            if i == 2:
                nu[sizes.count(N) - 1] = 0.0
            Y[i] = 500.0 * A[:, st + np.array([rng.integers(0, s) for s in sizes])] @ nu
            if i != 1:
                Y[i] += rng.normal(0, 500.0 / 30.0, mdl["M"])
        _solve[name] = (A, Y, np.array(sizes))
    return _solve[name]


@pytest.mark.parametrize("unit", uc.UNIT_IDS)
@pytest.mark.parametrize("name", sorted(SOLVE))
def test_explicit_solver_at_other_units(name, unit):
    """mfx_solve_exhaustive: [64, 64], [64, 64, 1] and [16, 16, 16, 2] take the plain tuple scan of solve_generic.hip
    (k3_applies needs three sub-dictionaries), [64, 64, 64] - 2^18 triples, every sub-dictionary >= 16 atoms - takes
    solve_k3.hip's screen.  (a) against the oracle at the same units, (b) against the library's own baseline result;
    weights in baseline units, objective over cy^2."""
    from microstructure_fingerprinting_amd import mf_utils as mfu
    from oracle import oracle as orc
    uname, c, cy, pow2 = UNIT[unit]
    A, Y, sizes = _solve_problem(name)
    four = sizes.size >= 4
    for i in range(Y.shape[0]):
        w, sub, tot, mo, yrec = mfu.solve_exhaustive_posweights(A * c, Y[i] * cy, sizes)
        refs = [("the oracle", orc.solve_exhaustive_posweights(A * c, Y[i] * cy, sizes), c, cy)]
        if pow2:
            refs.append(("its own baseline", mfu.solve_exhaustive_posweights(A, Y[i], sizes), 1.0, 1.0))
        assert np.all(np.isfinite(w)) and np.isfinite(mo)
        for what, (wr, subr, totr, mor, yrecr), cr, cyr in refs:
            msg = "%s signal %d at %s against %s: %s %s | %s %s" % (name, i, uname, what, sub, w, subr, wr)
            act = (wr > 1e-9 * np.abs(wr).max()) if four else np.ones(sizes.size, bool)
            assert np.array_equal(np.asarray(sub)[act], np.asarray(subr)[act]), msg
            assert np.allclose(w * c / cy, wr * cr / cyr, rtol=RTOL_W, atol=1e-10), msg
            assert np.isclose(mo / cy / cy, mor / cyr / cyr, rtol=RTOL_W, atol=1e-10), msg
            assert np.allclose(yrec / cy, yrecr / cyr, rtol=RTOL_W, atol=1e-10), msg


# ---- the FP64-only paths: 2-D protocols and weighted fits against their own baseline
@pytest.mark.parametrize("ec,ey", [(16, 0), (-10, 34)])
@pytest.mark.parametrize("K", [1, 2])
def test_fit2d_at_other_units(K, ec, ey):
    """engine.fit2d on the smallest fixture of test_fit2d_gpu (syn2, 72 atoms, 24 voxels): rows at (2^ec, 2^ey), in
    baseline units, against the rows at (1, 1) with that module's assert_rows."""
    import test_fit2d_gpu as F2
    from microstructure_fingerprinting_amd import engine
    from microstructure_fingerprinting_amd import mf_utils as U
    c, cy = 2.0 ** ec, 2.0 ** ey
    sch = np.load(os.path.join(F2.G, "rot2d_cases.npz"))["syn2_sch"]
    dic = F2.atoms(sch, 72, 6)
    T1 = U.RotateAtom2DTables(dic, sch, F2.Z, F2.DIFF)
    Y, peaks = F2.two_fascicle_voxels(T1, np.random.default_rng(7), 24, 0.1)
    pk = np.ascontiguousarray(peaks[:, :3 * K])
    base, st = engine.fit2d(T1, Y, np.full(24, K), None, pk, K, False)
    assert np.all(st == 0)
    Tu = U.RotateAtom2DTables(dic * c, sch, F2.Z, F2.DIFF)
    got, st = engine.fit2d(Tu, Y * cy, np.full(24, K), None, pk, K, False)
    assert np.all(st == 0)
    F2.assert_rows(uc.to_baseline(got, c, cy), base, K, "fit2d K=%d at 2^%d, 2^%d" % (K, ec, ey))


@pytest.mark.parametrize("ec,ey", [(16, 0), (-10, 34)])
@pytest.mark.parametrize("K", [1, 2])
def test_fit_weighted_at_other_units(K, ec, ey):
    """engine.fit_weighted on the smallest fixture of test_wfit_gpu ("trim": 48 atoms, 197 rows, 16 voxels with 0/1 masks
    and general weights): rows at (2^ec, 2^ey), in baseline units, against the rows at (1, 1) with that suite's
    assert_rows."""
    import _wfit_ref as R
    import test_wfit_gpu as WG
    from microstructure_fingerprinting_amd import engine, synth
    from microstructure_fingerprinting_amd import mf_utils as mfu
    from oracle import oracle as orc
    c, cy = 2.0 ** ec, 2.0 ** ey
    sch, dic, _ = synth.make_model("C2", 48)
    sub = np.ascontiguousarray(sch[:197])
    peaks, Y, W = WG.make_voxels(orc.init_tables(dic, sch, R.Z), sub, 16, np.random.default_rng(12))
    pk = np.ascontiguousarray(peaks[:, :3 * K])
    rows = []
    for cc, ccy in ((1.0, 1.0), (c, cy)):
        ms = mfu.init_PGSE_multishell_interp(dic * cc, sch, R.Z)
        plan = ms.plan_for(sub)
        got, st = engine.fit_weighted(plan, Y * ccy, W, np.full(16, K), None, pk, K, False)
        assert np.all(st == 0)
        rows.append(uc.to_baseline(got, cc, ccy))
    R.assert_rows(rows[1], rows[0], K, "fit_weighted K=%d at 2^%d, 2^%d" % (K, ec, ey))


# ---- below the boundary: what any policy must satisfy
@pytest.mark.parametrize("path", ["k2x-M62", "k3b"])
def test_tolerance_regime_rows_are_finite_and_consistent(path):
    """[N, N, 1] and [N, N, N] at (2^-14, 1), q = -70: the reference's absolute tolerance accepts unconstrained solutions
    there (negative weights), the library ranks with D >= 0 and decides with the tolerance, so it is neither the reference
    nor a plain NNLS ("Units") and no parity is asserted.  Asserted: every row is finite, and the returned MSE
    is the explicit residual of the returned M0, fractions and atoms on the oracle's rotations, recomputed in NumPy
    longdouble, to 1e-9 relative (floor (1e-12 |y|)^2 / M: a noise-free voxel's residual is rounding itself)."""
    from oracle import oracle as orc
    name, c, cy, _ = uc.TOLERANCE_REGIME
    cls, dirs, N, _ = PATHS[path]
    K, cs, _ = uc.CLASSES[cls]
    mdl = uc.model(dirs, N)
    got = _gpu_rows(path, c, cy)
    ref = uc.oracle_rows(mdl, cls, c, cy)
    assert np.all(np.isfinite(got))
    peaks, Y = uc.voxels(mdl, cls)
    T = uc.tables(mdl, c)
    M = mdl["M"]
    for v in range(Y.shape[0]):
        cols = [orc.interp(mdl["sch"], peaks[v, 3 * k:3 * k + 3], T)[:, int(got[v, 1 + K + k])] for k in range(K)]
        nu = list(got[v, 1:1 + K])
        if cs:
            cols.append(mdl["sig_csf"] * c)
            nu.append(got[v, 2 * K + 1])
        y = (Y[v] * cy).astype(np.longdouble)
        r = y - sum(np.longdouble(got[v, 0]) * np.longdouble(f) * col.astype(np.longdouble) for f, col in zip(nu, cols))
        mse = float(np.sum(r * r) / M)
        floor = float(np.sum(y * y)) * 1e-24 / M
        assert abs(got[v, -2] - mse) <= 1e-9 * mse + floor, (path, v, got[v, -2], mse)
    same = int(np.sum(np.all(np.isclose(got, ref, rtol=RTOL_W, atol=0), axis=1)))
    neg = int(np.sum(np.any(ref[:, uc.weight_columns(cls)] < 0, axis=1)))
    print("%s at %s: %d of %d rows equal the oracle's; %d oracle rows carry a negative weight" % (path, name, same, got.shape[0], neg))
