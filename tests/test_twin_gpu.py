"""Every fit path on dictionaries of near-twin atoms (tests/_twin_cases.py; tests/test_twin_host.py guards the
population's power on the oracle alone).

Every fast path ranks in low precision, protects the arg-min with a margin and decides a short list in FP64.  Here a
runner-up within the margin of the optimum is, in about half of the voxels, scanned first, so that the optimum has to
pass the low-precision test with almost no slack ("margin" ladder), and whole families lie inside the library's tie
window 1e-9 |y|^2 ("window" ladder), where the short lists fill and the hand-backs, the exhaustive exact passes and the
overflow fallback decide.  The paths are those of test_units_gpu.PATHS (its comment says how each case reaches its
kernel), each on both family shapes (N/2 x 2 and 8 x 8) and both ladders; VARIANTS adds, on the window ladder, the
debug hooks that force the hand-backs.

Comparisons, the CPU oracle the referee:
  * classes that the reference solves by Cramer (K + csf + ear <= 3): atom (and EAR) indices equal in EVERY voxel, the
    other columns within RTOL_W (test_fit_gpu._check, as test_units_gpu._compare does);
    mf_utils.solve_exhaustive_posweights bit for bit;
  * classes with four or more sub-dictionaries (a third-party NNLS per tuple in the reference, which does not define the
    order of rounding-level ties): indices equal wherever the compartment is active and the voxel's gap exceeds the tie
    window; below it another tuple is accepted only if its objective, re-scored by orc.nnls on the oracle's columns, does
    not exceed the oracle's min_obj by more than _twin_cases.INCONSISTENCY |y|^2.  The number of voxels that used this
    clause is printed.
Per path the fallback, guard and hand-back counters are printed; nothing is asserted on them but the overflow count of
the batched three-fascicle path."""
import numpy as np
import pytest

import _twin_cases as tc
import _units_cases as uc
import _wfit_ref as R
import test_parity_stress_gpu as PS
import test_solver_ties_gpu as TG
import test_units_gpu as UG

pytestmark = pytest.mark.gpu

RTOL_W = UG.RTOL_W

# variant -> (path of UG.PATHS, further debug hooks: (name, value while the path runs, value afterwards)); window ladder.
#   +cap4     mfx_debug_set_k2s_cap(4): a split-FP16 screen (fit_k2s.hip, fit_k2w.hip, the [N, N, 1] pipeline) that
#             lists more than 4 pairs hands the voxel back to the FP64 kernel;
#   +maxc0    mfx_debug_set_k2_maxc(0): the FP64 kernel's exhaustive exact pass (fit_k2.hip);
#   +xmaxc0   mfx_debug_set_k2x_maxc(0): fit_k2x.hip's exhaustive exact pass.
VARIANTS = {p + "+cap4": (p, [("mfx_debug_set_k2s_cap", 4, 0)])
            for p in ("k2s-M62", "k2w-forced-M131", "k2w-M260", "k2sx-M68-screen-on", "k2xc-M260")}
VARIANTS["k2-fp64-M62+maxc0"] = ("k2-fp64-M62", [("mfx_debug_set_k2_maxc", 0, -1)])
VARIANTS.update({p + "+xmaxc0": (p, [("mfx_debug_set_k2x_maxc", 0, -1)])
                 for p in ("k2x-M62", "k2sx-M68-screen-off", "k2x-NN_E", "k2x-NN_1_E")})

CASES = [(p, nb, cp, ladder) for p in sorted(UG.PATHS) for nb, cp in tc.shapes(UG.PATHS[p][2]) for ladder in sorted(tc.LADDERS)]
CASES += [(v, nb, cp, "window") for v in sorted(VARIANTS) for nb, cp in tc.shapes(UG.PATHS[VARIANTS[v][0]][2])]


def _case_id(c):
    return "%s-%dx%d-%s" % c


def _gpu_rows(name, mdl):
    """(rows, counters) of a path or variant on a model, its debug hooks set for the call and restored behind it"""
    from microstructure_fingerprinting_amd import _lib as L
    from microstructure_fingerprinting_amd import engine
    path, more = VARIANTS.get(name, (name, []))
    cls, _, _, hooks = UG.PATHS[path]
    hooks = list(hooks) + more
    lib = L.lib()
    peaks, Y = tc.voxels(mdl, cls)
    Kv, cm, em, maxfasc, csf_on, ear_on, sc, se, ne = uc.fit_args(mdl, cls, Y.shape[0], 1.0)
    try:
        for hook, on, _ in hooks:
            getattr(lib, hook)(on)
        got = engine.fit_batch(UG._plan(mdl, 1.0), Y, Kv, cm, em, peaks, maxfasc, csf_on, ear_on, sc, se, ne)
        counters = {"fallback": lib.mfx_debug_last_fallback_count(), "guard": lib.mfx_debug_last_guard_count(),
                    "counter 5": lib.mfx_debug_last_counter(5), "redone": lib.mfx_debug_last_counter(6)}
    finally:
        for hook, _, off in hooks:
            getattr(lib, hook)(off)
    return got, counters


def _compare_4up(got, ref, mdl, cls, what):
    """the second comparison of the module docstring; returns the number of voxels accepted below the tie window"""
    K, c, e = uc.CLASSES[cls]
    mf = max(K, 1)
    ids = slice(1 + mf, 1 + mf + K)
    cn, ce = 2 * mf + c + 1, 2 * mf + c + 2          # nu_ear, EAR index
    assert np.all(np.isfinite(got)), what
    peaks, Y = tc.voxels(mdl, cls)
    gap = tc.gap_and_order(mdl, cls)["gap"]
    active = ref[:, 1:1 + K] > 1e-9
    differs = np.any((got[:, ids] != ref[:, ids]) & active, axis=1)
    if e:
        differs |= (got[:, ce] != ref[:, ce]) & (ref[:, cn] > 1e-9)
    for v in np.flatnonzero(differs):
        msg = "%s voxel %d: got %s, oracle %s, gap %.3e |y|^2" % (what, v, got[v], ref[v], gap[v])
        assert gap[v] <= tc.TIE_WINDOW, msg
        y = np.ascontiguousarray(Y[v])
        extras = ([mdl["sig_csf"]] if c else []) + ([mdl["sig_ear"][:, int(got[v, ce])]] if e else [])
        obj = tc.rescore(tc.rotated(mdl, peaks[v], K), [int(a) for a in got[v, ids]], extras, y)
        excess = (obj - ref[v, -2] * mdl["M"]) / float(np.sum(y * y))
        assert excess <= tc.INCONSISTENCY, "%s: its objective exceeds the oracle's by %.3e |y|^2" % (msg, excess)
        assert np.isclose(got[v, -2], ref[v, -2], rtol=RTOL_W, atol=1e-9), msg
    same = ~differs
    PS._assert_rows(got[same], ref[same], mf, what, rtol=RTOL_W, ids_where_active=True, ear=(cn, ce) if e else None)
    return int(differs.sum())


@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_fit_path_on_twins(case):
    name, nbase, copies, ladder = case
    path = VARIANTS.get(name, (name,))[0]
    cls, dirs, N, _ = UG.PATHS[path]
    mdl = tc.model(dirs, nbase, copies, ladder)
    ref = tc.oracle_rows(mdl, cls)
    got, counters = _gpu_rows(name, mdl)
    what = _case_id(case)
    print("%s: %d voxels; %s" % (what, ref.shape[0], ", ".join("%s %d" % kv for kv in counters.items())))
    if sum(uc.CLASSES[cls]) >= 4:
        n = _compare_4up(got, ref, mdl, cls, what)
        print("%s: %d of %d voxels accepted below the tie window by their re-scored objective" % (what, n, ref.shape[0]))
    else:
        UG._compare(got, ref, cls, what + " against the oracle")
    if path == "k3b":
        assert counters["redone"] == 0
    if path == "k3b-cap4" and ladder == "window":
        assert counters["redone"] >= 1


# ---- mf_utils.solve_exhaustive_posweights on the oracle's rotated dictionaries
_solver_refs = {}


def _solver_problems(mdl, cls):
    K = uc.CLASSES[cls][0]
    key = (mdl["key"], cls)
    if key not in _solver_refs:
        from oracle import oracle as orc
        peaks, Y = tc.voxels(mdl, cls)
        sizes = np.array([mdl["N"]] * K)
        out = []
        for v in range(Y.shape[0]):
            A = np.ascontiguousarray(np.concatenate(tc.rotated(mdl, peaks[v], K), axis=1))
            y = np.ascontiguousarray(Y[v])
            out.append((A, y, sizes, orc.solve_exhaustive_posweights(A, y, sizes)))
        _solver_refs[key] = out
    return _solver_refs[key]


@pytest.mark.parametrize("ladder", sorted(tc.LADDERS))
@pytest.mark.parametrize("nbase,copies", tc.shapes(64), ids=lambda x: str(x))
@pytest.mark.parametrize("cls", ["NN", "NNN"])
def test_explicit_solver_on_twins(cls, nbase, copies, ladder):
    """[64, 64] (solve_generic.hip's plain scan) and [64, 64, 64] (solve_k3.hip's FP32 screen) on the rotated dictionaries
    of the class's voxels: (w, sub, tot, min_obj) bit for bit with the oracle."""
    from microstructure_fingerprinting_amd import mf_utils as mfu
    mdl = tc.model(20, nbase, copies, ladder)
    for v, (A, y, sizes, ref) in enumerate(_solver_problems(mdl, cls)):
        TG.assert_bit_equal(mfu.solve_exhaustive_posweights(A, y, sizes), ref, "%s %dx%d %s voxel %d" % (cls, nbase, copies, ladder, v))


# ---- weighted fits
@pytest.mark.parametrize("ladder", sorted(tc.LADDERS))
@pytest.mark.parametrize("nbase,copies", tc.shapes(64), ids=lambda x: str(x))
@pytest.mark.parametrize("cls", ["NN", "NN_1"])
def test_fit_weighted_on_twins(cls, nbase, copies, ladder):
    """engine.fit_weighted with W ~ U(0.05, 2) per measurement against _wfit_ref.ref_row (the oracle's solver on
    sqrt(W)-scaled oracle rotations) with that referee's assert_rows."""
    from microstructure_fingerprinting_amd import engine
    K, c, _ = uc.CLASSES[cls]
    mdl = tc.model(20, nbase, copies, ladder)
    peaks, Y = tc.voxels(mdl, cls)
    V, M = Y.shape
    W = np.random.default_rng([77, K, c, nbase, copies]).uniform(0.05, 2.0, (V, M))
    T = uc.tables(mdl, 1.0)
    ref = np.stack([R.ref_row(T, mdl["sch"], Y[v], W[v], [peaks[v, 3 * k:3 * k + 3] for k in range(K)], bool(c), mdl["sig_csf"],
                              K, bool(c)) for v in range(V)])
    got, st = engine.fit_weighted(UG._plan(mdl, 1.0), Y, W, np.full(V, K), np.full(V, bool(c)) if c else None, peaks, K,
                                  bool(c), mdl["sig_csf"] if c else None)
    assert np.all(st == 0)
    R.assert_rows(got, ref, K, "fit_weighted %s %dx%d %s" % (cls, nbase, copies, ladder))
