"""Dictionaries of near-twin atoms for the fits of 2-D (AxCaliber-like) protocols: the inputs of tests/test_twin2d_gpu.py
and of its precondition without a GPU, tests/test_twin2d_host.py.  The pattern of tests/_twin_cases.py and
tests/_w2d_ref.py: the rotation is an argument (the host test passes tests/_rot2d_ref.Referee, the GPU test the library's
own T.rotate, which the kernels must see bit for bit), everything is cached and read-only.

mfx_fit2d_k2_kernel (csrc/fit2d_kernels.h) ranks pairs on an MFMA-summed cross-Gram, protects the arg-min of a slot with a
4 M eps interval and the 1e-9 |y|^2 window, carries a lower bound across its 128 x 128 blocks, decides a short list of
512 slots in the reference's arithmetic and, when the list overflows, every pair.  Well-separated atoms pass all of it
with orders of magnitude to spare; here the optimum is contested.

A CASE is (scheme, base atoms, copies, ladder).  Its dictionary: `base atoms` smooth atoms of test_fit2d_gpu.atoms plus
copies - 1 further columns per atom, (1 - eps) base_i + eps base_other with eps = 10 ** U(LADDERS[ladder]) (the recipe of
_twin_cases.family_dictionary), the columns permuted so that a copy precedes its original about half the time.  For one
base atom the "other" is a second smooth atom that is not itself in the dictionary.  The 2-D rotation is linear in the
columns: twins stay twins in every rotated dictionary.

    32 x 2, 8 x 8, 1 x 64   N = 64: one Gram block
    72 x 2                  N = 144: 2 x 2 blocks, the second holds one full tile of 16 atoms; the bound crosses blocks
    24 x 2                  N = 48: three tiles, a half-filled wave
    1 x 48 (window only)    N = 48: still more listed slots (768) than the list holds
    12 x 2                  N = 24: three fascicles (8 voxels)
    fix 32 x 2 margin       1 776 rows: 222 chunks (6 voxels)

Voxels: test_fit2d_gpu.two_fascicle_voxels' mixtures (|cos| between the fascicles <= 0.85, |d_z| >= zmin, Rician noise at
SNR 30, fractions in [0.3, 0.7], planted atoms drawn over all columns), 24 per case on syn2; then two voxels whose signal
holds the first fascicle only (ONE: single atoms against pairs; with noise the second weight is either exactly 0 or far
from 0, so these do not reach the family expansions - expansion_voxels does) and two whose directions are identical (SAME: Det = 0 on the
diagonal meets twins off it; every twin pair is near-collinear there and is handed over unranked).

gap_and_order measures a case on the oracle alone, for two sub-dictionaries (+ CSF): see its docstring."""
import os

import numpy as np

import _rot2d_ref as RR
import _twin_cases as tc
import _w2d_ref as W2
import test_fit2d_gpu as F2          # atoms, csf_signal, rician, random_dirs, oracle_row: nothing of that module runs here
from oracle import oracle as orc

LADDERS, TIE_WINDOW = tc.LADDERS, tc.TIE_WINDOW
TWO, ONE, SAME = 0, 1, 2
ZMIN = {"syn2": 0.1, "fix": 0.3}
SHAPES = [(32, 2), (8, 8), (1, 64), (72, 2), (24, 2)]
CASES = [("syn2", nb, cp, ld) for nb, cp in SHAPES for ld in sorted(LADDERS)] + [("syn2", 1, 48, "window")]
FIX_CASE = ("fix", 32, 2, "margin")
K3_CASES = [("syn2", 12, 2, ld) for ld in sorted(LADDERS)]
FLOOD_CASES = [("syn2", 1, 64, "window"), ("syn2", 1, 48, "window")]
UNIT_CASES = [("syn2", 32, 2, "margin"), ("syn2", 8, 8, "window")]
# (id, c, cy, power of two): the dictionary (and the CSF column) times c, the signals times cy
UNITS = [("d2^16_y1", 2.0 ** 16, 1.0, True), ("d2^16_y2^-25", 2.0 ** 16, 2.0 ** -25, True),
         ("d2^-10_y2^43", 2.0 ** -10, 2.0 ** 43, True), ("d1_y2^24", 1.0, 2.0 ** 24, True),
         ("d1e4_y1", 1e4, 1.0, False), ("d1e-3_y1e13", 1e-3, 1e13, False)]
Q_SIGNALS = float(np.log2(1.0 / 500.0))     # DESIGN 2.1 counts q from signals near 500; these are near 1

# case -> seed of its voxels where seed 0 misses a condition of tests/test_twin2d_host.py (conditions on the fixtures:
# the seeds are chosen so that they hold)
VOXEL_SEEDS = {("syn2", 32, 2, "margin"): 20, ("syn2", 8, 8, "margin"): 14, ("syn2", 1, 64, "margin"): 21,
               ("syn2", 1, 64, "window"): 3, ("syn2", 1, 48, "window"): 14, ("syn2", 72, 2, "margin"): 13, ("syn2", 72, 2, "window"): 1,
               ("syn2", 24, 2, "margin"): 4, ("fix", 32, 2, "margin"): 36}
EXPANSION_CASES = [("syn2", 32, 2, "margin"), ("syn2", 32, 2, "window"), ("syn2", 8, 8, "window"), ("syn2", 72, 2, "window")]
EXPANSION_SEEDS = {("syn2", 32, 2, "margin"): 3, ("syn2", 32, 2, "window"): 2, ("syn2", 72, 2, "window"): 1}
# case -> seed of its dictionary's eps and permutation, likewise
DICT_SEEDS = {("syn2", 72, 2, "margin"): 1, ("syn2", 24, 2, "margin"): 1}

_sch, _dics, _vox, _rows, _gaps, _pairs = {}, {}, {}, {}, {}, {}


def case_id(case):
    return "%s-%dx%d-%s" % case


def scheme(name):
    if name not in _sch:
        _sch[name] = np.load(os.path.join(F2.G, "rot2d_cases.npz"))[name + "_sch"]
    return _sch[name]


def dictionary(case):
    """(dictionary [M x nbase copies], family id per column) of a case: the recipe of the module docstring"""
    if case not in _dics:
        name, nbase, copies, ladder = case
        sch = scheme(name)
        lo, hi = LADDERS[ladder]
        rng = np.random.default_rng([9200, sorted(ZMIN).index(name), nbase, copies, sorted(LADDERS).index(ladder),
                                     DICT_SEEDS.get(case, 0)])
        pool = F2.atoms(sch, nbase + 1, 5)
        base = pool[:, :nbase]
        cols, fam = [base], [np.arange(nbase)]
        for _ in range(copies - 1):
            eps = 10.0 ** rng.uniform(lo, hi, nbase)
            if nbase > 1:
                partner = base[:, (np.arange(nbase) + rng.integers(1, nbase, nbase)) % nbase]
            else:
                partner = pool[:, nbase:]
            cols.append((1.0 - eps) * base + eps * partner)
            fam.append(np.arange(nbase))
        perm = rng.permutation(nbase * copies)
        dic, fam = np.ascontiguousarray(np.concatenate(cols, axis=1)[:, perm]), np.concatenate(fam)[perm]
        dic.setflags(write=False)
        fam.setflags(write=False)
        _dics[case] = (dic, fam)
    return _dics[case]


class RefRotation:
    """tests/_rot2d_ref.Referee with the two methods of RotateAtom2DTables that the fixtures use"""

    def __init__(self, dic, sch):
        self.R = RR.Referee(dic, sch, F2.Z, F2.DIFF)
        self.M, self.N = self.R.M, self.R.N

    def rotate(self, dirs):
        out = []
        for d in np.asarray(dirs, dtype=np.float64).reshape(-1, 3):
            r = self.R.rotate(d)
            assert r.ok, "the referee's rotation fails for %s: %s" % (d, r.error)
            out.append(r.out)
        return np.array(out).reshape(-1, self.M, self.N)


class Rotation:
    """A rotation (RefRotation or RotateAtom2DTables) with every rotated dictionary kept: rotate(dirs [B, 3]) -> [B, M, N]
    read-only, rotate_cols(dirs, ids) its columns.  `tag` names it in the caches below."""

    def __init__(self, rot, tag):
        self.rot, self.tag, self.M, self.N = rot, tag, rot.M, rot.N
        self._D = {}

    def rotate(self, dirs):
        d = np.ascontiguousarray(np.asarray(dirs, dtype=np.float64).reshape(-1, 3))
        new = [k for k in range(d.shape[0]) if d[k].tobytes() not in self._D]
        if new:
            out = self.rot.rotate(d[new])
            for q, k in enumerate(new):
                a = np.ascontiguousarray(out[q])
                a.setflags(write=False)
                self._D[d[k].tobytes()] = a
        return [self._D[d[k].tobytes()] for k in range(d.shape[0])]

    def rotate_cols(self, dirs, ids):
        return np.array([D[:, int(i)] for D, i in zip(self.rotate(dirs), np.asarray(ids).reshape(-1))])


def ref_rotation(case, c=1.0):
    """the host tests' rotation of a case's dictionary in units of c"""
    key = ("ref", case, c)
    if key not in _dics:
        _dics[key] = Rotation(RefRotation(dictionary(case)[0] * c, scheme(case[0])), "ref%g" % c)
    return _dics[key]


def nvox(case):
    return (6, 0) if case[0] == "fix" else ((8, 0) if case[1] * case[2] == 24 else (24, 2))


def voxels(case, rot, nfasc=2, nv=None):
    """(Y [V, M], peaks [V, 3 nfasc], kind [V]) of a case on a Rotation of its dictionary in units of 1 (cached per
    rotation).  Fascicles beyond the second (nfasc = 3) cross the first two by the same rule.  nv: that many two-fascicle
    mixtures instead of the case's own number (the first ones are the same voxels)."""
    key = (case, rot.tag, nfasc, nv)
    if key not in _vox:
        name, nbase, copies, ladder = case
        N = nbase * copies
        V2, extra = nvox(case) if nv is None else (nv, 0)
        V = V2 + 2 * extra
        rng = np.random.default_rng([300, sorted(ZMIN).index(name), nbase, copies, sorted(LADDERS).index(ladder), nfasc,
                                     VOXEL_SEEDS.get(case, 0)])
        kind = np.array([TWO] * V2 + [ONE] * extra + [SAME] * extra)
        Y, peaks = np.zeros((V, rot.M)), np.zeros((V, 3 * nfasc))
        for v in range(V):
            while True:
                d = F2.random_dirs(rng, nfasc, ZMIN[name])
                if all(abs(d[a] @ d[b]) <= 0.85 for a in range(nfasc) for b in range(a)):
                    break
            ids = rng.integers(0, N, nfasc)
            f = rng.uniform(0.3, 0.7)
            if kind[v] == SAME:
                d[1] = d[0]
            cols = rot.rotate_cols(d, ids)
            if nfasc == 3:
                g = rng.uniform(0.2, 0.4)
                clean = (1.0 - g) * (f * cols[0] + (1.0 - f) * cols[1]) + g * cols[2]
            else:
                clean = cols[0] if kind[v] == ONE else f * cols[0] + (1.0 - f) * cols[1]
            Y[v] = F2.rician(rng, clean)
            peaks[v] = d.reshape(-1)
        for a in (Y, peaks, kind):
            a.setflags(write=False)
        _vox[key] = (Y, peaks, kind)
    return _vox[key]


def expansion_voxels(case, rot):
    """(Y [8, M], peaks [8, 6]) without noise, for the family expansions of mfx_fit2d_k2_kernel: even voxels hold atom i of
    the first fascicle plus t times atom j of the second, odd voxels t times atom i plus atom j, t = 10 ** U(-12, -9).
    The best pair's second (first) weight is then positive and below 1e-7 of the other one - the range in which the
    kernel expands the winner's row (column); every pair of that row (column) fits equally well up to rounding and the
    reference returns the first that attains its own rounded minimum.  tests/test_twin2d_host.py guards the range."""
    key = (case, rot.tag, "expansion")
    if key not in _vox:
        name, nbase, copies, ladder = case
        rng = np.random.default_rng([301, sorted(ZMIN).index(name), nbase, copies, sorted(LADDERS).index(ladder),
                                     EXPANSION_SEEDS.get(case, 0)])
        Y, peaks = np.zeros((8, rot.M)), np.zeros((8, 6))
        for v in range(8):
            while True:
                d = F2.random_dirs(rng, 2, ZMIN[name])
                if abs(d[0] @ d[1]) <= 0.85:
                    break
            ids = rng.integers(0, nbase * copies, 2)
            t = 10.0 ** rng.uniform(-12.0, -9.0)
            cols = rot.rotate_cols(d, ids)
            Y[v] = cols[0] + t * cols[1] if v % 2 == 0 else t * cols[0] + cols[1]
            peaks[v] = d.reshape(-1)
        Y.setflags(write=False)
        peaks.setflags(write=False)
        _vox[key] = (Y, peaks)
    return _vox[key]


def csf_voxels(case, rot):
    """the case's voxels with a fifth of the CSF signal mixed in: (Y, peaks, kind)"""
    Y, peaks, kind = voxels(case, rot)
    return 0.8 * Y + 0.2 * F2.csf_signal(scheme(case[0])), peaks, kind


def weights(case, kind, V, M):
    """'smooth': W ~ U(0.05, 2); 'mask': 1 with max(6, M // 8) rows per voxel zeroed; 'ones': 1"""
    if kind == "ones":
        return np.ones((V, M))
    rng = np.random.default_rng([77, case[1], case[2], sorted(LADDERS).index(case[3]), kind == "mask"])
    if kind == "smooth":
        return rng.uniform(0.05, 2.0, (V, M))
    W = np.ones((V, M))
    for v in range(V):
        W[v, rng.choice(M, W2.nbad(M), replace=False)] = 0.0
    return W


def oracle_rows(case, rot, K, csf=False, W=None, wkind=None, c=1.0, cy=1.0, base=None, nmax=None):
    """The referee's rows of a case's voxels as K-fascicle voxels (K + csf <= 3): the oracle's
    solve_exhaustive_posweights on the columns `rot` returns - test_fit2d_gpu.oracle_row, or _w2d_ref.ref_row on sqrt(W)-
    scaled columns when W is given (wkind names W in the cache).  `rot` rotates the dictionary in units of c; the voxels
    are those of `base` (the rotation in units of 1, default `rot`) times cy, the CSF column times c; the first nmax only."""
    key = (case, rot.tag, K, csf, wkind, c, cy, nmax)
    if key not in _rows:
        base = base or rot
        Y, peaks, _ = csf_voxels(case, base) if csf else voxels(case, base, max(K, 2))
        sig_csf = F2.csf_signal(scheme(case[0])) * c if csf else None
        rows = []
        for v in range(Y.shape[0] if nmax is None else nmax):
            dirs = peaks[v, :3 * K].reshape(K, 3)
            y = np.ascontiguousarray(Y[v] * cy)
            if W is None:
                rows.append(F2.oracle_row(rot, y, dirs, csf, sig_csf, K, csf))
            else:
                rows.append(W2.ref_row(rot.rotate(dirs), y, W[v], csf, sig_csf, K, csf))
        r = np.array(rows)
        r.setflags(write=False)
        _rows[key] = r
    return _rows[key]


def to_baseline(rows, c, cy):
    """a row at (c, cy) in baseline units: M0 c / cy, MSE / cy^2 (exact for powers of two)"""
    r = np.array(rows, dtype=np.float64)
    r[:, 0] = r[:, 0] * c / cy
    r[:, -2] = r[:, -2] / cy / cy
    return r


def pair_objectives(D0, D1, y):
    """float64 closed form of every pair (i of D0, j of D1): (obj [N, N] = min_{w >= 0} |y - w0 d_i - w1 d_j|^2, both [N, N]
    two positive weights, cc [N, N] = 1 - c^2).  A pair with 1 - c^2 <= 1e-8 (twins under identical directions) is scored as
    its better single atom: the closed form has no digits left there."""
    a11, a22 = np.sum(D0 * D0, axis=0)[:, None], np.sum(D1 * D1, axis=0)[None, :]
    y1, y2 = (D0.T @ y)[:, None], (D1.T @ y)[None, :]
    a12 = D0.T @ D1
    d1, d2, det = a22 * y1 - a12 * y2, a11 * y2 - a12 * y1, a11 * a22 - a12 * a12
    cc = det / (a11 * a22)
    both = (d1 > 0) & (d2 > 0) & (cc > 1e-8)
    with np.errstate(divide="ignore", invalid="ignore"):
        sc2 = np.where(both, (y1 * d1 + y2 * d2) / det, 0.0)
    s1 = np.maximum(np.where(y1 > 0, y1 * y1 / a11, 0.0), np.where(y2 > 0, y2 * y2 / a22, 0.0))
    return float(y @ y) - np.where(both, sc2, s1), both, cc


def pairs(case, rot, v):
    """pair_objectives of voxel v of a case (cached)"""
    key = (case, rot.tag, v)
    if key not in _pairs:
        Y, peaks, _ = voxels(case, rot)
        D = rot.rotate(peaks[v].reshape(2, 3))
        _pairs[key] = pair_objectives(D[0], D[1], Y[v])
    return _pairs[key]


def gap_and_order(case, rot, csf=False):
    """Per voxel of a case as a two-fascicle voxel (+ CSF), on the oracle alone (cached):
    gap     (objective of the best OTHER pair built from copies of the oracle's chosen atoms) - (the oracle's min_obj =
            MSE * M), over |y|^2: pair_objectives without CSF, orc.nnls with the CSF column kept;
    first   that runner-up precedes the oracle's pair in the reference's scan order i1 -> i2;
    within  the number of such other pairs within TIE_WINDOW |y|^2 of min_obj;
    mincc   the smallest 1 - c^2 between columns of different sub-dictionaries (the CSF column included)."""
    key = (case, rot.tag, csf)
    if key in _gaps:
        return _gaps[key]
    Y, peaks, kind = csf_voxels(case, rot) if csf else voxels(case, rot)
    rows = oracle_rows(case, rot, 2, csf)
    fam = dictionary(case)[1]
    V, M = Y.shape
    sc = F2.csf_signal(scheme(case[0]))
    out = {k: np.zeros(V) for k in ("gap", "within", "mincc")}
    out["first"] = np.zeros(V, bool)
    for v in range(V):
        y = np.ascontiguousarray(Y[v])
        ysq = float(y @ y)
        D = rot.rotate(peaks[v].reshape(2, 3))
        i, j = int(rows[v, 3]), int(rows[v, 4])
        fi, fj = np.flatnonzero(fam == fam[i]), np.flatnonzero(fam == fam[j])
        min_obj = rows[v, -2] * M
        obj_all, _, cc = pair_objectives(D[0], D[1], y)
        if csf:
            obj = np.array([[orc.nnls(np.stack([D[0][:, a], D[1][:, b], sc], axis=1), y)[1] ** 2 for b in fj] for a in fi])
            for Dk in D:
                c2 = (sc @ Dk) ** 2 / np.sum(Dk * Dk, axis=0) / (sc @ sc)
                cc = np.minimum(cc, 1.0 - float(c2.max()))
        else:
            obj = obj_all[np.ix_(fi, fj)].copy()
        obj[fi == i, fj == j] = np.inf
        a, b = np.unravel_index(np.argmin(obj), obj.shape)
        out["gap"][v] = (obj[a, b] - min_obj) / ysq
        out["first"][v] = (int(fi[a]), int(fj[b])) < (i, j)
        out["within"][v] = np.count_nonzero(obj - min_obj < TIE_WINDOW * ysq)
        out["mincc"][v] = float(np.min(cc))
    for a in out.values():
        a.setflags(write=False)
    _gaps[key] = out
    return out
