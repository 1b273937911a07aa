"""Inputs shared by tests/test_units_gpu.py and its precondition without a GPU, tests/test_units_host.py: one small
model per protocol length, one set of voxels per voxel class, and the UNITS in which dictionary and signals are stored.

A unit pair (c, cy) multiplies the dictionary (CSF and EAR columns included) by c and the signals by cy.  The reference
normalises neither, and its Cramer tests compare determinants that scale as |y| |d|^5 against an ABSOLUTE tolerance
(mf_utils.py:480-481, 562): with q = log2(cy) + 5 log2(c) the tolerance is inert around q = 0 - there a row at (c, cy)
is the baseline row with M0 -> M0 cy / c and MSE -> MSE cy^2 - and takes over near q = -40 ("Units"), where the
reference returns negative weights.  Every pair of UNITS lies in the inert region; tests/test_units_host.py measures the
boundary and asserts the distance.  The CPU oracle is the referee; its rows are computed once per process."""
import os

import numpy as np

from oracle import oracle as orc

Z = np.array([0.0, 0.0, 1.0])
E = 4
NTHREADS = max(1, min(os.cpu_count() or 1, 16))

# (id, c, cy, power of two)
UNITS = [("d2^%d_y2^%d" % (ec, ey), 2.0 ** ec, 2.0 ** ey, True)
         for ec, ey in ((16, 0),      # column norms ~3e5: past the FP16 range
                        (16, -25),    # large dictionary, small signals
                        (-10, 34),    # column norms ~4e-3
                        (0, -9),      # data normalised to ~1
                        (0, 24))]     # large signals
UNITS += [("d1e4_y1", 1e4, 1.0, False), ("d1e-3_y1e10", 1e-3, 1e10, False), ("d1_y1over500", 1.0, 1.0 / 500.0, False)]
UNIT_IDS = [u[0] for u in UNITS]
TOLERANCE_REGIME = ("d2^-14_y2^0", 2.0 ** -14, 1.0, True)    # q = -70: no policy of the library's is tested there but sanity

# class -> (fascicles, CSF column, EAR columns): sub-dictionary sizes [N] * K + [1] + [E]
CLASSES = {"N": (1, 0, 0), "N_1": (1, 1, 0), "N_E": (1, 0, 1), "N_1_E": (1, 1, 1),
           "NN": (2, 0, 0), "NN_1": (2, 1, 0), "NN_E": (2, 0, 1), "NN_1_E": (2, 1, 1),
           "NNN": (3, 0, 0), "NNN_1": (3, 1, 0)}

_models, _voxels, _tables, _rows = {}, {}, {}, {}


def q_of(c, cy):
    return float(np.log2(cy) + 5.0 * np.log2(c))


def model(dirs, N=64):
    """2 b0 + three shells of `dirs` directions each (M = 2 + 3 dirs), N atoms with S0 in 0.5 .. 1."""
    from microstructure_fingerprinting_amd import synth
    key = (dirs, N)
    if key not in _models:
        rng = np.random.default_rng(9000 + 7 * dirs + N)
        sch = synth.make_scheme(rng, 2, [1000, 2000, 3000], [dirs, dirs, dirs])
        dic = synth.make_dictionary(rng, sch, N)
        b = (orc.GAMMA_H * sch[:, 3] * sch[:, 5]) ** 2 * (sch[:, 4] - sch[:, 5] / 3)
        sig_csf = np.exp(-sch[:, 6] / 2.0) * np.exp(-b * 3e-9)
        sig_ear = np.stack([np.exp(-sch[:, 6] / 0.08) * np.exp(-b * x) for x in np.linspace(0.2e-9, 1.2e-9, E)], axis=1)
        _models[key] = {"key": key, "sch": sch, "dic": dic, "N": N, "M": sch.shape[0], "sig_csf": sig_csf, "sig_ear": sig_ear}
    return _models[key]


def tables(mdl, c):
    """the oracle's knot tables of the dictionary stored in units of c"""
    key = (mdl["key"], c)
    if key not in _tables:
        _tables[key] = orc.init_tables(mdl["dic"] * c, mdl["sch"], Z)
    return _tables[key]


def nvox(cls):
    """voxels per class: 16, and 8 where the oracle goes through a Lawson-Hanson solve for every one of N^3 tuples"""
    return 8 if cls == "NNN_1" else 16


def voxels(mdl, cls, V=None):
    """Baseline voxels (signals near 500) of one class: generic mixtures at SNR 30, then a noise-free mixture (V - 4), a
    voxel with one fascicle absent (V - 3: its last fascicle for K >= 2 - the tuples that differ only in the absent
    fascicle's atom tie N-fold - and for K = 1 its last extra column), and two voxels with a pair of identical peaks (for
    K = 1: generic voxels).  With K >= 2 and a CSF or EAR column, voxel V - 5 has that last extra column absent."""
    from microstructure_fingerprinting_amd import synth
    V = V or nvox(cls)
    key = (mdl["key"], cls, V)
    if key in _voxels:
        return _voxels[key]
    K, c, e = CLASSES[cls]
    rng = np.random.default_rng(100 + sorted(CLASSES).index(cls))
    sch, N, M = mdl["sch"], mdl["N"], mdl["M"]
    T = tables(mdl, 1.0)
    p = [synth.unit_vectors(rng, V) for _ in range(K)]
    if K >= 2:
        p[1][V - 2] = p[0][V - 2]
        p[K - 1][V - 1] = p[0][V - 1]
    peaks = np.ascontiguousarray(np.concatenate(p, axis=1))
    Y = rng.normal(0, 500.0 / 30.0, (V, M))
    Y[V - 4] = 0.0
    for v in range(V):
        comps = [orc.interp(sch, p[k][v], T)[:, rng.integers(0, N)] for k in range(K)]
        if c:
            comps.append(mdl["sig_csf"])
        if e:
            comps.append(mdl["sig_ear"][:, rng.integers(0, E)])
        nu = rng.dirichlet(2.0 * np.ones(len(comps)))
        if v == V - 3 and len(comps) > 1:
            nu[K - 1 if K >= 2 else -1] = 0.0
            nu /= nu.sum()
        if v == V - 5 and K >= 2 and len(comps) > K:
            nu[-1] = 0.0
            nu /= nu.sum()
        Y[v] += 500.0 * np.stack(comps, axis=1) @ nu
    _voxels[key] = (peaks, Y)
    return _voxels[key]


def fit_args(mdl, cls, V, c):
    """(K per voxel, CSF flags, EAR flags, maxfasc, csf_on, ear_on, sig_csf, sig_ear, E) of a class at dictionary unit c"""
    K, cs, e = CLASSES[cls]
    return (np.full(V, K), np.full(V, bool(cs)), np.full(V, bool(e)), max(K, 1), bool(cs), bool(e),
            mdl["sig_csf"] * c if cs else None, mdl["sig_ear"] * c if e else None, E if e else 0)


def oracle_rows(mdl, cls, c, cy, V=None):
    """the oracle's parameter rows of the class's voxels at (c, cy) (cached, read-only)"""
    V = V or nvox(cls)
    key = (mdl["key"], cls, V, c, cy)
    if key not in _rows:
        peaks, Y = voxels(mdl, cls, V)
        Kv, cm, em, maxfasc, csf_on, ear_on, sc, se, ne = fit_args(mdl, cls, V, c)
        r = orc.fit_batch(tables(mdl, c), mdl["sch"], Y * cy, Kv, cm, em, peaks, maxfasc, csf_on, ear_on, sc, se, ne,
                          nthreads=NTHREADS)
        r.setflags(write=False)
        _rows[key] = r
    return _rows[key]


def to_baseline(rows, c, cy):
    """a row at (c, cy) in baseline units: M0 c / cy, MSE / cy^2 (exact for powers of two); layout mf.py:420-450:
    [M0, fractions, atom indices, (nu_csf), (nu_ear, EAR index), MSE, R2]"""
    r = np.array(rows, dtype=np.float64, copy=True)
    r[:, 0] = r[:, 0] * c / cy
    r[:, -2] = r[:, -2] / cy / cy
    return r


def weight_columns(cls):
    """columns of a row that hold M0 and the fractions"""
    K, c, e = CLASSES[cls]
    mf = max(K, 1)
    cols = [0] + list(range(1, 1 + K))
    if c:
        cols.append(2 * mf + 1)
    if e:
        cols.append(2 * mf + c + 1)
    return cols
