"""Problems shared by tests/test_solver_ties_gpu.py and its guard without a GPU, tests/test_solver_ties_host.py:
inputs of the explicit-dictionary solver (csrc/solve_generic.hip) whose best index tuples tie - exactly (duplicated
columns) or up to rounding (two bit-identical sub-dictionaries: the tuples (i, j) and (j, i) hold the same columns).
Every problem is well conditioned; the CPU oracle is the referee and its answers are computed once per process."""
import numpy as np

from oracle import oracle as orc

SEEDS = range(60)
ONE_BLOCK = [((14, 14), 12), ((16, 16), 12), ((14, 14, 1), 12), ((16, 16, 1), 12)]      # at most 256 tuples
SEVERAL_BLOCKS = [((40, 40), 20), ((30, 30, 1), 20)]                                  # pairs straddle and share blocks
_cache = {}


def shape_id(v):
    return "x".join(str(n) for n in v) if isinstance(v, tuple) else "M%d" % v


def symmetric_problem(sizes, M, seed):
    """(A, y, dicsizes): two identical sub-dictionaries D (and a CSF-like column when len(sizes) == 3), the signal of
    two different atoms i, j of D plus noise."""
    rng = np.random.default_rng(seed)
    N = sizes[0]
    D = np.abs(rng.standard_normal((M, N))) + 0.2
    i, j = rng.choice(N, 2, replace=False)
    csf = np.exp(-np.linspace(0, 3, M))
    cols = [D, D] + ([csf[:, None]] if len(sizes) == 3 else [])
    y = 0.6 * D[:, i] + 0.3 * D[:, j] + (0.1 * csf if len(sizes) == 3 else 0.0) + 0.02 * rng.standard_normal(M)
    return np.ascontiguousarray(np.hstack(cols)), y, np.array(sizes)


def symmetric_reference(sizes, M):
    """[(A, y, dicsizes, oracle result)] over SEEDS."""
    key = ("sym", tuple(sizes), M)
    if key not in _cache:
        out = []
        for seed in SEEDS:
            A, y, ds = symmetric_problem(sizes, M, seed)
            out.append((A, y, ds, orc.solve_exhaustive_posweights(A, y, ds)))
        _cache[key] = out
    return _cache[key]


FOUR = [((12, 12, 1, 2), 16)]     # _4up: K' = 4 goes through the active-set optimum of the finalize stage


def symmetric_problem_four(sizes, M, seed):
    """(A, y, dicsizes) with K' = 4: two identical sub-dictionaries D, a CSF-like column and sizes[3] EAR-like columns; the
    signal of two different atoms of D, the CSF column and the first EAR column plus noise (every compartment active).
    The reference's Lawson-Hanson solve ties the mirrored tuples (i, j, ..) and (j, i, ..) exactly: its first hit,
    the one with the smaller tuple number, is the answer."""
    rng = np.random.default_rng(seed)
    N = sizes[0]
    D = np.abs(rng.standard_normal((M, N))) + 0.2
    i, j = rng.choice(N, 2, replace=False)
    csf = np.exp(-np.linspace(0, 3, M))
    ear = np.stack([np.exp(-np.linspace(0, 1.0 + k, M)) for k in range(sizes[3])], axis=1)
    y = 0.5 * D[:, i] + 0.25 * D[:, j] + 0.1 * csf + 0.15 * ear[:, 0] + 0.02 * rng.standard_normal(M)
    return np.ascontiguousarray(np.hstack([D, D, csf[:, None], ear])), y, np.array(sizes)


def symmetric_reference_four(sizes, M):
    """[(A, y, dicsizes, oracle result)] over SEEDS."""
    key = ("sym4", tuple(sizes), M)
    if key not in _cache:
        out = []
        for seed in SEEDS:
            A, y, ds = symmetric_problem_four(sizes, M, seed)
            out.append((A, y, ds, orc.solve_exhaustive_posweights(A, y, ds)))
        _cache[key] = out
    return _cache[key]


def swapped(cases):
    """Number of problems in which the oracle returns sub[0] > sub[1]: the pair in the other order than the first of
    the two in tuple-number order."""
    return sum(1 for (_, _, _, ref) in cases if ref[1][0] > ref[1][1])


def identical_peak_voxels(sch, T, V, seed, sig_csf=None, scale=500.0):
    """peaks [V, 6] with both fascicles along one direction and Y [V, M]: 0.6 / 0.3 of two different atoms of the
    oracle's rotation (and 0.1 of sig_csf), times scale, plus noise at SNR 50."""
    from microstructure_fingerprinting_amd import synth
    rng = np.random.default_rng(seed)
    d = synth.unit_vectors(rng, V)
    peaks = np.ascontiguousarray(np.hstack([d, d]))
    Y = np.zeros((V, sch.shape[0]))
    for v in range(V):
        D = orc.interp(sch, d[v], T)
        i, j = rng.choice(T["N"], 2, replace=False)
        y = 0.6 * D[:, i] + 0.3 * D[:, j] + (0.1 * sig_csf if sig_csf is not None else 0.0)
        Y[v] = scale * (y + 0.02 * rng.standard_normal(sch.shape[0]))
    return peaks, Y


def c2_model(N=16):
    """(sch, dictionary, oracle tables, sig_csf) of the synthetic C2 protocol (M = 200) with N atoms."""
    key = ("c2", N)
    if key not in _cache:
        from microstructure_fingerprinting_amd import synth
        sch, dic, _ = synth.make_model("C2", N)
        T = orc.init_tables(dic, sch, np.array([0.0, 0.0, 1.0]))
        b = (orc.GAMMA_H * sch[:, 3] * sch[:, 5]) ** 2 * (sch[:, 4] - sch[:, 5] / 3)
        _cache[key] = (sch, dic, T, np.exp(-sch[:, 6] / 2.0) * np.exp(-b * 3.0e-9))
    return _cache[key]


def k3_order_problem(kind, seed):
    """[4, 3, 4] with exact ties between triples (i1 small, i3 large) and (i1 large, i3 small).
    'within': column 3 of the first and of the third sub-dictionary duplicate their column 0: the four triples
    (0|3, 1, 0|3) tie exactly.  'cross': the third sub-dictionary holds columns 0 and 3 of the first at 0 and 3, the
    signal is made of those two: (0, 1, 3) and (3, 1, 0) hold the same three columns - the first in tuple-number order
    is (0, 1, 3), the first in the reference's i3 -> i1 -> i2 order is (3, 1, 0)."""
    rng = np.random.default_rng(seed)
    M = 10
    A1, A2, A3 = (np.abs(rng.standard_normal((M, n))) + 0.2 for n in (4, 3, 4))
    if kind == "within":
        A1[:, 3] = A1[:, 0]
        A3[:, 3] = A3[:, 0]
        y = 0.5 * A1[:, 0] + 0.3 * A2[:, 1] + 0.2 * A3[:, 0]
    else:
        A3[:, 0] = A1[:, 0]
        A3[:, 3] = A1[:, 3]
        y = 0.5 * A1[:, 0] + 0.3 * A2[:, 1] + 0.4 * A1[:, 3]
    y = y + 0.01 * rng.standard_normal(M)
    return np.ascontiguousarray(np.hstack([A1, A2, A3])), y, np.array([4, 3, 4])


def two_block_tie_problem():
    """[3, 300]: t = 300 i1 + i2.  Column 290 of the second sub-dictionary duplicates its column 5 and column 2 of the
    first its column 0; the signal is made of (0, 5): the tied tuples 5, 290, 605 and 890 lie in the scan blocks 0, 1,
    2 and 3."""
    rng = np.random.default_rng(5)
    M = 12
    A = np.abs(rng.standard_normal((M, 303))) + 0.2
    A[:, 3 + 290] = A[:, 3 + 5]
    A[:, 2] = A[:, 0]
    y = 0.7 * A[:, 0] + 0.4 * A[:, 3 + 5] + 0.01 * rng.standard_normal(M)
    return A, y, np.array([3, 300])


def all_tied_problem():
    """[1500, 1500], M = 8, every column the same positive vector: 2 250 000 exact ties."""
    rng = np.random.default_rng(6)
    c = np.abs(rng.standard_normal(8)) + 0.2
    A = np.ascontiguousarray(np.tile(c[:, None], (1, 3000)))
    return A, 2.0 * c + 0.01 * rng.standard_normal(8), np.array([1500, 1500])


def all_tied_triples_problem():
    """[128, 128, 128], M = 8: one positive vector per sub-dictionary in all of its columns, except column 0 of the
    first, which fits worse.  The 127 * 128 * 128 = 2 080 768 triples with i1 >= 1 tie exactly - more than the list
    of the three-dictionary screen (2^20) holds, so the plain scan takes over, and more than its list holds.  First
    hit in the reference's order: (1, 0, 0)."""
    rng = np.random.default_rng(8)
    c = np.abs(rng.standard_normal((8, 4))) + 0.2
    A = np.ascontiguousarray(np.repeat(c[:, :3], 128, axis=1))
    A[:, 0] = c[:, 3]
    return A, c[:, :3] @ np.array([0.5, 0.3, 0.2]) + 0.01 * rng.standard_normal(8), np.array([128, 128, 128])


PLANTED = (1450, 1480)       # tuple 1450 * 1500 + 1480 = 2 176 480 > 8192 * 256: the scan's second trip


def grid_stride_problem():
    rng = np.random.default_rng(7)
    A = np.abs(rng.standard_normal((8, 3000))) + 0.2
    y = 0.6 * A[:, PLANTED[0]] + 0.4 * A[:, 1500 + PLANTED[1]] + 1e-4 * rng.standard_normal(8)
    return A, y, np.array([1500, 1500])


MANY = {6: (3, 2, 2, 2, 2, 1), 7: (2, 2, 2, 2, 2, 2, 1), 8: (2, 2, 2, 2, 2, 2, 2, 1)}


def many_dictionaries_problem(Kp):
    """K' = 6, 7, 8: M = 24, positive columns, the signal of the last atom of every sub-dictionary plus 1 % noise.
    (The seeds leave a top-2 gap of 2.3e-3, 3.4e-3 and 1.6e-3 |y|^2: test_solver_ties_host.py.)"""
    sizes = np.array(MANY[Kp])
    rng = np.random.default_rng(1000 * Kp)
    M = 24
    A = np.abs(rng.standard_normal((M, int(sizes.sum())))) + 0.2
    last = np.cumsum(sizes) - 1
    w = rng.uniform(0.5, 1.5, Kp)
    y = A[:, last] @ w
    y = y + 0.01 * np.sqrt(np.mean(y * y)) * rng.standard_normal(M)
    return A, y, sizes


def top2_gap(A, y, sizes):
    """(best - runner-up gap of the objective over ALL tuples, relative to |y|^2; tuple of the best), by the oracle's
    NNLS on every tuple."""
    start = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    objs, tuples = [], []
    for t in np.ndindex(*[int(s) for s in sizes]):
        _, rn = orc.nnls(A[:, start + np.array(t)], y)
        objs.append(rn * rn)
        tuples.append(t)
    o = np.argsort(objs)
    return (objs[o[1]] - objs[o[0]]) / float(np.sum(y * y)), tuples[o[0]]
