"""Problems shared by tests/test_solve_batch_referee_gpu.py and its guard without a GPU,
tests/test_solve_batch_referee_host.py: batches for the batched explicit-dictionary solver (csrc/solve_batch.hip) that
take its signal sweep through more than one trip, mix overflowed, ordinary, all-zero and non-finite signals in one
batch, sit on the edges of the candidate list, tie across the seams of the 64 x 64 tiles, are built of near-twin atoms
and span hundreds of orders of magnitude.  Everything here is numpy and the CPU oracle; nothing needs a device.

pairs_in_window is the closed-form two-column NNLS objective of every pair (the reference's arithmetic, vectorised).  It
only states conditions on the fixtures - how many pairs tie, how many lie inside the library's window 1e-9 |y|^2 - and
is never the referee: that is the loop of one-problem solves, and the oracle where a test says so."""
import functools

import numpy as np

import _ties_cases as TC
import _twin_cases as TW
import _units_cases as UC

TIE_WINDOW = 1e-9      # the library's tie window, relative to |y|^2
SCAN_CAP = 16384       # MFX_SCAN_CAP: entries of a signal's candidate list


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


# ---- the referee of the fixtures' conditions
def pair_objectives(A1, A2, y):
    """(objective [n1 x n2] of every pair, |y|^2): sums over the rows in row order, then the four branches of the
    reference's two-column closed form, operation for operation."""
    M = y.size
    A11, A22, Y1, Y2 = np.zeros(A1.shape[1]), np.zeros(A2.shape[1]), np.zeros(A1.shape[1]), np.zeros(A2.shape[1])
    A12 = np.zeros((A1.shape[1], A2.shape[1]))
    ysq = 0.0
    for k in range(M):
        A11 = A11 + A1[k] * A1[k]
        A22 = A22 + A2[k] * A2[k]
        A12 = A12 + A1[k][:, None] * A2[k][None, :]
        Y1 = Y1 + y[k] * A1[k]
        Y2 = Y2 + y[k] * A2[k]
        ysq = ysq + y[k] * y[k]
    a11, a22, y1, y2 = A11[:, None], A22[None, :], Y1[:, None], Y2[None, :]
    a11, a22, y1, y2 = (np.broadcast_to(x, A12.shape) for x in (a11, a22, y1, y2))
    w1d = a22 * y1 - A12 * y2
    w2d = a11 * y2 - A12 * y1
    with np.errstate(divide="ignore", invalid="ignore"):
        det = a11 * a22 - A12 * A12
        w0, w1 = w1d / det, w2d / det
        both = ysq + w0 * w0 * a11 + w1 * w1 * a22 + 2 * (w0 * w1 * A12 - w0 * y1 - w1 * y2)
        first = ysq - y1 * (y1 / a11)
        second = ysq - y2 * (y2 / a22)
    none = np.full(A12.shape, ysq)
    res = np.select(
        [(w1d > 0) & (w2d > 0), (w1d >= 0) & (w2d <= 0), (w1d <= 0) & (w2d >= 0), (w1d < 0) & (w2d < 0)],
        [both, np.where(y1 >= 0, first, none), np.where(y2 >= 0, second, none),
         np.where(y1 > 0, first, np.where(y2 > 0, second, none))], default=ysq)
    return res, ysq


def pairs_in_window(A1, A2, y):
    """(pairs whose objective lies within 1e-9 |y|^2 of the best, pairs whose objective equals the best exactly)"""
    res, ysq = pair_objectives(A1, A2, y)
    best = res.min()
    return int(np.count_nonzero(res <= best + TIE_WINDOW * ysq)), int(np.count_nonzero(res == best))


# ---- A1. sweeps of three trips: [150, 149] and [150, 149, 1], M = 17, V = 500
SWEEP_V, SWEEP_M = 500, 17
SWEEP_SHAPES = [(150, 149), (150, 149, 1)]
SWEEP_ZERO, SWEEP_BAD = 229, (3, 230, 499)


@functools.lru_cache(maxsize=None)
def sweep_problem(sizes):
    """(A, Y [500 x 17], dicsizes): an |randn| dictionary; every signal 0.7 of an atom of the first sub-dictionary, 0.2 of
    one of every other, noise of 0.01 (the recipe of test_solve_batch_gpu.make_problem), the atoms drawn per signal.
    Row 229 is all zero; rows 3, 230 and 499 hold a NaN, an inf and a -inf."""
    sz = np.array(sizes)
    rng = np.random.default_rng([78, SWEEP_M] + [int(s) for s in sz])
    starts = np.concatenate(([0], np.cumsum(sz)[:-1]))
    A = np.abs(rng.standard_normal((SWEEP_M, int(sz.sum()))))
    Y = np.zeros((SWEEP_V, SWEEP_M))
    for v in range(SWEEP_V):
        for k, (s0, n) in enumerate(zip(starts, sz)):
            Y[v] += (0.7 if k == 0 else 0.2) * A[:, s0 + rng.integers(n)]
        Y[v] += 0.01 * rng.standard_normal(SWEEP_M)
    Y[SWEEP_ZERO] = 0.0
    Y[3, 5], Y[230, 0], Y[499, 16] = np.nan, np.inf, -np.inf
    return _frozen(A, Y) + (sz,)


# ---- A2. [1500, 1500], M = 8, V = 9: 576 tiles, trips of 4 / 4 / 1
PLANTED9 = [(0, 0), (63, 64), (64, 63), (100, 700), TC.PLANTED, (700, 100), (1407, 1472), (1472, 5), (1499, 1499)]


@functools.lru_cache(maxsize=None)
def planted_problem():
    """grid_stride_problem()'s dictionary and nine signals 0.6 a_i + 0.4 b_j + 1e-4 noise, (i, j) over PLANTED9: nine
    different tiles, the first, the ragged last one (rows and columns 1472 .. 1499) and both sides of the first seam."""
    A, _, sz = TC.grid_stride_problem()
    rng = np.random.default_rng(79)
    Y = np.stack([0.6 * A[:, i] + 0.4 * A[:, 1500 + j] + 1e-4 * rng.standard_normal(8) for i, j in PLANTED9])
    return _frozen(A, Y) + (sz,)


@functools.lru_cache(maxsize=None)
def all_tied_batch():
    """all_tied_problem()'s dictionary and nine signals a c + noise, a = 0.3 .. 3: 2 250 000 exact ties in each."""
    A, _, sz = TC.all_tied_problem()
    rng = np.random.default_rng(80)
    Y = np.stack([a * A[:, 0] + 0.01 * rng.standard_normal(8) for a in np.linspace(0.3, 3.0, 9)])
    return _frozen(A, Y) + (sz,)


# ---- A3. the clamp of a chunk to 65 535 signals
CLAMP_V, CLAMP_DISTINCT = 65541, 37


@functools.lru_cache(maxsize=None)
def clamp_problem(sizes):
    """(A, base [37 x 3], dicsizes), M = 3; the batch is base[np.arange(65541) % 37]"""
    sz = np.array(sizes)
    rng = np.random.default_rng([81] + [int(s) for s in sz])
    A = np.abs(rng.standard_normal((3, int(sz.sum())))) + 0.2
    base = np.abs(rng.standard_normal((CLAMP_DISTINCT, 3)))
    base[0] = 0.0
    return _frozen(A, base) + (sz,)


# ---- B. overflowed and ordinary signals in one batch
MIXED_KINDS = ["overflow", "unique", "nan", "overflow", "zero", "ties130", "unique", "overflow", "inf", "unique", "overflow",
               "unique"]
MIXED_DISTINCT = np.arange(6, 140, 14)      # the 10 columns per sub-dictionary that differ from c
MIXED_PLANTED = {1: (48, 104), 6: (6, 132), 9: (90, 20), 11: (132, 62)}     # row -> pair of distinct columns


@functools.lru_cache(maxsize=None)
def mixed_problem():
    """(A, Y [12 x 12], dicsizes [140, 140], c, r).  Both sub-dictionaries hold c in every column except the columns
    MIXED_DISTINCT.  An "overflow" row is a c + 0.05 |c| r / |r| with r pointing away from every distinct column, so each
    of them takes weight 0 and the 130 x 130 + 2 x 130 x 10 = 19 500 pairs with a column c tie exactly; a "unique" row
    is made of two distinct columns; "ties130" is c + 0.4 d with d a distinct column of the second sub-dictionary, which
    the 130 columns c of the first tie on."""
    rng = np.random.default_rng(141)
    M = 12
    c = np.abs(rng.standard_normal(M)) + 0.2
    A = np.tile(c[:, None], (1, 280))
    A[:, MIXED_DISTINCT] = np.abs(rng.standard_normal((M, 10))) + 0.2
    A[:, 140 + MIXED_DISTINCT] = np.abs(rng.standard_normal((M, 10))) + 0.2
    D = A[:, np.concatenate((MIXED_DISTINCT, 140 + MIXED_DISTINCT))]
    r = -np.mean(D - c[:, None] * ((c @ D) / (c @ c))[None, :], axis=1)
    tilt = 0.05 * np.sqrt(c @ c) * r / np.sqrt(r @ r)
    amp = iter((1.2, 0.4, 0.8, 2.0))
    Y = np.zeros((len(MIXED_KINDS), M))
    for v, kind in enumerate(MIXED_KINDS):
        if kind == "overflow":
            Y[v] = next(amp) * c + tilt
        elif kind == "unique":
            i, j = MIXED_PLANTED[v]
            Y[v] = 0.7 * A[:, i] + 0.4 * A[:, 140 + j] + 0.01 * rng.standard_normal(M)
        elif kind == "ties130":
            Y[v] = c + 0.4 * A[:, 140 + 34]
        elif kind in ("nan", "inf"):
            Y[v] = 0.9 * c + tilt
            Y[v, 7] = np.nan if kind == "nan" else np.inf
    return _frozen(A, Y, c, r)[:2] + (np.array([140, 140]), c, r)


CAP_EDGES = [((128, 128), "exactly full"), ((129, 128), "over by 128"), ((127, 129), "one short")]


@functools.lru_cache(maxsize=None)
def cap_edge_problem(sizes):
    """every column the same positive vector: n1 n2 exact ties; three signals"""
    rng = np.random.default_rng([142] + list(sizes))
    M = 12
    col = np.abs(rng.standard_normal(M)) + 0.2
    A = np.ascontiguousarray(np.tile(col[:, None], (1, sum(sizes))))
    Y = np.stack([1.5 * col, col + 0.01 * rng.standard_normal(M), 0.3 * col + 0.05 * np.abs(rng.standard_normal(M))])
    return _frozen(A, Y) + (np.array(sizes),)


# ---- C. ties across the seams of the tiles
MIRROR_N, MIRROR_M, MIRROR_V = 70, 20, 60
MIRROR_SEED = 2      # of seeds 0 .. 15 the one with most signals whose oracle answer is swapped AND straddles the seam
MIRROR_SHAPES = [(70, 70), (70, 70, 1)]


@functools.lru_cache(maxsize=None)
def mirror_problem(sizes, seed=MIRROR_SEED):
    """(A, Y [60 x 20], dicsizes, pairs [60 x 2]): two bit-identical sub-dictionaries D of 70 atoms (and a CSF-like column),
    as _ties_cases.symmetric_problem; signal v is 0.6 D_i + 0.3 D_j (+ 0.1 csf) + 0.02 noise with (i, j) drawn per
    signal.  The tuples (i, j) and (j, i) hold the same columns; with min(i, j) < 64 <= max(i, j) they lie in the tiles
    (0, 1) and (1, 0)."""
    rng = np.random.default_rng([143, seed])
    N, M = MIRROR_N, MIRROR_M
    D = np.abs(rng.standard_normal((M, N))) + 0.2
    csf = np.exp(-np.linspace(0, 3, M))
    k3 = len(sizes) == 3
    pairs = np.array([rng.choice(N, 2, replace=False) for _ in range(MIRROR_V)])
    noise = 0.02 * rng.standard_normal((MIRROR_V, M))
    Y = 0.6 * D[:, pairs[:, 0]].T + 0.3 * D[:, pairs[:, 1]].T + (0.1 * csf[None, :] if k3 else 0.0) + noise
    A = np.ascontiguousarray(np.hstack([D, D] + ([csf[:, None]] if k3 else [])))
    return _frozen(A, np.ascontiguousarray(Y), pairs)[:2] + (np.array(sizes), pairs)


def straddling(pairs):
    return int(np.count_nonzero((pairs.min(axis=1) < 64) & (pairs.max(axis=1) >= 64)))


@functools.lru_cache(maxsize=None)
def two_block_batch():
    """two_block_tie_problem()'s [3, 300] dictionary (column 2 of the first sub-dictionary duplicates its column 0, column
    290 of the second its column 5) and three signals: its own, made of (0, 5); one made of (2, 290) - the same two
    vectors, named by their duplicates; the first with other noise."""
    A, y, sz = TC.two_block_tie_problem()
    rng = np.random.default_rng(144)
    Y = np.stack([y, 0.7 * A[:, 2] + 0.4 * A[:, 3 + 290] + 0.01 * rng.standard_normal(12),
                  0.7 * A[:, 0] + 0.4 * A[:, 3 + 5] + 0.01 * rng.standard_normal(12)])
    return _frozen(np.ascontiguousarray(A), Y) + (sz,)


def k3_tiled_twin(seed):
    """[4, 3, 1], the tiled three-dictionary class: column 3 of the first sub-dictionary duplicates its column 0, the signal
    is made of (0, 1, 0): the triples (0, 1, 0) and (3, 1, 0) tie exactly."""
    rng = np.random.default_rng([145, seed])
    M = 10
    A1, A2, A3 = (np.abs(rng.standard_normal((M, n))) + 0.2 for n in (4, 3, 1))
    A1[:, 3] = A1[:, 0]
    y = 0.5 * A1[:, 0] + 0.3 * A2[:, 1] + 0.2 * A3[:, 0] + 0.01 * rng.standard_normal(M)
    return np.ascontiguousarray(np.hstack([A1, A2, A3])), y, np.array([4, 3, 1])


# ---- D. near-twin atoms, and signals of very different magnitudes
TWIN_V = 48
TWIN_FLOOR = {"margin": 10, "window": 40}      # signals with a runner-up inside the window (measured: see the host test)


@functools.lru_cache(maxsize=None)
def twin_problem(ladder, csf):
    """(A, Y [48 x 62], dicsizes): two family dictionaries of 12 atoms x 8 near copies (_twin_cases.family_dictionary) on
    the scheme of _units_cases.model(20, 96), [96, 96] or, with the model's CSF column, [96, 96, 1]; signal v is
    0.6 A1_i + 0.3 A2_j plus noise at SNR 30 (sigma = mean of the noise-free signal / 30), the same 48 signals for
    both classes."""
    mdl = UC.model(20, 96)
    rng = np.random.default_rng([5, len(ladder)])
    A1, _ = TW.family_dictionary(rng, mdl["sch"], 12, 8, ladder)
    A2, _ = TW.family_dictionary(rng, mdl["sch"], 12, 8, ladder)
    rs = np.random.default_rng([146, sorted(TW.LADDERS).index(ladder)])
    Y = np.zeros((TWIN_V, mdl["M"]))
    for v in range(TWIN_V):
        clean = 0.6 * A1[:, rs.integers(96)] + 0.3 * A2[:, rs.integers(96)]
        Y[v] = clean + np.mean(clean) / 30.0 * rs.standard_normal(mdl["M"])
    cols = [A1, A2] + ([mdl["sig_csf"][:, None]] if csf else [])
    return _frozen(np.ascontiguousarray(np.hstack(cols)), Y) + (np.array([96, 96, 1] if csf else [96, 96]),)


MAGNITUDES = (-300, -40, 0, 40, 300)


def magnitude_scales(V):
    """2 ** k per row, k cycling through MAGNITUDES: exact scalings, |y|^2 over 2^-600 .. 2^600 and normal"""
    return 2.0 ** np.array([MAGNITUDES[v % len(MAGNITUDES)] for v in range(V)], dtype=np.float64)
