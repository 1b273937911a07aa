"""Cases and referee of the solver's soft answers (include/mfx_solve_soft.h) for tests/test_solve_soft_host.py and
tests/test_solve_soft_gpu.py.

Inputs: the generator of tests/test_solve_batch_gpu.py (|randn| dictionary, 37 signals: signal 0 all zero, signal 1 planted
without noise, the others 0.7 of an atom of the first sub-dictionary, 0.2 of one of every other and noise of 0.01).

Referee: tests/_post_ref.py unchanged, on the explicit dictionary's blocks: ``gram`` in long double, ``pair_values`` with
the library's cut, ``posterior``.  Its bars are derived, not measured: a pair's F carries at most B = 16 M eps ||y||^2 /
(1 - c^2) (B = 16 M eps ||y||^2 for a pair at or below the cut and for a single atom), and bar_w / bar_log_sum follow from
B as that file's docstring derives them.  Its tail term counts the pairs as N^2 for a square voxel problem; for the
n1 x n2 pairs here the wrapper puts (n1 n2 + 4096) eps in its place.  One sub-dictionary has no pairs: its F(i), weights
and bars are stated here in the same terms (B = 16 M eps ||y||^2, tail (n + 4096) eps).

Every posterior comparison runs at two noise levels: SIGMA_PEAKED (T = 5e-3), where one pair carries the sum, and the
broad leg (sigma = 2, T = 8, unless BROAD_SIGMA raises it for a case), where the referee's effective number of pairs is
at least NEFF_FLOOR for every non-zero signal - only there can a wrong or missing term of the sums be seen."""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _post_ref as PR              # noqa: E402
import test_solve_batch_gpu as SB   # noqa: E402  (helpers only: the generator)

LD, EPS, TP = PR.LD, PR.EPS, PR.TP
V = SB.V
SHAPES = [(37, 5), (1, 90), (150, 149), (64, 64), (65, 63), (63, 65), (70, 1), (33, 31, 1), (150, 149, 1), (50,)]
MS = (17, 30)
CASES = [(s, M) for s in SHAPES for M in MS]
IDS = ["%s-M%d" % ("x".join(str(n) for n in s), M) for s, M in CASES]
SIGMA_PEAKED = 0.05
NEFF_FLOOR = 40.0
# (sizes, M) -> sigma of the broad leg where 2 leaves a signal below the floor: doubled until the referee's neff reaches it
# for all 36 non-zero signals (the signal that needs it is the planted one, three times as large as the others; the
# host test asserts the floor for every case)
BROAD_SIGMA = {((37, 5), 17): 4.0, ((37, 5), 30): 4.0, ((65, 63), 30): 4.0, ((70, 1), 30): 4.0, ((33, 31, 1), 30): 4.0,
               ((50,), 17): 8.0, ((50,), 30): 8.0}


def broad_sigma(sizes, M):
    return BROAD_SIGMA.get((tuple(sizes), M), 2.0)


def sigmas(sizes, M):
    return (SIGMA_PEAKED, broad_sigma(sizes, M))


def cut():
    return TP._cut()


@functools.lru_cache(maxsize=None)
def problem(sizes, M):
    """(A [M x sum sizes], Y [37 x M], sizes) of a case, read-only"""
    A, Y, sz = SB.make_problem(sizes, M)
    for a in (A, Y):
        a.setflags(write=False)
    return A, Y, sz


def blocks(A, sizes):
    """(D0, D1 or None, x or None) of an explicit dictionary"""
    n1 = sizes[0]
    if len(sizes) == 1:
        return A[:, :n1], None, None
    n2 = sizes[1]
    return A[:, :n1], A[:, n1:n1 + n2], (A[:, n1 + n2] if len(sizes) == 3 else None)


def pair_F(A, sizes, y, dt=LD):
    """(F [n1 x n2] (one sub-dictionary: [n x 1]), the 1 - c^2 of the bar, every 1 - c^2 tested against the cut, ||y||^2)"""
    D0, D1, x = blocks(A, sizes)
    if D1 is None:
        y_, D = y.astype(dt), D0.astype(dt)
        ysq = y_ @ y_
        F = ysq - TP._single(D.T @ y_, (D * D).sum(0))
        return F[:, None], np.ones((sizes[0], 1)), [], float(ysq)
    g = PR.gram(y, D0, D1, x, dt)
    F, c2bar, c2s, _ = PR.pair_values(g, x is not None, cut())
    return F, c2bar, c2s, float(g["ysq"])


def posterior_ref(F, c2bar, ysq, M, T, dt=LD, one=False):
    """PR.posterior with the tail term of n1 x n2 pairs (n atoms for one sub-dictionary) in place of N^2"""
    r = PR.posterior(F, c2bar, ysq, M, T, dt)
    n_sq, n_here = F.shape[0] * F.shape[0], F.shape[0] * F.shape[1]
    d = (n_here - n_sq) * EPS
    r["bar_w"] = [b + d for b in r["bar_w"]]
    r["bar_log_sum"] = r["bar_log_sum"] + d
    if one:
        r["w"], r["bar_w"] = r["w"][:1], r["bar_w"][:1]
    return r


def profile_ref(F, c2bar, ysq, M, one=False):
    """per served sub-dictionary: (obj [n], partner [n], bar [n] = B of the arg-min pair, sure [n]: the runner-up is more
    than 2 B away); one sub-dictionary: F(i) itself, partner -1"""
    if one:
        n = F.shape[0]
        return [(F[:, 0], np.full(n, -1), np.full(n, 16 * M * EPS * ysq), np.ones(n, dtype=bool))]
    out = []
    for ax in (1, 0):
        Fa = F if ax == 1 else F.T
        ca = c2bar if ax == 1 else c2bar.T
        arg = np.argmin(Fa, axis=1)
        rows = np.arange(Fa.shape[0])
        obj = Fa[rows, arg]
        bar = 16 * M * EPS * ysq / np.asarray(ca[rows, arg], dtype=np.float64)
        if Fa.shape[1] > 1:
            second = np.partition(Fa, 1, axis=1)[:, 1]
            sure = np.asarray(second - obj, dtype=np.float64) > 2 * bar
        else:
            sure = np.ones(Fa.shape[0], dtype=bool)
        out.append((obj, arg, bar, sure))
    return out


@functools.lru_cache(maxsize=None)
def referee(sizes, M):
    """The long-double referee of every signal of a case, made once and shared (read-only): a list over the signals of
    dict(ysq, prof=profile_ref(..), post={sigma: posterior_ref(..)}, clear)."""
    A, Y, _ = problem(sizes, M)
    res = []
    for v in range(V):
        F, c2bar, c2s, ysq = pair_F(A, sizes, Y[v])
        post = {s: posterior_ref(F, c2bar, ysq, M, 2.0 * s * s, one=len(sizes) == 1) for s in sigmas(sizes, M)}
        res.append({"ysq": ysq, "prof": profile_ref(F, c2bar, ysq, M, one=len(sizes) == 1), "post": post, "clear": PR.clear_of_the_cut(c2s, cut())})
    return res


def worst_ratio(w, log_sum, ref):
    """largest |got - referee| / bar over the weights of every served sub-dictionary and the log-sum"""
    r = max(float(np.max(np.abs(np.asarray(w[k]).astype(LD) - ref["w"][k]) / ref["bar_w"][k])) for k in range(len(ref["w"])))
    return max(r, float(abs(LD(log_sum) - ref["log_sum"]) / ref["bar_log_sum"]))


def check_profile(tag, obj, partner, refs):
    """obj / partner: per served sub-dictionary the row of one signal; refs: profile_ref's list"""
    for k in range(len(obj)):
        robj, rarg, bar, sure = refs[k]
        err = np.abs(obj[k].astype(LD) - robj)
        ratio = float(np.max(np.where(bar > 0, err / np.where(bar > 0, bar, 1.0), 0.0)))
        print("%s axis %d: worst |obj - ref| / B = %.3g, %d of %d partners decided" % (tag, k, ratio, int(sure.sum()), sure.size))
        assert np.all(err <= bar), "%s axis %d: objective beyond B" % (tag, k)
        if partner is not None:
            assert np.array_equal(partner[k][sure], rarg[sure]), "%s axis %d: partner" % (tag, k)
