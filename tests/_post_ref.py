"""Referee of the soft fits (include/mfx_post.h) for tests/test_post_host.py and tests/test_post_gpu.py.

The value F of every atom pair is restated on the host from the oracle's rotation (orc.interp, through the helpers of
tests/test_profile_gpu.py): without CSF the two-variable closed form, with CSF the best of all eight supports of the
three unknowns.  The kernel's cut is applied: a pair whose 1 - c^2 is not above mfx_profile_cut() is scored without
the supports that hold both of its atoms.  Weights and log-sum then follow the header's definitions with exp in the
working precision and the shift at the referee's own minimum.  Every function takes the working precision ``dt``:
long double is the referee, float64 its plain NumPy restatement.

The bar is derived, not measured.  A pair's F carries at most B = 16 M eps ||y||^2 / (1 - c^2) (the profile tests'
derivation; B = 16 M eps ||y||^2 for a pair at or below the cut, which is scored as a single atom), hence t = exp(-F / T)
a relative error of at most expm1(B / T).  With e(i, j) = t_ref expm1(B / T) / Z_ref, E_k[i] its row or column sum and
E its total, a weight may differ from the referee's by 2 (E_k[i] + w_ref E) + (N^2 + 4096) eps and log_sum by
2 E + (N^2 + 4096) eps: the factor 2 covers numerator and denominator moving together, the eps term summation, the exp
and the rounding of its argument.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_profile_gpu as TP   # noqa: E402  (helpers only: models, plans, the oracle's rotation)

LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)


def gram(y, D0, D1, x=None, dt=LD):
    y, D0, D1 = y.astype(dt), D0.astype(dt), D1.astype(dt)
    g = {"ysq": y @ y, "A11": (D0 * D0).sum(0)[:, None], "A22": (D1 * D1).sum(0)[None, :], "A12": D0.T @ D1,
         "Y1": (D0.T @ y)[:, None], "Y2": (D1.T @ y)[None, :]}
    if x is not None:
        x = x.astype(dt)
        g.update(X1=(D0.T @ x)[:, None], X2=(D1.T @ x)[None, :], xx=x @ x, xy=x @ y)
    return g


def pair_values(g, csf, cut):
    """(F [N x N] with the cut applied, the 1 - c^2 that enters the bar (1 where the pair is cut), every 1 - c^2 the
    kernel tests against the cut, the mask of cut pairs)"""
    A11, A22, A12, Y1, Y2 = (g[k] for k in ("A11", "A22", "A12", "Y1", "Y2"))
    c2u = 1 - A12 ** 2 / (A11 * A22)
    s = np.maximum(TP._single(Y1, A11), TP._single(Y2, A22))
    both = TP._pair_inner(A11, A22, A12, Y1, Y2)
    if not csf:
        below = c2u <= cut
        s = np.where(below, s, np.maximum(s, both))
        return g["ysq"] - s, np.where(below, 1.0, c2u), [c2u], below
    X1, X2, xx, xy = (g[k] for k in ("X1", "X2", "xx", "xy"))
    A11p, A22p, A12p = A11 - X1 * X1 / xx, A22 - X2 * X2 / xx, A12 - X1 * X2 / xx
    c2p = 1 - A12p ** 2 / (A11p * A22p)
    below = c2p <= cut
    s = np.maximum(s, TP._single(xy, xx))
    s = np.maximum(s, TP._pair_inner(A11, xx, X1, Y1, xy))
    s = np.maximum(s, TP._pair_inner(A22, xx, X2, Y2, xy))
    # all three: Cramer's rule on [[A11 A12 X1] [A12 A22 X2] [X1 X2 xx]] w = [Y1 Y2 xy]
    c00, c01, c02 = A22 * xx - X2 * X2, X1 * X2 - A12 * xx, A12 * X2 - A22 * X1
    c11, c12, c22 = A11 * xx - X1 * X1, A12 * X1 - A11 * X2, A11 * A22 - A12 * A12
    det = A11 * c00 + A12 * c01 + X1 * c02
    w1 = c00 * Y1 + c01 * Y2 + c02 * xy
    w2 = c01 * Y1 + c11 * Y2 + c12 * xy
    w3 = c02 * Y1 + c12 * Y2 + c22 * xy
    ok = (det > 0) & (w1 > 0) & (w2 > 0) & (w3 > 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        three = np.where(ok, (Y1 * w1 + Y2 * w2 + xy * w3) / det, -np.inf)
    s = np.where(below, s, np.maximum(s, np.maximum(both, three)))
    return g["ysq"] - s, np.where(below, 1.0, c2p), [c2u, c2p], below


def clear_of_the_cut(c2s, cut):
    """the input condition of every comparison: no pair within [cut / 4, 4 cut], where it could fall on either side, and
    every 1 - c^2 the kernel tests (plain and CSF-projected) on the same side"""
    side = None
    for c2 in c2s:
        if np.any((c2 >= cut / 4) & (c2 <= 4 * cut)):
            return False
        if side is not None and not np.array_equal(side, c2 <= cut):
            return False
        side = c2 <= cut
    return True


def posterior(F, c2bar, ysq, M, T, dt=LD):
    """weights, log_sum and their bars from the pair values: dict(w=[w0, w1], log_sum, bar_w=[b0, b1], bar_log_sum,
    Fmin, gap (distance of the two smallest F), neff (effective number of pairs that carry the sum))"""
    T = dt(T)
    N = F.shape[0]
    Fmin = F.min()
    t = np.exp(-(F - Fmin) / T)
    Z = t.sum()
    w = [t.sum(1) / Z, t.sum(0) / Z]
    e = t * np.expm1(16 * M * EPS * dt(ysq) / c2bar.astype(dt) / T) / Z
    E = e.sum()
    tail = (N * N + 4096) * EPS
    two = np.partition(F.reshape(-1), 1)[:2]
    return {"w": w, "log_sum": np.log(Z) - Fmin / T, "bar_w": [2 * (e.sum(1) + w[0] * E) + tail, 2 * (e.sum(0) + w[1] * E) + tail],
            "bar_log_sum": 2 * E + tail, "Fmin": float(Fmin), "gap": float(two[1] - two[0]),
            "neff": float(1 / ((t / Z) ** 2).sum())}


def voxel(kind, y, pk, csf, T, cut, dt=LD):
    """the referee of one two-fascicle voxel (``posterior``'s dict plus ``clear``: the input condition holds)"""
    g = gram(y, TP._rot(kind, pk[:3]), TP._rot(kind, pk[3:6]), TP._sig_csf(kind) if csf else None, dt)
    F, c2bar, c2s, below = pair_values(g, csf, cut)
    r = posterior(F, c2bar, float(g["ysq"]), y.shape[0], T, dt)
    r.update(clear=clear_of_the_cut(c2s, cut), ysq=float(g["ysq"]), F=F, ncut=int(below.sum()),
             c2min=float(min(c2[c2 > cut].min() for c2 in c2s)))
    return r


def worst_ratio(w, log_sum, ref):
    """largest |got - referee| / bar over both fascicles' weights and the log-sum"""
    r = max(float(np.max(np.abs(np.asarray(w[k]).astype(LD) - ref["w"][k]) / ref["bar_w"][k])) for k in range(2))
    return max(r, float(abs(LD(log_sum) - ref["log_sum"]) / ref["bar_log_sum"]))
