"""NumPy restatement of the resampling rule of the bootstrap conditional on measurement weights (include/mfx_wboot.h)
for tests/test_wboot_host.py and tests/test_wboot_gpu.py, on the generator, mulhi32 and scale of tests/_boot_ref.py.
Every line is one rounded float64 operation in the header's order, so that bits can be compared."""
import numpy as np

import _boot_ref as R


def status_of(y, p, w, n_act):
    """The first code that applies: 3 a weight negative or not finite, 4 no positive weight, 2 y or p not finite,
    1 M+ <= n_act, 0 fine."""
    if not np.all(np.isfinite(w) & (w >= 0)):
        return 3
    if not np.any(w > 0):
        return 4
    if not (np.all(np.isfinite(y)) and np.all(np.isfinite(p))):
        return 2
    if np.count_nonzero(w > 0) <= n_act:
        return 1
    return 0


def positive_group_lists(groups, w):
    """For every row m of positive weight: the rows of positive weight of its group, ascending (None for the others)."""
    g = np.asarray(groups)
    return [np.flatnonzero((g == g[m]) & (w > 0)) if w[m] > 0 else None for m in range(g.shape[0])]


def resample(Y, P, W, params, F, c, B, kind, seed, inflate, offset=0, groups=None, vox=None, draws=None):
    """(Ystar [V, B, M], status [V]) by the rule of mfx_wboot.h; W [V, M] or [M]; kind 0 wild, 1 residual within groups.
    ``draws``: a list that receives (v, b, m, j) for every draw of the residual kind."""
    Y, P, W = (np.asarray(a, dtype=np.float64) for a in (Y, P, W))
    V, M = Y.shape
    out = np.empty((V, B, M))
    status = np.zeros(V, dtype=np.int32)
    ms = np.arange(M, dtype=np.uint64)
    for v in range(V):
        w = W if W.ndim == 1 else W[v]
        n_act = R.n_active(params[v], F, c, False)
        status[v] = status_of(Y[v], P[v], w, n_act)
        if status[v]:
            out[v] = np.nan
            continue
        pos = w > 0
        a = R.scale(int(np.count_nonzero(pos)), n_act, inflate)
        iv = int(vox[v]) if vox is not None else v
        base = (int(offset) + iv * M) & ((1 << 64) - 1)
        idx = np.uint64(base) + ms            # m is the row of the full protocol; wraps modulo 2^64
        r = Y[v] - P[v]
        s = np.sqrt(w)
        lists = positive_group_lists(groups, w) if kind == 1 else None
        for b in range(B):
            u = R.philox_word0(idx, b, seed)
            if kind == 0:
                ar = a * r
                sg = np.where((u & np.uint64(1)) == 0, 1.0, -1.0)
                new = P[v] + sg * ar
            else:
                e = s * r
                j = np.array([lists[m][int(R.mulhi32(u[m], lists[m].size))] if pos[m] else m for m in range(M)])
                if draws is not None:
                    draws.extend((v, b, m, int(j[m])) for m in range(M) if pos[m])
                ae = a * e[j]
                with np.errstate(divide='ignore', invalid='ignore'):
                    new = P[v] + ae / s
            out[v, b] = np.where(pos, new, Y[v])
    return out, status
