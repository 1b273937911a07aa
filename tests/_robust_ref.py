"""What the robust fit's tests share: a NumPy statement of the weight rule of include/mfx_robust.h, one rounded float64
operation per line, and of the loop fit -> predict -> reweight -> weighted fit, built only from engine.fit_batch,
engine.predict and engine.fit_weighted - the loop a user writes by hand.  `oracle_backend` swaps those three for the
CPU oracle's chain (tests/_wfit_ref.py), which needs no GPU."""
import numpy as np

LOSSES = ("cutoff", "huber", "tukey")


def rule_one(y, p, w0, loss, c):
    """One voxel: (W [M], scale, state) from data y, prediction p, base weights w0 ([M] or None)."""
    y, p = np.asarray(y, dtype=np.float64), np.asarray(p, dtype=np.float64)
    M = y.shape[0]
    base = np.ones(M) if w0 is None else np.asarray(w0, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        a = np.abs(y - p)
        B = base > 0
        if np.any(~(base >= 0) | ~np.isfinite(base)) or not B.any():
            return base.copy(), np.nan, 3
        if not np.all(np.isfinite(a[B])):
            return base.copy(), np.nan, 1
        s = np.median(a[B])          # sorted middle; even n0: (a_lo + a_hi) / 2, two roundings
        if s == 0.0:
            return base.copy(), 0.0, 2
        thr = np.float64(c) * s
        if loss == "cutoff":
            psi = np.where(a <= thr, 1.0, 0.0)
        elif loss == "huber":
            psi = np.where(a <= thr, 1.0, thr / np.where(a <= thr, 1.0, a))
        elif loss == "tukey":
            u = a / thr
            t = 1.0 - u * u
            psi = np.where(u < 1.0, t * t, 0.0)
        else:
            raise ValueError(loss)
        W = np.where(B, psi if w0 is None else base * psi, 0.0)
    return W, float(s), 0


def median_by_order(a):
    """numpy.median restated from the (value, index) order, to check that ties do not matter."""
    a = np.asarray(a, dtype=np.float64)
    order = sorted(range(a.size), key=lambda i: (a[i], i))
    n = a.size
    if n % 2:
        return a[order[(n - 1) // 2]]
    return (a[order[n // 2 - 1]] + a[order[n // 2]]) / 2.0


def weights_ref(Y, P, W0, loss, c, Wprev=None):
    """The rule on a batch: (W [V, M], scale [V], state [V] int32, changed [V] int32 or None)."""
    Y, P = np.asarray(Y, dtype=np.float64), np.asarray(P, dtype=np.float64)
    V, M = Y.shape
    W, scale, state = np.zeros((V, M)), np.zeros(V), np.zeros(V, dtype=np.int32)
    for v in range(V):
        w0 = None if W0 is None else (W0 if np.ndim(W0) == 1 else W0[v])
        W[v], scale[v], state[v] = rule_one(Y[v], P[v], w0, loss, c)
    changed = None
    if Wprev is not None:
        changed = np.any(W.view(np.int64) != np.ascontiguousarray(Wprev, dtype=np.float64).view(np.int64), axis=1).astype(np.int32)
    return W, scale, state, changed


class engine_backend:
    """The three entry points of the hand-made loop on a plan."""
    def __init__(self, plan):
        from microstructure_fingerprinting_amd import engine
        self.e, self.plan = engine, plan

    def fit(self, Y, K, csf, peaks, maxfasc, csf_on, sig_csf):
        return self.e.fit_batch(self.plan, Y, K, csf, None, peaks, maxfasc, csf_on, False, sig_csf=sig_csf)

    def fit_w(self, Y, W, K, csf, peaks, maxfasc, csf_on, sig_csf):
        return self.e.fit_weighted(self.plan, Y, W, K, csf, peaks, maxfasc, csf_on, sig_csf)

    def predict(self, params, peaks, maxfasc, csf_on, sig_csf):
        """Rows the fit could not serve (NaN parameters) are NaN, as MFModelFit.predict has them."""
        bad = self.e.predict_bad_rows(params, maxfasc, csf_on, False, self.plan.tables.N, 0)
        P = self.e.predict(self.plan, np.where(bad[:, None], 0.0, params), peaks, maxfasc, csf_on, False, sig_csf if csf_on else None)
        P[bad] = np.nan
        return P


class oracle_backend:
    """The same three on the CPU: the oracle's fit, the weighted referee of tests/_wfit_ref.py, oracle rotations."""
    def __init__(self, T, sch):
        from oracle import oracle as orc
        import _wfit_ref as R
        self.orc, self.R, self.T, self.sch = orc, R, T, sch

    def fit(self, Y, K, csf, peaks, maxfasc, csf_on, sig_csf):
        V = Y.shape[0]
        cs = np.zeros(V, bool) if csf is None else np.asarray(csf, bool)
        return self.orc.fit_batch(self.T, self.sch, Y, np.asarray(K), cs, np.zeros(V, bool), peaks, maxfasc, csf_on, False,
                                  sig_csf, None, 0)

    def fit_w(self, Y, W, K, csf, peaks, maxfasc, csf_on, sig_csf):
        rows = [self.R.ref_row(self.T, self.sch, Y[v], W[v] if np.ndim(W) == 2 else W, peaks[v, :3 * K[v]].reshape(K[v], 3),
                               bool(csf[v]) if csf is not None else False, sig_csf, maxfasc, csf_on) for v in range(Y.shape[0])]
        return np.array(rows), np.zeros(Y.shape[0], dtype=np.int32)

    def predict(self, params, peaks, maxfasc, csf_on, sig_csf):
        V, M = params.shape[0], self.sch.shape[0]
        P = np.zeros((V, M))
        for v in range(V):
            for k in range(maxfasc):
                w = params[v, 0] * params[v, 1 + k]
                if w > 0:
                    P[v] = P[v] + w * self.orc.interp(self.sch, peaks[v, 3 * k:3 * k + 3], self.T)[:, int(params[v, 1 + maxfasc + k])]
            if csf_on and params[v, 0] * params[v, 1 + 2 * maxfasc] > 0:
                P[v] = P[v] + params[v, 0] * params[v, 1 + 2 * maxfasc] * sig_csf
        return P


def loop_ref(backend, Y, K, csf, peaks, maxfasc, csf_on, sig_csf=None, W0=None, loss="cutoff", c=4.45, n_iter=3, trace=False):
    """The hand-made loop: (params, W [V, M], dict(scale, state, status, n_changed [n_iter] int64)), always all n_iter.
    trace=True: the list of these results after 0, 1, .., n_iter iterations (one run serves every shorter loop)."""
    Y = np.ascontiguousarray(Y, dtype=np.float64)
    V, M = Y.shape
    K = np.asarray(K)
    if W0 is None:
        params, status = backend.fit(Y, K, csf, peaks, maxfasc, csf_on, sig_csf), np.zeros(V, dtype=np.int32)
        W = np.ones((V, M))
    else:
        W0 = np.asarray(W0, dtype=np.float64)
        params, status = backend.fit_w(Y, W0, K, csf, peaks, maxfasc, csf_on, sig_csf)
        W = np.ascontiguousarray(np.broadcast_to(W0, (V, M)))
    scale, state = np.zeros(V), np.zeros(V, dtype=np.int32)
    n_changed = np.zeros(n_iter, dtype=np.int64)

    def snap(n):
        return params.copy(), W.copy(), dict(scale=scale.copy(), state=state.copy(), status=np.array(status), n_changed=n_changed[:n].copy())
    out = [snap(0)]
    for it in range(n_iter):
        P = backend.predict(params, peaks, maxfasc, csf_on, sig_csf)
        W, scale, state, changed = weights_ref(Y, P, W0, loss, c, Wprev=W)
        n_changed[it] = int(changed.sum())
        params, status = backend.fit_w(Y, W, K, csf, peaks, maxfasc, csf_on, sig_csf)
        out.append(snap(it + 1))
    return out if trace else out[-1]
