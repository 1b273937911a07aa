"""What the tests of robust fits on 2-D protocols share (include/mfx_robust2d.h): the backends of tests/_robust_ref.loop_ref,
the loop a user writes by hand, and the voxels.

engine2d_backend   engine.fit2d, engine.fit2d_weighted and engine.predict2d on a RotateAtom2DTables; rows the fit could not
                   serve are predicted as NaN rows, as _robust_ref.engine_backend has them.
referee_backend    shares no kernel with the loop's fits: the CPU solver on sqrt(W) * T.rotate(dirs) (_w2d_ref.ref_row) and
                   the NumPy sum over T.rotate's columns.  K = 2 without CSF."""
import numpy as np


class engine2d_backend:
    def __init__(self, T):
        from microstructure_fingerprinting_amd import engine
        self.e, self.T = engine, T
        self.dir_status = None        # of the last fit: the directions are those of every fit of a loop

    def fit(self, Y, K, csf, peaks, maxfasc, csf_on, sig_csf):
        p, self.dir_status = self.e.fit2d(self.T, Y, K, csf, peaks, maxfasc, csf_on, sig_csf)
        return p

    def fit_w(self, Y, W, K, csf, peaks, maxfasc, csf_on, sig_csf):
        p, self.dir_status, wst = self.e.fit2d_weighted(self.T, Y, W, K, csf, peaks, maxfasc, csf_on, sig_csf)
        return p, wst

    def predict(self, params, peaks, maxfasc, csf_on, sig_csf):
        bad = self.e.predict_bad_rows(params, maxfasc, csf_on, False, self.T.N, 0)
        P, _ = self.e.predict2d(self.T, np.where(bad[:, None], 0.0, params), peaks, maxfasc, csf_on, sig_csf if csf_on else None)
        P[bad] = np.nan
        return P


class referee_backend:
    def __init__(self, T, peaks):
        import _w2d_ref as W2
        self.W2, self.T = W2, T
        self.D = [T.rotate(peaks[v].reshape(2, 3)) for v in range(peaks.shape[0])]     # [V][2, M, N]
        self.gaps = []                # the smallest top-2 gap of every fit of the loop

    def _fit(self, Y, W):
        rows = np.array([self.W2.ref_row(self.D[v], Y[v], W[v], False, None, 2, False) for v in range(Y.shape[0])])
        self.gaps.append(min(self.W2.gap(self.D[v], Y[v], W[v]) for v in range(Y.shape[0])))
        return rows

    def fit(self, Y, K, csf, peaks, maxfasc, csf_on, sig_csf):
        return self._fit(Y, np.ones_like(Y))

    def fit_w(self, Y, W, K, csf, peaks, maxfasc, csf_on, sig_csf):
        return self._fit(Y, np.broadcast_to(W, Y.shape)), np.zeros(Y.shape[0], dtype=np.int32)

    def predict(self, params, peaks, maxfasc, csf_on, sig_csf):
        P = np.zeros((params.shape[0], self.T.M))
        for v in range(params.shape[0]):
            for k in range(2):
                w = params[v, 0] * params[v, 1 + k]
                if w > 0:
                    P[v] = P[v] + w * self.D[v][k][:, int(params[v, 3 + k])]
        return P


def crossing_dirs(rng, zmin):
    while True:
        v = rng.standard_normal((24, 3))
        v /= np.sqrt(np.sum(v ** 2, axis=1, keepdims=True))
        d = np.ascontiguousarray(v[np.abs(v[:, 2]) >= zmin][:2])
        if d.shape[0] == 2 and abs(d[0] @ d[1]) <= 0.85:
            return d


def make_voxels(T, V, seed, zmin, n_bad=4):
    """The recipe of test_robust_gpu.make_voxels on the tables' own rotation: two crossing directions, a noisy mixture at
    M0 = 500 and SNR 30, n_bad random rows multiplied by U(0.1, 0.5)."""
    rng = np.random.default_rng(seed)
    M = T.M
    peaks, Y = np.zeros((V, 6)), np.zeros((V, M))
    for v in range(V):
        d = crossing_dirs(rng, zmin)
        ids = rng.integers(0, T.N, 2)
        f = rng.uniform(0.3, 0.7)
        cols = T.rotate_cols(d, ids)
        y = 500.0 * (f * cols[0] + (1.0 - f) * cols[1])
        y += rng.normal(0, 500.0 / 30.0, M)
        bad = rng.choice(M, n_bad, replace=False)
        y[bad] *= rng.uniform(0.1, 0.5, n_bad)
        peaks[v], Y[v] = d.reshape(-1), y
    return peaks, Y
