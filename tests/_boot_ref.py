"""NumPy restatement of the bootstrap's rule (include/mfx_boot.h) for tests/test_boot_host.py and tests/test_boot_gpu.py:
Philox4x32-10, both resampling kinds, the scale, the value table with its validity mask and the statistics.  Every
line is one rounded float64 operation in the header's order; the sums are plain Python loops in the order of b, so that
bits can be compared."""
import math

import numpy as np

BOOT_STREAM = 0x424f4f54
SOS_STREAM = 0x534f534d
M32 = 0xFFFFFFFF
Z = np.array([0.0, 0.0, 1.0])


def philox4x32_10(ctr, key):
    """Philox4x32-10 (Salmon et al., SC'11): counter (4 words), key (2 words) -> 4 words.  Plain Python integers."""
    c = [int(x) & M32 for x in ctr]
    k0, k1 = int(key[0]) & M32, int(key[1]) & M32
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k0, p1 & M32, (p0 >> 32) ^ c[3] ^ k1, p0 & M32]
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return c


def philox_word0(idx, b, seed, stream=BOOT_STREAM):
    """Output word 0 for arrays of 64-bit indices ``idx`` and one replicate ``b``: the vectorised form of the above."""
    idx = np.asarray(idx, dtype=np.uint64)
    c0, c1 = idx & np.uint64(M32), idx >> np.uint64(32)
    c2 = np.full(idx.shape, b, dtype=np.uint64)
    c3 = np.full(idx.shape, stream, dtype=np.uint64)
    k0, k1 = np.uint64(seed & M32), np.uint64((seed >> 32) & M32)
    m = np.uint64(M32)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & m, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & m
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & m, (k1 + np.uint64(0xBB67AE85)) & m
    return c0


def mulhi32(u, n):
    return (np.asarray(u, dtype=np.uint64) * np.uint64(n)) >> np.uint64(32)


def num_params(F, c, e):
    return 1 + 2 * F + int(c) + 2 * int(e) + 2


def n_active(row, F, c, e):
    w = list(row[1:1 + F]) + ([row[1 + 2 * F]] if c else []) + ([row[1 + 2 * F + int(c)]] if e else [])
    return int(sum(1 for x in w if x > 0))


def scale(M, n_act, inflate):
    if not inflate or M <= n_act:
        return 1.0
    return math.sqrt(float(M) / float(M - n_act))


def group_lists(groups):
    """For every row m: the rows of its group, ascending."""
    g = np.asarray(groups)
    return [np.flatnonzero(g == g[m]) for m in range(g.shape[0])]


def resample(Y, P, params, F, c, e, B, kind, seed, inflate, offset=0, groups=None, vox=None):
    """(Ystar [V, B, M], status [V]) by the rule of mfx_boot.h; kind 0 wild, 1 residual within groups."""
    Y, P = np.asarray(Y, dtype=np.float64), np.asarray(P, dtype=np.float64)
    V, M = Y.shape
    out = np.empty((V, B, M))
    status = np.zeros(V, dtype=np.int32)
    lists = group_lists(groups) if kind == 1 else None
    ms = np.arange(M, dtype=np.uint64)
    for v in range(V):
        n_act = n_active(params[v], F, c, e)
        if not (np.all(np.isfinite(Y[v])) and np.all(np.isfinite(P[v]))):
            status[v] = 2
        elif M <= n_act:
            status[v] = 1
        if status[v]:
            out[v] = np.nan
            continue
        a = scale(M, n_act, inflate)
        iv = int(vox[v]) if vox is not None else v
        base = (int(offset) + iv * M) & ((1 << 64) - 1)
        idx = (np.uint64(base) + ms)          # wraps modulo 2^64 like the device's unsigned arithmetic
        r = Y[v] - P[v]
        for b in range(B):
            u = philox_word0(idx, b, seed)
            if kind == 0:
                ar = a * r
                s = np.where((u & np.uint64(1)) == 0, 1.0, -1.0)
                out[v, b] = P[v] + s * ar
            else:
                j = np.array([lists[m][int(mulhi32(u[m], lists[m].size))] for m in range(M)])
                ar = a * r[j]
                out[v, b] = P[v] + ar
    return out, status


def columns(F, c, e, nprop):
    return 2 + F + int(c) + int(e) + F * nprop


def gather(reps, params0, F, c, e, props, N):
    """(X [V, B, C], valid [V, B, C] bool, agree [V, F]) from replicate rows [V, B, np] and the original rows [V, np]."""
    reps = np.asarray(reps, dtype=np.float64)
    V, B, _ = reps.shape
    props = np.zeros((0, N)) if props is None else np.atleast_2d(props)
    nprop = props.shape[0]
    C0, C = 2 + F + int(c) + int(e), columns(F, c, e, nprop)
    X = np.full((V, B, C), np.nan)
    valid = np.zeros((V, B, C), dtype=bool)
    agree = np.zeros((V, F), dtype=np.int32)
    for v in range(V):
        for b in range(B):
            row = reps[v, b]
            vals = [row[0]] + list(row[1:1 + F]) + ([row[1 + 2 * F]] if c else []) + ([row[1 + 2 * F + int(c)]] if e else [])
            vals.append(row[-2])
            X[v, b, :C0] = vals
            valid[v, b, :C0] = True
            for k in range(F):
                nu, idd = row[1 + k], row[1 + F + k]
                ok = nu > 0 and 0 <= idd < N and idd == math.floor(idd)
                if ok:
                    X[v, b, C0 + k * nprop:C0 + (k + 1) * nprop] = props[:, int(idd)]
                    valid[v, b, C0 + k * nprop:C0 + (k + 1) * nprop] = True
                    agree[v, k] += int(idd == params0[v, 1 + F + k])
    return X, valid, agree


def reduce_column(x, valid, q):
    """[n, mean, std, min, max, quantiles] of the valid entries of x in the order of b (mfx_boot.h)."""
    xs = [float(a) for a, ok in zip(x, valid) if ok]
    n = len(xs)
    out = [float(n)] + [np.nan] * (4 + len(q))
    if n == 0:
        return np.array(out)
    S, mn, mx = xs[0], xs[0], xs[0]
    for a in xs[1:]:
        S = S + a
        mn = a if a < mn else mn
        mx = a if a > mx else mx
    mean = S / float(n)
    out[1], out[3], out[4] = mean, mn, mx
    if n > 1:
        T = 0.0
        for a in xs:
            d = a - mean
            T = T + d * d
        out[2] = math.sqrt(T / float(n - 1))
    order = sorted(range(n), key=lambda i: (xs[i], i))
    for t, qq in enumerate(q):
        pos = float(qq) * float(n - 1)
        lo = int(math.floor(pos))
        hi = min(lo + 1, n - 1)
        xl, xh = xs[order[lo]], xs[order[hi]]
        out[5 + t] = xl + (xh - xl) * (pos - float(lo))
    return np.array(out)


def reduce(X, valid, q):
    """stats [V, C, 5 + Q]."""
    V, B, C = X.shape
    return np.array([[reduce_column(X[v, :, c], valid[v, :, c], q) for c in range(C)] for v in range(V)]).reshape(V, C, 5 + len(q))


def golden_model():
    """(d, sch, sig_csf, sig_ear): tests/golden/fit_cases.npz with its compartment signals."""
    import os
    from oracle import oracle as orc
    d = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fit_cases.npz"))
    sch = d["sch"]
    b = (orc.GAMMA_H * sch[:, 3] * sch[:, 5]) ** 2 * (sch[:, 4] - sch[:, 5] / 3)
    sig_csf = np.exp(-sch[:, 6] / float(d["T2_csf"])) * np.exp(-b * float(d["DIFF_csf"]))
    sig_ear = np.stack([np.exp(-sch[:, 6] / float(d["T2_ear"])) * np.exp(-b * x) for x in d["DIFF_ear"]], axis=1)
    return d, sch, sig_csf, sig_ear


def oracle_predict(T, sch, params, peaks, F, c, e, sig_csf, sig_ear):
    """The prediction of parameter rows by the oracle's rotation: sum over f0.., csf, ear of (M0 nu) s, in that order."""
    from oracle import oracle as orc
    V, M = params.shape[0], sch.shape[0]
    out = np.zeros((V, M))
    for v in range(V):
        row, acc = params[v], np.zeros(M)
        for k in range(F):
            w = row[0] * row[1 + k]
            if w > 0:
                acc = acc + w * orc.interp(sch, peaks[v, 3 * k:3 * k + 3], T)[:, int(row[1 + F + k])]
        if c and row[0] * row[1 + 2 * F] > 0:
            acc = acc + (row[0] * row[1 + 2 * F]) * sig_csf
        if e and row[0] * row[1 + 2 * F + int(c)] > 0:
            acc = acc + (row[0] * row[1 + 2 * F + int(c)]) * sig_ear[:, int(row[2 + 2 * F + int(c)])]
        out[v] = acc
    return out
