#!/usr/bin/env python3
"""Generate tests/golden/mcf_hp_cases.npz: 50-digit values of the MCF signal for inputs designed
around the places where csrc/mcf.hip can go wrong (matrix size and padding, squaring count, row
swaps in the Pade solve, DDE block handling), with the error of the float64 formulation beside them.

Nothing here comes from the float64 code under test except the tables handed to it: the signal is

    R = expm(-tau (p Lam - i q B)) diag(exp(-lam D (Delta - delta) / L^2)) expm(-tau (p Lam + i q B))
    E = |R[0,0]| exp(-b_par D),      p = D T / L^2,  q = gamma T L G_perp,  tau = delta / T

(for DDE R = R2 diag(exp(-lam D tmix / L^2)) R1, T the sum of all five times), evaluated with mpmath
at 50 digits from the exact values of the float64 inputs (scheme row, L, D, envdir, gamma, tables),
direction decomposition included, and rounded once to float64.  Lam and B are real, so the left
exponential is the complex conjugate of the right one; it is formed by conjugation, and an
exponential with q = 0 (a diagonal matrix) elementwise.  Both are identities, not approximations.

Stored per case: the inputs as the API takes them, E50, E_par, the squaring count s per encoding
block that csrc/mcf.hip's mcf_expm takes (restated in NumPy: exact 1-norm, theta_13, ceil(log2)),
where the Pade solve of each block swaps rows (V - U restated in NumPy, scipy.linalg.lu_factor's
pivots), whether the public API admits the case (q/p check, M <= 60) or only the C ABI does, and
the absolute error of the reference's float64 formulation (two scipy.linalg.expm per block and the
matrix products, as the reference writes them).  K_scipy is the largest

    err_scipy / (2^-52 E_par sum_b 2^s_b)

over all cases; the tests use 4 K_scipy as the bar for the kernel (see tests/test_mcf_hp_gpu.py).

Table sets: 0 = the cylinder tables at M = 64 from the closed form (exact_cylinder_tables: mpmath
Bessel zeros, Grebenkov's matrix elements), 1.. = synthetic tables (an ascending lam starting at 0,
a real symmetric B) built so that the Pade solve has to swap rows.

Usage:  python tests/golden/gen_golden_mcf_hp.py
(218 s on 8 CPUs; at most 16 processes are used, and the 64 x 64 DDE cases, about 100 s each, set the floor)
The module is also imported by tests/test_mcf_hp_host.py, which recomputes part of the fixture.
"""
import os
import time

os.environ.setdefault("OPENBLAS_NUM_THREADS", "1")
os.environ.setdefault("OMP_NUM_THREADS", "1")

import numpy as np  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "mcf_hp_cases.npz")
GAMMA = 2 * np.pi * 42.577480e6
THETA13 = 5.371920351148152
PADE13 = (64764752532480000., 32382376266240000., 7771770303897600., 1187353796428800.,
          129060195264000., 10559470521600., 670442572800., 33522128640.,
          1323241920., 40840800., 960960., 16380., 182., 1.)
M_SET = (1, 2, 3, 15, 16, 17, 31, 32, 33, 47, 48, 49, 59, 60, 61, 63, 64)
S_GROUPS = ((0, 0), (1, 8), (9, 14), (15, 1000))
EPS = 2.0 ** -52


# ----------------------------------------------------------------------------------------------
# exact tables
# ----------------------------------------------------------------------------------------------
def exact_cylinder_modes(M, dps=50):
    """[(alpha, n)] of the first M Neumann modes of the unit disk (J_n'(alpha) = 0, the constant mode
    first), alpha as mpmath numbers: scipy's zeros are only the starting points of mp.findroot."""
    import mpmath as mp
    from scipy import special as sp
    mp.mp.dps = dps
    cand = [(0.0, 0)]
    n = 0
    while True:
        z = sp.jnp_zeros(n, M)
        if len(cand) >= M and z[0] > sorted(a for a, _ in cand)[M - 1]:
            break
        cand += [(float(a), n) for a in z]
        n += 1
    cand.sort()
    modes = []
    for a, k in cand[:M]:
        if a == 0.0:
            modes.append((mp.mpf(0), 0))
        else:
            modes.append((mp.findroot(lambda x, k=k: mp.besselj(k, x, derivative=1), mp.mpf(a)), k))
    assert all(modes[i][0] < modes[i + 1][0] for i in range(M - 1))
    return modes


def exact_cylinder_tables(M, dps=50):
    """(lam [M], B [M, M], order [M]) in float64 from the closed form
    B_ij = [|n_i - n_j| = 1] sqrt(1 + [n_i = 0] + [n_j = 0]) beta_i beta_j (lam_i + lam_j - 2 n_i n_j) / (lam_i - lam_j)^2,
    beta = sqrt(lam / (lam - n^2)), beta = 1 for the constant mode (Grebenkov 2008)."""
    import mpmath as mp
    modes = exact_cylinder_modes(M, dps)
    lam = [a * a for a, _ in modes]
    beta = [mp.mpf(1) if l == 0 else mp.sqrt(l / (l - n * n)) for l, (_, n) in zip(lam, modes)]
    B = np.zeros((M, M))
    for i in range(M):
        for j in range(M):
            ni, nj = modes[i][1], modes[j][1]
            if abs(ni - nj) != 1:
                continue
            eps = mp.sqrt(1 + (ni == 0) + (nj == 0))
            B[i, j] = float(eps * beta[i] * beta[j] * (lam[i] + lam[j] - 2 * ni * nj) / (lam[i] - lam[j]) ** 2)
    return np.array([float(l) for l in lam]), B, np.array([n for _, n in modes])


# ----------------------------------------------------------------------------------------------
# the three evaluations of one case: 50 digits, the reference's float64 formulation, the kernel's s
# ----------------------------------------------------------------------------------------------
def _times(row, dde):
    if dde:
        return row[4] + row[5] + row[6] + row[11] + row[12]
    return row[4] + row[5]


def signal_mp(row, L, D, envdir, gamma, lam, B, M, dde, dps=50):
    """(E, E_par) as mpmath numbers at `dps` digits from the exact values of the float64 inputs."""
    import mpmath as mp
    mp.mp.dps = dps
    f = lambda x: mp.mpf(float(x))  # noqa: E731
    row = [f(x) for x in row]
    L, D, gamma = f(L), f(D), f(gamma)
    e = [f(x) for x in envdir]
    en = mp.sqrt(sum(x * x for x in e))
    e = [x / en for x in e]
    lamv = [f(x) for x in lam[:M]]
    nblk = 2 if dde else 1
    T = _times(row, dde)
    p = D * T / L ** 2
    v = [mp.mpc(1 if i == 0 else 0) for i in range(M)]
    bpar = mp.mpf(0)
    for b in range(nblk):
        g, G, Del, dl = row[7 * b:7 * b + 3], row[7 * b + 3], row[7 * b + 4], row[7 * b + 5]
        dot = sum(x * y for x, y in zip(g, e))
        par = [dot * x for x in e]
        perp = [x - y for x, y in zip(g, par)]
        Gpar = G * mp.sqrt(sum(x * x for x in par))
        Gperp = G * mp.sqrt(sum(x * x for x in perp))
        q = gamma * T * L * Gperp
        tau = dl / T
        d = [mp.exp(-l * D * (Del - dl) / L ** 2) for l in lamv]
        if q == 0:
            x = [mp.exp(-tau * p * l) for l in lamv]
            v = [x[i] * d[i] * x[i] * v[i] for i in range(M)]
        else:
            A = mp.matrix(M, M)
            for i in range(M):
                for j in range(M):
                    if B[i, j] != 0.0:
                        A[i, j] = mp.mpc(0, -tau * q * f(B[i, j]))
                A[i, i] += -tau * p * lamv[i]
            X = mp.expm(A, method='taylor')
            v = [sum(X[i, j] * v[j] for j in range(M)) for i in range(M)]
            v = [d[i] * v[i] for i in range(M)]
            v = [sum(mp.conj(X[i, j]) * v[j] for j in range(M)) for i in range(M)]
        if dde and b == 0:
            v = [mp.exp(-l * D * row[6] / L ** 2) * v[i] for i, l in enumerate(lamv)]
        bpar += (gamma * dl * Gpar) ** 2 * (Del - dl / 3)
    Epar = mp.exp(-bpar * D)
    return abs(v[0]) * Epar, Epar


def signal_ref64(row, L, D, envdir, gamma, lam, B, M, dde):
    """The reference's float64 formulation (its mcf.py, the loops of MCF_DDE and MCF_PGSE): two
    scipy.linalg.expm per block, dense products, Epurediff ** (time / Tmax) with Tmax this row's T."""
    from scipy.linalg import expm
    row = np.asarray(row, dtype=np.float64)
    envdir = np.asarray(envdir, dtype=np.float64)
    envdir = envdir / np.sqrt(np.sum(envdir ** 2))
    Lamvec = np.asarray(lam[:M], dtype=np.float64)
    Lam, Bm = np.diag(Lamvec), np.asarray(B[:M, :M], dtype=np.float64)
    T_i = _times(row, dde)
    with np.errstate(under='ignore'):
        Epurediff = np.exp(-Lamvec * D * T_i / L ** 2)
        p = D * T_i / L ** 2
        R, bpar = None, 0.0
        for b in range(2 if dde else 1):
            gdir, G, Del, dl = row[7 * b:7 * b + 3], row[7 * b + 3], row[7 * b + 4], row[7 * b + 5]
            gpar = np.dot(gdir, envdir) * envdir
            gperp = gdir - gpar
            Gpar = G * np.sqrt(np.sum(gpar ** 2))
            Gperp = G * np.sqrt(np.sum(gperp ** 2))
            qperp = gamma * T_i * L * Gperp
            Rb = (expm(-(p * Lam - (1j) * qperp * Bm) * (dl / T_i)) @ np.diag(Epurediff ** ((Del - dl) / T_i))
                  @ expm(-(p * Lam + (1j) * qperp * Bm) * (dl / T_i)))
            if R is None:
                R = Rb
            else:
                R = Rb @ np.diag(Epurediff ** (row[6] / T_i)) @ R
            bpar = bpar + (gamma * dl * Gpar) ** 2 * (Del - dl / 3)
        return np.abs(R[0, 0]) * np.exp(-bpar * D)


def kernel_blocks(row, L, D, envdir, gamma, lam, B, M, dde):
    """What csrc/mcf.hip's host code and mcf_expm make of a case, per encoding block:
    [(s, norm / theta_13, A / 2^s as a complex M x M array)], plus the row's kind (0, 1 or 2)."""
    row = np.asarray(row, dtype=np.float64)
    e = np.asarray(envdir, dtype=np.float64)
    e = e / np.sqrt(e[0] * e[0] + e[1] * e[1] + e[2] * e[2])
    lam = np.asarray(lam[:M], dtype=np.float64)
    B = np.asarray(B[:M, :M], dtype=np.float64)
    colsum = np.array([sum(abs(B[i, j]) for i in range(M) if i != j) for j in range(M)])
    T = _times(row, dde)
    p = D * T / (L * L)
    out, any_g, any_perp = [], False, False
    for b in range(2 if dde else 1):
        g, G, dl = row[7 * b:7 * b + 3], row[7 * b + 3], row[7 * b + 5]
        dot = g[0] * e[0] + g[1] * e[1] + g[2] * e[2]
        perp = g - dot * e
        Gperp = G * np.sqrt(perp[0] * perp[0] + perp[1] * perp[1] + perp[2] * perp[2])
        any_g, any_perp = any_g or G != 0.0, any_perp or Gperp != 0.0
        q = gamma * T * L * Gperp
        tau = dl / T
        dr, di = (p * lam) * tau, (q * np.diag(B)) * tau
        nrm = float(np.max(np.sqrt(dr * dr + di * di) + abs(q * tau) * colsum))
        s = int(np.ceil(np.log2(nrm / THETA13))) if nrm > THETA13 else 0
        A = (-(np.diag((p * lam) * tau)) - 1j * ((q * B) * tau)) * 2.0 ** -s
        out.append((s, nrm / THETA13, A))
    return out, (0 if not any_g else (1 if not any_perp else 2))


def pade13_uv(A):
    """(U, V) of the [13/13] Pade approximant in scipy's (and the kernel's) formulas and summation order."""
    b = PADE13
    I = np.eye(A.shape[0])
    A2 = A @ A
    A4 = A2 @ A2
    A6 = A4 @ A2
    U = A @ (A6 @ (b[13] * A6 + b[11] * A4 + b[9] * A2) + b[7] * A6 + b[5] * A4 + b[3] * A2 + b[1] * I)
    V = A6 @ (b[12] * A6 + b[10] * A4 + b[8] * A2) + b[6] * A6 + b[4] * A4 + b[2] * A2 + b[0] * I
    return U, V


def solve_swaps(A):
    """The steps k at which partial pivoting on V - U swaps rows, and the rows swapped in: [(k, row)]."""
    from scipy.linalg import lu_factor
    U, V = pade13_uv(A)
    _, piv = lu_factor(V - U)
    return [(int(k), int(r)) for k, r in enumerate(piv) if r != k]


def kernel_model(row, L, D, envdir, gamma, lam, B, M, dde, s_shift=0, bad_swap=False):
    """NumPy restatement of csrc/mcf.hip (float64 Pade 13, Gauss-Jordan with partial pivoting on the
    64 x 64 padded matrix, s squarings, the R[0,0] contractions), to separate what float64 Pade-13
    does from what the kernel does.  s_shift and bad_swap break it on purpose (the suite's teeth)."""
    row = np.asarray(row, dtype=np.float64)
    blocks, kind = kernel_blocks(row, L, D, envdir, gamma, lam, B, M, dde)
    e = np.asarray(envdir, dtype=np.float64)
    e = e / np.sqrt(np.sum(e * e))
    lam64 = np.zeros(64)
    lam64[:M] = lam[:M]
    T = _times(row, dde)
    v = np.zeros(64, dtype=complex)
    v[0] = 1.0
    bpar = 0.0
    for b, (s, _, A) in enumerate(blocks):
        g, G, Del, dl = row[7 * b:7 * b + 3], row[7 * b + 3], row[7 * b + 4], row[7 * b + 5]
        Gpar = G * np.sqrt(np.sum((np.dot(g, e) * e) ** 2))
        bpar += (gamma * dl * Gpar) ** 2 * (Del - dl / 3.0)
        A64 = np.zeros((64, 64), dtype=complex)
        A64[:M, :M] = A
        U, V = pade13_uv(A64)
        Q, P = V - U, V + U
        for k in range(64):
            mag = np.abs(Q[k:, k].real) + np.abs(Q[k:, k].imag)
            pr = k + int(np.argmax(mag))
            if pr != k:
                Q[[k, pr]] = Q[[pr, k]]
                if not bad_swap:   # bad_swap: the right-hand side keeps its rows (any other row with a non-zero
                    P[[k, pr]] = P[[pr, k]]   # pivot would still be a valid elimination, only a less stable one)
            fac = Q[:, k] / Q[k, k]
            fac[k] = 0.0
            Q = Q - np.outer(fac, Q[k])
            P = P - np.outer(fac, P[k])
        X = P / np.diag(Q)[:, None]
        for _ in range(max(s + s_shift, 0)):   # s_shift = -1: one squaring too few for the scaling taken
            X = X @ X
        with np.errstate(under='ignore'):
            d = np.exp(-(lam64 * D) * (Del - dl) / (L * L))
            v = np.conj(X) @ (d * (X @ v))
            if dde and b == 0:
                v = np.exp(-(lam64 * D) * row[6] / (L * L)) * v
    return abs(v[0]) * np.exp(-bpar * D)


def api_admits(row, L, D, gamma, lam, M, dde):
    """The public API's own limits: M <= 60 and the q/p check of Grebenkov's Eq. [36]."""
    if M > 60:
        return False
    Gmax = max(row[3], row[10]) if dde else row[3]
    return bool((gamma * L) * (L ** 2 / D) * Gmax < lam[M - 1])


def scale_of(E_par, s):
    """The unit of the bar: 2^-52 E_par sum_b 2^s_b."""
    s = np.atleast_2d(s)
    return EPS * np.asarray(E_par) * np.sum(np.where(s >= 0, 2.0 ** np.maximum(s, 0), 0.0), axis=-1)


def s_group(smax):
    return [i for i, (lo, hi) in enumerate(S_GROUPS) if lo <= smax <= hi][0]


# ----------------------------------------------------------------------------------------------
# cases
# ----------------------------------------------------------------------------------------------
X_, Y_, Z_ = np.eye(3)
OBL = np.array([1.0, 1.0, 1.0]) / np.sqrt(3.0)


def pgse_row(g, G, Del, dl):
    r = np.zeros(14)
    r[0:3], r[3], r[4], r[5], r[6] = g, G, Del, dl, Del + dl + 0.01
    return r


def dde_row(g1, G1, Del1, dl1, tmix, g2, G2, Del2, dl2):
    return np.r_[g1, G1, Del1, dl1, tmix, g2, G2, Del2, dl2, Del1 + dl1 + tmix + Del2 + dl2 + 0.005]


PGSE_ROWS = (pgse_row(X_, 0.06, 0.03, 0.01),
             pgse_row(np.array([0.6, 0.0, 0.8]), 0.04, 0.0431, 0.0106),
             pgse_row(Y_, 0.2, 0.02, 0.008))
D_POOL = (2e-9, 0.7e-9, 3e-9)


class Builder:
    def __init__(self, tables):
        self.tables = tables            # [(lam[64], B[64, 64], M_valid)]
        self.cases = []

    def add(self, group, row, L, D, M, tab=0, env=Z_, dde=False, gamma=GAMMA):
        lam, B, Mv = self.tables[tab]
        assert 1 <= M <= Mv
        row = np.asarray(row, dtype=np.float64)
        blocks, kind = kernel_blocks(row, L, D, env, gamma, lam, B, M, dde)
        assert kind == 2, "case %s is not matrix work" % group
        for s, ratio, _ in blocks:   # s must not hinge on the last bits of the norm
            assert ratio <= 1.0 or abs(np.log2(ratio) - round(np.log2(ratio))) > 1e-6
        self.cases.append(dict(group=group, row=row, L=float(L), D=float(D), M=int(M), tab=int(tab),
                               env=np.asarray(env, dtype=np.float64), dde=bool(dde), gamma=float(gamma)))
        return blocks

    def s_of(self, row, L, D, M, tab=0, env=Z_, dde=False):
        lam, B, _ = self.tables[tab]
        return [b[0] for b in kernel_blocks(row, L, D, env, GAMMA, lam, B, M, dde)[0]]

    def ratio_of(self, row, L, D, M, tab=0, env=Z_):
        lam, B, _ = self.tables[tab]
        return kernel_blocks(row, L, D, env, GAMMA, lam, B, M, False)[0][0][1]

    def radii_by_s(self, row, D, M, admissible=True, env=Z_):
        """{s: L} over a log grid of radii from 0.04 um to 60 um: for every s that occurs (and, if
        asked, passes the q/p check) the radius in the middle of its run."""
        lam = self.tables[0][0]
        runs = {}
        for L in np.geomspace(0.04e-6, 60e-6, 600):
            if admissible and not api_admits(row, L, D, GAMMA, lam, M, False):
                continue
            runs.setdefault(self.s_of(row, L, D, M, env=env)[0], []).append(L)
        return {s: v[len(v) // 2] for s, v in runs.items()}

    def boundary_radius(self, row, D, M, k):
        """L with norm / theta_13 = 2^k (bisection; the norm falls with L at these radii)."""
        lo, hi = 0.03e-6, 10e-6
        assert self.ratio_of(row, lo, D, M) > 2.0 ** k > self.ratio_of(row, hi, D, M)
        for _ in range(200):
            mid = np.sqrt(lo * hi)
            if self.ratio_of(row, mid, D, M) > 2.0 ** k:
                lo = mid
            else:
                hi = mid
        return lo


SYNTH_MULTS = (1.0, 2.0, 3.0, 0.5)
SYNTH_L, SYNTH_D, SYNTH_DEL, SYNTH_DL = 5e-6, 1e-9, 0.03, 0.01


def synth_row(mult):
    """PGSE row with q tau = gamma L G delta = mult at the synthetic cases' radius."""
    return pgse_row(X_, mult / (GAMMA * SYNTH_L * SYNTH_DL), SYNTH_DEL, SYNTH_DL)


def swaps_at(lam, B, M, mult):
    blocks, _ = kernel_blocks(synth_row(mult), SYNTH_L, SYNTH_D, Z_, GAMMA, lam, B, M, False)
    return solve_swaps(blocks[0][2])


def synthetic_tables(rng):
    """Table sets for which the Pade solve swaps rows.  A 2 x 2 block A = -i theta sigma_x gives
    V - U ~ cos(theta/2) I + i sin(theta/2) sigma_x: for pi/2 < theta < 3 pi/2 (of the scaled matrix) the
    off-diagonal entry is the larger one.  Blocks away from row 0 are coupled to it (R[0,0] has to see
    what the swap does), which is why the swaps are verified numerically per case and not assumed.
    Returns [(lam[64], B[64, 64], M_valid, base)], base = q tau at which the blocks have their theta."""
    out = []

    def table(M, blocks, links, lamstep):
        B = np.zeros((64, 64))
        for (i, j), th in blocks:
            B[i, j] = B[j, i] = th
        for (i, j), c in links:
            B[i, j] = B[j, i] = c
        lam = np.zeros(64)
        lam[:M] = lamstep * np.arange(M)
        return lam, B, M

    out.append(table(64, [((0, 1), 2.0)], [((1, 5), 0.3)], 0.05))                      # 1: first swap at row 0
    out.append(table(64, [((15, 16), 4.0)], [((0, 15), 0.6), ((0, 16), 0.4)], 0.05))   # 2: across a tile edge
    out.append(table(64, [((62, 63), 2.0)], [((0, 62), 0.7), ((0, 63), 0.5)], 0.02))   # 3: the last rows
    out.append(table(64, [((0, 1), 4.0), ((15, 16), 2.0), ((31, 32), 2.5), ((47, 48), 3.5), ((62, 63), 2.0)],
                     [((1, 15), 0.5), ((16, 31), 0.5), ((32, 47), 0.5), ((48, 62), 0.5), ((0, 63), 0.3)], 0.02))  # 4
    for M, nrm in ((4, 5.0), (6, 5.0), (8, 5.0)):                                     # 5, 6, 7: random symmetric,
        for _ in range(2000):                                                          # drawn until one swaps
            R = rng.standard_normal((M, M))
            R = R + R.T
            R *= nrm / np.max(np.sum(np.abs(R), axis=0))
            B = np.zeros((64, 64))
            B[:M, :M] = R
            lam = np.zeros(64)
            lam[:M] = 0.1 * np.arange(M)
            if any(swaps_at(lam, B, M, mult) for mult in SYNTH_MULTS):
                break
        else:
            raise SystemExit("no random symmetric %d x %d table swapped rows" % (M, M))
        out.append((lam, B, M))
    return out


def build_cases():
    t0 = time.time()
    lam64, B64, _ = exact_cylinder_tables(64)
    print("closed-form tables: %.1f s" % (time.time() - t0), flush=True)
    rng = np.random.default_rng(20260)
    tables = [(lam64, B64, 64)] + synthetic_tables(rng)
    bld = Builder(tables)

    # matrix size: every M of M_SET at a low, a middle and a high squaring count
    for mi, M in enumerate(M_SET):
        if M == 1:   # lam = [0], B = [[0]]: X = 1 whatever the radius; reaches the kernel through the C ABI only
            for i, L in enumerate((0.1e-6, 1e-6, 5e-6)):
                bld.add("size", PGSE_ROWS[i], L, D_POOL[i], 1)
            continue
        row, D = PGSE_ROWS[mi % 3], D_POOL[(mi // 3) % 3]
        if mi % 3 == 2:
            row = pgse_row(Y_, 0.03, 0.02, 0.008)     # G = 0.2 leaves the q/p check little room at M <= 60
        rs = bld.radii_by_s(row, D, M, admissible=M <= 60)
        ss = sorted(s for s in rs if s <= 20)
        pick = [ss[0], ss[len(ss) // 2], ss[-1]] if M >= 47 else [ss[0], ss[len(ss) // 3], ss[2 * len(ss) // 3], ss[-1]]
        for s in pick:
            bld.add("size", row, rs[s], D, M)

    # squaring count: every s from 0 to 21 at M = 17, 16 and 3 (cheap in mpmath), rows and D in turn
    for M in (17, 16, 3):
        for ri in range(3 if M == 17 else 1):
            row, D = PGSE_ROWS[ri] if ri < 2 else pgse_row(X_, 0.02, 0.05, 0.03), D_POOL[ri]
            rs = bld.radii_by_s(row, D, M)
            for s in sorted(rs):
                if s <= 21 and (M == 17 or s % 2 == ri % 2):
                    bld.add("s", row, rs[s], D, M)

    # both sides of a change of s: norm / theta_13 = 2^k (1 -+ 0.004)
    for M, ri, ks in ((17, 0, (3, 9, 15)), (17, 1, (6, 12)), (33, 0, (10,))):
        row, D = PGSE_ROWS[ri], D_POOL[ri]
        for k in ks:
            Lb = bld.boundary_radius(row, D, M, k)
            lo = bld.add("boundary", row, Lb * 1.002, D, M)[0]
            hi = bld.add("boundary", row, Lb * 0.998, D, M)[0]
            assert lo[0] == k and hi[0] == k + 1 and lo[1] > 0.99 * 2.0 ** k and hi[1] < 1.01 * 2.0 ** k

    # rows
    lam = lam64

    def g_limit(M, L, D):                                        # G at the q/p limit of the API
        return lam[M - 1] * D / (GAMMA * L ** 3)
    for M, radii in ((17, (0.3e-6, 2e-6, 6e-6)), (20, (1e-6,))):
        for L in radii:
            D = 1.5e-9
            Gphys = min(0.08, 0.5 * g_limit(M, L, D))
            bld.add("row:Delta=delta", pgse_row(X_, Gphys, 0.015, 0.015), L, D, M)
            bld.add("row:delta=Delta/80", pgse_row(Y_, Gphys, 0.04, 0.0005), L, D, M)
            bld.add("row:perp=1e-9", pgse_row(np.array([1e-9, 0.0, 1.0]), 0.08, 0.03, 0.01), L, D, M)
            bld.add("row:envdir", pgse_row(np.array([0.6, 0.0, 0.8]), Gphys, 0.03, 0.012), L, D, M,
                    env=np.array([0.3, -0.5, 0.81]) * 2.5)
    for M, L, D in ((17, 6e-6, 1.5e-9), (17, 10e-6, 1.5e-9), (20, 8e-6, 1.5e-9), (60, 12e-6, 1.5e-9)):
        bld.add("row:qp-limit", pgse_row(X_, 0.995 * g_limit(M, L, D), 0.03, 0.01), L, D, M)
    # signals below 1e-6: large radius, strong gradient, long pulses (found by a float64 scan; check_coverage asserts it)
    for M, L, D, fr in ((17, 6e-6, 1.5e-9, 0.25), (20, 8e-6, 2.5e-9, 0.25), (20, 8e-6, 1.5e-9, 0.7), (60, 12e-6, 2e-9, 0.25)):
        bld.add("row:low-signal", pgse_row(X_, fr * g_limit(M, L, D), 0.06, 0.03), L, D, M)

    # DDE
    def dde_variants(G):
        return [dde_row(X_, G, 0.02, 0.008, 0.005, X_, G, 0.02, 0.008),                # parallel pair
                dde_row(X_, G, 0.02, 0.008, 0.0, -X_, G, 0.02, 0.008),                # antiparallel, tmix = 0
                dde_row(X_, G, 0.02, 0.008, 0.02, Y_, G, 0.02, 0.008),                # orthogonal, tmix = 20 ms
                dde_row(X_, G, 0.015, 0.01, 0.01, Y_, 0.7 * G, 0.03, 0.004),          # different delta and Delta
                dde_row(X_, 0.0, 0.02, 0.008, 0.005, Y_, G, 0.025, 0.006),            # first block G = 0
                dde_row(OBL, G, 0.02, 0.008, 0.02, X_, 0.0, 0.02, 0.008),             # second block G = 0
                dde_row(Z_, G, 0.015, 0.01, 0.0, X_, G, 0.02, 0.008),                 # first block along the axis
                dde_row(OBL, G, 0.02, 0.008, 0.005, Z_, G, 0.03, 0.008)]              # second block along the axis
    for M, L, D, sel in ((17, 0.2e-6, 2e-9, range(8)), (17, 3e-6, 1e-9, range(8)), (60, 2e-6, 1.7e-9, (2, 3, 4)),
                         (64, 0.5e-6, 2e-9, (1, 3)), (64, 3e-6, 1e-9, (6,))):
        G = 0.05 if M > 17 else 0.04
        for vi in sel:
            bld.add("dde:%d" % vi, dde_variants(G)[vi], L, D, M, dde=True)

    # pivoting: synthetic tables through the C ABI; q tau = base x (1, 2^2, 2^5) so that the scaled blocks keep their theta
    #   gamma T L G tau = gamma L G delta = base  ->  G = base / (gamma L delta)
    def synth(tab, M, mult, dde=False):
        row = synth_row(mult)
        if dde:
            row = dde_row(X_, row[3], SYNTH_DEL, SYNTH_DL, 0.005, Y_, 0.5 * row[3], SYNTH_DEL, SYNTH_DL)
        return bld.add("pivot", row, SYNTH_L, SYNTH_D, M, tab=tab, dde=dde)
    synth(1, 64, 1.0)
    synth(1, 17, 2.0)
    synth(1, 2, 1.0)
    synth(2, 64, 1.0)
    synth(2, 17, 4.0)
    synth(3, 64, 1.0)
    synth(3, 64, 2.0)
    synth(4, 64, 1.0)
    synth(4, 64, 4.0)
    synth(4, 49, 1.0, dde=True)
    for mult in SYNTH_MULTS:
        synth(5, 4, mult)
        synth(6, 6, mult)
        synth(7, 8, mult)
    print("%d cases" % len(bld.cases), flush=True)
    return tables, bld.cases


def _mp_job(args):
    c, lam, B, dps = args
    E, Ep = signal_mp(c["row"], c["L"], c["D"], c["env"], c["gamma"], lam, B, c["M"], c["dde"], dps)
    if dps == 50:
        return float(E), float(Ep)
    return E, Ep


def analyse(tables, cases):
    """Everything stored beside E50 that needs no mpmath: s, swaps, API admission, the float64 baseline."""
    for c in cases:
        lam, B, _ = tables[c["tab"]]
        blocks, _ = kernel_blocks(c["row"], c["L"], c["D"], c["env"], c["gamma"], lam, B, c["M"], c["dde"])
        c["s"] = [b[0] for b in blocks] + [-1] * (2 - len(blocks))
        swaps = [solve_swaps(b[2]) for b in blocks]
        c["n_swaps"] = sum(len(x) for x in swaps)
        flat = [k for x in swaps for k, _ in x]
        c["swap_first"] = min((x[0][0] for x in swaps if x), default=-1)
        c["swap_max"] = max(flat, default=-1)
        c["api"] = api_admits(c["row"], c["L"], c["D"], c["gamma"], lam, c["M"], c["dde"])
        c["E64"] = float(signal_ref64(c["row"], c["L"], c["D"], c["env"], c["gamma"], lam, B, c["M"], c["dde"]))


def check_coverage(d):
    """The coverage the fixture promises, counted from the stored arrays (also run by the host test)."""
    group = [str(g) for g in d["group"]]
    M, s, dde = d["M"], d["s"], d["dde"]
    size = np.array([g == "size" for g in group])
    for m in M_SET:
        assert len(set(s[size & (M == m), 0])) >= (3 if m > 1 else 1), "matrix size %d: fewer than three s" % m
        assert np.all(~d["api"][M == m]) if m > 60 or m == 1 else np.any(d["api"][M == m])
    smax = s.max(axis=1)
    assert set(range(20)) <= set(smax.tolist()), "a squaring count in 0..19 is missing"
    bnd = np.nonzero([g == "boundary" for g in group])[0]
    assert len(bnd) >= 8 and len(bnd) % 2 == 0
    for a, b in zip(bnd[::2], bnd[1::2]):
        assert s[b, 0] == s[a, 0] + 1 and abs(d["L"][a] / d["L"][b] - 1) < 0.01 and np.array_equal(d["row"][a], d["row"][b])
    for g in ("row:Delta=delta", "row:delta=Delta/80", "row:perp=1e-9", "row:envdir", "row:qp-limit", "row:low-signal"):
        assert sum(x == g for x in group) >= 2, "row group %s is missing" % g
    r = d["row"]
    assert np.all(r[[g == "row:Delta=delta" for g in group], 4] == r[[g == "row:Delta=delta" for g in group], 5])
    assert np.all(d["E50"][[g == "row:low-signal" for g in group]] < 1e-6)
    assert np.all(d["E50"][[g == "row:low-signal" for g in group]] > 1e-12)
    for v in range(8):
        ms = set(M[[g == "dde:%d" % v for g in group]].tolist())
        assert 17 in ms, "DDE variant %d is missing" % v
    dm = set(M[dde].tolist())
    assert {17, 60, 64} <= dm
    assert np.any(dde & (r[:, 6] == 0.0)) and np.any(dde & (r[:, 6] == 0.02))
    assert np.any(dde & ((r[:, 3] == 0.0) | (r[:, 10] == 0.0)))
    piv = np.array([g == "pivot" for g in group])
    sw = d["n_swaps"] > 0
    assert np.sum(sw) >= 8, "fewer than 8 cases swap rows"
    assert np.any(d["swap_first"][sw] == 0) and np.any(d["swap_max"] >= 48) and np.any(d["swap_first"] == 15)
    assert np.any(sw & piv & dde) and np.any(sw & (d["n_swaps"] >= 4))
    assert not np.any(sw & ~piv), "a physical case swaps rows: say so in the tests"
    assert np.any(sw & (smax > 0)) and np.any(sw & (smax == 0))


def main():
    import multiprocessing as mpr
    t0 = time.time()
    tables, cases = build_cases()
    analyse(tables, cases)
    nproc = min(16, os.cpu_count() or 1)
    order = sorted(range(len(cases)), key=lambda i: -(cases[i]["M"] ** 3) * (2 if cases[i]["dde"] else 1))
    jobs = [(cases[i], tables[cases[i]["tab"]][0], tables[cases[i]["tab"]][1], 50) for i in order]
    # the 80-digit repeat: ten cheap cases (M <= 20) spread over s
    small = sorted((i for i in range(len(cases)) if cases[i]["M"] <= 20 and cases[i]["M"] > 1), key=lambda i: max(cases[i]["s"]))
    rep = [small[int(round(j * (len(small) - 1) / 9.0))] for j in range(10)]
    jobs80 = [(cases[i], tables[cases[i]["tab"]][0], tables[cases[i]["tab"]][1], 80) for i in rep]
    with mpr.Pool(nproc) as pool:
        res = []
        for n, r in enumerate(pool.imap(_mp_job, jobs, chunksize=1)):
            res.append(r)
            if n % 10 == 0:
                print("  %d / %d  (%.0f s)" % (n + 1, len(jobs), time.time() - t0), flush=True)
        res80 = pool.map(_mp_job, jobs80, chunksize=1)
    for i, (E, Ep) in zip(order, res):
        cases[i]["E50"], cases[i]["E_par"] = E, Ep
    import mpmath as mp
    mp.mp.dps = 80
    for i, (E80, _) in zip(rep, res80):
        c = cases[i]
        E50, _ = signal_mp(c["row"], c["L"], c["D"], c["env"], c["gamma"], tables[c["tab"]][0], tables[c["tab"]][1],
                           c["M"], c["dde"], 50)
        mp.mp.dps = 80
        rel = abs(E50 - E80) / abs(E80)
        print("  80-digit repeat: case %d (s = %s) differs by %s relative" % (i, c["s"], mp.nstr(rel, 3)))
        if rel > mp.mpf(10) ** -30:
            raise SystemExit("50-digit and 80-digit values differ: fixture not written")
    d = dict(
        group=np.array([c["group"] for c in cases]), row=np.stack([c["row"] for c in cases]),
        L=np.array([c["L"] for c in cases]), D=np.array([c["D"] for c in cases]),
        envdir=np.stack([c["env"] for c in cases]), gamma=np.array([c["gamma"] for c in cases]),
        M=np.array([c["M"] for c in cases], dtype=np.int64), tab=np.array([c["tab"] for c in cases], dtype=np.int64),
        dde=np.array([c["dde"] for c in cases]), api=np.array([c["api"] for c in cases]),
        s=np.array([c["s"] for c in cases], dtype=np.int64), n_swaps=np.array([c["n_swaps"] for c in cases], dtype=np.int64),
        swap_first=np.array([c["swap_first"] for c in cases], dtype=np.int64),
        swap_max=np.array([c["swap_max"] for c in cases], dtype=np.int64),
        E50=np.array([c["E50"] for c in cases]), E_par=np.array([c["E_par"] for c in cases]),
        err_scipy=np.array([abs(c["E64"] - c["E50"]) for c in cases]),
        tab_lam=np.stack([t[0] for t in tables]), tab_B=np.stack([t[1] for t in tables]),
        tab_M=np.array([t[2] for t in tables], dtype=np.int64), rep80=np.array(rep, dtype=np.int64))
    ratio = d["err_scipy"] / scale_of(d["E_par"], d["s"])
    d["K_scipy"] = np.float64(ratio.max())
    smax = d["s"].max(axis=1)
    for gi, (lo, hi) in enumerate(S_GROUPS):
        m = (smax >= lo) & (smax <= hi)
        w = np.nonzero(m)[0][np.argmax(ratio[m])]
        print("scipy baseline, s in %d..%s: %d cases, largest ratio %.3f (case %d, %s, M = %d, L = %.3g, s = %s)"
              % (lo, hi if hi < 1000 else "", m.sum(), ratio[w], w, d["group"][w], d["M"][w], d["L"][w], d["s"][w]))
    print("K_scipy = %.4f" % d["K_scipy"])
    check_coverage(d)
    if d["K_scipy"] > 8:
        raise SystemExit("K_scipy above 8: the 2^s law does not describe the baseline; fixture not written")
    np.savez_compressed(OUT, **d)
    print("wrote %s: %d cases, %d bytes, %.0f s" % (OUT, len(cases), os.path.getsize(OUT), time.time() - t0))


if __name__ == "__main__":
    main()
