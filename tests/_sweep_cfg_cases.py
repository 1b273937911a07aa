"""Cases that reach every kernel of csrc/profile.hip and csrc/posterior.hip, for tests/test_sweep_cfg_host.py and
tests/test_sweep_cfg_gpu.py.

The two files instantiate 86 kernels.  A K = 2 kernel is a *form*: one of the four configurations of soft_sweep.h
(KSTEPS, NW, TILES, NBUF), with or without G-bracketed rows (BR) and a CSF column, in one of six families: posterior,
profile, landscape and their weighted twins.  sweep_pick chooses the configuration from M <= 200, the two flags and the
LDS bytes of the dictionary; this module restates that choice (``lds_bytes``, ``pick``, ``interval``) from the kernels'
carve-up, without the library, and builds one row per form whose dictionary size lies inside the form's interval, plus
a second row at the family's limit for every (50, 4, 1, 1) and (140, 4, 1, 1) form.  The GPU test asks the library's
debug hook which form it launched; nothing here predicts it for the library.

Inputs.  One pool of 4112 atoms per multi-shell protocol (synth.make_dictionary, one seed: the same atoms on both
protocols); a dictionary of N atoms is the pool's first N.  Four subject protocols: 23 rows exact-G, its twin with half
of the diffusion rows at G strictly between the table's shells, 203 rows exact-G, and its bracketed twin.  Per protocol
two independently drawn fascicle directions (synth.make_voxels draws them) and one weight vector; per row one signal of
synth.make_voxels' recipe (two atoms among the row's N, Dirichlet fractions, M0 = 500, SNR 30) on the oracle's rotation.

What the referee shares.  A pair's |d_i|^2, |d_j|^2, d_i.d_j (and d.x, x.x) depend on the protocol, the two directions
and the weights only, and those of the first N atoms are the leading block of those of the pool.  They are computed in
long double once per (protocol, weights) at the largest N any row of that protocol uses; a row adds its own d.y, x.y and
||y||^2 (N M products).  The same blocks give every 1 - c^2 the kernels test against the cut, so the input condition of
tests/_post_ref.py (``clear_of_the_cut``) is checked once per block and holds for every leading sub-block.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _post_ref as R   # noqa: E402

LD, EPS = R.LD, R.EPS
Z = np.array([0.0, 0.0, 1.0])
POOL = 4112
SIGMA = 500.0 / 30.0
T2_CSF, DIFF_CSF = 2.0, 3.0e-9
CUT = 1e-8                      # mfx_profile_cut(); the GPU test asserts that the library says the same

# ---- the configurations and the LDS formula (soft_sweep.h: SWEEP_CFG, sweep_front, sweep_pick; the families' own arrays:
# profile.hip prof_own_dbl / prof_own_int, posterior.hip post_own_dbl / POST_OWN_INT)
SWEEP_CFG = [(50, 8, 2, 2), (50, 4, 1, 2), (50, 4, 1, 1), (140, 4, 1, 1)]
LDS_MAX = 160 * 1024
KINDS = ("post", "prof", "land")


def lds_bytes(kind, cfg, NP, br, csf, wgt):
    ks, nw, tiles, nbuf = cfg
    MP, cw = 4 * ks, 16 * tiles
    dbl = nbuf * tiles * MP * 16 + MP + (MP if csf else 0) + (MP if wgt else 0) + 2 * MP + (4 * MP if br else 0)
    dbl += 4 * NP + (2 * NP if csf else 0)
    ints = 2 * MP + (2 * MP if br else 0)
    if kind == "post":
        dbl, ints = dbl + 2 * NP + 2 * nw * cw, ints + 2
    elif kind == "prof":
        dbl, ints = dbl + 2 * NP + 4 * nw * cw, ints + NP + 2 * nw * cw
    return 8 * dbl + 4 * ints


def path(M, br, csf):
    """the configurations sweep_pick tries, in its order"""
    if M > 200:
        return [3]
    return [1, 2] if (csf or br) else [0, 1, 2]


def pick(kind, M, br, csf, wgt, NP):
    for c in path(M, br, csf):
        if lds_bytes(kind, SWEEP_CFG[c], NP, br, csf, wgt) <= LDS_MAX:
            return c
    return -1


def cfg_max(kind, c, br, csf, wgt):
    """largest padded dictionary that fits configuration c"""
    n = 0
    while lds_bytes(kind, SWEEP_CFG[c], n + 16, br, csf, wgt) <= LDS_MAX:
        n += 16
    return n


def interval(kind, M, br, csf, wgt, c):
    """(lo, hi): the padded dictionary sizes, multiples of 16, at which sweep_pick returns c"""
    p = path(M, br, csf)
    i = p.index(c)
    lo = 16 if i == 0 else cfg_max(kind, p[i - 1], br, csf, wgt) + 16
    return lo, cfg_max(kind, c, br, csf, wgt)


def max_atoms(kind, M, br, csf, wgt):
    return cfg_max(kind, path(M, br, csf)[-1], br, csf, wgt)


# ---- protocols
PROTOS = ("short", "short_br", "long", "long_br")
_DIRS = {"short": [7, 7, 7], "long": [67, 67, 67]}
_SEED = {"short": 8101, "long": 8102, "pool": 8100, "short_br": 8111, "long_br": 8112}
_DIR_SEED = {"short": 8201, "short_br": 8202, "long": 8203, "long_br": 8204}
_W_SEED = {"short": 8301, "short_br": 8302, "long": 8303, "long_br": 8304}
_cache = {}


def _memo(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def base(proto):
    return proto.split("_")[0]


def is_br(proto):
    return proto.endswith("_br")


def scheme_ms(b):
    """the multi-shell protocol the dictionary is tabulated on: 2 b0 rows and three shells"""
    from microstructure_fingerprinting_amd import synth
    return _memo(("ms", b), lambda: np.ascontiguousarray(
        synth.make_scheme(np.random.default_rng(_SEED[b]), 2, [1000, 2000, 3000], _DIRS[b])))


def scheme(proto):
    """the subject protocol: the multi-shell one, or its twin with every second diffusion row at one of four gradient
    strengths strictly between the table's shells (tests/test_fit_gpu.py's bracketed protocol)"""
    def make():
        sch = scheme_ms(base(proto)).copy()
        if is_br(proto):
            rng = np.random.default_rng(_SEED[proto])
            Gs = np.unique(sch[:, 3])
            nz = np.where(sch[:, 3] > 0)[0]
            between = [0.3 * Gs[1] + 0.7 * Gs[2], 0.55 * Gs[2] + 0.45 * Gs[3], 0.9 * Gs[2] + 0.1 * Gs[3], 0.5 * (Gs[1] + Gs[2])]
            sch[nz[::2], 3] = rng.choice(between, size=nz[::2].size)
        return np.ascontiguousarray(sch)
    return _memo(("sch", proto), make)


def M_of(proto):
    return scheme(proto).shape[0]


def pool(b):
    from microstructure_fingerprinting_amd import synth
    return _memo(("pool", b), lambda: np.ascontiguousarray(
        synth.make_dictionary(np.random.default_rng(_SEED["pool"]), scheme_ms(b), POOL)))


def interpolator(b, N):
    """the library's tables of the pool's first N atoms (host object; the device copy is made on first use)"""
    from microstructure_fingerprinting_amd import mf_utils as mfu
    return _memo(("ms_interp", b, N), lambda: mfu.init_PGSE_multishell_interp(pool(b)[:, :N], scheme_ms(b), Z))


def sig_csf(proto):
    from microstructure_fingerprinting_amd import synth
    sch = scheme(proto)
    b = (synth.GAMMA_H * sch[:, 3] * sch[:, 5]) ** 2 * (sch[:, 4] - sch[:, 5] / 3)
    return np.exp(-sch[:, 6] / T2_CSF) * np.exp(-b * DIFF_CSF)


def n_block(proto):
    """the largest dictionary any row of this protocol uses"""
    return max(r["N"] for r in rows() + k1_rows() if r["proto"] == proto)


def peaks(proto):
    """two independently drawn directions [6], as synth.make_voxels draws them"""
    from microstructure_fingerprinting_amd import synth
    def make():
        rng = np.random.default_rng(_DIR_SEED[proto])
        return np.ascontiguousarray(np.concatenate([synth.unit_vectors(rng, 1), synth.unit_vectors(rng, 1)], axis=1)[0])
    return _memo(("pk", proto), make)


def rotated(proto):
    """the oracle's rotated dictionaries (D_0, D_1), [M x n_block] each"""
    def make():
        from oracle import oracle as orc
        ms = interpolator(base(proto), n_block(proto))
        T = {"S": ms.S, "N": ms.num_subs, "G_un": ms.Gms_un, "off": ms.off, "x": ms.x_flat, "Y": ms.Y_flat,
             "scheme_DeldelTE": ms["scheme_DeldelTE"]}
        pk = peaks(proto)
        out = [orc.interp(scheme(proto), pk[3 * k:3 * k + 3], T) for k in range(2)]
        return [np.ascontiguousarray(o.reshape(o.shape[0], -1)) for o in out]
    return _memo(("rot", proto), make)


def weights(proto):
    """tests/test_wsoft_gpu.py's _weights for one voxel: real values in [0, 4], about 15 % exact zeros"""
    def make():
        rng = np.random.default_rng(_W_SEED[proto])
        M = M_of(proto)
        W = rng.uniform(0.0, 4.0, M)
        W[rng.random(M) < 0.15] = 0.0
        return np.ascontiguousarray(W)
    return _memo(("W", proto), make)


def block(proto, wgt, dt=LD):
    """what the referee shares between the rows of (protocol, weights): the scaled operands and, in precision dt, the
    Gram quantities that do not depend on y, at n_block atoms"""
    def make():
        s = np.sqrt(weights(proto)) if wgt else np.ones(M_of(proto))
        D0, D1 = (s[:, None] * D for D in rotated(proto))
        x = s * sig_csf(proto)
        a0, a1, xl = D0.astype(dt), D1.astype(dt), x.astype(dt)
        return {"s": s, "D0": D0, "D1": D1, "x": x, "A11": (a0 * a0).sum(0), "A22": (a1 * a1).sum(0), "A12": a0.T @ a1,
                "X1": a0.T @ xl, "X2": a1.T @ xl, "xx": xl @ xl}
    return _memo(("block", proto, bool(wgt), np.dtype(dt).name), make)


def block_c2(proto, wgt):
    """every 1 - c^2 the kernels test against the cut, at n_block atoms: [plain, CSF-projected]"""
    b = block(proto, wgt)
    A11, A22, A12, X1, X2, xx = b["A11"][:, None], b["A22"][None, :], b["A12"], b["X1"][:, None], b["X2"][None, :], b["xx"]
    c2u = 1 - A12 ** 2 / (A11 * A22)
    A11p, A22p, A12p = A11 - X1 * X1 / xx, A22 - X2 * X2 / xx, A12 - X1 * X2 / xx
    return [c2u, 1 - A12p ** 2 / (A11p * A22p)]


def signal(proto, N, seed):
    """one two-fascicle signal of synth.make_voxels' recipe on the protocol's directions: atoms among the first N"""
    rng = np.random.default_rng(seed)
    D = rotated(proto)
    atoms = rng.integers(0, N, 2)
    nu = rng.dirichlet(np.ones(2))
    y = 500.0 * (nu[0] * D[0][:, atoms[0]] + nu[1] * D[1][:, atoms[1]])
    return np.ascontiguousarray(y + rng.normal(0, SIGMA, y.shape))


def gram(proto, wgt, N, y, csf, dt=LD):
    """tests/_post_ref.py's gram() of the row: the block's leading N atoms and the row's own sums with y"""
    b = block(proto, wgt, dt)
    ys = (b["s"] * y).astype(dt)
    g = {"ysq": ys @ ys, "A11": b["A11"][:N, None], "A22": b["A22"][None, :N], "A12": b["A12"][:N, :N],
         "Y1": (b["D0"][:, :N].astype(dt).T @ ys)[:, None], "Y2": (b["D1"][:, :N].astype(dt).T @ ys)[None, :]}
    if csf:
        g.update(X1=b["X1"][:N, None], X2=b["X2"][None, :N], xx=b["xx"], xy=b["x"].astype(dt) @ ys)
    return g


def referee(row, dt=LD, y=None, N=None):
    """dict(F [N x N], c2bar, c2s, ysq, M, below) of a row (tests/_post_ref.py's pair_values with the cut)"""
    N = row["N"] if N is None else N
    y = signal(row["proto"], row["N"], row["seed"]) if y is None else y
    g = gram(row["proto"], row["wgt"], N, y, row["csf"], dt)
    F, c2bar, c2s, below = R.pair_values(g, row["csf"], CUT)
    return {"F": F, "c2bar": c2bar, "c2s": c2s, "ysq": float(g["ysq"]), "M": M_of(row["proto"]), "below": below}


# ---- the case table
def _row(kind, wgt, proto, csf, c, N, limit):
    ks, nw, tiles, nbuf = SWEEP_CFG[c]
    r = {"kind": kind, "wgt": bool(wgt), "proto": proto, "csf": bool(csf), "cfg": c, "N": int(N), "limit": bool(limit),
         "form": (ks, nw, tiles, nbuf, int(is_br(proto)), int(csf), int(kind == "land"), int(wgt))}
    r["id"] = "%s%s-%s%s-cfg%d-%d%s" % ("w" if wgt else "", kind, proto, "-csf" if csf else "", c, N, "-limit" if limit else "")
    return r


def rows():
    """one row per K = 2 form of each family, and a row at the limit for every NBUF = 1 form.  A form's own row sits 27
    atoms into its interval (a second tile, the last one padded), or at 293 atoms (19 tiles: a second sweep of the
    4-wave forms, a third of the 8-wave form, a padded last tile) where the interval starts at 16."""
    def make():
        out = []
        for kind in KINDS:
            for wgt in (False, True):
                for proto in PROTOS:
                    M, br = M_of(proto), is_br(proto)
                    for csf in (False, True):
                        for c in path(M, br, csf):
                            lo, hi = interval(kind, M, br, csf, wgt, c)
                            N = 293 if lo == 16 else lo + 16 - 5
                            assert N <= hi
                            out.append(_row(kind, wgt, proto, csf, c, N, False))
                            if SWEEP_CFG[c][3] == 1:
                                out.append(_row(kind, wgt, proto, csf, c, hi, True))
        for i, r in enumerate(out):
            r["seed"] = 9000 + i
        return out
    return _memo("rows", make)


def k1_rows():
    """the eight K = 1 kernels: (CSF, WGT) of the profile and the posterior, the whole pool on the short protocol"""
    def make():
        out = []
        for kind in ("post", "prof"):
            for wgt in (False, True):
                for csf in (False, True):
                    out.append({"kind": kind, "wgt": wgt, "proto": "short", "csf": csf, "N": POOL, "seed": 9900 + len(out),
                                "id": "%s%s-k1%s" % ("w" if wgt else "", kind, "-csf" if csf else "")})
        return out
    return _memo("k1rows", make)


def kernel_name(r):
    """the template instance a row names (for counting)"""
    if "form" not in r:
        return ("k1", r["kind"], r["csf"], r["wgt"])
    return ("k2", "prof" if r["kind"] == "land" else r["kind"]) + r["form"]
