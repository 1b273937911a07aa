"""Cases, referee arithmetic and error bar for the Monte-Carlo phase average (csrc/mc_average.hip,
mfx_monte_carlo_average[_dev], mf_utils.monte_carlo_average / get_PGSE_from_phases).  Shared by
tests/golden/gen_golden_mc_hp.py (50-digit means -> tests/golden/mc_hp_cases.npz), tests/test_mc_referee_host.py
and tests/test_mc_referee_gpu.py.  Plain NumPy; imports no GPU code.

The operation rounds its argument in float64 in a fixed order,

    arg_l = fl(Ds * fl(fl(fl(g0 p0) + fl(g1 p1)) + fl(g2 p2)))        (terms beyond dim absent)
    S     = (1/n) sum_l cos(arg_l)

`argument()` computes arg_l in exactly that order with one ufunc call per rounding, so nothing can fuse; the
generator then takes cos of that exact double, the sum and the mean at 50 digits.  An argument that was
contracted, reassociated or had Ds folded into g differs by about |arg| 2^-53 per term, which the rungs from
1e6 upwards resolve.

Every case gives each acquisition's phases another scale (scale * (1 + ref)), puts sequences on the last
acquisition and leaves at least one acquisition unused (the nchunks = 65 case has a single acquisition, its
table is 6 MB already), so a wrong tile_start or an acquisition off by one cannot pass.

The bar (see `bar`):   (C_COS + R) 2^-53 A + 2^-53 |S|,   A = (1/n) sum_l |cos(arg_l)|.
"""
import hashlib

import numpy as np

U = 2.0 ** -53

# the kernel's structure (csrc/mc_average.hip: MFX_MC_TS, MFX_MC_THREADS, MFX_MC_SP, MFX_MC_CHUNK, the wave size)
TS, THREADS, SP, WAVE = 8, 256, 16, 64
CHUNK = THREADS * SP
WAVES = THREADS // WAVE

# Error of the device's double-precision cos in units of 2^-53 |cos(x)| (a correctly rounded result scores at
# most 1; one ulp is between 1 and 2 of these units).  No statement of the bound ships with the ROCm
# installation this was written on, so it was measured once: one-spin calls with dim = 1, phase 1.0, Ds = 1.0
# return cos(g) of the device bit for bit (every other lane adds +0.0), for the 1 097 001 finite arguments
# of every case below but the two of 262 145 spins, against the 50-digit cosine.  Largest error seen: 1.1615 at
# x = 8.3788038980673427; per ladder rung 1.16, 1.13, 1.13, 1.15 and 1.11 (1e12), see DESIGN.md section 4.7.  C_COS = that maximum rounded up to the next integer,
# plus 1 for arguments not sampled.
C_COS_MEASURED_MAX = 1.1615
C_COS = 3

LADDER_SCALES = (1.0, 1e2, 1e4, 1e6, 1e12)
LADDER_DS = (1.0, float(np.sqrt(2.0 / 3.0)))
SPIN_SEAMS = (1, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 8193, 64 * CHUNK + 1)
TILE_COUNTS = (1, 7, 8, 9, 16, 17)
PGSE_EXTS = (("bfloat", ">f4"), ("lsingle", "<f4"), ("ldouble", "<f8"), ("bsingle", ">f4"))
LADDER_DM = np.array([2, 0, 2, 0, 0, 2, 2, 0, 2, 0, 2], dtype=np.int64)      # acquisition 1 unused


def roundings(n_spin):
    """R: the roundings on the longest path of the device's sum, read off csrc/mc_average.hip.
      SP - 1 = 15  mfx_mc_partial_kernel, `acc[t] += cos(...)` over MFX_MC_SP iterations (the first add is onto 0.0: exact)
      6            mfx_mc_wave_sum over the 64 lanes (offsets 32, 16, 8, 4, 2, 1), as lane 0 sees it
      WAVES - 1 = 3  `v += s_part[w][...]`, w = 1..3
      ceil(nchunks / 64) - 1   mfx_mc_finalize_kernel's strided loop `v += a.partial[...]` (again the first add is exact)
      6            mfx_mc_wave_sum in the finalize wave
      1            `v / (double)a.num_spins`
    Each rounding is at most 2^-53 of a partial sum, which is at most sum_l |cos(arg_l)| (first order in 2^-53)."""
    nchunks = -(-int(n_spin) // CHUNK)
    return (SP - 1) + 6 + (WAVES - 1) + (-(-nchunks // WAVE) - 1) + 6 + 1


def bar(n_spin, S, A, c_cos=None):
    """|S_device - S_50digit| <= (C_COS + R) 2^-53 A + 2^-53 |S|: the cosines' own error and the R roundings of the
    sum, both relative to the mean magnitude A of the terms, plus the rounding of the 50-digit mean to double."""
    c = C_COS if c_cos is None else c_cos
    return (c + roundings(n_spin)) * U * np.asarray(A) + U * np.abs(np.asarray(S))


# ----------------------------------------------------------------------------------------------
# the case table
# ----------------------------------------------------------------------------------------------
def _case(name, family, n_spin, n_ref, dm, scale, Ds=1.0, dim=3, **kw):
    c = dict(name=name, family=family, n_spin=int(n_spin), n_ref=int(n_ref), dm=np.asarray(dm, dtype=np.int64),
             scale=float(scale), Ds=float(Ds), dim=int(dim), zero_rows=(), phase_zeros=False, g_special=False, pgse=None)
    c.update(kw)
    return c


def interleaved_mapping():
    """The tile-seam counts as one unsorted delta_mapping: acquisitions 1..6 carry 1, 7, 8, 9, 16, 17 sequences,
    dealt round-robin from the fullest down (6 5 4 3 2 1 6 5 4 3 2 6 5 ...), so no two neighbours share an
    acquisition until only the fullest ones are left and order[] is far from the identity."""
    left = {r + 1: n for r, n in enumerate(TILE_COUNTS)}
    out = []
    while any(left.values()):
        for r in sorted(left, reverse=True):
            if left[r]:
                out.append(r)
                left[r] -= 1
    return np.array(out, dtype=np.int64)


def _pgse_spec(kind, ext, dtype):
    """A simulated scheme of 3 rows and a new scheme of 10 rows ([gx gy gz G Delta delta TE]), one acquisition unused
    and the last one used."""
    rng = np.random.default_rng([20261, len(kind), ord(ext[0]), ord(ext[1])])
    t = [(0.030, 0.010), (0.040, 0.012), (0.050, 0.015)]
    if kind == "dup":                       # rows 0 and 2 share (Delta, delta): the last one wins, row 0 goes unused
        t[2] = t[0]
    dirs = np.array([[0.6, 0.48, 0.64], [-0.5, 0.7, 0.51], [0.41, -0.62, 0.67]])
    dirs = dirs / np.sqrt(np.sum(dirs ** 2, axis=1))[:, None]
    sim = np.array([np.r_[dirs[i], (0.03, 0.045, 0.02)[i], t[i][0], t[i][1], t[i][0] + t[i][1] + 0.01] for i in range(3)])
    use = (2, 1) if kind == "dup" else (0, 2)
    new = []
    for i in range(10):
        d = rng.uniform(0.2, 1.0, 3) * rng.choice([-1.0, 1.0], 3)
        if kind == "dim2":
            d[2] = rng.uniform(0.1, 0.3)    # non-zero z components that dim = 2 has to ignore
        d = d / np.sqrt(np.sum(d ** 2))
        j = use[(i * 7 // 3) % 2]
        new.append(np.r_[d, rng.uniform(0.01, 0.06), sim[j, 4], sim[j, 5], sim[j, 6]])
    kw = dict(dim=2, D_sim=3.0e-9, D=2.0e-9) if kind == "dim2" else {}
    return dict(kind=kind, ext=ext, dtype=dtype, sch_sim=sim, sch_new=np.array(new), kwargs=kw)


def build_table():
    T = []
    for si, scale in enumerate(LADDER_SCALES):                       # argument ladder
        for di, Ds in enumerate(LADDER_DS):
            T.append(_case("ladder:%g:Ds%d" % (scale, di), "ladder", 4099, 3, LADDER_DM, scale, Ds=Ds))
    for n in SPIN_SEAMS:                                             # spin seams (+ an all-zero g among tile mates)
        big = n > 10000
        dm = [0, 0] if big else [1, 1, 1]
        T.append(_case("spin:%d" % n, "spin", n, 1 if big else 2, dm, 1e4))
        T.append(_case("zero-g:%d" % n, "zero-g", n, 1 if big else 2, [0, 0, 0] if big else [1, 1, 1], 1e4, zero_rows=(0, 2)))
    for c in TILE_COUNTS:                                            # tile seams, three layouts
        T.append(_case("tile:single:%d" % c, "tile", 257, 3, [2] * c, 1e4))
    T.append(_case("tile:together", "tile", 257, 7, np.repeat(np.arange(1, 7), TILE_COUNTS), 1e4))
    T.append(_case("tile:interleaved", "tile", 257, 7, interleaved_mapping(), 1e4))
    for dim in (1, 2, 3):                                            # dimensions
        T.append(_case("dim:%d" % dim, "dim", 4097, 3, LADDER_DM, 1e4, dim=dim))
    T.append(_case("special:Ds0", "special", 4099, 3, LADDER_DM, 1e4, Ds=0.0))
    T.append(_case("special:phase-zeros", "special", 4099, 3, LADDER_DM, 1e4, Ds=LADDER_DS[1], phase_zeros=True))
    T.append(_case("special:g-inf-nan", "special", 257, 2, [1] * TS, 1e4, g_special=True))
    for ext, dt in PGSE_EXTS:                                        # get_PGSE_from_phases end to end
        T.append(_case("pgse:ext:%s" % ext, "pgse", 4097, 3, [], 1e4, pgse=_pgse_spec("ext", ext, dt)))
    T.append(_case("pgse:dup", "pgse", 4097, 3, [], 1e4, pgse=_pgse_spec("dup", "ldouble", "<f8")))
    T.append(_case("pgse:dim2", "pgse", 4097, 3, [], 1e4, pgse=_pgse_spec("dim2", "bdouble", ">f8")))
    for i, c in enumerate(T):
        c["seed"] = [20260, i]
    assert len({c["name"] for c in T}) == len(T)
    return T


TABLE = build_table()
BY_NAME = {c["name"]: c for c in TABLE}


def raw_phases(c):
    """[n_ref * n_spin, 3 or dim] float64 from the case's seed, acquisition ref scaled by scale * (1 + ref).  PGSE cases
    draw three components (one file each) whatever their dim."""
    rng = np.random.default_rng(c["seed"])
    ncol = 3 if c["pgse"] else c["dim"]
    ph = rng.standard_normal((c["n_ref"] * c["n_spin"], ncol))
    ph *= np.repeat(c["scale"] * (1.0 + np.arange(c["n_ref"])), c["n_spin"])[:, None]
    if c["phase_zeros"]:
        k = rng.integers(0, 8, ph.shape)
        ph[k == 0] = 0.0
        ph[k == 1] = -0.0
    return ph


def pgse_contract(sch_sim, sch, dim):
    """(delta_mapping, gscaling) as get_PGSE_from_phases documents them: a new sequence uses the LAST simulated row with
    its (Delta, delta); its gradient scaling is the ratio, component by component, of the new gradient vector G g to
    the simulated one."""
    dm = np.array([max(j for j in range(sch_sim.shape[0]) if sch_sim[j, 4] == r[4] and sch_sim[j, 5] == r[5]) for r in sch],
                  dtype=np.int64)
    g_new = sch[:, :3] * sch[:, 3][:, None]
    g_sim = sch_sim[:, :3] * sch_sim[:, 3][:, None]
    return dm, np.ascontiguousarray(g_new[:, :dim] / g_sim[dm, :dim])


def inputs(c):
    """(phases [n_ref * n_spin, dim], delta_mapping, gscaling [n_seq, dim], Ds, n_spin): what the referee, the oracle and
    monte_carlo_average are given.  For a PGSE case: what the function's documented contract makes of the files."""
    ph = raw_phases(c)
    if c["pgse"]:
        p = c["pgse"]
        dim = p["kwargs"].get("dim", 3)
        ph = np.ascontiguousarray(ph.astype(p["dtype"]).astype(np.float64)[:, :dim])     # what the file can hold
        dm, gs = pgse_contract(p["sch_sim"], p["sch_new"], dim)
        Ds = float(np.sqrt(p["kwargs"]["D"] / p["kwargs"]["D_sim"])) if "D" in p["kwargs"] else 1.0
        return ph, dm, gs, Ds, c["n_spin"]
    rng = np.random.default_rng(c["seed"] + [1])
    gs = rng.uniform(-1.5, 1.5, (c["dm"].size, c["dim"]))
    for r in c["zero_rows"]:
        gs[r] = 0.0
    if c["g_special"]:                       # in the middle of a full tile of 8
        gs[3, 1] = np.inf
        gs[4, 0] = np.nan
    return ph, c["dm"], gs, c["Ds"], c["n_spin"]


def case_dim(c):
    return c["pgse"]["kwargs"].get("dim", 3) if c["pgse"] else c["dim"]


def checksum(c, inp=None):
    """SHA-256 of the bytes of everything `inputs` returns (and of a PGSE case's schemes)."""
    ph, dm, gs, Ds, n = inp if inp is not None else inputs(c)
    h = hashlib.sha256()
    for a in (ph, dm, gs, np.array([Ds]), np.array([n], dtype=np.int64)):
        h.update(np.ascontiguousarray(a).tobytes())
    if c["pgse"]:
        h.update(np.ascontiguousarray(c["pgse"]["sch_sim"]).tobytes())
        h.update(np.ascontiguousarray(c["pgse"]["sch_new"]).tobytes())
    return h.hexdigest()


# ----------------------------------------------------------------------------------------------
# the referee's argument, the variants the bar must reject, and the kernel's sum order
# ----------------------------------------------------------------------------------------------
def argument(ph, dm, gs, Ds, n_spin, variant=None, ref_shift=0):
    """arg [n_seq, n_spin] in float64.  variant None: the operation's definition, one ufunc call per rounding.
    'contracted': the inner product in np.longdouble, rounded once.  'folded': Ds multiplied into g first.
    ref_shift: use the phases of acquisition (ref + ref_shift) mod n_ref."""
    n = int(n_spin)
    dim = ph.shape[1]
    n_ref = ph.shape[0] // n
    out = np.empty((len(dm), n))
    with np.errstate(invalid="ignore", over="ignore"):
        for i, r in enumerate(dm):
            r = (int(r) + ref_shift) % n_ref
            blk = ph[r * n:(r + 1) * n]
            g = gs[i]
            if variant == "contracted":
                a = np.longdouble(g[0]) * blk[:, 0].astype(np.longdouble)
                for d in range(1, dim):
                    a = a + np.longdouble(g[d]) * blk[:, d].astype(np.longdouble)
                out[i] = np.multiply(Ds, a.astype(np.float64))
                continue
            if variant == "folded":
                g = np.multiply(Ds, g)
            a = np.multiply(g[0], blk[:, 0])
            for d in range(1, dim):
                a = np.add(a, np.multiply(g[d], blk[:, d]))
            out[i] = a if variant == "folded" else np.multiply(Ds, a)
    return out


def kernel_order_mean(terms, n_spin, n_sum=None):
    """mean over spins of terms [n_seq, n_spin], added in the device's order: spin = chunk * 4096 + it * 256 + thread,
    16 sequential adds per thread, the shuffle tree of a wave (v[l] += v[l + o], o = 32..1, read at lane 0), the four
    waves in turn, the chunks strided over 64 lanes, the tree again, one division.  Absent spins add nothing, which
    a +0.0 term restates exactly.  n_sum < n_spin leaves the last spins out (a break, for the teeth tests)."""
    n = int(n_spin)
    t = np.asarray(terms, dtype=np.float64)[:, :n if n_sum is None else n_sum]
    nseq = t.shape[0]
    nchunks = -(-n // CHUNK)
    pad = np.zeros((nseq, nchunks * CHUNK))
    pad[:, :t.shape[1]] = t
    x = pad.reshape(nseq, nchunks, SP, THREADS)
    acc = np.zeros((nseq, nchunks, THREADS))
    for it in range(SP):
        acc = acc + x[:, :, it, :]
    v = acc.reshape(nseq, nchunks, WAVES, WAVE)
    o = WAVE // 2
    while o:
        v = v[..., :o] + v[..., o:2 * o]
        o //= 2
    w = v[..., 0]
    part = w[:, :, 0]
    for k in range(1, WAVES):
        part = part + w[:, :, k]
    rounds = -(-nchunks // WAVE)
    lanes = np.zeros((nseq, rounds * WAVE))
    lanes[:, :nchunks] = part
    lanes = lanes.reshape(nseq, rounds, WAVE)
    v = np.zeros((nseq, WAVE))
    for k in range(rounds):
        v = v + lanes[:, k, :]
    o = WAVE // 2
    while o:
        v = v[:, :o] + v[:, o:2 * o]
        o //= 2
    return v[:, 0] / float(n)


def load_golden(path):
    """{name: (S [n_seq], A [n_seq], sha)} from tests/golden/mc_hp_cases.npz."""
    with np.load(path) as z:
        names, off, S, A, sha = [str(x) for x in z["names"]], z["offsets"], z["S"], z["A"], [str(x) for x in z["sha256"]]
    return {nm: (S[off[i]:off[i + 1]], A[off[i]:off[i + 1]], sha[i]) for i, nm in enumerate(names)}
