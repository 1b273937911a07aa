"""Host-side mirror of the reference's ``mf_utils`` names for the fingerprinting hot path.

Same names, argument meaning and error behaviour as
``microstructure_fingerprinting/mf_utils.py`` of the reference (cited below as ``ref``), but
every numeric evaluation runs in the HIP library ``libmfx.so`` (include/mfx.h):

=============================================  ================================================
reference function (ref line)                  what runs where here
=============================================  ================================================
solve_exhaustive_posweights (ref:115)          checks on host, search on device (mfx_solve_exhaustive)
ExhaustiveSolver / .._posweights_batch (new)   the same for many signals against one dictionary (mfx_solve_batch)
init_PGSE_multishell_interp (ref:1959)         per-shell knot tables built once on host (NumPy),
                                               uploaded lazily to HBM (mfx_tables_create)
interp_PGSE_from_multishell (ref:1693)         checks on host, evaluation on device (mfx_rotate)
rotate_atom (ref:1205)                         per-shell knot tables on host, evaluation on device
rotate_atom_2Dprotocol (ref:1440)              reference side on host (NumPy), per-direction plan and
                                               evaluation on device (mfx_rot2d_*)
rotate_scheme_mat, vrrotvec2mat, rotate_vector host (O(M) NumPy)
get_perp_vector, project_PGSE_scheme_xy_plane  host
import_PGSE_scheme (ref:2128)                  host (input normalisation, once per fit)
get_PGSE_scheme_from_bval_bvec_dense (2197)    host
gen_SoS_MRI (ref:2303)                         checks on host, Philox draws and magnitude on device (mfx_sos_noise)
monte_carlo_average (ref:2762)                 device (mfx_monte_carlo_average)
get_PGSE_from_phases (ref:2813)                file parsing / (Delta, delta) mapping on host, phase planes
                                               uploaded once, cosine reduction on device
DT_* / peaks_to_DT_vec (ref:865-1135)          host (orientation input normalisation)
loadmat (ref:3026)                             host (SciPy)
=============================================  ================================================

Nothing in this module falls back to a NumPy evaluation when the device library is missing.
"""
import ctypes as C
import hashlib

import numpy as np

from . import _lib as L
from . import engine

__all__ = ["get_gyromagnetic_ratio", "solve_exhaustive_posweights", "init_PGSE_multishell_interp",
           "interp_PGSE_from_multishell", "rotate_atom", "RotateAtomTables", "import_PGSE_scheme",
           "get_PGSE_scheme_from_bval_bvec_dense", "loadmat", "MultiShellInterpolator",
           "rotate_atom_2Dprotocol", "RotateAtom2DTables", "rotate_scheme_mat", "vrrotvec2mat", "rotate_vector",
           "get_perp_vector", "project_PGSE_scheme_xy_plane", "fit_2Dprotocol", "Fit2DResult", "gen_SoS_MRI", "profile_by_property", "profile_interval",
           "posterior_moments", "posterior_quantile", "posterior_by_property"]


def get_gyromagnetic_ratio(element='H'):
    """Gyromagnetic ratio [rad/s/T] (ref:1138-1150)."""
    table = {('hydrogen', 'H', 'proton'): 42.577480e6, ('carbon', 'C'): 10.7084e6, ('phosphorus', 'P'): 17.235e6}
    for names, mhz in table.items():
        if element in names:
            return 2 * np.pi * mhz
    raise ValueError('Gyromagnetic ratio for nucleus of element %s unknown.' % element)


# ---------------------------------------------------------------------------------------------
# knot tables
# ---------------------------------------------------------------------------------------------
class ShellKnots:
    """Knots of one shell's 1-D linear interpolant: ``x`` ascending (P,), ``y`` (P, N).
    Attribute names follow SciPy's interp1d objects, which the reference stores (ref:2074-2080)."""

    def __init__(self, x, y):
        self.x = np.ascontiguousarray(x, dtype=np.float64)
        self.y = np.ascontiguousarray(y, dtype=np.float64)


def _shell_knots(dots, rows, extra_knot=None):
    """Sorted de-duplicated knots of one shell + left-edge cluster merge.

    dots: |g.ordir| of the shell's samples; rows: their signals (n, N).
    np.unique keeps the first occurrence of exactly repeated abscissae (ref:2048-2053); knots closer
    than 1e-3 to the smallest one are replaced by their centre of mass (ref:2059-2072, 1398-1412).
    extra_knot: optional (x, row) appended when no knot equals x exactly (rotate_atom, ref:1384-1394).
    """
    xu, first = np.unique(dots, return_index=True)
    Y = rows[first, :]
    if extra_knot is not None and not np.any(xu == extra_knot[0]):
        xu = np.append(xu, [extra_knot[0]])
        Y = np.append(Y, np.reshape(extra_knot[1], (1, -1)), axis=0)
    near = np.abs(xu - xu[0]) < 1e-3
    c = int(np.sum(near))
    if c > 1:
        xu = np.append(np.mean(xu[near]), xu[c:])
        Y = np.append(np.mean(Y[near, :], axis=0, keepdims=True), Y[c:, :], axis=0)
    return ShellKnots(xu, Y)


def _check_gnorms(sch, tol=1e-3):
    gn = np.sqrt(np.sum(sch[:, 0:3] ** 2, axis=1))
    if np.any(np.abs(1 - gn[gn > 0]) > tol):
        raise ValueError("Gradient directions in multi-shell scheme matrix should all either have zero or "
                         "unit norm.")


class MultiShellInterpolator(dict):
    """Result of :func:`init_PGSE_multishell_interp`.

    Behaves like the reference's dict (keys ``scheme_DeldelTE``, ``num_subs``, ``Gms_un``,
    ``interpolators``; ref:2081-2085) and additionally owns the HBM copy of the tables."""

    def __init__(self, scheme_DeldelTE, Gms_un, shells, device=0):
        super().__init__()
        self['scheme_DeldelTE'] = np.array(scheme_DeldelTE, dtype=np.float64)
        self['num_subs'] = int(shells[0].y.shape[1])
        self['Gms_un'] = np.ascontiguousarray(Gms_un, dtype=np.float64)
        self['interpolators'] = list(shells)
        self.device = device
        self._tables = None
        self._plans = {}

    # convenience views used by bench/tests
    num_subs = property(lambda self: self['num_subs'])
    Gms_un = property(lambda self: self['Gms_un'])
    S = property(lambda self: len(self['interpolators']))
    off = property(lambda self: np.concatenate([[0], np.cumsum([s.x.size for s in self['interpolators']])])
                   .astype(np.int32))
    x_flat = property(lambda self: np.ascontiguousarray(np.concatenate([s.x for s in self['interpolators']])))
    Y_flat = property(lambda self: np.ascontiguousarray(np.concatenate([s.y for s in self['interpolators']], axis=0)))

    @classmethod
    def from_mapping(cls, m, device=0):
        """Accept the reference's own dict (SciPy interp1d objects expose ``.x`` / ``.y`` too)."""
        if isinstance(m, cls):
            return m
        if m['Gms_un'].size != len(m['interpolators']):
            raise ValueError("msinterp['Gms_un'] has size %d vs expected %d to match "
                             "len(msinterp['interpolators'])" % (m['Gms_un'].size, len(m['interpolators'])))
        shells = [ShellKnots(f.x, np.asarray(f.y).reshape(len(f.x), -1)) for f in m['interpolators']]
        if shells[0].y.shape[1] != m['num_subs']:
            raise ValueError("Inconsistency in msinterp regarding number of substrates. Make sure the "
                             "interpolator was initialized on the right dictionary.")
        return cls(m['scheme_DeldelTE'], m['Gms_un'], shells, device=device)

    def device_tables(self):
        if self._tables is None or self._tables.device != self.device:
            self._tables = engine.DeviceTables([s.x for s in self['interpolators']],
                                               [s.y for s in self['interpolators']], self['Gms_un'],
                                               device=self.device)
            self._plans = {}
        return self._tables

    def plan_for(self, sch_mat):
        """Device row plan of a protocol (cached per distinct scheme matrix)."""
        sch = L.f64c(sch_mat)
        key = (sch.shape, hashlib.sha1(sch.tobytes()).hexdigest(), self.device)
        p = self._plans.get(key)
        if p is None:
            if len(self._plans) > 8:
                self._plans.clear()
            p = engine.Plan(self.device_tables(), scheme=sch)
            self._plans[key] = p
        return p

    # --- flat (de)serialisation, used to broadcast the dictionary over RCCL
    def pack(self):
        hdr = {"sizes": [int(s.x.size) for s in self['interpolators']], "N": self['num_subs'],
               "S": len(self['interpolators'])}
        flat = np.concatenate([self['scheme_DeldelTE'], self['Gms_un'], self.x_flat, self.Y_flat.reshape(-1)])
        return hdr, np.ascontiguousarray(flat, dtype=np.float64)

    @classmethod
    def unpack(cls, hdr, flat, device=0):
        S, N, sizes = hdr["S"], hdr["N"], hdr["sizes"]
        P = int(sum(sizes))
        tim, flat = flat[:3], flat[3:]
        G, flat = flat[:S], flat[S:]
        x, Y = flat[:P], flat[P:P + P * N].reshape(P, N)
        shells, o = [], 0
        for n in sizes:
            shells.append(ShellKnots(x[o:o + n], Y[o:o + n]))
            o += n
        return cls(tim, G, shells, device=device)


def init_PGSE_multishell_interp(sig_ms, sch_mat_ms, ordir, device=0):
    """Per-shell interpolation tables of a dense multi-shell dictionary (ref:1959-2085).

    Returns a :class:`MultiShellInterpolator` (a dict with the reference's keys)."""
    ordir = np.asarray(ordir, dtype=np.float64)
    if ordir.size != 3:
        raise ValueError("Direction of dictionary computed with dense sampling (ordir) should have 3 entries.")
    ordir = np.squeeze(ordir) if ordir.ndim > 1 else ordir
    sch_mat_ms = np.asarray(sch_mat_ms, dtype=np.float64)
    if not np.all(np.isclose(sch_mat_ms[0, 4:7], sch_mat_ms[:, 4:7])):
        raise ValueError("Delta, delta and TE values should all be identical in multi-shell sampling.")
    sig_ms = np.asarray(sig_ms, dtype=np.float64)
    if sig_ms.ndim == 1:
        sig_ms = sig_ms.reshape((sig_ms.size, 1))
    nrm = np.sqrt((ordir ** 2).sum())
    if np.abs(1 - nrm) > 1e-3:
        raise ValueError("Orientation vector of the multi-shell signal must have unit norm. Detected %g." % nrm)
    _check_gnorms(sch_mat_ms)
    dots = np.abs(np.dot(sch_mat_ms[:, 0:3], ordir))
    G_un, which = np.unique(sch_mat_ms[:, 3], return_inverse=True)
    shells = []
    for s, G in enumerate(G_un):
        rows = np.where(which == s)[0]
        if G == 0:
            # b0 shell: constant interpolant through the first b0 row (ref:2019-2046)
            same = np.all(np.isclose(sig_ms[rows, :], sig_ms[rows[0], :]), axis=0)
            if np.any(~same):
                bad = np.where(~same)[0]
                raise ValueError('Distinct signal values in provided multi-shell sampling for zero gradients '
                                 '(b0 acquistions), for %d substrate(s) [%s]'
                                 % (bad.shape[0], " ".join("{:d}".format(b) for b in bad)))
            shells.append(ShellKnots([0.0, 1.0], np.repeat([sig_ms[rows[0], :]], 2, axis=0)))
        else:
            shells.append(_shell_knots(dots[rows], sig_ms[rows, :]))
    return MultiShellInterpolator(sch_mat_ms[0, 4:7], G_un, shells, device=device)


def interp_PGSE_from_multishell(sch_mat, newdir, sig_ms=None, sch_mat_ms=None, ordir=None, msinterp=None):
    """Single-fascicle PGSE signals rotated to ``newdir`` and resampled on ``sch_mat`` (ref:1693-1956).

    Returns ``np.squeeze`` of the (Nseq, Nsub) array, like the reference."""
    if msinterp is None:
        if sig_ms is None or sch_mat_ms is None or ordir is None:
            raise ValueError("If msinterp is not specified, sig_ms, sch_mat_ms and ordir must all be specified.")
        if np.asarray(sch_mat_ms).shape[0] != np.asarray(sig_ms).shape[0]:
            raise ValueError("Number of lines in dense multishell scheme (%d) does not match number of signal "
                             "values per substrate (%d)." % (np.asarray(sch_mat_ms).shape[0],
                                                             np.asarray(sig_ms).shape[0]))
        ms = init_PGSE_multishell_interp(sig_ms, sch_mat_ms, ordir)
    else:
        ms = MultiShellInterpolator.from_mapping(msinterp)
    sch_mat = np.asarray(sch_mat, dtype=np.float64)
    if not np.all(np.isclose(ms['scheme_DeldelTE'], sch_mat[:, 4:7])):          # ref:1786-1789
        raise ValueError("Delta, delta and TE values should all be identical to those in the multi-shell "
                         "sampling.")
    newdir = np.asarray(newdir, dtype=np.float64)
    if newdir.size != 3:
        raise ValueError("Direction of fascicle for new signal (newdir) should have 3 entries.")
    newdir = np.ascontiguousarray(newdir.reshape(3))
    nrm = np.sqrt((newdir ** 2).sum())
    if np.abs(1 - nrm) > 1e-3:                                                   # ref:1798-1802
        raise ValueError("Orientation vector of the new signal must have unit norm. Detected %g." % nrm)
    _check_gnorms(sch_mat)                                                       # ref:1804-1807
    plan = ms.plan_for(sch_mat)               # raises ValueError outside the table's G range (ref:1829-1836)
    out = np.zeros((sch_mat.shape[0], ms['num_subs']))
    L.check(L.lib().mfx_rotate(plan.handle(), L.dptr(newdir), 1, 0, L.dptr(out)))
    return np.squeeze(out)


class RotateAtomTables:
    """Direction-independent part of :func:`rotate_atom` (ref:1233-1412), hoisted out of the call:
    per-(G, Delta, delta) shell knots incl. the free-diffusion knot at |g.n| = 1, resident in HBM.
    ``rotate(newdirs)`` evaluates B directions in one device call."""

    def __init__(self, sig, sch_mat, ordir, DIFF, S0, warnings=True, device=0):
        assert isinstance(sig, np.ndarray), "Input sig should be a NumPy ndarray"
        assert isinstance(sch_mat, np.ndarray), "Input sch_mat should be a NumPy ndarray"
        assert isinstance(ordir, np.ndarray), "Input ordir should be a NumPy ndarray"
        assert isinstance(S0, np.ndarray), "Input S0 should be a NumPy ndarray"
        self.sig_shape = sig.shape
        Dv = np.asarray(DIFF, dtype=np.float64).reshape(-1)   # scalar, or one value per substrate
        Dv = Dv[0] if Dv.size == 1 else Dv
        sig = np.asarray(sig, dtype=np.float64)
        S0 = np.asarray(S0, dtype=np.float64)
        if sig.ndim == 1:
            sig = sig.reshape((sig.size, 1))
        if S0.ndim == 1:
            S0 = S0[:, np.newaxis]
        if sch_mat.shape[1] < 6:
            raise ValueError('sch_mat must be a N-by-6 or7 matrix')
        if sch_mat.shape[0] != sig.shape[0]:
            raise ValueError('sch_mat and sig must have the same number of rows')
        assert sig.shape == S0.shape, "The S0 matrix should have the same size as the signal matrix"
        sch = np.asarray(sch_mat, dtype=np.float64)
        M = sch.shape[0]
        gn = np.sqrt((sch[:, 0:3] ** 2).sum(axis=1, keepdims=True))
        gn[gn == 0] = np.inf
        ghat = np.ascontiguousarray(sch[:, 0:3] / gn)                 # b0 rows -> zero vector -> |g.n| = 0
        odir = np.asarray(ordir, dtype=np.float64).reshape(3)
        dots = np.abs(np.dot(ghat, odir / np.sqrt((odir ** 2).sum())))
        gam = get_gyromagnetic_ratio('H')
        bvals = (gam * sch[:, 3] * sch[:, 5]) ** 2 * (sch[:, 4] - sch[:, 5] / 3)
        trip, which = np.unique(sch[:, 3:6], return_inverse=True, axis=0)
        which = np.asarray(which).reshape(-1)
        shells, shell_of_row = [], np.zeros(M, dtype=np.int32)
        for s in range(trip.shape[0]):
            rows = np.where(which == s)[0]
            b = bvals[rows[0]]
            if b == 0:
                # no rotation for b0 rows (ref:1298-1300): one constant 2-knot shell per row
                for m in rows:
                    shell_of_row[m] = len(shells)
                    shells.append(ShellKnots([0.0, 1.0], np.repeat(sig[m:m + 1, :], 2, axis=0)))
                continue
            if rows.size < 2:
                raise ValueError("Fewer than 2 identical (G, Del, del) triplets detected for triplet %d/%d "
                                 "(%g, %g, %g), b=%g s/mm^2, probably not a HARDI shell."
                                 % (s + 1, trip.shape[0], trip[s, 0], trip[s, 1], trip[s, 2], b / 1e6))
            if rows.size < 10 and warnings:
                print("WARNING: rotate_atom: fewer than 10 data points detected for acquisition parameters "
                      "(G, Del, del) %d/%d (%g, %g, %g), b=%g s/mm^2.\nQuality of approximation may be poor."
                      % (s + 1, trip.shape[0], trip[s, 0], trip[s, 1], trip[s, 2], b / 1e6))
            ok = np.all(np.isclose(S0[rows, :], S0[rows[0], :]), axis=0)
            if np.any(~ok):
                bad = np.where(~ok)[0]
                raise ValueError('Distinct values in provided S0 image for shell  %d/%d (b=%g s/mm^2) for %d '
                                 'substrate(s) [%s]' % (s + 1, trip.shape[0], b / 1e6, bad.shape[0],
                                                        " ".join("{:d}".format(x) for x in bad)))
            free = np.exp(-b * Dv) * S0[rows[0], :]
            shell_of_row[rows] = len(shells)
            shells.append(_shell_knots(dots[rows], sig[rows, :], extra_knot=(1.0, free)))
        self.N = sig.shape[1]
        self.M = M
        self.tables = engine.DeviceTables([k.x for k in shells], [k.y for k in shells],
                                          np.arange(len(shells), dtype=np.float64), device=device)
        self.plan = engine.Plan(self.tables, gdirs=ghat, shell_of_row=shell_of_row)

    def rotate(self, newdirs):
        d = L.f64c(np.asarray(newdirs, dtype=np.float64).reshape(-1, 3))
        out = np.zeros((d.shape[0], self.M, self.N))
        L.check(L.lib().mfx_rotate(self.plan.handle(), L.dptr(d), d.shape[0], 1, L.dptr(out)))
        return out


def rotate_atom(sig, sch_mat, ordir, newdir, DIFF, S0, warnings=True):
    """Rotate HARDI signals of single fascicles from ``ordir`` to ``newdir`` (ref:1205-1437)."""
    assert isinstance(newdir, np.ndarray), "Input newdir should be a NumPy ndarray"
    T = RotateAtomTables(sig, sch_mat, ordir, DIFF, S0, warnings=warnings)
    out = T.rotate(np.asarray(newdir, dtype=np.float64).reshape(1, 3))[0]
    if np.any(np.isnan(out)):                                                    # ref:1428-1436
        bad = np.where(np.any(np.isnan(out), axis=0))[0]
        raise ValueError('Nan detected after rotation of substrate(s) for %d substrate(s): [%s]'
                         % (bad.shape[0], " ".join("%d" % b for b in bad)))
    return np.reshape(out, T.sig_shape)


# ---------------------------------------------------------------------------------------------
# rotations and 2-D (AxCaliber-like) protocols
# ---------------------------------------------------------------------------------------------
def get_perp_vector(v):
    """Unit vector(s) with a zero dot product with ``v`` along the first axis (ref:769-811).

    Where ``v`` has zero entries the result has ones there; otherwise its first entries are 1 and the
    last one cancels the dot product.  Normalised along the first axis."""
    u = np.zeros(v.shape)
    zero = np.abs(v) < (10 * 2.2204e-16)
    full = np.sum(zero, axis=0) == 0
    u[zero] = 1
    u[:-1, full] = 1
    u[-1, full] = -np.sum(v[:-1, full], axis=0) / v[-1, full]
    return u / np.sqrt(np.sum(u ** 2, axis=0))


def rotate_vector(v, rot_axis, theta):
    """Rotation of the 3-vector ``v`` by ``theta`` radians about the unit axis ``rot_axis`` (ref:814-839)."""
    nsq = np.sum(rot_axis ** 2)
    if ~np.isclose(1, nsq):
        raise ValueError("rotation axis should have unit norm, detected %g" % np.sqrt(nsq))
    c = np.cos(theta)
    return c * v + np.sin(theta) * np.cross(rot_axis, v) + (1 - c) * (np.dot(rot_axis, v) * rot_axis)


def vrrotvec2mat(rotax, theta):
    """3x3 rotation matrix of angle ``theta`` about the unit axis ``rotax`` (ref:842-862)."""
    if rotax.size != 3:
        raise ValueError("rotation axis should be a 3-element NumPy array")
    if ~np.isclose(np.sum(rotax ** 2), 1):
        raise ValueError("rotation axis should have unit norm")
    s, c = np.sin(theta), np.cos(theta)
    t = 1 - c
    x, y, z = rotax[0], rotax[1], rotax[2]
    return np.array([[t * x * x + c, t * x * y - s * z, t * x * z + s * y],
                     [t * x * y + s * z, t * y * y + c, t * y * z - s * x],
                     [t * x * z - s * y, t * y * z + s * x, t * z * z + c]])


def rotate_scheme_mat(sch_mat, cyldir1, cyldir2):
    """Scheme matrix seen by a fascicle along ``cyldir1`` when the fascicle is along ``cyldir2`` (ref:1153-1202).

    Gradients are rotated by ``vrrotvec2mat(cyldir1 x cyldir2, -arccos(cyldir1 . cyldir2))``, entries with
    magnitude <= eps are set to 0 and non-zero rows renormalised.  When the two directions are parallel the
    input object itself is returned, as the reference does."""
    if cyldir1.size != 3 or cyldir2.size != 3:
        raise ValueError("cyldir1 and cyldir2 should be 3-elements NumPy arrays.")
    if ~np.isclose(np.sum(cyldir1 ** 2), 1) or ~np.isclose(np.sum(cyldir2 ** 2), 1):
        raise ValueError("cyldir1 and cyldir2 should have unit norm.")
    ax = np.cross(cyldir1, cyldir2)
    axsq = np.sum(ax ** 2)
    if not axsq > 0:
        return sch_mat
    R = vrrotvec2mat(ax / np.sqrt(axsq), -np.arccos(np.dot(cyldir1, cyldir2)))
    g = sch_mat[:, :3] @ R.T
    g[np.abs(g) <= np.finfo(float).eps] = 0
    gn = np.sqrt(np.sum(g ** 2, axis=1, keepdims=True))
    nz = np.squeeze(gn > 0)
    g[nz, :] = g[nz, :] / gn[nz, :]
    if sch_mat.shape[1] > 3:
        return np.hstack((g, sch_mat[:, 3:]))
    return g


def project_PGSE_scheme_xy_plane(sch_mat):
    """Scheme with the gradients' z component removed (ref:2088-2125).

    ``sch_mat``: array, or path of a text file with a one-line header.  The result has gz = 0, unit
    [gx, gy] and G' with (gz G)^2 + G'^2 = G^2; zero gradients stay zero, the other columns are kept."""
    if isinstance(sch_mat, str):
        sch_mat = np.loadtxt(sch_mat, skiprows=1)
    if sch_mat.ndim == 1:
        sch_mat = sch_mat[np.newaxis, :]
    gxy = np.sqrt(sch_mat[:, 0] ** 2 + sch_mat[:, 1] ** 2)
    out = np.zeros(sch_mat.shape)
    out[:, 3] = sch_mat[:, 3] * gxy
    gxy[gxy == 0] = 1
    out[:, :2] = sch_mat[:, :2] / gxy[:, np.newaxis]
    out[sch_mat[:, 3] == 0, :4] = 0
    out[:, 4:] = sch_mat[:, 4:]
    Gz = np.abs(sch_mat[:, 2]) * sch_mat[:, 3]
    G_chk_sq = out[:, 3] ** 2 + Gz ** 2
    assert np.all(np.abs(np.sqrt(G_chk_sq) - sch_mat[:, 3]) <= 1e-4 * sch_mat[:, 3]), \
        "Inconsistency with gradient intensities during projection in xy plane"
    return out


# status codes of include/mfx_rot2d.h
ROT2D_OK, ROT2D_NEWDIR_NORM, ROT2D_CHK_NEW, ROT2D_CHK_PAR_NEW, ROT2D_REF_UNIQUE, ROT2D_REF_PAIRS, ROT2D_NEW_UNIQUE, \
    ROT2D_NEW_PAIRS, ROT2D_VANISHED, ROT2D_INTERP_B0, ROT2D_NO_REF_LINE = range(11)


def _perp_components(sm_eff, G):
    """g_perp (normalised first two columns, a view of ``sm_eff``, normalised in place like the reference),
    |g_perp| before normalisation, G_perp and G_par (ref:1509-1516, 1532-1539)."""
    g_perp = sm_eff[:, 0:2]
    n = np.sqrt(np.sum(g_perp ** 2, axis=1))
    nz = n > 0
    g_perp[nz, :] = sm_eff[nz, 0:2] / n[nz][:, np.newaxis]
    return g_perp, n, G * n, np.abs(sm_eff[:, 2]) * G


class RotateAtom2DTables:
    """Direction-independent part of :func:`rotate_atom_2Dprotocol` (ref:1440-1690), built once on the host
    with the reference's NumPy arithmetic and kept in HBM: the reference fascicle's S_par / S_perp, per
    (Delta, delta) pair its unique perpendicular directions and opposite pairs, the b0 values that rows
    without a perpendicular component take, and one sorted knot table per reference line.

    ``rotate(newdirs)`` -> [B, M, N] and ``rotate_cols(newdirs, cols)`` -> [B, M] evaluate B directions
    in one device call; ``engine.rotate2d_dev`` is the device-resident variant.  ``sch_mat`` is not
    modified (the reference normalises its first two columns in place when ``refdir`` is along z; the
    new fascicle's side sees those normalised columns here too)."""

    def __init__(self, sig, sch_mat, refdir, DIFF, device=0):
        sig = np.asarray(sig, dtype=np.float64)
        self.sig_shape = sig.shape
        if sig.ndim == 1:
            sig = sig[:, np.newaxis]
        sch = np.array(sch_mat, dtype=np.float64)          # private copy (see the class docstring)
        if np.any(sch[:, 2] != 0):
            raise ValueError("Use the original schemefile with zeros for gz.\n"
                             "Specify the reference and new orientations separately.")
        if self.sig_shape[0] != sch.shape[0]:
            raise ValueError("Signal and scheme matrix must have the same number of elements (sequences) along "
                             "their first dimension. Detected %d and %d." % (self.sig_shape[0], sch.shape[0]))
        gam = get_gyromagnetic_ratio('H')
        G, Delta, delta = sch[:, 3], sch[:, 4], sch[:, 5]
        is_b0 = G == 0
        sm_ref = rotate_scheme_mat(sch, np.array([0, 0, 1]), np.asarray(refdir))
        g_perp_ref, _, G_perp_ref, G_par_ref = _perp_components(sm_ref, G)
        chk_ref = np.isclose(G ** 2, G_perp_ref ** 2 + G_par_ref ** 2)
        assert np.all(chk_ref), "Inconsistency in parallel and perpendicular gradient components for reference fasicle."
        b_par_ref = (gam * delta * G_par_ref) ** 2 * (Delta - delta / 3)
        S_par_ref = np.exp(-b_par_ref * DIFF)
        S_perp_ref = sig / S_par_ref[:, np.newaxis]
        chk_par_ref = np.isclose(S_par_ref[is_b0], 1)
        assert np.all(chk_par_ref), "Reference fascicle: parallel signal should  be one in b0 sequences."
        self.sm_eff_ref, self.S_par_ref, self.S_perp_ref = sm_ref, S_par_ref, S_perp_ref

        M, N = sig.shape
        _, i_un = np.unique(sch[:, 4:6], return_inverse=True, axis=0)
        i_un = np.asarray(i_un).reshape(-1)
        P = int(i_un.max()) + 1
        # constant rows: every b0 row's signal, then the mean b0 signal of pairs with several b0 rows
        cst = [sig[m] for m in np.where(is_b0)[0]]
        row_const = np.full(M, -1, dtype=np.int32)
        row_const[is_b0] = np.arange(len(cst), dtype=np.int32)
        pair_off, pair_rows = [0], []
        ref_info = np.zeros((P, 3), dtype=np.int32)
        ref_dirs = np.zeros((P, 5, 2))
        ref_tab = np.full((P, 5), -1, dtype=np.int32)
        van_const = np.full(P, -1, dtype=np.int32)
        tab_off, kx, ky = [0], [], []
        for p in range(P):
            ind = np.where(i_un == p)[0]
            pair_rows.append(ind)
            pair_off.append(pair_off[-1] + ind.size)
            b0 = np.where(is_b0 & (i_un == p))[0]
            if b0.size == 1:
                van_const[p] = row_const[b0[0]]
            elif b0.size > 1:
                van_const[p] = len(cst)
                cst.append(np.mean(sig[b0, :], axis=0))
            # reference side (ref:1571-1601); a failure is recorded, the device reports it in the reference's order
            un, inv = np.unique(g_perp_ref[ind, :], return_inverse=True, axis=0)
            inv = np.asarray(inv).reshape(-1)
            if un.shape[0] not in (3, 5):
                ref_info[p] = (ROT2D_REF_UNIQUE, un.shape[0], 0)
                continue
            ig, ig_op = np.where(np.isclose(un @ un.T, -1))
            if ig.size not in (2, 4):
                ref_info[p] = (ROT2D_REF_PAIRS, ig.size, 0)
                continue
            ref_info[p] = (ROT2D_OK, 0, un.shape[0])
            ref_dirs[p, :un.shape[0]] = un
            for u in range(un.shape[0]):
                k = np.where(ig == u)[0]
                if k.size != 1:
                    ref_tab[p, u] = -1 - k.size          # the reference's comparison would not broadcast
                    continue
                rows = ind[(inv == ig[k[0]]) | (inv == ig_op[k[0]])]
                x = G_perp_ref[rows] * np.sign(g_perp_ref[rows, :] @ un[u])
                order = np.argsort(x, kind="mergesort")     # interp1d(assume_sorted=False)
                ref_tab[p, u] = len(tab_off) - 1
                kx.append(x[order])
                ky.append(S_perp_ref[rows, :][order])
                tab_off.append(tab_off[-1] + rows.size)
        self.M, self.N, self.P, self.device = M, N, P, device
        self._arrays = dict(
            sch=np.ascontiguousarray(sch[:, :6]), pair_off=np.array(pair_off, dtype=np.int32),
            pair_rows=np.ascontiguousarray(np.concatenate(pair_rows), dtype=np.int32), ref_info=ref_info,
            ref_dirs=ref_dirs, ref_tab=ref_tab, row_const=row_const, van_const=van_const,
            cst=np.ascontiguousarray(np.array(cst).reshape(-1, N)) if cst else np.zeros((1, N)),
            tab_off=np.array(tab_off, dtype=np.int32),
            kx=np.ascontiguousarray(np.concatenate(kx)) if kx else np.zeros(1),
            ky=np.ascontiguousarray(np.concatenate(ky, axis=0)) if ky else np.zeros((1, N)))
        self.num_const = len(cst)
        self.num_tables = len(tab_off) - 1
        self.gamma, self.DIFF = gam, float(DIFF)
        self._h = None

    def handle(self):
        if self._h is None:
            a = self._arrays
            h = C.c_void_p()
            L.check(L.lib().mfx_rot2d_create(
                L.dptr(a["sch"]), self.M, L.iptr(a["pair_off"]), L.iptr(a["pair_rows"]), self.P, L.iptr(a["ref_info"]),
                L.dptr(a["ref_dirs"]), L.iptr(a["ref_tab"]), L.iptr(a["row_const"]), L.iptr(a["van_const"]),
                L.dptr(a["cst"]), self.num_const, L.iptr(a["tab_off"]), L.dptr(a["kx"]), L.dptr(a["ky"]),
                self.num_tables, self.N, self.gamma, self.DIFF, self.device, C.byref(h)))
            self._h = h
        return self._h

    def close(self):
        if self._h is not None:
            L.lib().mfx_rot2d_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def error_for(self, rec):
        """The exception the reference raises for a status record {code, pair, value, value2}."""
        code, p, v, v2 = (int(r) for r in rec)
        P = self.P
        if code == ROT2D_NEWDIR_NORM:
            return ValueError("cyldir1 and cyldir2 should have unit norm.")
        if code == ROT2D_CHK_NEW:
            return AssertionError("Inconsistency in parallel and perpendicular gradient components for new fascicle.")
        if code == ROT2D_CHK_PAR_NEW:
            return AssertionError("New fascicle: parallel signal should  be equal to 1 in b0 sequences.")
        if code in (ROT2D_REF_UNIQUE, ROT2D_NEW_UNIQUE):
            return AssertionError("Problem at delta pair %d/%d: found %d unique gradient directions in plane "
                                  "perpendicular to %s fascicle (including b0 zero dirs)."
                                  % (p + 1, P, v, "reference" if code == ROT2D_REF_UNIQUE else "new"))
        if code == ROT2D_REF_PAIRS:
            return AssertionError("Problem at delta pair %d/%d: found %d instead of 4 (2x2, redundant) pairs of "
                                  "opposite directions in plane perpendicular to reference fascicle." % (p + 1, P, v))
        if code == ROT2D_NEW_PAIRS:
            return AssertionError("Problem at delta pair %d/%d: found %d instead of 2 pairs of opposite directions, "
                                  "in plane  perpendicular to new fascicle." % (p + 1, P, v))
        if code == ROT2D_VANISHED:
            return AssertionError("Shell %d/%d: some new line directions are completely parallel to new fascicle, "
                                  "implying free diffusion. However, no b0 measurements in the reference signal are "
                                  "available for this shell. We therefore can't properly scale the new signal."
                                  % (p + 1, P))
        if code == ROT2D_INTERP_B0:
            return AssertionError("Problem at delta pair %d/%d, new line direction %d/%d: trying to interpolate b0 "
                                  "sequences." % (p + 1, P, v, v2))
        if code == ROT2D_NO_REF_LINE:
            return ValueError("operands could not be broadcast together with shapes (%d,) (%d,) " % (v, v2))
        return L.MfxError("mfx_rot2d: unknown status %d" % code)

    def raise_for_status(self, status):
        """Raise the reference's exception for the lowest-index failing direction of a [B, 4] status array."""
        status = np.asarray(status).reshape(-1, 4)
        bad = np.nonzero(status[:, 0])[0]
        if bad.size:
            raise self.error_for(status[bad[0]])

    def rotate(self, newdirs):
        """Signals for fascicles along each of ``newdirs`` [B, 3] (not normalised) -> [B, M, N]."""
        d = L.f64c(np.asarray(newdirs, dtype=np.float64).reshape(-1, 3))
        out = np.zeros((d.shape[0], self.M, self.N))
        status = np.zeros((d.shape[0], 4), dtype=np.int32)
        if d.shape[0]:
            L.check(L.lib().mfx_rot2d_rotate(self.handle(), L.dptr(d), d.shape[0], L.dptr(out), L.iptr(status)))
        self.raise_for_status(status)
        return out

    def fit(self, data, peaks, numfasc, csf_mask=None, sig_csf=None, on_error='raise', *, weights=None, robust=None):
        """Fit ``data`` [V, M]: voxel v has ``numfasc[v]`` fascicles along ``peaks[v, 3k:3k+3]`` (unit vectors,
        peaks [V, 3 maxfasc]) and, where ``csf_mask[v]``, a CSF column ``sig_csf`` [M].  Per voxel the dictionaries
        ``rotate(peaks[v, 3k:3k+3])`` side by side go through ``solve_exhaustive_posweights`` on the device; returns
        a :class:`Fit2DResult`.  ``on_error='raise'`` raises the reference's exception for the lowest voxel with a
        failing direction (what a loop over the voxels would have raised first); ``'nan'`` returns NaN rows there
        and the status records.  ``weights``: measurement weights [V, M] or [M], boolean or numeric, >= 0 (a 0/1 outlier
        mask, inverse noise variances): the fit minimises sum_m W[v, m] (y_m - model_m)^2 (``engine.fit2d_weighted``,
        include/mfx_w2d.h), MSE = min_obj / sum_m W and R2 the squared weighted correlation; the result keeps them in
        ``weights``.  Negative or non-finite weights, or a voxel without a positive weight, raise ValueError before any
        device call; ``on_error`` is about directions only.  ``robust``: None / False (the fit above), True or a dict with
        keys among 'loss' ('cutoff' | 'huber' | 'tukey'), 'c' (>= 1, in units of the median absolute residual) and 'n_iter'
        (True = {'loss': 'cutoff', 'c': 4.45, 'n_iter': 3}): the fit, then n_iter times predict -> weights from the
        residuals -> weighted fit, on the device (``engine.fit2d_robust``, include/mfx_robust2d.h); ``weights`` are then the
        base weights.  The result keeps the final weights in ``weights`` - ``posterior(fit=r)``, ``profile``, ``interval``
        and ``posterior_moments`` on them answer for the final weighted objective - and has ``robust_info``,
        ``robust_scale``, ``n_rejected`` and ``outlier_mask()``."""
        return _fit2d(self, data, peaks, numfasc, csf_mask, sig_csf, on_error, weights, robust)

    def bootstrap(self, data, peaks, numfasc, fit=None, csf_mask=None, sig_csf=None, on_error='raise', *, B=200, kind='wild',
                  seed=0, inflate=True, q=(0.025, 0.975), props=None, voxels=None, keep=False, groups=None, weights=None,
                  fixed_weights=False):
        """Model-free uncertainty of every estimated parameter (``engine.fit2d_bootstrap``, include/mfx_boot2d.h; the rule is
        that of include/mfx_boot.h): the residuals of each voxel's own fit - ``fit``, a :class:`Fit2DResult` of these
        voxels, or a fit made here - are resampled into ``B`` replicate signals, every replicate is fitted as ``fit`` fits
        it, bit for bit, and the B parameter rows of a voxel are reduced to statistics, all on the device.  ``data``,
        ``peaks``, ``numfasc``, ``csf_mask``, ``sig_csf`` as for ``fit``; every voxel class is served.  The replicates of a
        voxel share its directions: for one and two fascicles without a CSF column the rotated dictionaries' column norms
        and cross-Gram are formed once per voxel, not once per replicate.  ``kind`` 'wild' flips the sign of every
        residual at random; 'residual' draws, for every measurement, a residual of its group - ``groups`` [M] integers,
        default ``engine.boot_groups(sch_mat)``: rows sharing (G, Delta, delta); a group of one row redraws its own
        residual, so that row is its prediction plus its (inflated) residual in every replicate.  ``inflate`` scales the
        residuals by sqrt(M / (M - number of active compartments)).  ``q``: the quantiles kept.  ``props``: a dict
        mapping a name to an [N] array of atom properties, whose values at the chosen atoms are bootstrapped too.
        ``voxels``: positions in this batch (default: all); the random stream is keyed by the batch position, so a subset
        gives the replicates the whole batch gives.  ``keep``: also return the replicate parameter rows.  A voxel with a
        failing direction: ``on_error='raise'`` raises the reference's exception for the lowest of them, ``'nan'`` keeps
        its record in ``dir_status``, status 2 and NaN statistics.  A ``fit`` made with ``weights=`` or ``robust=`` is
        served only with ``fixed_weights=True`` (without it: NotImplementedError): the bootstrap then holds the fit's final
        measurement weights (``fit.weights``; without a ``fit``, ``weights=`` as for ``fit``, and the own weighted fit is
        made here) fixed - every replicate is fitted by the weighted fit on those weights and the fit's own parameters are
        the ones resampled around (``engine.fit2d_weighted_bootstrap``; include/mfx_wboot2d.h, the rule is that of
        include/mfx_wboot.h).  No replicate re-runs the rejection, so after a robust fit the result is CONDITIONAL ON THE
        ROWS THAT WERE REJECTED: it says how stable the estimate is given that choice of outliers, not how stable the
        choice is.  Rows of weight 0 are left as measured, 'residual' draws among the rows of positive weight in units of
        sqrt(weight), and ``inflate`` counts the rows of positive weight.  ``fit`` and ``weights=`` both given and
        different, ``fixed_weights=True`` without either, and ``weights=`` without ``fixed_weights=True`` are ValueErrors.
        Returns a :class:`Bootstrap2DResult`."""
        return _boot2d(self, data, peaks, numfasc, fit, csf_mask, sig_csf, on_error, B, kind, seed, inflate, q, props, voxels,
                       keep, groups, weights=weights, fixed_weights=fixed_weights)

    def _predict_args(self, fit_or_params, peaks, sig_csf):
        """Argument checks of predict / residuals / simulate (before any device call): (params, peaks, maxfasc, csf_on, sig_csf)."""
        params = fit_or_params.params if isinstance(fit_or_params, Fit2DResult) else fit_or_params
        params = np.asarray(params, dtype=np.float64)
        if params.ndim != 2:
            raise ValueError("params should be a 2-D array [voxels x parameters], got shape %s" % (params.shape,))
        V = params.shape[0]
        peaks = np.asarray(peaks, dtype=np.float64)
        if peaks.ndim != 2 or peaks.shape[0] != V or peaks.shape[1] % 3 != 0:
            raise ValueError("peaks should have shape (%d, 3 maxfasc)" % V)
        maxfasc = peaks.shape[1] // 3
        if maxfasc > 3:
            raise NotImplementedError("the 2-D protocol prediction serves at most 3 fascicles per voxel (peaks holds %d)" % maxfasc)
        extra = params.shape[1] - 3 - 2 * maxfasc
        if extra not in (0, 1):
            raise ValueError("params should have 1 + 2 maxfasc + csf + 2 columns for the %d fascicle(s) of peaks, got shape %s"
                             % (maxfasc, params.shape))
        csf_on = bool(extra)
        if csf_on:
            if sig_csf is None:
                raise ValueError("params hold a CSF fraction: sig_csf is needed")
            sig_csf = np.asarray(sig_csf, dtype=np.float64).reshape(-1)
            if sig_csf.size != self.M:
                raise ValueError("sig_csf has %d entries, protocol has %d" % (sig_csf.size, self.M))
        return params, peaks, maxfasc, csf_on, (sig_csf if csf_on else None)

    def _predict(self, fit_or_params, peaks, sig_csf, on_error, data=None, **noise):
        if on_error not in ("raise", "nan"):
            raise ValueError("on_error should be 'raise' or 'nan'")
        params, peaks, maxfasc, csf_on, sig_csf = self._predict_args(fit_or_params, peaks, sig_csf)
        if data is not None:
            data = np.asarray(data, dtype=np.float64)
            if data.shape != (params.shape[0], self.M):
                raise ValueError("data has shape %s, protocol has %d measurements for %d voxels" % (data.shape, self.M, params.shape[0]))
        unserved = np.isnan(params[:, 0])           # the NaN rows of voxels a fit could not serve
        if unserved.any():
            params = np.where(unserved[:, None], 0.0, params)
        out, dstat = engine.predict2d(self, params, peaks, maxfasc, csf_on, sig_csf, **noise)
        if on_error == "raise":
            bad = np.flatnonzero(dstat[:, 0])
            if bad.size:
                raise self.error_for(dstat[bad[0], :4])
        out[unserved] = np.nan
        return out if data is None else data - out

    def predict(self, fit_or_params, peaks, sig_csf=None, on_error='raise'):
        """The signal [V, M] that parameter rows stand for (``engine.predict2d``, include/mfx_predict2d.h): per present
        fascicle the column ``rotate_cols`` returns, times M0 nu, summed in the order f0, f1, f2, csf - the ``y_rec`` the
        reference's solver computes.  ``fit_or_params``: a :class:`Fit2DResult` or rows in its layout [V, 1 + 2 maxfasc +
        csf + 2] (the column count says whether there is a CSF fraction, which needs ``sig_csf`` [M]); ``peaks``
        [V, 3 maxfasc] as for ``fit``.  A voxel the fit could not serve (a NaN row) is NaN.  A present fascicle (M0 nu > 0)
        with a failing direction: ``on_error='raise'`` raises the reference's exception for the lowest such voxel,
        ``'nan'`` returns NaN rows.  Atom indices outside the dictionary and negative or non-finite weights raise
        ValueError before anything is launched."""
        return self._predict(fit_or_params, peaks, sig_csf, on_error)

    def residuals(self, data, fit_or_params, peaks, sig_csf=None):
        """``data - predict(fit_or_params, peaks, sig_csf)`` [V, M]."""
        return self._predict(fit_or_params, peaks, sig_csf, 'raise', data=data)

    def simulate(self, params, peaks, sig_csf=None, *, SNR=None, sigma_g=None, N=1, seed=None, offset=0):
        """``predict`` with the sum-of-squares magnitude noise of ``N`` coils (Rician for N = 1) applied in the same pass:
        give either ``sigma_g`` (a scalar, one value per voxel or one per element) or ``SNR``, which sets ``sigma_g = M0 /
        SNR`` in every voxel.  ``seed=None`` draws a seed from NumPy's global generator; an int makes the call reproducible
        by itself.  Element (v, m) draws with index ``offset + v M + m``."""
        if (SNR is None) == (sigma_g is None):
            raise ValueError("simulate needs exactly one of SNR and sigma_g")
        if isinstance(N, bool) or int(N) != N or N < 1:
            raise ValueError("N should be a positive integer, got %r" % (N,))
        prm = params.params if isinstance(params, Fit2DResult) else np.asarray(params, dtype=np.float64)
        if SNR is not None:
            if prm.ndim != 2:
                raise ValueError("params should be a 2-D array [voxels x parameters], got shape %s" % (prm.shape,))
            sigma_g = prm[:, 0] / SNR
        return self._predict(prm, peaks, sig_csf, 'raise', sigma_g=sigma_g, ncoils=int(N), seed=_sos_seed(seed), offset=offset)

    def posterior(self, data, peaks, numfasc, sigma=None, fit=None, props=None, on_error='raise', *, weights=None):
        """The soft answer beside ``fit``'s arg-min (``engine.posterior2d``, include/mfx_soft2d.h): for every atom of each
        fascicle its posterior weight given the noise level, proportional to the sum over all partner atoms of
        exp(-F / 2 sigma^2).  ``data``, ``peaks``, ``numfasc`` as for ``fit`` (voxels of one or two fascicles are served;
        the others get NaN rows, status -1 and are counted).  ``sigma``: the noise standard deviation, a scalar or one
        value per voxel; default: the fit's residual variance, sigma^2 = MSE * M / (M - K) per voxel, from ``fit`` (a
        :class:`Fit2DResult` of the same voxels) or from a fit made here; a voxel with MSE = 0 gets status 1.  ``props``:
        a dict mapping a name to an [N] array of atom properties, for the result's ``mean``, ``std``, ``quantile`` and
        ``by_property``.  Returns a ``mf.Posterior`` (its ``dir_status`` [V, 5] holds the failing directions' records:
        such voxels have status 5 and NaN rows with ``on_error='nan'``; ``'raise'`` raises the reference's exception for
        the lowest of them).  ``weights``: the measurement weights of a weighted fit, as for ``fit`` (default: those of
        ``fit``, a result of ``fit(weights=...)``; ValueError when both are given and differ).  F is then the weighted
        sum of squares and ``sigma`` the noise of a measurement of weight 1: measurement m has variance sigma^2 / W_m;
        the default is sigma^2 = MSE * sum_m W / (n_pos - K) with n_pos the number of positive weights."""
        from .mf import Posterior
        data, peaks, numfasc, maxfasc = _soft2d_args(self, data, peaks, numfasc, on_error)
        props = _soft2d_props(self, props)
        V = data.shape[0]
        W = _w2d_weights(self, weights, V) if weights is not None else None
        if fit is not None:
            if np.asarray(fit.MSE).shape != (V,):
                raise ValueError("fit should hold the same %d voxels" % V)
            fw = getattr(fit, "weights", None)
            if W is None:
                W = fw
            elif fw is None or not np.array_equal(np.broadcast_to(fw, (V, self.M)), np.broadcast_to(W, (V, self.M))):
                raise ValueError("weights differ from those of fit (%d voxels): give one of them" % V)
        scope = (numfasc >= 1) & (numfasc <= 2)
        if fit is None:
            mse = np.full(V, np.nan)
            ix = np.flatnonzero(scope)
            if ix.size and W is None:
                mse[ix] = engine.fit2d(self, data[ix], numfasc[ix], None, peaks[ix], maxfasc, False)[0][:, -2]
            elif ix.size:
                mse[ix] = engine.fit2d_weighted(self, data[ix], W[ix] if W.ndim == 2 else W, numfasc[ix], None, peaks[ix],
                                                maxfasc, False)[0][:, -2]
        else:
            mse = np.asarray(fit.MSE, dtype=np.float64)
        if W is None:
            sse, n_meas = mse * self.M, float(self.M)
        else:
            sse, n_meas = mse * np.sum(W, axis=-1), np.count_nonzero(W > 0, axis=-1).astype(np.float64)
        if sigma is None:
            dof = n_meas - numfasc.astype(np.float64)
            with np.errstate(invalid='ignore', divide='ignore'):
                sig = np.sqrt(sse / dof)
            if W is not None:
                sig = np.where(dof > 0, sig, np.nan)
        else:
            sig = engine._per_voxel(sigma, V, "sigma")
        w, log_sum, status, dstat, n_uns = engine.posterior2d(self, data, numfasc, peaks, maxfasc, sig,
                                                              shift=np.where(np.isfinite(sse), sse, 0.0), W=W)
        _soft2d_raise(self, dstat, on_error)
        r = Posterior(w, log_sum, status, n_uns, np.arange(V), props, numfasc, 2.0 * sig ** 2, self.M, W=W)
        r.dir_status = dstat
        return r

    def profile(self, data, peaks, numfasc, partner=False, props=None, on_error='raise', *, weights=None):
        """What the exhaustive search of ``fit`` saw beside its arg-min (``engine.profile2d``): for every atom of each
        fascicle the smallest sum of squared residuals any partner atom reaches with it.  Arguments as ``posterior``.
        Returns a ``mf.ObjectiveProfile``: ``obj`` [V, maxfasc, N], ``partner`` (int32, -1 where there is none; None
        unless asked for), ``n_unsupported``, ``by_property(name)``, and ``dir_status`` [V, 5].  ``weights``: measurement
        weights as for ``fit``: ``obj`` is the weighted sum of squares, whose minimum is the weighted fit's MSE * sum_m W."""
        from .mf import ObjectiveProfile
        data, peaks, numfasc, maxfasc = _soft2d_args(self, data, peaks, numfasc, on_error)
        props = _soft2d_props(self, props)
        W = _w2d_weights(self, weights, data.shape[0]) if weights is not None else None
        obj, par, dstat, n_uns = engine.profile2d(self, data, numfasc, peaks, maxfasc, partner=partner, W=W)
        _soft2d_raise(self, dstat, on_error)
        r = ObjectiveProfile(obj, par, n_uns, np.arange(data.shape[0]), props)
        r.dir_status = dstat
        return r

    def interval(self, data, peaks, numfasc, values, rel=0.0, delta=0.0, *, weights=None):
        """The range of the atom property ``values`` [N] that fits the data within a margin of the optimum
        (``profile_interval`` of ``profile``): ``(lo, hi, count)`` of shape [V, maxfasc]; NaN / 0 for absent fascicles
        and voxels out of scope.  ``weights``: measurement weights as for ``fit``."""
        return profile_interval(self.profile(data, peaks, numfasc, weights=weights).obj, values, rel, delta)

    def posterior_moments(self, data, peaks, numfasc, values, sigma=None, *, weights=None):
        """Posterior mean and standard deviation of the atom property ``values`` [N] per voxel and fascicle
        (``posterior_moments`` of the weights of ``posterior``): ``(mean, std)`` of shape [V, maxfasc].  ``weights``:
        measurement weights as for ``fit``."""
        return posterior_moments(self.posterior(data, peaks, numfasc, sigma=sigma, weights=weights).weights, values)

    def rotate_cols(self, newdirs, cols):
        """Atom ``cols[b]`` for a fascicle along ``newdirs[b]`` -> [B, M]."""
        d = L.f64c(np.asarray(newdirs, dtype=np.float64).reshape(-1, 3))
        c = np.ascontiguousarray(np.asarray(cols).reshape(-1), dtype=np.int32)
        if c.shape[0] != d.shape[0]:
            raise ValueError("rotate_cols: one atom index per direction")
        out = np.zeros((d.shape[0], self.M))
        status = np.zeros((d.shape[0], 4), dtype=np.int32)
        if d.shape[0]:
            L.check(L.lib().mfx_rot2d_rotate_cols(self.handle(), L.dptr(d), L.iptr(c), d.shape[0], L.dptr(out),
                                                  L.iptr(status)))
        self.raise_for_status(status)
        return out


class Fit2DResult:
    """Parameters of voxels fitted with a 2-D protocol: ``params`` [V, num_params(maxfasc, csf_on, False)] and
    its columns ``M0`` [V], ``frac`` [V, maxfasc], ``atoms`` [V, maxfasc] (int64 atom indices; 0 for an absent
    fascicle or a voxel that was not fitted), ``frac_csf`` [V] (None without a CSF column), ``MSE``, ``R2`` [V];
    ``status`` [V, 5] int32: {code, pair, value, value2, fascicle} of the voxel's lowest failing fascicle
    direction, zeros for a fitted voxel (such a voxel's row is NaN).  ``weights``: the measurement weights [V, M] or [M]
    (float64) of a weighted fit, None for an unweighted one.  A robust fit (``fit(..., robust=...)``) keeps its final
    weights [V, M] there and has ``robust_info`` (``engine.fit2d_robust``'s dict; None otherwise), ``robust_scale`` [V]
    (the median absolute residual the last weights were made with), ``n_rejected`` [V] and ``outlier_mask()``."""

    robust_info = robust_scale = n_rejected = _robust_base = None

    def __init__(self, params, status, maxfasc, csf_on, weights=None):
        params = np.asarray(params, dtype=np.float64)
        maxfasc = int(maxfasc)
        if params.ndim != 2 or params.shape[1] != engine.num_params(maxfasc, bool(csf_on), False):
            raise ValueError("params should have %d columns" % engine.num_params(maxfasc, bool(csf_on), False))
        self.params, self.status = params, np.asarray(status, dtype=np.int32).reshape(params.shape[0], 5)
        self.maxfasc, self.csf_on = maxfasc, bool(csf_on)
        self.weights = weights
        self.M0 = params[:, 0]
        self.frac = params[:, 1:1 + maxfasc]
        ids = params[:, 1 + maxfasc:1 + 2 * maxfasc]
        self.atoms = np.where(np.isfinite(ids), ids, 0).astype(np.int64)
        self.frac_csf = params[:, 1 + 2 * maxfasc] if csf_on else None
        self.MSE, self.R2 = params[:, -2], params[:, -1]

    @property
    def failed(self):
        """Indices of the voxels that were not fitted."""
        return np.flatnonzero(self.status[:, 0])

    def _set_robust(self, info, base):
        self.robust_info, self._robust_base = info, base
        self.robust_scale = info['scale']
        self.n_rejected = np.count_nonzero(self.outlier_mask(), axis=1)

    def outlier_mask(self):
        """The measurements a robust fit rejected, bool [V, M]: True where a row the base weights admit ended with weight 0."""
        if self.robust_info is None:
            raise RuntimeError("this fit is not a robust fit (fit(..., robust=...)): it has rejected nothing")
        base = np.ones(self.weights.shape[1], dtype=bool) if self._robust_base is None else np.asarray(self._robust_base) > 0
        return base & (self.weights == 0)


class Bootstrap2DResult:
    """Result of ``RotateAtom2DTables.bootstrap``: flat arrays over the bootstrapped voxels, as :class:`Fit2DResult`'s.
    ``mean(name)``, ``std(name)``, ``min(name)``, ``max(name)``, ``quantile(name, q)`` and ``n_valid(name)`` are taken over
    the replicates of a voxel: ``name`` is one of the ``props`` given ([n, maxfasc]; a replicate counts for fascicle k only
    where its weight nu_k is positive - ``n_valid`` says how many did), 'frac' (the fascicle weights, [n, maxfasc]), or
    'M0', 'frac_csf', 'MSE' ([n]); these count every replicate.  ``agreement`` [n, maxfasc]: the share of replicates that
    chose the own fit's atom with a positive weight; ``status`` [n]: 0 fine, 1 no degree of freedom, 2 original row not
    usable (a non-finite measurement, a failing direction); ``dir_status`` [n, 5]: the failing directions' records of
    :class:`Fit2DResult`; ``stats`` [n, C, 5 + Q] with ``columns``, the table the members are cut from; ``replicates``
    [n, B, num_params] with ``keep=True``, else None; ``B``, ``seed``, ``q``, ``voxels`` (the batch positions the rows
    stand for).  ``weights``: the measurement weights [n, M] or [M] a ``fixed_weights=True`` bootstrap held fixed, else
    None; ``status`` then also has 3 (a weight negative or not finite) and 4 (no positive weight), 1 counts the rows of
    positive weight, and 'MSE' is the weighted MSE.  No replicate re-ran a rejection: after a robust fit the statistics are
    conditional on the rows that were rejected."""

    def __init__(self, res, prop_names, q, voxels, maxfasc, csf_on, B, seed, weights=None):
        self.weights = weights
        self.stats, self.columns, self.replicates = res['stats'], res['columns'], res['replicates']
        self.status, self.dir_status = res['status'], res['dir_status']
        self.B, self.seed, self.q, self.voxels = int(B), seed, np.asarray(q, dtype=np.float64), voxels
        self.maxfasc, self.csf_on = int(maxfasc), bool(csf_on)
        self._names = list(prop_names)
        self.agreement = res['agree'].astype(np.float64) / float(B)

    def _cols(self, name):
        """(column indices, per fascicle?) of a statistic's name."""
        if name in self._names:
            t = self._names.index(name)
            return [self.columns.index(('prop', k, t)) for k in range(self.maxfasc)], True
        if name == 'frac':
            return [self.columns.index('nu_%d' % k) for k in range(self.maxfasc)], True
        single = {'M0': 'M0', 'MSE': 'MSE'}
        if self.csf_on:
            single['frac_csf'] = 'nu_csf'
        if name in single:
            return [self.columns.index(single[name])], False
        raise ValueError("unknown bootstrap statistic %s (have: %s)" % (name, ", ".join(self._names + ['frac'] + sorted(single))))

    def _stat(self, name, i):
        cols, per_fasc = self._cols(name)
        return self.stats[:, cols, i] if per_fasc else self.stats[:, cols[0], i]

    def n_valid(self, name):
        return self._stat(name, 0).astype(np.int64)

    def mean(self, name):
        return self._stat(name, 1)

    def std(self, name):
        return self._stat(name, 2)

    def min(self, name):
        return self._stat(name, 3)

    def max(self, name):
        return self._stat(name, 4)

    def quantile(self, name, q):
        """The quantile ``q`` - one of those the bootstrap was asked for (``self.q``) - by linear interpolation."""
        hit = np.flatnonzero(self.q == float(q))
        if hit.size == 0:
            raise ValueError("quantile %r was not asked for (have: %s)" % (q, ", ".join("%g" % x for x in self.q)))
        return self._stat(name, 5 + int(hit[0]))


def _boot2d(T, data, peaks, numfasc, fit, csf_mask, sig_csf, on_error, B, kind, seed, inflate, q, props, voxels, keep, groups,
            max_bytes=None, weights=None, fixed_weights=False):
    """RotateAtom2DTables.bootstrap: every argument is checked before any device call."""
    if not isinstance(fixed_weights, (bool, np.bool_)):
        raise ValueError("fixed_weights should be True or False, got %r" % (fixed_weights,))
    if weights is not None and not fixed_weights:
        raise ValueError("weights= is served only with fixed_weights=True: the bootstrap holds them fixed in every replicate")
    B, code, qa = engine._boot_rule(B, kind, q, seed)
    data, peaks, numfasc, maxfasc = _soft2d_args(T, data, peaks, numfasc, on_error)
    if maxfasc > 3:
        raise NotImplementedError("the 2-D protocol fit serves at most 3 fascicles per voxel (peaks holds %d)" % maxfasc)
    V = data.shape[0]
    csf = None
    if csf_mask is not None:
        csf = np.asarray(csf_mask).astype(bool)
        if csf.shape != (V,):
            raise ValueError("csf_mask should have one entry per voxel")
    csf_on = csf is not None
    if csf_on and np.any(csf) and sig_csf is None:
        raise ValueError("voxels flagged CSF need sig_csf")
    if sig_csf is not None and np.asarray(sig_csf).size != T.M:
        raise ValueError("sig_csf has %d entries, protocol has %d" % (np.asarray(sig_csf).size, T.M))
    if csf_on and sig_csf is None:
        sig_csf = np.zeros(T.M)   # (no voxel is flagged: never read)
    p0 = None
    if fit is not None:
        if not isinstance(fit, Fit2DResult):
            raise ValueError("fit should be the Fit2DResult of these voxels")
        if (fit.weights is not None or fit.robust_info is not None) and not fixed_weights:
            raise NotImplementedError("bootstrap of a weighted or robust fit is not served")
        if fit.params.shape[0] != V or fit.maxfasc != maxfasc or fit.csf_on != csf_on:
            raise ValueError("fit should hold the same %d voxels in the layout of these arguments (maxfasc = %d, csf %s)"
                             % (V, maxfasc, csf_on))
        p0 = fit.params
    W = None
    if fixed_weights:
        W = _w2d_weights(T, weights, V) if weights is not None else None
        fw = fit.weights if fit is not None else None
        if W is None:
            W = None if fw is None else np.ascontiguousarray(fw, dtype=np.float64)   # (checked when the fit was made)
        elif fit is not None and (fw is None or not np.array_equal(np.broadcast_to(fw, (V, T.M)), np.broadcast_to(W, (V, T.M)))):
            raise ValueError("weights differ from those of fit (%d voxels): give one of them" % V)
        if W is None:
            raise ValueError("fixed_weights=True needs a fit made with weights= or robust=: %s"
                             % ("this fit has no measurement weights" if fit is not None else "no fit and no weights= were given"))
    props = _soft2d_props(T, props)
    names = list(props)
    pr = np.stack([props[n] for n in names]) if names else None
    if code == 1 and groups is None:
        groups = np.unique(T._arrays['sch'][:, 3:6], axis=0, return_inverse=True)[1].reshape(-1)
    gr = engine._boot_groups_arg(code, groups, T.M, None)
    vox = np.arange(V) if voxels is None else np.asarray(voxels, dtype=np.int64).reshape(-1)
    if vox.size and (vox.min() < 0 or vox.max() >= V):
        raise ValueError("voxels should be positions in the batch (0..%d)" % (V - 1))
    extra = {} if max_bytes is None else {'max_bytes': max_bytes}
    if W is not None:
        Wv = W if W.ndim == 1 else np.ascontiguousarray(W[vox])   # the shared [M] vector as it is, else the voxels' rows
        res = engine.fit2d_weighted_bootstrap(T, data[vox], Wv, numfasc[vox], csf[vox] if csf_on else None, peaks[vox], maxfasc,
                                              csf_on, sig_csf, B=B, kind=kind, seed=seed, inflate=inflate, q=qa, props=pr, groups=gr,
                                              params=np.ascontiguousarray(p0[vox]) if p0 is not None else None, vox=vox, keep=keep,
                                              **extra)
        _soft2d_raise(T, res['dir_status'], on_error)
        return Bootstrap2DResult(res, names, qa, vox, maxfasc, csf_on, B, seed, weights=Wv)
    res = engine.fit2d_bootstrap(T, data[vox], numfasc[vox], csf[vox] if csf_on else None, peaks[vox], maxfasc, csf_on, sig_csf,
                                 B=B, kind=kind, seed=seed, inflate=inflate, q=qa, props=pr, groups=gr,
                                 params=np.ascontiguousarray(p0[vox]) if p0 is not None else None, vox=vox, keep=keep, **extra)
    _soft2d_raise(T, res['dir_status'], on_error)
    return Bootstrap2DResult(res, names, qa, vox, maxfasc, csf_on, B, seed)


def _w2d_weights(T, weights, V):
    """weights argument of the 2-D protocols' entry points -> float64 [V, M] or [M], checked before any device call (every
    failure a ValueError naming the voxel count, as MFModel.fit's)."""
    w = np.asarray(weights)
    if w.dtype == object or not (np.issubdtype(w.dtype, np.number) or w.dtype == np.bool_) or np.iscomplexobj(w):
        raise ValueError("weights should be boolean or real numbers (%d voxel(s))." % V)
    if w.shape != (T.M,) and w.shape != (V, T.M):
        raise ValueError("weights not compatible with the data of %d voxel(s): expected shape (%d, %d) or (%d,), got %s."
                         % (V, V, T.M, T.M, w.shape))
    w = np.ascontiguousarray(w, dtype=np.float64)
    bad = ~np.isfinite(w) | (w < 0)
    if bad.any():
        n_bad = V if w.ndim == 1 else int(np.count_nonzero(bad.any(axis=1)))
        raise ValueError("Detected %d of %d voxel(s) with negative or non-finite weights." % (n_bad, V))
    none = ~(w > 0).any(axis=-1)
    if np.any(none):
        n_none = V if w.ndim == 1 else int(np.count_nonzero(none))
        raise ValueError("Detected %d of %d voxel(s) without a positive weight." % (n_none, V))
    return w


def _fit2d(T, data, peaks, numfasc, csf_mask, sig_csf, on_error, weights=None, robust=None):
    if on_error not in ("raise", "nan"):
        raise ValueError("on_error should be 'raise' or 'nan'")
    opts = engine.robust_options(robust)
    data = np.asarray(data, dtype=np.float64)
    if data.ndim != 2 or data.shape[1] != T.M:
        raise ValueError("data has shape %s, protocol has %d measurements" % (data.shape, T.M))
    V = data.shape[0]
    numfasc = np.asarray(numfasc)
    if numfasc.shape != (V,):
        raise ValueError("numfasc should have one entry per voxel")
    peaks = np.asarray(peaks, dtype=np.float64)
    if peaks.ndim != 2 or peaks.shape[0] != V or peaks.shape[1] % 3 != 0:
        raise ValueError("peaks should have shape (%d, 3 maxfasc)" % V)
    maxfasc = peaks.shape[1] // 3
    if maxfasc > 3:
        raise NotImplementedError("the 2-D protocol fit serves at most 3 fascicles per voxel (peaks holds %d)" % maxfasc)
    if V and (numfasc.min() < 0 or numfasc.max() > maxfasc):
        raise ValueError("numfasc should lie in 0..%d (the directions peaks holds per voxel)" % maxfasc)
    csf = None
    if csf_mask is not None:
        csf = np.asarray(csf_mask).astype(bool)
        if csf.shape != (V,):
            raise ValueError("csf_mask should have one entry per voxel")
    csf_on = csf is not None
    if csf is not None and np.any(csf):
        if sig_csf is None:
            raise ValueError("voxels flagged CSF need sig_csf")
    if sig_csf is not None and np.asarray(sig_csf).size != T.M:
        raise ValueError("sig_csf has %d entries, protocol has %d" % (np.asarray(sig_csf).size, T.M))
    W = _w2d_weights(T, weights, V) if weights is not None else None
    if opts is not None:
        sc = sig_csf if (sig_csf is not None or not csf_on) else np.zeros(T.M)   # (no voxel is flagged: never read)
        params, Wf, info = engine.fit2d_robust(T, data, numfasc, csf, peaks, maxfasc, csf_on, sc, W0=W, **opts)
        if on_error == "raise":
            bad = np.flatnonzero(info['dir_status'][:, 0])
            if bad.size:
                raise T.error_for(info['dir_status'][bad[0], :4])
        r = Fit2DResult(params, info['dir_status'], maxfasc, csf_on, Wf)
        r._set_robust(info, W)
        return r
    if W is None:
        params, status = engine.fit2d(T, data, numfasc, csf, peaks, maxfasc, csf_on, sig_csf)
    else:
        params, status, _ = engine.fit2d_weighted(T, data, W, numfasc, csf, peaks, maxfasc, csf_on, sig_csf)
    if on_error == "raise":
        bad = np.flatnonzero(status[:, 0])
        if bad.size:
            raise T.error_for(status[bad[0], :4])
    return Fit2DResult(params, status, maxfasc, csf_on, W)


def _soft2d_args(T, data, peaks, numfasc, on_error):
    """Argument checks of RotateAtom2DTables.posterior / .profile (before any device call)."""
    if on_error not in ("raise", "nan"):
        raise ValueError("on_error should be 'raise' or 'nan'")
    data = np.asarray(data, dtype=np.float64)
    if data.ndim != 2 or data.shape[1] != T.M:
        raise ValueError("data has shape %s, protocol has %d measurements" % (data.shape, T.M))
    V = data.shape[0]
    numfasc = np.asarray(numfasc)
    if numfasc.shape != (V,):
        raise ValueError("numfasc should have one entry per voxel")
    peaks = np.asarray(peaks, dtype=np.float64)
    if peaks.ndim != 2 or peaks.shape[0] != V or peaks.shape[1] % 3 != 0:
        raise ValueError("peaks should have shape (%d, 3 maxfasc)" % V)
    maxfasc = peaks.shape[1] // 3
    if V and (numfasc.min() < 0 or numfasc.max() > maxfasc):
        raise ValueError("numfasc should lie in 0..%d (the directions peaks holds per voxel)" % maxfasc)
    return data, peaks, numfasc.astype(np.int64), maxfasc


def _soft2d_props(T, props):
    out = {}
    for name, v in (props or {}).items():
        v = np.asarray(v, dtype=np.float64).reshape(-1)
        if v.shape[0] != T.N:
            raise ValueError("property %s has %d entries, the dictionary has %d atoms" % (name, v.shape[0], T.N))
        out[name] = v
    return out


def _soft2d_raise(T, dir_status, on_error):
    if on_error == "raise":
        bad = np.flatnonzero(dir_status[:, 0])
        if bad.size:
            raise T.error_for(dir_status[bad[0], :4])


def fit_2Dprotocol(sig, sch_mat, refdir, DIFF, data, peaks, numfasc, csf_mask=None, sig_csf=None, on_error='raise',
                   device=0, *, weights=None, robust=None):
    """Fit voxels of a 2-D protocol: :class:`RotateAtom2DTables` of (sig, sch_mat, refdir, DIFF), then its ``fit``
    (``weights``: its measurement weights; ``robust``: its robust options)."""
    return RotateAtom2DTables(sig, sch_mat, refdir, DIFF, device=device).fit(data, peaks, numfasc, csf_mask, sig_csf,
                                                                            on_error, weights=weights, robust=robust)


def rotate_atom_2Dprotocol(sig, sch_mat, refdir, newdir, DIFF):
    """Signals of a 2-D (AxCaliber-like) protocol rotated from a fascicle along ``refdir`` to one along
    ``newdir`` (ref:1440-1690).  ``sig`` [M] or [M, N]; returns the same shape.  ``newdir`` is not normalised."""
    T = RotateAtom2DTables(sig, sch_mat, refdir, DIFF)
    newdir = np.asarray(newdir, dtype=np.float64)
    if newdir.size != 3:
        raise ValueError("cyldir1 and cyldir2 should be 3-elements NumPy arrays.")
    if ~np.isclose(np.sum(newdir ** 2), 1):         # also checked on the device, for batches
        raise ValueError("cyldir1 and cyldir2 should have unit norm.")
    return np.reshape(T.rotate(newdir.reshape(1, 3))[0], T.sig_shape)


# ---------------------------------------------------------------------------------------------
# solver
# ---------------------------------------------------------------------------------------------
def solve_exhaustive_posweights(A, y, dicsizes, printmsg=None):
    """Combinatorial NNLS with exactly one atom per sub-dictionary (ref:115-214).

    Returns ``(w_nneg, ind_atoms_subdic, ind_atoms_totdic, min_obj, y_recons)``."""
    if printmsg is not None:
        print(printmsg, end="")
    # input checks: same conditions and AssertionError as ref:157-188
    assert isinstance(A, np.ndarray), "A should be a NumPy ndarray"
    assert A.ndim == 2, "A should be a 2D array"
    assert not np.any(np.all(A == 0, axis=0)), "All-zero columns detected in A"
    assert isinstance(y, np.ndarray), "y should be a NumPy ndarray"
    assert A.size > 0 and y.size > 0, "A and y should not be empty arrays"
    assert A.shape[0] == y.size, ("Number of rows in A (%d) should match number of elements in y (%d)"
                                  % (A.shape[0], y.size))
    assert isinstance(dicsizes, np.ndarray), "dicsizes should be a NumPy ndarray"
    assert np.all(dicsizes > 0), "All entries of dicsizes should be > 0"
    assert A.shape[1] == np.sum(dicsizes), ("Number of columns of A (%d) does not equal sum of size of "
                                            "sub-matrices in diclengths array (%d)"
                                            % (A.shape[1], np.sum(dicsizes)))
    A64 = L.f64c(A)
    y64 = L.f64c(y).reshape(-1)
    sizes = np.ascontiguousarray(dicsizes, dtype=np.int64).reshape(-1)
    Kp = sizes.size
    w = np.zeros(Kp)
    sub = np.zeros(Kp, dtype=np.int64)
    tot = np.zeros(Kp, dtype=np.int64)
    obj = np.zeros(1)
    yrec = np.zeros(A64.shape[0])
    L.check(L.lib().mfx_solve_exhaustive(L.dptr(A64), A64.shape[1], A64.shape[0], L.lptr(sizes), Kp, L.dptr(y64),
                                         L.dptr(w), L.lptr(sub), L.lptr(tot), L.dptr(obj), L.dptr(yrec)))
    if Kp <= 3:
        # the reference's Numba kernels return int32 index arrays (ref:218-224, 284-286, 466-468)
        sub, tot = sub.astype(np.int32), tot.astype(np.int32)
    return w, sub, tot, float(obj[0]), yrec


def _check_dictionary(A, dicsizes):
    """The checks of ``solve_exhaustive_posweights`` that concern the dictionary: same conditions and texts (ref:157-188)."""
    assert isinstance(A, np.ndarray), "A should be a NumPy ndarray"
    assert A.ndim == 2, "A should be a 2D array"
    assert not np.any(np.all(A == 0, axis=0)), "All-zero columns detected in A"
    assert A.size > 0, "A and y should not be empty arrays"
    assert isinstance(dicsizes, np.ndarray), "dicsizes should be a NumPy ndarray"
    assert np.all(dicsizes > 0), "All entries of dicsizes should be > 0"
    assert A.shape[1] == np.sum(dicsizes), ("Number of columns of A (%d) does not equal sum of size of "
                                            "sub-matrices in diclengths array (%d)"
                                            % (A.shape[1], np.sum(dicsizes)))


class ExhaustiveSolver:
    """``solve_exhaustive_posweights`` for MANY signals against ONE dictionary (include/mfx_solve.h).

    The dictionary and its Gram matrix live on the device for the life of the object; per signal only ``A^T y`` and
    ``||y||^2`` are formed.  Row ``v`` of a batch equals, bit for bit, what ``solve_exhaustive_posweights(A, Y[v],
    dicsizes)`` returns (the batch never takes that function's matrix-pipe screen for three large sub-dictionaries; it
    returns what the plain scan returns there).  The checks on ``A`` and ``dicsizes`` are those of the one-problem
    function, made here before the device is touched.  A context manager; ``close()`` releases the device memory."""

    def __init__(self, A, dicsizes, device=0):
        _check_dictionary(A, dicsizes)
        self._A = L.f64c(A)
        self.dicsizes = np.ascontiguousarray(dicsizes, dtype=np.int64).reshape(-1)
        self.M = int(self._A.shape[0])
        self.num_columns = int(self._A.shape[1])
        self.Kp = int(self.dicsizes.size)
        self.device = int(device)
        self.starts = np.concatenate(([0], np.cumsum(self.dicsizes)[:-1])).astype(np.int64)
        self._h = None
        self._starts_dev = {}

    def handle(self):
        if self._h is None:
            h = C.c_void_p()
            L.check(L.lib().mfx_solve_create(L.dptr(self._A), self.num_columns, self.M, L.lptr(self.dicsizes), self.Kp,
                                             self.device, C.byref(h)))
            self._h = h
        return self._h

    def close(self):
        if self._h is not None:
            L.lib().mfx_solve_destroy(self._h)
            self._h = None
        self._starts_dev = {}

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def starts_on(self, dev):
        """First column of every sub-dictionary as an int64 tensor on the torch device ``dev``, uploaded once."""
        import torch
        key = str(dev)
        if key not in self._starts_dev:
            self._starts_dev[key] = torch.from_numpy(self.starts).to(dev)
        return self._starts_dev[key]

    @property
    def bytes_per_signal(self):
        """Scratch bytes one signal of a batch takes on the device: what ``max_bytes`` is counted in."""
        return int(L.lib().mfx_solve_bytes_per_signal(self.handle()))

    def signal_rows(self, shape):
        """V of signals of this shape, ``[V, M]`` or one ``[M]`` vector; a ValueError that names both shapes otherwise."""
        shape = tuple(shape)
        if len(shape) == 1 and shape[0] == self.M:
            return 1
        if len(shape) != 2 or shape[1] != self.M:
            raise ValueError("signals should have shape (V, %d) or (%d,) for a dictionary of shape %s, got %s"
                             % (self.M, self.M, (self.M, self.num_columns), shape))
        return int(shape[0])

    def index_dtype(self):
        # the reference's Numba kernels return int32 index arrays for up to three sub-dictionaries (ref:218-224, 284-286, 466-468)
        return np.int32 if self.Kp <= 3 else np.int64

    def solve(self, Y, recons=True, max_bytes=0):
        """Signals ``Y [V, M]`` (or one ``[M]`` vector: V = 1) -> ``(w [V, Kp], ind_subdic [V, Kp], ind_totdic [V, Kp],
        min_obj [V], y_recons [V, M] or None without ``recons``, status [V])``.  status 1: the signal holds a non-finite
        value; its weights, objective and reconstruction are NaN and its indices -1.  The signals go through the device
        in chunks whose scratch stays within ``max_bytes`` (0: 256 MiB)."""
        assert isinstance(Y, np.ndarray), "y should be a NumPy ndarray"
        V = self.signal_rows(Y.shape)
        Kp, M = self.Kp, self.M
        w = np.zeros((V, Kp))
        sub = np.zeros((V, Kp), dtype=np.int64)
        obj = np.zeros(V)
        yrec = np.zeros((V, M)) if recons else None
        status = np.zeros(V, dtype=np.int32)
        if V > 0:
            Y64 = L.f64c(Y).reshape(V, M)
            L.check(L.lib().mfx_solve_batch(self.handle(), L.dptr(Y64), V, int(max_bytes), L.dptr(w), L.lptr(sub), L.dptr(obj),
                                            L.opt(yrec), L.iptr(status)))
        tot = np.where(sub >= 0, sub + self.starts[None, :], -1)
        dt = self.index_dtype()
        return w, sub.astype(dt), tot.astype(dt), obj, yrec, status

    # ---- the soft answers beside the arg-min (include/mfx_solve_soft.h)
    def soft_bytes_per_signal(self, what):
        """Scratch bytes one signal takes in ``profile`` (what='profile') or ``posterior`` (what='posterior')."""
        code = {'profile': L.SOLVE_SOFT_PROFILE, 'posterior': L.SOLVE_SOFT_POST}[what]
        return int(L.lib().mfx_solve_soft_bytes_per_signal(self.handle(), code))

    def _soft_signals(self, Y):
        assert isinstance(Y, np.ndarray), "y should be a NumPy ndarray"
        V = self.signal_rows(Y.shape)
        return V, L.f64c(Y).reshape(V, self.M)

    def _soft_props(self, props, sizes):
        """``props`` {name: values} as {name: [values of every served sub-dictionary]}: one array shared by the
        sub-dictionaries where their sizes agree, or a list with one array each."""
        res = {}
        for name, vals in (props or {}).items():
            if isinstance(vals, (list, tuple)) and len(vals) == len(sizes) and all(np.ndim(x) == 1 for x in vals):
                per = [np.asarray(x, dtype=np.float64) for x in vals]
            else:
                per = [np.asarray(vals, dtype=np.float64).reshape(-1)] * len(sizes)
            for k, (x, n) in enumerate(zip(per, sizes)):
                if x.shape != (n,):
                    raise ValueError("property %r of sub-dictionary %d should have %d values, got shape %s" % (name, k, n, x.shape))
            res[name] = per
        return res

    def profile(self, Y, partner=False, props=None, max_bytes=0):
        """Objective profiles of signals ``Y [V, M]`` (or one ``[M]`` vector): for every atom of each sub-dictionary
        the best objective any partner atom reaches with it.  Served: one sub-dictionary, two, and three whose last has
        one column (that column is always in the fit, like the CSF compartment); NotImplementedError otherwise.
        ``props``: {name: values} per-atom properties for ``by_property`` / ``interval``.  Returns a ``SolverProfile``."""
        V, Y64 = self._soft_signals(Y)
        sizes = [int(n) for n in self.dicsizes[:min(self.Kp, 2)]]
        pr = self._soft_props(props, sizes)
        engine.solve_soft_sizes(self)
        obj = [np.zeros((V, n)) for n in sizes]
        par = [np.zeros((V, n), dtype=np.int32) for n in sizes] if partner else None
        status = np.zeros(V, dtype=np.int32)
        if V > 0:
            two = len(sizes) > 1
            L.check(L.lib().mfx_solve_profile(self.handle(), L.dptr(Y64), V, int(max_bytes), L.dptr(obj[0]),
                                              L.dptr(obj[1]) if two else None, L.iptr(par[0]) if par else None,
                                              L.iptr(par[1]) if par and two else None, L.iptr(status)))
        return SolverProfile(obj, par, status, pr)

    def posterior(self, Y, sigma=None, shift=None, props=None, max_bytes=0):
        """Posterior weights of every atom of each served sub-dictionary given the noise level: w proportional to the sum
        over all partner atoms of exp(-F / 2 sigma^2).  ``sigma``: the noise standard deviation, a scalar or ``[V]``
        (default: the residual variance of the best fit, sigma^2 = min F / (M - Kp); a signal with min F <= 0 or
        M <= Kp gets status 1).  ``shift`` ``[V]``: a value near each signal's smallest objective (default: min F itself).
        Returns a ``SolverPosterior``."""
        V, Y64 = self._soft_signals(Y)
        sizes = [int(n) for n in self.dicsizes[:min(self.Kp, 2)]]
        pr = self._soft_props(props, sizes)
        sig = engine._per_voxel(sigma, V, "sigma") if sigma is not None else None
        sh = engine._per_voxel(shift, V, "shift") if shift is not None else None
        engine.solve_soft_sizes(self)
        w = [np.zeros((V, n)) for n in sizes]
        log_sum, min_obj, status = np.zeros(V), np.zeros(V), np.zeros(V, dtype=np.int32)
        T = np.zeros(V)
        if V > 0:
            two = len(sizes) > 1
            if sig is None:
                # min F first: a call at T = 1 (its shift is min F, so no exponent is positive), of which min_obj is kept
                L.check(L.lib().mfx_solve_post(self.handle(), L.dptr(Y64), V, L.dptr(np.ones(V)), None, int(max_bytes), L.dptr(w[0]),
                                               L.dptr(w[1]) if two else None, L.dptr(log_sum), L.dptr(min_obj), L.iptr(status)))
                dof = self.M - self.Kp
                with np.errstate(invalid='ignore', divide='ignore'):
                    sig = np.where((min_obj > 0) & (dof > 0), np.sqrt(min_obj / max(dof, 1)), np.nan)
            T = np.ascontiguousarray(2.0 * sig ** 2)
            L.check(L.lib().mfx_solve_post(self.handle(), L.dptr(Y64), V, L.dptr(T), L.opt(sh), int(max_bytes), L.dptr(w[0]),
                                           L.dptr(w[1]) if two else None, L.dptr(log_sum), L.dptr(min_obj), L.iptr(status)))
        return SolverPosterior(w, log_sum, min_obj, status, T, self.M, pr)

    def posterior_moments(self, Y, values, sigma=None, k=0):
        """(mean, std) ``[V]`` of the per-atom property ``values`` of sub-dictionary ``k`` under ``posterior(Y, sigma)``."""
        return posterior_moments(self.posterior(Y, sigma=sigma).weights[k], values)


class _SolverSoft(object):
    def _values(self, name, k):
        if name not in self._props:
            raise KeyError("no property %r (given: %s)" % (name, sorted(self._props)))
        return self._props[name][k]


class SolverProfile(_SolverSoft):
    """Result of ``ExhaustiveSolver.profile``: ``obj`` a list with one ``[V, n_k]`` array per served sub-dictionary,
    ``partner`` the arg-min partner indices likewise (or None), ``status`` ``[V]`` (0 ok, 5 a non-finite signal)."""

    def __init__(self, obj, partner, status, props):
        self.obj, self.partner, self.status, self._props = obj, partner, status, props

    def by_property(self, name, k=0):
        """(levels, obj_by_level [V, len(levels)]) of sub-dictionary ``k`` (``profile_by_property``)."""
        return profile_by_property(self.obj[k], self._values(name, k))

    def interval(self, name, rel=0.0, delta=0.0, k=0):
        """(lo, hi, count) ``[V]``: the range of ``name`` that fits within the margin of the optimum (``profile_interval``)."""
        return profile_interval(self.obj[k], self._values(name, k), rel=rel, delta=delta)


class SolverPosterior(_SolverSoft):
    """Result of ``ExhaustiveSolver.posterior``: ``weights`` a list with one ``[V, n_k]`` array per served
    sub-dictionary (each row sums to 1), ``log_sum`` ``[V]`` = log sum exp(-F / T), ``min_obj`` ``[V]`` = min F, ``status``
    ``[V]`` (the codes of include/mfx_solve_soft.h), ``T`` ``[V]`` = 2 sigma^2."""

    def __init__(self, weights, log_sum, min_obj, status, T, M, props):
        self.weights, self.log_sum, self.min_obj, self.status, self.T = weights, log_sum, min_obj, status, T
        self._M, self._props = M, props

    def mean(self, name, k=0):
        return posterior_moments(self.weights[k], self._values(name, k))[0]

    def std(self, name, k=0):
        return posterior_moments(self.weights[k], self._values(name, k))[1]

    def quantile(self, name, q, k=0):
        return posterior_quantile(self.weights[k], self._values(name, k), q)

    def by_property(self, name, k=0):
        return posterior_by_property(self.weights[k], self._values(name, k))

    def log_evidence(self):
        """log_sum - sum_k log n_k - (M / 2) log(pi T) per signal: the log of the Gaussian likelihood averaged over a
        uniform prior on the tuples of atoms (a profile-likelihood evidence: the weights are maximised per tuple)."""
        with np.errstate(invalid='ignore', divide='ignore'):
            return self.log_sum - sum(np.log(w.shape[-1]) for w in self.weights) - 0.5 * self._M * np.log(np.pi * self.T)


def solve_exhaustive_posweights_batch(A, Y, dicsizes, device=0, **kw):
    """One-shot form of ``ExhaustiveSolver(A, dicsizes).solve(Y, **kw)``."""
    with ExhaustiveSolver(A, dicsizes, device=device) as S:
        return S.solve(Y, **kw)


# ---------------------------------------------------------------------------------------------
# protocol helpers (input normalisation before the voxel loop)
# ---------------------------------------------------------------------------------------------
def import_PGSE_scheme(scheme):
    """Load / validate a PGSE scheme ``[gx gy gz G Delta delta TE]`` (ref:2128-2192)."""
    if isinstance(scheme, str):
        with open(scheme, 'r') as f:
            skip = 1 if 'version' in f.readline().lower() else 0
        sch = np.loadtxt(scheme, skiprows=skip)
    elif isinstance(scheme, np.ndarray):
        sch = scheme
    else:
        raise TypeError("Unable to import a PGSE scheme matrix from input")
    if sch.ndim == 1:
        sch = sch[np.newaxis, :]
    if sch.shape[1] != 7:
        raise RuntimeError("Detected %s instead of expected 7 colums in PGSE scheme matrix." % sch.shape[1])
    gn = np.sqrt(np.sum(sch[:, :3] ** 2, axis=1))
    nbad = np.sum(np.abs(1 - gn[gn > 0]) > 1e-4)
    if nbad > 0:
        raise ValueError("Detected %d non-zero gradients which did not have unit norm. Please normalize." % nbad)
    G, Dl, dl, TE = sch[:, 3], sch[:, 4], sch[:, 5], sch[:, 6]
    for arr, what in ((G, 'gradient intensity (4th column)'), (Dl, 'gradient separation Delta (5th column)'),
                      (dl, 'gradient duration delta (6th column)'), (TE, 'echo time TE (7th column)')):
        if np.any(arr < 0):
            raise ValueError('Detected %d sequence(s) with negative %s.' % (np.sum(arr < 0), what))
    if np.any(dl > Dl):
        raise ValueError('Detected %d sequence(s) in which delta (6th column) was greater than Delta '
                         '(5th column).' % np.sum(dl > Dl))
    if np.any(TE < (Dl + dl) * 0.999):
        raise ValueError('Detected %d sequence(s) in which TE (7th column) was lower than Delta+delta.'
                         % np.sum(TE < (Dl + dl)))
    return sch


def _as_text_table(x):
    """A b-value / b-vector argument: a path to a whitespace-separated text file, or array-like."""
    return np.loadtxt(x) if isinstance(x, str) else np.asarray(x)


def _gradient_rows(bvecs, n):
    """b-vectors as an [n x 3] array of unit rows (zero rows stay zero).  Accepts 3 x n (FSL) and n x 3; a 3 x 3 input is
    read as 3 x n like the reference does (its test on shape[0] comes first, ref:2253-2259)."""
    if bvecs.shape[0] == 3:
        g = np.array(bvecs.T, dtype=np.float64)
    elif bvecs.shape[1] == 3:
        g = np.array(bvecs, dtype=np.float64)
    else:
        raise ValueError("Vectors in bvecs should be 3-dimensional. However, detected no dimension with size 3.")
    length = np.sqrt(np.sum(g ** 2, axis=1))
    nz = length > 0
    g[nz] = g[nz] / length[nz][:, np.newaxis]
    return g


def _snap_to_shells(G, shells, Gtol):
    """Each gradient intensity in G replaced by the dense scheme's shell value within Gtol of it; the number of
    (value, shell) matches must equal G.size - a value near no shell, or near two, is the reference's mapping error.
    Where two shells match the larger one would win (the reference assigns shell after shell in ascending order)."""
    near = np.abs(G[:, np.newaxis] - shells[np.newaxis, :]) < Gtol         # [n, S]
    n_matches = int(np.count_nonzero(near))
    last_match = near.shape[1] - 1 - np.argmax(near[:, ::-1], axis=1)
    return np.where(near.any(axis=1), shells[last_match], 0.0), n_matches


def get_PGSE_scheme_from_bval_bvec_dense(sch_mat_dense, bvals, bvecs, Gtol=1e-3):
    """Subject protocol [gx gy gz G Delta delta TE] from b-values [s/mm^2] and b-vectors, for a dictionary simulated on the
    dense multi-shell scheme ``sch_mat_dense``: timing (Delta, delta, TE) is the dense scheme's - which must be a single
    one - and every b-value is turned into a gradient intensity and snapped onto the dense scheme's shell within ``Gtol``
    [T/m] of it (reference mf_utils.py:2197-2300; same ValueErrors)."""
    dense = import_PGSE_scheme(sch_mat_dense)
    b_si = np.asarray(_as_text_table(bvals), dtype=np.float64).ravel() * 1e6          # s/mm^2 -> s/m^2
    vec = _as_text_table(bvecs)
    if isinstance(bvecs, str):
        vec = np.atleast_2d(vec)
    n = b_si.size
    if np.ndim(vec) != 2:
        raise ValueError("bvecs array should have 2 dimensions, detected %d." % np.ndim(vec))
    if n not in vec.shape:
        raise ValueError("Number of b-vectors does not match number of b-values (%d)" % n)
    timing = dense[:, 4:6]
    if not np.all(timing == timing[0]):
        raise ValueError('Detected different pairs of (Delta, delta) values in reference scheme matrix '
                         '(note that zeros count as values), which is currently not supported.')
    Delta, delta, TE = dense[0, 4:7]
    G = np.sqrt(b_si / (Delta - delta / 3)) / (get_gyromagnetic_ratio('H') * delta)     # b = (gamma G delta)^2 (Delta - delta/3)
    G_shell, n_matches = _snap_to_shells(G, np.unique(dense[:, 3]), Gtol)
    g = _gradient_rows(vec, n)
    if n_matches != n:
        raise ValueError('Mismatch between reference scheme matrix and bvals.  Could only map %d/%d b-values '
                         '(equivalently, gradient intensities G) from the specified bvals to the b-values '
                         'contained in the reference scheme matrix. You may want to change the tolerance on '
                         'gradient intensity G (currently %g T/m).' % (n_matches, n, Gtol))
    return np.column_stack([g, G_shell, np.full(n, Delta), np.full(n, delta), np.full(n, TE)])


# ---------------------------------------------------------------------------------------------
# diffusion-tensor <-> peak helpers (orientation inputs of MFModel.fit / cleanup_2fascicles)
# ---------------------------------------------------------------------------------------------
# position of each upper-triangle element (row, col) in the 6-vector, per storage convention
_DT_ORDER = {
    'row':      ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)),     # xx xy xz yy yz zz  (.nrrd)
    'column':   ((0, 0), (0, 1), (1, 1), (0, 2), (1, 2), (2, 2)),     # xx xy yy xz yz zz  (NIfTI)
    'diagonal': ((0, 0), (1, 1), (2, 2), (0, 1), (1, 2), (0, 2)),     # xx yy zz xy yz xz
}


def _dt_order(order):
    try:
        return _DT_ORDER[order]
    except (KeyError, TypeError):
        raise ValueError('Unknown order "%s".' % (order,))


def DT_array_to_vec(DT, order='row'):
    """(..., 3, 3) symmetric tensors -> (..., 6) vectors in the given element order (ref:865-898)."""
    DT = np.asarray(DT)
    if DT.ndim < 2:
        raise ValueError('DT should have at least 2 dimensions. Detected %d.' % DT.ndim)
    if DT.shape[-2:] != (3, 3):
        raise ValueError('Last 2 dimensions of DT should be (3, 3). Detected (%d, %d).' % DT.shape[-2:])
    pos = _dt_order(order)
    return np.stack([DT[..., r, c] for (r, c) in pos], axis=-1)


def DT_vec_to_2Darray(DT_vec, order):
    """(..., 6) vectors -> (..., 3, 3) symmetric tensors (ref:901-957)."""
    DT_vec = np.asarray(DT_vec)
    if DT_vec.shape[-1] != 6:
        raise ValueError("Last dimension of input should have size 6, detected %d." % DT_vec.shape[-1])
    pos = _dt_order(order)
    out = np.zeros(DT_vec.shape[:-1] + (3, 3))
    for e, (r, c) in enumerate(pos):
        out[..., r, c] = DT_vec[..., e]
        out[..., c, r] = DT_vec[..., e]
    return out


def DT_vec_to_peaks(DT_vec, order, mask=None):
    """Principal direction of every tensor in a (..., 6) array: the unit eigenvector of the largest eigenvalue, a zero
    vector where that eigenvalue is zero (an all-zero tensor) and outside ``mask`` (reference mf_utils.py:960-1019).
    A single 6-vector gives a single 3-vector."""
    tensors = np.asarray(DT_vec)
    single = tensors.ndim == 1
    if single:
        tensors = tensors[np.newaxis, :]
    if tensors.shape[-1] != 6:
        raise ValueError('DT_vec should have size 6 along last dimension. Detected %d.' % (tensors.shape[-1],))
    grid = tensors.shape[:-1]
    inside = np.ones(grid, dtype=bool) if mask is None else np.asarray(mask)
    if inside.ndim != len(grid):
        raise ValueError('mask should have %d dimension(s) since DT_vec has %d, detected %d instead.'
                         % (len(grid), len(grid) + 1, inside.ndim))
    inside = inside > 0
    peaks = np.zeros(grid + (3,))
    if np.any(inside):
        evals, evecs = np.linalg.eigh(DT_vec_to_2Darray(tensors[inside], order))      # eigenvalues ascending
        principal = evecs[:, :, 2]
        principal[np.abs(evals[:, 2]) == 0] = 0.0                # eigh hands back the identity for a zero tensor
        peaks[inside] = principal
    return peaks[0] if single and peaks.shape[0] == 1 else (np.squeeze(peaks) if single else peaks)


def peaks_to_DT_vec(peaks, order, lam_par=2e-3, lam_perp=0.1e-3):
    """Stick-like tensors ``lam_par v v' + lam_perp (I - v v')`` for display (ref:1022-1135).

    The reference draws a random perpendicular pair (p1, p2) and sums ``lam_perp (p1 p1' + p2 p2')``;
    for any orthonormal completion that sum is ``lam_perp (I - v v')``, which is what is formed here
    (same tensor up to rounding, and deterministic).  Returns a list with one (..., 6) array per
    peak; like the reference, non-zero input peaks are normalised in place."""
    if peaks.ndim < 2:
        raise ValueError('peaks array should have at least 2 dimensions. Detected %d.' % peaks.ndim)
    if peaks.shape[-1] != 3:
        raise ValueError('Last dimension of peaks should have size 3, detected %d.' % (peaks.shape[-1]))
    if lam_par < lam_perp:
        raise ValueError('Parallel diffusivity should be greater than or equal to perpendicular diffusivity.')
    pos = _dt_order(order)
    nrm = np.sqrt(np.sum(peaks ** 2, axis=-1))
    nz = nrm > 0
    peaks[nz, :] = peaks[nz, :] / nrm[nz][:, np.newaxis]
    v = peaks[nz, :]
    DT = (lam_par - lam_perp) * v[:, :, np.newaxis] * v[:, np.newaxis, :] + lam_perp * np.eye(3)
    tens = np.zeros(peaks.shape[:-1] + (6,))
    tens[nz, :] = np.stack([DT[:, r, c] for (r, c) in pos], axis=-1)
    return [tens[..., k, :] for k in range(peaks.shape[-2])]


# ---------------------------------------------------------------------------------------------
# Monte-Carlo signal synthesis from stored spin phases (dictionary generation)
# ---------------------------------------------------------------------------------------------
def monte_carlo_average(sim_phases, delta_mapping, gscaling, Dscaling, num_spins, device=0):
    """``S_i = mean_l cos(Dscaling * sum_n gscaling[i,n] * sim_phases[delta_mapping[i]*num_spins + l, n])``
    (ref:2758-2810), evaluated on the GPU.  Per-term arithmetic follows the reference order; the
    spins are summed in a fixed tree order instead of sequentially."""
    ph = L.f64c(sim_phases)
    if ph.ndim != 2:
        raise ValueError("sim_phases should have 2 dimensions (n_spin*n_ref, n_dim), detected %d." % ph.ndim)
    dm = np.ascontiguousarray(delta_mapping, dtype=np.int64).reshape(-1)
    gs = L.f64c(gscaling)
    if gs.ndim != 2 or gs.shape[0] != dm.size or gs.shape[1] != ph.shape[1]:
        raise ValueError("gscaling should have shape (%d, %d), got %s." % (dm.size, ph.shape[1], gs.shape))
    out = np.zeros(dm.size)
    L.check(L.lib().mfx_monte_carlo_average(L.dptr(ph), ph.shape[0], ph.shape[1], L.lptr(dm), L.dptr(gs),
                                            float(Dscaling), int(num_spins), dm.size, L.dptr(out), int(device)))
    return out


def _phase_file_format(phasefile):
    """('<'|'>', 'f4'|'f8', bytes per item, directory, basename, extension) from the file name
    (ref:2904-2934): extension = endianness letter (b/l) + storage type (single|float|double)."""
    import os
    folder, tail = os.path.split(phasefile)
    base, ext = os.path.splitext(tail)
    if not ext:
        raise ValueError("Phase file extension not found.\nAborting as there is no way to tell which level of "
                         "precision was used to store the phase values (e.g., float, double, ...).")
    endian = {'b': '>', 'l': '<'}.get(ext[1].lower())
    if endian is None:
        raise ValueError("Phase file extension (after the dot) should start with a b for big endian or with a l "
                         "for little endian. Detected: \"%s\"." % ext[1])
    if ext[2:] in ('single', 'float'):
        kind, width = 'f4', 4
    elif ext[2:] == 'double':
        kind, width = 'f8', 8
    else:
        raise ValueError("Data type of phase file specified in file extension (\"%s\") not supported." % ext[2:])
    return endian, kind, width, folder, base, ext


def get_PGSE_from_phases(phasefile, sch_mat_sim, sch_mat, dim=None, D_sim=None, D=None, device=0):
    """PGSE signal for protocol ``sch_mat`` from the spins' phases of a reference Monte-Carlo run
    (ref:2813-3015; same arguments, checks and messages).  The phase files (one per gradient
    component, ``*_phase_x|y|z.<b|l><single|float|double>``) are staged to HBM as one plane per
    component -- no host-side interleaving -- and reduced there."""
    import os
    import torch
    names = ['x', 'y', 'z']
    MAXDIM = 3
    D_ratio_sqrt = 1.0
    if D is not None:
        if D_sim is None:
            raise NameError("Simulation diffusivity should be specified if new signal diffusivity is set.")
        D_ratio_sqrt = float(np.sqrt(D / D_sim))
    if dim is None:
        dim = MAXDIM
    elif dim > MAXDIM:
        raise ValueError("dim should be less than or equal to %d." % MAXDIM)
    sch_sim = import_PGSE_scheme(sch_mat_sim)
    sch = import_PGSE_scheme(sch_mat)
    if np.any(sch[:, dim:MAXDIM] != 0):
        print("WARNING get_PGSE_from_phases: detected non-zero entries in gradient components after dimension %d.\n"
              "Those components will be ignored but make sure the right acquisition protocol was provided.\n"
              "It is common for such protocols to contain zeros in those gradient components, for instance after "
              "projection into the xy-plane of a 3D protocol.\n" % dim)
    num_seq, num_ref = sch.shape[0], sch_sim.shape[0]
    g_sim = sch_sim[:, :3] * sch_sim[:, 3][:, np.newaxis]
    g_new = sch[:, :3] * sch[:, 3][:, np.newaxis]
    # each new sequence -> LAST simulated sequence with the same (Delta, delta) (ref:2874-2880)
    delta_mapping = np.full(num_seq, -1, dtype=np.int64)
    for i in range(num_ref):
        delta_mapping[np.all(sch[:, 4:6] == sch_sim[i, 4:6], axis=1)] = i
    bad = np.where(delta_mapping < 0)[0]
    if bad.size > 0:
        listing = '\n'.join('\t%4d -- %5g -- %5g' % (b, sch[b, 4] * 1e3, sch[b, 5] * 1e3) for b in bad)
        raise ValueError('Acquisition protocol contains %d (Delta,delta) pair(s) (out of %d) not used to simulate the '
                         'directional phases in the Monte Carlo simulation. List of unmatched sequences:\nSequ. no. '
                         '-- Delta [ms] -- delta [ms]\n%s' % (bad.size, num_seq, listing))
    with np.errstate(divide='ignore', invalid='ignore'):
        gscaling = np.ascontiguousarray(g_new[:, :dim] / g_sim[delta_mapping, :dim])
    if not os.path.isfile(phasefile):
        raise RuntimeError("File %s does not exist." % phasefile)
    nbytes = os.path.getsize(phasefile)
    endian, kind, width, folder, base, ext = _phase_file_format(phasefile)
    if nbytes % (num_ref * width) != 0:
        raise RuntimeError("Phase file %s is either corrupted or inconsistently named. Storage precision of items "
                           "(%d bytes) times number of reference simulation sequences (%d) does not divide total "
                           "size (%d bytes)." % (phasefile, width, num_ref, nbytes))
    num_entries = nbytes // width
    num_spins = num_entries // num_ref
    lib = L.lib()
    if lib.mfx_device_count() <= 0:
        raise L.MfxError("no HIP device available (this library has no CPU path)")
    dev = torch.device("cuda", int(device))
    planes = torch.empty((dim, num_entries), dtype=torch.float64, device=dev)     # one plane per component
    for i in range(dim):
        f_i = os.path.join(folder, base[:-len(names[i])] + names[i] + ext)
        if not os.path.isfile(f_i):
            raise RuntimeError("Phase file %s not found." % f_i)
        raw = np.fromfile(f_i, dtype=endian + kind, count=num_entries, sep="")
        planes[i].copy_(torch.from_numpy(raw.astype(np.float64)))
    out = np.zeros(num_seq)
    with torch.cuda.device(dev):
        st = torch.cuda.current_stream(dev)
        L.check(lib.mfx_monte_carlo_average_dev(planes.data_ptr(), num_entries, 1, num_entries, dim, L.lptr(delta_mapping),
                                                L.dptr(gscaling), D_ratio_sqrt, num_spins, num_seq, L.dptr(out),
                                                st.cuda_stream))
    return out


def loadmat(filename):
    """``scipy.io.loadmat`` with MATLAB structs converted to nested dicts (ref:3026-3087)."""
    import scipy.io
    try:
        from scipy.io.matlab import mat_struct
    except ImportError:  # older SciPy
        from scipy.io.matlab.mio5_params import mat_struct

    def conv(o):
        if isinstance(o, mat_struct):
            return {k: conv(v) for k, v in o.__dict__.items() if k != '_fieldnames'}
        return o

    data = scipy.io.loadmat(filename, struct_as_record=False, squeeze_me=True)
    return {k: conv(v) for k, v in data.items()}


def gen_SoS_MRI(S0, sigma_g, N=1, *, seed=None, device=0):
    """Simulates Sum-of-Squares MRI signal for phased-array systems (ref:2303-2354).

    Produces S_out = sqrt{ sum_{i=1}^N |S_i|^2 }, where S_i = S_0 + eps1 + (1i)*eps2, with eps1, eps2 two
    independent zero-mean Gaussian variables of standard deviation sigma_g, identical in all N coils and in both
    channels.  S_out follows a non-central Chi distribution (Rician for N = 1).

    Args:
      S0: N-D NumPy array with the true, real-valued MRI contrast (a complex S0 raises TypeError: the reference's
        arithmetic squares a complex in-phase term without taking its modulus and does not give the magnitude its
        docstring promises).  A torch CUDA tensor stays on its device: a new float64 tensor comes back, on torch's
        current stream, without a copy through the host (S0 itself is not changed; one that is not float64 and
        contiguous is converted first).
      sigma_g: scalar, or array with the shape of S0 (one standard deviation per entry).  Where an entry is 0
        beside others that are not, the result there is sqrt(N) |S0|, as the reference's arithmetic gives.  A sigma_g
        given as a tensor is not inspected on the host (that would wait for the device), so an all-zero tensor gives
        sqrt(N) |S0| too, where the all-zero early return below gives sqrt(N) S0, sign included.
      N: the effective number of coils.  Default is 1 (Rician noise).
      seed: None draws a 64-bit seed from NumPy's global generator (np.random.seed makes a script repeatable, as
        with the reference); an int makes the call reproducible by itself.  The draws are a Philox4x32-10 stream
        of this library and do not reproduce NumPy's: the distribution is the contract.
      device: GPU that draws for NumPy input.

    Returns:
      An array (or tensor) with the shape of S0; np.sqrt(N)*S0 when every sigma_g is 0.

    Raises:
      ValueError: if sigma_g is not a scalar but its shape does not match that of S0.
    """
    if type(S0).__module__.split('.')[0] == 'torch':
        import torch
        if S0.is_complex():
            raise TypeError("gen_SoS_MRI: S0 should be real-valued, got %s" % (S0.dtype,))
        if not torch.is_tensor(sigma_g) and np.ndim(sigma_g) == 0 and sigma_g == 0:
            return np.sqrt(N) * S0
        sg = sigma_g if torch.is_tensor(sigma_g) or np.ndim(sigma_g) == 0 else torch.as_tensor(np.asarray(sigma_g))
        if torch.is_tensor(sg) and sg.numel() > 1 and sg.shape != S0.shape:
            raise ValueError('sigma_g should either be a scalar or have the shape (%s) of S0 for 1-to-1 '
                             'correspondance. Detected (%s) instead.'
                             % (", ".join("%d" % x for x in S0.shape), ", ".join("%d" % x for x in sg.shape)))
        if not S0.is_cuda:
            raise TypeError("gen_SoS_MRI: a tensor S0 should live on the GPU (pass NumPy arrays otherwise)")
        if torch.is_tensor(sg) and sg.numel() > 1:
            sg = sg.reshape(S0.shape)
        return engine.sos_noise_dev(S0.to(torch.float64).contiguous(), sg, int(N), _sos_seed(seed))
    if np.iscomplexobj(S0) or np.iscomplexobj(sigma_g):
        raise TypeError("gen_SoS_MRI: S0 and sigma_g should be real-valued, got %s" % (np.asarray(S0).dtype,))
    if np.all(sigma_g == 0):
        return np.sqrt(N) * S0  # perfect noiseless scenario (ref:2332-2333)
    S0 = np.asarray(S0)
    if np.ndim(sigma_g) > 0 and sigma_g.size > 1 and S0.shape != sigma_g.shape:   # ref:2335-2343
        raise ValueError('sigma_g should either be a scalar or have '
                         'the shape (%s) of S0 for 1-to-1 '
                         'correspondance. Detected (%s) instead.'
                         % (", ".join("%d" % x for x in S0.shape),
                            ", ".join("%d" % x for x in sigma_g.shape)))
    if int(N) != N or N < 1:
        raise ValueError("N should be a positive integer, got %r" % (N,))
    sg = np.asarray(sigma_g, dtype=np.float64)
    out = engine.sos_noise(S0, sg.reshape(-1)[:1] if sg.size == 1 else sg, int(N), _sos_seed(seed), 0, device)
    # a sigma_g of shape (1, 1) beside an S0 of shape (N,) still gives shape (N,) (ref:2350-2353)
    return np.reshape(out, S0.shape)


def _is_torch(x):
    return type(x).__module__.split('.')[0] == 'torch'


def _property_levels(obj, values):
    """(levels, index of every atom's level, obj, torch or None) for the two profile helpers below."""
    values = np.asarray(values.cpu() if _is_torch(values) else values, dtype=np.float64).reshape(-1)
    if obj.shape[-1] != values.shape[0]:
        raise ValueError("obj has %d atoms along its last axis, values has %d" % (obj.shape[-1], values.shape[0]))
    if np.isnan(values).any():
        raise ValueError("values should not hold NaN")
    levels, inv = np.unique(values, return_inverse=True)
    return levels, np.asarray(inv).reshape(-1), values


def profile_by_property(obj, values):
    """An objective profile over atoms (``engine.profile``: obj [..., N]) as a function of one per-atom property
    (``values`` [N]: rad, fin, ... - the arrays named by the dictionary's ``fasc_propnames``).  Returns
    ``(levels, obj_by_level)``: the sorted distinct property values and, along a last axis of that length, the minimum
    of obj over the atoms at each level.  A row that holds NaN (a voxel class the profile does not serve) stays NaN.
    NumPy in, NumPy out; a torch tensor in, tensors out on its device."""
    levels, inv, _ = _property_levels(obj, values)
    if _is_torch(obj):
        import torch
        cols = [obj[..., torch.as_tensor(np.flatnonzero(inv == p), device=obj.device)].amin(dim=-1) for p in range(levels.size)]
        return torch.as_tensor(levels, device=obj.device), torch.stack(cols, dim=-1)
    obj = np.asarray(obj, dtype=np.float64)
    return levels, np.stack([obj[..., inv == p].min(axis=-1) for p in range(levels.size)], axis=-1)


def profile_interval(obj, values, rel=0.0, delta=0.0):
    """The range of a per-atom property that fits within a margin of the optimum: among the atoms with
    ``obj <= obj_min * (1 + rel) + delta`` (obj_min the minimum of obj [..., N] along its last axis) the smallest and
    the largest of ``values`` [N], and how many atoms that is: ``(lo, hi, count)`` of shape obj.shape[:-1].  NaN rows
    give lo = hi = NaN and count 0.  NumPy in, NumPy out; a torch tensor in, tensors out on its device."""
    if rel < 0 or delta < 0:
        raise ValueError("rel and delta should not be negative")
    _, _, values = _property_levels(obj, values)
    if _is_torch(obj):
        import torch
        v = torch.as_tensor(values, device=obj.device)
        bad = torch.isnan(obj).any(dim=-1, keepdim=True)
        omin = obj.amin(dim=-1, keepdim=True)
        sel = (obj <= omin * (1.0 + rel) + delta) & ~bad
        inf = torch.tensor(float('inf'), dtype=torch.float64, device=obj.device)
        lo = torch.where(sel, v, inf).amin(dim=-1)
        hi = torch.where(sel, v, -inf).amax(dim=-1)
        nan = torch.tensor(float('nan'), dtype=torch.float64, device=obj.device)
        return torch.where(bad[..., 0], nan, lo), torch.where(bad[..., 0], nan, hi), sel.sum(dim=-1)
    obj = np.asarray(obj, dtype=np.float64)
    bad = np.isnan(obj).any(axis=-1, keepdims=True)
    with np.errstate(invalid='ignore'):
        omin = obj.min(axis=-1, keepdims=True)
        sel = (obj <= omin * (1.0 + rel) + delta) & ~bad
    lo = np.where(sel, values, np.inf).min(axis=-1)
    hi = np.where(sel, values, -np.inf).max(axis=-1)
    return np.where(bad[..., 0], np.nan, lo), np.where(bad[..., 0], np.nan, hi), sel.sum(axis=-1)


def posterior_moments(w, values):
    """Mean and standard deviation of one per-atom property (``values`` [N]) under posterior weights over atoms
    (``engine.posterior``: w [..., N], each row summing to 1): ``(mean, std)`` of shape w.shape[:-1], std the square
    root of sum w (values - mean)^2.  A row that holds NaN (an absent fascicle, a voxel out of scope or with a non-zero
    status) gives NaN.  NumPy in, NumPy out; a torch tensor in, tensors out on its device."""
    _, _, values = _property_levels(w, values)
    if _is_torch(w):
        import torch
        v = torch.as_tensor(values, device=w.device)
        mean = (w * v).sum(dim=-1)
        return mean, torch.sqrt((w * (v - mean[..., None]) ** 2).sum(dim=-1))
    w = np.asarray(w, dtype=np.float64)
    mean = (w * values).sum(axis=-1)
    return mean, np.sqrt((w * (values - mean[..., None]) ** 2).sum(axis=-1))


def posterior_quantile(w, values, q):
    """The lower weighted quantile of a per-atom property under posterior weights w [..., N]: with the atoms sorted by
    value, the smallest value whose cumulative weight reaches ``q`` times the row's total (0 <= q <= 1).  NaN rows give
    NaN.  NumPy in, NumPy out; a torch tensor in, a tensor out on its device."""
    q = float(q)
    if not 0.0 <= q <= 1.0:
        raise ValueError("q should lie in [0, 1]")
    _, _, values = _property_levels(w, values)
    order = np.argsort(values, kind='stable')
    vs = values[order]
    if _is_torch(w):
        import torch
        c = torch.cumsum(w[..., torch.as_tensor(order, device=w.device)], dim=-1)
        reach = c >= q * c[..., -1:]
        first = torch.argmax(reach.to(torch.int8), dim=-1)      # the first True
        out = torch.as_tensor(vs, device=w.device)[first]
        return torch.where(reach.any(dim=-1), out, torch.full_like(out, float('nan')))
    w = np.asarray(w, dtype=np.float64)
    c = np.cumsum(w[..., order], axis=-1)
    with np.errstate(invalid='ignore'):
        reach = c >= q * c[..., -1:]
    return np.where(reach.any(axis=-1), vs[np.argmax(reach, axis=-1)], np.nan)


def posterior_by_property(w, values):
    """Posterior weights over atoms (w [..., N]) as a distribution over one per-atom property: ``(levels,
    weight_by_level)``, the sorted distinct property values and, along a last axis of that length, the sum of w over the
    atoms at each level - the counterpart of ``profile_by_property`` with sums in place of minima.  NaN rows stay NaN.
    NumPy in, NumPy out; a torch tensor in, tensors out on its device."""
    levels, inv, _ = _property_levels(w, values)
    if _is_torch(w):
        import torch
        cols = [w[..., torch.as_tensor(np.flatnonzero(inv == p), device=w.device)].sum(dim=-1) for p in range(levels.size)]
        return torch.as_tensor(levels, device=w.device), torch.stack(cols, dim=-1)
    w = np.asarray(w, dtype=np.float64)
    return levels, np.stack([w[..., inv == p].sum(axis=-1) for p in range(levels.size)], axis=-1)


def _sos_seed(seed):
    if seed is None:
        return int(np.random.randint(0, 2 ** 64, dtype=np.uint64))
    return int(seed) & ((1 << 64) - 1)
