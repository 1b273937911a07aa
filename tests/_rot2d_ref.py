"""Independent float64 referee for rotate_atom_2Dprotocol (reference mf_utils.py:1153-1202, 1440-1690).

A plain NumPy restatement of the reference's computation for one new fascicle direction, written from the
reference's description.  It imports nothing from the package under test: no tables, no plan arrays, no
rotate_scheme_mat.  It has the same standing as oracle/ and tests/_post_ref.py.

    R = Referee(sig, sch_mat, refdir, DIFF)      # the reference fascicle's side, once
    r = R.rotate(newdir)                         # Result: out [M, N] or None, error (type name, message) or None,
                                                 # clear, unclear (names of the decisions too close to call), margins
                                                 # (the gaps, and how many rows vanished / were extrapolated)

What the reference does, in its order:
  1. the scheme's gradient directions are rotated by the rotation that takes z onto the fascicle (axis z x d,
     angle -acos(z . d)); components of magnitude <= eps become 0, rows are renormalised; d parallel to z leaves
     the scheme as it is.  The first two components, normalised, are the row's perpendicular direction; their
     norm n gives G_perp = G n, and G_par = |g_z| G.  The reference normalises in place, so with refdir along z
     the new fascicle's side sees the scheme's first two columns already normalised.
  2. S_par = exp(-(gamma delta G_par)^2 (Delta - delta / 3) DIFF); S_perp_ref = sig / S_par_ref.
  3. per (Delta, delta) pair, in np.unique order: the unique perpendicular directions (exact comparison,
     lexicographic order) must number 3 or 5 on either side; opposite pairs are those with isclose(dot, -1).
  4. DW rows whose perpendicular component vanished take the pair's b0 signal (the mean over several b0 rows).
  5. per new line (opposite pair, in order; a row on two lines keeps the later one): signed abscissa
     G_perp sign(g_perp . line); the reference line is the one that holds the first arg-max of
     gdir_ref_un @ linedir_new; S_perp is interpolated linearly over the reference line's (stably sorted) signed
     G_perp with searchsorted(side='left') clipped to [1, P - 1], which extrapolates beyond the end knots.
  6. out = S_par_new * S_perp_new.

Clearance.  The device's acos / sin / cos / exp and its unfused dot products differ from the C library's and BLAS's
in the last bit.  A direction is "clear" when no decision of the new fascicle's side sits where such a
difference could turn it.  The bands, each stated as a factor or a gap (a term of the rotation has magnitude <= 1, so
one last-bit difference moves a rotated component by at most eps / 2; dot products of unit vectors and |d|^2 move
by a few eps):
  norm      ||d|^2 - 1| against isclose's 1e-8 + 1e-5: unclear within a gap of GAP_TOL = 1e-12 of the tolerance
  zeroing   every rotated component r against |r| <= eps: unclear when eps / 2 < |r| < 2 eps (a factor 2 either side)
  opposite  every dot of two unique directions against |dot + 1| <= 1e-8 + 1e-5: unclear within the factor
            1 +- 1e-6 of the tolerance
  chk_new   |G^2 - (G_perp^2 + G_par^2)| against 1e-8 + 1e-5 (G_perp^2 + G_par^2), and
  chk_par   |S_par - 1| on b0 rows against 1e-8 + 1e-5: unclear within a factor 2 of the tolerance
  argmax    largest minus second-largest entry of gdir_ref_un @ linedir_new: unclear below a gap of GAP_DOT = 1e-12
  knot      an abscissa within the factor 1 +- 1e-12 of a repeated knot (the only knots where the two neighbouring
            intervals' values differ: linear interpolation is continuous at a simple knot), or beyond a repeated
            end knot, where the clipped interval has zero width
A direction that is not clear is still a valid input; it is only left out of value and status comparisons.
"""
import numpy as np

EPS = float(np.finfo(np.float64).eps)
GAMMA = 2 * np.pi * 42.577480e6          # 1H, rad / (s T), the reference's get_gyromagnetic_ratio('H')
ISCLOSE_RTOL, ISCLOSE_ATOL = 1e-5, 1e-8
GAP_TOL = 1e-12
GAP_DOT = 1e-12
BAND_OPPOSITE = 1e-6
BAND_KNOT = 1e-12

MSG_NORM = "cyldir1 and cyldir2 should have unit norm."
MSG_CHK_NEW = "Inconsistency in parallel and perpendicular gradient components for new fascicle."
MSG_CHK_PAR_NEW = "New fascicle: parallel signal should  be equal to 1 in b0 sequences."


class Result:
    def __init__(self, out, error, unclear, margins):
        self.out, self.error, self.unclear, self.margins = out, error, unclear, margins
        self.clear = not unclear

    @property
    def ok(self):
        return self.error is None


def _isclose(a, b):
    return np.abs(a - b) <= ISCLOSE_ATOL + ISCLOSE_RTOL * np.abs(b)


def _rotation(d):
    """Matrix of the rotation about z x d by -acos(z . d) (Rodrigues), or None when d is parallel to z."""
    ax = np.array([-d[1], d[0], 0.0])                    # z x d
    sq = ax[0] * ax[0] + ax[1] * ax[1] + ax[2] * ax[2]
    if not sq > 0:
        return None
    x, y, z = ax / np.sqrt(sq)
    th = -np.arccos(d[2])
    s, c = np.sin(th), np.cos(th)
    t = 1 - c
    return np.array([[t * x * x + c, t * x * y - s * z, t * x * z + s * y],
                     [t * x * y + s * z, t * y * y + c, t * y * z - s * x],
                     [t * x * z - s * y, t * y * z + s * x, t * z * z + c]])


def _effective_scheme(g, d):
    """(rotated unit gradient directions [M, 3], the components before zeroing or None).  Without a rotation the
    array itself comes back, as in the reference, so that the caller's in-place normalisation reaches it."""
    R = _rotation(d)
    if R is None:
        return g, None
    raw = np.stack([g[:, 0] * R[k, 0] + g[:, 1] * R[k, 1] + g[:, 2] * R[k, 2] for k in range(3)], axis=1)
    r = raw.copy()
    r[np.abs(r) <= EPS] = 0.0
    n = np.sqrt(r[:, 0] ** 2 + r[:, 1] ** 2 + r[:, 2] ** 2)
    nz = n > 0
    r[nz] = r[nz] / n[nz, None]
    return r, raw


def _perp(g_eff):
    """normalises the first two columns of g_eff in place; returns their norm before that"""
    n = np.sqrt(g_eff[:, 0] ** 2 + g_eff[:, 1] ** 2)
    nz = n > 0
    g_eff[nz, 0:2] = g_eff[nz, 0:2] / n[nz, None]
    return n


def _unique_rows(v):
    """np.unique(v, axis=0, return_inverse=True) for [n, 2]: lexicographic, -0.0 == 0.0"""
    order = np.lexsort((v[:, 1], v[:, 0]))
    s = v[order]
    new = np.ones(s.shape[0], dtype=bool)
    new[1:] = (s[1:, 0] != s[:-1, 0]) | (s[1:, 1] != s[:-1, 1])
    inv = np.empty(s.shape[0], dtype=np.int64)
    inv[order] = np.cumsum(new) - 1
    return s[new], inv


def _opposite(un):
    """[(i, j)] in row-major order with isclose(un_i . un_j, -1), and all the dots"""
    dots = un[:, 0][:, None] * un[:, 0][None, :] + un[:, 1][:, None] * un[:, 1][None, :]
    ii, jj = np.where(_isclose(dots, -1.0))
    return list(zip(ii.tolist(), jj.tolist())), dots


class Referee:
    def __init__(self, sig, sch_mat, refdir, DIFF):
        sig = np.array(sig, dtype=np.float64)
        self.sig = sig[:, None] if sig.ndim == 1 else sig
        sch = np.array(sch_mat, dtype=np.float64)
        refdir = np.array(refdir, dtype=np.float64)
        if np.any(sch[:, 2] != 0) or self.sig.shape[0] != sch.shape[0]:
            raise ValueError("referee: gz must be zero and sig must have one row per protocol row")
        if not _isclose(np.sum(refdir ** 2), 1.0):
            raise ValueError(MSG_NORM)
        self.M, self.N = self.sig.shape
        self.DIFF = float(DIFF)
        self.G, self.Delta, self.delta = sch[:, 3].copy(), sch[:, 4].copy(), sch[:, 5].copy()
        self.is_b0 = self.G == 0
        # self.g is what the new fascicle's side sees: normalised in place when refdir is along z
        self.g = sch[:, 0:3].copy()
        g_ref, _ = _effective_scheme(self.g, refdir)
        n_ref = _perp(g_ref)
        self.gperp_ref = g_ref[:, 0:2].copy()
        self.Gperp_ref = self.G * n_ref
        Gpar_ref = np.abs(g_ref[:, 2]) * self.G
        if not np.all(_isclose(self.G ** 2, self.Gperp_ref ** 2 + Gpar_ref ** 2)):
            raise AssertionError("Inconsistency in parallel and perpendicular gradient components for reference fasicle.")
        self.Spar_ref = np.exp(-((GAMMA * self.delta * Gpar_ref) ** 2 * (self.Delta - self.delta / 3)) * self.DIFF)
        if not np.all(_isclose(self.Spar_ref[self.is_b0], 1.0)):
            raise AssertionError("Reference fascicle: parallel signal should  be one in b0 sequences.")
        self.Sperp_ref = self.sig / self.Spar_ref[:, None]
        # (Delta, delta) pairs in lexicographic order
        keys = sorted({(a, b) for a, b in zip(self.Delta.tolist(), self.delta.tolist())})
        self.pairs = [np.where((self.Delta == a) & (self.delta == b))[0] for a, b in keys]
        self.P = len(self.pairs)
        self.ref_side = [self._reference_pair(rows) for rows in self.pairs]

    def _reference_pair(self, rows):
        un, inv = _unique_rows(self.gperp_ref[rows])
        if un.shape[0] not in (3, 5):
            return dict(error="unique", n=un.shape[0])
        opp, _ = _opposite(un)
        if len(opp) not in (2, 4):
            return dict(error="pairs", n=len(opp))
        return dict(error=None, un=un, inv=inv, opp=opp, tables={})

    def _table(self, p, u):
        """the sorted knots of the reference line that holds unique direction u of pair p: (x [K], y [K, N])"""
        side = self.ref_side[p]
        if u not in side["tables"]:
            i, j = next(o for o in side["opp"] if o[0] == u)
            rows = self.pairs[p][(side["inv"] == i) | (side["inv"] == j)]
            dots = self.gperp_ref[rows, 0] * side["un"][u, 0] + self.gperp_ref[rows, 1] * side["un"][u, 1]
            x = self.Gperp_ref[rows] * np.sign(dots)
            order = np.argsort(x, kind="stable")
            side["tables"][u] = (x[order], self.Sperp_ref[rows][order])
        return side["tables"][u]

    def rotate(self, newdir):
        d = np.array(newdir, dtype=np.float64).reshape(3)
        unclear, margins = [], {}

        def fail(kind, msg):
            return Result(None, (kind, msg), unclear, margins)

        def band(name, flag):
            if flag and name not in unclear:
                unclear.append(name)

        nsq = float(np.sum(d ** 2))
        tol1 = ISCLOSE_ATOL + ISCLOSE_RTOL
        margins["norm"] = abs(abs(nsq - 1.0) - tol1)
        band("norm", margins["norm"] < GAP_TOL)
        if not _isclose(nsq, 1.0):
            return fail("ValueError", MSG_NORM)
        g_new, raw = _effective_scheme(self.g.copy(), d)
        if raw is not None:
            a = np.abs(raw)
            band("zeroing", bool(np.any((a > EPS / 2) & (a < 2 * EPS))))
        n_new = _perp(g_new)
        gperp = g_new[:, 0:2]
        Gperp = self.G * n_new
        Gpar = np.abs(g_new[:, 2]) * self.G
        rhs = Gperp ** 2 + Gpar ** 2
        dev, tol = np.abs(self.G ** 2 - rhs), ISCLOSE_ATOL + ISCLOSE_RTOL * np.abs(rhs)
        band("chk_new", bool(np.any((dev > tol / 2) & (dev < 2 * tol))))
        if np.any(dev > tol):
            return fail("AssertionError", MSG_CHK_NEW)
        Spar = np.exp(-((GAMMA * self.delta * Gpar) ** 2 * (self.Delta - self.delta / 3)) * self.DIFF)
        dev = np.abs(Spar[self.is_b0] - 1.0)
        band("chk_par", bool(np.any((dev > tol1 / 2) & (dev < 2 * tol1))))
        if np.any(dev > tol1):
            return fail("AssertionError", MSG_CHK_PAR_NEW)
        Sperp = np.zeros((self.M, self.N))
        Sperp[self.is_b0] = self.sig[self.is_b0]
        vanished = (~(n_new > 0)) & ~self.is_b0
        P = self.P
        margins["opposite"], margins["argmax"], margins["knot"] = np.inf, np.inf, np.inf
        margins["vanished"], margins["extrapolated"] = int(vanished.sum()), 0
        for p, rows in enumerate(self.pairs):
            side = self.ref_side[p]
            if side["error"] == "unique":
                return fail("AssertionError", "Problem at delta pair %d/%d: found %d unique gradient directions in plane "
                            "perpendicular to reference fascicle (including b0 zero dirs)." % (p + 1, P, side["n"]))
            if side["error"] == "pairs":
                return fail("AssertionError", "Problem at delta pair %d/%d: found %d instead of 4 (2x2, redundant) pairs "
                            "of opposite directions in plane perpendicular to reference fascicle." % (p + 1, P, side["n"]))
            un, inv = _unique_rows(gperp[rows])
            if un.shape[0] not in (3, 5):
                return fail("AssertionError", "Problem at delta pair %d/%d: found %d unique gradient directions in plane "
                            "perpendicular to new fascicle (including b0 zero dirs)." % (p + 1, P, un.shape[0]))
            opp, dots = _opposite(un)
            off = np.abs(np.abs(dots + 1.0) / tol1 - 1.0)
            margins["opposite"] = min(margins["opposite"], float(off.min()))
            band("opposite", bool(off.min() < BAND_OPPOSITE))
            lines = [(i, j) for i, j in opp if i < j]
            if len(lines) not in (1, 2):
                return fail("AssertionError", "Problem at delta pair %d/%d: found %d instead of 2 pairs of opposite "
                            "directions, in plane  perpendicular to new fascicle." % (p + 1, P, len(lines)))
            van = rows[vanished[rows]]
            b0 = rows[self.is_b0[rows]]
            if van.size:
                if b0.size == 0:
                    return fail("AssertionError", "Shell %d/%d: some new line directions are completely parallel to new "
                                "fascicle, implying free diffusion. However, no b0 measurements in the reference signal "
                                "are available for this shell. We therefore can't properly scale the new signal."
                                % (p + 1, P))
                Sperp[van] = self.sig[b0[0]] if b0.size == 1 else np.mean(self.sig[b0], axis=0)
            for l, (i, j) in enumerate(lines):
                line = un[i]
                sel = rows[(inv == i) | (inv == j)]
                if np.any(self.is_b0[sel]):
                    return fail("AssertionError", "Problem at delta pair %d/%d, new line direction %d/%d: trying to "
                                "interpolate b0 sequences." % (p + 1, P, l, len(lines)))
                x_new = Gperp[sel] * np.sign(gperp[sel, 0] * line[0] + gperp[sel, 1] * line[1])
                score = side["un"][:, 0] * line[0] + side["un"][:, 1] * line[1]
                u = int(np.argmax(score))
                top = np.sort(score)
                margins["argmax"] = min(margins["argmax"], float(top[-1] - top[-2]))
                band("argmax", bool(top[-1] - top[-2] < GAP_DOT))
                hits = sum(1 for o in side["opp"] if o[0] == u)
                if hits != 1:
                    return fail("ValueError", "operands could not be broadcast together with shapes (%d,) (%d,) "
                                % (rows.size, hits))
                kx, ky = self._table(p, u)
                K = kx.shape[0]
                hi = np.clip(np.searchsorted(kx, x_new, side="left"), 1, K - 1)
                lo = hi - 1
                slope = (ky[hi] - ky[lo]) / (kx[hi] - kx[lo])[:, None]
                Sperp[sel] = slope * (x_new - kx[lo])[:, None] + ky[lo]
                margins["extrapolated"] += int(np.sum((x_new < kx[0]) | (x_new > kx[-1])))
                # knots where the neighbouring intervals' values differ: repeated ones
                rep = np.zeros(K, dtype=bool)
                same = kx[1:] == kx[:-1]
                rep[1:] |= same
                rep[:-1] |= same
                if np.any(rep):
                    kr = kx[rep]
                    rel = np.abs(x_new[:, None] - kr[None, :]) / np.maximum(np.abs(kr[None, :]), 1e-300)
                    margins["knot"] = min(margins["knot"], float(rel.min()))
                    band("knot", bool(rel.min() < BAND_KNOT) or bool(np.any(kx[hi] == kx[lo])))
        return Result(Spar[:, None] * Sperp, None, unclear, margins)
