"""Thin object layer over the C ABI: device tables, protocol plans, batched fit."""
import ctypes as C

import numpy as np

from . import _lib as L
from . import nifti


class DeviceTables:
    """Per-shell knot tables resident in HBM (mfx_tables)."""

    def __init__(self, xs, Ys, G_un, device=0):
        self.xs = [np.ascontiguousarray(x, dtype=np.float64) for x in xs]
        self.Ys = [np.ascontiguousarray(y, dtype=np.float64) for y in Ys]
        self.G_un = np.ascontiguousarray(G_un, dtype=np.float64)
        self.N = int(self.Ys[0].shape[1])
        self.S = len(self.xs)
        self.device = device
        self._h = None
        self.off = np.concatenate([[0], np.cumsum([x.size for x in self.xs])]).astype(np.int32)

    def handle(self):
        if self._h is None:
            x = np.ascontiguousarray(np.concatenate(self.xs))
            Y = np.ascontiguousarray(np.concatenate(self.Ys, axis=0))
            h = C.c_void_p()
            L.check(L.lib().mfx_tables_create(L.dptr(x), L.iptr(self.off), L.dptr(Y), L.dptr(self.G_un), self.S,
                                             self.N, self.device, C.byref(h)))
            self._h = h
        return self._h

    def close(self):
        if self._h is not None:
            L.lib().mfx_tables_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Plan:
    """Per-protocol row->shell mapping resident in HBM (mfx_plan)."""

    def __init__(self, tables, scheme=None, gdirs=None, shell_of_row=None):
        self.tables = tables
        self.scheme = None          # the [M x 7] scheme of a multi-shell plan (boot_groups reads it)
        h = C.c_void_p()
        if scheme is not None:
            sch = L.f64c(scheme)
            if sch.ndim != 2 or sch.shape[1] != 7:
                raise ValueError("pgse_scheme should have 7 columns")
            self.M = sch.shape[0]
            self.scheme = sch
            L.check(L.lib().mfx_plan_create_multishell(tables.handle(), L.dptr(sch), self.M, C.byref(h)))
        else:
            g = L.f64c(gdirs)
            s = np.ascontiguousarray(shell_of_row, dtype=np.int32)
            self.M = g.shape[0]
            L.check(L.lib().mfx_plan_create_explicit(tables.handle(), L.dptr(g), L.iptr(s), self.M, C.byref(h)))
        self._h = h

    def handle(self):
        return self._h

    def close(self):
        if self._h is not None:
            L.lib().mfx_plan_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def num_params(maxfasc, csf_on, ear_on):
    return 1 + 2 * maxfasc + int(csf_on) + 2 * int(ear_on) + 2   # mf.py:381


# ---- argument and marshalling plumbing shared by the entry points below (all of it runs before any device call)
def _f64_cuda(*tensors):
    """Asserts that every tensor given (None: an absent optional one) is a contiguous CUDA float64 tensor."""
    import torch
    for t in tensors:
        assert t is None or (t.is_cuda and t.dtype == torch.float64 and t.is_contiguous())


def _out_like(out, shape, dev):
    """The output tensor of a device entry point: ``out`` if the caller gave one, else a new one; asserted either way."""
    import torch
    if out is None:
        out = torch.empty(shape, dtype=torch.float64, device=dev)
    assert out.is_cuda and out.dtype == torch.float64 and out.is_contiguous() and tuple(out.shape) == tuple(shape)
    return out


def _tptr(t):
    """The device pointer of an optional tensor (None: a null pointer)."""
    return t.data_ptr() if t is not None else None


def _w_stride(M, V, w_shape):
    """w_stride of measurement weights: M for [V, M], 0 for one [M] vector shared by the voxels."""
    if tuple(w_shape) == (M,):
        return 0
    if tuple(w_shape) == (V, M):
        return M
    raise ValueError("weights should have shape (%d, %d) or (%d,), got %s (%d voxels)" % (V, M, M, tuple(w_shape), V))


def _host_weights(M, V, W):
    """Optional NumPy weights of a host entry point: (float64 array or None, w_stride)."""
    if W is None:
        return None, 0
    W = L.f64c(W)
    return W, _w_stride(M, V, W.shape)


def _w_chunk(W, w_stride, ix):
    """The weights of the voxels ``ix`` of a class: their rows of [V, M] weights, the shared [M] vector as it is."""
    return np.ascontiguousarray(W[ix]) if W is not None and w_stride else W


def _twin(name, h, Y, W, w_stride, *rest):
    """One C call from one argument list: ``mfx_<name>(h, Y, *rest)``, or with weights its twin ``mfx_w<name>(h, Y, W,
    w_stride, *rest)`` (include/mfx_wsoft.h, include/mfx_w2d.h).  Y and W are pointers, W None without weights."""
    if W is None:
        L.check(getattr(L.lib(), "mfx_" + name)(h, Y, *rest))
    else:
        L.check(getattr(L.lib(), "mfx_w" + name)(h, Y, W, w_stride, *rest))


def _k_arg(V, maxfasc, K):
    """Per-voxel fascicle counts as int32 [V], each in 0..maxfasc."""
    K = np.ascontiguousarray(np.asarray(K).reshape(-1), dtype=np.int32)
    if K.shape != (V,):
        raise ValueError("K should have one entry per voxel")
    if V and (K.min() < 0 or K.max() > maxfasc):
        raise ValueError("K should lie in 0..maxfasc = %d" % maxfasc)
    return K


def _mixed_args(M, V, maxfasc, K, csf, csf_on, sig_csf, need_sig=False):
    """The per-voxel arguments of a mixed-batch fit: (K int32 [V], csf uint8 [V] or None, sig_csf float64 [M] or None).
    ``need_sig``: csf_on alone, without a flagged voxel, already asks for sig_csf (the robust fits predict with it)."""
    K = _k_arg(V, maxfasc, K)
    cs = None
    if csf is not None:
        cs = np.ascontiguousarray(np.asarray(csf).reshape(-1).astype(bool), dtype=np.uint8)
        if cs.shape != (V,):
            raise ValueError("csf should have one entry per voxel")
    sc = L.f64c(sig_csf).reshape(-1) if sig_csf is not None else None
    if cs is not None and np.any(cs) and (not csf_on or sc is None):
        raise ValueError("voxels flagged CSF need csf_on and sig_csf")
    if need_sig and csf_on and sc is None:
        raise ValueError("csf_on needs sig_csf")
    if sc is not None and sc.shape[0] != M:
        raise ValueError("sig_csf has %d entries, protocol has %d" % (sc.shape[0], M))
    return K, cs, sc


def _batch_args(V, K, csf, ear, peaks, maxfasc, csf_on, ear_on, sig_csf, sig_ear):
    """The per-voxel arguments of fit_batch and fit_batch_volume and their output: (K, csf, ear, peaks, out, sig_csf,
    sig_ear)."""
    K = np.ascontiguousarray(K, dtype=np.int32)
    if K.shape[0] != V:
        raise ValueError("K should have one entry per voxel")
    csf_a = np.ascontiguousarray(csf, dtype=np.uint8) if csf is not None else np.zeros(V, np.uint8)
    ear_a = np.ascontiguousarray(ear, dtype=np.uint8) if ear is not None else np.zeros(V, np.uint8)
    pk = L.f64c(peaks).reshape(V, -1) if maxfasc > 0 else np.zeros((V, 3))
    if maxfasc > 0 and pk.shape[1] != 3 * maxfasc:
        raise ValueError("peaks should have %d columns" % (3 * maxfasc))
    out = np.zeros((V, num_params(maxfasc, csf_on, ear_on)))
    return K, csf_a, ear_a, pk, out, L.f64c_opt(sig_csf), L.f64c_opt(sig_ear)


class FileOrderVolume(object):
    """A 4-D data volume in the layout NIfTI files (and nibabel's arrays) have: ``array`` is Fortran-contiguous with
    shape (..., M), i.e. one 3-D image per measurement, in one of the scalar types of ``NIFTI_CODES``; ``slope`` /
    ``inter`` are the header's scaling (slope 0: none).  ``get_fdata()`` gives what nib.load(f).get_fdata() would."""
    NIFTI_CODES = {'u1': 2, 'i2': 4, 'i4': 8, 'f4': 16, 'f8': 64, 'i1': 256, 'u2': 512, 'u4': 768}

    def __init__(self, array, slope=0.0, inter=0.0):
        self.array, self.slope, self.inter = array, float(slope), float(inter)
        self.shape = array.shape

    @staticmethod
    def accepts(a):
        return (isinstance(a, np.ndarray) and a.ndim >= 2 and a.flags.f_contiguous and not a.flags.c_contiguous
                and a.dtype.isnative and a.dtype.str[1:] in FileOrderVolume.NIFTI_CODES)

    @property
    def scaled(self):
        return nifti._scaled(self.slope, self.inter)

    def get_fdata(self):
        d = self.array.astype(np.float64)
        return d * self.slope + self.inter if self.scaled else d

    def file_order_index(self, c_flat_index):
        """Positions inside one 3-D image of the voxels with C-order flat indices ``c_flat_index`` of the image grid."""
        grid = self.shape[:-1]
        return np.ravel_multi_index(np.unravel_index(c_flat_index, grid), grid, order='F').astype(np.int64)


def volume_rows(vol, vox, device=0):
    """mfx_volume_rows: ``vol.get_fdata().reshape(-1, n, order='F')[vox]`` (float64 [V x n]) with the conversion, scaling
    and gather on the device - for the per-voxel quantities MFModel.fit indexes with the mask beside the data."""
    a = vol.array
    n = a.shape[-1]
    nvox = int(np.prod(a.shape[:-1]))
    vox = np.ascontiguousarray(vox, dtype=np.int64)
    V = vox.shape[0]
    if V and (vox.min() < 0 or vox.max() >= nvox):
        raise ValueError("voxel indices out of range")
    out = np.zeros((V, n))
    L.check(L.lib().mfx_volume_rows(a.ctypes.data, FileOrderVolume.NIFTI_CODES[a.dtype.str[1:]], vol.slope, vol.inter, nvox, n,
                                    L.lptr(vox), V, L.dptr(out), int(device)))
    return out


def fit_batch_volume(plan, vol, vox, K, csf, ear, peaks, maxfasc, csf_on, ear_on, sig_csf=None, sig_ear=None, E=0):
    """mfx_fit_batch_volume: like ``fit_batch(plan, vol.get_fdata().reshape(-1, M, order='F')[vox], ...)`` with the
    volume uploaded in its own layout and type and the conversion, scaling and ROI gather (mf.py:623-657) on the device."""
    a = vol.array
    M = a.shape[-1]
    if M != plan.M:
        raise ValueError("data has %d measurements, protocol has %d" % (M, plan.M))
    nvox = int(np.prod(a.shape[:-1]))
    vox = np.ascontiguousarray(vox, dtype=np.int64)
    V = vox.shape[0]
    if V and (vox.min() < 0 or vox.max() >= nvox):
        raise ValueError("voxel indices out of range")
    K, csf_a, ear_a, pk, out, sc, se = _batch_args(V, K, csf, ear, peaks, maxfasc, csf_on, ear_on, sig_csf, sig_ear)
    L.check(L.lib().mfx_fit_batch_volume(plan.handle(), a.ctypes.data, FileOrderVolume.NIFTI_CODES[a.dtype.str[1:]],
                                         vol.slope, vol.inter, nvox, L.lptr(vox), L.iptr(K), L.bptr(csf_a), L.bptr(ear_a),
                                         L.dptr(pk), int(maxfasc), int(csf_on), int(ear_on), L.opt(sc), L.opt(se), int(E), V,
                                         L.dptr(out)))
    return out


def fit_batch(plan, Y, K, csf, ear, peaks, maxfasc, csf_on, ear_on, sig_csf=None, sig_ear=None, E=0, rows=None):
    """Host-buffer voxel loop (mfx_fit_batch_rows): returns params_in_mask [V x num_params] (mf.py:1018-1028).

    ``rows`` (int64 [V], optional): voxel v's signal is ``Y[rows[v]]`` -- the ROI gather ``data[mask > 0]`` of the
    reference (mf.py:644) done by the library while it stages the upload; Y then is the whole [n_vox_total x M] volume."""
    Y = L.f64c(Y)
    if Y.ndim != 2:
        raise ValueError("Y should be a 2-D array [voxels x measurements]")
    M = Y.shape[1]
    if rows is not None:
        rows = np.ascontiguousarray(rows, dtype=np.int64)
        V = rows.shape[0]
        if V and (rows.min() < 0 or rows.max() >= Y.shape[0]):
            raise ValueError("rows out of range")
    else:
        V = Y.shape[0]
    if M != plan.M:
        raise ValueError("data has %d measurements, protocol has %d" % (M, plan.M))
    K, csf_a, ear_a, pk, out, sc, se = _batch_args(V, K, csf, ear, peaks, maxfasc, csf_on, ear_on, sig_csf, sig_ear)
    L.check(L.lib().mfx_fit_batch_rows(plan.handle(), L.dptr(Y), L.opt(rows, L.lptr), L.iptr(K), L.bptr(csf_a), L.bptr(ear_a),
                                       L.dptr(pk), int(maxfasc), int(csf_on), int(ear_on), L.opt(sc), L.opt(se), int(E), V,
                                       L.dptr(out)))
    return out


def fit_batch_dev(plan, d_Y, d_peaks, maxfasc, csf_on=False, ear_on=False, d_sig_csf=None, d_sig_ear=None, E=0,
                  out=None, check=True):
    """Device-resident voxel loop (mfx_fit_batch_dev) on torch CUDA tensors of ONE voxel class (every voxel:
    K == maxfasc, csf == csf_on, ear == ear_on).  Enqueues on torch's current stream and returns the [V x num_params]
    output tensor without waiting; ``check=True`` then waits and raises what the kernels flagged (a fascicle
    direction that is not a unit vector: the reference's per-voxel ValueError, mf_utils.py:1798-1802)."""
    import torch
    _f64_cuda(d_Y)
    V = d_Y.shape[0]
    if d_Y.shape[1] != plan.M:
        raise ValueError("data has %d measurements, protocol has %d" % (d_Y.shape[1], plan.M))
    if maxfasc > 0:
        _f64_cuda(d_peaks)
        if tuple(d_peaks.shape) != (V, 3 * maxfasc):
            raise ValueError("peaks should have shape (%d, %d)" % (V, 3 * maxfasc))
    if out is None:
        out = torch.zeros((V, num_params(maxfasc, csf_on, ear_on)), dtype=torch.float64, device=d_Y.device)
    st = torch.cuda.current_stream(d_Y.device).cuda_stream
    L.check(L.lib().mfx_fit_batch_dev(plan.handle(), d_Y.data_ptr(), d_peaks.data_ptr() if maxfasc > 0 else None,
                                      int(maxfasc), int(bool(csf_on)), int(bool(ear_on)), _tptr(d_sig_csf), _tptr(d_sig_ear),
                                      int(E), V, out.data_ptr(), st))
    if check:
        L.check(L.lib().mfx_plan_status(plan.handle(), st))
    return out


def rotate_columns_dev(plan, d_dirs, d_cols, normalise=False):
    """Device-resident single-atom rotation: torch CUDA tensors dirs [B,3] f64, cols [B] i32 -> [B,M] f64."""
    import torch
    _f64_cuda(d_dirs)
    cols = d_cols.to(torch.int32).contiguous()
    B = d_dirs.shape[0]
    out = torch.empty((B, plan.M), dtype=torch.float64, device=d_dirs.device)
    st = torch.cuda.current_stream(d_dirs.device).cuda_stream
    L.check(L.lib().mfx_rotate_cols_dev(plan.handle(), d_dirs.data_ptr(), cols.data_ptr(), B, int(normalise),
                                        out.data_ptr(), st))
    return out


SIGMA_SCALAR, SIGMA_VOXEL, SIGMA_ELEMENT = 0, 1, 2   # include/mfx_predict.h
_U64 = (1 << 64) - 1


def _predict_shapes(plan, p_shape, pk_shape, maxfasc, csf_on, ear_on, y_shape, M_csf, ear_shape, E):
    """Argument checks shared by predict and predict_dev (before any device call); returns V."""
    maxfasc = int(maxfasc)
    if maxfasc < 0 or maxfasc > 3:
        raise ValueError("maxfasc must be 0..3")
    npar = num_params(maxfasc, csf_on, ear_on)
    if len(p_shape) != 2 or p_shape[1] != npar:
        raise ValueError("params should have %d columns (maxfasc = %d, csf_on = %s, ear_on = %s), got shape %s"
                         % (npar, maxfasc, bool(csf_on), bool(ear_on), tuple(p_shape)))
    V = p_shape[0]
    if maxfasc > 0 and (pk_shape is None or tuple(pk_shape) != (V, 3 * maxfasc)):
        raise ValueError("peaks should have shape (%d, %d)" % (V, 3 * maxfasc))
    if csf_on and M_csf != plan.M:
        raise ValueError("sig_csf has %s entries, protocol has %d" % (M_csf, plan.M))
    if ear_on and (ear_shape is None or tuple(ear_shape) != (plan.M, E) or E < 1):
        raise ValueError("sig_ear should have shape (%d, E) with E >= 1" % plan.M)
    if y_shape is not None and tuple(y_shape) != (V, plan.M):
        raise ValueError("data has shape %s, protocol has %d measurements for %d voxels" % (tuple(y_shape), plan.M, V))
    return V


def _sigma_mode(shape, numel, V, M, what="sigma_g"):
    if numel == 1:
        return SIGMA_SCALAR
    if tuple(shape) == (V, M):
        return SIGMA_ELEMENT
    if tuple(shape) in ((V,), (V, 1)):
        return SIGMA_VOXEL
    raise ValueError("%s should be a scalar, one value per voxel (%d) or one per element (%d, %d), got shape %s"
                     % (what, V, V, M, tuple(shape)))


def predict_bad_rows(params, maxfasc, csf_on, ear_on, N, E):
    """bool [V]: the rows of params [V x num_params] that predict refuses - a weight M0 * nu that is negative or not
    finite, or, beside a positive weight, an atom index that is not an integer in [0, N) (fascicles) or [0, E) (EAR).
    The same rule as the library's (csrc/predict.hip), for callers that want to set such rows aside first."""
    P = np.asarray(params, dtype=np.float64)
    F = int(maxfasc)
    cols = [(1 + k, 1 + F + k, N) for k in range(F)]
    if csf_on:
        cols.append((1 + 2 * F, None, 0))
    if ear_on:
        cols.append((1 + 2 * F + int(bool(csf_on)), 2 + 2 * F + int(bool(csf_on)), E))
    bad = np.zeros(P.shape[0], dtype=bool)
    with np.errstate(invalid='ignore', over='ignore'):
        for iw, iid, lim in cols:
            w = P[:, 0] * P[:, iw]
            bad |= ~(w >= 0) | np.isinf(w)
            if iid is not None:
                i = P[:, iid]
                bad |= (w > 0) & ~((i >= 0) & (i < lim) & (i == np.floor(i)))
    return bad


def predict_dev(plan, d_params, d_peaks, maxfasc, csf_on=False, ear_on=False, d_sig_csf=None, d_sig_ear=None, E=0,
                d_Y=None, sigma_g=None, ncoils=0, seed=0, offset=0, out=None, check=True):
    """Forward model on the device (mfx_predict_dev): parameter rows [V x num_params] in the layout fit_batch_dev
    returns and peaks [V x 3 maxfasc] (torch CUDA float64 tensors) -> the signal [V x M] they stand for.  With
    ``ncoils`` > 0 the magnitude noise of ``sos_noise_dev`` is applied in the same pass, ``sigma_g`` a number or a
    tensor with one value, one per voxel or one per element; element (v, m) draws with index ``offset + v M + m``.
    With ``d_Y`` [V x M] the per-voxel residual sum of squares and R2 come back too: ``(out, stats [V x 2])``.
    Enqueues on torch's current stream; ``check=True`` then waits and raises the ValueError of a bad atom index or
    weight (that voxel's row is NaN) or of a direction that is not a unit vector."""
    import torch
    d_peaks, d_sig_csf, d_sig_ear = d_peaks if maxfasc > 0 else None, d_sig_csf if csf_on else None, d_sig_ear if ear_on else None
    _f64_cuda(d_params, d_peaks, d_sig_csf, d_sig_ear, d_Y)
    dev = d_params.device
    V = _predict_shapes(plan, d_params.shape, d_peaks.shape if maxfasc > 0 else None, maxfasc, csf_on, ear_on,
                        d_Y.shape if d_Y is not None else None, d_sig_csf.numel() if csf_on else None,
                        d_sig_ear.shape if ear_on else None, E)
    M = plan.M
    mode, d_sigma = SIGMA_SCALAR, None
    if ncoils:
        if sigma_g is None:
            raise ValueError("noise (ncoils > 0) needs sigma_g")
        d_sigma = (sigma_g.to(device=dev, dtype=torch.float64).contiguous() if torch.is_tensor(sigma_g)
                   else torch.full((1,), float(sigma_g), dtype=torch.float64, device=dev))
        mode = _sigma_mode(d_sigma.shape, d_sigma.numel(), V, M)
    out = _out_like(out, (V, M), dev)
    stats = torch.empty((V, 2), dtype=torch.float64, device=dev) if d_Y is not None else None
    status = torch.zeros(2, dtype=torch.int32, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    L.check(L.lib().mfx_predict_dev(plan.handle(), d_params.data_ptr(), _tptr(d_peaks), int(maxfasc), int(bool(csf_on)),
                                    int(bool(ear_on)), _tptr(d_sig_csf), _tptr(d_sig_ear), int(E), V, _tptr(d_Y),
                                    _tptr(d_sigma), mode, int(ncoils), int(seed) & _U64, int(offset) & _U64, out.data_ptr(),
                                    _tptr(stats), status.data_ptr(), st))
    if check:
        flag, vox = status.tolist()
        dir_err = None
        try:     # read (and clear) the plan's word in any case, so that nothing of this batch is reported by the next call
            L.check(L.lib().mfx_plan_status(plan.handle(), st))
        except ValueError as e:
            dir_err = e
        if flag:
            raise ValueError("predict: voxel %d of the batch has %s" % (vox, " and ".join(
                w for b, w in ((1, "an atom index that is not an integer inside its dictionary"),
                               (2, "a weight M0 * nu that is negative or not finite")) if flag & b)))
        if dir_err is not None:
            raise dir_err
    return out if stats is None else (out, stats)


def predict(plan, params, peaks, maxfasc, csf_on=False, ear_on=False, sig_csf=None, sig_ear=None, E=0, Y=None,
            sigma_g=None, ncoils=0, seed=0, offset=0):
    """predict_dev on NumPy buffers (mfx_predict): returns out [V x M], or (out, stats [V x 2]) when Y is given.
    Bad atom indices and weights raise ValueError before anything is launched."""
    params = L.f64c(params)
    pk = L.f64c(peaks) if maxfasc > 0 else None
    sc = L.f64c(sig_csf).reshape(-1) if csf_on else None
    se = L.f64c(sig_ear) if ear_on else None
    Yc = L.f64c_opt(Y)
    V = _predict_shapes(plan, params.shape, pk.shape if pk is not None else None, maxfasc, csf_on, ear_on,
                        Yc.shape if Yc is not None else None, sc.shape[0] if sc is not None else None,
                        se.shape if se is not None else None, E)
    M = plan.M
    mode, sg = SIGMA_SCALAR, None
    if ncoils:
        if sigma_g is None:
            raise ValueError("noise (ncoils > 0) needs sigma_g")
        sg = np.atleast_1d(L.f64c(sigma_g))
        mode = _sigma_mode(sg.shape, sg.size, V, M)
    out = np.zeros((V, M))
    stats = np.zeros((V, 2)) if Yc is not None else None
    L.check(L.lib().mfx_predict(plan.handle(), L.dptr(params), L.opt(pk), int(maxfasc), int(bool(csf_on)), int(bool(ear_on)),
                                L.opt(sc), L.opt(se), int(E), V, L.opt(Yc), L.opt(sg), mode, int(ncoils), int(seed) & _U64,
                                int(offset) & _U64, L.dptr(out), L.opt(stats)))
    return out if stats is None else (out, stats)


def sos_noise_dev(d_S0, sigma_g, ncoils=1, seed=0, offset=0, out=None):
    """Sum-of-squares magnitude noise on the device (mfx_sos_noise_dev): sqrt(sum over ``ncoils`` coils of
    (S0 + sigma a)^2 + (sigma b)^2), a, b standard normals.  ``d_S0``: torch CUDA float64 tensor of any shape;
    ``sigma_g``: a number, or a tensor with one value or the shape of ``d_S0``.  Element i (C order) draws from the
    counter ``offset + i`` of the Philox stream keyed by ``seed``: splitting an array into calls with matching
    offsets gives the same values.  Enqueues on torch's current stream; ``out`` may be ``d_S0`` itself."""
    import torch
    _f64_cuda(d_S0)
    dev = d_S0.device
    d_sigma = (sigma_g.to(device=dev, dtype=torch.float64).contiguous() if torch.is_tensor(sigma_g)
               else torch.full((1,), float(sigma_g), dtype=torch.float64, device=dev))
    if d_sigma.numel() != 1 and d_sigma.shape != d_S0.shape:
        raise ValueError("sigma_g should be a scalar or have the shape %s of S0, got %s"
                         % (tuple(d_S0.shape), tuple(d_sigma.shape)))
    if int(ncoils) < 1:
        raise ValueError("ncoils should be at least 1")
    out = _out_like(out, d_S0.shape, dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    L.check(L.lib().mfx_sos_noise_dev(d_S0.data_ptr(), d_S0.numel(), d_sigma.data_ptr(),
                                      SIGMA_SCALAR if d_sigma.numel() == 1 else SIGMA_ELEMENT, int(ncoils),
                                      int(seed) & _U64, int(offset) & _U64, out.data_ptr(),
                                      dev.index if dev.index is not None else torch.cuda.current_device(), st))
    return out


def sos_noise(S0, sigma_g, ncoils=1, seed=0, offset=0, device=0):
    """sos_noise_dev on NumPy buffers (mfx_sos_noise): S0 float64 of any shape, sigma_g with one value or S0's shape."""
    S0 = L.f64c(S0)
    sg = np.atleast_1d(L.f64c(sigma_g))
    if sg.size != 1 and sg.shape != S0.shape:
        raise ValueError("sigma_g should be a scalar or have the shape %s of S0, got %s" % (S0.shape, sg.shape))
    out = np.zeros(S0.shape)
    L.check(L.lib().mfx_sos_noise(L.dptr(S0), S0.size, L.dptr(sg), SIGMA_SCALAR if sg.size == 1 else SIGMA_ELEMENT,
                                  int(ncoils), int(seed) & _U64, int(offset) & _U64, L.dptr(out), int(device)))
    return out


_PROFILE_SCOPE, _SOFT2D_SCOPE = "objective profiles", "soft fits and profiles of 2-D protocols"


def _soft_shapes(what, M, y_shape, pk_shape, K, csf_on=False, M_csf=None):
    """Argument checks shared by the profile, posterior and pair-objective entry points (``what`` _PROFILE_SCOPE) and their
    2-D protocol forms (_SOFT2D_SCOPE, which have no CSF column), before any device call; returns V."""
    K = int(K)
    if K not in (1, 2):
        raise NotImplementedError("%s serve K = 1 or 2 fascicles (got %d): three fascicles and voxels without one are out "
                                  "of scope" % (what, K))
    if len(y_shape) != 2 or y_shape[1] != M:
        raise ValueError("data has shape %s, protocol has %d measurements" % (tuple(y_shape), M))
    V = y_shape[0]
    if pk_shape is None or tuple(pk_shape) != (V, 3 * K):
        raise ValueError("peaks should have shape (%d, %d)" % (V, 3 * K))
    if csf_on and M_csf != M:
        raise ValueError("sig_csf has %s entries, protocol has %d" % (M_csf, M))
    return V


def _soft_dev_args(what, M, d_Y, d_peaks, K, d_W, csf_on=False, d_sig_csf=None, T_shift=()):
    """Argument checks of the device forms of those entry points, shapes first and the tensors' kind last; ``T_shift``
    the posteriors' (T, shift).  Returns (V, w_stride, the pointer of sig_csf: None without a CSF column)."""
    import torch
    if csf_on and d_sig_csf is None:
        raise ValueError("csf_on without d_sig_csf")
    d_sig_csf = d_sig_csf if csf_on else None
    V = _soft_shapes(what, M, d_Y.shape, d_peaks.shape, K, csf_on, d_sig_csf.numel() if csf_on else None)
    for t, name in zip(T_shift, ("T", "shift")):
        if not torch.is_tensor(t) or tuple(t.shape) != (V,):
            raise ValueError("%s should be a tensor with one entry per voxel (%d)" % (name, V))
    w_stride = _w_stride(M, V, d_W.shape) if d_W is not None else None
    _f64_cuda(d_Y, d_peaks, *T_shift, d_sig_csf, d_W)
    return V, w_stride, _tptr(d_sig_csf)


def profile_dev(plan, d_Y, d_peaks, K, csf_on=False, d_sig_csf=None, partner=False, out=None, d_W=None):
    """Objective profiles on the device (mfx_profile_dev) for torch CUDA float64 tensors of ONE voxel class (every
    voxel: K fascicles, CSF or not, no EAR): ``obj`` [V x K x N], obj[v, k, i] the smallest sum of squared residuals
    any partner atom reaches beside atom i of fascicle k (include/mfx_profile.h has the definitions), and with
    ``partner=True`` also the int32 tensor of the arg-min partners (-1 for K = 1).  Enqueues on torch's current
    stream and returns without waiting; a direction that is not a unit vector flags the plan's status word.
    ``d_W``: measurement weights [V x M] or [M] of a weighted fit (mfx_wprofile_dev, include/mfx_wsoft.h): the profile of
    sum_m W (y_m - model_m)^2; a voxel whose weights are unusable (one negative or not finite, none positive) gets NaN
    values and partner -1."""
    import torch
    V, w_stride, sc = _soft_dev_args(_PROFILE_SCOPE, plan.M, d_Y, d_peaks, K, d_W, csf_on, d_sig_csf)
    N = plan.tables.N
    out = _out_like(out, (V, int(K), N), d_Y.device)
    part = torch.empty((V, int(K), N), dtype=torch.int32, device=d_Y.device) if partner else None
    st = torch.cuda.current_stream(d_Y.device).cuda_stream
    _twin("profile_dev", plan.handle(), d_Y.data_ptr(), _tptr(d_W), w_stride, d_peaks.data_ptr(), int(K), int(bool(csf_on)), sc,
          V, out.data_ptr(), _tptr(part), st)
    return (out, part) if partner else out


def pair_objectives_dev(plan, d_Y, d_peaks, csf_on=False, d_sig_csf=None, d_W=None):
    """The objective of every atom pair (mfx_pair_objectives_dev): [V x N x N] torch tensor, two-fascicle voxels.
    ``d_W``: measurement weights [V x M] or [M] (mfx_wpair_objectives_dev)."""
    import torch
    V, w_stride, sc = _soft_dev_args(_PROFILE_SCOPE, plan.M, d_Y, d_peaks, 2, d_W, csf_on, d_sig_csf)
    N = plan.tables.N
    out = torch.empty((V, N, N), dtype=torch.float64, device=d_Y.device)
    st = torch.cuda.current_stream(d_Y.device).cuda_stream
    _twin("pair_objectives_dev", plan.handle(), d_Y.data_ptr(), _tptr(d_W), w_stride, d_peaks.data_ptr(), int(bool(csf_on)), sc,
          V, out.data_ptr(), st)
    return out


def profile_classes(K, csf, ear, maxfasc):
    """Bins the voxels of a mixed volume for the profile: ([(k, csf_flag, indices)], n_unsupported).  In scope: one or
    two fascicles (k <= maxfasc), with or without CSF, no EAR."""
    K = np.asarray(K).astype(np.int64)
    V = K.shape[0]
    csf = np.zeros(V, bool) if csf is None else np.asarray(csf).astype(bool)
    ear = np.zeros(V, bool) if ear is None else np.asarray(ear).astype(bool)
    if csf.shape != (V,) or ear.shape != (V,):
        raise ValueError("K, csf and ear should have one entry per voxel")
    if V and K.max() > maxfasc:
        raise ValueError("K exceeds maxfasc = %d" % maxfasc)
    ok = (K >= 1) & (K <= 2) & ~ear
    bins = []
    for k in (1, 2):
        for c in (False, True):
            ix = np.flatnonzero(ok & (K == k) & (csf == c))
            if ix.size:
                bins.append((k, c, ix))
    return bins, int(V - np.count_nonzero(ok))


def _soft_host_args(plan, Y, K, csf, peaks, maxfasc, csf_on, sig_csf, W):
    """Argument checks of ``profile`` and ``posterior`` (before any device call): (Y, V, maxfasc, W, w_stride, peaks
    [V x 3 maxfasc], sig_csf).  The voxel classes are binned by the caller (``profile_classes`` checks K and the flags)."""
    Y = L.f64c(Y)
    maxfasc = int(maxfasc)
    if Y.ndim != 2 or Y.shape[1] != plan.M:
        raise ValueError("data has shape %s, protocol has %d measurements" % (Y.shape, plan.M))
    V = Y.shape[0]
    if np.asarray(K).shape != (V,):
        raise ValueError("K should have one entry per voxel")
    W, w_stride = _host_weights(plan.M, V, W)
    pk = L.f64c(peaks).reshape(V, -1) if maxfasc > 0 else np.zeros((V, 0))
    if pk.shape[1] != 3 * maxfasc:
        raise ValueError("peaks should have %d columns" % (3 * maxfasc))
    sc = L.f64c(sig_csf).reshape(-1) if sig_csf is not None else None
    if np.any(csf) and (not csf_on or sc is None):
        raise ValueError("voxels flagged CSF need csf_on and sig_csf")
    if sc is not None and sc.shape[0] != plan.M:
        raise ValueError("sig_csf has %d entries, protocol has %d" % (sc.shape[0], plan.M))
    return Y, V, maxfasc, W, w_stride, pk, sc


def profile(plan, Y, K, csf, peaks, maxfasc, csf_on, sig_csf, partner=False, ear=None, W=None):
    """Objective profiles of a mixed set of voxels on NumPy arrays (mfx_profile, one call per voxel class): Y [V x M],
    per-voxel K, csf (and ear) flags, peaks [V x 3 maxfasc] as for ``fit_batch``.  Returns ``(obj, partner,
    n_unsupported)``: obj [V x maxfasc x N] float64 (rows of absent fascicles and of the voxel classes out of scope -
    EAR, no fascicle, three fascicles - are NaN), partner [V x maxfasc x N] int32 (-1 where there is none) or None,
    and the number of voxels out of scope.  ``W``: measurement weights [V x M] or [M] of a weighted fit (mfx_wprofile):
    the profile of sum_m W (y_m - model_m)^2, whose minimum is ``fit_weighted``'s MSE * sum_m W; a voxel whose weights are
    unusable (one negative or not finite, none positive) gets NaN values and partner -1."""
    Y, V, maxfasc, W, w_stride, pk, sc = _soft_host_args(plan, Y, K, csf, peaks, maxfasc, csf_on, sig_csf, W)
    bins, n_uns = profile_classes(K, csf, ear, maxfasc)
    N = plan.tables.N
    obj = np.full((V, maxfasc, N), np.nan)
    par = np.full((V, maxfasc, N), -1, dtype=np.int32) if partner else None
    for k, c, ix in bins:
        Yc, pc = np.ascontiguousarray(Y[ix]), np.ascontiguousarray(pk[ix, :3 * k])
        o = np.zeros((ix.size, k, N))
        p = np.zeros((ix.size, k, N), dtype=np.int32) if partner else None
        Wc = _w_chunk(W, w_stride, ix)
        _twin("profile", plan.handle(), L.dptr(Yc), L.opt(Wc), w_stride, L.dptr(pc), k, int(c), L.dptr(sc) if c else None,
              ix.size, L.dptr(o), L.opt(p, L.iptr))
        obj[ix, :k] = o
        if partner:
            par[ix, :k] = p
    return obj, par, n_uns


def pair_objectives(plan, Y, peaks, csf_on=False, sig_csf=None, W=None):
    """The objective of every atom pair of two-fascicle voxels (mfx_pair_objectives): Y [V x M], peaks [V x 6] ->
    [V x N x N], out[v, i, j] = min over non-negative weights of |y - w1 D_0[:, i] - w2 D_1[:, j] (- wx sig_csf)|^2.
    ``W``: measurement weights [V x M] or [M] (mfx_wpair_objectives): the weighted sum of squares."""
    Y = L.f64c(Y)
    pk = L.f64c(peaks)
    sc = L.f64c(sig_csf).reshape(-1) if csf_on else None
    if csf_on and sig_csf is None:
        raise ValueError("csf_on without sig_csf")
    V = _soft_shapes(_PROFILE_SCOPE, plan.M, Y.shape, pk.shape, 2, csf_on, sc.shape[0] if sc is not None else None)
    W, w_stride = _host_weights(plan.M, V, W)
    N = plan.tables.N
    out = np.zeros((V, N, N))
    _twin("pair_objectives", plan.handle(), L.dptr(Y), L.opt(W), w_stride, L.dptr(pk), int(bool(csf_on)), L.opt(sc), V,
          L.dptr(out))
    return out


def _per_voxel(x, V, what):
    """A scalar or a [V] array as a float64 [V] array."""
    x = np.asarray(x, dtype=np.float64)
    if x.ndim == 0:
        return np.full(V, float(x))
    if x.shape != (V,):
        raise ValueError("%s should be a scalar or have one entry per voxel (%d), got shape %s" % (what, V, x.shape))
    return np.ascontiguousarray(x)


def posterior_dev(plan, d_Y, d_peaks, K, T, shift, csf_on=False, d_sig_csf=None, d_W=None):
    """Soft fit on the device (mfx_post_dev) for torch CUDA float64 tensors of ONE voxel class (every voxel: K
    fascicles, CSF or not, no EAR).  ``T`` [V] the temperatures (2 sigma^2), ``shift`` [V] a value near each voxel's
    smallest objective (include/mfx_post.h has the definitions).  Returns ``(w, log_sum, status)``: w [V x K x N]
    the posterior weight of every atom of each fascicle, log_sum [V] = log sum exp(-F / T), status [V] int32 (0 ok,
    1 unusable T or shift, 2 unusable shift: an exponent above 700 or a vanishing sum; rows of such voxels are NaN).
    Enqueues on torch's current stream and returns without waiting.  ``d_W``: measurement weights [V x M] or [M] of a
    weighted fit (mfx_wpost_dev, include/mfx_wsoft.h): F is the weighted sum of squares and T = 2 sigma^2 means that
    measurement m has noise variance sigma^2 / W_m; status 3: a weight is negative or not finite, 4: none is positive."""
    import torch
    V, w_stride, sc = _soft_dev_args(_PROFILE_SCOPE, plan.M, d_Y, d_peaks, K, d_W, csf_on, d_sig_csf, (T, shift))
    N = plan.tables.N
    w = torch.empty((V, int(K), N), dtype=torch.float64, device=d_Y.device)
    log_sum = torch.empty((V,), dtype=torch.float64, device=d_Y.device)
    status = torch.empty((V,), dtype=torch.int32, device=d_Y.device)
    st = torch.cuda.current_stream(d_Y.device).cuda_stream
    _twin("post_dev", plan.handle(), d_Y.data_ptr(), _tptr(d_W), w_stride, d_peaks.data_ptr(), int(K), int(bool(csf_on)), sc,
          T.data_ptr(), shift.data_ptr(), V, w.data_ptr(), log_sum.data_ptr(), status.data_ptr(), st)
    return w, log_sum, status


def posterior(plan, Y, K, csf, peaks, maxfasc, csf_on, sig_csf, sigma, shift=None, ear=None, W=None):
    """Soft fit of a mixed set of voxels on NumPy arrays (mfx_post, one call per voxel class): Y [V x M], per-voxel K,
    csf (and ear) flags, peaks [V x 3 maxfasc] as for ``fit_batch``; ``sigma`` the noise standard deviation (a scalar
    or [V]; the temperature is 2 sigma^2); ``shift`` [V] a value near each voxel's smallest objective, default: MSE * M
    of the library's own fit of the same voxels.  Returns ``(w, log_sum, status, n_unsupported)``: w [V x maxfasc x N]
    float64, log_sum [V], status [V] int32 (the codes of include/mfx_post.h, and -1 for a voxel class out of scope: EAR,
    no fascicle, three fascicles - counted in n_unsupported); rows of absent fascicles and of voxels with a non-zero
    status are NaN.  ``W``: measurement weights [V x M] or [M] of a weighted fit (mfx_wpost): F is the weighted sum of
    squares, ``sigma`` the noise of a measurement of weight 1 (measurement m has variance sigma^2 / W_m), the default
    shift ``fit_weighted``'s objective MSE * sum_m W; status 3: a weight is negative or not finite, 4: none is positive."""
    Y, V, maxfasc, W, w_stride, pk, sc = _soft_host_args(plan, Y, K, csf, peaks, maxfasc, csf_on, sig_csf, W)
    sig = _per_voxel(sigma, V, "sigma")
    sh = _per_voxel(shift, V, "shift") if shift is not None else None
    bins, n_uns = profile_classes(K, csf, ear, maxfasc)
    N = plan.tables.N
    w = np.full((V, maxfasc, N), np.nan)
    log_sum = np.full(V, np.nan)
    status = np.full(V, -1, dtype=np.int32)
    for k, c, ix in bins:
        Yc, pc, Wc = np.ascontiguousarray(Y[ix]), np.ascontiguousarray(pk[ix, :3 * k]), _w_chunk(W, w_stride, ix)
        if sh is not None:
            shc = np.ascontiguousarray(sh[ix])
        elif W is None:
            fit = fit_batch(plan, Yc, np.full(ix.size, k), np.full(ix.size, c), None, pc, k, c, False, sc if c else None)
            shc = np.ascontiguousarray(fit[:, -2] * plan.M)
        else:   # the weighted fit's objective; a voxel with unusable weights has a NaN row there and status 3 / 4 here
            fit, fst = fit_weighted(plan, Yc, Wc, np.full(ix.size, k), np.full(ix.size, c), pc, k, c, sc if c else None)
            with np.errstate(invalid='ignore', over='ignore'):
                sw = np.sum(Wc, axis=-1) if w_stride else np.full(ix.size, np.sum(Wc))
                shc = np.ascontiguousarray(fit[:, -2] * sw)
            shc[fst != 0] = 0.0
        Tc = np.ascontiguousarray(2.0 * sig[ix] ** 2)
        wc, lc, stc = np.zeros((ix.size, k, N)), np.zeros(ix.size), np.zeros(ix.size, dtype=np.int32)
        _twin("post", plan.handle(), L.dptr(Yc), L.opt(Wc), w_stride, L.dptr(pc), k, int(c), L.dptr(sc) if c else None,
              L.dptr(Tc), L.dptr(shc), ix.size, L.dptr(wc), L.dptr(lc), L.iptr(stc))
        w[ix, :k], log_sum[ix], status[ix] = wc, lc, stc
    return w, log_sum, status, n_uns


def rotate2d_dev(tables, d_dirs, d_cols=None):
    """Device-resident 2-D protocol rotation (mfx_rot2d_rotate_dev / mfx_rot2d_rotate_cols_dev) for a
    mf_utils.RotateAtom2DTables: torch CUDA tensors dirs [B,3] f64 (and cols [B] int: one atom per direction)
    -> (out [B,M,N] f64, or [B,M] with cols; status [B,4] int32), enqueued on torch's current stream without a
    host synchronisation.  A failing direction's output is NaN; ``tables.raise_for_status(status.cpu())``
    raises the reference's exception for the first one."""
    import torch
    _f64_cuda(d_dirs)
    B = d_dirs.shape[0]
    h = tables.handle()
    st = torch.cuda.current_stream(d_dirs.device).cuda_stream
    status = torch.empty((B, 4), dtype=torch.int32, device=d_dirs.device)
    if d_cols is None:
        out = torch.empty((B, tables.M, tables.N), dtype=torch.float64, device=d_dirs.device)
        L.check(L.lib().mfx_rot2d_rotate_dev(h, d_dirs.data_ptr(), B, out.data_ptr(), status.data_ptr(), st))
    else:
        cols = d_cols.to(torch.int32).contiguous()
        assert cols.shape == (B,)
        out = torch.empty((B, tables.M), dtype=torch.float64, device=d_dirs.device)
        L.check(L.lib().mfx_rot2d_rotate_cols_dev(h, d_dirs.data_ptr(), cols.data_ptr(), B, out.data_ptr(),
                                                  status.data_ptr(), st))
    return out, status


def _fit2d_shapes(tables, y_shape, pk_shape, maxfasc):
    """Argument checks shared by the 2-D protocol fit's entry points (before any device call); returns V."""
    if maxfasc < 0 or maxfasc > 3:
        raise NotImplementedError("the 2-D protocol fit serves 0 to 3 fascicles per voxel (maxfasc = %d)" % maxfasc)
    if len(y_shape) != 2 or y_shape[1] != tables.M:
        raise ValueError("data has shape %s, protocol has %d measurements" % (tuple(y_shape), tables.M))
    V = y_shape[0]
    if tuple(pk_shape) != (V, 3 * maxfasc):
        raise ValueError("peaks should have shape (%d, %d)" % (V, 3 * maxfasc))
    return V


def fit2d_dev(tables, d_Y, d_peaks, maxfasc, out=None):
    """Device-resident fit of voxels of a 2-D (AxCaliber-like) protocol (mfx_fit2d_batch_dev) for a
    mf_utils.RotateAtom2DTables and ONE voxel class: every voxel has ``maxfasc`` fascicles and no CSF column.
    torch CUDA float64 tensors d_Y [V, M], d_peaks [V, 3 maxfasc] -> (params [V, num_params(maxfasc, False, False)]
    f64, status [V, 5] int32: the failing direction's record and fascicle index, zeros for a fitted voxel).
    Enqueues on torch's current stream and returns without waiting; a voxel with a failing direction has a NaN row."""
    import torch
    maxfasc = int(maxfasc)
    _f64_cuda(d_Y, d_peaks)
    V = _fit2d_shapes(tables, d_Y.shape, d_peaks.shape, maxfasc)
    out = _out_like(out, (V, num_params(maxfasc, False, False)), d_Y.device)
    status = torch.empty((V, 5), dtype=torch.int32, device=d_Y.device)
    st = torch.cuda.current_stream(d_Y.device).cuda_stream
    L.check(L.lib().mfx_fit2d_batch_dev(tables.handle(), d_Y.data_ptr(), d_peaks.data_ptr(), maxfasc, V, out.data_ptr(),
                                        status.data_ptr(), st))
    return out, status


def fit2d(tables, Y, K, csf, peaks, maxfasc, csf_on, sig_csf=None):
    """Fit of a mixed set of voxels of a 2-D protocol on NumPy arrays (mfx_fit2d_batch): Y [V, M], per-voxel fascicle
    counts K [V] in 0..maxfasc, CSF flags csf [V] (or None), peaks [V, 3 maxfasc] -> (params [V, num_params(maxfasc,
    csf_on, False)], status [V, 5] int32).  A voxel with a failing direction has a NaN row and a non-zero record."""
    Y = L.f64c(Y)
    maxfasc = int(maxfasc)
    pk = L.f64c(peaks).reshape(Y.shape[0], -1) if (maxfasc > 0 and Y.ndim == 2) else np.zeros((Y.shape[0], 0))
    V = _fit2d_shapes(tables, Y.shape, pk.shape, maxfasc)
    K, cs, sc = _mixed_args(tables.M, V, maxfasc, K, csf, csf_on, sig_csf)
    params = np.zeros((V, num_params(maxfasc, bool(csf_on), False)))
    status = np.zeros((V, 5), dtype=np.int32)
    L.check(L.lib().mfx_fit2d_batch(tables.handle(), L.dptr(Y), L.iptr(K), L.opt(cs, L.bptr), L.dptr(pk) if maxfasc > 0 else None,
                                    maxfasc, int(bool(csf_on)), L.opt(sc), V, L.dptr(params), L.iptr(status)))
    return params, status


def fit2d_weighted_dev(tables, d_Y, d_W, d_peaks, maxfasc, out=None):
    """Device-resident weighted fit of voxels of a 2-D protocol (mfx_wfit2d_batch_dev, include/mfx_w2d.h) for ONE voxel
    class, arguments as ``fit2d_dev`` and d_W [V, M] or [M] the weights >= 0 of the measurements: minimises
    sum_m W[v, m] (y_m - model_m)^2.  Returns (params, status [V, 5] int32, wstatus [V] int32: 0 fitted, 1 a negative or
    non-finite weight, 2 no positive weight; such a voxel has a NaN row).  MSE = min_obj / sum_m W, R2 the squared
    weighted correlation.  Enqueues on torch's current stream and returns without waiting."""
    import torch
    maxfasc = int(maxfasc)
    V = _fit2d_shapes(tables, d_Y.shape, d_peaks.shape, maxfasc)
    w_stride = _w_stride(tables.M, V, d_W.shape)
    _f64_cuda(d_Y, d_W, d_peaks)
    out = _out_like(out, (V, num_params(maxfasc, False, False)), d_Y.device)
    status = torch.empty((V, 5), dtype=torch.int32, device=d_Y.device)
    wstatus = torch.empty((V,), dtype=torch.int32, device=d_Y.device)
    st = torch.cuda.current_stream(d_Y.device).cuda_stream
    L.check(L.lib().mfx_wfit2d_batch_dev(tables.handle(), d_Y.data_ptr(), d_W.data_ptr(), w_stride,
                                         d_peaks.data_ptr() if maxfasc > 0 else None, maxfasc, V, out.data_ptr(),
                                         status.data_ptr(), wstatus.data_ptr(), st))
    return out, status, wstatus


def fit2d_weighted(tables, Y, W, K, csf, peaks, maxfasc, csf_on, sig_csf=None):
    """Weighted fit of a mixed set of voxels of a 2-D protocol on NumPy arrays (mfx_wfit2d_batch): arguments as ``fit2d``
    and W [V, M] or [M] the weights >= 0 of the measurements (a 0/1 outlier mask, inverse noise variances, ...).
    Returns (params, status [V, 5] int32, wstatus [V] int32: 1 a negative or non-finite weight, 2 no positive weight;
    such a voxel, like one with a failing direction, has a NaN row)."""
    Y = L.f64c(Y)
    W = L.f64c(W)
    maxfasc = int(maxfasc)
    pk = L.f64c(peaks).reshape(Y.shape[0], -1) if (maxfasc > 0 and Y.ndim == 2) else np.zeros((Y.shape[0], 0))
    V = _fit2d_shapes(tables, Y.shape, pk.shape, maxfasc)
    w_stride = _w_stride(tables.M, V, W.shape)
    K, cs, sc = _mixed_args(tables.M, V, maxfasc, K, csf, csf_on, sig_csf)
    params = np.zeros((V, num_params(maxfasc, bool(csf_on), False)))
    status = np.zeros((V, 5), dtype=np.int32)
    wstatus = np.zeros(V, dtype=np.int32)
    L.check(L.lib().mfx_wfit2d_batch(tables.handle(), L.dptr(Y), L.dptr(W), w_stride, L.iptr(K), L.opt(cs, L.bptr),
                                     L.dptr(pk) if maxfasc > 0 else None, maxfasc, int(bool(csf_on)), L.opt(sc), V,
                                     L.dptr(params), L.iptr(status), L.iptr(wstatus)))
    return params, status, wstatus


def _predict2d_shapes(tables, p_shape, pk_shape, maxfasc, csf_on, y_shape, M_csf):
    """Argument checks shared by predict2d and predict2d_dev (before any device call); returns V."""
    maxfasc = int(maxfasc)
    if maxfasc < 0 or maxfasc > 3:
        raise NotImplementedError("the 2-D protocol prediction serves 0 to 3 fascicles per voxel (maxfasc = %d)" % maxfasc)
    npar = num_params(maxfasc, csf_on, False)
    if len(p_shape) != 2 or p_shape[1] != npar:
        raise ValueError("params should have %d columns (maxfasc = %d, csf_on = %s), got shape %s"
                         % (npar, maxfasc, bool(csf_on), tuple(p_shape)))
    V = p_shape[0]
    if maxfasc > 0 and (pk_shape is None or tuple(pk_shape) != (V, 3 * maxfasc)):
        raise ValueError("peaks should have shape (%d, %d)" % (V, 3 * maxfasc))
    if csf_on and M_csf != tables.M:
        raise ValueError("sig_csf has %s entries, protocol has %d" % (M_csf, tables.M))
    if y_shape is not None and tuple(y_shape) != (V, tables.M):
        raise ValueError("data has shape %s, protocol has %d measurements for %d voxels" % (tuple(y_shape), tables.M, V))
    return V


def predict2d_dev(tables, d_params, d_peaks, maxfasc, csf_on=False, d_sig_csf=None, d_Y=None, sigma_g=None, ncoils=0, seed=0,
                  offset=0, out=None):
    """Forward model of a 2-D (AxCaliber-like) protocol on the device (mfx_predict2d_dev, include/mfx_predict2d.h) for a
    mf_utils.RotateAtom2DTables: parameter rows [V, num_params(maxfasc, csf_on, False)] in the layout ``fit2d_dev``
    returns and peaks [V, 3 maxfasc] (torch CUDA float64 tensors) -> the signal [V, M] they stand for: per present
    fascicle the column ``rotate_cols`` returns, bit for bit, times M0 nu, summed in the order f0, f1, f2, csf.  With
    ``ncoils`` > 0 the magnitude noise of ``sos_noise_dev`` is applied in the same pass (``sigma_g`` a number or a tensor
    with one value, one per voxel or one per element; element (v, m) draws with index ``offset + v M + m``); with ``d_Y``
    [V, M] the per-voxel residual sum of squares and R2 come back too.  Returns (out, stats [V, 2] or None, status [2]
    int32, dir_status [V, 5] int32): a row with a bad atom index or weight is NaN and flags ``status`` (bits 1 / 2); a
    present fascicle with a failing direction gives a NaN row and its record in ``dir_status``.  Enqueues on torch's
    current stream and returns without waiting."""
    import torch
    maxfasc = int(maxfasc)
    d_peaks, d_sig_csf = d_peaks if maxfasc > 0 else None, d_sig_csf if csf_on else None
    _f64_cuda(d_params, d_peaks, d_sig_csf, d_Y)
    dev = d_params.device
    V = _predict2d_shapes(tables, d_params.shape, d_peaks.shape if maxfasc > 0 else None, maxfasc, csf_on,
                          d_Y.shape if d_Y is not None else None, d_sig_csf.numel() if csf_on else None)
    M = tables.M
    mode, d_sigma = SIGMA_SCALAR, None
    if ncoils:
        if sigma_g is None:
            raise ValueError("noise (ncoils > 0) needs sigma_g")
        d_sigma = (sigma_g.to(device=dev, dtype=torch.float64).contiguous() if torch.is_tensor(sigma_g)
                   else torch.full((1,), float(sigma_g), dtype=torch.float64, device=dev))
        mode = _sigma_mode(d_sigma.shape, d_sigma.numel(), V, M)
    out = _out_like(out, (V, M), dev)
    stats = torch.empty((V, 2), dtype=torch.float64, device=dev) if d_Y is not None else None
    status = torch.zeros(2, dtype=torch.int32, device=dev)
    dstat = torch.empty((V, 5), dtype=torch.int32, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    L.check(L.lib().mfx_predict2d_dev(tables.handle(), d_params.data_ptr(), _tptr(d_peaks), maxfasc, int(bool(csf_on)),
                                      _tptr(d_sig_csf), V, _tptr(d_Y), _tptr(d_sigma), mode, int(ncoils), int(seed) & _U64,
                                      int(offset) & _U64, out.data_ptr(), _tptr(stats), status.data_ptr(), dstat.data_ptr(), st))
    return out, stats, status, dstat


def predict2d(tables, params, peaks, maxfasc, csf_on=False, sig_csf=None, Y=None, sigma_g=None, ncoils=0, seed=0, offset=0):
    """predict2d_dev on NumPy buffers (mfx_predict2d): returns (out [V, M], dir_status [V, 5] int32), or (out, stats
    [V, 2], dir_status) when Y is given.  Bad atom indices and weights raise ValueError before anything is launched; a
    present fascicle with a failing direction gives a NaN row and its record in ``dir_status``."""
    maxfasc = int(maxfasc)
    params = L.f64c(params)
    pk = L.f64c(peaks) if maxfasc > 0 else None
    sc = L.f64c(sig_csf).reshape(-1) if csf_on else None
    Yc = L.f64c_opt(Y)
    V = _predict2d_shapes(tables, params.shape, pk.shape if pk is not None else None, maxfasc, csf_on,
                          Yc.shape if Yc is not None else None, sc.shape[0] if sc is not None else None)
    M = tables.M
    mode, sg = SIGMA_SCALAR, None
    if ncoils:
        if sigma_g is None:
            raise ValueError("noise (ncoils > 0) needs sigma_g")
        sg = np.atleast_1d(L.f64c(sigma_g))
        mode = _sigma_mode(sg.shape, sg.size, V, M)
    out = np.zeros((V, M))
    stats = np.zeros((V, 2)) if Yc is not None else None
    dstat = np.zeros((V, 5), dtype=np.int32)
    L.check(L.lib().mfx_predict2d(tables.handle(), L.dptr(params), L.opt(pk), maxfasc, int(bool(csf_on)), L.opt(sc), V,
                                  L.opt(Yc), L.opt(sg), mode, int(ncoils), int(seed) & _U64, int(offset) & _U64, L.dptr(out),
                                  L.opt(stats), L.iptr(dstat)))
    return (out, dstat) if stats is None else (out, stats, dstat)


def posterior2d_dev(tables, d_Y, d_peaks, K, T, shift, d_W=None):
    """Soft fit of voxels of a 2-D (AxCaliber-like) protocol on the device (mfx_post2d_dev, include/mfx_soft2d.h) for a
    mf_utils.RotateAtom2DTables and torch CUDA float64 tensors of ONE voxel class (every voxel: K fascicles, no CSF):
    d_Y [V, M], d_peaks [V, 3 K], ``T`` [V] the temperatures (2 sigma^2), ``shift`` [V] a value near each voxel's smallest
    objective.  Returns ``(w, log_sum, status, dir_status)``: w [V, K, N] the posterior weight of every atom of each
    fascicle, log_sum [V] = log sum exp(-F / T), status [V] int32 (0 ok, 1 unusable T or shift, 2 unusable shift, 5 a
    failing fascicle direction; rows of such voxels are NaN), dir_status [V, 5] int32 the failing direction's record as
    ``fit2d_dev`` gives it.  Enqueues on torch's current stream and returns without waiting.  ``d_W``: measurement weights
    [V, M] or [M] of a weighted fit (mfx_wpost2d_dev, include/mfx_w2d.h): F is the weighted sum of squares and
    T = 2 sigma^2 means that measurement m has variance sigma^2 / W_m; status 3: a weight is negative or not finite,
    4: none is positive."""
    import torch
    V, w_stride, _ = _soft_dev_args(_SOFT2D_SCOPE, tables.M, d_Y, d_peaks, K, d_W, T_shift=(T, shift))
    N = tables.N
    w = torch.empty((V, int(K), N), dtype=torch.float64, device=d_Y.device)
    log_sum = torch.empty((V,), dtype=torch.float64, device=d_Y.device)
    status = torch.empty((V,), dtype=torch.int32, device=d_Y.device)
    dir_status = torch.empty((V, 5), dtype=torch.int32, device=d_Y.device)
    st = torch.cuda.current_stream(d_Y.device).cuda_stream
    _twin("post2d_dev", tables.handle(), d_Y.data_ptr(), _tptr(d_W), w_stride, d_peaks.data_ptr(), int(K), T.data_ptr(),
          shift.data_ptr(), V, w.data_ptr(), log_sum.data_ptr(), status.data_ptr(), dir_status.data_ptr(), st)
    return w, log_sum, status, dir_status


def profile2d_dev(tables, d_Y, d_peaks, K, partner=False, out=None, d_W=None):
    """Objective profiles of voxels of a 2-D protocol on the device (mfx_profile2d_dev) for ONE voxel class, arguments
    as ``posterior2d_dev``.  Returns ``(obj, partner, dir_status)``: obj [V, K, N] float64, obj[v, k, i] the smallest sum
    of squared residuals any partner atom reaches beside atom i of fascicle k; the int32 tensor of the arg-min partners
    (-1 for K = 1) with ``partner=True``, else None; dir_status [V, 5] int32.  A voxel with a failing direction has NaN
    values and partner -1.  Enqueues on torch's current stream and returns without waiting.  ``d_W``: measurement weights
    [V, M] or [M] (mfx_wprofile2d_dev): obj is the weighted sum of squares; a voxel with unusable weights has NaN values
    and partner -1."""
    import torch
    V, w_stride, _ = _soft_dev_args(_SOFT2D_SCOPE, tables.M, d_Y, d_peaks, K, d_W)
    N = tables.N
    out = _out_like(out, (V, int(K), N), d_Y.device)
    part = torch.empty((V, int(K), N), dtype=torch.int32, device=d_Y.device) if partner else None
    dir_status = torch.empty((V, 5), dtype=torch.int32, device=d_Y.device)
    st = torch.cuda.current_stream(d_Y.device).cuda_stream
    _twin("profile2d_dev", tables.handle(), d_Y.data_ptr(), _tptr(d_W), w_stride, d_peaks.data_ptr(), int(K), V, out.data_ptr(),
          _tptr(part), dir_status.data_ptr(), st)
    return out, part, dir_status


def _soft2d_host_args(tables, Y, K, peaks, maxfasc, csf):
    """Argument checks of ``posterior2d`` and ``profile2d`` (before any device call): (Y, peaks [V x 3 maxfasc], maxfasc,
    bins [(k, indices)], n_unsupported).  In scope: one or two fascicles without a CSF column."""
    Y = L.f64c(Y)
    maxfasc = int(maxfasc)
    if Y.ndim != 2 or Y.shape[1] != tables.M:
        raise ValueError("data has shape %s, protocol has %d measurements" % (Y.shape, tables.M))
    V = Y.shape[0]
    K = np.asarray(K)
    if K.shape != (V,):
        raise ValueError("K should have one entry per voxel")
    pk = L.f64c(peaks).reshape(V, -1) if maxfasc > 0 else np.zeros((V, 0))
    if pk.shape[1] != 3 * maxfasc:
        raise ValueError("peaks should have %d columns" % (3 * maxfasc))
    K = K.astype(np.int64)
    if V and (K.min() < 0 or K.max() > maxfasc):
        raise ValueError("K should lie in 0..maxfasc = %d" % maxfasc)
    csf = np.zeros(V, bool) if csf is None else np.asarray(csf).astype(bool)
    if csf.shape != (V,):
        raise ValueError("csf should have one entry per voxel")
    ok = (K >= 1) & (K <= 2) & ~csf
    bins = [(k, np.flatnonzero(ok & (K == k))) for k in (1, 2)]
    return Y, pk, maxfasc, [(k, ix) for k, ix in bins if ix.size], int(V - np.count_nonzero(ok))


def posterior2d(tables, Y, K, peaks, maxfasc, sigma, shift=None, csf=None, W=None):
    """Soft fit of a mixed set of voxels of a 2-D protocol on NumPy arrays (mfx_post2d, one call per fascicle count):
    Y [V, M], per-voxel K, peaks [V, 3 maxfasc] as for ``fit2d``; ``sigma`` the noise standard deviation (a scalar or
    [V]; the temperature is 2 sigma^2); ``shift`` [V] a value near each voxel's smallest objective, default: MSE * M of
    ``fit2d`` on the same voxels.  Returns ``(w, log_sum, status, dir_status, n_unsupported)``: w [V, maxfasc, N] float64,
    log_sum [V], status [V] int32 (the codes of include/mfx_soft2d.h, and -1 for a voxel out of scope: no fascicle, three
    fascicles, a CSF flag - counted in n_unsupported), dir_status [V, 5] int32 (the failing direction's record of a voxel
    with status 5); rows of absent fascicles and of voxels with a non-zero status are NaN.  ``W``: measurement weights
    [V, M] or [M] of a weighted fit (mfx_wpost2d): F is the weighted sum of squares, ``sigma`` the noise of a measurement
    of weight 1 (measurement m has variance sigma^2 / W_m), the default shift ``fit2d_weighted``'s objective
    MSE * sum_m W; status 3: a weight is negative or not finite, 4: none is positive."""
    Y, pk, maxfasc, bins, n_uns = _soft2d_host_args(tables, Y, K, peaks, maxfasc, csf)
    V, N = Y.shape[0], tables.N
    W, w_stride = _host_weights(tables.M, V, W)
    sig = _per_voxel(sigma, V, "sigma")
    sh = _per_voxel(shift, V, "shift") if shift is not None else None
    w = np.full((V, maxfasc, N), np.nan)
    log_sum = np.full(V, np.nan)
    status = np.full(V, -1, dtype=np.int32)
    dir_status = np.zeros((V, 5), dtype=np.int32)
    for k, ix in bins:
        Yc, pc, Wc = np.ascontiguousarray(Y[ix]), np.ascontiguousarray(pk[ix, :3 * k]), _w_chunk(W, w_stride, ix)
        if sh is not None:
            shc = np.ascontiguousarray(sh[ix])
        elif W is None:   # a voxel with a failing direction has a NaN row there and status 5 here
            fit, fst = fit2d(tables, Yc, np.full(ix.size, k), None, pc, k, False)
            shc = np.ascontiguousarray(np.where(fst[:, 0] == 0, fit[:, -2] * tables.M, 0.0))
        else:             # the weighted fit's objective; unusable weights: a NaN row there, status 3 / 4 here
            fit, fst, wst = fit2d_weighted(tables, Yc, Wc, np.full(ix.size, k), None, pc, k, False)
            with np.errstate(invalid='ignore', over='ignore'):
                sw = np.sum(Wc, axis=-1) if w_stride else np.full(ix.size, np.sum(Wc))
                shc = np.ascontiguousarray(np.where((fst[:, 0] == 0) & (wst == 0), fit[:, -2] * sw, 0.0))
        Tc = np.ascontiguousarray(2.0 * sig[ix] ** 2)
        wc, lc = np.zeros((ix.size, k, N)), np.zeros(ix.size)
        stc, dsc = np.zeros(ix.size, dtype=np.int32), np.zeros((ix.size, 5), dtype=np.int32)
        _twin("post2d", tables.handle(), L.dptr(Yc), L.opt(Wc), w_stride, L.dptr(pc), k, L.dptr(Tc), L.dptr(shc), ix.size,
              L.dptr(wc), L.dptr(lc), L.iptr(stc), L.iptr(dsc))
        w[ix, :k], log_sum[ix], status[ix], dir_status[ix] = wc, lc, stc, dsc
    return w, log_sum, status, dir_status, n_uns


def profile2d(tables, Y, K, peaks, maxfasc, partner=False, csf=None, W=None):
    """Objective profiles of a mixed set of voxels of a 2-D protocol on NumPy arrays (mfx_profile2d, one call per
    fascicle count), arguments as ``posterior2d``.  Returns ``(obj, partner, dir_status, n_unsupported)``: obj
    [V, maxfasc, N] float64 (rows of absent fascicles, of voxels out of scope and of voxels with a failing direction are
    NaN), partner [V, maxfasc, N] int32 (-1 where there is none) or None, dir_status [V, 5] int32.  ``W``: measurement
    weights [V, M] or [M] (mfx_wprofile2d): obj is the weighted sum of squares; a voxel with unusable weights has NaN rows."""
    Y, pk, maxfasc, bins, n_uns = _soft2d_host_args(tables, Y, K, peaks, maxfasc, csf)
    V, N = Y.shape[0], tables.N
    W, w_stride = _host_weights(tables.M, V, W)
    obj = np.full((V, maxfasc, N), np.nan)
    par = np.full((V, maxfasc, N), -1, dtype=np.int32) if partner else None
    dir_status = np.zeros((V, 5), dtype=np.int32)
    for k, ix in bins:
        Yc, pc = np.ascontiguousarray(Y[ix]), np.ascontiguousarray(pk[ix, :3 * k])
        o, dsc = np.zeros((ix.size, k, N)), np.zeros((ix.size, 5), dtype=np.int32)
        p = np.zeros((ix.size, k, N), dtype=np.int32) if partner else None
        Wc = _w_chunk(W, w_stride, ix)
        _twin("profile2d", tables.handle(), L.dptr(Yc), L.opt(Wc), w_stride, L.dptr(pc), k, ix.size, L.dptr(o), L.opt(p, L.iptr),
              L.iptr(dsc))
        obj[ix, :k], dir_status[ix] = o, dsc
        if partner:
            par[ix, :k] = p
    return obj, par, dir_status, n_uns


def _wfit_shapes(plan, y_shape, w_shape, pk_shape, maxfasc):
    """Argument checks shared by the weighted fit's entry points (before any device call); returns (V, w_stride)."""
    if maxfasc < 0 or maxfasc > 3:
        raise ValueError("the weighted fit is not served for maxfasc = %d: it takes 0 to 3 fascicles per voxel" % maxfasc)
    if len(y_shape) != 2 or y_shape[1] != plan.M:
        raise ValueError("data has shape %s, protocol has %d measurements" % (tuple(y_shape), plan.M))
    V = y_shape[0]
    w_stride = _w_stride(plan.M, V, w_shape)
    if tuple(pk_shape) != (V, 3 * maxfasc):
        raise ValueError("peaks should have shape (%d, %d)" % (V, 3 * maxfasc))
    return V, w_stride


def fit_weighted_dev(plan, d_Y, d_W, d_peaks, maxfasc, out=None):
    """Device-resident weighted fit (mfx_wfit_batch_dev) of ONE voxel class: every voxel has ``maxfasc`` fascicles and
    no CSF column.  torch CUDA float64 tensors d_Y [V, M], d_W [V, M] or [M] (weights >= 0 of the measurements),
    d_peaks [V, 3 maxfasc] -> (params [V, num_params(maxfasc, False, False)] f64, status [V] int32: 0 fitted, 1 a
    negative or non-finite weight, 2 no positive weight; a voxel with a non-zero status has a NaN row).  Enqueues on
    torch's current stream and returns without waiting; a direction that is not a unit vector is reported by
    mfx_plan_status as in fit_batch_dev."""
    import torch
    maxfasc = int(maxfasc)
    _f64_cuda(d_Y, d_W, d_peaks)
    V, w_stride = _wfit_shapes(plan, d_Y.shape, d_W.shape, d_peaks.shape, maxfasc)
    out = _out_like(out, (V, num_params(maxfasc, False, False)), d_Y.device)
    status = torch.empty((V,), dtype=torch.int32, device=d_Y.device)
    st = torch.cuda.current_stream(d_Y.device).cuda_stream
    L.check(L.lib().mfx_wfit_batch_dev(plan.handle(), d_Y.data_ptr(), d_W.data_ptr(), w_stride,
                                       d_peaks.data_ptr() if maxfasc > 0 else None, maxfasc, V, out.data_ptr(),
                                       status.data_ptr(), st))
    return out, status


def fit_weighted(plan, Y, W, K, csf, peaks, maxfasc, csf_on, sig_csf=None, ear=None):
    """Weighted fit of a mixed set of voxels on NumPy arrays (mfx_wfit_batch): Y [V, M], weights W [V, M] or [M] (>= 0;
    a 0/1 outlier mask, inverse noise variances, ...), fascicle counts K [V] in 0..maxfasc, CSF flags csf [V] (or None),
    peaks [V, 3 maxfasc] -> (params [V, num_params(maxfasc, csf_on, False)], status [V] int32).  Minimises
    sum_m W[v, m] (y_m - model_m)^2: the reference chain on rows scaled by sqrt(W).  status 1: a negative or non-finite
    weight, 2: no positive weight; such a voxel has a NaN row.  EAR compartments are not served with weights."""
    if ear is not None and np.any(ear):
        raise ValueError("the weighted fit is not served for voxels with an EAR compartment (%d flagged)"
                         % int(np.count_nonzero(ear)))
    Y = L.f64c(Y)
    W = L.f64c(W)
    maxfasc = int(maxfasc)
    pk = L.f64c(peaks).reshape(Y.shape[0], -1) if (maxfasc > 0 and Y.ndim == 2) else np.zeros((Y.shape[0], 0))
    V, w_stride = _wfit_shapes(plan, Y.shape, W.shape, pk.shape, maxfasc)
    K, cs, sc = _mixed_args(plan.M, V, maxfasc, K, csf, csf_on, sig_csf)
    params = np.zeros((V, num_params(maxfasc, bool(csf_on), False)))
    status = np.zeros(V, dtype=np.int32)
    L.check(L.lib().mfx_wfit_batch(plan.handle(), L.dptr(Y), L.dptr(W), w_stride, L.iptr(K), L.opt(cs, L.bptr),
                                   L.dptr(pk) if maxfasc > 0 else None, maxfasc, int(bool(csf_on)), L.opt(sc), V, L.dptr(params),
                                   L.iptr(status)))
    if V:
        L.check(L.lib().mfx_plan_status(plan.handle(), None))   # a direction that is not a unit vector: ValueError
    return params, status


ROBUST_LOSSES = {'cutoff': 0, 'huber': 1, 'tukey': 2}   # include/mfx_robust.h
ROBUST_DEFAULTS = {'loss': 'cutoff', 'c': 4.45, 'n_iter': 3}


def _robust_rule(loss, c, n_iter=0):
    """The robust rule's parameters checked (before any device call); returns (loss code, c, n_iter)."""
    if not isinstance(loss, str) or loss not in ROBUST_LOSSES:
        raise ValueError("robust loss should be one of %s, got %r" % (", ".join(repr(k) for k in ROBUST_LOSSES), loss))
    try:
        cf = float(c)
    except (TypeError, ValueError):
        raise ValueError("robust c should be a finite number >= 1, got %r" % (c,))
    if not (cf >= 1.0) or not np.isfinite(cf):
        raise ValueError("robust c should be a finite number >= 1, got %r" % (c,))
    if isinstance(n_iter, bool) or not isinstance(n_iter, (int, np.integer)) or n_iter < 0:
        raise ValueError("robust n_iter should be a non-negative integer, got %r" % (n_iter,))
    return ROBUST_LOSSES[loss], cf, int(n_iter)


def robust_options(robust):
    """MFModel.fit's ``robust`` argument -> None (the plain path) or the dict {'loss', 'c', 'n_iter'}, checked."""
    if robust is None or robust is False:
        return None
    opts = dict(ROBUST_DEFAULTS)
    if robust is not True:
        if not isinstance(robust, dict):
            raise ValueError("robust should be None, a bool or a dict with keys among 'loss', 'c', 'n_iter', got %r" % (robust,))
        unknown = sorted(set(robust) - set(opts), key=str)
        if unknown:
            raise ValueError("robust has unknown key(s) %s: it takes 'loss', 'c', 'n_iter'" % ", ".join(repr(k) for k in unknown))
        opts.update(robust)
    _robust_rule(opts['loss'], opts['c'], opts['n_iter'])
    return opts


def _robust_w_shapes(M, y_shape, p_shape, w0_shape, wprev_shape=None):
    """Argument checks of the weight rule's entry points (before any device call); returns (V, w0_stride)."""
    if len(y_shape) != 2 or y_shape[1] < 1:
        raise ValueError("data should have shape (voxels, measurements), got %s" % (tuple(y_shape),))
    V = y_shape[0]
    if M is not None and y_shape[1] != M:
        raise ValueError("data has shape %s, protocol has %d measurements" % (tuple(y_shape), M))
    M = y_shape[1]
    if p_shape is not None and tuple(p_shape) != (V, M):
        raise ValueError("prediction should have the data's shape (%d, %d), got %s" % (V, M, tuple(p_shape)))
    w0_stride = 0
    if w0_shape is not None:
        if tuple(w0_shape) == (M,):
            w0_stride = 0
        elif tuple(w0_shape) == (V, M):
            w0_stride = M
        else:
            raise ValueError("base weights should have shape (%d, %d) or (%d,), got %s (%d voxels)"
                             % (V, M, M, tuple(w0_shape), V))
    if wprev_shape is not None and tuple(wprev_shape) != (V, M):
        raise ValueError("previous weights should have shape (%d, %d), got %s" % (V, M, tuple(wprev_shape)))
    return V, w0_stride


def robust_weights_dev(d_Y, d_P, d_W0=None, loss='cutoff', c=4.45, d_Wprev=None, out=None):
    """The robust weight rule on the device (mfx_robust_weights_dev; include/mfx_robust.h states it operation by
    operation): torch CUDA float64 tensors d_Y, d_P [V, M] (data and prediction), optional base weights d_W0 [V, M] or
    [M], optional previous weights d_Wprev [V, M] -> (W [V, M], scale [V], state [V] int32, changed [V] int32 or None
    without d_Wprev).  ``loss`` 'cutoff' | 'huber' | 'tukey', ``c`` >= 1 in units of the median absolute residual.
    ``out`` may be d_Wprev itself.  Enqueues on torch's current stream and returns without waiting."""
    import torch
    code, cf, _ = _robust_rule(loss, c)
    _f64_cuda(d_Y, d_P, d_W0, d_Wprev, out)
    V, w0_stride = _robust_w_shapes(None, d_Y.shape, d_P.shape, d_W0.shape if d_W0 is not None else None,
                                    d_Wprev.shape if d_Wprev is not None else None)
    M = d_Y.shape[1]
    out = _out_like(out, (V, M), d_Y.device)
    scale = torch.empty((V,), dtype=torch.float64, device=d_Y.device)
    state = torch.empty((V,), dtype=torch.int32, device=d_Y.device)
    changed = torch.empty((V,), dtype=torch.int32, device=d_Y.device) if d_Wprev is not None else None
    st = torch.cuda.current_stream(d_Y.device).cuda_stream
    with torch.cuda.device(d_Y.device):
        L.check(L.lib().mfx_robust_weights_dev(M, d_Y.data_ptr(), d_P.data_ptr(), _tptr(d_W0), w0_stride, code, cf, V,
                                               _tptr(d_Wprev), out.data_ptr(), scale.data_ptr(), state.data_ptr(),
                                               _tptr(changed), st))
    return out, scale, state, changed


def robust_weights(Y, P, W0=None, loss='cutoff', c=4.45, Wprev=None, device=0):
    """robust_weights_dev on NumPy arrays: Y, P [V, M], W0 [V, M] | [M] | None, Wprev [V, M] | None ->
    (W [V, M], scale [V], state [V] int32, changed [V] int32 or None)."""
    _robust_rule(loss, c)
    Y, P = L.f64c(Y), L.f64c(P)
    W0, Wprev = L.f64c_opt(W0), L.f64c_opt(Wprev)
    _robust_w_shapes(None, Y.shape, P.shape, W0.shape if W0 is not None else None, Wprev.shape if Wprev is not None else None)
    if L.lib().mfx_device_count() <= 0:
        raise L.MfxError("no HIP device available (this library has no CPU path)")
    import torch
    dev = torch.device("cuda", int(device))

    def t(x):
        return torch.from_numpy(x).to(dev) if x is not None else None
    W, scale, state, changed = robust_weights_dev(t(Y), t(P), t(W0), loss, c, t(Wprev))
    return (W.cpu().numpy(), scale.cpu().numpy(), state.cpu().numpy(), changed.cpu().numpy() if changed is not None else None)


def fit_robust_dev(plan, d_Y, d_peaks, maxfasc, d_W0=None, loss='cutoff', c=4.45, n_iter=3):
    """Device-resident robust fit (mfx_rfit_batch_dev) of ONE voxel class: every voxel has ``maxfasc`` fascicles and no
    CSF column.  The plain fit (the weighted fit on the base weights d_W0 [V, M] or [M], if given), then ``n_iter``
    times: predict, reweight by the rule of ``robust_weights_dev``, weighted fit.  torch CUDA float64 tensors ->
    (params [V, num_params(maxfasc, False, False)], W [V, M], info) with info = {'scale' [V], 'state' [V] int32,
    'status' [V] int32 (the last weighted fit's), 'n_changed' [n_iter] int32}, all tensors.  Always runs all
    iterations; enqueues on torch's current stream and returns without waiting."""
    import torch
    maxfasc = int(maxfasc)
    code, cf, n_iter = _robust_rule(loss, c, n_iter)
    _f64_cuda(d_Y, d_peaks if maxfasc > 0 else None, d_W0)
    V, w0_stride = _wfit_shapes(plan, d_Y.shape, d_W0.shape if d_W0 is not None else (plan.M,),
                                d_peaks.shape if maxfasc > 0 else (d_Y.shape[0], 0), maxfasc)
    dev = d_Y.device
    params = torch.empty((V, num_params(maxfasc, False, False)), dtype=torch.float64, device=dev)
    W = torch.empty((V, plan.M), dtype=torch.float64, device=dev)
    scale = torch.empty((V,), dtype=torch.float64, device=dev)
    state = torch.empty((V,), dtype=torch.int32, device=dev)
    status = torch.empty((V,), dtype=torch.int32, device=dev)
    nch = torch.zeros((n_iter,), dtype=torch.int32, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    with torch.cuda.device(dev):
        L.check(L.lib().mfx_rfit_batch_dev(plan.handle(), d_Y.data_ptr(), _tptr(d_W0), w0_stride,
                                           d_peaks.data_ptr() if maxfasc > 0 else None, maxfasc, code, cf, n_iter, V,
                                           params.data_ptr(), W.data_ptr(), scale.data_ptr(), state.data_ptr(),
                                           status.data_ptr(), nch.data_ptr() if n_iter > 0 else None, st))
    return params, W, {'scale': scale, 'state': state, 'status': status, 'n_changed': nch}


def fit_robust(plan, Y, K, csf, peaks, maxfasc, csf_on, sig_csf=None, W0=None, loss='cutoff', c=4.45, n_iter=3, ear=None):
    """Robust fit of a mixed set of voxels on NumPy arrays (mfx_rfit_batch): Y [V, M], fascicle counts K [V] in
    0..maxfasc, CSF flags csf [V] (or None), peaks [V, 3 maxfasc], optional base weights W0 [V, M] or [M] (rows excluded
    for good, noise levels) -> (params [V, num_params(maxfasc, csf_on, False)], W [V, M], info).  The plain fit (the
    weighted fit on W0, if given), then up to ``n_iter`` times: predict, weights from the residuals by the rule of
    ``robust_weights_dev`` (``loss``, ``c``), weighted fit - with the data resident on the device throughout.  info:
    'scale' [V] the median absolute residual the last weights were made with, 'state' [V] int32 (0 reweighted, 1 no
    finite prediction, 2 scale 0, 3 unusable base weights), 'status' [V] int32 of the last weighted fit, 'n_changed'
    [n_iter] int64 voxels whose weights each iteration changed, 'n_iter_used'.  The loop may stop early once an
    iteration changed nothing; the results are those of all n_iter iterations.  EAR compartments are not served."""
    if ear is not None and np.any(ear):
        raise ValueError("the robust fit is not served for voxels with an EAR compartment (%d flagged)"
                         % int(np.count_nonzero(ear)))
    code, cf, n_iter = _robust_rule(loss, c, n_iter)
    Y = L.f64c(Y)
    W0 = L.f64c_opt(W0)
    maxfasc = int(maxfasc)
    pk = L.f64c(peaks).reshape(Y.shape[0], -1) if (maxfasc > 0 and Y.ndim == 2) else np.zeros((Y.shape[0], 0))
    V, w0_stride = _wfit_shapes(plan, Y.shape, W0.shape if W0 is not None else (plan.M,), pk.shape, maxfasc)
    K, cs, sc = _mixed_args(plan.M, V, maxfasc, K, csf, csf_on, sig_csf, need_sig=True)
    M = plan.M
    params = np.zeros((V, num_params(maxfasc, bool(csf_on), False)))
    W = np.zeros((V, M))
    scale = np.zeros(V)
    state = np.zeros(V, dtype=np.int32)
    status = np.zeros(V, dtype=np.int32)
    nch = np.zeros(max(n_iter, 1), dtype=np.int64)
    used = np.zeros(1, dtype=np.int32)
    L.check(L.lib().mfx_rfit_batch(plan.handle(), L.dptr(Y), L.opt(W0), w0_stride, L.iptr(K), L.opt(cs, L.bptr),
                                   L.dptr(pk) if maxfasc > 0 else None, maxfasc, int(bool(csf_on)), L.opt(sc), code, cf, n_iter,
                                   V, L.dptr(params), L.dptr(W), L.dptr(scale), L.iptr(state), L.iptr(status), L.lptr(nch),
                                   L.iptr(used)))
    if V:
        L.check(L.lib().mfx_plan_status(plan.handle(), None))   # a direction that is not a unit vector: ValueError
    return params, W, {'scale': scale, 'state': state, 'status': status, 'n_changed': nch[:n_iter].copy(),
                       'n_iter_used': int(used[0])}


def fit2d_robust_dev(tables, d_Y, d_peaks, maxfasc, d_W0=None, loss='cutoff', c=4.45, n_iter=3):
    """Device-resident robust fit of voxels of a 2-D protocol (mfx_rfit2d_batch_dev, include/mfx_robust2d.h) for a
    mf_utils.RotateAtom2DTables and ONE voxel class: every voxel has ``maxfasc`` fascicles and no CSF column.  The loop of
    ``fit_robust_dev`` on ``fit2d_dev``, ``predict2d_dev`` and ``fit2d_weighted_dev``, with the directions' plan made
    once.  torch CUDA float64 tensors -> (params [V, num_params(maxfasc, False, False)], W [V, M], info) with info =
    {'scale' [V], 'state' [V] int32, 'dir_status' [V, 5] int32, 'status' [V] int32 (the last weighted fit's weight
    status), 'n_changed' [n_iter] int32}, all tensors.  Always runs all iterations; enqueues on torch's current stream
    and returns without waiting."""
    import torch
    maxfasc = int(maxfasc)
    code, cf, n_iter = _robust_rule(loss, c, n_iter)
    _f64_cuda(d_Y, d_peaks if maxfasc > 0 else None, d_W0)
    V = _fit2d_shapes(tables, d_Y.shape, d_peaks.shape if maxfasc > 0 else (d_Y.shape[0], 0), maxfasc)
    w0_stride = _w_stride(tables.M, V, d_W0.shape) if d_W0 is not None else 0
    dev = d_Y.device
    params = torch.empty((V, num_params(maxfasc, False, False)), dtype=torch.float64, device=dev)
    W = torch.empty((V, tables.M), dtype=torch.float64, device=dev)
    scale = torch.empty((V,), dtype=torch.float64, device=dev)
    state = torch.empty((V,), dtype=torch.int32, device=dev)
    dstat = torch.empty((V, 5), dtype=torch.int32, device=dev)
    wstat = torch.empty((V,), dtype=torch.int32, device=dev)
    nch = torch.zeros((n_iter,), dtype=torch.int32, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    L.check(L.lib().mfx_rfit2d_batch_dev(tables.handle(), d_Y.data_ptr(), _tptr(d_W0), w0_stride,
                                         d_peaks.data_ptr() if maxfasc > 0 else None, maxfasc, code, cf, n_iter, V,
                                         params.data_ptr(), W.data_ptr(), scale.data_ptr(), state.data_ptr(), dstat.data_ptr(),
                                         wstat.data_ptr(), nch.data_ptr() if n_iter > 0 else None, st))
    return params, W, {'scale': scale, 'state': state, 'dir_status': dstat, 'status': wstat, 'n_changed': nch}


def fit2d_robust(tables, Y, K, csf, peaks, maxfasc, csf_on, sig_csf=None, W0=None, loss='cutoff', c=4.45, n_iter=3):
    """Robust fit of a mixed set of voxels of a 2-D protocol on NumPy arrays (mfx_rfit2d_batch): arguments as ``fit2d``,
    optional base weights W0 [V, M] or [M] -> (params, W [V, M], info).  The plain fit (the weighted fit on W0, if given),
    then up to ``n_iter`` times: predict, weights from the residuals by the rule of ``robust_weights_dev`` (``loss``,
    ``c``), weighted fit - with the data resident on the device throughout and the directions' plan made once per class.
    info is ``fit_robust``'s dict - 'scale', 'state', 'status' [V] int32 (the last weighted fit's weight status),
    'n_changed' [n_iter] int64, 'n_iter_used' - plus 'dir_status' [V, 5] int32: a voxel with a failing direction has a NaN
    row, state 1, its base weights and its record there.  The loop may stop early once an iteration changed nothing; the
    results are those of all n_iter iterations."""
    code, cf, n_iter = _robust_rule(loss, c, n_iter)
    Y = L.f64c(Y)
    W0 = L.f64c_opt(W0)
    maxfasc = int(maxfasc)
    pk = L.f64c(peaks).reshape(Y.shape[0], -1) if (maxfasc > 0 and Y.ndim == 2) else np.zeros((Y.shape[0], 0))
    V = _fit2d_shapes(tables, Y.shape, pk.shape, maxfasc)
    w0_stride = _w_stride(tables.M, V, W0.shape) if W0 is not None else 0
    K, cs, sc = _mixed_args(tables.M, V, maxfasc, K, csf, csf_on, sig_csf, need_sig=True)
    M = tables.M
    params = np.zeros((V, num_params(maxfasc, bool(csf_on), False)))
    W = np.zeros((V, M))
    scale = np.zeros(V)
    state = np.zeros(V, dtype=np.int32)
    dstat = np.zeros((V, 5), dtype=np.int32)
    wstat = np.zeros(V, dtype=np.int32)
    nch = np.zeros(max(n_iter, 1), dtype=np.int64)
    used = np.zeros(1, dtype=np.int32)
    L.check(L.lib().mfx_rfit2d_batch(tables.handle(), L.dptr(Y), L.opt(W0), w0_stride, L.iptr(K), L.opt(cs, L.bptr),
                                     L.dptr(pk) if maxfasc > 0 else None, maxfasc, int(bool(csf_on)), L.opt(sc), code, cf, n_iter, V,
                                     L.dptr(params), L.dptr(W), L.dptr(scale), L.iptr(state), L.iptr(dstat), L.iptr(wstat),
                                     L.lptr(nch), L.iptr(used)))
    return params, W, {'scale': scale, 'state': state, 'status': wstat, 'dir_status': dstat,
                       'n_changed': nch[:n_iter].copy(), 'n_iter_used': int(used[0])}


BOOT_KINDS = {'wild': 0, 'residual': 1}   # include/mfx_boot.h
BOOT_MAX_B, BOOT_MAX_Q, BOOT_NSTAT = 4096, 32, 5
BOOT_DEFAULT_BYTES = 256 << 20


def boot_columns(maxfasc, csf_on, ear_on, nprop=0):
    """The column names of the bootstrap's value table for a parameter layout (include/mfx_boot.h): 'M0', 'nu_k',
    'nu_csf', 'nu_ear', 'MSE', then ('prop', k, t) for fascicle k and property table t."""
    cols = ['M0'] + ['nu_%d' % k for k in range(int(maxfasc))]
    cols += ['nu_csf'] if csf_on else []
    cols += ['nu_ear'] if ear_on else []
    cols.append('MSE')
    return cols + [('prop', k, t) for k in range(int(maxfasc)) for t in range(int(nprop))]


def boot_groups(scheme):
    """The default groups of the residual bootstrap: int32 [M], rows sharing (G, Delta, delta) share a group."""
    sch = L.f64c(scheme)
    if sch.ndim != 2 or sch.shape[1] != 7:
        raise ValueError("pgse_scheme should have 7 columns")
    return np.ascontiguousarray(np.unique(sch[:, 3:6], axis=0, return_inverse=True)[1].reshape(-1), dtype=np.int32)


def _boot_rule(B, kind, q=(), seed=0, offset=0, reduce=True):
    """The bootstrap's options checked (before any device call); returns (B, kind code, q float64 [Q])."""
    if isinstance(B, bool) or not isinstance(B, (int, np.integer)) or B < 1:
        raise ValueError("bootstrap B should be an integer >= 1, got %r" % (B,))
    if not isinstance(kind, str) or kind not in BOOT_KINDS:
        raise ValueError("bootstrap kind should be one of %s, got %r" % (", ".join(repr(k) for k in BOOT_KINDS), kind))
    try:
        qa = np.ascontiguousarray(np.atleast_1d(np.asarray(q, dtype=np.float64)).reshape(-1))
    except (TypeError, ValueError):
        raise ValueError("bootstrap q should be numbers in [0, 1], got %r" % (q,))
    if qa.size and not np.all((qa >= 0.0) & (qa <= 1.0)):
        raise ValueError("bootstrap q should lie in [0, 1], got %r" % (q,))
    for name, x in (("seed", seed), ("offset", offset)):
        if isinstance(x, bool) or not isinstance(x, (int, np.integer)):
            raise ValueError("bootstrap %s should be an integer, got %r" % (name, x))
    if reduce and B > BOOT_MAX_B:
        raise NotImplementedError("at most %d bootstrap replicates are reduced on the device (got B = %d)" % (BOOT_MAX_B, B))
    if qa.size > BOOT_MAX_Q:
        raise NotImplementedError("at most %d bootstrap quantiles (got %d)" % (BOOT_MAX_Q, qa.size))
    return int(B), BOOT_KINDS[kind], qa


def _boot_groups_arg(kind, groups, M, scheme):
    """int32 [M] groups of the residual bootstrap (None for the wild one): given, or the default from the scheme."""
    if kind != 1:
        return None
    if groups is None:
        if scheme is None:
            raise ValueError("the residual bootstrap needs groups (the plan knows no scheme to derive them from)")
        groups = boot_groups(scheme)
    g = np.asarray(groups)
    if g.shape != (M,) or g.dtype.kind not in 'iu':
        raise ValueError("groups should be %d integers (one per measurement), got shape %s" % (M, g.shape))
    return np.ascontiguousarray(g, dtype=np.int32)


def boot_resample_dev(d_Y, d_P, d_params, maxfasc, csf_on=False, ear_on=False, B=200, kind='wild', seed=0, inflate=True,
                      offset=0, d_groups=None, d_peaks=None, d_vox=None):
    """The bootstrap's resampling rule on the device (mfx_boot_resample_dev; include/mfx_boot.h states it operation by
    operation): torch CUDA float64 tensors d_Y, d_P [V, M] (data and the prediction of the voxels' own fit), d_params
    [V, num_params] (their parameter rows: the number of positive weights scales the residuals with ``inflate``),
    optional d_peaks [V, 3 maxfasc], d_groups [M] int32 (kind 'residual'), d_vox [V] int64 (batch indices, default
    0..V-1) -> (Ystar [V, B, M], peaks [V B, 3 maxfasc] or None, status [V] int32).  Enqueues on torch's current stream
    and returns without waiting."""
    import torch
    B, code, _ = _boot_rule(B, kind, (), seed, offset, reduce=False)
    maxfasc = int(maxfasc)
    if maxfasc < 0 or maxfasc > 3:
        raise ValueError("maxfasc must be 0..3")
    _f64_cuda(d_Y, d_P, d_params, d_peaks)
    if d_Y.dim() != 2 or d_Y.shape[1] < 1:
        raise ValueError("data should have shape (voxels, measurements), got %s" % (tuple(d_Y.shape),))
    V, M = d_Y.shape
    if tuple(d_P.shape) != (V, M):
        raise ValueError("prediction should have the data's shape (%d, %d), got %s" % (V, M, tuple(d_P.shape)))
    npar = num_params(maxfasc, csf_on, ear_on)
    if tuple(d_params.shape) != (V, npar):
        raise ValueError("params should have shape (%d, %d), got %s" % (V, npar, tuple(d_params.shape)))
    if d_peaks is not None and (maxfasc == 0 or tuple(d_peaks.shape) != (V, 3 * maxfasc)):
        raise ValueError("peaks should have shape (%d, %d)" % (V, 3 * maxfasc))
    if code == 1:
        if d_groups is None:
            raise ValueError("the residual bootstrap needs groups")
        assert d_groups.is_cuda and d_groups.dtype == torch.int32 and d_groups.is_contiguous()
        if tuple(d_groups.shape) != (M,):
            raise ValueError("groups should be %d integers (one per measurement), got shape %s" % (M, tuple(d_groups.shape)))
    if d_vox is not None:
        assert d_vox.is_cuda and d_vox.dtype == torch.int64 and d_vox.is_contiguous()
        if tuple(d_vox.shape) != (V,):
            raise ValueError("vox should have one entry per voxel")
    dev = d_Y.device
    Ys = torch.empty((V, B, M), dtype=torch.float64, device=dev)
    pk = torch.empty((V * B, 3 * maxfasc), dtype=torch.float64, device=dev) if d_peaks is not None else None
    status = torch.empty((V,), dtype=torch.int32, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    with torch.cuda.device(dev):
        L.check(L.lib().mfx_boot_resample_dev(M, d_Y.data_ptr(), d_P.data_ptr(), d_params.data_ptr(), maxfasc, int(bool(csf_on)),
                                              int(bool(ear_on)), _tptr(d_peaks), d_groups.data_ptr() if code == 1 else None,
                                              _tptr(d_vox), V, B, code, int(bool(inflate)), int(seed) & _U64,
                                              int(offset) & _U64, Ys.data_ptr(), _tptr(pk), status.data_ptr(), st))
    return Ys, pk, status


def boot_reduce_dev(d_X, d_valid, q=()):
    """The bootstrap's statistics on the device (mfx_boot_reduce_dev): torch CUDA tensors d_X [V, B, C] float64 and d_valid
    [V, B, C] uint8 or bool -> stats [V, C, 5 + Q] float64: per voxel and column over the valid replicates the count, the
    mean (serial sum in replicate order), the standard deviation (two-pass, ddof = 1), the smallest and largest value and
    the quantiles ``q`` by linear interpolation.  Enqueues on torch's current stream and returns without waiting."""
    import torch
    if d_X.dim() != 3 or d_X.shape[1] < 1 or d_X.shape[2] < 1:
        raise ValueError("X should have shape (voxels, replicates, columns), got %s" % (tuple(d_X.shape),))
    V, B, Cn = d_X.shape
    _, _, qa = _boot_rule(B, 'wild', q)
    if tuple(d_valid.shape) != (V, B, Cn):
        raise ValueError("valid should have the shape of X %s, got %s" % ((V, B, Cn), tuple(d_valid.shape)))
    _f64_cuda(d_X)
    assert d_valid.is_cuda and d_valid.dtype in (torch.uint8, torch.bool) and d_valid.is_contiguous()
    dev = d_X.device
    d_q = torch.from_numpy(qa).to(dev) if qa.size else None
    stats = torch.empty((V, Cn, BOOT_NSTAT + qa.size), dtype=torch.float64, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    with torch.cuda.device(dev):
        L.check(L.lib().mfx_boot_reduce_dev(d_X.data_ptr(), d_valid.data_ptr(), V, B, Cn, _tptr(d_q), int(qa.size), stats.data_ptr(),
                                            st))
    return stats


def fit_bootstrap_dev(plan, d_Y, d_peaks, maxfasc, csf_on=False, ear_on=False, d_sig_csf=None, d_sig_ear=None, E=0, B=200,
                      kind='wild', seed=0, inflate=True, offset=0, q=(0.025, 0.975), d_props=None, d_groups=None, d_params=None,
                      d_pred=None, d_vox=None, max_bytes=BOOT_DEFAULT_BYTES, keep=False):
    """Device-resident bootstrap (mfx_boot_fit_dev) of ONE voxel class (every voxel: K == maxfasc, csf == csf_on,
    ear == ear_on), torch CUDA tensors as ``fit_batch_dev`` takes them.  The voxels' own fit (``d_params`` [V, num_params],
    fitted here if None) is predicted (``d_pred`` [V, M] if given), its residuals are resampled into B replicates per
    voxel by the rule of ``boot_resample_dev``, the replicates are fitted by ``fit_batch_dev``'s kernels and reduced:
    returns {'stats' [V, C, 5 + Q], 'agree' [V, maxfasc] int32, 'status' [V] int32, 'replicates' [V, B, num_params] or
    None (``keep``), 'columns' (``boot_columns``)}; d_props [nprop, N] are the property tables whose values at the chosen
    atoms become columns.  Voxel chunks keep the replicate signals within ``max_bytes``.  Enqueues on torch's current
    stream and returns without waiting; a direction that is not a unit vector is reported by mfx_plan_status."""
    import torch
    B, code, qa = _boot_rule(B, kind, q, seed, offset)
    maxfasc = int(maxfasc)
    if maxfasc < 0 or maxfasc > 3:
        raise ValueError("maxfasc must be 0..3")
    _f64_cuda(d_Y, d_peaks if maxfasc > 0 else None, d_sig_csf if csf_on else None, d_sig_ear if ear_on else None, d_props,
              d_params, d_pred)
    if d_Y.dim() != 2 or d_Y.shape[1] != plan.M:
        raise ValueError("data should have shape (voxels, %d), got %s" % (plan.M, tuple(d_Y.shape)))
    V, M = d_Y.shape
    npar = num_params(maxfasc, csf_on, ear_on)
    if maxfasc > 0 and (d_peaks is None or tuple(d_peaks.shape) != (V, 3 * maxfasc)):
        raise ValueError("peaks should have shape (%d, %d)" % (V, 3 * maxfasc))
    if csf_on and (d_sig_csf is None or d_sig_csf.numel() != M):
        raise ValueError("csf_on needs sig_csf with %d entries" % M)
    if ear_on and (d_sig_ear is None or tuple(d_sig_ear.shape) != (M, E) or E < 1):
        raise ValueError("sig_ear should have shape (%d, E) with E >= 1" % M)
    if d_params is not None and tuple(d_params.shape) != (V, npar):
        raise ValueError("params should have shape (%d, %d), got %s" % (V, npar, tuple(d_params.shape)))
    if d_pred is not None and (d_params is None or tuple(d_pred.shape) != (V, M)):
        raise ValueError("a prediction needs the parameters it was made from and the data's shape (%d, %d)" % (V, M))
    nprop = 0
    if d_props is not None:
        if d_props.dim() != 2 or d_props.shape[1] != plan.tables.N:
            raise ValueError("props should have shape (nprop, %d), got %s" % (plan.tables.N, tuple(d_props.shape)))
        nprop = int(d_props.shape[0])
    dev = d_Y.device
    if code == 1 and d_groups is None:
        d_groups = torch.from_numpy(_boot_groups_arg(code, None, M, plan.scheme)).to(dev)
    if code == 1:
        assert d_groups.is_cuda and d_groups.dtype == torch.int32 and d_groups.is_contiguous()
        if tuple(d_groups.shape) != (M,):
            raise ValueError("groups should be %d integers (one per measurement), got shape %s" % (M, tuple(d_groups.shape)))
    if d_vox is not None:
        assert d_vox.is_cuda and d_vox.dtype == torch.int64 and d_vox.is_contiguous()
        if tuple(d_vox.shape) != (V,):
            raise ValueError("vox should have one entry per voxel")
    cols = boot_columns(maxfasc, csf_on, ear_on, nprop)
    d_q = torch.from_numpy(qa).to(dev) if qa.size else None
    stats = torch.empty((V, len(cols), BOOT_NSTAT + qa.size), dtype=torch.float64, device=dev)
    agree = torch.zeros((V, maxfasc), dtype=torch.int32, device=dev)
    status = torch.zeros((V,), dtype=torch.int32, device=dev)
    reps = torch.empty((V, B, npar), dtype=torch.float64, device=dev) if keep else None
    st = torch.cuda.current_stream(dev).cuda_stream
    with torch.cuda.device(dev):
        L.check(L.lib().mfx_boot_fit_dev(plan.handle(), d_Y.data_ptr(), _tptr(d_peaks) if maxfasc > 0 else None, maxfasc,
                                         int(bool(csf_on)), int(bool(ear_on)), _tptr(d_sig_csf) if csf_on else None,
                                         _tptr(d_sig_ear) if ear_on else None, int(E), _tptr(d_params), _tptr(d_pred),
                                         _tptr(d_groups) if code == 1 else None, _tptr(d_vox), V, B, code, int(bool(inflate)),
                                         int(seed) & _U64, int(offset) & _U64, _tptr(d_props), nprop, _tptr(d_q), int(qa.size),
                                         int(max_bytes), stats.data_ptr(), agree.data_ptr() if maxfasc > 0 else None,
                                         status.data_ptr(), _tptr(reps), st))
    return {'stats': stats, 'agree': agree, 'status': status, 'replicates': reps, 'columns': cols}


def fit_bootstrap(plan, Y, K, csf, ear, peaks, maxfasc, csf_on, ear_on, sig_csf=None, sig_ear=None, E=0, B=200, kind='wild',
                  seed=0, inflate=True, offset=0, q=(0.025, 0.975), props=None, groups=None, params=None, vox=None,
                  max_bytes=BOOT_DEFAULT_BYTES, keep=False):
    """Bootstrap of a mixed set of voxels on NumPy arrays (mfx_boot_fit), arguments as ``fit_batch`` takes them: every
    voxel class of the plain fit is served (K in 0..maxfasc, CSF, EAR).  ``params`` [V, num_params]: the voxels' own fit
    (fitted here if None); ``vox`` [V] int64: the voxels' batch indices (default 0..V-1) - the random stream is keyed by
    them, so a subset gives the replicates the whole batch gives; ``props`` [nprop, N]: property tables; ``groups`` [M]:
    the residual bootstrap's groups (default ``boot_groups`` of the plan's scheme).  Returns {'stats' [V, C, 5 + Q]
    (count, mean, std, min, max, quantiles per column of ``boot_columns``), 'agree' [V, maxfasc] int32 (replicates that
    chose the original atom with a positive weight), 'status' [V] int32 (0 fine, 1 no degree of freedom, 2 original row
    not usable), 'replicates' [V, B, num_params] or None (``keep``), 'columns'}."""
    B, code, qa = _boot_rule(B, kind, q, seed, offset)
    maxfasc = int(maxfasc)
    if maxfasc < 0 or maxfasc > 3:
        raise ValueError("maxfasc must be 0..3")
    Y = L.f64c(Y)
    if Y.ndim != 2 or Y.shape[1] != plan.M:
        raise ValueError("data should have shape (voxels, %d), got %s" % (plan.M, Y.shape))
    V, M = Y.shape
    csf_on, ear_on = bool(csf_on), bool(ear_on)
    npar = num_params(maxfasc, csf_on, ear_on)
    K = _k_arg(V, maxfasc, K)
    flags = []
    for name, f, on in (("csf", csf, csf_on), ("ear", ear, ear_on)):
        a = None
        if f is not None:
            a = np.ascontiguousarray(np.asarray(f).reshape(-1).astype(bool), dtype=np.uint8)
            if a.shape != (V,):
                raise ValueError("%s should have one entry per voxel" % name)
            if a.any() and not on:
                raise ValueError("voxels flagged %s need %s_on" % (name.upper(), name))
        flags.append(a)
    pk = None
    if maxfasc > 0:
        pk = L.f64c(peaks).reshape(V, -1)
        if pk.shape != (V, 3 * maxfasc):
            raise ValueError("peaks should have shape (%d, %d)" % (V, 3 * maxfasc))
    sc = L.f64c(sig_csf).reshape(-1) if sig_csf is not None else None
    se = L.f64c_opt(sig_ear)
    if csf_on and (sc is None or sc.shape[0] != M):
        raise ValueError("csf_on needs sig_csf with %d entries" % M)
    if ear_on and (se is None or se.shape != (M, E) or E < 1):
        raise ValueError("sig_ear should have shape (%d, E) with E >= 1" % M)
    p0 = None
    if params is not None:
        p0 = L.f64c(params)
        if p0.shape != (V, npar):
            raise ValueError("params should have shape (%d, %d), got %s" % (V, npar, p0.shape))
    vx = None
    if vox is not None:
        vx = np.ascontiguousarray(np.asarray(vox).reshape(-1), dtype=np.int64)
        if vx.shape != (V,):
            raise ValueError("vox should have one entry per voxel")
    pr, nprop = None, 0
    if props is not None:
        pr = np.atleast_2d(L.f64c(props))
        N = getattr(getattr(plan, 'tables', None), 'N', pr.shape[1])
        if pr.ndim != 2 or pr.shape[1] != N:
            raise ValueError("props should have shape (nprop, %d), got %s" % (N, pr.shape))
        nprop = pr.shape[0]
    gr = _boot_groups_arg(code, groups, M, getattr(plan, 'scheme', None))
    cols = boot_columns(maxfasc, csf_on, ear_on, nprop)
    stats = np.zeros((V, len(cols), BOOT_NSTAT + qa.size))
    agree = np.zeros((V, maxfasc), dtype=np.int32)
    status = np.zeros(V, dtype=np.int32)
    reps = np.zeros((V, B, npar)) if keep else None
    L.check(L.lib().mfx_boot_fit(plan.handle(), L.dptr(Y), L.iptr(K), L.opt(flags[0], L.bptr), L.opt(flags[1], L.bptr), L.opt(pk),
                                 maxfasc, int(csf_on), int(ear_on), L.opt(sc) if csf_on else None,
                                 L.opt(se) if ear_on else None, int(E), L.opt(p0), L.opt(gr, L.iptr), L.opt(vx, L.lptr), V, B,
                                 code, int(bool(inflate)), int(seed) & _U64, int(offset) & _U64, L.opt(pr), nprop,
                                 L.dptr(qa) if qa.size else None, int(qa.size), int(max_bytes), L.dptr(stats),
                                 L.iptr(agree) if maxfasc > 0 else None, L.iptr(status), L.opt(reps)))
    if V:
        L.check(L.lib().mfx_plan_status(plan.handle(), None))   # a direction that is not a unit vector: ValueError
    return {'stats': stats, 'agree': agree, 'status': status, 'replicates': reps, 'columns': cols}


def _wboot_dev_opts(M, V, code, d_groups, d_vox, scheme=None, dev=None):
    """The optional device arguments of the weighted bootstrap's entry points, checked: the groups of the residual kind
    (int32 [M]; derived from ``scheme`` where one is given and d_groups is not) and the batch indices (int64 [V])."""
    import torch
    if code == 1:
        if d_groups is None:
            if scheme is None:
                raise ValueError("the residual bootstrap needs groups")
            d_groups = torch.from_numpy(_boot_groups_arg(code, None, M, scheme)).to(dev)
        assert d_groups.is_cuda and d_groups.dtype == torch.int32 and d_groups.is_contiguous()
        if tuple(d_groups.shape) != (M,):
            raise ValueError("groups should be %d integers (one per measurement), got shape %s" % (M, tuple(d_groups.shape)))
    if d_vox is not None:
        assert d_vox.is_cuda and d_vox.dtype == torch.int64 and d_vox.is_contiguous()
        if tuple(d_vox.shape) != (V,):
            raise ValueError("vox should have one entry per voxel")
    return d_groups


def wboot_resample_dev(d_Y, d_P, d_W, d_params, maxfasc, csf_on=False, B=200, kind='wild', seed=0, inflate=True, offset=0,
                       d_groups=None, d_peaks=None, d_vox=None):
    """The resampling rule of the bootstrap conditional on measurement weights, on the device (mfx_wboot_resample_dev;
    include/mfx_wboot.h states it operation by operation): ``boot_resample_dev`` with weights d_W [V, M] or [M] (>= 0) and
    parameter rows d_params [V, num_params(maxfasc, csf_on, False)] of the weighted fit.  A row of weight 0 is left as
    measured; the wild kind flips the residuals of the other rows; the residual kind draws among the rows of positive
    weight of a group, in units of sqrt(W).  -> (Ystar [V, B, M], peaks [V B, 3 maxfasc] or None, status [V] int32: 0 fine,
    1 no degree of freedom among the rows of positive weight, 2 data or prediction not finite, 3 a weight negative or
    not finite, 4 no positive weight).  Enqueues on torch's current stream and returns without waiting."""
    import torch
    B, code, _ = _boot_rule(B, kind, (), seed, offset, reduce=False)
    maxfasc = int(maxfasc)
    if maxfasc < 0 or maxfasc > 3:
        raise ValueError("maxfasc must be 0..3")
    _f64_cuda(d_Y, d_P, d_W, d_params, d_peaks)
    if d_Y.dim() != 2 or d_Y.shape[1] < 1:
        raise ValueError("data should have shape (voxels, measurements), got %s" % (tuple(d_Y.shape),))
    V, M = d_Y.shape
    if tuple(d_P.shape) != (V, M):
        raise ValueError("prediction should have the data's shape (%d, %d), got %s" % (V, M, tuple(d_P.shape)))
    w_stride = _w_stride(M, V, d_W.shape)
    npar = num_params(maxfasc, csf_on, False)
    if tuple(d_params.shape) != (V, npar):
        raise ValueError("params should have shape (%d, %d), got %s" % (V, npar, tuple(d_params.shape)))
    if d_peaks is not None and (maxfasc == 0 or tuple(d_peaks.shape) != (V, 3 * maxfasc)):
        raise ValueError("peaks should have shape (%d, %d)" % (V, 3 * maxfasc))
    d_groups = _wboot_dev_opts(M, V, code, d_groups, d_vox)
    dev = d_Y.device
    Ys = torch.empty((V, B, M), dtype=torch.float64, device=dev)
    pk = torch.empty((V * B, 3 * maxfasc), dtype=torch.float64, device=dev) if d_peaks is not None else None
    status = torch.empty((V,), dtype=torch.int32, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    with torch.cuda.device(dev):
        L.check(L.lib().mfx_wboot_resample_dev(M, d_Y.data_ptr(), d_P.data_ptr(), d_W.data_ptr(), w_stride, d_params.data_ptr(),
                                               maxfasc, int(bool(csf_on)), _tptr(d_peaks), _tptr(d_groups) if code == 1 else None,
                                               _tptr(d_vox), V, B, code, int(bool(inflate)), int(seed) & _U64, int(offset) & _U64,
                                               Ys.data_ptr(), _tptr(pk), status.data_ptr(), st))
    return Ys, pk, status


def fit_weighted_replicates_dev(plan, d_Ystar, d_W, d_peaks, maxfasc):
    """The replicate weighted fit on the device (mfx_wboot_fit_rows_dev, include/mfx_wboot.h) of ONE voxel class (every
    voxel ``maxfasc`` fascicles, no CSF column): B signals per voxel on the voxel's weights and directions.  torch CUDA
    float64 tensors d_Ystar [V, B, M], d_W [V, M] or [M], d_peaks [V, 3 maxfasc] -> (params [V, B, num_params(maxfasc,
    False, False)], status [V] int32 as ``fit_weighted_dev`` gives it for the voxel's weights).  Every row equals, bit for
    bit, the row ``fit_weighted_dev`` returns for that signal with those weights and directions; for two fascicles the
    weighted cross-Gram of a voxel is formed once, not once per row.  Enqueues on torch's current stream and returns
    without waiting."""
    import torch
    maxfasc = int(maxfasc)
    _f64_cuda(d_Ystar, d_W, d_peaks if maxfasc > 0 else None)
    if d_Ystar.dim() != 3 or d_Ystar.shape[1] < 1:
        raise ValueError("replicate signals should have shape (voxels, B >= 1, %d), got %s" % (plan.M, tuple(d_Ystar.shape)))
    V, B, M = d_Ystar.shape
    _, w_stride = _wfit_shapes(plan, (V, M), d_W.shape, d_peaks.shape if maxfasc > 0 else (V, 0), maxfasc)
    dev = d_Ystar.device
    out = torch.empty((V, B, num_params(maxfasc, False, False)), dtype=torch.float64, device=dev)
    status = torch.empty((V,), dtype=torch.int32, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    with torch.cuda.device(dev):
        L.check(L.lib().mfx_wboot_fit_rows_dev(plan.handle(), d_Ystar.data_ptr(), d_W.data_ptr(), w_stride,
                                               _tptr(d_peaks) if maxfasc > 0 else None, maxfasc, V, B, out.data_ptr(),
                                               status.data_ptr(), st))
    return out, status


def fit_weighted_bootstrap_dev(plan, d_Y, d_W, d_peaks, maxfasc, csf_on=False, d_sig_csf=None, B=200, kind='wild', seed=0,
                               inflate=True, offset=0, q=(0.025, 0.975), d_props=None, d_groups=None, d_params=None, d_pred=None,
                               d_vox=None, max_bytes=BOOT_DEFAULT_BYTES, keep=False):
    """Device-resident bootstrap conditional on measurement weights (mfx_wboot_fit_dev) of ONE voxel class (every voxel:
    K == maxfasc, csf == csf_on), arguments as ``fit_bootstrap_dev`` takes them, without EAR, plus the weights d_W [V, M]
    or [M].  The weights are held fixed: the own weighted fit (``d_params``, fitted here if None) is predicted, its
    residuals are resampled by the rule of ``wboot_resample_dev``, the replicates are fitted with the same weights
    (``fit_weighted_replicates_dev``) and reduced.  Returns the dict of ``fit_bootstrap_dev`` (the MSE column is the
    weighted MSE; status as ``wboot_resample_dev``).  Enqueues on torch's current stream and returns without waiting."""
    import torch
    B, code, qa = _boot_rule(B, kind, q, seed, offset)
    maxfasc = int(maxfasc)
    _f64_cuda(d_Y, d_W, d_peaks if maxfasc > 0 else None, d_sig_csf if csf_on else None, d_props, d_params, d_pred)
    V, w_stride = _wfit_shapes(plan, d_Y.shape, d_W.shape, d_peaks.shape if maxfasc > 0 else (d_Y.shape[0], 0), maxfasc)
    M = plan.M
    npar = num_params(maxfasc, csf_on, False)
    if csf_on and (d_sig_csf is None or d_sig_csf.numel() != M):
        raise ValueError("csf_on needs sig_csf with %d entries" % M)
    if d_params is not None and tuple(d_params.shape) != (V, npar):
        raise ValueError("params should have shape (%d, %d), got %s" % (V, npar, tuple(d_params.shape)))
    if d_pred is not None and (d_params is None or tuple(d_pred.shape) != (V, M)):
        raise ValueError("a prediction needs the parameters it was made from and the data's shape (%d, %d)" % (V, M))
    nprop = 0
    if d_props is not None:
        if d_props.dim() != 2 or d_props.shape[1] != plan.tables.N:
            raise ValueError("props should have shape (nprop, %d), got %s" % (plan.tables.N, tuple(d_props.shape)))
        nprop = int(d_props.shape[0])
    dev = d_Y.device
    d_groups = _wboot_dev_opts(M, V, code, d_groups, d_vox, plan.scheme, dev)
    cols = boot_columns(maxfasc, csf_on, False, nprop)
    d_q = torch.from_numpy(qa).to(dev) if qa.size else None
    stats = torch.empty((V, len(cols), BOOT_NSTAT + qa.size), dtype=torch.float64, device=dev)
    agree = torch.zeros((V, maxfasc), dtype=torch.int32, device=dev)
    status = torch.zeros((V,), dtype=torch.int32, device=dev)
    reps = torch.empty((V, B, npar), dtype=torch.float64, device=dev) if keep else None
    st = torch.cuda.current_stream(dev).cuda_stream
    with torch.cuda.device(dev):
        L.check(L.lib().mfx_wboot_fit_dev(plan.handle(), d_Y.data_ptr(), d_W.data_ptr(), w_stride,
                                          _tptr(d_peaks) if maxfasc > 0 else None, maxfasc, int(bool(csf_on)),
                                          _tptr(d_sig_csf) if csf_on else None, _tptr(d_params), _tptr(d_pred),
                                          _tptr(d_groups) if code == 1 else None, _tptr(d_vox), V, B, code, int(bool(inflate)),
                                          int(seed) & _U64, int(offset) & _U64, _tptr(d_props), nprop, _tptr(d_q), int(qa.size),
                                          int(max_bytes), stats.data_ptr(), agree.data_ptr() if maxfasc > 0 else None,
                                          status.data_ptr(), _tptr(reps), st))
    return {'stats': stats, 'agree': agree, 'status': status, 'replicates': reps, 'columns': cols}


def fit_weighted_bootstrap(plan, Y, W, K, csf, peaks, maxfasc, csf_on, sig_csf=None, B=200, kind='wild', seed=0, inflate=True,
                           offset=0, q=(0.025, 0.975), props=None, groups=None, params=None, vox=None,
                           max_bytes=BOOT_DEFAULT_BYTES, keep=False):
    """Bootstrap conditional on measurement weights of a mixed set of voxels on NumPy arrays (mfx_wboot_fit), arguments
    as ``fit_weighted`` takes them and the options of ``fit_bootstrap``: every voxel class of the weighted fit is served
    (K in 0..maxfasc, CSF; no EAR).  The weights W [V, M] or [M] - those of a weighted fit, or the final weights of a robust
    fit - are held fixed in every replicate: nothing is rejected anew, so the result is conditional on them.  ``params``
    [V, num_params(maxfasc, csf_on, False)]: the voxels' own weighted fit (fitted here if None).  Returns the dict of
    ``fit_bootstrap``; status 0 fine, 1 no degree of freedom among the rows of positive weight, 2 original row not usable,
    3 a weight negative or not finite, 4 no positive weight."""
    B, code, qa = _boot_rule(B, kind, q, seed, offset)
    maxfasc = int(maxfasc)
    Y = L.f64c(Y)
    W = L.f64c(W)
    pk = L.f64c(peaks).reshape(Y.shape[0], -1) if (maxfasc > 0 and Y.ndim == 2) else np.zeros((Y.shape[0], 0))
    V, w_stride = _wfit_shapes(plan, Y.shape, W.shape, pk.shape, maxfasc)
    M = plan.M
    csf_on = bool(csf_on)
    K, cs, sc = _mixed_args(M, V, maxfasc, K, csf, csf_on, sig_csf, need_sig=True)
    npar = num_params(maxfasc, csf_on, False)
    p0 = None
    if params is not None:
        p0 = L.f64c(params)
        if p0.shape != (V, npar):
            raise ValueError("params should have shape (%d, %d), got %s" % (V, npar, p0.shape))
    vx = None
    if vox is not None:
        vx = np.ascontiguousarray(np.asarray(vox).reshape(-1), dtype=np.int64)
        if vx.shape != (V,):
            raise ValueError("vox should have one entry per voxel")
    pr, nprop = None, 0
    if props is not None:
        pr = np.atleast_2d(L.f64c(props))
        N = getattr(getattr(plan, 'tables', None), 'N', pr.shape[1])
        if pr.ndim != 2 or pr.shape[1] != N:
            raise ValueError("props should have shape (nprop, %d), got %s" % (N, pr.shape))
        nprop = pr.shape[0]
    gr = _boot_groups_arg(code, groups, M, getattr(plan, 'scheme', None))
    cols = boot_columns(maxfasc, csf_on, False, nprop)
    stats = np.zeros((V, len(cols), BOOT_NSTAT + qa.size))
    agree = np.zeros((V, maxfasc), dtype=np.int32)
    status = np.zeros(V, dtype=np.int32)
    reps = np.zeros((V, B, npar)) if keep else None
    L.check(L.lib().mfx_wboot_fit(plan.handle(), L.dptr(Y), L.dptr(W), w_stride, L.iptr(K), L.opt(cs, L.bptr),
                                  L.dptr(pk) if maxfasc > 0 else None, maxfasc, int(csf_on), L.opt(sc) if csf_on else None, L.opt(p0),
                                  L.opt(gr, L.iptr), L.opt(vx, L.lptr), V, B, code, int(bool(inflate)), int(seed) & _U64,
                                  int(offset) & _U64, L.opt(pr), nprop, L.dptr(qa) if qa.size else None, int(qa.size), int(max_bytes),
                                  L.dptr(stats), L.iptr(agree) if maxfasc > 0 else None, L.iptr(status), L.opt(reps)))
    if V:
        L.check(L.lib().mfx_plan_status(plan.handle(), None))   # a direction that is not a unit vector: ValueError
    return {'stats': stats, 'agree': agree, 'status': status, 'replicates': reps, 'columns': cols}


def _boot2d_maxfasc(maxfasc):
    maxfasc = int(maxfasc)
    if maxfasc < 0 or maxfasc > 3:
        raise NotImplementedError("the 2-D protocol fit serves 0 to 3 fascicles per voxel (maxfasc = %d)" % maxfasc)
    return maxfasc


def _boot2d_props_shape(tables, shape):
    """nprop of property tables [nprop, N] of a 2-D protocol's dictionary."""
    if len(shape) != 2 or shape[1] != tables.N:
        raise ValueError("props should have shape (nprop, %d), got %s" % (tables.N, tuple(shape)))
    return int(shape[0])


def fit2d_replicates_dev(tables, d_Ystar, d_peaks, maxfasc):
    """The replicate fit of a 2-D protocol on the device (mfx_boot2d_fit_rows_dev, include/mfx_boot2d.h) for a
    mf_utils.RotateAtom2DTables and ONE voxel class (every voxel ``maxfasc`` fascicles, no CSF column): B signals per
    voxel on one set of directions - the replicates of a bootstrap, or many noise realisations of one voxel geometry.
    torch CUDA float64 tensors d_Ystar [V, B, M], d_peaks [V, 3 maxfasc] -> (params [V, B, num_params(maxfasc, False,
    False)], status [V, 5] int32 per voxel).  Every row equals, bit for bit, the row ``fit2d_dev`` returns for that signal
    with those directions; for one and two fascicles the directions' records, the dictionaries' column norms and their
    cross-Gram are formed once per voxel, not once per row.  Enqueues on torch's current stream and returns without
    waiting."""
    import torch
    maxfasc = _boot2d_maxfasc(maxfasc)
    _f64_cuda(d_Ystar, d_peaks if maxfasc > 0 else None)
    if d_Ystar.dim() != 3 or d_Ystar.shape[1] < 1 or d_Ystar.shape[2] != tables.M:
        raise ValueError("replicate signals should have shape (voxels, B >= 1, %d), got %s" % (tables.M, tuple(d_Ystar.shape)))
    V, B, _ = d_Ystar.shape
    if maxfasc > 0 and (d_peaks is None or tuple(d_peaks.shape) != (V, 3 * maxfasc)):
        raise ValueError("peaks should have shape (%d, %d)" % (V, 3 * maxfasc))
    dev = d_Ystar.device
    out = torch.empty((V, B, num_params(maxfasc, False, False)), dtype=torch.float64, device=dev)
    status = torch.empty((V, 5), dtype=torch.int32, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    with torch.cuda.device(dev):
        L.check(L.lib().mfx_boot2d_fit_rows_dev(tables.handle(), d_Ystar.data_ptr(), _tptr(d_peaks) if maxfasc > 0 else None,
                                                maxfasc, V, B, out.data_ptr(), status.data_ptr(), st))
    return out, status


def fit2d_bootstrap_dev(tables, d_Y, d_peaks, maxfasc, csf_on=False, d_sig_csf=None, B=200, kind='wild', seed=0, inflate=True,
                        offset=0, q=(0.025, 0.975), d_props=None, d_groups=None, d_params=None, d_pred=None, d_vox=None,
                        max_bytes=BOOT_DEFAULT_BYTES, keep=False):
    """Device-resident bootstrap of voxels of a 2-D protocol (mfx_boot2d_fit_dev) for ONE voxel class (every voxel: K ==
    maxfasc, csf == csf_on), arguments as ``fit_bootstrap_dev`` takes them, without EAR, on a mf_utils.RotateAtom2DTables.
    The residual bootstrap needs ``d_groups`` [M] int32.  Returns the dict of ``fit_bootstrap_dev`` plus 'dir_status'
    [V, 5] int32 (the failing directions' records: such a voxel has status 2 and NaN statistics).  Enqueues on torch's
    current stream and returns without waiting."""
    import torch
    B, code, qa = _boot_rule(B, kind, q, seed, offset)
    maxfasc = _boot2d_maxfasc(maxfasc)
    _f64_cuda(d_Y, d_peaks if maxfasc > 0 else None, d_sig_csf if csf_on else None, d_props, d_params, d_pred)
    if d_Y.dim() != 2 or d_Y.shape[1] != tables.M:
        raise ValueError("data should have shape (voxels, %d), got %s" % (tables.M, tuple(d_Y.shape)))
    V, M = d_Y.shape
    npar = num_params(maxfasc, csf_on, False)
    if maxfasc > 0 and (d_peaks is None or tuple(d_peaks.shape) != (V, 3 * maxfasc)):
        raise ValueError("peaks should have shape (%d, %d)" % (V, 3 * maxfasc))
    if csf_on and (d_sig_csf is None or d_sig_csf.numel() != M):
        raise ValueError("csf_on needs sig_csf with %d entries" % M)
    if d_params is not None and tuple(d_params.shape) != (V, npar):
        raise ValueError("params should have shape (%d, %d), got %s" % (V, npar, tuple(d_params.shape)))
    if d_pred is not None and (d_params is None or tuple(d_pred.shape) != (V, M)):
        raise ValueError("a prediction needs the parameters it was made from and the data's shape (%d, %d)" % (V, M))
    nprop = _boot2d_props_shape(tables, d_props.shape) if d_props is not None else 0
    if code == 1:
        if d_groups is None:
            raise ValueError("the residual bootstrap needs groups")
        assert d_groups.is_cuda and d_groups.dtype == torch.int32 and d_groups.is_contiguous()
        if tuple(d_groups.shape) != (M,):
            raise ValueError("groups should be %d integers (one per measurement), got shape %s" % (M, tuple(d_groups.shape)))
    if d_vox is not None:
        assert d_vox.is_cuda and d_vox.dtype == torch.int64 and d_vox.is_contiguous()
        if tuple(d_vox.shape) != (V,):
            raise ValueError("vox should have one entry per voxel")
    dev = d_Y.device
    cols = boot_columns(maxfasc, csf_on, False, nprop)
    d_q = torch.from_numpy(qa).to(dev) if qa.size else None
    stats = torch.empty((V, len(cols), BOOT_NSTAT + qa.size), dtype=torch.float64, device=dev)
    agree = torch.zeros((V, maxfasc), dtype=torch.int32, device=dev)
    status = torch.zeros((V,), dtype=torch.int32, device=dev)
    dstat = torch.zeros((V, 5), dtype=torch.int32, device=dev)
    reps = torch.empty((V, B, npar), dtype=torch.float64, device=dev) if keep else None
    st = torch.cuda.current_stream(dev).cuda_stream
    with torch.cuda.device(dev):
        L.check(L.lib().mfx_boot2d_fit_dev(tables.handle(), d_Y.data_ptr(), _tptr(d_peaks) if maxfasc > 0 else None, maxfasc,
                                           int(bool(csf_on)), _tptr(d_sig_csf) if csf_on else None, _tptr(d_params), _tptr(d_pred),
                                           _tptr(d_groups) if code == 1 else None, _tptr(d_vox), V, B, code, int(bool(inflate)),
                                           int(seed) & _U64, int(offset) & _U64, _tptr(d_props), nprop, _tptr(d_q), int(qa.size),
                                           int(max_bytes), stats.data_ptr(), agree.data_ptr() if maxfasc > 0 else None,
                                           status.data_ptr(), dstat.data_ptr(), _tptr(reps), st))
    return {'stats': stats, 'agree': agree, 'status': status, 'dir_status': dstat, 'replicates': reps, 'columns': cols}


def fit2d_bootstrap(tables, Y, K, csf, peaks, maxfasc, csf_on, sig_csf=None, B=200, kind='wild', seed=0, inflate=True, offset=0,
                    q=(0.025, 0.975), props=None, groups=None, params=None, vox=None, max_bytes=BOOT_DEFAULT_BYTES, keep=False):
    """Bootstrap of a mixed set of voxels of a 2-D protocol on NumPy arrays (mfx_boot2d_fit), arguments as ``fit2d`` takes
    them and the options of ``fit_bootstrap``: every voxel class of ``fit2d`` is served (K in 0..maxfasc, CSF).  One and
    two fascicles without CSF share the directions' work among a voxel's replicates (``fit2d_replicates_dev``); the other
    classes fit the replicate rows one by one.  ``groups`` [M] is needed for kind 'residual'.  Returns the dict of
    ``fit_bootstrap`` plus 'dir_status' [V, 5] int32: a voxel with a failing direction keeps its record there, has status 2
    and NaN statistics."""
    B, code, qa = _boot_rule(B, kind, q, seed, offset)
    maxfasc = _boot2d_maxfasc(maxfasc)
    Y = L.f64c(Y)
    pk = L.f64c(peaks).reshape(Y.shape[0], -1) if (maxfasc > 0 and Y.ndim == 2) else np.zeros((Y.shape[0], 0))
    V = _fit2d_shapes(tables, Y.shape, pk.shape, maxfasc)
    M = tables.M
    csf_on = bool(csf_on)
    K, cs, sc = _mixed_args(M, V, maxfasc, K, csf, csf_on, sig_csf, need_sig=True)
    npar = num_params(maxfasc, csf_on, False)
    p0 = None
    if params is not None:
        p0 = L.f64c(params)
        if p0.shape != (V, npar):
            raise ValueError("params should have shape (%d, %d), got %s" % (V, npar, p0.shape))
    vx = None
    if vox is not None:
        vx = np.ascontiguousarray(np.asarray(vox).reshape(-1), dtype=np.int64)
        if vx.shape != (V,):
            raise ValueError("vox should have one entry per voxel")
    pr, nprop = None, 0
    if props is not None:
        pr = np.atleast_2d(L.f64c(props))
        nprop = _boot2d_props_shape(tables, pr.shape)
    gr = _boot_groups_arg(code, groups, M, None)
    cols = boot_columns(maxfasc, csf_on, False, nprop)
    stats = np.zeros((V, len(cols), BOOT_NSTAT + qa.size))
    agree = np.zeros((V, maxfasc), dtype=np.int32)
    status = np.zeros(V, dtype=np.int32)
    dstat = np.zeros((V, 5), dtype=np.int32)
    reps = np.zeros((V, B, npar)) if keep else None
    L.check(L.lib().mfx_boot2d_fit(tables.handle(), L.dptr(Y), L.iptr(K), L.opt(cs, L.bptr), L.dptr(pk) if maxfasc > 0 else None,
                                   maxfasc, int(csf_on), L.opt(sc) if csf_on else None, L.opt(p0), L.opt(gr, L.iptr),
                                   L.opt(vx, L.lptr), V, B, code, int(bool(inflate)), int(seed) & _U64, int(offset) & _U64,
                                   L.opt(pr), nprop, L.dptr(qa) if qa.size else None, int(qa.size), int(max_bytes), L.dptr(stats),
                                   L.iptr(agree) if maxfasc > 0 else None, L.iptr(status), L.iptr(dstat), L.opt(reps)))
    return {'stats': stats, 'agree': agree, 'status': status, 'dir_status': dstat, 'replicates': reps, 'columns': cols}


def fit2d_weighted_replicates_dev(tables, d_Ystar, d_W, d_peaks, maxfasc):
    """The weighted replicate fit of a 2-D protocol on the device (mfx_wboot2d_fit_rows_dev, include/mfx_wboot2d.h) for a
    mf_utils.RotateAtom2DTables and ONE voxel class (every voxel ``maxfasc`` fascicles, no CSF column): B signals per
    voxel on the voxel's weights and directions.  torch CUDA float64 tensors d_Ystar [V, B, M], d_W [V, M] or [M],
    d_peaks [V, 3 maxfasc] -> (params [V, B, num_params(maxfasc, False, False)], status [V, 5] int32 per voxel, wstatus
    [V] int32 as ``fit2d_weighted_dev`` gives it for the voxel's weights).  Every row equals, bit for bit, the row
    ``fit2d_weighted_dev`` returns for that signal with those weights and directions; for one and two fascicles sqrt(W),
    the directions' records, the scaled dictionaries' column norms and their cross-Gram are formed once per voxel, not
    once per row.  Enqueues on torch's current stream and returns without waiting."""
    import torch
    maxfasc = _boot2d_maxfasc(maxfasc)
    _f64_cuda(d_Ystar, d_W, d_peaks if maxfasc > 0 else None)
    if d_Ystar.dim() != 3 or d_Ystar.shape[1] < 1 or d_Ystar.shape[2] != tables.M:
        raise ValueError("replicate signals should have shape (voxels, B >= 1, %d), got %s" % (tables.M, tuple(d_Ystar.shape)))
    V, B, M = d_Ystar.shape
    if maxfasc > 0 and (d_peaks is None or tuple(d_peaks.shape) != (V, 3 * maxfasc)):
        raise ValueError("peaks should have shape (%d, %d)" % (V, 3 * maxfasc))
    w_stride = _w_stride(M, V, d_W.shape)
    dev = d_Ystar.device
    out = torch.empty((V, B, num_params(maxfasc, False, False)), dtype=torch.float64, device=dev)
    status = torch.empty((V, 5), dtype=torch.int32, device=dev)
    wstatus = torch.empty((V,), dtype=torch.int32, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    with torch.cuda.device(dev):
        L.check(L.lib().mfx_wboot2d_fit_rows_dev(tables.handle(), d_Ystar.data_ptr(), d_W.data_ptr(), w_stride,
                                                 _tptr(d_peaks) if maxfasc > 0 else None, maxfasc, V, B, out.data_ptr(),
                                                 status.data_ptr(), wstatus.data_ptr(), st))
    return out, status, wstatus


def fit2d_weighted_bootstrap_dev(tables, d_Y, d_W, d_peaks, maxfasc, csf_on=False, d_sig_csf=None, B=200, kind='wild', seed=0,
                                 inflate=True, offset=0, q=(0.025, 0.975), d_props=None, d_groups=None, d_params=None,
                                 d_pred=None, d_vox=None, max_bytes=BOOT_DEFAULT_BYTES, keep=False):
    """Device-resident bootstrap of voxels of a 2-D protocol conditional on measurement weights (mfx_wboot2d_fit_dev) for
    ONE voxel class (every voxel: K == maxfasc, csf == csf_on), arguments as ``fit2d_bootstrap_dev`` takes them plus the
    weights d_W [V, M] or [M].  The weights are held fixed: the own weighted fit (``d_params``, fitted here if None) is
    predicted, its residuals are resampled by the rule of ``wboot_resample_dev``, the replicates are fitted with the same
    weights (``fit2d_weighted_replicates_dev``) and reduced.  Returns the dict of ``fit2d_bootstrap_dev`` (the MSE column is
    the weighted MSE; status 2 for a failing direction, else as ``wboot_resample_dev``).  Enqueues on torch's current
    stream and returns without waiting."""
    import torch
    B, code, qa = _boot_rule(B, kind, q, seed, offset)
    maxfasc = _boot2d_maxfasc(maxfasc)
    _f64_cuda(d_Y, d_W, d_peaks if maxfasc > 0 else None, d_sig_csf if csf_on else None, d_props, d_params, d_pred)
    if d_Y.dim() != 2 or d_Y.shape[1] != tables.M:
        raise ValueError("data should have shape (voxels, %d), got %s" % (tables.M, tuple(d_Y.shape)))
    V, M = d_Y.shape
    w_stride = _w_stride(M, V, d_W.shape)
    npar = num_params(maxfasc, csf_on, False)
    if maxfasc > 0 and (d_peaks is None or tuple(d_peaks.shape) != (V, 3 * maxfasc)):
        raise ValueError("peaks should have shape (%d, %d)" % (V, 3 * maxfasc))
    if csf_on and (d_sig_csf is None or d_sig_csf.numel() != M):
        raise ValueError("csf_on needs sig_csf with %d entries" % M)
    if d_params is not None and tuple(d_params.shape) != (V, npar):
        raise ValueError("params should have shape (%d, %d), got %s" % (V, npar, tuple(d_params.shape)))
    if d_pred is not None and (d_params is None or tuple(d_pred.shape) != (V, M)):
        raise ValueError("a prediction needs the parameters it was made from and the data's shape (%d, %d)" % (V, M))
    nprop = _boot2d_props_shape(tables, d_props.shape) if d_props is not None else 0
    d_groups = _wboot_dev_opts(M, V, code, d_groups, d_vox)
    dev = d_Y.device
    cols = boot_columns(maxfasc, csf_on, False, nprop)
    d_q = torch.from_numpy(qa).to(dev) if qa.size else None
    stats = torch.empty((V, len(cols), BOOT_NSTAT + qa.size), dtype=torch.float64, device=dev)
    agree = torch.zeros((V, maxfasc), dtype=torch.int32, device=dev)
    status = torch.zeros((V,), dtype=torch.int32, device=dev)
    dstat = torch.zeros((V, 5), dtype=torch.int32, device=dev)
    reps = torch.empty((V, B, npar), dtype=torch.float64, device=dev) if keep else None
    st = torch.cuda.current_stream(dev).cuda_stream
    with torch.cuda.device(dev):
        L.check(L.lib().mfx_wboot2d_fit_dev(tables.handle(), d_Y.data_ptr(), d_W.data_ptr(), w_stride,
                                            _tptr(d_peaks) if maxfasc > 0 else None, maxfasc, int(bool(csf_on)),
                                            _tptr(d_sig_csf) if csf_on else None, _tptr(d_params), _tptr(d_pred),
                                            _tptr(d_groups) if code == 1 else None, _tptr(d_vox), V, B, code, int(bool(inflate)),
                                            int(seed) & _U64, int(offset) & _U64, _tptr(d_props), nprop, _tptr(d_q), int(qa.size),
                                            int(max_bytes), stats.data_ptr(), agree.data_ptr() if maxfasc > 0 else None,
                                            status.data_ptr(), dstat.data_ptr(), _tptr(reps), st))
    return {'stats': stats, 'agree': agree, 'status': status, 'dir_status': dstat, 'replicates': reps, 'columns': cols}


def fit2d_weighted_bootstrap(tables, Y, W, K, csf, peaks, maxfasc, csf_on, sig_csf=None, B=200, kind='wild', seed=0, inflate=True,
                             offset=0, q=(0.025, 0.975), props=None, groups=None, params=None, vox=None,
                             max_bytes=BOOT_DEFAULT_BYTES, keep=False):
    """Bootstrap of a mixed set of voxels of a 2-D protocol conditional on measurement weights, on NumPy arrays
    (mfx_wboot2d_fit): arguments as ``fit2d_weighted`` takes them and the options of ``fit2d_bootstrap``; every voxel class
    of ``fit2d_weighted`` is served (K in 0..maxfasc, CSF).  The weights W [V, M] or [M] - those of a weighted fit, or the
    final weights of a robust fit - are held fixed in every replicate: nothing is rejected anew, so the result is
    conditional on them.  ``params`` [V, num_params(maxfasc, csf_on, False)]: the voxels' own weighted fit (fitted here if
    None).  Returns the dict of ``fit2d_bootstrap``; status 2 for a failing direction (its record in 'dir_status'), else
    0 fine, 1 no degree of freedom among the rows of positive weight, 2 original row not usable, 3 a weight negative or
    not finite, 4 no positive weight."""
    B, code, qa = _boot_rule(B, kind, q, seed, offset)
    maxfasc = _boot2d_maxfasc(maxfasc)
    Y = L.f64c(Y)
    W = L.f64c(W)
    pk = L.f64c(peaks).reshape(Y.shape[0], -1) if (maxfasc > 0 and Y.ndim == 2) else np.zeros((Y.shape[0], 0))
    V = _fit2d_shapes(tables, Y.shape, pk.shape, maxfasc)
    M = tables.M
    w_stride = _w_stride(M, V, W.shape)
    csf_on = bool(csf_on)
    K, cs, sc = _mixed_args(M, V, maxfasc, K, csf, csf_on, sig_csf, need_sig=True)
    npar = num_params(maxfasc, csf_on, False)
    p0 = None
    if params is not None:
        p0 = L.f64c(params)
        if p0.shape != (V, npar):
            raise ValueError("params should have shape (%d, %d), got %s" % (V, npar, p0.shape))
    vx = None
    if vox is not None:
        vx = np.ascontiguousarray(np.asarray(vox).reshape(-1), dtype=np.int64)
        if vx.shape != (V,):
            raise ValueError("vox should have one entry per voxel")
    pr, nprop = None, 0
    if props is not None:
        pr = np.atleast_2d(L.f64c(props))
        nprop = _boot2d_props_shape(tables, pr.shape)
    gr = _boot_groups_arg(code, groups, M, None)
    cols = boot_columns(maxfasc, csf_on, False, nprop)
    stats = np.zeros((V, len(cols), BOOT_NSTAT + qa.size))
    agree = np.zeros((V, maxfasc), dtype=np.int32)
    status = np.zeros(V, dtype=np.int32)
    dstat = np.zeros((V, 5), dtype=np.int32)
    reps = np.zeros((V, B, npar)) if keep else None
    L.check(L.lib().mfx_wboot2d_fit(tables.handle(), L.dptr(Y), L.dptr(W), w_stride, L.iptr(K), L.opt(cs, L.bptr),
                                    L.dptr(pk) if maxfasc > 0 else None, maxfasc, int(csf_on), L.opt(sc) if csf_on else None,
                                    L.opt(p0), L.opt(gr, L.iptr), L.opt(vx, L.lptr), V, B, code, int(bool(inflate)),
                                    int(seed) & _U64, int(offset) & _U64, L.opt(pr), nprop, L.dptr(qa) if qa.size else None,
                                    int(qa.size), int(max_bytes), L.dptr(stats), L.iptr(agree) if maxfasc > 0 else None,
                                    L.iptr(status), L.iptr(dstat), L.opt(reps)))
    return {'stats': stats, 'agree': agree, 'status': status, 'dir_status': dstat, 'replicates': reps, 'columns': cols}


def solve_batch_dev(solver, d_Y, out=None, recons=True, max_bytes=0):
    """The batched explicit-dictionary solver on the device (mfx_solve_batch_dev, include/mfx_solve.h) for a
    mf_utils.ExhaustiveSolver: torch CUDA float64 signals d_Y [V, M] (or one [M] vector) -> (w [V, Kp] float64, sub [V, Kp]
    int64, tot [V, Kp] int64, obj [V] float64, yrec [V, M] float64 or None without ``recons``, status [V] int32), the rows
    ``solver.solve`` returns, bit for bit (the indices stay int64 on the device).  ``out``: a dict that may hold tensors
    'w', 'sub', 'obj', 'yrec', 'status' of those shapes and types to write into; 'yrec' is not touched without ``recons``.
    Enqueues on torch's current stream and returns without waiting."""
    import torch
    _f64_cuda(d_Y)
    V = solver.signal_rows(d_Y.shape)
    out = dict(out) if out is not None else {}
    unknown = set(out) - {'w', 'sub', 'obj', 'yrec', 'status'}
    if unknown:
        raise ValueError("out may hold 'w', 'sub', 'obj', 'yrec', 'status', got %s" % sorted(unknown))
    dev, Kp, M = d_Y.device, solver.Kp, solver.M
    if dev.index is not None and dev.index != solver.device:
        raise ValueError("signals live on %s, the solver on device %d" % (dev, solver.device))

    def buf(name, shape, dtype):
        t = out.get(name)
        if t is None:
            return torch.empty(shape, dtype=dtype, device=dev)
        if not (t.is_cuda and t.dtype == dtype and t.is_contiguous()) or tuple(t.shape) != tuple(shape):
            raise ValueError("out[%r] should be a contiguous CUDA %s tensor of shape %s, got %s of shape %s"
                             % (name, dtype, tuple(shape), t.dtype, tuple(t.shape)))
        return t
    w, sub = buf('w', (V, Kp), torch.float64), buf('sub', (V, Kp), torch.int64)
    obj, status = buf('obj', (V,), torch.float64), buf('status', (V,), torch.int32)
    yrec = buf('yrec', (V, M), torch.float64) if recons else None
    with torch.cuda.device(dev):
        starts = solver.starts_on(dev)
        if V > 0:
            st = torch.cuda.current_stream(dev).cuda_stream
            L.check(L.lib().mfx_solve_batch_dev(solver.handle(), d_Y.data_ptr(), V, int(max_bytes), w.data_ptr(), sub.data_ptr(),
                                                obj.data_ptr(), _tptr(yrec), status.data_ptr(), st))
        tot = torch.where(sub >= 0, sub + starts[None, :], sub)
    return w, sub, tot, obj, yrec, status


def solve_soft_sizes(solver):
    """(n1, n2) of the sub-dictionaries a solver's soft answers cover (n2 = 0 with one sub-dictionary; a third
    sub-dictionary of one column is the CSF column and has no row of its own); NotImplementedError with the library's
    message for a class they do not serve.  Touches the handle, nothing else."""
    L.check(L.lib().mfx_solve_soft_served(solver.handle()))
    return int(solver.dicsizes[0]), (int(solver.dicsizes[1]) if solver.Kp > 1 else 0)


def _solve_soft_head(solver, d_Y, out, names):
    """The argument checks of ``solve_batch_dev`` for the two entry points below: (V, the torch device, out as a dict)."""
    V = solver.signal_rows(d_Y.shape)
    out = dict(out) if out is not None else {}
    unknown = set(out) - set(names)
    if unknown:
        raise ValueError("out may hold %s, got %s" % (", ".join(repr(n) for n in names), sorted(unknown)))
    dev = d_Y.device
    if dev.index is not None and dev.index != solver.device:
        raise ValueError("signals live on %s, the solver on device %d" % (dev, solver.device))
    return V, dev, out


def _solve_soft_buf(out, dev, name, shape, dtype):
    import torch
    t = out.get(name)
    if t is None:
        return torch.empty(shape, dtype=dtype, device=dev)
    if not (t.is_cuda and t.dtype == dtype and t.is_contiguous()) or tuple(t.shape) != tuple(shape):
        raise ValueError("out[%r] should be a contiguous CUDA %s tensor of shape %s, got %s of shape %s"
                         % (name, dtype, tuple(shape), t.dtype, tuple(t.shape)))
    return t


def solve_profile_dev(solver, d_Y, partner=False, out=None, max_bytes=0):
    """Objective profiles of a mf_utils.ExhaustiveSolver on the device (mfx_solve_profile_dev, include/mfx_solve_soft.h):
    torch CUDA float64 signals d_Y [V, M] (or one [M] vector) -> ``(obj, partner, status)``: obj a list with one [V, n_k]
    float64 tensor per served sub-dictionary (obj[0][v, i] = min_j F(i, j), obj[1][v, j] = min_i F(i, j); one
    sub-dictionary: [F(i)]), partner the arg-min indices as int32 tensors of the same shapes (-1 with one
    sub-dictionary) or None without ``partner``, status [V] int32 (0 ok, 5 a non-finite signal: NaN rows, partners -1).
    ``out``: a dict that may hold tensors 'obj0', 'obj1', 'partner0', 'partner1', 'status' to write into.  Enqueues on
    torch's current stream and returns without waiting."""
    import torch
    _f64_cuda(d_Y)
    V, dev, out = _solve_soft_head(solver, d_Y, out, ('obj0', 'obj1', 'partner0', 'partner1', 'status'))
    n1, n2 = solve_soft_sizes(solver)
    obj = [_solve_soft_buf(out, dev, 'obj0', (V, n1), torch.float64)]
    if n2:
        obj.append(_solve_soft_buf(out, dev, 'obj1', (V, n2), torch.float64))
    par = None
    if partner:
        par = [_solve_soft_buf(out, dev, 'partner%d' % k, (V, n), torch.int32) for k, n in enumerate((n1, n2)[:len(obj)])]
    status = _solve_soft_buf(out, dev, 'status', (V,), torch.int32)
    if V > 0:
        with torch.cuda.device(dev):
            st = torch.cuda.current_stream(dev).cuda_stream
            L.check(L.lib().mfx_solve_profile_dev(solver.handle(), d_Y.data_ptr(), V, int(max_bytes), obj[0].data_ptr(),
                                                  _tptr(obj[1] if n2 else None), _tptr(par[0] if par else None),
                                                  _tptr(par[1] if par and n2 else None), status.data_ptr(), st))
    return obj, par, status


def solve_posterior_dev(solver, d_Y, d_T, d_shift=None, out=None, max_bytes=0):
    """Posterior weights of a mf_utils.ExhaustiveSolver on the device (mfx_solve_post_dev, include/mfx_solve_soft.h): torch
    CUDA float64 signals d_Y [V, M] (or one [M] vector), temperatures d_T [V] (2 sigma^2), d_shift [V] a value near each
    signal's smallest objective or None (the library takes min F itself) -> ``(w, log_sum, min_obj, status)``: w a list
    with one [V, n_k] float64 tensor per served sub-dictionary, log_sum [V] = log sum exp(-F / T), min_obj [V] = min F,
    status [V] int32 (0 ok, 1 unusable T or shift, 2 an exponent above 700 or a vanishing sum, 5 a non-finite signal;
    rows of such signals are NaN).  ``out``: a dict that may hold tensors 'w0', 'w1', 'log_sum', 'min_obj', 'status' to
    write into.  Enqueues on torch's current stream and returns without waiting."""
    import torch
    _f64_cuda(d_Y, d_T, d_shift)
    V, dev, out = _solve_soft_head(solver, d_Y, out, ('w0', 'w1', 'log_sum', 'min_obj', 'status'))
    for t, what in ((d_T, "T"), (d_shift, "shift")):
        if t is not None and tuple(t.shape) != (V,):
            raise ValueError("%s should have one entry per signal (%d), got shape %s" % (what, V, tuple(t.shape)))
        if t is not None and t.device != dev:
            raise ValueError("%s lives on %s, the signals on %s" % (what, t.device, dev))
    n1, n2 = solve_soft_sizes(solver)
    w = [_solve_soft_buf(out, dev, 'w0', (V, n1), torch.float64)]
    if n2:
        w.append(_solve_soft_buf(out, dev, 'w1', (V, n2), torch.float64))
    log_sum = _solve_soft_buf(out, dev, 'log_sum', (V,), torch.float64)
    min_obj = _solve_soft_buf(out, dev, 'min_obj', (V,), torch.float64)
    status = _solve_soft_buf(out, dev, 'status', (V,), torch.int32)
    if V > 0:
        with torch.cuda.device(dev):
            st = torch.cuda.current_stream(dev).cuda_stream
            L.check(L.lib().mfx_solve_post_dev(solver.handle(), d_Y.data_ptr(), V, d_T.data_ptr(), _tptr(d_shift), int(max_bytes),
                                               w[0].data_ptr(), _tptr(w[1] if n2 else None), log_sum.data_ptr(),
                                               min_obj.data_ptr(), status.data_ptr(), st))
    return w, log_sum, min_obj, status


def cleanup_select(f1, f2, p1, p2, cos_min, ratio, w_keep, w_small, device=0):
    """Voxel loop of cleanup_2fascicles (mfx_cleanup_2fascicles; ref mf.py:170-335): weights f1, f2 [n] and directions p1, p2
    [n x 3] of the ROI voxels -> (peaks [n x 6], count [n])."""
    f1, f2, p1, p2 = L.f64c(f1), L.f64c(f2), L.f64c(p1), L.f64c(p2)
    n = f1.shape[0]
    if f2.shape != (n,) or p1.shape != (n, 3) or p2.shape != (n, 3):
        raise ValueError("cleanup_select: f1, f2 should have shape (n,), p1, p2 (n, 3)")
    peaks = np.zeros((n, 6))
    count = np.zeros(n)
    L.check(L.lib().mfx_cleanup_2fascicles(L.dptr(f1), L.dptr(f2), L.dptr(p1), L.dptr(p2), n, float(cos_min), float(ratio),
                                           float(w_keep), float(w_small), L.dptr(peaks), L.dptr(count), int(device)))
    return peaks, count
