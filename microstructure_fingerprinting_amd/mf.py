"""DIPY-style user API: ``MFModel(dictionary).fit(...) -> MFModelFit``.

Mirror of the reference's ``microstructure_fingerprinting/mf.py`` (cited as ``ref``) for the fitting
path: same constructor, same ``fit`` signature / accepted inputs / exceptions, same ``params`` layout
and the same attributes on the fit object -- but the per-voxel loop of ``ref:976-1032`` (serial or
``multiprocessing.Pool`` over ``_fit_voxel``, ``ref:340-461``) is ONE batched call into the HIP
library (``engine.fit_batch`` -> ``mfx_fit_batch``); ``parallel=True`` shards the ROI over all
visible GPUs instead of over CPU processes.
"""
import os
import threading
import time

import numpy as np

from . import _lib as L
from . import dist as mdist
from . import engine
from . import mf_utils as mfu
from . import nifti


def _load_volume(x):
    """str -> (array, affine) from a NIfTI file; ndarray -> (x, None)."""
    if isinstance(x, str):
        return nifti.load(x)
    return x, None


# ---------------------------------------------------------------------------------------------
# peak clean-up ahead of the fit (post-processing of a 2-tensor / 2-peak estimate)
# ---------------------------------------------------------------------------------------------
CLEANUP_RATIO = 2.5        # dominant/minor weight ratio beyond which the minor fascicle is dropped ...
CLEANUP_W_KEEP = 0.20      # ... unless its own weight reaches this value
CLEANUP_W_SMALL = 0.075    # absolute weight under which a fascicle is always dropped
CLEANUP_ANG_MIN = 15       # crossing angle [deg] under which two peaks are merged


def _directions_from(mu, peakmode):
    """(n, 2|3|6) orientation descriptors -> (n, 3) direction vectors."""
    if peakmode == 'colat_longit':
        st = np.sin(mu[..., 0])
        return np.stack([st * np.cos(mu[..., 1]), st * np.sin(mu[..., 1]), np.cos(mu[..., 0])], axis=-1)
    if peakmode == 'peaks':
        return np.array(mu, dtype=np.float64)
    return mfu.DT_vec_to_peaks(mu, 'column')


def cleanup_2fascicles(frac1, frac2, peakmode, mu1, mu2, mask, frac12=None):
    """Select 0, 1 or 2 of two detected fascicle orientations per voxel (same arguments, thresholds and
    results as ref mf.py:36-335; NeuroImage 184 (2019) 964-980).

    Per mask voxel, in this order: peaks closer than 15 deg are merged into population 0 (sign-aware sum,
    weights added); a population more than 2.5x lighter than the other one and lighter than 0.20 is
    dropped (population 1 moves to slot 0 when population 0 goes); populations lighter than 0.075 are
    dropped; the survivors are ordered by descending weight.  Returns ``(peaks_out, num_fasc_out)`` with
    shapes ``mask.shape + (6,)`` and ``mask.shape``."""
    if (frac1 is None or frac2 is None) and frac12 is None:
        raise ValueError("If fractions of first and second fascicles set to None, argument frac12 is required "
                         "to specify both fractions simultanously. A total of 6 arguments should be passed, not 5.")
    mask = _load_volume(mask)[0]
    frac1 = _load_volume(frac1)[0]
    frac2 = _load_volume(frac2)[0]
    if frac12 is not None:
        frac12 = _load_volume(frac12)[0]
        if frac12.shape[-1] < 2:
            raise ValueError("Last dimension of frac12 should have size at least 2.")
        if frac12.shape[mask.ndim] == 1:           # (nx, ny, nz, 1, 2)
            frac1, frac2 = frac12[..., 0, 0], frac12[..., 0, 1]
        else:
            frac1, frac2 = frac12[..., 0], frac12[..., 1]
    if frac1.shape != mask.shape:
        raise ValueError("frac1 should have the same shape as mask")
    if frac2.shape != mask.shape:
        raise ValueError("frac2 should have the same shape as mask")
    mu1 = _load_volume(mu1)[0]
    mu2 = _load_volume(mu2)[0]
    width = {'colat_longit': 2, 'peaks': 3, 'tensor': 6}.get(peakmode)
    if width is None:
        raise ValueError('Unknown peak mode %s' % peakmode)
    if peakmode == 'tensor':                        # tensor files are often (nx, ny, nz, 1, 6)
        if mu1.shape[mask.ndim] == 1:
            mu1 = mu1[..., 0, :]
        if mu2.shape[mask.ndim] == 1:
            mu2 = mu2[..., 0, :]
    if mu1.shape[-1] != width or mu2.shape[-1] != width:
        raise ValueError("In '%s' peak mode, last dimension of mu1 and mu2 should have size %d. Detected %d and %d."
                         % (peakmode, width, mu1.shape[-1], mu2.shape[-1]))

    roi = mask > 0
    f1 = np.ascontiguousarray(frac1[roi], dtype=np.float64)
    f2 = np.ascontiguousarray(frac2[roi], dtype=np.float64)
    p1 = np.ascontiguousarray(_directions_from(mu1[roi], peakmode), dtype=np.float64)
    p2 = np.ascontiguousarray(_directions_from(mu2[roi], peakmode), dtype=np.float64)
    # the voxel loop (ref:170-335) runs on the device, one thread per ROI voxel (csrc/cleanup.hip)
    peaks, count = engine.cleanup_select(f1, f2, p1, p2, np.cos(CLEANUP_ANG_MIN * np.pi / 180), CLEANUP_RATIO,
                                         CLEANUP_W_KEEP, CLEANUP_W_SMALL)

    peaks_out = np.zeros(mask.shape + (6,))
    peaks_out[roi] = peaks
    num_fasc_out = np.zeros(mask.shape)
    num_fasc_out[roi] = count
    return peaks_out, num_fasc_out


class MFModel():
    r"""Microstructure Fingerprinting model (ref:464-1051)."""
    MAX_FASC = 2          # ref:467
    SHARD_DEVICES = None  # parallel=True: device of every shard; None: each visible GPU once (a device may be named twice)
    MAX_PROG_LINES = 100  # ref:468 (kept for API compatibility; progress is per batch here)
    DFT_DISP_ITVL = 5     # ref:469

    def __init__(self, dictionary, device=0):
        if isinstance(dictionary, str):
            self.dic = mfu.loadmat(dictionary)
        elif isinstance(dictionary, dict):
            self.dic = dictionary
        else:
            raise ValueError("Dictionary should either be a valid path to a Matlab-like mat file or a "
                             "Python dictionary.")
        self.device = device
        # per-shell knot tables, built once on the host (ref:506-509); uploaded to HBM on first use
        self.ms_interpolator = mfu.init_PGSE_multishell_interp(self.dic['dictionary'], self.dic['sch_mat'],
                                                               self.dic['orientation'], device=device)
        print("Initiated model based on dictionary with %d single-fascicle fingerprint(s) and %d "
              "fingerprint(s) for the extra-axonal restricted (EAR) compartment."
              % (self.dic['num_atom'], self.dic['num_ear']))

    # ------------------------------------------------------------------------------------------
    def fit(self, data, mask, numfasc, *, peaks=None, colat_longit=None, tensors=None, pgse_scheme=None,
            bvals=None, bvecs=None, csf_mask=None, ear_mask=None, verbose=1, parallel=False, weights=None, robust=None):
        r"""Fingerprinting on the pre-computed dictionary (ref:516-1051; same arguments).

        ``weights`` (keyword only, default None: the plain sum of squares, exactly the code path without it):
        non-negative weights of the measurements, minimising ``sum_m W[v, m] (y_m - model_m)^2`` in every voxel
        (``engine.fit_weighted``: the reference chain on rows scaled by ``sqrt(W)``).  An array or NIfTI path of the
        data's shape (gathered to the ROI like the data) or one ``[M]`` vector shared by all voxels; bool (an outlier
        mask: False drops the measurement) or any numeric type.  Negative or non-finite weights, a voxel without a
        positive weight and weights together with ``ear_mask`` raise ValueError before anything is launched.  MSE is
        ``min_obj / sum W`` and R2 the weighted correlation; ``param_names`` and the maps are unchanged, and the fit
        keeps ``weights_roi`` in its fitinfo.  With ``parallel=True`` a weighted fit still runs on one device.

        ``robust`` (keyword only, default None; None and False are exactly the code path without it): a robust fit,
        ``engine.fit_robust`` - the fit, then ``n_iter`` times weights derived from the residuals (per voxel, in units
        of the median absolute residual) and a weighted refit, iterated on the device.  True stands for
        ``{'loss': 'cutoff', 'c': 4.45, 'n_iter': 3}`` (drop what lies beyond 4.45 median absolute residuals); a dict
        overrides any of the three (``loss`` 'cutoff' | 'huber' | 'tukey', ``c`` >= 1).  ``weights`` then are the base
        weights: a row of weight 0 stays out for good and does not enter the median.  Not served together with
        ``ear_mask`` (the ValueError of ``weights``); runs on one device.  The fit keeps the final weights as
        ``weights_roi`` - profiles, intervals and posteriors answer for the final weighted objective - and gains
        ``robust_info``, ``robust_scale``, ``n_rejected`` and ``outlier_mask()``."""
        VRB = verbose
        ropts = engine.robust_options(robust)
        nii_affine = None
        t0 = time.time()
        if isinstance(data, str) and VRB >= 2:
            print("Loading data from file %s..." % data)
        # a volume in file order (a NIfTI file, or nibabel's Fortran-ordered array) stays as it is: conversion to
        # float64, the header's scaling and the ROI gather (ref:623-657) run on the device (mfx_fit_batch_volume)
        vol = None
        if isinstance(data, str):
            raw, slope, inter, aff = nifti.load_raw(data)
            if engine.FileOrderVolume.accepts(raw):
                vol = engine.FileOrderVolume(raw, slope, inter)
                data_arr = raw
            else:
                data_arr = np.array(raw, dtype=np.float64)
                if nifti._scaled(slope, inter):
                    data_arr = data_arr * slope + inter
        else:
            data_arr, aff = data, None
            if engine.FileOrderVolume.accepts(data_arr):
                vol = engine.FileOrderVolume(data_arr)
        nii_affine = aff
        if isinstance(data, str) and VRB >= 2:
            print("Data loaded in %g s." % (time.time() - t0))
        mask_arr, aff = _load_volume(mask)
        if nii_affine is None:
            nii_affine = aff
        img_shape = mask_arr.shape
        roi = mask_arr > 0
        roi_index = np.flatnonzero(roi.reshape(-1))     # ROI order == np.where(mask > 0) (C order)
        ROI_size = int(roi_index.shape[0])
        _fidx = []

        def file_order_roi():   # the ROI voxels' positions inside one 3-D image of a file-order volume (computed once)
            if not _fidx:
                _fidx.append(np.ravel_multi_index(np.unravel_index(roi_index, img_shape), img_shape, order='F').astype(np.int64))
            return _fidx[0]

        def roi_rows(arr):      # arr[mask > 0] of a (grid x n) volume as float64 rows
            if engine.FileOrderVolume.accepts(arr) and arr.shape[:-1] == img_shape and ROI_size >= 4096:
                # a file-order (Fortran) volume: indexing it with the C-ordered mask, or reshaping it to C-order rows,
                # first copies the whole volume on one host core (0.2-0.6 s at 1e6 ROI voxels) - the device gathers it
                # like the data (mfx_volume_rows)
                return engine.volume_rows(engine.FileOrderVolume(arr), file_order_roi(), device=self.ms_interpolator.device)
            return np.asarray(arr.reshape(-1, arr.shape[-1])[roi_index], dtype=np.float64)
        if ROI_size == 0:
            raise ValueError("No voxel detected in mask. Please provide a non-empty mask.")
        if data_arr.shape[:-1] != img_shape:
            raise ValueError("Data and mask not compatible. Based on data, mask should have shape (%s), got (%s) "
                             "instead." % (" ".join("%d" % x for x in data_arr.shape[:-1]),
                                           " ".join("%d" % x for x in img_shape)))
        # ---- number of fascicles (ref:660-687)
        if np.isscalar(numfasc) and not isinstance(numfasc, str):
            numfasc_roi = np.full(ROI_size, numfasc, dtype=int)
        else:
            nf, _ = _load_volume(numfasc)
            if mask_arr.shape != nf.shape:
                raise ValueError("Data and argument numfasc not compatible.  Based on data, numfasc should have "
                                 "shape (%s), got (%s) instead." % (" ".join("%d" % x for x in img_shape),
                                                                   " ".join("%d" % x for x in nf.shape)))
            numfasc_roi = nf[roi].astype(int)
        maxfasc = int(np.max(numfasc_roi))
        if maxfasc > MFModel.MAX_FASC:
            raise ValueError("Detected %d mask voxel(s) in numfasc with number of axon populations greater than "
                             "allowed maximum of %d." % (np.sum(numfasc_roi > MFModel.MAX_FASC), MFModel.MAX_FASC))
        # ---- fascicle directions: peaks | colat_longit | tensors (ref:693-815)
        if peaks is not None:
            pk, aff = _load_volume(peaks)
            if nii_affine is None:
                nii_affine = aff
            if pk.shape[:-1] != img_shape:
                raise ValueError("Arg. peaks not compatible. Based on data, it should have shape (%s x), with x a "
                                 "multiple of 3. Got (%s) instead." % (" ".join("%d" % x for x in img_shape),
                                                                       " ".join("%d" % x for x in pk.shape)))
            if pk.shape[-1] % 3 != 0:
                raise ValueError("Size of last dimension of arg. peaks should be a multiple of 3, got %d instead."
                                 % pk.shape[-1])
            if pk.shape[-1] > maxfasc * 3 and VRB >= 1:
                print("Ignoring last %d value(s) along last dimension of peaks, as max number of axon populations "
                      "in mask is %d." % (pk.shape[-1] - maxfasc * 3, maxfasc))
            peaks_roi = np.ascontiguousarray(roi_rows(np.asarray(pk))[:, :3 * maxfasc], dtype=np.float64)
        elif colat_longit is not None or tensors is not None:
            arg = colat_longit if colat_longit is not None else tensors
            dims = ((2,),) if colat_longit is not None else ((6,), (1, 6))
            arg = arg if isinstance(arg, list) else [arg]
            peaks_roi = np.zeros((ROI_size, 3 * len(arg)))
            if len(arg) > maxfasc and VRB >= 1:
                print("Ignoring %d peak orientation argument(s) because max number of axon populations in mask "
                      "is %d." % (len(arg) - maxfasc, maxfasc))
            for i in range(min(len(arg), maxfasc)):
                a_i, aff = _load_volume(arg[i])
                if nii_affine is None:
                    nii_affine = aff
                if a_i.shape not in [img_shape + d for d in dims]:
                    want = " or ".join("(" + " ".join("%d" % x for x in img_shape + d) + ")" for d in dims)
                    raise ValueError("Peak orientation arg. %d of %d seems incompatible. Based on data, it should "
                                     "have shape %s, got (%s) instead."
                                     % (i + 1, len(arg), want, " ".join("%d" % x for x in a_i.shape)))
                if colat_longit is not None:
                    ang = roi_rows(a_i)
                    th, ph = ang[:, 0], ang[:, 1]
                    peaks_roi[:, 3 * i + 0] = np.sin(th) * np.cos(ph)
                    peaks_roi[:, 3 * i + 1] = np.sin(th) * np.sin(ph)
                    peaks_roi[:, 3 * i + 2] = np.cos(th)
                else:
                    if a_i.shape[mask_arr.ndim] == 1:
                        a_i = a_i[(slice(None),) * mask_arr.ndim + (0, slice(None))]
                    # NIfTI 'column' order of the upper triangle; principal eigenvector, 0 for zero tensors
                    peaks_roi[:, 3 * i:3 * i + 3] = mfu.DT_vec_to_peaks(roi_rows(a_i), 'column')
            peaks_roi = np.ascontiguousarray(peaks_roi[:, :3 * maxfasc])
            if peaks_roi.shape[1] < 3 * maxfasc:
                peaks_roi = np.concatenate([peaks_roi, np.zeros((ROI_size, 3 * maxfasc - peaks_roi.shape[1]))], axis=1)
        else:
            raise RuntimeError("At least one of peaks, colat_longit and tensors must be specified.")
        for k in range(maxfasc):   # missing peak where numfasc demands one (ref:803-815)
            zero_k = ~np.any(peaks_roi[:, 3 * k:3 * k + 3], axis=1)
            n0 = int(np.count_nonzero(zero_k & (numfasc_roi >= k + 1))) if zero_k.any() else 0
            if n0 > 0:
                raise ValueError("Detected %d voxel(s) in which the main orientation of axon population %d/%d was a "
                                 "zero vector, although numfasc specifies the presence of that population."
                                 % (n0, k + 1, maxfasc))
        # ---- protocol (ref:821-846)
        pgse_scheme = self._protocol(pgse_scheme, bvals, bvecs)
        num_seq = pgse_scheme.shape[0]
        # ---- optional compartments (ref:852-894)
        csf_mask, aff = self._roi_flags(csf_mask, roi, img_shape, ROI_size, "csf_mask")
        if nii_affine is None:
            nii_affine = aff
        ear_mask, aff = self._roi_flags(ear_mask, roi, img_shape, ROI_size, "ear_mask")
        if nii_affine is None:
            nii_affine = aff
        csf_on = bool(np.any(csf_mask > 0))
        ear_on = bool(np.any(ear_mask > 0))
        n_empty = int(np.sum((numfasc_roi + csf_mask + ear_mask) == 0))
        if n_empty > 0 and VRB >= 2:
            print("WARNING: detected %d voxel(s) in mask with zero  axon population, no cerebrospinal fluid (CSF) "
                  "and no extra-axonal restricted (EAR) compartment specified. No estimation will be performed "
                  "there." % (n_empty,))
        sig_csf, sig_ear, num_ear = self._extra_signals(pgse_scheme, csf_on, ear_on)
        if data_arr.shape[-1] != num_seq:
            raise ValueError("Data has %d measurements per voxel but the protocol has %d." % (data_arr.shape[-1],
                                                                                                num_seq))
        # ---- measurement weights: gathered to the ROI like the data and checked on the host before any launch
        weights_roi = None
        if weights is not None:
            weights_roi = self._roi_weights(weights, roi_index, img_shape, num_seq, ROI_size)
        if weights is not None or ropts is not None:
            if ear_on:
                raise ValueError("weights are not served together with ear_mask: %d of %d voxel(s) in mask have an EAR "
                                 "compartment." % (int(np.count_nonzero(ear_mask)), ROI_size))
        # ---- what the reference checks in every voxel with a fascicle, through interp_PGSE_from_multishell
        # (mf_utils.py:1786-1789 and 1804-1807), checked once per fit here: the protocol's timing must be the
        # dictionary's, its gradient directions zero or unit vectors
        if maxfasc > 0:
            self._check_protocol(pgse_scheme)
        # ---- the voxel loop, batched on the device (replaces ref:976-1032)
        # ROI order == np.where(mask > 0).  A float64 C-contiguous volume is handed over as it is with the ROI's row
        # numbers: the library gathers the rows while it stages the upload (the reference's data[mask > 0], ref:644)
        if vol is not None:
            Y = vol
            rows = file_order_roi()
        elif isinstance(data_arr, np.ndarray) and data_arr.dtype == np.float64 and data_arr.flags.c_contiguous:
            Y = data_arr.reshape(-1, num_seq)
            rows = roi_index.astype(np.int64, copy=False)
        else:
            Y = np.ascontiguousarray(data_arr[roi], dtype=np.float64)
            rows = None
        st = time.time()
        if VRB >= 2:
            print("Starting estimation in %d voxel(s) on the GPU%s." % (ROI_size, "s (sharded)" if parallel else ""))
        args = (numfasc_roi, csf_mask, ear_mask, peaks_roi, maxfasc, csf_on, ear_on, sig_csf, sig_ear, num_ear)
        devs = list(range(L.lib().mfx_device_count())) if self.SHARD_DEVICES is None else list(self.SHARD_DEVICES)
        robust_fit = None
        if ropts is not None:   # one device: the ROI's rows stay there through the fits and the reweighting between them
            plan = self.ms_interpolator.plan_for(pgse_scheme)
            Y_roi = (engine.volume_rows(vol, rows, device=self.ms_interpolator.device) if vol is not None
                     else (Y[rows] if rows is not None else Y))
            params_in_mask, w_final, rinfo = engine.fit_robust(plan, Y_roi, numfasc_roi, csf_mask, peaks_roi, maxfasc, csf_on,
                                                               sig_csf, W0=weights_roi, **ropts)
            if np.any(rinfo['status']):
                raise ValueError("robust fit: %d of %d voxel(s) have unusable weights."
                                 % (int(np.count_nonzero(rinfo['status'])), ROI_size))
            robust_fit = (rinfo, weights_roi, dict(ropts))
            weights_roi = w_final
        elif weights_roi is not None:   # one device: the ROI's rows on the host, then the weighted kernels
            plan = self.ms_interpolator.plan_for(pgse_scheme)
            Y_roi = (engine.volume_rows(vol, rows, device=self.ms_interpolator.device) if vol is not None
                     else (Y[rows] if rows is not None else Y))
            params_in_mask, wstat = engine.fit_weighted(plan, Y_roi, weights_roi, numfasc_roi, csf_mask, peaks_roi, maxfasc,
                                                        csf_on, sig_csf)
            if np.any(wstat):
                raise ValueError("weighted fit: %d of %d voxel(s) have unusable weights." % (int(np.count_nonzero(wstat)), ROI_size))
        elif parallel and len(devs) > 1 and ROI_size >= 2 * len(devs):
            params_in_mask = self._fit_sharded(pgse_scheme, Y, rows, args, devs)
        else:
            plan = self.ms_interpolator.plan_for(pgse_scheme)
            params_in_mask = (engine.fit_batch_volume(plan, Y, rows, *args) if vol is not None
                              else engine.fit_batch(plan, Y, *args, rows=rows))
        if VRB >= 2:
            print("Estimation performed in %g second(s)." % (time.time() - st))
        fitinfo = {'maxfasc': maxfasc, 'csf_on': csf_on, 'ear_on': ear_on, 'affine': nii_affine, 'mask': mask_arr,
                   'fasc_propnames': [x.strip() for x in self.dic['fasc_propnames']], 'peaks_roi': peaks_roi,
                   'roi_index': roi_index, 'model': self, 'pgse_scheme': pgse_scheme,
                   'numfasc_roi': numfasc_roi, 'csf_roi': np.asarray(csf_mask, dtype=bool),
                   'ear_roi': np.asarray(ear_mask, dtype=bool)}
        if weights_roi is not None:
            fitinfo['weights_roi'] = weights_roi
        if robust_fit is not None:
            fitinfo['robust_info'], fitinfo['robust_base'], fitinfo['robust_options'] = robust_fit
        for n in fitinfo['fasc_propnames']:
            fitinfo['_dict_' + n] = self.dic[n]
        if ear_on:
            fitinfo['DIFF_ear'] = np.atleast_1d(self.dic['DIFF_ear'])
        return MFModelFit(fitinfo, params_in_mask, verbose=VRB)

    def _extra_signals(self, pgse_scheme, csf_on, ear_on):
        """(sig_csf [M] | None, sig_ear [M x num_ear] | None, num_ear) of a protocol (ref:918-925)."""
        gam = mfu.get_gyromagnetic_ratio('H')
        G, Delta, delta, TE = pgse_scheme[:, 3], pgse_scheme[:, 4], pgse_scheme[:, 5], pgse_scheme[:, 6]
        b = (gam * G * delta) ** 2 * (Delta - delta / 3)
        sig_csf = sig_ear = None
        num_ear = int(self.dic['num_ear'])
        if csf_on:   # ref:918-920
            sig_csf = np.exp(-TE / self.dic['T2_csf']) * np.exp(-b * self.dic['DIFF_csf'])
        if ear_on:   # ref:921-925
            DIFF_ear = np.atleast_1d(self.dic['DIFF_ear'])
            sig_ear = np.zeros((pgse_scheme.shape[0], num_ear))
            for i in range(num_ear):
                sig_ear[:, i] = np.exp(-TE / self.dic['T2_ear']) * np.exp(-b * DIFF_ear[i])
        return sig_csf, sig_ear, num_ear

    def _check_protocol(self, pgse_scheme):
        """What the reference checks in every voxel with a fascicle (mf_utils.py:1786-1789, 1804-1807)."""
        if not np.all(np.isclose(self.ms_interpolator['scheme_DeldelTE'], pgse_scheme[:, 4:7])):
            raise ValueError("Delta, delta and TE values should all be identical to those in the multi-shell "
                             "sampling.")
        mfu._check_gnorms(pgse_scheme)

    def _protocol(self, pgse_scheme, bvals, bvecs):
        """The protocol arguments of fit (ref:821-846) as a float64 [M x 7] scheme matrix."""
        if pgse_scheme is not None:
            if isinstance(pgse_scheme, str):
                pgse_scheme = np.loadtxt(pgse_scheme, skiprows=1)
            if pgse_scheme.shape[1] != 7:
                raise ValueError("pgse_scheme should have 7 columns,  detected %d instead." % (pgse_scheme.shape[1],))
        else:
            if bvals is None or bvecs is None:
                raise TypeError("If no schemefile is provided, then both bvals and bvecs must be specified.")
            pgse_scheme = mfu.get_PGSE_scheme_from_bval_bvec_dense(self.dic['sch_mat'], bvals, bvecs, 1e-3)
        return np.ascontiguousarray(pgse_scheme, dtype=np.float64)

    def predict(self, params_in_mask, peaks, *, pgse_scheme=None, bvals=None, bvecs=None, data=None, sigma_g=None, N=0,
                seed=0, offset=0):
        """The DW-MRI signal that parameter rows stand for: the reference's ``y_rec`` (ref:413-419), which its fit
        computes in every voxel and drops.

        ``params_in_mask`` [V x num_params] has the layout of ``MFModelFit.params_in_mask`` (M0, nu_f, ID_f, nu_csf,
        nu_ear, ID_ear, MSE, R2; the last two are ignored) and ``peaks`` [V x 3 maxfasc] the fascicle directions;
        the number of columns says which optional compartments are there.  The protocol is given as in ``fit``.
        Returns the signals [V x M]; with ``data`` [V x M] also ``stats`` [V x 2], the residual sum of squares and
        R2 per voxel.  ``N`` >= 1 (with ``sigma_g``; one without the other is an error) adds the magnitude noise of ``mf_utils.gen_SoS_MRI`` with ``sigma_g`` (a scalar, one
        value per voxel or one per element) in the same pass.  NumPy arrays in, NumPy arrays out; torch CUDA
        float64 tensors in, tensors out on torch's current stream, nothing copied to the host."""
        if sigma_g is not None and not N:
            raise ValueError("sigma_g is given but the number of coils N is 0: pass N >= 1 for noise (simulate does)")
        sch = self._protocol(pgse_scheme, bvals, bvecs)
        on_dev = type(params_in_mask).__module__.split('.')[0] == 'torch'
        if params_in_mask.ndim != 2:
            raise ValueError("params_in_mask should be a 2-D array [voxels x parameters]")
        maxfasc = 0 if peaks is None else int(peaks.shape[-1]) // 3
        extra = params_in_mask.shape[1] - 3 - 2 * maxfasc
        if peaks is not None and (peaks.ndim != 2 or peaks.shape[1] != 3 * maxfasc) or extra not in (0, 1, 2, 3):
            raise ValueError("peaks should have 3 columns per fascicle and params_in_mask 1 + 2 maxfasc + csf + 2 ear + 2 "
                             "columns; got shapes %s and %s" % (None if peaks is None else tuple(peaks.shape),
                                                                tuple(params_in_mask.shape)))
        csf_on, ear_on = bool(extra & 1), bool(extra & 2)
        if maxfasc > 0:
            self._check_protocol(sch)
        sig_csf, sig_ear, num_ear = self._extra_signals(sch, csf_on, ear_on)
        plan = self.ms_interpolator.plan_for(sch)
        if on_dev:
            import torch
            dev = params_in_mask.device
            d_csf = torch.as_tensor(sig_csf, device=dev) if csf_on else None
            d_ear = torch.as_tensor(np.ascontiguousarray(sig_ear), device=dev) if ear_on else None
            return engine.predict_dev(plan, params_in_mask, peaks, maxfasc, csf_on, ear_on, d_csf, d_ear, num_ear,
                                      d_Y=data, sigma_g=sigma_g, ncoils=N, seed=seed, offset=offset)
        return engine.predict(plan, params_in_mask, peaks, maxfasc, csf_on, ear_on, sig_csf, sig_ear, num_ear, Y=data,
                              sigma_g=sigma_g, ncoils=N, seed=seed, offset=offset)

    def simulate(self, params_in_mask, peaks, *, SNR=None, sigma_g=None, N=1, seed=None, offset=0, pgse_scheme=None,
                 bvals=None, bvecs=None):
        """``predict`` with the sum-of-squares magnitude noise of ``N`` coils (Rician for N = 1): give either
        ``sigma_g`` or ``SNR``, which sets ``sigma_g = M0 / SNR`` in every voxel.  ``seed=None`` draws a seed from
        NumPy's global generator; an int makes the call reproducible by itself."""
        if (SNR is None) == (sigma_g is None):
            raise ValueError("simulate needs exactly one of SNR and sigma_g")
        if SNR is not None:
            sigma_g = params_in_mask[:, 0] / SNR
        return self.predict(params_in_mask, peaks, pgse_scheme=pgse_scheme, bvals=bvals, bvecs=bvecs, sigma_g=sigma_g,
                            N=N, seed=mfu._sos_seed(seed), offset=offset)

    @staticmethod
    def _roi_weights(weights, roi_index, img_shape, num_seq, ROI_size):
        """weights argument -> float64 [ROI_size x M] or [M], checked (every failure a ValueError naming the voxel count)."""
        w = weights
        if isinstance(w, str):
            w, _ = _load_volume(w)
        w = np.asarray(w)
        if w.dtype == object or not (np.issubdtype(w.dtype, np.number) or w.dtype == np.bool_):
            raise ValueError("weights should be boolean or numeric (%d voxel(s) in mask)." % ROI_size)
        if w.shape == (num_seq,):
            w_roi = np.ascontiguousarray(w, dtype=np.float64)
        elif w.shape == tuple(img_shape) + (num_seq,):
            w_roi = np.ascontiguousarray(w.reshape(-1, num_seq)[roi_index], dtype=np.float64)
        else:
            raise ValueError("weights not compatible with the data of %d voxel(s) in mask: expected shape (%s) or (%d), "
                             "got (%s)." % (ROI_size, " ".join("%d" % x for x in tuple(img_shape) + (num_seq,)), num_seq,
                                            " ".join("%d" % x for x in w.shape)))
        bad = ~np.isfinite(w_roi) | (w_roi < 0)
        if bad.any():
            n_bad = ROI_size if w_roi.ndim == 1 else int(np.count_nonzero(bad.any(axis=1)))
            raise ValueError("Detected %d of %d voxel(s) in mask with negative or non-finite weights." % (n_bad, ROI_size))
        none = ~(w_roi > 0).any(axis=-1)
        if np.any(none):
            n_none = ROI_size if w_roi.ndim == 1 else int(np.count_nonzero(none))
            raise ValueError("Detected %d of %d voxel(s) in mask without a positive weight." % (n_none, ROI_size))
        return w_roi

    @staticmethod
    def _roi_flags(m, roi, img_shape, ROI_size, name):
        """csf_mask / ear_mask argument -> bool[ROI_size] (ref:852-894)."""
        aff = None
        if m is None:
            return np.zeros(ROI_size, dtype=bool), aff
        if np.isscalar(m) and not isinstance(m, str):
            return np.full(ROI_size, m > 0, dtype=bool), aff
        m, aff = _load_volume(m)
        if m.shape != img_shape:
            raise ValueError("Arg. %s incomptabible. Based on data, it should have shape (%s), detected (%s) instead."
                             % (name, " ".join("%d" % x for x in img_shape), " ".join("%d" % x for x in m.shape)))
        return (m[roi] > 0), aff

    def _fit_sharded(self, pgse_scheme, Y, rows, args, devs):
        """parallel=True: one host thread per GPU (ctypes releases the GIL), each device with its own copy of the
        tables.  The voxels of every class (numfasc, CSF, EAR: their cost differs by up to 40x) are dealt round-robin
        over the devices so that each gets the same mix (reference: mp.Pool over voxels, ref:978-1009).
        (Multi-process / multi-node runs use dist.py.)"""
        numfasc_roi, csf_mask, ear_mask, peaks_roi, maxfasc, csf_on, ear_on, sig_csf, sig_ear, num_ear = args
        V = numfasc_roi.shape[0]
        ndev = len(devs)
        out = [None] * ndev
        idx = [mdist.balanced_shard_indices(numfasc_roi, csf_mask, ear_mask, d, ndev) for d in range(ndev)]
        errs = []

        def work(d):
            try:
                ix = idx[d]
                ms = mfu.MultiShellInterpolator(self.ms_interpolator['scheme_DeldelTE'], self.ms_interpolator['Gms_un'],
                                                self.ms_interpolator['interpolators'], device=devs[d])
                part = (numfasc_roi[ix], csf_mask[ix], ear_mask[ix], peaks_roi[ix], maxfasc, csf_on, ear_on, sig_csf,
                        sig_ear, num_ear)
                if isinstance(Y, engine.FileOrderVolume):
                    out[d] = engine.fit_batch_volume(ms.plan_for(pgse_scheme), Y, rows[ix], *part)
                else:
                    out[d] = engine.fit_batch(ms.plan_for(pgse_scheme), Y, *part, rows=(ix if rows is None else rows[ix]))
            except Exception as e:   # re-raised below, like pool.get() (ref:1006-1008)
                errs.append(e)
        th = [threading.Thread(target=work, args=(d,)) for d in range(ndev)]
        [t.start() for t in th]
        [t.join() for t in th]
        if errs:
            raise errs[0]
        full = np.zeros((V, out[0].shape[1]))
        for d in range(ndev):
            full[idx[d]] = out[d]
        return full


class MFModelFit():
    """Fit object: one ndarray attribute per estimated map + ``param_names`` (ref:1054-1229)."""

    def __init__(self, fitinfo, model_params, verbose=0):
        self.affine = fitinfo['affine']
        nf, csf_on, ear_on, mask = fitinfo['maxfasc'], fitinfo['csf_on'], fitinfo['ear_on'], fitinfo['mask']
        ROI_size = model_params.shape[0]
        flat = fitinfo.get('roi_index')            # flat indices of the ROI voxels (== np.where(mask > 0) order)
        if flat is None:
            flat = np.flatnonzero(np.asarray(mask) > 0)
        assert ROI_size == flat.shape[0], 'Inconsistent mask and model parameter array'
        self.params_in_mask = model_params
        # what predict() needs (not maps: param_names and write_nifti do not see them)
        self._model, self._pgse_scheme = fitinfo.get('model'), fitinfo.get('pgse_scheme')
        self._nf, self._csf_on, self._ear_on = nf, bool(csf_on), bool(ear_on)
        self._peaks_roi, self._roi_flat, self._grid = fitinfo.get('peaks_roi'), flat, tuple(mask.shape)
        # per-voxel classes and per-atom properties (profile() and interval())
        self._numfasc_roi, self._csf_roi, self._ear_roi = (fitinfo.get(k) for k in ('numfasc_roi', 'csf_roi', 'ear_roi'))
        self._props = {n: np.asarray(fitinfo['_dict_' + n], dtype=np.float64).reshape(-1) for n in fitinfo['fasc_propnames']}
        self.weights_roi = fitinfo.get('weights_roi')   # float64 [ROI x M] or [M] of a weighted fit, else None (not a map)
        # of a robust fit (else None): the per-voxel diagnostics of engine.fit_robust, the base weights and the options
        self.robust_info, self._robust_base = fitinfo.get('robust_info'), fitinfo.get('robust_base')
        self.robust_options = fitinfo.get('robust_options')
        whole = ROI_size == int(np.prod(mask.shape))

        def to_map(vals, extra=()):
            if whole:     # every voxel is in the ROI: the map is the parameter column itself, reshaped
                return np.array(vals, dtype=np.float64).reshape(mask.shape + tuple(extra))
            m = np.zeros(mask.shape + tuple(extra))
            m.reshape((-1,) + tuple(extra))[flat] = vals
            return m
        names = ['M0']
        self.M0 = to_map(model_params[:, 0])
        for k in range(nf):
            setattr(self, 'frac_f%d' % k, to_map(model_params[:, k + 1]))
            setattr(self, 'peak_f%d' % k, to_map(fitinfo['peaks_roi'][:, 3 * k:3 * (k + 1)], (3,)))
            names += ['frac_f%d' % k, 'peak_f%d' % k]
        IDs = [model_params[:, 1 + nf + k].astype(np.intp) for k in range(nf)]
        active = [model_params[:, k + 1] > 0 for k in range(nf)]
        for prop in fitinfo['fasc_propnames']:     # per-fascicle properties and nu-weighted totals (ref:1106-1129)
            tot = np.zeros(ROI_size)
            for k in range(nf):
                nu_k = model_params[:, k + 1]
                prop_k = fitinfo['_dict_' + prop][IDs[k]] * active[k]
                tot += nu_k * prop_k
                setattr(self, prop + '_f%d' % k, to_map(prop_k))
                names.append(prop + '_f%d' % k)
            setattr(self, prop + '_tot', to_map(tot))
            names.append(prop + '_tot')
        if csf_on:
            self.frac_csf = to_map(model_params[:, 2 * nf + 1])
            names.append('frac_csf')
        if ear_on:
            nu_e = model_params[:, 2 * nf + csf_on + 1]
            self.frac_ear = to_map(nu_e)
            ID_e = model_params[:, 2 * nf + csf_on + 2].astype(int)
            self.D_ear = to_map(fitinfo['DIFF_ear'][ID_e] * (nu_e > 0))
            names += ['frac_ear', 'D_ear']
        self.MSE = to_map(model_params[:, -2])
        self.R2 = to_map(model_params[:, -1])
        names += ['MSE', 'R2']
        self.param_names = names
        if self.robust_info is not None:   # maps of a robust fit (not in param_names: write_nifti leaves them out)
            self.robust_scale = to_map(self.robust_info['scale'])
            self.n_rejected = to_map(np.count_nonzero(self._rejected_roi(), axis=1))
        if verbose >= 2:
            print("Microstructure Fingerprinting fit object constructed; maps: %s" % ", ".join(names))

    def _rejected_roi(self):
        """bool [ROI x M]: the base rows (positive base weight; every row without base weights) whose final weight is 0."""
        if self.robust_info is None:
            raise RuntimeError("this fit is not a robust fit (MFModel.fit(..., robust=...)): it has rejected nothing")
        base = np.ones(self.weights_roi.shape[1], dtype=bool) if self._robust_base is None else np.asarray(self._robust_base) > 0
        return base & (self.weights_roi == 0)

    def outlier_mask(self):
        """The measurements a robust fit rejected, bool of shape ``mask.shape + (M,)``: True where a row the base weights
        admit ended with weight 0 (False outside the ROI)."""
        rej = self._rejected_roi()
        out = np.zeros((int(np.prod(self._grid)), rej.shape[1]), dtype=bool)
        out[self._roi_flat] = rej
        return out.reshape(self._grid + (rej.shape[1],))

    PREDICT_CHUNK = 1 << 16   # ROI voxels per device call of predict() / residuals()

    def _predict_chunks(self):
        """The predicted signals of the ROI, PREDICT_CHUNK voxels at a time: (ROI slice, [n x M] float64)."""
        if self._model is None or self._pgse_scheme is None:
            raise RuntimeError("this fit object was not made by MFModel.fit: it knows neither its model nor its protocol")
        m = self._model
        for i0 in range(0, self._roi_flat.shape[0], self.PREDICT_CHUNK):
            sl = slice(i0, i0 + self.PREDICT_CHUNK)
            P = self.params_in_mask[sl]
            # a voxel whose parameters cannot be predicted (non-finite or negative weights, an index outside the
            # dictionary: a fit of unusable data) gets a NaN row; it does not stop the volume
            bad = engine.predict_bad_rows(P, self._nf, self._csf_on, self._ear_on, int(m.dic['num_atom']), int(m.dic['num_ear']))
            if bad.any():
                P = np.where(bad[:, None], 0.0, P)
            pred = m.predict(P, self._peaks_roi[sl], pgse_scheme=self._pgse_scheme)
            if bad.any():
                pred[bad] = np.nan
            yield sl, pred

    def _volume_out(self, out, dtype):
        shape = self._grid + (self._pgse_scheme.shape[0],)
        if out is None:
            return np.zeros(shape, dtype=dtype)
        if not isinstance(out, np.ndarray) or out.shape != shape or not out.flags.c_contiguous:
            raise ValueError("out should be a C-contiguous array of shape (%s)" % " ".join("%d" % x for x in shape))
        out[...] = 0
        return out

    def predict(self, dtype=np.float64, out=None):
        """The signal the fitted parameters stand for, shape ``mask.shape + (M,)``, zeros outside the ROI (the
        reference computes it in every voxel, ref:413-419, and drops it).  ``dtype`` (or ``out``'s type) may be
        np.float32: the volume is rounded from the float64 prediction one chunk of voxels at a time, so that a
        whole-brain prediction never exists in float64.  A voxel whose parameters cannot be predicted (a weight that is
        negative or not finite, an atom index outside its dictionary) is NaN."""
        vol = self._volume_out(out, dtype)
        rows = vol.reshape(-1, vol.shape[-1])
        for sl, pred in self._predict_chunks():
            rows[self._roi_flat[sl]] = pred
        return vol

    def residuals(self, data, dtype=np.float64, out=None):
        """``data - predict()`` inside the ROI, zeros outside; ``data`` as given to ``fit`` (array or NIfTI file)."""
        data_arr, _ = _load_volume(data)
        vol = self._volume_out(out, dtype)
        if data_arr.shape != vol.shape:
            raise ValueError("data should have shape (%s), got (%s)" % (" ".join("%d" % x for x in vol.shape),
                                                                        " ".join("%d" % x for x in data_arr.shape)))
        rows = vol.reshape(-1, vol.shape[-1])
        for sl, pred in self._predict_chunks():
            idx = self._roi_flat[sl]
            rows[idx] = np.asarray(data_arr[np.unravel_index(idx, self._grid)], dtype=np.float64) - pred
        return vol

    PROFILE_BYTES = 256 << 20   # largest [chunk x K x N] float64 buffer of interval()

    def _profile_setup(self, data):
        if self._model is None or self._pgse_scheme is None or self._numfasc_roi is None:
            raise RuntimeError("this fit object was not made by MFModel.fit: it knows neither its model nor its protocol "
                               "nor the voxels' classes")
        data_arr, _ = _load_volume(data)
        shape = self._grid + (self._pgse_scheme.shape[0],)
        if data_arr.shape != shape:
            raise ValueError("data should have shape (%s), got (%s)" % (" ".join("%d" % x for x in shape),
                                                                        " ".join("%d" % x for x in data_arr.shape)))
        m = self._model
        sig_csf = m._extra_signals(self._pgse_scheme, self._csf_on, False)[0]
        return data_arr, m.ms_interpolator.plan_for(self._pgse_scheme), sig_csf

    def _data_rows(self, data_arr, idx):
        return np.ascontiguousarray(data_arr[np.unravel_index(idx, self._grid)], dtype=np.float64)

    def _weights_rows(self, vox):
        """The measurement weights of the ROI positions ``vox`` for the profile and posterior entry points: None for an
        unweighted fit, the shared [M] vector as it is, else the voxels' rows [n x M]."""
        W = self.weights_roi
        if W is None:
            return None
        W = np.asarray(W, dtype=np.float64)
        return W if W.ndim == 1 else np.ascontiguousarray(W[vox])

    def profile(self, data, voxels=None, partner=False):
        """What the exhaustive search saw beside its arg-min: for every atom of each fascicle the smallest sum of
        squared residuals any partner atom reaches with it (``engine.profile``).  ``data`` as given to ``fit``;
        ``voxels``: positions in the ROI (default: all of it - [ROI x maxfasc x N] float64 on the host, meant for
        regions, not for brains: see ``interval``).  Returns an object with ``obj`` [n x maxfasc x N], ``partner``
        (int32, -1 where there is none; None unless asked for), ``n_unsupported`` (voxels with EAR or without a
        fascicle: their rows are NaN) and ``by_property(name)`` -> (levels, obj_by_level).  After a weighted fit the
        values are those of the weighted objective sum_m W (y_m - model_m)^2 (``weights_roi``), so that the smallest one
        is the fit's own MSE * sum_m W."""
        data_arr, plan, sig_csf = self._profile_setup(data)
        vox = np.arange(self._roi_flat.shape[0]) if voxels is None else np.asarray(voxels, dtype=np.int64).reshape(-1)
        obj, par, n_uns = engine.profile(plan, self._data_rows(data_arr, self._roi_flat[vox]), self._numfasc_roi[vox],
                                         self._csf_roi[vox], self._peaks_roi[vox], self._nf, self._csf_on, sig_csf,
                                         partner=partner, ear=self._ear_roi[vox], W=self._weights_rows(vox))
        return ObjectiveProfile(obj, par, n_uns, vox, self._props)

    def interval(self, data, name, rel=0.0, delta=0.0):
        """The range of the fascicle property ``name`` (one of the dictionary's ``fasc_propnames``) that fits the data
        within a margin of the optimum: per voxel and fascicle, over the atoms whose profile value is at most
        ``min * (1 + rel) + delta``, the smallest and largest property value and the number of such atoms
        (``mf_utils.profile_interval``).  Returns ``(lo, hi, count)`` volumes of shape ``mask.shape + (maxfasc,)``;
        NaN / 0 outside the ROI, for absent fascicles and for voxels out of the profile's scope.  The profiles are
        computed and reduced on the device, PROFILE_BYTES of them at a time; only the three numbers per voxel and
        fascicle come back."""
        import torch
        if name not in self._props:
            raise ValueError("unknown fascicle property %s (have: %s)" % (name, ", ".join(sorted(self._props))))
        data_arr, plan, sig_csf = self._profile_setup(data)
        nf, R = self._nf, self._roi_flat.shape[0]
        N = plan.tables.N
        dev = torch.device("cuda", plan.tables.device)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        d_csf = t(sig_csf) if self._csf_on else None
        shared_W = self.weights_roi is not None and np.ndim(self.weights_roi) == 1
        d_Ws = t(self._weights_rows(None)) if shared_W else None   # a shared [M] vector is passed once
        lo, hi = np.full((R, nf), np.nan), np.full((R, nf), np.nan)
        cnt = np.zeros((R, nf), dtype=np.int64)
        chunk = max(1, int(self.PROFILE_BYTES // (8 * 2 * N)))
        bins, _ = engine.profile_classes(self._numfasc_roi, self._csf_roi, self._ear_roi, nf)
        with torch.cuda.device(dev):
            for k, c, ix in bins:
                for i0 in range(0, ix.size, chunk):
                    sub = ix[i0:i0 + chunk]
                    d_W = d_Ws if (shared_W or self.weights_roi is None) else t(self._weights_rows(sub))
                    obj = engine.profile_dev(plan, t(self._data_rows(data_arr, self._roi_flat[sub])),
                                             t(self._peaks_roi[sub, :3 * k]), k, c, d_csf if c else None, d_W=d_W)
                    l, h, n = mfu.profile_interval(obj, self._props[name], rel, delta)
                    L.check(L.lib().mfx_plan_status(plan.handle(), torch.cuda.current_stream(dev).cuda_stream))
                    lo[sub, :k], hi[sub, :k], cnt[sub, :k] = l.cpu().numpy(), h.cpu().numpy(), n.cpu().numpy()

        def to_map(vals, fill):
            m = np.full((int(np.prod(self._grid)), nf), fill, dtype=vals.dtype)
            m[self._roi_flat] = vals
            return m.reshape(self._grid + (nf,))
        return to_map(lo, np.nan), to_map(hi, np.nan), to_map(cnt, 0)

    def _posterior_inputs(self, sigma, vox):
        """(sigma [n], shift [n]) of the ROI positions ``vox``: the shift is the fit's own objective MSE * M; ``sigma``
        None means sigma^2 = MSE * M / (M - K - csf), the residual variance of the fit.  After a weighted fit the
        objective is MSE * sum_m W and M becomes the number of positive weights; no degree of freedom left gives NaN."""
        M = self._pgse_scheme.shape[0]
        W = self._weights_rows(vox)
        if W is None:
            sse = np.asarray(self.params_in_mask[vox, -2], dtype=np.float64) * M
            n_pos = M
        else:
            with np.errstate(invalid='ignore', over='ignore'):
                sse = np.asarray(self.params_in_mask[vox, -2], dtype=np.float64) * np.sum(W, axis=-1)
                n_pos = np.count_nonzero(W > 0, axis=-1).astype(np.float64)
        if sigma is None:
            dof = n_pos - self._numfasc_roi[vox].astype(np.float64) - self._csf_roi[vox].astype(np.float64)
            with np.errstate(invalid='ignore', divide='ignore'):
                sig = np.sqrt(sse / dof)
            if W is not None:
                sig = np.where(dof > 0, sig, np.nan)
        else:
            sig = np.asarray(sigma, dtype=np.float64)
            if sig.ndim == 0:
                sig = np.full(vox.shape[0], float(sig))
            elif sig.shape == (self._roi_flat.shape[0],):
                sig = sig[vox]
            else:
                raise ValueError("sigma should be a scalar or have one entry per ROI voxel (%d), got shape %s"
                                 % (self._roi_flat.shape[0], sig.shape))
        return np.ascontiguousarray(sig), np.ascontiguousarray(sse)

    def posterior(self, data, sigma=None, voxels=None):
        """The soft answer beside the arg-min: for every atom of each fascicle its posterior weight given the noise
        level, w proportional to the sum over all partner atoms of exp(-F / 2 sigma^2) (``engine.posterior``).  ``data``
        as given to ``fit``; ``sigma``: the noise standard deviation, a scalar or one value per ROI voxel (default: the
        fit's residual variance, sigma^2 = MSE * M / (M - K - csf) per voxel; a voxel with MSE = 0 gets status 1);
        ``voxels``: positions in the ROI (default: all of it - [ROI x maxfasc x N] float64 on the host, meant for
        regions: see ``posterior_moments``).  Returns a ``Posterior``.  After a weighted fit F is the weighted objective
        (``weights_roi``) and ``sigma`` the noise of a measurement of weight 1: measurement m has variance sigma^2 / W_m;
        the default is sigma^2 = MSE * sum_m W / (n_pos - K - csf) with n_pos the number of positive weights."""
        data_arr, plan, sig_csf = self._profile_setup(data)
        vox = np.arange(self._roi_flat.shape[0]) if voxels is None else np.asarray(voxels, dtype=np.int64).reshape(-1)
        sig, shift = self._posterior_inputs(sigma, vox)
        W = self._weights_rows(vox)
        w, log_sum, status, n_uns = engine.posterior(plan, self._data_rows(data_arr, self._roi_flat[vox]),
                                                     self._numfasc_roi[vox], self._csf_roi[vox], self._peaks_roi[vox],
                                                     self._nf, self._csf_on, sig_csf, sig, shift=shift, ear=self._ear_roi[vox],
                                                     W=W)
        return Posterior(w, log_sum, status, n_uns, vox, self._props, self._numfasc_roi[vox], 2.0 * sig ** 2, plan.M, W=W)

    def posterior_moments(self, data, name, sigma=None):
        """Posterior mean and standard deviation of the fascicle property ``name`` (one of the dictionary's
        ``fasc_propnames``) per voxel and fascicle (``mf_utils.posterior_moments`` of the weights of ``posterior``):
        ``(mean, std)`` volumes of shape ``mask.shape + (maxfasc,)``; NaN outside the ROI, for absent fascicles, for
        voxels out of the posterior's scope (EAR, no fascicle) and for voxels with a non-zero status.  The weights are
        computed and reduced on the device, PROFILE_BYTES of them at a time; only the two numbers per voxel and
        fascicle come back."""
        import torch
        if name not in self._props:
            raise ValueError("unknown fascicle property %s (have: %s)" % (name, ", ".join(sorted(self._props))))
        data_arr, plan, sig_csf = self._profile_setup(data)
        nf, R = self._nf, self._roi_flat.shape[0]
        N = plan.tables.N
        sig, shift = self._posterior_inputs(sigma, np.arange(R))
        dev = torch.device("cuda", plan.tables.device)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        d_csf = t(sig_csf) if self._csf_on else None
        shared_W = self.weights_roi is not None and np.ndim(self.weights_roi) == 1
        d_Ws = t(self._weights_rows(None)) if shared_W else None   # a shared [M] vector is passed once
        mean, std = np.full((R, nf), np.nan), np.full((R, nf), np.nan)
        chunk = max(1, int(self.PROFILE_BYTES // (8 * 2 * N)))
        bins, _ = engine.profile_classes(self._numfasc_roi, self._csf_roi, self._ear_roi, nf)
        with torch.cuda.device(dev):
            for k, c, ix in bins:
                for i0 in range(0, ix.size, chunk):
                    sub = ix[i0:i0 + chunk]
                    d_W = d_Ws if (shared_W or self.weights_roi is None) else t(self._weights_rows(sub))
                    w, _, _ = engine.posterior_dev(plan, t(self._data_rows(data_arr, self._roi_flat[sub])),
                                                   t(self._peaks_roi[sub, :3 * k]), k, t(2.0 * sig[sub] ** 2), t(shift[sub]),
                                                   c, d_csf if c else None, d_W=d_W)
                    m, sd = mfu.posterior_moments(w, self._props[name])
                    L.check(L.lib().mfx_plan_status(plan.handle(), torch.cuda.current_stream(dev).cuda_stream))
                    mean[sub, :k], std[sub, :k] = m.cpu().numpy(), sd.cpu().numpy()

        def to_map(vals):
            m = np.full((int(np.prod(self._grid)), nf), np.nan)
            m[self._roi_flat] = vals
            return m.reshape(self._grid + (nf,))
        return to_map(mean), to_map(std)

    def bootstrap(self, data, B=200, *, kind='wild', seed=0, inflate=True, q=(0.025, 0.975), voxels=None, keep=False,
                  groups=None, fixed_weights=False):
        """Model-free uncertainty of every estimated parameter: the residuals of each voxel's own fit are resampled
        into ``B`` replicate signals, every replicate is fitted by the plain fit, and the B parameter rows of a voxel
        are reduced to statistics, all on the device (``engine.fit_bootstrap``; include/mfx_boot.h states the rule).
        ``data`` as given to ``fit``.  ``kind`` 'wild' flips the sign of every residual at random; 'residual' draws, for
        every measurement, a residual of its group - ``groups`` [M] integers, default: rows sharing (G, Delta, delta).
        ``inflate`` scales the residuals by sqrt(M / (M - number of active compartments)).  ``q``: the quantiles kept.
        ``voxels``: positions in the ROI (default: all of it); the random stream is keyed by the ROI position, so a
        subset gives the replicates the whole ROI gives.  ``keep``: also return the replicate parameter rows.  Every
        voxel class of the plain fit is served (CSF, EAR).  A fit made with ``weights=`` or ``robust=`` is served only
        with ``fixed_weights=True``: the bootstrap then holds the fit's final measurement weights (``weights_roi``) fixed
        - every replicate is fitted by the weighted fit on those weights and the fit's own parameters are the ones
        resampled around (``engine.fit_weighted_bootstrap``; include/mfx_wboot.h states the rule).  No replicate re-runs
        the rejection, so after a robust fit the result is CONDITIONAL ON THE ROWS THAT WERE REJECTED: it says how
        stable the estimate is given that choice of outliers, not how stable the choice is.  Rows of weight 0 are left
        as measured, 'residual' draws among the rows of positive weight in units of sqrt(weight), and ``inflate`` counts
        the rows of positive weight.  ``fixed_weights=True`` on a fit without weights is a ValueError.
        Returns a ``BootstrapResult``."""
        if not isinstance(fixed_weights, (bool, np.bool_)):
            raise ValueError("fixed_weights should be True or False, got %r" % (fixed_weights,))
        weighted = self.weights_roi is not None or self.robust_info is not None
        if weighted and not fixed_weights:
            raise NotImplementedError("bootstrap of a weighted or robust fit is not served")
        if fixed_weights and self.weights_roi is None:
            raise ValueError("fixed_weights=True needs a fit made with weights= or robust=: this fit has no measurement weights")
        B, _, qa = engine._boot_rule(B, kind, q, seed)
        if self._model is None or self._pgse_scheme is None or self._numfasc_roi is None:
            raise RuntimeError("this fit object was not made by MFModel.fit: it knows neither its model nor its protocol "
                               "nor the voxels' classes")
        sch = self._pgse_scheme
        gr = engine._boot_groups_arg(engine.BOOT_KINDS[kind], groups, sch.shape[0], sch)
        R = self._roi_flat.shape[0]
        vox = np.arange(R) if voxels is None else np.asarray(voxels, dtype=np.int64).reshape(-1)
        if vox.size and (vox.min() < 0 or vox.max() >= R):
            raise ValueError("voxels should be positions in the ROI (0..%d)" % (R - 1))
        data_arr, _ = _load_volume(data)
        shape = self._grid + (sch.shape[0],)
        if data_arr.shape != shape:
            raise ValueError("data should have shape (%s), got (%s)" % (" ".join("%d" % x for x in shape),
                                                                        " ".join("%d" % x for x in data_arr.shape)))
        m = self._model
        sig_csf, sig_ear, num_ear = m._extra_signals(sch, self._csf_on, self._ear_on)
        plan = m.ms_interpolator.plan_for(sch)
        names = list(self._props)
        props = np.stack([self._props[n] for n in names]) if names else None
        if fixed_weights:
            W = np.asarray(self.weights_roi, dtype=np.float64)
            W = W if W.ndim == 1 else np.ascontiguousarray(W[vox])   # the shared [M] vector as it is, else the voxels' rows
            res = engine.fit_weighted_bootstrap(plan, self._data_rows(data_arr, self._roi_flat[vox]), W, self._numfasc_roi[vox],
                                                self._csf_roi[vox], self._peaks_roi[vox] if self._nf > 0 else None, self._nf,
                                                self._csf_on, sig_csf, B=B, kind=kind, seed=seed, inflate=inflate, q=qa,
                                                props=props, groups=gr, params=np.ascontiguousarray(self.params_in_mask[vox]),
                                                vox=vox, keep=keep)
            return BootstrapResult(res, names, qa, vox, self._roi_flat, self._grid, self._nf, self._csf_on, False, B, seed,
                                   weights=W)
        res = engine.fit_bootstrap(plan, self._data_rows(data_arr, self._roi_flat[vox]), self._numfasc_roi[vox],
                                   self._csf_roi[vox], self._ear_roi[vox], self._peaks_roi[vox] if self._nf > 0 else None,
                                   self._nf, self._csf_on, self._ear_on, sig_csf, sig_ear, num_ear, B=B, kind=kind, seed=seed,
                                   inflate=inflate, q=qa, props=props, groups=gr,
                                   params=np.ascontiguousarray(self.params_in_mask[vox]), vox=vox, keep=keep)
        return BootstrapResult(res, names, qa, vox, self._roi_flat, self._grid, self._nf, self._csf_on, self._ear_on, B, seed)

    def write_nifti(self, output_basename, affine=None):
        """One NIfTI file per parameter map, ``<stem>_<param><ext>``; returns the file names (reference mf.py:1177-1229).
        ``output_basename`` may end in .nii.gz (kept), .nii or nothing (both give .nii); any other extension is refused."""
        xfm = self.affine if affine is None else affine
        if xfm is None:
            raise ValueError("Argument affine must be explicitely passed  because no affine transform matrix was "
                             "found during model fitting. Expecting NumPy array with shape (4, 4).")
        stem, ext = _nifti_stem(output_basename)
        written = []
        for name in self.param_names:
            target = "%s_%s%s" % (stem, name, ext)
            nifti.save(getattr(self, name), xfm, target)
            written.append(target)
        return written


class ObjectiveProfile(object):
    """Result of ``MFModelFit.profile``: ``obj`` [n x maxfasc x N], ``partner`` (or None), ``n_unsupported``, ``voxels``
    (the ROI positions the rows stand for)."""

    def __init__(self, obj, partner, n_unsupported, voxels, props):
        self.obj, self.partner, self.n_unsupported, self.voxels, self._props = obj, partner, n_unsupported, voxels, props

    def by_property(self, name):
        """(levels, obj_by_level [n x maxfasc x len(levels)]): the profile as a function of the property ``name``."""
        if name not in self._props:
            raise ValueError("unknown fascicle property %s (have: %s)" % (name, ", ".join(sorted(self._props))))
        return mfu.profile_by_property(self.obj, self._props[name])


class Posterior(object):
    """Result of ``MFModelFit.posterior``: ``weights`` [n x maxfasc x N] (each present fascicle's row sums to 1; NaN rows
    for absent fascicles, voxels out of scope and voxels with a non-zero status), ``log_sum`` [n] = log of the sum of
    exp(-F / T) over all atoms (pairs), ``status`` [n] (0 ok, 1 unusable temperature, 2 unusable shift, 3 a measurement
    weight that is negative or not finite, 4 no positive measurement weight - the last two after a weighted fit only -,
    -1 a voxel class out of scope), ``n_unsupported``, ``voxels`` (the ROI positions the rows stand for).  ``W``: the
    measurement weights [n x M] or [M] the posterior was computed with (None: an unweighted fit)."""

    def __init__(self, weights, log_sum, status, n_unsupported, voxels, props, numfasc, T, M, W=None):
        self.weights, self.log_sum, self.status, self.n_unsupported, self.voxels = weights, log_sum, status, n_unsupported, voxels
        self._props, self._K, self._T, self._M = props, np.asarray(numfasc, dtype=np.float64), np.asarray(T, dtype=np.float64), int(M)
        # of a weighted posterior: the number of positive weights and the sum of their logarithms, per voxel (or shared)
        self._n_pos, self._sum_log_w = None, None
        if W is not None:
            W = np.asarray(W, dtype=np.float64)
            pos = W > 0
            self._n_pos = np.count_nonzero(pos, axis=-1).astype(np.float64)
            with np.errstate(invalid='ignore', divide='ignore'):
                self._sum_log_w = np.sum(np.log(np.where(pos, W, 1.0)), axis=-1)

    def _values(self, name):
        if name not in self._props:
            raise ValueError("unknown fascicle property %s (have: %s)" % (name, ", ".join(sorted(self._props))))
        return self._props[name]

    def mean(self, name):
        """Posterior mean of the property ``name`` [n x maxfasc]."""
        return mfu.posterior_moments(self.weights, self._values(name))[0]

    def std(self, name):
        """Posterior standard deviation of the property ``name`` [n x maxfasc]."""
        return mfu.posterior_moments(self.weights, self._values(name))[1]

    def quantile(self, name, q):
        """Lower weighted quantile of the property ``name`` [n x maxfasc] (``mf_utils.posterior_quantile``)."""
        return mfu.posterior_quantile(self.weights, self._values(name), q)

    def by_property(self, name):
        """(levels, weight_by_level [n x maxfasc x len(levels)]): the posterior as a distribution over ``name``."""
        return mfu.posterior_by_property(self.weights, self._values(name))

    def log_evidence(self):
        """log_sum - K log N - (M / 2) log(pi T) per voxel: the log of the Gaussian likelihood averaged over a uniform
        prior on the K-tuples of atoms, which lets a one-fascicle and a two-fascicle explanation of the same voxel be
        compared.  It is a profile-likelihood evidence: the fascicle (and CSF) weights are maximised for every tuple,
        not integrated over.  NaN where log_sum is.  For a weighted posterior measurement m has variance T / (2 W_m), and
        the expression is log_sum - K log N - (n_pos / 2) log(pi T) + (1 / 2) sum over the positive weights of log W_m,
        n_pos their number: the same value when every weight is 1."""
        N = self.weights.shape[-1]
        with np.errstate(invalid='ignore', divide='ignore'):
            if self._n_pos is None:
                return self.log_sum - self._K * np.log(N) - 0.5 * self._M * np.log(np.pi * self._T)
            return self.log_sum - self._K * np.log(N) - 0.5 * self._n_pos * np.log(np.pi * self._T) + 0.5 * self._sum_log_w


class BootstrapResult(object):
    """Result of ``MFModelFit.bootstrap``.  ``mean(name)``, ``std(name)``, ``quantile(name, q)`` and ``n_valid(name)`` give
    volumes over the replicates of a voxel: ``name`` is a fascicle property of the dictionary (shape ``mask.shape +
    (maxfasc,)``; a replicate counts for fascicle k only where its weight nu_k is positive - ``n_valid`` says how many
    did), 'frac' (the fascicle weights, ``mask.shape + (maxfasc,)``), or 'M0', 'frac_csf', 'frac_ear', 'MSE'
    (``mask.shape``); these count every replicate.  NaN (0 for ``n_valid``) outside the mask and outside ``voxels``.
    ``agreement`` (``mask.shape + (maxfasc,)``): the share of replicates that chose the original fit's atom with a
    positive weight; ``status`` (``mask.shape``, -1 outside): 0 fine, 1 no degree of freedom, 2 original row not
    usable; ``B``, ``seed``, ``q``, ``voxels`` (the ROI positions bootstrapped); ``stats`` [n x C x (5 + Q)] with
    ``columns``, the table the maps are cut from; ``replicates`` [n x B x num_params] with ``keep=True``, else None.
    ``weights``: the measurement weights [n x M] or [M] a ``fixed_weights=True`` bootstrap held fixed (status then also
    3: a weight negative or not finite, 4: no positive weight), else None."""

    def __init__(self, res, prop_names, q, voxels, roi_flat, grid, nf, csf_on, ear_on, B, seed, weights=None):
        self.weights = weights
        self.stats, self.columns, self.replicates = res['stats'], res['columns'], res['replicates']
        self.B, self.seed, self.q, self.voxels = int(B), seed, np.asarray(q, dtype=np.float64), voxels
        self._names, self._flat, self._grid, self._nf = list(prop_names), roi_flat[voxels], tuple(grid), nf
        self._csf_on, self._ear_on = csf_on, ear_on
        self.agreement = self._to_map(res['agree'].astype(np.float64) / float(B), np.nan)
        self.status = self._to_map(res['status'], -1)

    def _to_map(self, vals, fill):
        vals = np.asarray(vals)
        m = np.full((int(np.prod(self._grid)),) + vals.shape[1:], fill, dtype=vals.dtype)
        m[self._flat] = vals
        return m.reshape(self._grid + vals.shape[1:])

    def _cols(self, name):
        """(column indices, per fascicle?) of a statistic's name."""
        if name in self._names:
            t = self._names.index(name)
            return [self.columns.index(('prop', k, t)) for k in range(self._nf)], True
        if name == 'frac':
            return [self.columns.index('nu_%d' % k) for k in range(self._nf)], True
        single = {'M0': 'M0', 'MSE': 'MSE'}
        if self._csf_on:
            single['frac_csf'] = 'nu_csf'
        if self._ear_on:
            single['frac_ear'] = 'nu_ear'
        if name in single:
            return [self.columns.index(single[name])], False
        raise ValueError("unknown bootstrap statistic %s (have: %s)" % (name, ", ".join(self._names + ['frac'] + sorted(single))))

    def _stat(self, name, i, fill=np.nan):
        cols, per_fasc = self._cols(name)
        vals = self.stats[:, cols, i] if per_fasc else self.stats[:, cols[0], i]
        return self._to_map(vals, fill)

    def n_valid(self, name):
        return self._stat(name, 0, 0.0).astype(np.int64)

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


def _nifti_stem(output_basename):
    """('dir/name', '.nii' | '.nii.gz') of an output name for MFModelFit.write_nifti."""
    if output_basename.endswith('.nii.gz') and len(output_basename) > len('.nii.gz'):
        return output_basename[:-len('.nii.gz')], '.nii.gz'
    stem, ext = os.path.splitext(output_basename)
    if ext and ext != '.nii':
        raise ValueError("Unknown NIfTI extension %s in output %s" % (ext, output_basename))
    return stem, '.nii'
