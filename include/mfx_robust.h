/*
 * mfx_robust.h -- C ABI of the robust fit: measurement weights derived from the residuals of a fit, and the loop
 * fit -> predict -> reweight -> weighted fit iterated on the device.  The fits are those of mfx.h (mfx_fit_batch) and
 * mfx_wfit.h (mfx_wfit_batch), the prediction is mfx_predict_dev of mfx_predict.h; the one new computation is the
 * weight rule below.  Kept apart from the other headers, with its own version.  Conventions are those of mfx_wfit.h:
 * plain pointers, row-major float64, 0 or an MFX_ERR_* code returned, mfx_last_error() gives the message, no CPU
 * path (without a usable device every entry point returns MFX_ERR_NO_DEVICE).
 *
 * The weight rule, per voxel, from the data row y [M], the prediction row p [M] and base weights W0 [M] (null: all
 * ones).  Every step is ONE correctly rounded float64 operation, in this order (fl = rounding to nearest even):
 *   a_m   = | fl(y_m - p_m) |
 *   B     = { m : W0[m] > 0 } (every m without W0), n0 = |B|
 *   s     = the median of a over B as numpy.median returns it: with the a_m of B ordered by (value, index) into
 *           a_(0) <= ... <= a_(n0-1):  odd n0: a_((n0-1)/2);  even n0: fl( fl(a_(n0/2-1) + a_(n0/2)) / 2 )
 *   thr   = fl(c s)
 *   psi_m = MFX_ROBUST_CUTOFF (0):  1 if a_m <= thr, else 0
 *           MFX_ROBUST_HUBER  (1):  1 if a_m <= thr, else fl(thr / a_m)
 *           MFX_ROBUST_TUKEY  (2):  u = fl(a_m / thr); if u < 1: t = fl(1 - fl(u u)), psi = fl(t t); else 0
 *   W[m]  = psi_m without W0; fl(W0[m] psi_m) for m in B; 0 for m outside B
 *   scale = s
 * state of a voxel, int32, the first that applies in the order 3, 1, 2; in a non-zero state W is a copy of W0 (ones
 * without W0): nothing is rejected, the voxel goes on with its base weights, and scale is NaN (state 3, 1) or 0 (2):
 *   0  reweighted
 *   3  a base weight is negative or not finite, or n0 = 0 (the weighted fit then reports its own status 1 / 2)
 *   1  some a_m, m in B, is not finite (the NaN row of a voxel the fit could not serve)
 *   2  s == 0: more than half of the rows of B are fitted exactly, rejection is undefined
 * With previous weights Wprev [V x M], changed[v] = 1 iff some W[v, m] differs bitwise from Wprev[v, m], else 0.
 * c >= 1 is required (MFX_ERR_ARG otherwise): with cutoff and huber the ceil(n0 / 2) rows of B with a_m <= s then keep a
 * positive weight, so reweighting never leaves a voxel without data.  tukey gives a row at u = 1 the weight 0, so the
 * same holds for c > 1 only: at c = 1 exactly the rows at the median go, and a voxel whose residuals all have one
 * magnitude keeps no row - the weighted fit then reports status 2 for it.
 * Protocols of more than 8192 measurements return MFX_ERR_UNSUPPORTED (the weighted fit's limit).
 *
 * The loop (mfx_rfit_batch_dev, mfx_rfit_batch), per voxel class:
 *   fit 0: the unweighted class fit (what mfx_fit_batch launches) without W0, else the weighted class fit on W0
 *   n_iter times: p = prediction of the current parameters -> W by the rule above from (y, p, W0) -> weighted fit on W
 * params rows are those of mfx_wfit_batch, [M0, nu_0 .., atom_0 .., (nu_csf if csf_on), MSE, R2], MSE and R2 those
 * of the last fit (weighted ones for n_iter > 0 or with W0); status is the last fit's (zeros after an unweighted one).
 * With n_iter = 0, W = W0 spread to [V x M] (ones without W0) and scale and state are zero.  n_changed[i] is the
 * number of voxels whose weights iteration i changed (iteration 0 against W0 spread, or the ones).
 * Not served: extra-axonal (EAR) columns - no argument carries them - and maxfasc > 3, which returns
 * MFX_ERR_UNSUPPORTED before anything is enqueued.  No convergence is promised: hard rejection can cycle, and n_changed
 * is the diagnostic.
 */
#ifndef MFX_ROBUST_H
#define MFX_ROBUST_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define MFX_ROBUST_CUTOFF 0
#define MFX_ROBUST_HUBER 1
#define MFX_ROBUST_TUKEY 2

/* version of this header's entry points; bumped on a signature change or a new entry point */
int mfx_robust_abi_version(void);

/* The weight rule alone on device buffers; needs no plan.  d_Y, d_P [V x M]; d_W0 [V x M] (w0_stride = M), [M]
 * (w0_stride = 0) or NULL; d_Wprev [V x M] or NULL -> d_W [V x M], d_scale [V], d_state [V] int32, d_changed [V] int32
 * (NULL: not wanted; without d_Wprev it is zero).  d_Wprev may be d_W itself (weights updated in place); d_W must not
 * overlap d_W0.  Only enqueues on `stream` (hipStream_t as void*, NULL = default stream). */
int mfx_robust_weights_dev(int M, const double* d_Y, const double* d_P, const double* d_W0, int64_t w0_stride, int loss,
                           double c, int64_t V, const double* d_Wprev, double* d_W, double* d_scale, int32_t* d_state,
                           int32_t* d_changed, void* stream);

/* The loop on one homogeneous class on device buffers: every voxel has K = maxfasc fascicles and no CSF column, as
 * mfx_wfit_batch_dev serves.  d_Y [V x M], d_W0 as above, d_peaks [V x 3 maxfasc] -> d_params [V x (1 + 2 maxfasc + 2)],
 * d_W [V x M], d_scale [V], d_state [V], d_status [V], d_nchanged [n_iter] int32.  Always runs all n_iter iterations
 * and only enqueues on `stream`. */
int mfx_rfit_batch_dev(const void* plan, const double* d_Y, const double* d_W0, int64_t w0_stride, const double* d_peaks,
                       int maxfasc, int loss, double c, int n_iter, int64_t V, double* d_params, double* d_W,
                       double* d_scale, int32_t* d_state, int32_t* d_status, int32_t* d_nchanged, void* stream);

/* The loop on a mixed batch on host buffers, binned by (K, CSF flag) as mfx_wfit_batch does: K [V] in 0..maxfasc,
 * csf [V] flags (NULL: none; flagged voxels need csf_on and sig_csf [M]), W0 [V x M], [M] or NULL, peaks
 * [V x 3 maxfasc] -> params [V x (1 + 2 maxfasc + csf_on + 2)], W_out [V x M], scale [V], state [V], status [V],
 * n_changed [n_iter] int64, *n_iter_used.  The data of a chunk of voxels is uploaded once and stays on the device
 * through its iterations.  A chunk stops once an iteration changed none of its weights - the kernels are
 * deterministic, so the results are those of all n_iter iterations; *n_iter_used is the largest number of iterations
 * a chunk ran.  Waits for its own work. */
int mfx_rfit_batch(const void* plan, const double* Y, const double* W0, int64_t w0_stride, const int32_t* K,
                   const uint8_t* csf, const double* peaks, int maxfasc, int csf_on, const double* sig_csf, int loss,
                   double c, int n_iter, int64_t V, double* params, double* W_out, double* scale, int32_t* state,
                   int32_t* status, int64_t* n_changed, int32_t* n_iter_used);

#ifdef __cplusplus
}
#endif
#endif
