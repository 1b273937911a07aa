/*
 * mfx_robust2d.h -- C ABI of the robust fit of voxels of a 2-D (AxCaliber-like) protocol: the loop of mfx_robust.h,
 * fit -> predict -> reweight -> weighted fit iterated on the device, on a handle of mfx_rot2d.h (mfx_rot2d_create).
 * The fits are those of mfx_fit2d.h and mfx_w2d.h, the prediction is that of mfx_predict2d.h, the weight rule, its
 * states, the loss codes MFX_ROBUST_* and the condition c >= 1 are those of mfx_robust.h (mfx_robust_weights_dev, which
 * needs no plan, is the rule alone).  Kept apart from the other headers, with its own version.  Conventions are those
 * of mfx_w2d.h: plain pointers, row-major float64, 0 or an MFX_ERR_* code returned, mfx_last_error() gives the message,
 * no CPU path (without a usable device every entry point returns MFX_ERR_NO_DEVICE).
 *
 * The loop, per voxel class:
 *   fit 0: the unweighted class fit (what mfx_fit2d_batch launches) without W0, else the weighted class fit on W0
 *   n_iter times: p = prediction of the current parameters -> W by the rule from (y, p, W0), in place -> weighted fit on W
 * The directions' plan and the kernels' records are computed ONCE per class chunk and serve fit 0, every prediction and
 * every refit.  params rows are those of mfx_wfit2d_batch; MSE and R2 are those of the last fit.  dir_status [V x 5] is the
 * record of mfx_fit2d.h, wstatus [V] the weighted fit's weight status (mfx_w2d.h; zeros after an unweighted fit).  With
 * n_iter = 0, W = W0 spread to [V x M] (ones without W0) and scale and state are zero.  n_changed[i] is the number of
 * voxels whose weights iteration i changed.
 * A voxel with a failing direction has a NaN row: its prediction is NaN, its state 1, it keeps its base weights, and its
 * dir_status says why.  A voxel with unusable base weights has state 3 and the weighted fit's wstatus.
 * Not served: extra-axonal (EAR) columns - no argument carries them - and maxfasc > 3 (MFX_ERR_UNSUPPORTED).
 */
#ifndef MFX_ROBUST2D_H
#define MFX_ROBUST2D_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* version of this header's entry points; bumped on a signature change or a new entry point */
int mfx_robust2d_abi_version(void);

/* The loop on one homogeneous class on device buffers: every voxel has K = maxfasc fascicles and no CSF column.
 * d_Y [V x M], d_W0 [V x M] (w0_stride = M), [M] (w0_stride = 0) or NULL, d_peaks [V x 3 maxfasc] -> d_params
 * [V x (1 + 2 maxfasc + 2)], d_W [V x M], d_scale [V], d_state [V], d_dir_status [V x 5], d_wstatus [V], d_nchanged
 * [n_iter] int32.  Always runs all n_iter iterations and only enqueues on `stream` (hipStream_t as void*, NULL = default
 * stream). */
int mfx_rfit2d_batch_dev(void* h, const double* d_Y, const double* d_W0, int64_t w0_stride, const double* d_peaks, int maxfasc,
                         int loss, double c, int n_iter, int64_t V, double* d_params, double* d_W, double* d_scale,
                         int32_t* d_state, int32_t* d_dir_status, int32_t* d_wstatus, int32_t* d_nchanged, void* stream);

/* The loop on a mixed batch on host buffers, binned by (K, CSF flag) as mfx_wfit2d_batch does: K [V] in 0..maxfasc,
 * csf [V] flags (NULL: none; flagged voxels need csf_on and sig_csf [M]), W0 [V x M], [M] or NULL, peaks
 * [V x 3 maxfasc] -> params [V x (1 + 2 maxfasc + csf_on + 2)], W_out [V x M], scale [V], state [V], dir_status [V x 5],
 * wstatus [V], n_changed [n_iter] int64, *n_iter_used.  The data of a chunk of voxels is uploaded once and stays on the
 * device through its iterations.  A chunk stops once an iteration changed none of its weights - the kernels are
 * deterministic, so the results are those of all n_iter iterations; *n_iter_used is the largest number of iterations
 * a chunk ran.  Waits for its own work. */
int mfx_rfit2d_batch(void* h, const double* Y, const double* W0, int64_t w0_stride, const int32_t* K, const uint8_t* csf,
                     const double* peaks, int maxfasc, int csf_on, const double* sig_csf, int loss, double c, int n_iter,
                     int64_t V, double* params, double* W_out, double* scale, int32_t* state, int32_t* dir_status,
                     int32_t* wstatus, int64_t* n_changed, int32_t* n_iter_used);

/* diagnostics: the number of directions the calling thread's last mfx_rfit2d_* call handed to the plan kernel */
int64_t mfx_robust2d_debug_last_plan_directions(void);

#ifdef __cplusplus
}
#endif
#endif
