/*
 * mfx_wfit.h -- C ABI of the weighted fit: mfx_fit_batch with a non-negative weight per voxel and measurement
 * (outlier masks, per-shell noise levels).  For weights W [V x M] the voxel's problem is
 *
 *   min_w  sum_m W[v,m] (y_m - sum_k w_k D_k[m, a_k])^2          w >= 0, one atom a_k per fascicle
 *
 * which is the reference chain on rows scaled by s = sqrt(W):
 *   solve_exhaustive_posweights(s[:, None] * A, s * y, dicsizes).
 * Kept apart from mfx.h, with its own version.  Conventions are those of mfx.h: plain pointers, row-major float64,
 * 0 or an MFX_ERR_* code returned, mfx_last_error() gives the message, no CPU path (without a usable device every
 * entry point returns MFX_ERR_NO_DEVICE).  With no weights a caller uses mfx_fit_batch: nothing there changed.
 *
 * Semantics, per voxel:
 *   s_m     = sqrt(W[v,m]), correctly rounded in float64
 *   a[m,i]  = fl(s_m * D_k[m,i]), D_k[m,i] bit for bit the entry mfx_rotate and the unweighted kernels produce
 *   y'_m    = fl(s_m * y_m)
 *   M0, nu_k, atom indices, nu_csf: what the reference chain returns on (a, y') - rotation,
 *           solve_exhaustive_posweights, the packing of mf.py:420-450 - with the strict-'<' first-hit rule in the
 *           reference's scan order.  The CSF column is scaled like the others.
 *   MSE     = min_obj / sum_m W[v,m]; for a 0/1 mask the MSE over the kept measurements.
 *   R2      = the squared weighted Pearson correlation of y and y_rec (weights W, weighted means); 0 when fewer than
 *           two weights are positive or a weighted variance is 0 (the analogue of mf.py:449-450).  For a 0/1 mask
 *           this is corrcoef over the kept rows.
 *   Indices, nu, MSE and R2 are invariant under W -> c W.
 * Weights are [V x M] (w_stride = M) or one [M] vector shared by all voxels (w_stride = 0).
 *
 * params row of a voxel (1 + 2 maxfasc + csf_on + 2 doubles), as mfx_fit_batch without EAR:
 *   [M0, nu_0 .. nu_{maxfasc-1}, atom_0 .. atom_{maxfasc-1}, (nu_csf if csf_on), MSE, R2]
 * status of a voxel, int32:
 *   0  fitted
 *   1  a weight is negative or not finite
 *   2  no positive weight (the reference would assert on all-zero columns)
 * A voxel with a non-zero status has a NaN row and is skipped by every kernel.  A fascicle direction that is not a
 * unit vector flags the plan's status word (mfx_plan_status), exactly as in the unweighted fit.
 *
 * Voxel classes: two fascicles without a CSF column run one fused kernel (the scaled dictionaries are never written
 * to memory) for dictionaries up to mfx_wfit_max_atoms(plan, 2) atoms; one fascicle without CSF runs a
 * one-thread-per-atom kernel.  Every other class (a CSF column, three fascicles, larger dictionaries) has its scaled
 * dictionaries materialised in voxel chunks and goes through the explicit solver behind mfx_solve_exhaustive on the
 * device: slow, same results.  K = 0 without CSF gives a zero row.
 * Not served: extra-axonal (EAR) columns - no argument carries them - and maxfasc > 3, which returns
 * MFX_ERR_UNSUPPORTED before anything is enqueued.
 */
#ifndef MFX_WFIT_H
#define MFX_WFIT_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* version of this header's entry points; bumped on a signature change or a new entry point */
int mfx_wfit_abi_version(void);

/* largest dictionary the fused kernel of K fascicles serves on this plan's protocol (0: no fused kernel) */
int mfx_wfit_max_atoms(const void* plan, int K);

/* One homogeneous class on device buffers: every voxel has K = maxfasc fascicles and no CSF column.
 * d_Y [V x M], d_W [V x M] (w_stride = M) or [M] (w_stride = 0), d_peaks [V x 3 maxfasc]
 * -> d_params [V x (1 + 2 maxfasc + 2)], d_status [V].
 * Only enqueues on `stream` (hipStream_t as void*, NULL = default stream). */
int mfx_wfit_batch_dev(const void* plan, const double* d_Y, const double* d_W, int64_t w_stride, const double* d_peaks,
                       int maxfasc, int64_t V, double* d_params, int32_t* d_status, void* stream);

/* A mixed batch on host buffers: K [V] in 0..maxfasc, csf [V] flags (NULL: none; flagged voxels need csf_on and
 * sig_csf [M]), W as above, peaks [V x 3 maxfasc] -> params [V x (1 + 2 maxfasc + csf_on + 2)], status [V].  Bins
 * the voxels by class, uploads class by class and waits for its own work. */
int mfx_wfit_batch(const void* plan, const double* Y, const double* W, int64_t w_stride, const int32_t* K,
                   const uint8_t* csf, const double* peaks, int maxfasc, int csf_on, const double* sig_csf, int64_t V,
                   double* params, int32_t* status);

/* diagnostics: 1 = every class of the calling thread's next calls takes the materialise-and-solve path */
void mfx_wfit_debug_set_force_explicit(int enabled);

#ifdef __cplusplus
}
#endif
#endif
