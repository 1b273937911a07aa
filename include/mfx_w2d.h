/*
 * mfx_w2d.h -- C ABI of measurement weights for voxels measured with a 2-D (AxCaliber-like) protocol: the fit of
 * mfx_fit2d.h and the soft fits and objective profiles of mfx_soft2d.h with a weight W[v, m] >= 0 per voxel and
 * measurement, on a handle of mfx_rot2d.h (mfx_rot2d_create).  What mfx_wfit.h and mfx_wsoft.h give for multi-shell
 * plans.  Kept apart from every other header, with its own version.  Conventions are those of mfx_fit2d.h: plain
 * pointers, row-major float64, 0 or an MFX_ERR_* code returned, mfx_last_error() gives the message, no CPU path
 * (without a usable device every entry point returns MFX_ERR_NO_DEVICE).  The _dev variants take device pointers and
 * a hipStream_t (as void*, NULL = default stream) and only enqueue work; the others wait for their own work.
 *
 * Definitions.  The voxel's problem is  min sum_m W[v,m] (y_m - sum_k w_k D_k[m, a_k])^2,  w >= 0.  With
 * s_m = sqrt(W[v,m]) (correctly rounded), a[m,i] = fl(s_m * D_k[m,i]) - D_k[m,i] bit for bit the entry
 * mfx_rot2d_rotate returns, the product a separate operation - and y'_m = fl(s_m y_m), every result is the
 * unweighted one on (a, y'); a CSF column is scaled like the others.
 *   Fit       M0, nu, atoms and nu_csf are the reference chain's on (a, y') with its strict-< first hit (the row
 *             layout of mfx_fit2d.h).  MSE = min_obj / sum_m W.  R2 is the squared weighted Pearson correlation of y
 *             and the unscaled y_rec (weighted means, weights W); 0 with fewer than two positive weights or a
 *             vanishing weighted variance.
 *   Profile, posterior   F_W is exactly the F of mfx_soft2d.h evaluated on (a, y'): the closed form, the single-atom
 *             cases, the cut mfx_profile_cut() and the tie rule are the same, the outputs and their layout too.
 *             T = 2 sigma^2 means that measurement m has variance sigma^2 / W_m.  Sums run in mfx_soft2d.h's fixed
 *             order; no floating-point atomics.
 * Weights are [V x M] (w_stride = M) or one vector [M] shared by all voxels (w_stride = 0); any other stride is
 * MFX_ERR_ARG.
 *
 * Statuses.  Every entry point writes the direction record [V x 5] of mfx_fit2d.h.
 *   Fit: beside it the weight status, int32 [V]: 0 fitted, 1 a weight is negative or not finite, 2 no weight is
 *     positive.  A failing direction is tested first: its record is written, the row is NaN and the weight status
 *     is left 0.  Then the weights are tested; a flagged voxel gets a NaN row.
 *   Posterior status, int32 [V]: 5 a failing direction (tested first), 1 T is not finite or <= 0 or shift is not
 *     finite, 3 a weight is negative or not finite, 4 no weight is positive, 2 the shift is unusable (an exponent
 *     above 700, or Z is 0 or not finite), 0 ok - tested in this order.  A flagged voxel gets NaN rows and a NaN
 *     log_sum.
 *   Profile: a voxel with a failing direction or unusable weights gets NaN rows and partner -1.
 * The neighbours of a flagged voxel are untouched.
 *
 * Identities, by construction.  W = 1 multiplies by exactly 1.0: the fused kernels (K = 1, 2 without a CSF column)
 * reproduce mfx_fit2d_batch*, mfx_post2d* and mfx_profile2d* bit for bit; the materialise-and-solve classes of the
 * fit agree with theirs in every column but R2, which agrees to rounding (the weighted moments are summed by
 * another routine).  Indices, nu, MSE and R2 are invariant under W -> c W up to rounding (exactly for c a power of
 * four).  (c W, c T, c shift) gives the posterior of (W, T, shift) up to rounding.  A 0/1 mask gives the values of
 * the chain on the rotated dictionaries with the masked rows deleted - a masked row contributes exact zeros to
 * every sum - with MSE and R2 over the kept rows.
 *
 * Limits.  The K = 2 kernels keep per-atom statistics in the 160 KiB of LDS of a workgroup, whatever the number of
 * rows (s and y' are read from memory): mfx_w2d_max_atoms(h, what) gives the largest N they serve.  Beyond it the
 * posterior and the profile return MFX_ERR_UNSUPPORTED with the limit in the message and launch nothing; the fit
 * takes the materialise-and-solve path (slow, same results), as it does for a CSF column, three fascicles and under
 * mfx_w2d_debug_set_force_explicit.  The posterior and the profile serve K = 1 or 2 without a CSF column; any other
 * K is MFX_ERR_UNSUPPORTED.  The fit returns MFX_ERR_UNSUPPORTED for maxfasc > 3.  EAR columns are not served.
 */
#ifndef MFX_W2D_H
#define MFX_W2D_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* version of this header's entry points; bumped on a signature change or a new entry point */
int mfx_w2d_abi_version(void);

/* largest dictionary the K = 2 kernel serves; what = 0: fit, 1: posterior, 2: profile (0 for any other value) */
int mfx_w2d_max_atoms(void* h, int what);

/* One homogeneous class on device buffers: every voxel has K = maxfasc fascicles and no CSF column.
 * d_Y [V x M], d_W [V x M] or [M], d_peaks [V x 3 maxfasc] -> d_params [V x (1 + 2 maxfasc + 2)], d_status [V x 5],
 * d_wstatus [V]. */
int mfx_wfit2d_batch_dev(void* h, const double* d_Y, const double* d_W, int64_t w_stride, const double* d_peaks, int maxfasc,
                         int64_t V, double* d_params, int32_t* d_status, int32_t* d_wstatus, void* stream);

/* A mixed batch on host buffers: K [V] in 0..maxfasc, csf [V] flags (NULL: none; flagged voxels need csf_on and
 * sig_csf [M]), peaks [V x 3 maxfasc] -> params [V x (1 + 2 maxfasc + csf_on + 2)], status [V x 5], wstatus [V].  Bins
 * the voxels by class and waits for its own work. */
int mfx_wfit2d_batch(void* h, const double* Y, const double* W, int64_t w_stride, const int32_t* K, const uint8_t* csf,
                     const double* peaks, int maxfasc, int csf_on, const double* sig_csf, int64_t V, double* params,
                     int32_t* status, int32_t* wstatus);

/* d_Y [V x M], d_W, d_peaks [V x 3 K], d_T [V], d_shift [V] -> d_w [V x K x N], d_log_sum [V], d_status [V],
 * d_dir_status [V x 5] */
int mfx_wpost2d_dev(void* h, const double* d_Y, const double* d_W, int64_t w_stride, const double* d_peaks, int K,
                    const double* d_T, const double* d_shift, int64_t V, double* d_w, double* d_log_sum, int32_t* d_status,
                    int32_t* d_dir_status, void* stream);
int mfx_wpost2d(void* h, const double* Y, const double* W, int64_t w_stride, const double* peaks, int K, const double* T,
                const double* shift, int64_t V, double* w, double* log_sum, int32_t* status, int32_t* dir_status);

/* d_Y [V x M], d_W, d_peaks [V x 3 K] -> d_obj [V x K x N], d_partner [V x K x N] or NULL, d_dir_status [V x 5] */
int mfx_wprofile2d_dev(void* h, const double* d_Y, const double* d_W, int64_t w_stride, const double* d_peaks, int K, int64_t V,
                       double* d_obj, int32_t* d_partner, int32_t* d_dir_status, void* stream);
int mfx_wprofile2d(void* h, const double* Y, const double* W, int64_t w_stride, const double* peaks, int K, int64_t V,
                   double* obj, int32_t* partner, int32_t* dir_status);

/* diagnostics: 1 = every fit class of the calling thread's next calls takes the materialise-and-solve path */
void mfx_w2d_debug_set_force_explicit(int enabled);

#ifdef __cplusplus
}
#endif
#endif
