/*
 * mfx_wboot.h -- C ABI of the bootstrap CONDITIONAL ON A FIT'S MEASUREMENT WEIGHTS: the bootstrap of mfx_boot.h around
 * the weighted fit of mfx_wfit.h.  The weights W of a voxel - those a weighted fit was given, or the final weights of a
 * robust fit - are held fixed: no replicate re-runs a rejection, so after a robust fit the result is conditional on the
 * rows that were rejected.  Kept apart from the other headers, with its own version.  Conventions are those of mfx.h:
 * plain pointers, row-major float64, 0 or an MFX_ERR_* code returned, mfx_last_error() gives the message, no CPU path
 * (without a usable device every entry point returns MFX_ERR_NO_DEVICE).
 *
 * The resampling rule.  Per voxel v of the call, from the data row y [M], the prediction row p [M] of the voxel's own
 * weighted fit (what mfx_predict_dev returns on its parameter row), the weights W [M] - the voxel's row (w_stride = M)
 * or one vector shared by all voxels (w_stride = 0) - and that parameter row in mfx_wfit.h's layout (no EAR columns).
 * status of a voxel, int32, the first that applies:
 *   3  a weight is negative or not finite
 *   4  no positive weight
 *   2  some y_m or p_m is not finite
 *   1  M+ <= n_act: M+ = the number of rows with W_m > 0, n_act = the number of strictly positive weights of the
 *      parameter row (nu_k, nu_csf), as in mfx_boot.h (looked at with inflate = 0 too)
 *   0  fine
 * In a non-zero status every y*_m of the voxel is NaN.  Otherwise every step is ONE correctly rounded float64 operation,
 * in this order (fl = rounding to nearest even; the build has no contraction):
 *   residual  r_m = fl(y_m - p_m)
 *   scale     inflate = 0: a = 1.  inflate = 1: a = sqrt( fl( M+ / (M+ - n_act) ) ), the division, then the square root
 *   draw      that of mfx_boot.h, word for word: Philox4x32-10, key = the 64-bit seed (low word, high word), counter =
 *             (low word of idx, high word of idx, b, MFX_BOOT_STREAM), idx = offset + i_v M + m in 64-bit unsigned
 *             arithmetic, i_v the voxel's batch index (vox[v], or v without vox) and m the row OF THE FULL PROTOCOL;
 *             u = output word 0
 *   W_m = 0   y*_m = y_m: the row has no say in the fit and is left as measured
 *   kind MFX_BOOT_WILD, W_m > 0:      s = +1 if bit 0 of u is 0, else -1;  y*_m = fl( p_m + s fl(a r_m) )
 *   kind MFX_BOOT_RESIDUAL, W_m > 0:  the draw is made in standardised units: s_m = sqrt(W_m), e_m = fl(s_m r_m).  The
 *             group of m counts only its rows with W > 0, n_g+ of them; j = the mulhi32(u, n_g+)-th of those rows in row
 *             order;  y*_m = fl( p_m + fl( fl(a e_j) / s_m ) )
 * With W = 1 everywhere (per voxel or shared) both kinds reproduce mfx_boot_resample_dev bit for bit (s = 1, e = r, a
 * division by 1).  A 0/1 mask is NOT claimed to equal the rule of mfx_boot.h on the protocol with the masked rows
 * deleted: idx counts the rows of the full protocol, so the kept rows draw other words there.
 * Output rows are ordered (v, b): Y* [V x B x M]; the voxel's directions are copied to every replicate row.
 *
 * The value table and the statistics are those of mfx_boot.h with ear_on = 0, through mfx_boot_gather_dev and
 * mfx_boot_reduce_dev unchanged; the MSE column holds the weighted MSE of mfx_wfit.h.
 *
 * The replicate fit.  mfx_wboot_fit_rows_dev fits B signals per voxel on the voxel's weights and directions: row (v, b)
 * equals, bit for bit, the row mfx_wfit_batch_dev returns for (Y*[v, b], W[v], peaks[v]).  Two fascicles without a CSF
 * column, for dictionaries up to mfx_wfit_max_atoms(plan, 2) atoms, take the SHARED path: the cross-Gram
 * D_0^T diag(W) D_1 of a voxel is formed once, by the chunk loop of the weighted two-fascicle kernel, and every
 * replicate scans the stored accumulator tiles instead of forming them again; everything else a replicate does is that
 * kernel's arithmetic, unchanged.  Every other class (one fascicle, a CSF column, three fascicles, larger dictionaries),
 * and everything under mfx_wboot_debug_set_force_plain(1), takes the PLAIN path: weight rows and directions are copied
 * to the replicate rows of a voxel chunk (a shared [M] vector stays shared) and the class launcher of mfx_wfit.h runs on
 * them untouched - slow, same results.
 * A voxel in a non-zero status is fitted as a zero row and its replicate rows are NaN afterwards: no fit kernel sees a
 * NaN of this header's making.  B <= MFX_BOOT_MAX_B, Q <= MFX_BOOT_MAX_Q and maxfasc <= 3, else MFX_ERR_UNSUPPORTED
 * before any launch; so for protocols of more than 8192 measurements.
 * 2-D protocols with weights are served by mfx_wboot2d.h.  Not served: re-running a robust rejection per replicate, EAR
 * columns.
 */
#ifndef MFX_WBOOT_H
#define MFX_WBOOT_H
#include <stdint.h>

#include "mfx_boot.h"
#ifdef __cplusplus
extern "C" {
#endif

/* version of this header's entry points; bumped on a signature change or a new entry point */
int mfx_wboot_abi_version(void);

/* replicates a workgroup of the shared path finishes on one pass over a voxel's Gram (the replicate counts around it
 * are the kernel's seams) */
int mfx_wboot_rep_tile(void);

/* diagnostics: 1 = every class of the calling thread's next calls takes the plain path */
void mfx_wboot_debug_set_force_plain(int enabled);

/* The resampling rule alone on device buffers; needs no plan.  d_Y, d_P [V x M]; d_W [V x M] (w_stride = M) or [M]
 * (w_stride = 0); d_params [V x (1 + 2 maxfasc + csf_on + 2)] (only the weights are read); d_peaks [V x 3 maxfasc] or
 * NULL (then d_peaks_out is not written); d_groups [M] int32 (kind 1; ignored for kind 0); d_vox [V] int64 batch
 * indices or NULL (identity) -> d_Ystar [V x B x M], d_peaks_out [V B x 3 maxfasc], d_status [V].  Only enqueues on
 * `stream` (hipStream_t as void*, NULL = default stream). */
int mfx_wboot_resample_dev(int M, const double* d_Y, const double* d_P, const double* d_W, int64_t w_stride,
                           const double* d_params, int maxfasc, int csf_on, const double* d_peaks, const int32_t* d_groups,
                           const int64_t* d_vox, int64_t V, int B, int kind, int inflate, uint64_t seed, uint64_t offset,
                           double* d_Ystar, double* d_peaks_out, int32_t* d_status, void* stream);

/* The replicate weighted fit of one class on device buffers: every voxel has K = maxfasc fascicles and no CSF column.
 * d_Ystar [V x B x M], d_W as above, d_peaks [V x 3 maxfasc] -> d_params [V x B x (1 + 2 maxfasc + 2)], d_status [V]
 * (mfx_wfit.h's status of the voxel's weights; such a voxel has NaN rows).  Scratch of the shared path, the accumulator
 * tiles of a voxel's Gram (8 NB^2 bytes, NB = the padded dictionary size rounded up to 128), comes from the stream's
 * arena in chunks of voxels of at most 256 MiB.  Only enqueues on `stream`. */
int mfx_wboot_fit_rows_dev(const void* plan, const double* d_Ystar, const double* d_W, int64_t w_stride, const double* d_peaks,
                           int maxfasc, int64_t V, int B, double* d_params, int32_t* d_status, void* stream);

/* The bootstrap of one homogeneous class on device buffers: every voxel has maxfasc fascicles and the CSF column iff
 * csf_on.  Arguments as mfx_boot_fit_dev takes them, without EAR, plus the weights: d_params0 [V x np] the voxels' own
 * weighted fit (NULL: the weighted fit runs first), d_pred0 [V x M] its prediction (NULL: mfx_predict_dev runs).  Per
 * chunk of voxels - sized so that the replicate signals and the replicate fit's scratch of a chunk stay within
 * max_bytes (<= 0: 256 MiB; one voxel at the least) - resample, replicate fit, mfx_boot_gather_dev,
 * mfx_boot_reduce_dev.  -> d_stats [V x C x (5 + Q)], d_agree [V x maxfasc] (NULL with maxfasc = 0), d_status [V],
 * d_keep [V x B x np] the replicate rows (NULL: not kept).  Only enqueues on `stream`. */
int mfx_wboot_fit_dev(const void* plan, const double* d_Y, const double* d_W, int64_t w_stride, const double* d_peaks, int maxfasc,
                      int csf_on, const double* d_sig_csf, const double* d_params0, const double* d_pred0, const int32_t* d_groups,
                      const int64_t* d_vox, int64_t V, int B, int kind, int inflate, uint64_t seed, uint64_t offset,
                      const double* d_props, int nprop, const double* d_q, int Q, int64_t max_bytes, double* d_stats,
                      int32_t* d_agree, int32_t* d_status, double* d_keep, void* stream);

/* A mixed batch on host buffers, as mfx_wfit_batch takes it: K [V] in 0..maxfasc, csf [V] flags (NULL: none), W [V x M]
 * or [M], peaks [V x 3 maxfasc], sig_csf [M]; params0, groups, vox, props, q as in mfx_boot_fit.  The voxels are binned
 * by class (class_batch.h) and every class runs as mfx_wboot_fit_dev does, in its own layout; the results come back in
 * the batch's layout (maxfasc, csf_on) by the rules of mfx_boot_fit: stats [V x C x (5 + Q)], agree [V x maxfasc],
 * status [V], keep [V x B x np] (NULL: not kept).  Waits for its own work. */
int mfx_wboot_fit(const void* plan, const double* Y, const double* W, int64_t w_stride, const int32_t* K, const uint8_t* csf,
                  const double* peaks, int maxfasc, int csf_on, const double* sig_csf, const double* params0,
                  const int32_t* groups, const int64_t* vox, int64_t V, int B, int kind, int inflate, uint64_t seed,
                  uint64_t offset, const double* props, int nprop, const double* q, int Q, int64_t max_bytes, double* stats,
                  int32_t* agree, int32_t* status, double* keep);

#ifdef __cplusplus
}
#endif
#endif
