/*
 * mfx_boot.h -- C ABI of the bootstrap: the residuals of a voxel's own fit are resampled into B replicate signals, the
 * replicates are fitted by the plain fit of mfx.h (mfx_fit_batch_dev), and the B parameter rows of every voxel are
 * reduced to statistics, all on the device.  It serves every voxel class of the unweighted fit: 0..3 fascicles, with or
 * without the CSF and EAR compartments.  Kept apart from the other headers, with its own version.  Conventions are
 * those of mfx.h: plain pointers, row-major float64, 0 or an MFX_ERR_* code returned, mfx_last_error() gives the
 * message, no CPU path (without a usable device every entry point returns MFX_ERR_NO_DEVICE).
 *
 * The resampling rule.  Per voxel v of the call, measurement m = 0..M-1 and replicate b = 0..B-1, from the data row
 * y [M], the prediction row p [M] of the voxel's own fit (what mfx_predict_dev returns on its parameter row) and that
 * parameter row.  Every step is ONE correctly rounded float64 operation, in this order (fl = rounding to nearest
 * even; the build has no contraction):
 *   residual  r_m = fl(y_m - p_m)
 *   scale     inflate = 0: a = 1.  inflate = 1: a = sqrt( fl( M / (M - n_act) ) ), the division, then the square
 *             root; n_act = the number of strictly positive weights of the parameter row (nu_k, nu_csf, nu_ear)
 *   draw      Philox4x32-10 (Salmon et al., SC'11; the generator of mfx_predict.h), key = the 64-bit seed (low word,
 *             high word), counter = (low word of idx, high word of idx, b, MFX_BOOT_STREAM), with
 *             idx = offset + i_v M + m in 64-bit unsigned arithmetic, i_v the voxel's BATCH index: vox[v], or v
 *             without vox.  u = output word 0.  A replicate therefore depends on (seed, offset, i_v, m, b) and the
 *             voxel's own rows only - not on V, on how a batch is cut into chunks or classes, nor on a subset.
 *   kind MFX_BOOT_WILD (0):      s = +1 if bit 0 of u is 0, else -1;  y*_m = fl( p_m + s fl(a r_m) )
 *   kind MFX_BOOT_RESIDUAL (1):  groups [M] int32 names the group of every row (any values); the group of m has n_g
 *             rows, j = the mulhi32(u, n_g)-th of them in row order (mulhi32(u, n) = floor(u n / 2^32) < n);
 *             y*_m = fl( p_m + fl(a r_j) ).  The residuals are NOT centred: a group's residuals are drawn as they are.
 * Output rows are ordered (v, b): Y* [V x B x M]; the voxel's directions are copied to every replicate row,
 * peaks* [V B x 3 maxfasc].
 * status of a voxel, int32, the first that applies:
 *   2  the original row is not usable: some y_m or p_m is not finite (mfx_predict_dev writes a NaN row for a weight
 *      that is negative or not finite and for an atom index outside its dictionary)
 *   1  M <= n_act: no degree of freedom (looked at with inflate = 0 too)
 *   0  fine
 * In a non-zero status every y*_m of the voxel is NaN.  (Inside mfx_boot_fit_dev such rows are fitted as zero rows and
 * their replicate parameters are NaN afterwards: the fit kernels never see a NaN of this header's making.)
 *
 * The value table.  From replicate parameter rows [V x B x np] in the layout of mfx_fit_batch_dev for (maxfasc,
 * csf_on, ear_on), np = 1 + 2 maxfasc + csf_on + 2 ear_on + 2, and nprop property tables props [nprop x N]:
 *   column 0 M0;  1 + k: nu_k;  then nu_csf (csf_on), nu_ear (ear_on), MSE;  then for every fascicle k and property t,
 *   column C0 + k nprop + t = props[t][atom_k], C0 = 2 + maxfasc + csf_on + ear_on;  C = C0 + maxfasc nprop.
 * A property column of fascicle k is valid in a replicate only where nu_k > 0 (an atom chosen with zero weight is the
 * solver's first hit and says nothing) and the atom is an integer in [0, N); every other column is valid.  For a voxel
 * whose status is not 0 nothing is valid, and its replicate rows are overwritten with NaN.
 * agree [V x maxfasc] int32: the replicates with nu_k > 0 and the atom of the original fit's row.
 *
 * The statistics.  Per voxel and column, over the n valid replicates x_0 .. x_(n-1) in the order of b; stats
 * [V x C x (5 + Q)]:
 *   0  n
 *   1  mean  = fl(S / n), S the serial sum ((x_0 + x_1) + x_2) + ...
 *   2  std   = sqrt( fl( T / (n - 1) ) ), T the serial sum of fl(d d), d = fl(x_i - mean);  NaN for n < 2
 *   3  min   4  max
 *   5 + i  the quantile q_i by linear interpolation: with the x ordered by (value, b) into x_(0) <= ..,
 *          pos = fl(q_i (n - 1)), lo = floor(pos), hi = min(lo + 1, n - 1), value = fl( x_(lo) + fl( fl(x_(hi) - x_(lo)) (pos - lo) ) )
 * n = 0 gives NaN everywhere but in n.  B <= MFX_BOOT_MAX_B (the B values of a column are held in LDS) and
 * Q <= MFX_BOOT_MAX_Q, else MFX_ERR_UNSUPPORTED before any launch.  Protocols of more than 8192 measurements return
 * MFX_ERR_UNSUPPORTED.
 * Not served: weighted and robust fits; mfx_wboot.h bootstraps them with the fit's weights held fixed.  (2-D
 * protocols: mfx_boot2d.h, by this rule, value table and statistics.)
 */
#ifndef MFX_BOOT_H
#define MFX_BOOT_H
#include <stdint.h>

#include "mfx.h"
#ifdef __cplusplus
extern "C" {
#endif

#define MFX_BOOT_WILD 0
#define MFX_BOOT_RESIDUAL 1
#define MFX_BOOT_STREAM 0x424f4f54u /* fourth counter word; mfx_predict.h's noise uses 0x534f534d */
#define MFX_BOOT_MAX_B 4096
#define MFX_BOOT_MAX_Q 32
#define MFX_BOOT_NSTAT 5 /* n, mean, std, min, max; the quantiles follow */

/* version of this header's entry points; bumped on a signature change or a new entry point */
int mfx_boot_abi_version(void);

/* The resampling rule alone on device buffers; needs no plan.  d_Y, d_P [V x M]; d_params [V x np] (np for maxfasc,
 * csf_on, ear_on: only the weights are read); d_peaks [V x 3 maxfasc] or NULL (then d_peaks_out is not written);
 * d_groups [M] int32 (kind 1; ignored for kind 0); d_vox [V] int64 batch indices or NULL (identity) ->
 * d_Ystar [V x B x M], d_peaks_out [V B x 3 maxfasc], d_status [V].  Only enqueues on `stream` (hipStream_t as void*,
 * NULL = default stream). */
int mfx_boot_resample_dev(int M, const double* d_Y, const double* d_P, const double* d_params, int maxfasc, int csf_on,
                          int ear_on, const double* d_peaks, const int32_t* d_groups, const int64_t* d_vox, int64_t V, int B,
                          int kind, int inflate, uint64_t seed, uint64_t offset, double* d_Ystar, double* d_peaks_out,
                          int32_t* d_status, void* stream);

/* The value table: d_params [V x B x np] replicate rows (overwritten with NaN where d_status is given and not 0),
 * d_params0 [V x np] the original rows, d_props [nprop x N] (NULL with nprop = 0), d_status [V] or NULL ->
 * d_X [V x B x C], d_valid [V x B x C] uint8, d_agree [V x maxfasc] int32 (NULL: not wanted).  Only enqueues. */
int mfx_boot_gather_dev(double* d_params, const double* d_params0, int maxfasc, int csf_on, int ear_on, const double* d_props,
                        int nprop, int N, const int32_t* d_status, int64_t V, int B, double* d_X, uint8_t* d_valid,
                        int32_t* d_agree, void* stream);

/* The statistics: d_X, d_valid [V x B x C], d_q [Q] in [0, 1] (NULL with Q = 0) -> d_stats [V x C x (5 + Q)].  Only enqueues. */
int mfx_boot_reduce_dev(const double* d_X, const uint8_t* d_valid, int64_t V, int B, int C, const double* d_q, int Q,
                        double* d_stats, void* stream);

/* One homogeneous class on device buffers, as mfx_fit_batch_dev takes it: every voxel has maxfasc fascicles, the CSF
 * column iff csf_on, the EAR columns iff ear_on.  d_params0 [V x np] the voxels' own fit (NULL: mfx_fit_batch_dev runs
 * first), d_pred0 [V x M] its prediction (NULL: mfx_predict_dev runs).  Then, in chunks of voxels sized so that the
 * replicate signals of a chunk, Vc B M 8 bytes, stay within max_bytes (<= 0: 256 MiB; one voxel at the least):
 * resample, mfx_fit_batch_dev on the Vc B replicate rows, gather, reduce.  -> d_stats [V x C x (5 + Q)], d_agree
 * [V x maxfasc] (NULL with maxfasc = 0), d_status [V], d_keep [V x B x np] the replicate rows (NULL: not kept).
 * Scratch comes from the calling thread's arena of the stream; only enqueues on `stream`.  A direction that is not a
 * unit vector flags the plan's status word as in the plain fit (mfx_plan_status). */
int mfx_boot_fit_dev(const mfx_plan* p, const double* d_Y, const double* d_peaks, int maxfasc, int csf_on, int ear_on,
                     const double* d_sig_csf, const double* d_sig_ear, int E, const double* d_params0, const double* d_pred0,
                     const int32_t* d_groups, const int64_t* d_vox, int64_t V, int B, int kind, int inflate, uint64_t seed,
                     uint64_t offset, const double* d_props, int nprop, const double* d_q, int Q, int64_t max_bytes,
                     double* d_stats, int32_t* d_agree, int32_t* d_status, double* d_keep, void* stream);

/* A mixed batch on host buffers, as mfx_fit_batch takes it: K [V] in 0..maxfasc, csf, ear [V] flags (NULL: none),
 * peaks [V x 3 maxfasc], sig_csf [M], sig_ear [M x E]; params0 [V x np] the voxels' own fit in the batch's layout
 * (NULL: fitted here); groups [M] (kind 1); vox [V] batch indices (NULL: identity) - the voxel's batch index, not its
 * place in its class, feeds the counter; props [nprop x N]; q [Q].  The voxels are binned by class (class_batch.h) and
 * every class runs as mfx_boot_fit_dev does, in its own layout; the results come back in the batch's layout
 * (maxfasc, csf_on, ear_on): stats [V x C x (5 + Q)], agree [V x maxfasc], status [V], keep [V x B x np] (NULL: not
 * kept).  A compartment a voxel does not have has weight 0 in every replicate (n = B, mean 0), the properties of a
 * fascicle it does not have are never valid, and its agree is 0.  Waits for its own work. */
int mfx_boot_fit(const mfx_plan* p, const double* Y, const int32_t* K, const uint8_t* csf, const uint8_t* ear,
                 const double* peaks, int maxfasc, int csf_on, int ear_on, const double* sig_csf, const double* sig_ear, int E,
                 const double* params0, const int32_t* groups, const int64_t* vox, int64_t V, int B, int kind, int inflate,
                 uint64_t seed, uint64_t offset, const double* props, int nprop, const double* q, int Q, int64_t max_bytes,
                 double* stats, int32_t* agree, int32_t* status, double* keep);

#ifdef __cplusplus
}
#endif
#endif
