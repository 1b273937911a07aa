/*
 * mfx_soft2d.h -- C ABI of the soft fits and objective profiles of voxels measured with a 2-D
 * (AxCaliber-like) protocol: what mfx_post.h and mfx_profile.h give for multi-shell plans, on a handle of
 * mfx_rot2d.h (mfx_rot2d_create).  Kept apart from every other header, with its own version.  Conventions
 * are those of mfx_fit2d.h: plain pointers, row-major float64, 0 or an MFX_ERR_* code returned,
 * mfx_last_error() gives the message, no CPU path (without a usable device every entry point returns
 * MFX_ERR_NO_DEVICE).  The _dev variants take device pointers and a hipStream_t (as void*, NULL = default
 * stream) and only enqueue work; the others wait for their own work.
 *
 * Definitions.  A voxel has the signal y (M values) and K fascicle directions (peaks [V x 3 K]).  D_k
 * [M x N] is, bit for bit, the dictionary mfx_rot2d_rotate returns for direction k.  All voxels of one call
 * belong to ONE class, K in {1, 2}, without a CSF column.  F(i, j) (K = 2) and F(i) (K = 1) are EXACTLY
 * the values mfx_profile.h defines: the two-variable closed form of lsqnonneg_2var_opt from ||y||^2,
 * A11, A12, A22, Y1, Y2, the single-atom cases, and the cut mfx_profile_cut() on 1 - c^2 at or below which
 * a pair is scored as the better of its two single atoms.  F(i) = ||y||^2 - max(Y_i, 0)^2 / A_ii.
 *
 * Posterior (mfx_post2d*).  Inputs T[v] > 0 and shift[v] as in mfx_post.h; outputs by its formulas:
 *   K = 2   t(i, j) = exp(-(F(i, j) - shift) / T),  R0[i] = sum_j t(i, j),  R1[j] = sum_i t(i, j),
 *           Z = sum_i R0[i],  w[v, 0, i] = R0[i] / Z,  w[v, 1, j] = R1[j] / Z,  log_sum[v] = log Z - shift / T
 *   K = 1   t(i) = exp(-(F(i) - shift) / T),  w[v, 0, i] = t(i) / Z,  Z = sum_i t(i)
 * w [V x K x N] float64, log_sum [V] float64, status [V] int32:
 *   0   ok
 *   1   T is not finite or <= 0, or shift is not finite
 *   2   an exponent above 700 was met, or Z is 0 or not finite: the shift is unusable
 *   5   a fascicle direction of the voxel failed the rotation (tested before T and shift)
 * A voxel with a non-zero status gets NaN rows and a NaN log_sum; its neighbours are untouched.
 *
 * Profile (mfx_profile2d*).  obj [V x K x N] float64 and partner [V x K x N] int32 (may be NULL) as in
 * mfx_profile.h: obj[v, 0, i] = min_j F(i, j) with partner the arg-min j, obj[v, 1, j] = min_i F(i, j) with
 * partner the arg-min i; K = 1: obj[v, 0, i] = F(i), partner -1.  A tie goes to the lowest index: the
 * partner is the lowest index whose F, as computed, equals the minimum.  A voxel with a failing direction
 * gets NaN rows and partner -1.
 *
 * dir_status [V x 5] int32 is written by every entry point: the record of mfx_fit2d.h, {code, pair, value,
 * value2, fascicle} of the voxel's lowest failing fascicle direction, zeros for a voxel whose directions
 * are usable.
 *
 * All sums run in a fixed order with no floating-point atomics (K = 2, a workgroup per voxel walks the
 * pairs in blocks of 128 x 128 atoms; rows: the partner index ascending within a lane, over the 16 lanes of
 * the row, the block's two column halves in order, then the blocks in order; columns: over a lane's rows
 * ascending, the lane groups, the block's two row halves, then the blocks; Z: the row sums in index
 * order): the result of a voxel does not depend on the launch or on the other voxels of the call.
 *
 * Out of scope: CSF columns on 2-D protocols, three fascicles, the EAR compartment, measurement weights,
 * the all-pairs landscape.  K other than 1 or 2 returns MFX_ERR_UNSUPPORTED.
 *
 * Limits.  K = 2 keeps per-atom statistics and the running row and column results in the 160 KiB of LDS of
 * a workgroup, whatever the number of rows: mfx_soft2d_max_atoms(h, what) gives the largest N (what = 0:
 * posterior, 1: profile).  Beyond it the entry points return MFX_ERR_UNSUPPORTED with the limit in the
 * message and launch nothing.  K = 1 has no limit of its own.
 */
#ifndef MFX_SOFT2D_H
#define MFX_SOFT2D_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* version of this header's entry points; bumped on a signature change or a new entry point */
int mfx_soft2d_abi_version(void);

/* largest dictionary the K = 2 kernel serves; what = 0: posterior, 1: profile (0 for any other value) */
int mfx_soft2d_max_atoms(void* h, int what);

/* d_Y [V x M], d_peaks [V x 3 K], d_T [V], d_shift [V] -> d_w [V x K x N], d_log_sum [V], d_status [V],
 * d_dir_status [V x 5] */
int mfx_post2d_dev(void* h, const double* d_Y, const double* d_peaks, int K, const double* d_T, const double* d_shift,
                   int64_t V, double* d_w, double* d_log_sum, int32_t* d_status, int32_t* d_dir_status, void* stream);
int mfx_post2d(void* h, const double* Y, const double* peaks, int K, const double* T, const double* shift, int64_t V,
               double* w, double* log_sum, int32_t* status, int32_t* dir_status);

/* d_Y [V x M], d_peaks [V x 3 K] -> d_obj [V x K x N], d_partner [V x K x N] or NULL, d_dir_status [V x 5] */
int mfx_profile2d_dev(void* h, const double* d_Y, const double* d_peaks, int K, int64_t V, double* d_obj,
                      int32_t* d_partner, int32_t* d_dir_status, void* stream);
int mfx_profile2d(void* h, const double* Y, const double* peaks, int K, int64_t V, double* obj, int32_t* partner,
                  int32_t* dir_status);

#ifdef __cplusplus
}
#endif
#endif
