/*
 * mfx_post.h -- C ABI of the soft fits: per-atom posterior weights of each fascicle given the noise
 * level, and the log-sum that compares explanations of a voxel.  The fit reports the arg-min over
 * all atom pairs and mfx_profile.h the minimum per atom; these entry points report, per atom of each
 * fascicle, the sum over every partner atom of exp(-F / T), normalised per voxel.
 *
 * Kept apart from mfx.h so that mfx.h's symbol list and version stay as they are; this header has
 * its own version.  Conventions are those of mfx.h and mfx_profile.h: plain pointers, row-major
 * float64, 0 or an MFX_ERR_* code returned, the library's last-error call gives the message, no CPU
 * path (without a usable device every entry point returns MFX_ERR_NO_DEVICE).  The _dev variant
 * takes device pointers and a hipStream_t (as void*, NULL = default stream) and only enqueues work;
 * the other waits for its own work.
 *
 * Definitions.  A voxel has the signal y (M values) and K fascicle directions (peaks [V x 3 K]);
 * D_k [M x N] is the dictionary rotated onto direction k.  All voxels of one call belong to ONE
 * class (K in {1, 2}, csf_on).  F(i, j) is EXACTLY the value mfx_profile.h defines for the pair of
 * atom i of D_0 and atom j of D_1: the two-variable closed form of lsqnonneg_2var_opt, the
 * single-atom cases, with csf_on the form with the CSF column x projected out and the sign of w_x
 * deciding, and the cut mfx_profile_cut() on 1 - c^2 below which a pair is scored as its better
 * single atom.  For K = 1, F(i) = ||y||^2 - max(Y_i, 0)^2 / A_ii (and its CSF form).
 *
 * Two further inputs per voxel v, float64 [V] each:
 *   T[v] > 0    the temperature; T = 2 sigma^2 for Gaussian noise of standard deviation sigma
 *   shift[v]    any value near min F; it only keeps the exponentials in range and cancels in the
 *               weights
 *
 *   K = 2   t(i, j)    = exp(-(F(i, j) - shift) / T)
 *           R0[i]      = sum_j t(i, j),   R1[j] = sum_i t(i, j),   Z = sum_i R0[i]
 *           w[v, 0, i] = R0[i] / Z,       w[v, 1, j] = R1[j] / Z
 *           log_sum[v] = log Z - shift / T          (= log sum_ij exp(-F / T))
 *   K = 1   t(i) = exp(-(F(i) - shift) / T),   w[v, 0, i] = t(i) / Z,   Z = sum_i t(i)
 *
 * Outputs: w [V x K x N] float64, log_sum [V] float64, status [V] int32:
 *   0   ok
 *   1   T is not finite or <= 0, or shift is not finite
 *   2   an exponent above 700 was met, or Z is 0 or not finite: the shift is unusable
 * A voxel with a non-zero status gets NaN rows and a NaN log_sum; its neighbours are untouched.
 * Padded atoms contribute t = 0.
 *
 * All sums run in a fixed order (rows: the partner index ascending within a lane, then over the 16
 * lanes of a row; columns: over a lane's rows, the lane groups, then the waves in wave order; Z:
 * the row sums in index order) with no global atomics: the result of a voxel does not depend on the
 * launch or on the other voxels of the call.
 *
 * Out of scope, as for the profile: three fascicles, the EAR compartment, voxels with no fascicle,
 * 2-D protocols, measurement weights.  Callers that bin mixed volumes write NaN rows for the other
 * classes and count them (engine.posterior does).
 *
 * Limits.  The protocols of the FP64 fit kernel: exact-G and G-bracketed rows, M <= 560.  K = 2
 * keeps per-atom statistics and the running column sums in the 160 KiB of LDS of a workgroup:
 * mfx_post_max_atoms() gives the largest N for a plan and mode; it is never smaller than
 * mfx_profile_max_atoms() of the same plan (one double per atom and slab slot where the profile
 * keeps two and an index).  Beyond either limit: MFX_ERR_UNSUPPORTED, the limit in the message, no
 * launch.  A fascicle direction that fails the reference's unit-norm test flags the plan's status
 * word like the fit does (mfx_plan_status: MFX_ERR_DIR_NORM); the voxel is still computed.
 */
#ifndef MFX_POST_H
#define MFX_POST_H
#include <stdint.h>

#include "mfx.h"
#ifdef __cplusplus
extern "C" {
#endif

/* version of this header's entry points; bumped on a signature change or a new entry point */
int mfx_post_abi_version(void);

/* largest dictionary the K = 2 kernel serves for this plan (0 for a protocol out of range) */
int mfx_post_max_atoms(const mfx_plan* p, int csf_on);

/*
 * Debug: which K = 2 kernel the calling thread's last launch through this header or mfx_wpost* of
 * mfx_wsoft.h was.  form[8] = (KSTEPS, NW, TILES, NBUF, BR, CSF, LAND, WGT) as
 * mfx_profile_debug_last_config of mfx_profile.h gives it, LAND always 0.  Returns 1, or 0 with
 * form untouched before the thread's first such launch.  K = 1 calls and calls refused before the
 * launch leave the record as it is.  Since 2.
 */
int mfx_post_debug_last_config(int* form);

/*
 * d_Y [V x M], d_peaks [V x 3 K], d_sig_csf [M] (csf_on), d_T [V], d_shift [V]; d_w [V x K x N]
 * float64, d_log_sum [V] float64, d_status [V] int32.  One workgroup per voxel; nothing of size
 * N x N is stored.
 */
int mfx_post_dev(const mfx_plan* p, const double* d_Y, const double* d_peaks, int K, int csf_on,
                 const double* d_sig_csf, const double* d_T, const double* d_shift, int64_t V, double* d_w,
                 double* d_log_sum, int32_t* d_status, void* stream);
int mfx_post(const mfx_plan* p, const double* Y, const double* peaks, int K, int csf_on, const double* sig_csf,
             const double* T, const double* shift, int64_t V, double* w, double* log_sum, int32_t* status);

#ifdef __cplusplus
}
#endif
#endif
