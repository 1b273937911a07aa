/*
 * mfx_wsoft.h -- C ABI of the objective profiles and the soft fits of a WEIGHTED fit: mfx_profile.h
 * and mfx_post.h with a non-negative weight per voxel and measurement (outlier masks, per-shell noise
 * levels), so that the landscape and the posterior are those of the problem mfx_wfit.h solved.
 *
 * Kept apart from the other headers, with its own version: mfx.h, mfx_profile.h, mfx_post.h and
 * mfx_wfit.h, their symbol lists and their versions stay as they are.  Conventions are theirs: plain
 * pointers, row-major float64, 0 or an MFX_ERR_* code returned, the library's last-error call gives
 * the message, no CPU path (without a usable device every entry point returns MFX_ERR_NO_DEVICE).
 * The _dev variants take device pointers and a hipStream_t (as void*, NULL = default stream) and
 * only enqueue work; the others wait for their own work.  With no weights a caller uses mfx_profile /
 * mfx_pair_objectives / mfx_post: nothing there changed.
 *
 * Semantics, per voxel, word for word those of mfx_wfit.h.  Weights are W [V x M] (w_stride = M) or
 * one [M] vector shared by all voxels (w_stride = 0):
 *   s_m     = sqrt(W[v,m]), correctly rounded in float64
 *   a[m,i]  = fl(s_m * D_k[m,i]), D_k[m,i] bit for bit the entry mfx_rotate and the unweighted kernels
 *             produce (a separate multiplication: the library is built without contraction)
 *   y'_m    = fl(s_m * y_m)
 *   x'_m    = fl(s_m * x_m) for the CSF column x = sig_csf
 * F_W(i, j) is EXACTLY the F of mfx_profile.h evaluated on (a, y', x'): the same closed form, the
 * same single-atom and CSF cases, the same cut mfx_profile_cut() on 1 - c^2 of the scaled atoms.
 *
 *   profile     obj[v, k, i] = min over the partners of F_W, partner the arg-min with the tie rules of
 *               mfx_profile.h; min_i obj[v, 0, i] is the weighted fit's objective MSE * sum_m W[v,m].
 *   landscape   out[v, i, j] = F_W(i, j)
 *   posterior   the formulas of mfx_post.h with F_W in place of F.  T = 2 sigma^2 now means that
 *               measurement m has noise variance sigma^2 / W[v,m].  Sums run in the fixed order of
 *               mfx_post.h; a voxel's result does not depend on the launch or on its neighbours.
 *
 * The weights of a voxel are checked in the kernel, uniformly over its workgroup, before anything is
 * computed (after the posterior's own check of T and shift, status 1):
 *   posterior status 3   a weight is negative or not finite
 *   posterior status 4   no weight is positive
 * Such a voxel gets NaN rows and a NaN log_sum; in the profile and the landscape NaN values and
 * partner -1.  Its neighbours are untouched.
 *
 * Identities that hold by construction.  W = 1 everywhere multiplies by exactly 1.0: the result
 * equals the unweighted entry point's bit for bit wherever both run the same kernel configuration
 * (the extra array in LDS lowers the dictionary sizes at which a configuration stops fitting by 16
 * to 48 atoms for M <= 200 and by up to 144 for M <= 560).  (c W, c T, c shift) for c > 0 gives the
 * weights of (W, T, shift) up to rounding, exactly so where sqrt(c) is a power of two.  A 0/1 mask
 * gives the values of the protocol with the masked rows deleted, up to the summation order.
 *
 * Out of scope, as for the unweighted entry points: three fascicles, the EAR compartment, voxels with
 * no fascicle, 2-D protocols; each call takes ONE class (K in {1, 2}, csf_on).
 *
 * Limits.  Those of mfx_profile.h and mfx_post.h: exact-G and G-bracketed rows, M <= 560, and for
 * K = 2 the dictionary that fits the 160 KiB of LDS with one more double per padded measurement:
 * mfx_wsoft_max_atoms().  Beyond either limit: MFX_ERR_UNSUPPORTED, the limit in the message, no
 * launch.  A fascicle direction that fails the reference's unit-norm test flags the plan's status
 * word (mfx_plan_status: MFX_ERR_DIR_NORM); the voxel is still computed.
 */
#ifndef MFX_WSOFT_H
#define MFX_WSOFT_H
#include <stdint.h>

#include "mfx.h"
#ifdef __cplusplus
extern "C" {
#endif

/* version of this header's entry points; bumped on a signature change or a new entry point */
int mfx_wsoft_abi_version(void);

/* largest dictionary the weighted K = 2 kernels serve for this plan (0 for a protocol out of range);
 * what: 0 the posterior, 1 the profile, 2 the landscape */
int mfx_wsoft_max_atoms(const mfx_plan* p, int csf_on, int what);

/* mfx_post_dev / mfx_post with d_W [V x M] (w_stride = M) or [M] (w_stride = 0) */
int mfx_wpost_dev(const mfx_plan* p, const double* d_Y, const double* d_W, int64_t w_stride, const double* d_peaks, int K,
                  int csf_on, const double* d_sig_csf, const double* d_T, const double* d_shift, int64_t V, double* d_w,
                  double* d_log_sum, int32_t* d_status, void* stream);
int mfx_wpost(const mfx_plan* p, const double* Y, const double* W, int64_t w_stride, const double* peaks, int K, int csf_on,
              const double* sig_csf, const double* T, const double* shift, int64_t V, double* w, double* log_sum,
              int32_t* status);

/* mfx_profile_dev / mfx_profile with the weights */
int mfx_wprofile_dev(const mfx_plan* p, const double* d_Y, const double* d_W, int64_t w_stride, const double* d_peaks, int K,
                     int csf_on, const double* d_sig_csf, int64_t V, double* d_obj, int32_t* d_partner, void* stream);
int mfx_wprofile(const mfx_plan* p, const double* Y, const double* W, int64_t w_stride, const double* peaks, int K,
                 int csf_on, const double* sig_csf, int64_t V, double* obj, int32_t* partner);

/* mfx_pair_objectives_dev / mfx_pair_objectives (K = 2) with the weights */
int mfx_wpair_objectives_dev(const mfx_plan* p, const double* d_Y, const double* d_W, int64_t w_stride,
                             const double* d_peaks, int csf_on, const double* d_sig_csf, int64_t V, double* d_out,
                             void* stream);
int mfx_wpair_objectives(const mfx_plan* p, const double* Y, const double* W, int64_t w_stride, const double* peaks,
                         int csf_on, const double* sig_csf, int64_t V, double* out);

#ifdef __cplusplus
}
#endif
#endif
