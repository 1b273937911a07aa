/*
 * mfx_wboot2d.h -- C ABI of the bootstrap CONDITIONAL ON A FIT'S MEASUREMENT WEIGHTS for voxels of a 2-D (AxCaliber-like)
 * protocol, on a handle of mfx_rot2d.h (mfx_rot2d_create): the bootstrap of mfx_boot2d.h around the weighted fit of
 * mfx_w2d.h, with the resampling rule of mfx_wboot.h (mfx_wboot_resample_dev, word for word) and the value table and
 * statistics of mfx_boot.h with ear_on = 0.  The weights W of a voxel - those a weighted fit was given, or the final
 * weights of a robust fit - are held fixed: no replicate re-runs a rejection, so after a robust fit the result is
 * conditional on the rows that were rejected.  Kept apart from the other headers, with its own version.  Conventions are
 * those of mfx.h: plain pointers, row-major float64, 0 or an MFX_ERR_* code returned, mfx_last_error() gives the message,
 * no CPU path (without a usable device every entry point returns MFX_ERR_NO_DEVICE).
 *
 * The primitive underneath is the WEIGHTED REPLICATE FIT: B signals per voxel on the voxel's weights W [M] - its row of
 * d_W [V x M] (w_stride = M) or one vector shared by all voxels (w_stride = 0) - and directions.  Row (v, b) equals, bit
 * for bit, the row mfx_wfit2d_batch_dev returns for (Y*[v, b], W[v], peaks[v]).  One and two fascicles without a CSF
 * column, for dictionaries of up to mfx_wboot2d_max_atoms(h) atoms, take the SHARED path: s = sqrt(W), sum W, the
 * directions' records, the norms |fl(s_m d)|^2 and the weighted cross-Gram are formed ONCE per voxel, and every row is
 * finished on them by the arithmetic of the weighted kernels of mfx_w2d.h.  Every other class (a CSF column, three
 * fascicles, larger dictionaries), and everything under mfx_wboot2d_debug_set_force_plain(1), takes the PLAIN path:
 * weight rows and directions are copied to the replicate rows of a voxel chunk (a shared [M] vector stays shared) and
 * the class launcher of mfx_w2d.h runs on them untouched - slow, same results.
 *
 * status of a voxel, int32, the first that applies:
 *   2  a direction fails (mfx_rot2d.h's status codes); its record is kept in dir_status [V x 5] (the record of
 *      mfx_fit2d.h).  Tested first, as in mfx_w2d.h
 *   otherwise the status of mfx_wboot.h: 3 a weight is negative or not finite, 4 no positive weight, 2 some y_m or p_m is
 *   not finite, 1 M+ <= n_act, 0 fine
 * A voxel in a non-zero status has NaN replicate rows and NaN statistics; its replicate signals are zero rows while they
 * are fitted, so no fit kernel sees a NaN.  Its neighbours are untouched.
 * No floating-point atomics and fixed summation orders: a replicate's row does not depend on B, V, the chunking or the
 * voxel's position.
 * B <= MFX_BOOT_MAX_B, Q <= MFX_BOOT_MAX_Q and maxfasc <= 3 in the bootstrap entry points, else MFX_ERR_UNSUPPORTED before
 * any launch.
 * Not served: re-running a robust rejection per replicate, EAR columns.
 */
#ifndef MFX_WBOOT2D_H
#define MFX_WBOOT2D_H
#include <stdint.h>

#include "mfx_boot.h"
#ifdef __cplusplus
extern "C" {
#endif

/* version of this header's entry points; bumped on a signature change or a new entry point */
int mfx_wboot2d_abi_version(void);

/* replicates per register tile of the column statistics kernel (the replicate counts around it are the kernel's seams) */
int mfx_wboot2d_rep_tile(void);

/* the largest dictionary whose two-fascicle voxels take the shared path (0 for a NULL handle) */
int mfx_wboot2d_max_atoms(void* h);

/* diagnostics: 1 = every class of the calling thread's next calls takes the plain path */
void mfx_wboot2d_debug_set_force_plain(int enabled);

/* The weighted replicate fit of one class on device buffers: every voxel has K = maxfasc fascicles and no CSF column.
 * d_Ystar [V x B x M], d_W [V x M] (w_stride = M) or [M] (w_stride = 0), d_peaks [V x 3 maxfasc] -> d_params
 * [V x B x (1 + 2 maxfasc + 2)], d_status [V x 5] (the directions' record per voxel, not per row), d_wstatus [V]
 * (mfx_w2d.h's status of the voxel's weights: 0 usable, 1 a negative or non-finite weight, 2 no positive weight; a
 * voxel flagged in either has NaN rows).  Scratch (s and sum W of a voxel, y'* = s y* [B x M], the Gram [NP x NP], NP = N
 * rounded up to 16, and D'^T y'* [B x K x NP]) comes from the stream's arena, in chunks of voxels of at most 256 MiB.
 * Only enqueues on `stream` (hipStream_t as void*, NULL = default stream). */
int mfx_wboot2d_fit_rows_dev(void* h, const double* d_Ystar, const double* d_W, int64_t w_stride, const double* d_peaks,
                             int maxfasc, int64_t V, int B, double* d_params, int32_t* d_status, int32_t* d_wstatus,
                             void* stream);

/* The bootstrap of one homogeneous class on device buffers: every voxel has maxfasc fascicles and the CSF column iff
 * csf_on.  Arguments as mfx_boot2d_fit_dev takes them, plus the weights: d_params0 [V x np] the voxels' own weighted fit
 * (NULL: the fit of mfx_w2d.h runs first), d_pred0 [V x M] its prediction (NULL: mfx_predict2d's kernel runs).  Per chunk
 * of voxels - sized so that the replicate signals and the replicate fit's scratch of a chunk stay within max_bytes
 * (<= 0: 256 MiB; one voxel at the least) - the directions are prepared once and serve the own fit, the prediction and
 * the replicate fit; then mfx_wboot_resample_dev, the replicate fit, mfx_boot_gather_dev, mfx_boot_reduce_dev.
 * -> d_stats [V x C x (5 + Q)], d_agree [V x maxfasc] (NULL with maxfasc = 0), d_status [V], d_dir_status [V x 5], d_keep
 * [V x B x np] the replicate rows (NULL: not kept).  Only enqueues on `stream`. */
int mfx_wboot2d_fit_dev(void* h, const double* d_Y, const double* d_W, int64_t w_stride, const double* d_peaks, int maxfasc,
                        int csf_on, const double* d_sig_csf, const double* d_params0, const double* d_pred0,
                        const int32_t* d_groups, const int64_t* d_vox, int64_t V, int B, int kind, int inflate, uint64_t seed,
                        uint64_t offset, const double* d_props, int nprop, const double* d_q, int Q, int64_t max_bytes,
                        double* d_stats, int32_t* d_agree, int32_t* d_status, int32_t* d_dir_status, double* d_keep,
                        void* stream);

/* A mixed batch on host buffers, as mfx_wfit2d_batch takes it: W [V x M] or [M], K [V] in 0..maxfasc, csf [V] flags (NULL:
 * none), peaks [V x 3 maxfasc], sig_csf [M]; params0, groups, vox, props, q as in mfx_boot_fit.  The voxels are binned by
 * class (class_batch.h) and every class runs as mfx_wboot2d_fit_dev does, in its own layout; the results come back in the
 * batch's layout (maxfasc, csf_on) by the rules of mfx_boot_fit: stats [V x C x (5 + Q)], agree [V x maxfasc], status
 * [V], dir_status [V x 5], keep [V x B x np] (NULL: not kept).  K = 0 without CSF keeps zero rows.  Waits for its own
 * work. */
int mfx_wboot2d_fit(void* h, const double* Y, const double* W, int64_t w_stride, const int32_t* K, const uint8_t* csf,
                    const double* peaks, int maxfasc, int csf_on, const double* sig_csf, const double* params0,
                    const int32_t* groups, const int64_t* vox, int64_t V, int B, int kind, int inflate, uint64_t seed,
                    uint64_t offset, const double* props, int nprop, const double* q, int Q, int64_t max_bytes, double* stats,
                    int32_t* agree, int32_t* status, int32_t* dir_status, double* keep);

#ifdef __cplusplus
}
#endif
#endif
