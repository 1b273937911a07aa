/*
 * mfx_boot2d.h -- C ABI of the bootstrap for voxels of a 2-D (AxCaliber-like) protocol, on a handle of mfx_rot2d.h
 * (mfx_rot2d_create): the bootstrap of mfx_boot.h - the same resampling rule, value table and statistics, word for word,
 * with ear_on = 0 (the parameter rows of mfx_fit2d.h have the layout of mfx.h's rows without EAR columns) - around the fit
 * of mfx_fit2d.h and the prediction of mfx_predict2d.h.  Kept apart from the other headers, with its own version.
 * Conventions are those of mfx.h: plain pointers, row-major float64, 0 or an MFX_ERR_* code returned, mfx_last_error()
 * gives the message, no CPU path (without a usable device every entry point returns MFX_ERR_NO_DEVICE).
 *
 * The primitive underneath is the REPLICATE FIT: B signals per voxel on one set of directions (the replicates of a
 * bootstrap, or many noise realisations of one voxel geometry).  The B rows of a voxel share both rotated dictionaries,
 * their column norms and the cross-Gram D_0^T D_1; only D^T y* differs between them.  For one and two fascicles without a
 * CSF column the directions' records, the column norms and the Gram are therefore formed ONCE per voxel, and every row
 * is finished on them by the arithmetic of the plain kernels: a replicate's row equals, bit for bit, the row
 * mfx_fit2d_batch_dev returns for that signal with those directions.  Every other class (a CSF column, three fascicles,
 * dictionaries beyond mfx_fit2d_max_atoms(h, 2)) takes the plain path: the kernels of mfx_fit2d.h on the replicate rows
 * with the directions copied, in chunks of voxels - slow, same results.
 *
 * A voxel with a failing direction (mfx_rot2d.h's status codes) keeps its record in dir_status [V x 5] (the record of
 * mfx_fit2d.h); its replicate rows are NaN, its bootstrap status is 2 and its statistics are NaN.  No fit kernel sees a
 * NaN signal: the replicate signals of a voxel in a non-zero status are zero rows while they are fitted.
 * B <= MFX_BOOT_MAX_B and Q <= MFX_BOOT_MAX_Q in the bootstrap entry points, else MFX_ERR_UNSUPPORTED before any launch.
 * Measurement weights and robust fits are served by mfx_wboot2d.h (the weights held fixed).  Not served: EAR columns.
 */
#ifndef MFX_BOOT2D_H
#define MFX_BOOT2D_H
#include <stdint.h>

#include "mfx_boot.h"
#ifdef __cplusplus
extern "C" {
#endif

/* version of this header's entry points; bumped on a signature change or a new entry point */
int mfx_boot2d_abi_version(void);

/* replicates per register tile of the column statistics kernel (the replicate counts around it are the kernel's seams) */
int mfx_boot2d_rep_tile(void);

/* diagnostics: 1 = every class of the calling thread's next calls takes the plain path */
void mfx_boot2d_debug_set_force_plain(int enabled);

/* The replicate fit of one class on device buffers: every voxel has K = maxfasc fascicles and no CSF column.
 * d_Ystar [V x B x M], d_peaks [V x 3 maxfasc] -> d_params [V x B x (1 + 2 maxfasc + 2)], d_status [V x 5] (per voxel, not
 * per row).  Scratch (the Gram [NP x NP] of a voxel, NP = N rounded up to 16, and D^T y* [B x K x NP]) comes from the
 * stream's arena, in chunks of voxels of at most 256 MiB.  Only enqueues on `stream` (hipStream_t as void*, NULL =
 * default stream). */
int mfx_boot2d_fit_rows_dev(void* h, const double* d_Ystar, const double* d_peaks, int maxfasc, int64_t V, int B,
                            double* d_params, int32_t* d_status, void* stream);

/* The bootstrap of one homogeneous class on device buffers: every voxel has maxfasc fascicles and the CSF column iff
 * csf_on.  Arguments as mfx_boot_fit_dev takes them, without EAR: d_params0 [V x np] the voxels' own fit (NULL: the fit
 * of mfx_fit2d.h runs first), d_pred0 [V x M] its prediction (NULL: mfx_predict2d's kernel runs).  Per chunk of voxels -
 * sized so that the replicate signals and the replicate fit's scratch of a chunk stay within max_bytes (<= 0: 256 MiB;
 * one voxel at the least) - the directions are prepared once and serve the own fit, the prediction and the replicate
 * fit; then mfx_boot_resample_dev, the replicate fit, mfx_boot_gather_dev, mfx_boot_reduce_dev.  -> d_stats
 * [V x C x (5 + Q)], d_agree [V x maxfasc] (NULL with maxfasc = 0), d_status [V], d_dir_status [V x 5], d_keep
 * [V x B x np] the replicate rows (NULL: not kept).  Only enqueues on `stream`. */
int mfx_boot2d_fit_dev(void* h, const double* d_Y, const double* d_peaks, int maxfasc, int csf_on, const double* d_sig_csf,
                       const double* d_params0, const double* d_pred0, const int32_t* d_groups, const int64_t* d_vox, int64_t V,
                       int B, int kind, int inflate, uint64_t seed, uint64_t offset, const double* d_props, int nprop,
                       const double* d_q, int Q, int64_t max_bytes, double* d_stats, int32_t* d_agree, int32_t* d_status,
                       int32_t* d_dir_status, double* d_keep, void* stream);

/* A mixed batch on host buffers, as mfx_fit2d_batch takes it: K [V] in 0..maxfasc, csf [V] flags (NULL: none), peaks
 * [V x 3 maxfasc], sig_csf [M]; params0, groups, vox, props, q as in mfx_boot_fit.  The voxels are binned by class
 * (class_batch.h) and every class runs as mfx_boot2d_fit_dev does, in its own layout; the results come back in the
 * batch's layout (maxfasc, csf_on) by the rules of mfx_boot_fit: stats [V x C x (5 + Q)], agree [V x maxfasc], status
 * [V], dir_status [V x 5], keep [V x B x np] (NULL: not kept).  K = 0 without CSF keeps zero rows.  Waits for its own
 * work. */
int mfx_boot2d_fit(void* h, const double* Y, const int32_t* K, const uint8_t* csf, const double* peaks, int maxfasc, int csf_on,
                   const double* sig_csf, const double* params0, const int32_t* groups, const int64_t* vox, int64_t V, int B,
                   int kind, int inflate, uint64_t seed, uint64_t offset, const double* props, int nprop, const double* q, int Q,
                   int64_t max_bytes, double* stats, int32_t* agree, int32_t* status, int32_t* dir_status, double* keep);

#ifdef __cplusplus
}
#endif
#endif
