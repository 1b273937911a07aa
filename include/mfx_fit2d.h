/*
 * mfx_fit2d.h -- C ABI of the batched fit of voxels measured with a 2-D (AxCaliber-like) protocol: per voxel
 * the reference chain
 *
 *   D_k = rotate_atom_2Dprotocol(sig, sch_mat, refdir, peaks[3k:3k+3], DIFF)      k < K
 *   A   = [D_0 | ... | D_{K-1} | sig_csf if the voxel is flagged]
 *   w, ind, _, SoS, y_rec = solve_exhaustive_posweights(A, y, [N]*K (+[1]))
 *   row = the packing of mf.py:420-450
 *
 * on a handle of mfx_rot2d.h (mfx_rot2d_create).  Kept apart from mfx.h, with its own version.  Conventions
 * are those of mfx.h: plain pointers, row-major float64, 0 or an MFX_ERR_* code returned, mfx_last_error()
 * gives the message, no CPU path (without a usable device every entry point returns MFX_ERR_NO_DEVICE).
 *
 * params row of a voxel (engine.num_params(maxfasc, csf_on, False) = 1 + 2 maxfasc + csf_on + 2 doubles):
 *   [M0, nu_0 .. nu_{maxfasc-1}, atom_0 .. atom_{maxfasc-1}, (nu_csf if csf_on), MSE, R2]
 * status record of a voxel, int32[5]: {code, pair, value, value2, fascicle}: the mfx_rot2d.h record of the
 * voxel's lowest failing fascicle direction and that fascicle's index; code 0 = the voxel was fitted.  A voxel
 * with a failing direction is not fitted: its params row is NaN.
 *
 * Voxel classes: two fascicles without a CSF column run one fused kernel (the rotated dictionaries are never
 * written to memory in full) for dictionaries up to mfx_fit2d_max_atoms(h, 2) atoms; one fascicle without CSF
 * runs a one-thread-per-atom kernel.  Every other class (a CSF column, three fascicles, larger dictionaries)
 * has its dictionaries materialised in voxel chunks and goes through the explicit solver behind
 * mfx_solve_exhaustive on the device: slow, same results.  K = 0 without CSF gives a zero row.  Extra-axonal
 * (EAR) columns are not served: no argument carries them, and maxfasc > 3 returns MFX_ERR_UNSUPPORTED.
 */
#ifndef MFX_FIT2D_H
#define MFX_FIT2D_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* version of this header's entry points; bumped on a signature change or a new entry point */
int mfx_fit2d_abi_version(void);

/* largest dictionary the fused kernel of K fascicles serves (0: no fused kernel for this K) */
int mfx_fit2d_max_atoms(void* h, int K);

/* One homogeneous class on device buffers: every voxel has K = maxfasc fascicles and no CSF column.
 * d_Y [V x M], d_peaks [V x 3 maxfasc] -> d_params [V x (1 + 2 maxfasc + 2)], d_status [V x 5].
 * Only enqueues on `stream` (hipStream_t as void*, NULL = default stream). */
int mfx_fit2d_batch_dev(void* h, const double* d_Y, const double* d_peaks, int maxfasc, int64_t V, double* d_params,
                        int32_t* d_status, void* stream);

/* A mixed batch on host buffers: K [V] in 0..maxfasc, csf [V] flags (NULL: none; flagged voxels need csf_on and
 * sig_csf [M]), peaks [V x 3 maxfasc] -> params [V x (1 + 2 maxfasc + csf_on + 2)], status [V x 5].  Bins the
 * voxels by class and waits for its own work. */
int mfx_fit2d_batch(void* h, const double* Y, const int32_t* K, const uint8_t* csf, const double* peaks, int maxfasc,
                    int csf_on, const double* sig_csf, int64_t V, double* params, int32_t* status);

/* diagnostics: 1 = every class of the calling thread's next calls takes the materialise-and-solve path */
void mfx_fit2d_debug_set_force_explicit(int enabled);

#ifdef __cplusplus
}
#endif
#endif
