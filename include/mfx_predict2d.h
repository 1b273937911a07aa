/*
 * mfx_predict2d.h -- C ABI of the forward model of 2-D (AxCaliber-like) protocols: parameters -> signal, the y_rec
 * of the reference chain of mfx_fit2d.h (rotate_atom_2Dprotocol per fascicle -> solve_exhaustive_posweights), with
 * the optional magnitude noise and residual of mfx_predict.h in the same pass.  On a handle of mfx_rot2d.h
 * (mfx_rot2d_create).  Kept apart from every other header, with its own version.  Conventions are those of mfx.h:
 * plain pointers, row-major float64, 0 or an MFX_ERR_* code returned, mfx_last_error() gives the message, no CPU
 * path (without a usable device every entry point returns MFX_ERR_NO_DEVICE).
 *
 * params [V x (1 + 2 maxfasc + csf_on + 2)] has the layout of mfx_fit2d.h's rows:
 *   [M0, nu_0 .. nu_{maxfasc-1}, atom_0 .. atom_{maxfasc-1}, (nu_csf if csf_on), MSE, R2]      (the last two are ignored)
 * peaks [V x 3 maxfasc] the fascicle directions, sig_csf [M] the CSF signal (csf_on).  out [V x M]:
 *
 *   out[v, m] = acc after, for c = f0, f1, f2, csf in that order and only where w_c = fl(M0 * nu_c) > 0:
 *               acc = fl(acc + fl(w_c * s_c[m])),   acc starting at 0.0
 *
 * with s_c[m] of a fascicle the entry mfx_rot2d_rotate_cols returns for (direction, atom): the same expression on the
 * same operands, the same bits.  A compartment whose weight is exactly 0 is skipped: its direction and atom index are
 * not looked at (an absent fascicle's zero direction does not flag the voxel).  A fascicle with positive weight whose
 * direction fails (mfx_rot2d.h's status codes) gives a NaN row, and dir_status [V x 5] holds the record
 * {code, pair, value, value2, fascicle} of mfx_fit2d.h for the lowest such fascicle (zeros for a served voxel).
 * An atom index that is not an integer in [0, N), or a weight that is negative or not finite, is an argument error:
 * the host entry point returns MFX_ERR_ARG before any launch; the device entry point writes a NaN row (no table is
 * read out of range) and flags status[0] with the MFX_PRED_ST_* bits of mfx_predict.h, status[1] holding one such
 * voxel.  status is int32[2] in device memory, zeroed by the caller.
 *
 * Y [V x M] not NULL: stats [V x 2] receives per voxel the residual sum of squares and R2 by the rule of
 * mfx_predict.h, summed by one wave in a fixed order that depends on M alone.
 * ncoils > 0: the magnitude noise of mfx_sos_noise (mfx_predict.h) is applied in the same pass with element index
 * i = v M + m; sigma / sigma_mode (MFX_SIGMA_*) / seed / offset as in mfx_predict.h.
 *
 * maxfasc > 3 and protocols of more than the rotation's 4000 rows return MFX_ERR_UNSUPPORTED.  Extra-axonal (EAR)
 * columns are not served: no argument carries them.
 */
#ifndef MFX_PREDICT2D_H
#define MFX_PREDICT2D_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* version of this header's entry points; bumped on a signature change or a new entry point */
int mfx_predict2d_abi_version(void);

/* Device buffers; only enqueues on `stream` (hipStream_t as void*, NULL = default stream): the plan of the V maxfasc
 * directions, their records and the prediction kernel, with scratch from the stream's arena. */
int mfx_predict2d_dev(void* h, const double* d_params, const double* d_peaks, int maxfasc, int csf_on,
                      const double* d_sig_csf, int64_t V, const double* d_Y, const double* d_sigma, int sigma_mode, int ncoils,
                      uint64_t seed, uint64_t offset, double* d_out, double* d_stats, int32_t* d_status,
                      int32_t* d_dir_status, void* stream);

/* Host buffers; checks atom indices and weights first, waits for its own work. */
int mfx_predict2d(void* h, const double* params, const double* peaks, int maxfasc, int csf_on, const double* sig_csf,
                  int64_t V, const double* Y, const double* sigma, int sigma_mode, int ncoils, uint64_t seed, uint64_t offset,
                  double* out, double* stats, int32_t* dir_status);

#ifdef __cplusplus
}
#endif
#endif
