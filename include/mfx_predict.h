/*
 * mfx_predict.h -- C ABI of the forward model: parameters -> DW-MRI signal (the y_rec that the
 * reference's voxel loop computes and drops, mf.py:413-419), and the sum-of-squares magnitude noise
 * of the reference's mf_utils.gen_SoS_MRI (mf_utils.py:2303-2354).
 *
 * Kept apart from mfx.h so that mfx.h's symbol list and version stay as they are; this header has
 * its own version.  Conventions are those of mfx.h: plain pointers, row-major float64, 0 or an
 * MFX_ERR_* code returned, the library's last-error call gives the message, no CPU path (without a
 * usable device every entry point returns MFX_ERR_NO_DEVICE).  The _dev variants take device
 * pointers and a hipStream_t (as void*, NULL = default stream) and only enqueue work; the others
 * wait for their own work.
 *
 * Prediction.  params [V x num_params] has the layout of the fit's output (mf.py:376-381):
 *   M0, nu_f[maxfasc], ID_f[maxfasc], nu_csf (if csf_on), nu_ear, ID_ear (if ear_on), MSE, R2
 * (the last two are ignored), peaks [V x 3 maxfasc] the fascicle directions, sig_csf [M] and
 * sig_ear [M x E] the optional compartments' signals.  out [V x M]:
 *
 *   out[v, m] = sum over the compartments c = f0, f1, ..., csf, ear, in that order, of
 *               (M0_v * nu_{v,c}) * s_c[m]
 *
 * with s_c[m] of a fascicle the atom ID evaluated along the voxel's direction exactly as the
 * library's single-atom rotation evaluates it (same bits for the same direction and atom).
 * A compartment whose weight M0 * nu is exactly 0 is skipped: its direction and ID are not read.
 * A fascicle with positive weight whose direction fails the reference's unit-norm test flags the
 * plan's status word like the fit does (reported by the plan's status call as MFX_ERR_DIR_NORM).
 * An ID that is not an integer in [0, N) (or [0, E)), or a weight that is negative or not finite,
 * is an argument error: the host entry point returns MFX_ERR_ARG before any launch; the device
 * entry point writes a NaN row (no table is read out of range) and flags status[0], status[1]
 * holding one such voxel.  status is int32[2] in device memory, zeroed by the caller.
 *
 * Noise (ncoils > 0): the value above is S0 of the model below and the noisy magnitude is stored
 * instead, in the same pass.  sigma_mode says how sigma is indexed:
 */
#ifndef MFX_PREDICT_H
#define MFX_PREDICT_H
#include <stdint.h>

#include "mfx.h"
#ifdef __cplusplus
extern "C" {
#endif

#define MFX_SIGMA_SCALAR 0    /* sigma[0] for every element */
#define MFX_SIGMA_VOXEL 1     /* sigma[v] (prediction only) */
#define MFX_SIGMA_ELEMENT 2   /* sigma[i], i the element's index in the output */

#define MFX_PRED_ST_ID 1       /* status[0] bits of the device entry point: an atom index out of range */
#define MFX_PRED_ST_WEIGHT 2   /* a weight that is negative or not finite */

/* version of this header's entry points; bumped on a signature change or a new entry point */
int mfx_predict_abi_version(void);

/*
 * Residual (Y [V x M] not NULL): stats [V x 2] receives per voxel the residual sum of squares
 * sum_m (Y - out)^2 and the coefficient of determination by the reference's rule (mf.py:449-450:
 * corrcoef(Y, out)^2 when M > 1 and both have a positive spread, else 0).  One wave sums a voxel in
 * a fixed order that does not depend on the launch.
 */
int mfx_predict_dev(const mfx_plan* p, const double* d_params, const double* d_peaks, int maxfasc, int csf_on,
                    int ear_on, const double* d_sig_csf, const double* d_sig_ear, int E, int64_t V, const double* d_Y,
                    const double* d_sigma, int sigma_mode, int ncoils, uint64_t seed, uint64_t offset, double* d_out,
                    double* d_stats, int32_t* d_status, void* stream);
int mfx_predict(const mfx_plan* p, const double* params, const double* peaks, int maxfasc, int csf_on, int ear_on,
                const double* sig_csf, const double* sig_ear, int E, int64_t V, const double* Y, const double* sigma,
                int sigma_mode, int ncoils, uint64_t seed, uint64_t offset, double* out, double* stats);

/*
 * out[i] = sqrt( sum_{j < ncoils} (S0[i] + sigma_i a_ij)^2 + (sigma_i b_ij)^2 ), a and b independent
 * standard normals (sqrt(ncoils) |S0[i]| where sigma_i is 0).  Counter-based generator, Philox4x32-10:
 * key = seed, counter = (low and high word of offset + i, j, a stream constant); its four words make
 * two 53-bit uniforms, one Box-Muller pair, one coil's (a, b).  Element i's value therefore depends on
 * (seed, offset + i, ncoils, S0[i], sigma_i) only -- not on n, nor on how an array is split into calls.
 * The fused noise of the prediction is this function with i = v M + m.
 * sigma_mode: MFX_SIGMA_SCALAR or MFX_SIGMA_ELEMENT.  out may alias S0.
 */
int mfx_sos_noise_dev(const double* d_S0, int64_t n, const double* d_sigma, int sigma_mode, int ncoils, uint64_t seed,
                      uint64_t offset, double* d_out, int device, void* stream);
int mfx_sos_noise(const double* S0, int64_t n, const double* sigma, int sigma_mode, int ncoils, uint64_t seed,
                  uint64_t offset, double* out, int device);

#ifdef __cplusplus
}
#endif
#endif
