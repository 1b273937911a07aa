/*
 * mfx_profile.h -- C ABI of the objective profiles: what the exhaustive search of the fit sees and
 * throws away.  The fit reports the arg-min over all atom pairs; these entry points report, per atom
 * of each fascicle, the best objective any partner reaches with it (the profile of the objective
 * along that atom), or the objective of every pair (the landscape of single voxels).
 *
 * Kept apart from mfx.h so that mfx.h's symbol list and version stay as they are; this header has
 * its own version.  Conventions are those of mfx.h: plain pointers, row-major float64, 0 or an
 * MFX_ERR_* code returned, the library's last-error call gives the message, no CPU path (without a
 * usable device every entry point returns MFX_ERR_NO_DEVICE).  The _dev variants take device
 * pointers and a hipStream_t (as void*, NULL = default stream) and only enqueue work; the others
 * wait for their own work.
 *
 * Definitions.  A voxel has the signal y (M values) and K fascicle directions d_0 .. d_{K-1}
 * (peaks [V x 3 K]); D_k [M x N] is the dictionary rotated onto d_k, the columns the fit and
 * mfx_rotate produce.  All voxels of one call belong to ONE class (K, csf_on).
 *
 *   K = 2   obj[v, 0, i] = min_j F(D_0[:, i], D_1[:, j]),   partner[v, 0, i] = the arg-min j
 *           obj[v, 1, j] = min_i F(D_0[:, i], D_1[:, j]),   partner[v, 1, j] = the arg-min i
 *           F(a, b) = min_{w >= 0} || y - w_1 a - w_2 b ||^2, the value the reference's
 *           lsqnonneg_2var_opt returns (mf_utils.py:404-459) from ||y||^2, A11 = a.a, A12 = a.b,
 *           A22 = b.b, Y1 = a.y, Y2 = b.y: the unconstrained optimum when both of its weights are
 *           positive, else the better of the two single atoms (weight clipped at 0).
 *           A tie goes to the lowest index.
 *   K = 1   obj[v, 0, i] = ||y||^2 - max(Y_i, 0)^2 / A_ii,   partner = -1
 *   csf_on  the same with the weight w_x >= 0 of the fixed column x = sig_csf [M] as a further
 *           unknown.  x is projected out of a, b and y:
 *             A11' = A11 - (a.x)^2 / x.x,  A12' = A12 - (a.x)(b.x) / x.x,  Y1' = Y1 - (a.x)(x.y) / x.x,
 *             ||y'||^2 = ||y||^2 - (x.y)^2 / x.x   (likewise for b)
 *           the two-variable form is evaluated on the primed quantities, w_x = (x.y - w_1 a.x -
 *           w_2 b.x) / x.x is recovered; if w_x >= 0 that is the value, otherwise the value is the
 *           plain F(a, b) (by convexity the optimum then has w_x = 0).
 *
 * Values are sums of squares (not divided by M), float64, NOT clamped at zero.  min_i obj[v, 0, i]
 * is the fit's objective MSE * M and its arg-min the fitted atom.
 *
 * The cut.  A pair whose 1 - c^2 (c the cosine of the two atoms; of the primed atoms with csf_on)
 * is not above mfx_profile_cut() is scored as the better of its two single atoms, an upper bound of
 * F: the two-atom form loses its digits like 1 / (1 - c^2).  An atom whose primed norm a'.a' is not
 * above the cut times a.a (an atom parallel to x) contributes nothing beside x.
 *
 * Out of scope: three fascicles, the EAR compartment, voxels with no fascicle, 2-D protocols.  The
 * entry points take K = 1 or 2 only; callers that bin mixed volumes write NaN rows (partner -1)
 * for the other classes and count them (engine.profile does).
 *
 * Limits.  The protocols of the FP64 fit kernel: exact-G and G-bracketed rows, M <= 560.  K = 2
 * keeps per-atom statistics and the running column minima in the 160 KiB of LDS of a workgroup:
 * mfx_profile_max_atoms() gives the largest N for a plan and mode (exact-G protocols, profile:
 * 2480 atoms for M <= 200, 1872 with CSF; 1376 and 976 for M <= 560; G-bracketed rows cost a few
 * hundred atoms).  Beyond either limit: MFX_ERR_UNSUPPORTED, the limit in
 * the message.  A fascicle direction that fails the reference's unit-norm test flags the plan's
 * status word like the fit does (mfx_plan_status: MFX_ERR_DIR_NORM); the voxel is still computed.
 */
#ifndef MFX_PROFILE_H
#define MFX_PROFILE_H
#include <stdint.h>

#include "mfx.h"
#ifdef __cplusplus
extern "C" {
#endif

/* version of this header's entry points; bumped on a signature change or a new entry point */
int mfx_profile_abi_version(void);

/* the cut on 1 - c^2 described above (a compile-time constant of the library, at most 1e-6) */
double mfx_profile_cut(void);

/* largest dictionary the K = 2 kernels serve for this plan; landscape != 0: the all-pairs mode */
int mfx_profile_max_atoms(const mfx_plan* p, int csf_on, int landscape);

/*
 * Debug: which K = 2 kernel the calling thread's last launch through this header or the weighted
 * forms of mfx_wsoft.h (mfx_wprofile*, mfx_wpair_objectives*) was.  form[8] = (KSTEPS, NW, TILES,
 * NBUF, BR, CSF, LAND, WGT): k-steps of 4 rows (the padded M is 4 KSTEPS), waves per workgroup,
 * 16-atom column tiles per chunk, LDS chunk buffers, G-bracketed rows, the CSF form, the landscape
 * form, measurement weights.  Returns 1, or 0 with form untouched before the thread's first such
 * launch.  K = 1 calls and calls refused before the launch leave the record as it is.  Since 2.
 */
int mfx_profile_debug_last_config(int* form);

/*
 * Profile.  d_Y [V x M], d_peaks [V x 3 K], d_sig_csf [M] (csf_on), d_obj [V x K x N] float64,
 * d_partner [V x K x N] int32 or NULL.  One workgroup per voxel; no global atomics, nothing of
 * size N x N is stored.  The result does not depend on the launch (fixed reduction orders).
 */
int mfx_profile_dev(const mfx_plan* p, const double* d_Y, const double* d_peaks, int K, int csf_on,
                    const double* d_sig_csf, int64_t V, double* d_obj, int32_t* d_partner, void* stream);
int mfx_profile(const mfx_plan* p, const double* Y, const double* peaks, int K, int csf_on, const double* sig_csf,
                int64_t V, double* obj, int32_t* partner);

/*
 * Landscape (K = 2): out [V x N x N], out[v, i, j] = F(D_0[:, i], D_1[:, j]) (with csf_on: the
 * three-unknown value above).  Meant for single voxels: V N^2 doubles are written.
 */
int mfx_pair_objectives_dev(const mfx_plan* p, const double* d_Y, const double* d_peaks, int csf_on,
                            const double* d_sig_csf, int64_t V, double* d_out, void* stream);
int mfx_pair_objectives(const mfx_plan* p, const double* Y, const double* peaks, int csf_on, const double* sig_csf,
                        int64_t V, double* out);

#ifdef __cplusplus
}
#endif
#endif
