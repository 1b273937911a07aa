/*
 * mfx_solve_soft.h -- C ABI of the soft answers of the batched explicit-dictionary solver (mfx_solve.h): for many
 * signals against ONE fixed dictionary, the objective profile of every atom (what mfx_profile.h serves per voxel) and
 * the posterior weight of every atom given the noise level (what mfx_post.h serves per voxel).  The handle of
 * mfx_solve_create already owns G = A^T A; per signal only A^T y and ||y||^2 are formed, by the solver's own kernel.
 * Kept apart from mfx_solve.h so that its symbol list and version stay as they are; this header has its own version.
 * Conventions are those of mfx_solve.h: plain pointers, row-major float64, 0 or an MFX_ERR_* code returned,
 * mfx_last_error() gives the message, no CPU path (without a usable device every entry point that computes returns
 * MFX_ERR_NO_DEVICE).  The _dev forms take device pointers and a hipStream_t (as void*, NULL = default stream), only
 * enqueue, and take their scratch from the stream's arena; the host forms wait for their own work.
 *
 * CLASSES SERVED, by the handle's dicsizes (the columns of A in that order):
 *   [n]          F(i) = ||y||^2 - max(Y_i, 0)^2 / A_ii: the K = 1 form of mfx_profile.h / mfx_post.h
 *   [n1, n2]     any sizes, n2 = 1 included: F(i, j) of atom i of the first and atom j of the second sub-dictionary is
 *                the two-variable form of mfx_profile.h, with the cut mfx_profile_cut() on 1 - c^2
 *   [n1, n2, 1]  the third column is x, the CSF form of mfx_profile.h: x projected out of both atoms and the signal,
 *                the two-variable form on the primed quantities, the sign of w_x deciding between that and the plain
 *                F(i, j); the cut applies to the primed atoms
 * Every other class: MFX_ERR_UNSUPPORTED, the class named in the message, no launch and no output written.
 *
 * F is the value mfx_profile.h defines, evaluated from G, A^T y and the sequential sum ||y||^2 (the one the solver's
 * tiled route uses) by the pair-scoring functions of the per-voxel kernels: for equal Gram scalars the same bits.
 *
 * PROFILE.  obj0[v, i] = min_j F(i, j), partner0[v, i] the arg-min j; obj1[v, j] = min_i F(i, j), partner1[v, j] the
 * arg-min i.  A tie goes to the lowest index.  One sub-dictionary: obj0[v, i] = F(i), partners -1, and obj1 / partner1
 * must be NULL.  Values are sums of squares, NOT clamped at zero.  status[v]: 0 ok, 5 the signal holds a non-finite
 * value (mfx_solve_batch's status 1, renumbered beside the posterior's codes): NaN rows, partners -1.
 *
 * POSTERIOR.  With T[v] > 0 the temperature (2 sigma^2) and shift[v] any value near min F (mfx_post.h):
 *   t(i, j) = exp(-(F(i, j) - shift) / T),  R0[i] = sum_j t(i, j),  R1[j] = sum_i t(i, j),  Z = sum_i R0[i]
 *   w0[v, i] = R0[i] / Z,  w1[v, j] = R1[j] / Z,  log_sum[v] = log Z - shift / T
 * (one sub-dictionary: t(i) = exp(-(F(i) - shift) / T), w0 = t / Z, w1 must be NULL).  shift == NULL: the library takes
 * the signal's own min F, from a minimum pass of its own; minF [V] (or NULL) receives min F of every signal either way.
 * status[v]:
 *   0   ok
 *   1   T is not finite or <= 0, or a given shift is not finite
 *   2   an exponent above 700 was met, or Z is 0 or not finite: the shift is unusable
 *   5   the signal holds a non-finite value
 * A signal with a non-zero status gets NaN rows and a NaN log_sum (status 5: a NaN minF too); its neighbours are
 * untouched.
 *
 * DETERMINISM.  No floating-point atomics.  The pairs are cut into 64 x 64 tiles, tile (tr, tc) holding rows 64 tr ..
 * and columns 64 tc ..; the geometry depends on the sizes alone.  Inside a tile a row sum runs over the tile's 64
 * columns as a butterfly (partners at distance 32, 16, 8, 4, 2, 1; a column beyond n2 adds an exact 0); a column sum
 * runs over the rows r = w, w + 4, w + 8, .. of each of four groups w = 0 .. 3 in increasing r, then over the groups
 * in the order 0, 1, 2, 3.  R0[i] adds the tiles' row sums in increasing tc, R1[j] the tiles' column sums in increasing
 * tr, Z adds R0 in index order.  Minima are order-independent; ties are resolved by the index.  A signal's row of
 * every output is therefore the same bits whatever the other signals of the call, V, its position, max_bytes and the
 * chunking, and however the signals are dealt to the workgroups.
 *
 * SCRATCH.  The signals go in chunks whose scratch stays within max_bytes (<= 0: 256 MiB; one signal at the least).
 * With P = tiles_c n1 + tiles_r n2 (tiles_r = ceil(n1 / 64), tiles_c = ceil(n2 / 64); P = 0 for one sub-dictionary)
 * a signal takes 8 (columns + 8) + 12 P bytes in the profile and 8 (columns + 8) + 8 P bytes in the posterior.
 *
 * Out of scope: per-signal measurement weights (they would make the Gram per-signal, which is what the per-voxel
 * kernels of mfx_wsoft.h are for; a shared [M] weight vector is the caller scaling the rows of A and Y by sqrt(W)),
 * three general sub-dictionaries and four or more, bootstrap on the solver, the landscape ([n1 x n2] values per
 * signal), sharding over several devices.
 */
#ifndef MFX_SOLVE_SOFT_H
#define MFX_SOLVE_SOFT_H
#include <stdint.h>

#include "mfx.h"
#ifdef __cplusplus
extern "C" {
#endif

#define MFX_SOLVE_SOFT_PROFILE 0
#define MFX_SOLVE_SOFT_POST 1

/* version of this header's entry points; bumped on a signature change or a new entry point */
int mfx_solve_soft_abi_version(void);

/* 0 if the handle's class is served, else MFX_ERR_UNSUPPORTED with the class in the message (MFX_ERR_ARG for a null
 * handle).  Needs no device. */
int mfx_solve_soft_served(const void* h);

/* scratch bytes one signal takes in mfx_solve_profile* (what = MFX_SOLVE_SOFT_PROFILE) or mfx_solve_post* (what =
 * MFX_SOLVE_SOFT_POST): what max_bytes is counted in.  -1 for a null handle, an unserved class or another `what`. */
int64_t mfx_solve_soft_bytes_per_signal(const void* h, int what);

/* d_Y [V x M] -> d_obj0 [V x n1], d_obj1 [V x n2], d_partner0 [V x n1], d_partner1 [V x n2] int32 (both NULL or both
 * given; one sub-dictionary: d_obj1 and d_partner1 NULL, d_partner0 optional), d_status [V] int32. */
int mfx_solve_profile_dev(void* h, const double* d_Y, int64_t V, int64_t max_bytes, double* d_obj0, double* d_obj1,
                          int32_t* d_partner0, int32_t* d_partner1, int32_t* d_status, void* stream);
int mfx_solve_profile(void* h, const double* Y, int64_t V, int64_t max_bytes, double* obj0, double* obj1, int32_t* partner0,
                      int32_t* partner1, int32_t* status);

/* d_Y [V x M], d_T [V], d_shift [V] or NULL -> d_w0 [V x n1], d_w1 [V x n2] (one sub-dictionary: NULL), d_log_sum [V],
 * d_minF [V] or NULL, d_status [V] int32. */
int mfx_solve_post_dev(void* h, const double* d_Y, int64_t V, const double* d_T, const double* d_shift, int64_t max_bytes,
                       double* d_w0, double* d_w1, double* d_log_sum, double* d_minF, int32_t* d_status, void* stream);
int mfx_solve_post(void* h, const double* Y, int64_t V, const double* T, const double* shift, int64_t max_bytes, double* w0,
                   double* w1, double* log_sum, double* minF, int32_t* status);

#ifdef __cplusplus
}
#endif
#endif
