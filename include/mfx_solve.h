/*
 * mfx_solve.h -- C ABI of the batched explicit-dictionary solver: many signals against ONE fixed dictionary.
 * mfx_solve_exhaustive (mfx.h) serves one problem per call and pays for the dictionary every time: its upload, its Gram
 * matrix A^T A, a dozen allocations and a device synchronisation.  A handle of this header owns the dictionary and its
 * Gram on the device; per signal only A^T y and ||y||^2 are formed.  Kept apart from mfx.h, with its own version.
 * Conventions are those of mfx.h: plain pointers, row-major float64, 0 or an MFX_ERR_* code returned, mfx_last_error()
 * gives the message, no CPU path (without a usable device every entry point returns MFX_ERR_NO_DEVICE).
 *
 * THE CONTRACT.  Row v of a batch equals, bit for bit, what mfx_solve_exhaustive(A, Y[v], dicsizes) returns: weights,
 * sub-dictionary indices, objective and reconstruction - wherever the one-problem path does not switch to its
 * matrix-pipe screen (three sub-dictionaries, every size >= 16 and >= 2^18 tuples; the batch never uses that screen and
 * returns what the plain scan returns).  Claimed for finite signals.  A row of Y with a non-finite value gets status 1,
 * NaN weights, objective and reconstruction, indices -1, and is not scanned; every other row has status 0.
 *
 * Limits and messages are those of mfx_solve_exhaustive: at most 8 sub-dictionaries, 30000 columns, 2^40 index tuples.
 * Two sub-dictionaries, and three whose last has ONE column (the CSF-column class), run a tiled scan that reads the
 * Gram once per chunk of signals; every other class runs the one-problem scan with a signal dimension.
 */
#ifndef MFX_SOLVE_H
#define MFX_SOLVE_H
#include <stdint.h>

#include "mfx.h"
#ifdef __cplusplus
extern "C" {
#endif

/* version of this header's entry points; bumped on a signature change or a new entry point */
int mfx_solve_abi_version(void);

/* A solver for the dictionary A [M x lda] (the first sum(dicsizes) columns of every row count), dicsizes [Kp], on
 * `device`.  The dictionary is uploaded compacted, its Gram is summed sequentially over the rows (the one-problem path's
 * order), and for the tiled classes the signal-independent part of the score's error bound is tabulated per pair. */
int mfx_solve_create(const double* A, int64_t lda, int M, const int64_t* dicsizes, int Kp, int device, void** h);
void mfx_solve_destroy(void* h);
/* sum(dicsizes); -1 for a null handle */
int64_t mfx_solve_num_columns(const void* h);
/* scratch bytes one signal of a batch takes on the calling thread's route (what max_bytes is counted in):
 * 8 (columns + 4) + 8 cells + 16 min(tuples, 16384), cells = 4 per 64 x 64 tile of the pairs on the tiled route and
 * min(8192, ceil(tuples / 256)) otherwise; -1 for a null handle */
int64_t mfx_solve_bytes_per_signal(const void* h);

/* V signals d_Y [V x M] on device buffers -> d_w [V x Kp], d_sub [V x Kp] (index inside each sub-dictionary), d_obj [V],
 * d_yrec [V x M] (NULL: not written), d_status [V].  The signals go in chunks whose scratch (A^T y, the per-block maxima
 * and the candidate lists of every signal) stays within max_bytes (<= 0: 256 MiB; one signal at the least); scratch comes
 * from the stream's arena.  Only enqueues on `stream` (hipStream_t as void*, NULL = default stream). */
int mfx_solve_batch_dev(void* h, const double* d_Y, int64_t V, int64_t max_bytes, double* d_w, int64_t* d_sub, double* d_obj,
                        double* d_yrec, int32_t* d_status, void* stream);

/* The same on host buffers (yrec may be NULL).  Waits for its own work. */
int mfx_solve_batch(void* h, const double* Y, int64_t V, int64_t max_bytes, double* w, int64_t* sub, double* obj, double* yrec,
                    int32_t* status);

/* diagnostics: 1 = the tiled classes of the calling thread's next calls take the route of every other class */
void mfx_solve_debug_set_force_generic(int enabled);

#ifdef __cplusplus
}
#endif
#endif
