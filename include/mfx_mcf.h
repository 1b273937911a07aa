/*
 * mfx_mcf.h -- C ABI of the MCF signal synthesis (reference mcf.py: MCF_PGSE, MCF_DDE).
 *
 * Kept apart from mfx.h so that mfx.h's symbol list and version stay as they are; this header
 * has its own version.  Conventions are those of mfx.h: plain pointers, row-major float64,
 * 0 or an MFX_ERR_* code returned, mfx_last_error() gives the message, no CPU path (without a
 * usable device every entry point returns MFX_ERR_NO_DEVICE).  The entry points run on the
 * calling thread's current HIP device and wait for their own work.
 *
 * Signal of an impermeable cylinder of radius L[a], free diffusivity diff[a] inside, axis
 * envdir, for every row of a PGSE or DDE protocol, by the multiple-correlation-function matrix
 * formalism on M Laplace eigenmodes (Grebenkov 2008).  The Python layer (mcf.py) does the
 * reference's validation first (scheme checks, q/p accuracy check, gradient norms); the
 * library only rejects malformed arguments.
 *
 * lam   [M]        Laplace eigenvalues, ascending, lam[0] = 0
 * B     [M x M]    real symmetric coupling matrix <u_i | x | u_j>
 * M                1 <= M <= 64
 * seq   [n_seq x 7]  PGSE rows  [gx gy gz G Delta delta TE]            (mfx_mcf_pgse)
 *       [n_seq x 14] DDE rows   [g1 G1 Delta1 delta1 tau_mix g2 G2 Delta2 delta2 TE] (mfx_mcf_dde)
 * L, diff [n_atoms]  radius [m] and diffusivity [m^2/s] of each atom (> 0, finite)
 * envdir [3]       cylinder axis, non-zero; divided by its norm here as the reference does
 * E_out [n_seq x n_atoms]  normalised signal, laid out like a dictionary's columns
 */
#ifndef MFX_MCF_H
#define MFX_MCF_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* version of this header's entry points; bumped on a signature change or a new entry point */
int mfx_mcf_abi_version(void);

int mfx_mcf_pgse(const double* lam, const double* B, int M, const double* seq, int64_t n_seq, const double* L,
                 const double* diff, int64_t n_atoms, const double* envdir, double gamma, double* E_out);

int mfx_mcf_dde(const double* lam, const double* B, int M, const double* seq, int64_t n_seq, const double* L,
                const double* diff, int64_t n_atoms, const double* envdir, double gamma, double* E_out);

#ifdef __cplusplus
}
#endif
#endif
