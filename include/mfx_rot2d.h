/*
 * mfx_rot2d.h -- C ABI of the 2-D (AxCaliber-like) protocol rotation (reference mf_utils.py:
 * rotate_atom_2Dprotocol), for B fascicle directions per call.
 *
 * Kept apart from mfx.h so that mfx.h's symbol list and version stay as they are; this header
 * has its own version.  Conventions are those of mfx.h: plain pointers, row-major float64,
 * 0 or an MFX_ERR_* code returned, mfx_last_error() gives the message, no CPU path (without a
 * usable device every entry point returns MFX_ERR_NO_DEVICE).  The _dev variants take device
 * pointers and a hipStream_t (as void*, NULL = default stream) and only enqueue work; the others
 * wait for their own work.
 *
 * The direction-independent part (the reference fascicle's side) is computed on the host by the
 * Python layer (mf_utils.RotateAtom2DTables) with the reference's own NumPy arithmetic and handed
 * over here once:
 *
 * sch       [M x 6]   gx gy gz G Delta delta of every row, as the new fascicle's side sees them
 * pair_off  [P + 1]   rows of (Delta, delta) pair p (np.unique order) are pair_rows[pair_off[p] ..]
 * pair_rows [M]       row indices, ascending within a pair
 * ref_info  [P x 3]   per pair: status code of the reference side (0 or MFX_ROT2D_REF_*), the count
 *                     its message prints, the number of unique perpendicular directions (<= 5 when 0)
 * ref_dirs  [P x 5 x 2]  those directions in np.unique's lexicographic order
 * ref_tab   [P x 5]   knot table of the line through direction u (u with its opposite), or
 *                     -1 - (times u occurs among the reference's opposite pairs) when there is none
 * row_const [M]       b0 rows: constant row holding the row's signal; -1 for the other rows
 * van_const [P]       constant row that vanished rows of pair p take; -1 when p has no b0 row
 * cst       [C x N]   constant rows
 * tab_off   [T + 1]   knots of table t are knot_x[tab_off[t] ..], at least 2, ascending (stable sort)
 * knot_x    [K]       signed perpendicular gradient strengths of the reference line
 * knot_y    [K x N]   perpendicular signals S_perp_ref at those knots
 *
 * Status record of each direction, int32[4]: {code, pair (0-based), value, value2}; code 0 = the
 * direction succeeded.  The codes name the first check that failed in the reference's order.  The per-(direction, row)
 * plan records behind these entry points are shared with the fit of mfx_fit2d.h, which takes the same handle:
 */
#ifndef MFX_ROT2D_H
#define MFX_ROT2D_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define MFX_ROT2D_OK 0
#define MFX_ROT2D_NEWDIR_NORM 1   /* newdir does not have unit norm */
#define MFX_ROT2D_CHK_NEW 2       /* G^2 != G_perp^2 + G_par^2 for the new fascicle */
#define MFX_ROT2D_CHK_PAR_NEW 3   /* S_par != 1 on a b0 row for the new fascicle */
#define MFX_ROT2D_REF_UNIQUE 4    /* value: unique directions on the reference side */
#define MFX_ROT2D_REF_PAIRS 5     /* value: opposite (ordered) pairs on the reference side */
#define MFX_ROT2D_NEW_UNIQUE 6    /* value: unique directions on the new side */
#define MFX_ROT2D_NEW_PAIRS 7     /* value: opposite (upper-triangle) pairs on the new side */
#define MFX_ROT2D_VANISHED 8      /* rows with a vanished perpendicular component, no b0 row in the pair */
#define MFX_ROT2D_INTERP_B0 9     /* value: line index (0-based), value2: number of lines */
#define MFX_ROT2D_NO_REF_LINE 10  /* value: rows of the pair, value2: matches of the chosen reference direction */

/* version of this header's entry points; bumped on a signature change or a new entry point */
int mfx_rot2d_abi_version(void);

int mfx_rot2d_create(const double* sch, int M, const int32_t* pair_off, const int32_t* pair_rows, int P,
                     const int32_t* ref_info, const double* ref_dirs, const int32_t* ref_tab, const int32_t* row_const,
                     const int32_t* van_const, const double* cst, int C, const int32_t* tab_off, const double* knot_x,
                     const double* knot_y, int T, int N, double gamma, double diff, int device, void** out);
void mfx_rot2d_destroy(void* h);

/* B directions dirs [B x 3] -> out [B x M x N]; status [B x 4].  Failing directions' output is NaN. */
int mfx_rot2d_rotate(void* h, const double* dirs, int64_t B, double* out, int32_t* status);
int mfx_rot2d_rotate_dev(void* h, const double* d_dirs, int64_t B, double* d_out, int32_t* d_status, void* stream);

/* B (direction, atom) pairs: out[b, m] = rotate(dirs[b])[m, cols[b]] -> out [B x M]; status [B x 4] */
int mfx_rot2d_rotate_cols(void* h, const double* dirs, const int32_t* cols, int64_t B, double* out, int32_t* status);
int mfx_rot2d_rotate_cols_dev(void* h, const double* d_dirs, const int32_t* d_cols, int64_t B, double* d_out,
                              int32_t* d_status, void* stream);

#ifdef __cplusplus
}
#endif
#endif
