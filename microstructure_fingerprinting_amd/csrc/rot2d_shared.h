// rot2d_shared.h -- what rotate2d.hip (the 2-D protocol rotation) and fit2d.hip (the fit that starts from it) share:
// the device view of a mfx_rot2d handle, the plan records of a batch of directions, and the ONE expression that turns
// a plan record into a dictionary entry, so that the fit sees bit for bit the columns mfx_rot2d_rotate returns.
#pragma once
#include "mfx_host.h"
#include "../../include/mfx_rot2d.h"

constexpr int R2_MAX_ROWS = 4000;   // perpendicular directions of every row in LDS: 2 x 4000 doubles
constexpr int R2_OP_ZERO = -1;      // op >= 1: interpolate on knot interval [op-1, op]; op <= -2: constant row -2 - op

struct Rot2dDev {
  int M, P, N, C, T, K;
  const double* sch;      // [M x 6]
  const int* pair_off;    // [P + 1]
  const int* pair_rows;   // [M]
  const int* ref_info;    // [P x 3]
  const double* ref_dirs; // [P x 5 x 2]
  const int* ref_tab;     // [P x 5]
  const int* row_const;   // [M]
  const int* van_const;   // [P]
  const double* cst;      // [C x N]
  const int* tab_off;     // [T + 1]
  const double* kx;       // [K]
  const double* ky;       // [K x N]
  const double* slope;    // [K x N], row k: interval [k-1, k] (unused for a table's first knot)
  double gamma, diff;
};

struct Rot2dPlan {
  int* op;        // [B x M]
  double* x;      // [B x M] abscissa of interpolated rows
  double* spar;   // [B x M] S_par_new
  double* n2;     // [B x M] |g_perp| of the new side (before its normalisation)
  int* status;    // [B x 4]
};

struct mfx_rot2d {
  int device = 0;
  Rot2dDev d{};
  void* mem = nullptr;
};

// One entry from its operands: SciPy's _call_linear then S_par_new * S_perp_new (op >= 1; a = slope, y = the knot's
// value, dx = x - kx[op-1]), S_par * 0 (the reference's zero-initialised S_perp_new), or S_par * the constant row's y.
__device__ __forceinline__ double r2_value(int o, double s, double a, double dx, double y) {
  return o >= 1 ? s * (a * dx + y) : (o == R2_OP_ZERO ? s * 0.0 : s * y);
}
// the operands of atom n on a row with operation o (0 where r2_value does not read them)
__device__ __forceinline__ void r2_operands(const Rot2dDev& D, int o, int n, double& a, double& y) {
  a = o >= 1 ? D.slope[(size_t)o * D.N + n] : 0.0;
  y = o >= 1 ? D.ky[(size_t)(o - 1) * D.N + n] : (o == R2_OP_ZERO ? 0.0 : D.cst[(size_t)(-2 - o) * D.N + n]);
}
// entry (row with plan record {o, x, s}, atom n)
__device__ __forceinline__ double r2_elem(const Rot2dDev& D, int o, double x, double s, int n) {
  double a, y;
  r2_operands(D, o, n, a, y);
  return r2_value(o, s, a, o >= 1 ? x - D.kx[o - 1] : 0.0, y);
}

// plan scratch of B directions, on the caller's stream
struct PlanMem {
  StreamMem mem;
  Rot2dPlan pl{};
  explicit PlanMem(hipStream_t s) : mem(s) {}
  int alloc(int64_t B, int M, int* d_status) {
    const size_t n = (size_t)B * M;
    HIPCHK(mem.alloc(n * (sizeof(int) + 3 * sizeof(double)) + 64));
    char* p = mem.as<char>();
    pl.x = (double*)p;
    pl.spar = (double*)(p + n * sizeof(double));
    pl.n2 = (double*)(p + 2 * n * sizeof(double));
    pl.op = (int*)(p + 3 * n * sizeof(double));
    pl.status = d_status;
    return MFX_OK;
  }
};

// rotate2d.hip: enqueue mfx_rot2d_plan_kernel over B directions (records and status into pl)
int mfx_rot2d_plan_enqueue(const mfx_rot2d* h, const double* d_dirs, int64_t B, const Rot2dPlan& pl, hipStream_t st);
// directions handed to mfx_rot2d_plan_kernel by the calling thread since the last reset (robust2d.hip's diagnostic)
void mfx_rot2d_plan_count_reset();
int64_t mfx_rot2d_plan_count();

// ---- on prepared directions (F2Dirs of fit2d_shared.h): d_rec the F2Rec records [V KR x M] (void*: the type lives in every
// translation unit's own namespace), d_pstat [V KR x 4] the directions' status records.  They only enqueue.
// predict2d.hip: the prediction kernel; fascicle k of a parameter row (maxfasc layout) reads slot k of the voxel's KR
int mfx_predict2d_launch(const mfx_rot2d* h, const void* d_rec, const int* d_pstat, int KR, const double* d_params, int maxfasc,
                         int csf_on, const double* d_sig_csf, int64_t V, const double* d_Y, const double* d_sigma, int sigma_mode,
                         int ncoils, uint64_t seed, uint64_t offset, double* d_out, double* d_stats, int32_t* d_status,
                         int32_t* d_dir_status, hipStream_t st);
// fit2d.hip / w2d.hip: one fit class (every voxel K fascicles, the CSF column d_xc or null) into rows of the (maxfasc, csf_on)
// layout, as mfx_fit2d_batch* / mfx_wfit2d_batch* run it for the class
int mfx_fit2d_class_prepared(const mfx_rot2d* h, const double* d_Y, const void* d_rec, const int* d_pstat, int K, const double* d_xc,
                             int maxfasc, int csf_on, int64_t V, double* d_params, int32_t* d_vstat, hipStream_t st);
int mfx_wfit2d_class_prepared(const mfx_rot2d* h, const double* d_Y, const double* d_W, int64_t wstride, const void* d_rec,
                              const int* d_pstat, int K, const double* d_xc, int maxfasc, int csf_on, int64_t V, double* d_params,
                              int32_t* d_vstat, int32_t* d_wstat, hipStream_t st);
