// rotate2d.hip -- rotate_atom_2Dprotocol for B fascicle directions (include/mfx_rot2d.h; reference
// mf_utils.py:1440-1690).
//
// The reference fascicle's side (its rotated scheme, S_par_ref, S_perp_ref, the per-pair unique perpendicular
// directions and opposite pairs, one sorted knot table per reference line) does not depend on the new direction;
// the Python layer computes it once with the reference's NumPy arithmetic and the handle keeps it in HBM.
//
// Two kernels per call:
//   mfx_rot2d_plan_kernel   one workgroup per direction: rotates the scheme onto it (rotate_scheme_mat), forms
//                           G_perp, G_par, S_par and the checks, then walks the (Delta, delta) pairs in the
//                           reference's order (unique directions by exact comparison, opposite pairs by
//                           numpy.isclose, vanished rows, the new lines, the reference line by first argmax, the
//                           interpolation bracket).  It writes one operation per (direction, row) and one status
//                           record per direction: the first failing check in the reference's order.
//   mfx_rot2d_eval_kernel   out[b, m, n] = S_par * (slope[h][n] * (x - x[h-1]) + y[h-1][n]) (SciPy's _call_linear,
//                           then S_par_new * S_perp_new), or S_par * const row, or S_par * 0 (the reference's
//                           zero-initialised S_perp_new).  Stores are coalesced over the atoms n.
// plus mfx_rot2d_cols_kernel, the one-atom-per-direction evaluation.
// The handle's device view, the plan records and the expression that turns a record into an entry live in rot2d_shared.h:
// fit2d.hip (the fit of 2-D protocols) launches the plan kernel through mfx_rot2d_plan_enqueue and evaluates the same function.
#include "rot2d_shared.h"

#include <cmath>
#include <vector>

namespace {

constexpr int R2_PLAN_WG = 256;
constexpr int R2_EVAL_WG = 256;
constexpr int R2_EVAL_ROWS = 8;

// numpy.isclose(a, b) with rtol 1e-5, atol 1e-8
__host__ __device__ inline bool r2_isclose(double a, double b) {
  return (fabs(a - b) <= 1e-08 + 1e-05 * fabs(b) && isfinite(b)) || a == b;
}

// np.unique(axis=0) order: x, then y (float comparison: -0.0 == 0.0)
__device__ inline bool r2_lex_less(double ax, double ay, double bx, double by) {
  return ax < bx || (ax == bx && ay < by);
}

__global__ __launch_bounds__(R2_PLAN_WG) void mfx_rot2d_plan_kernel(Rot2dDev D, const double* __restrict__ dirs,
                                                                    Rot2dPlan pl) {
  __shared__ double s_px[R2_MAX_ROWS], s_py[R2_MAX_ROWS];
  __shared__ double s_ux[5], s_uy[5];
  __shared__ int s_first[8];
  __shared__ int s_pi[2], s_pj[2];
  __shared__ int s_cnt, s_npair, s_flag, s_flag2;
  const int tid = threadIdx.x;
  const int64_t b = blockIdx.x;
  const int M = D.M;
  int* op = pl.op + b * M;
  double* xs = pl.x + b * M;
  double* sp = pl.spar + b * M;
  double* nn = pl.n2 + b * M;
  int st[4] = {MFX_ROT2D_OK, 0, 0, 0};

  // rotate_scheme_mat(sch_mat, [0, 0, 1], newdir)
  const double d0 = dirs[3 * b], d1 = dirs[3 * b + 1], d2 = dirs[3 * b + 2];
  const double nsq = (d0 * d0 + d1 * d1) + d2 * d2;
  if (!r2_isclose(nsq, 1.0)) {
    if (tid == 0) {
      pl.status[4 * b] = MFX_ROT2D_NEWDIR_NORM;
      pl.status[4 * b + 1] = pl.status[4 * b + 2] = pl.status[4 * b + 3] = 0;
    }
    return;
  }
  const double c0 = 0.0 * d2 - 1.0 * d1, c1 = 1.0 * d0 - 0.0 * d2, c2 = 0.0 * d1 - 0.0 * d0;
  const double csq = (c0 * c0 + c1 * c1) + c2 * c2;
  const bool rot = csq > 0.0;   // otherwise the reference returns the scheme itself
  double R[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
  if (rot) {
    const double cn = sqrt(csq);
    const double x = c0 / cn, y = c1 / cn, z = c2 / cn;
    const double ang = -acos(d2);   // vrrotvec2mat(axis, -arccos(z . newdir))
    const double s = sin(ang), c = cos(ang), t = 1.0 - c;
    R[0][0] = t * x * x + c; R[0][1] = t * x * y - s * z; R[0][2] = t * x * z + s * y;
    R[1][0] = t * x * y + s * z; R[1][1] = t * y * y + c; R[1][2] = t * y * z - s * x;
    R[2][0] = t * x * z - s * y; R[2][1] = t * y * z + s * x; R[2][2] = t * z * z + c;
  }
  if (tid == 0) { s_flag = 0; s_flag2 = 0; }
  __syncthreads();
  const double eps = 2.220446049250313e-16;
  // s_px / s_py are indexed by position in pair_rows (the order the pair loop walks)
  for (int i = tid; i < M; i += R2_PLAN_WG) {
    const int m = D.pair_rows[i];
    const double* s = D.sch + 6 * (size_t)m;
    double r0 = s[0], r1 = s[1], r2 = s[2];
    if (rot) {
      const double g0 = r0, g1 = r1, g2 = r2;
      r0 = (g0 * R[0][0] + g1 * R[0][1]) + g2 * R[0][2];
      r1 = (g0 * R[1][0] + g1 * R[1][1]) + g2 * R[1][2];
      r2 = (g0 * R[2][0] + g1 * R[2][1]) + g2 * R[2][2];
      if (fabs(r0) <= eps) r0 = 0.0;
      if (fabs(r1) <= eps) r1 = 0.0;
      if (fabs(r2) <= eps) r2 = 0.0;
      const double rn = sqrt((r0 * r0 + r1 * r1) + r2 * r2);
      if (rn > 0.0) { r0 = r0 / rn; r1 = r1 / rn; r2 = r2 / rn; }
    }
    const double n2 = sqrt(r0 * r0 + r1 * r1);
    double px = r0, py = r1;
    if (n2 > 0.0) { px = r0 / n2; py = r1 / n2; }
    s_px[i] = px;
    s_py[i] = py;
    const double G = s[3], Del = s[4], del = s[5];
    const double Gperp = G * n2, Gpar = fabs(r2) * G;
    if (!r2_isclose(G * G, Gperp * Gperp + Gpar * Gpar)) s_flag = 1;
    const double gd = (D.gamma * del) * Gpar;
    const double bpar = (gd * gd) * (Del - del / 3.0);
    const double spar = exp(-bpar * D.diff);
    if (G == 0.0 && !r2_isclose(spar, 1.0)) s_flag2 = 1;
    nn[m] = n2;
    xs[m] = 0.0;
    sp[m] = spar;
    op[m] = G == 0.0 ? -2 - D.row_const[m] : R2_OP_ZERO;
  }
  __syncthreads();
  if (s_flag) st[0] = MFX_ROT2D_CHK_NEW;
  else if (s_flag2) st[0] = MFX_ROT2D_CHK_PAR_NEW;

  for (int p = 0; p < D.P && st[0] == MFX_ROT2D_OK; ++p) {
    const int* ri = D.ref_info + 3 * p;
    if (ri[0] != MFX_ROT2D_OK) { st[0] = ri[0]; st[1] = p; st[2] = ri[1]; break; }
    const int r0 = D.pair_off[p], r1 = D.pair_off[p + 1];
    // unique perpendicular directions of the new side: row i is a first occurrence when no earlier row of the pair
    // has the same direction (exact comparison)
    __syncthreads();
    if (tid == 0) { s_cnt = 0; s_flag = 0; }
    __syncthreads();
    for (int i = r0 + tid; i < r1; i += R2_PLAN_WG) {
      const double x = s_px[i], y = s_py[i];
      bool first = true;
      for (int k = r0; k < i; ++k)
        if (s_px[k] == x && s_py[k] == y) { first = false; break; }
      if (first) {
        const int slot = atomicAdd(&s_cnt, 1);
        if (slot < 8) s_first[slot] = i;
      }
    }
    __syncthreads();
    const int nu = s_cnt;
    if (nu != 3 && nu != 5) { st[0] = MFX_ROT2D_NEW_UNIQUE; st[1] = p; st[2] = nu; break; }
    if (tid == 0) {
      // lexicographic order (the slots were filled in arbitrary order; the directions are distinct)
      double ux[5], uy[5];
      for (int k = 0; k < nu; ++k) {
        const int f = s_first[k];
        const double x = s_px[f], y = s_py[f];
        int q = k;
        while (q > 0 && r2_lex_less(x, y, ux[q - 1], uy[q - 1])) { ux[q] = ux[q - 1]; uy[q] = uy[q - 1]; --q; }
        ux[q] = x; uy[q] = y;
      }
      int np_ = 0;
      for (int i = 0; i < nu; ++i)
        for (int j = i + 1; j < nu; ++j)
          if (r2_isclose(ux[i] * ux[j] + uy[i] * uy[j], -1.0)) {
            if (np_ < 2) { s_pi[np_] = i; s_pj[np_] = j; }
            ++np_;
          }
      for (int k = 0; k < nu; ++k) { s_ux[k] = ux[k]; s_uy[k] = uy[k]; }
      s_npair = np_;
    }
    __syncthreads();
    const int npair = s_npair;
    if (npair != 1 && npair != 2) { st[0] = MFX_ROT2D_NEW_PAIRS; st[1] = p; st[2] = npair; break; }
    // rows whose perpendicular component vanished: the pair's b0 value
    for (int i = r0 + tid; i < r1; i += R2_PLAN_WG) {
      const int m = D.pair_rows[i];
      if (D.sch[6 * (size_t)m + 3] != 0.0 && !(nn[m] > 0.0)) s_flag = 1;
    }
    __syncthreads();
    if (s_flag) {
      const int vc = D.van_const[p];
      if (vc < 0) { st[0] = MFX_ROT2D_VANISHED; st[1] = p; break; }
      for (int i = r0 + tid; i < r1; i += R2_PLAN_WG) {
        const int m = D.pair_rows[i];
        if (D.sch[6 * (size_t)m + 3] != 0.0 && !(nn[m] > 0.0)) op[m] = -2 - vc;
      }
    }
    // the new lines, in order (a row on two lines keeps the later one, as the reference's assignments do)
    for (int l = 0; l < npair && st[0] == MFX_ROT2D_OK; ++l) {
      const double lx = s_ux[s_pi[l]], ly = s_uy[s_pi[l]], ox = s_ux[s_pj[l]], oy = s_uy[s_pj[l]];
      __syncthreads();
      if (tid == 0) s_flag2 = 0;
      __syncthreads();
      for (int i = r0 + tid; i < r1; i += R2_PLAN_WG) {
        const int m = D.pair_rows[i];
        const bool on = (s_px[i] == lx && s_py[i] == ly) || (s_px[i] == ox && s_py[i] == oy);
        if (on && D.sch[6 * (size_t)m + 3] == 0.0) s_flag2 = 1;
      }
      __syncthreads();
      if (s_flag2) { st[0] = MFX_ROT2D_INTERP_B0; st[1] = p; st[2] = l; st[3] = npair; break; }
      // reference direction closest to the line: first maximum of gdir_ref_un @ linedir_new
      const int nref = ri[2];
      const double* rd = D.ref_dirs + 10 * p;
      int best = 0;
      double bv = rd[0] * lx + rd[1] * ly;
      for (int k = 1; k < nref; ++k) {
        const double v = rd[2 * k] * lx + rd[2 * k + 1] * ly;
        if (v > bv) { bv = v; best = k; }
      }
      const int t = D.ref_tab[5 * p + best];
      if (t < 0) { st[0] = MFX_ROT2D_NO_REF_LINE; st[1] = p; st[2] = r1 - r0; st[3] = -1 - t; break; }
      const int k0 = D.tab_off[t], P = D.tab_off[t + 1] - k0;
      const double* kx = D.kx + k0;
      for (int i = r0 + tid; i < r1; i += R2_PLAN_WG) {
        const int m = D.pair_rows[i];
        const double px = s_px[i], py = s_py[i];
        if (!((px == lx && py == ly) || (px == ox && py == oy))) continue;
        const double dot = px * lx + py * ly;
        const double sg = dot > 0.0 ? 1.0 : (dot < 0.0 ? -1.0 : (dot == 0.0 ? 0.0 : dot));
        const double xv = (D.sch[6 * (size_t)m + 3] * nn[m]) * sg;
        // searchsorted(kx, xv, side='left') (NaN sorts last), clipped to [1, P-1]
        int lo = 0, hi = P;
        if (xv != xv) lo = P;
        while (lo < hi) {
          const int mid = (lo + hi) >> 1;
          if (kx[mid] < xv) lo = mid + 1;
          else hi = mid;
        }
        const int j = lo < 1 ? 1 : (lo > P - 1 ? P - 1 : lo);
        op[m] = k0 + j;
        xs[m] = xv;
      }
    }
  }
  if (tid == 0) {
    pl.status[4 * b] = st[0];
    pl.status[4 * b + 1] = st[1];
    pl.status[4 * b + 2] = st[2];
    pl.status[4 * b + 3] = st[3];
  }
}

// grid (direction, block of R2_EVAL_ROWS rows); the row's operation is wave-uniform, the atoms n run across lanes
// vec: N even and out 16-byte aligned (the tables are laid out 16-byte aligned by mfx_rot2d_create)
__global__ __launch_bounds__(R2_EVAL_WG) void mfx_rot2d_eval_kernel(Rot2dDev D, Rot2dPlan pl, double* __restrict__ out,
                                                                    int vec) {
  const int64_t b = blockIdx.x;
  const int M = D.M, N = D.N;
  const bool bad = pl.status[4 * b] != MFX_ROT2D_OK;
  for (int r = 0; r < R2_EVAL_ROWS; ++r) {
    const int m = blockIdx.y * R2_EVAL_ROWS + r;
    if (m >= M) break;
    const int64_t i = b * M + m;
    double* dst = out + i * N;
    if (bad) {
      for (int n = threadIdx.x; n < N; n += R2_EVAL_WG) dst[n] = __builtin_nan("");
      continue;
    }
    const int o = pl.op[i];
    const double x = pl.x[i], s = pl.spar[i];
    if (o >= 1) {
      const double xl = D.kx[o - 1];
      const double dx = x - xl;
      const double* sl = D.slope + (size_t)o * N;
      const double* yl = D.ky + (size_t)(o - 1) * N;
      if (vec) {
        for (int n = 2 * threadIdx.x; n < N; n += 2 * R2_EVAL_WG) {
          const double2 a = *reinterpret_cast<const double2*>(sl + n);
          const double2 y = *reinterpret_cast<const double2*>(yl + n);
          double2 v;
          v.x = r2_value(o, s, a.x, dx, y.x);
          v.y = r2_value(o, s, a.y, dx, y.y);
          *reinterpret_cast<double2*>(dst + n) = v;
        }
      } else {
        for (int n = threadIdx.x; n < N; n += R2_EVAL_WG) dst[n] = r2_value(o, s, sl[n], dx, yl[n]);
      }
    } else if (o == R2_OP_ZERO) {
      const double v = r2_value(o, s, 0.0, 0.0, 0.0);
      for (int n = threadIdx.x; n < N; n += R2_EVAL_WG) dst[n] = v;
    } else {
      const double* c = D.cst + (size_t)(-2 - o) * N;
      for (int n = threadIdx.x; n < N; n += R2_EVAL_WG) dst[n] = r2_value(o, s, 0.0, 0.0, c[n]);
    }
  }
}

// out[b, m] = rotated atom cols[b] of direction b; thread per (b, m)
__global__ __launch_bounds__(256) void mfx_rot2d_cols_kernel(Rot2dDev D, Rot2dPlan pl, const int* __restrict__ cols,
                                                             int64_t B, double* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B * D.M) return;
  const int64_t b = i / D.M;
  const int n = cols[b];
  if (pl.status[4 * b] != MFX_ROT2D_OK || n < 0 || n >= D.N) { out[i] = __builtin_nan(""); return; }
  const int o = pl.op[i];
  const double x = pl.x[i], s = pl.spar[i];
  out[i] = r2_elem(D, o, x, s, n);
}

int r2_launch(const mfx_rot2d* h, const double* d_dirs, const int* d_cols, int64_t B, double* d_out, int* d_status,
              hipStream_t st) {
  if (B > 0x7fffffff) return mfx_fail(MFX_ERR_UNSUPPORTED, "mfx_rot2d: more than 2^31 - 1 directions");
  PlanMem pm(st);
  if (int rc = pm.alloc(B, h->d.M, d_status)) return rc;
  if (int rc = mfx_rot2d_plan_enqueue(h, d_dirs, B, pm.pl, st)) return rc;
  if (d_cols) {
    const int64_t blocks = (B * h->d.M + 255) / 256;
    if (blocks > 0x7fffffff) return mfx_fail(MFX_ERR_UNSUPPORTED, "mfx_rot2d_rotate_cols: batch too large");
    hipLaunchKernelGGL(mfx_rot2d_cols_kernel, dim3((unsigned)blocks), dim3(256), 0, st, h->d, pm.pl, d_cols, B, d_out);
  } else {
    const dim3 grid((unsigned)B, (unsigned)((h->d.M + R2_EVAL_ROWS - 1) / R2_EVAL_ROWS));
    const int vec = (h->d.N % 2 == 0) && ((uintptr_t)d_out % 16 == 0);
    hipLaunchKernelGGL(mfx_rot2d_eval_kernel, grid, dim3(R2_EVAL_WG), 0, st, h->d, pm.pl, d_out, vec);
  }
  HIPCHK(hipGetLastError());
  return MFX_OK;
}

int r2_host(const mfx_rot2d* h, const double* dirs, const int32_t* cols, int64_t B, double* out, int32_t* status,
            const char* fn) {
  const size_t n_out = (size_t)B * h->d.M * (cols ? 1 : h->d.N);
  DevMem dd, dc, dout, dst;
  HIPCHK(dd.alloc(sizeof(double) * 3 * B));
  HIPCHK(dout.alloc(sizeof(double) * n_out));
  HIPCHK(dst.alloc(sizeof(int32_t) * 4 * B));
  HIPCHK(hipMemcpy(dd.p, dirs, sizeof(double) * 3 * B, hipMemcpyHostToDevice));
  if (cols) {
    HIPCHK(dc.alloc(sizeof(int32_t) * B));
    HIPCHK(hipMemcpy(dc.p, cols, sizeof(int32_t) * B, hipMemcpyHostToDevice));
  }
  if (int rc = r2_launch(h, dd.as<double>(), dc.as<int>(), B, dout.as<double>(), dst.as<int>(), nullptr)) return rc;
  hipError_t e = hipMemcpy(out, dout.p, sizeof(double) * n_out, hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(status, dst.p, sizeof(int32_t) * 4 * B, hipMemcpyDeviceToHost);
  if (e != hipSuccess) return mfx_fail(MFX_ERR_HIP, "%s: %s", fn, hipGetErrorString(e));
  return MFX_OK;
}

}  // namespace

static thread_local int64_t g_plan_dirs = 0;
void mfx_rot2d_plan_count_reset() { g_plan_dirs = 0; }
int64_t mfx_rot2d_plan_count() { return g_plan_dirs; }

int mfx_rot2d_plan_enqueue(const mfx_rot2d* h, const double* d_dirs, int64_t B, const Rot2dPlan& pl, hipStream_t st) {
  g_plan_dirs += B;
  hipLaunchKernelGGL(mfx_rot2d_plan_kernel, dim3((unsigned)B), dim3(R2_PLAN_WG), 0, st, h->d, d_dirs, pl);
  HIPCHK(hipGetLastError());
  return MFX_OK;
}

extern "C" int mfx_rot2d_abi_version(void) { return 1; }

extern "C" int mfx_rot2d_create(const double* sch, int M, const int32_t* pair_off, const int32_t* pair_rows, int P,
                                const int32_t* ref_info, const double* ref_dirs, const int32_t* ref_tab,
                                const int32_t* row_const, const int32_t* van_const, const double* cst, int C,
                                const int32_t* tab_off, const double* knot_x, const double* knot_y, int T, int N,
                                double gamma, double diff, int device, void** out) {
  const char* fn = "mfx_rot2d_create";
  if (!sch || !pair_off || !pair_rows || !ref_info || !ref_dirs || !ref_tab || !row_const || !van_const || !tab_off ||
      !out || (C > 0 && !cst) || (T > 0 && (!knot_x || !knot_y)))
    return mfx_fail(MFX_ERR_ARG, "%s: null argument", fn);
  if (M < 1 || P < 1 || N < 1 || C < 0 || T < 0) return mfx_fail(MFX_ERR_ARG, "%s: need M, P, N >= 1", fn);
  if (M > R2_MAX_ROWS) return mfx_fail(MFX_ERR_UNSUPPORTED, "%s: more than %d protocol rows", fn, R2_MAX_ROWS);
  // every index the kernels follow is checked here
  if (pair_off[0] != 0 || pair_off[P] != M) return mfx_fail(MFX_ERR_ARG, "%s: pair_off must run from 0 to M", fn);
  for (int p = 0; p < P; ++p) {
    if (pair_off[p + 1] < pair_off[p]) return mfx_fail(MFX_ERR_ARG, "%s: pair_off must not decrease", fn);
    if (ref_info[3 * p] == MFX_ROT2D_OK && (ref_info[3 * p + 2] < 1 || ref_info[3 * p + 2] > 5))
      return mfx_fail(MFX_ERR_ARG, "%s: pair %d: 1 to 5 reference directions", fn, p);
    for (int u = 0; u < 5; ++u)
      if (ref_tab[5 * p + u] >= T) return mfx_fail(MFX_ERR_ARG, "%s: pair %d: table index out of range", fn, p);
    if (van_const[p] < -1 || van_const[p] >= C) return mfx_fail(MFX_ERR_ARG, "%s: van_const out of range", fn);
  }
  std::vector<char> seen((size_t)M, 0);
  for (int i = 0; i < M; ++i) {
    const int m = pair_rows[i];
    if (m < 0 || m >= M || seen[(size_t)m]) return mfx_fail(MFX_ERR_ARG, "%s: pair_rows must be a permutation", fn);
    seen[(size_t)m] = 1;
    if (row_const[i] < -1 || row_const[i] >= C) return mfx_fail(MFX_ERR_ARG, "%s: row_const out of range", fn);
    if (sch[6 * (size_t)i + 3] == 0.0 && row_const[i] < 0)
      return mfx_fail(MFX_ERR_ARG, "%s: b0 row %d without a constant row", fn, i);
  }
  if (tab_off[0] != 0) return mfx_fail(MFX_ERR_ARG, "%s: tab_off must start at 0", fn);
  for (int t = 0; t < T; ++t)
    if (tab_off[t + 1] - tab_off[t] < 2) return mfx_fail(MFX_ERR_ARG, "%s: table %d has fewer than 2 knots", fn, t);
  const int K = tab_off[T];
  if (int rc = mfx_require_device(device)) return rc;
  // slopes of SciPy's _call_linear, per interval: (y_hi - y_lo) / (x_hi - x_lo)
  std::vector<double> slope((size_t)K * N, 0.0);
  for (int t = 0; t < T; ++t)
    for (int k = tab_off[t] + 1; k < tab_off[t + 1]; ++k) {
      const double dx = knot_x[k] - knot_x[k - 1];
      for (int n = 0; n < N; ++n)
        slope[(size_t)k * N + n] = (knot_y[(size_t)k * N + n] - knot_y[(size_t)(k - 1) * N + n]) / dx;
    }
  // one device block: doubles first, then the int32 arrays
  const size_t nd = (size_t)M * 6 + (size_t)P * 10 + (size_t)C * N + (size_t)K + 2 * (size_t)K * N + 8;
  const size_t ni = (size_t)(P + 1) + M + 3 * (size_t)P + 5 * (size_t)P + M + P + (size_t)(T + 1);
  std::vector<double> hd;
  hd.reserve(nd);
  std::vector<int32_t> hi;
  hi.reserve(ni);
  // every double array starts at an even offset (16-byte aligned for the eval kernel's double2 loads)
  auto put = [](auto& v, const auto* src, size_t n) {
    if (sizeof(*src) == 8 && v.size() % 2) v.push_back(0);
    v.insert(v.end(), src, src + n);
    return v.size() - n;
  };
  const size_t o_sch = put(hd, sch, (size_t)M * 6), o_rd = put(hd, ref_dirs, (size_t)P * 10);
  const size_t o_cst = C > 0 ? put(hd, cst, (size_t)C * N) : hd.size();
  const size_t o_kx = K > 0 ? put(hd, knot_x, K) : hd.size();
  const size_t o_ky = K > 0 ? put(hd, knot_y, (size_t)K * N) : hd.size();
  const size_t o_sl = put(hd, slope.data(), slope.size());
  const size_t o_po = put(hi, pair_off, P + 1), o_pr = put(hi, pair_rows, M), o_ri = put(hi, ref_info, 3 * (size_t)P);
  const size_t o_rt = put(hi, ref_tab, 5 * (size_t)P), o_rc = put(hi, row_const, M), o_vc = put(hi, van_const, P);
  const size_t o_to = put(hi, tab_off, T + 1);
  mfx_rot2d* h = new mfx_rot2d;
  h->device = device;
  const size_t bytes_d = sizeof(double) * (hd.size() + 2), bytes = bytes_d + sizeof(int32_t) * hi.size();
  if (hipMalloc(&h->mem, bytes) != hipSuccess) {
    delete h;
    return mfx_fail(MFX_ERR_HIP, "%s: hipMalloc of %zu bytes failed", fn, bytes);
  }
  double* dd = (double*)h->mem;
  int32_t* di = (int32_t*)((char*)h->mem + bytes_d);
  if (hipMemcpy(dd, hd.data(), sizeof(double) * hd.size(), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(di, hi.data(), sizeof(int32_t) * hi.size(), hipMemcpyHostToDevice) != hipSuccess) {
    (void)hipFree(h->mem);
    delete h;
    return mfx_fail(MFX_ERR_HIP, "%s: upload failed", fn);
  }
  Rot2dDev& d = h->d;
  d.M = M; d.P = P; d.N = N; d.C = C; d.T = T; d.K = K;
  d.sch = dd + o_sch; d.ref_dirs = dd + o_rd; d.cst = dd + o_cst; d.kx = dd + o_kx; d.ky = dd + o_ky; d.slope = dd + o_sl;
  d.pair_off = di + o_po; d.pair_rows = di + o_pr; d.ref_info = di + o_ri; d.ref_tab = di + o_rt;
  d.row_const = di + o_rc; d.van_const = di + o_vc; d.tab_off = di + o_to;
  d.gamma = gamma; d.diff = diff;
  *out = h;
  return MFX_OK;
}

extern "C" void mfx_rot2d_destroy(void* hv) {
  mfx_rot2d* h = (mfx_rot2d*)hv;
  if (!h) return;
  if (h->mem) {
    (void)hipSetDevice(h->device);
    (void)hipFree(h->mem);
  }
  delete h;
}

extern "C" int mfx_rot2d_rotate_dev(void* hv, const double* d_dirs, int64_t B, double* d_out, int32_t* d_status,
                                    void* stream) {
  if (mfx_device_count() <= 0) return mfx_no_device();
  const mfx_rot2d* h = (const mfx_rot2d*)hv;
  if (!h || B < 0 || (B > 0 && (!d_dirs || !d_out || !d_status))) return mfx_fail(MFX_ERR_ARG, "mfx_rot2d_rotate_dev: bad argument");
  if (B == 0) return MFX_OK;
  if (int rc = mfx_require_device(h->device)) return rc;
  return r2_launch(h, d_dirs, nullptr, B, d_out, d_status, (hipStream_t)stream);
}

extern "C" int mfx_rot2d_rotate(void* hv, const double* dirs, int64_t B, double* out, int32_t* status) {
  if (mfx_device_count() <= 0) return mfx_no_device();
  const mfx_rot2d* h = (const mfx_rot2d*)hv;
  if (!h || B < 0 || (B > 0 && (!dirs || !out || !status))) return mfx_fail(MFX_ERR_ARG, "mfx_rot2d_rotate: bad argument");
  if (B == 0) return MFX_OK;
  if (int rc = mfx_require_device(h->device)) return rc;
  return r2_host(h, dirs, nullptr, B, out, status, "mfx_rot2d_rotate");
}

extern "C" int mfx_rot2d_rotate_cols_dev(void* hv, const double* d_dirs, const int32_t* d_cols, int64_t B, double* d_out,
                                         int32_t* d_status, void* stream) {
  if (mfx_device_count() <= 0) return mfx_no_device();
  const mfx_rot2d* h = (const mfx_rot2d*)hv;
  if (!h || B < 0 || (B > 0 && (!d_dirs || !d_cols || !d_out || !d_status)))
    return mfx_fail(MFX_ERR_ARG, "mfx_rot2d_rotate_cols_dev: bad argument");
  if (B == 0) return MFX_OK;
  if (int rc = mfx_require_device(h->device)) return rc;
  return r2_launch(h, d_dirs, d_cols, B, d_out, d_status, (hipStream_t)stream);
}

extern "C" int mfx_rot2d_rotate_cols(void* hv, const double* dirs, const int32_t* cols, int64_t B, double* out,
                                     int32_t* status) {
  if (mfx_device_count() <= 0) return mfx_no_device();
  const mfx_rot2d* h = (const mfx_rot2d*)hv;
  if (!h || B < 0 || (B > 0 && (!dirs || !cols || !out || !status)))
    return mfx_fail(MFX_ERR_ARG, "mfx_rot2d_rotate_cols: bad argument");
  if (B == 0) return MFX_OK;
  for (int64_t b = 0; b < B; ++b)
    if (cols[b] < 0 || cols[b] >= h->d.N) return mfx_fail(MFX_ERR_ARG, "mfx_rot2d_rotate_cols: atom index %d out of range", cols[b]);
  if (int rc = mfx_require_device(h->device)) return rc;
  return r2_host(h, dirs, cols, B, out, status, "mfx_rot2d_rotate_cols");
}
