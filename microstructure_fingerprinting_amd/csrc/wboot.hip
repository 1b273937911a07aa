// wboot.hip -- the bootstrap conditional on a fit's measurement weights (include/mfx_wboot.h): the own weighted fit
// (fit_w.hip's class launcher), its prediction (mfx_predict_dev), the resampling rule of mfx_wboot.h, the REPLICATE
// WEIGHTED FIT, and the value table and statistics of boot.hip through their public entry points.  The host side of a
// mixed batch, the per-class arguments and the front and tail of the class loop are boot_shared.h's, as in boot.hip.
//
// wboot_table_kernel     kind 1, once per weight row (one workgroup per voxel, or one for a shared vector): boot.hip's
//                        group table over the rows with W > 0 only - for every such row m the place of its group's list
//                        (start[m]), the group's positive rows (cnt[m]) and the list itself (rows), ascending.
// mfx_wboot_resample_kernel<KIND>  One wave per (voxel, replicate) row, 4 rows per workgroup, as boot.hip's.  Pass 1
//                        looks at the weights, y and p (status, M+; integer sums over the wave), the scale a is formed
//                        on the device (M+ differs between voxels); pass 2 is the rule line by line, one rounding each.
// The replicate fit (wb_rows).  Two fascicles without a CSF column, up to mfx_wfit_max_atoms(plan, 2) atoms: the shared
// path - wfit_kernels.h's two-fascicle kernel as W_GRAM once per voxel (the accumulator tiles of the cross-Gram to
// scratch G) and as W_REP once per (voxel, replicate), WB_R = 1 replicate per workgroup and pass over G.  Every other
// class, and everything under mfx_wboot_debug_set_force_plain(1): weight rows and directions copied to the replicate
// rows of a voxel chunk (a shared vector stays shared), fit_w.hip's class launcher on them untouched.
#include "wfit_kernels.h"
#include "boot_shared.h"
#include "sos_shared.h"
#include "../../include/mfx_wboot.h"
#include "../../include/mfx_predict.h"
#include "../../include/mfx_wfit.h"

#include <algorithm>
#include <cstring>
#include <vector>

namespace {

thread_local int g_force_plain = 0;

constexpr int WB_R = 1;                  // replicates per workgroup of the shared path
constexpr int WB_MAX_ROWS = 8192;
constexpr int WB_MAXF = 3;
constexpr double WB_DBL_MAX = 1.79769313486231570815e308;

unsigned wb_grid(int64_t n) { return (unsigned)((n + 255) / 256); }

// per weight row: start, cnt, rows [M] ints each (3 M ints a row), over the rows with W > 0
__global__ __launch_bounds__(256) void wboot_table_kernel(const int* __restrict__ groups, const double* __restrict__ W, int64_t wstride,
                                                         int M, int* __restrict__ tab) {
  const double* __restrict__ w = W + (size_t)blockIdx.x * wstride;
  int* start = tab + (size_t)blockIdx.x * 3 * M;
  int* cnt = start + M;
  int* rows = cnt + M;
  for (int m = threadIdx.x; m < M; m += 256) {
    const int g = groups[m];
    int less = 0, eq = 0, before = 0;
    for (int j = 0; j < M; ++j) {
      const int gj = groups[j];
      const bool pj = w[j] > 0.0;
      less += pj && gj < g;
      eq += pj && gj == g;
      before += pj && gj == g && j < m;
    }
    const bool pm = w[m] > 0.0;
    start[m] = pm ? less : 0;
    cnt[m] = pm ? eq : 0;
    if (pm) rows[less + before] = m;   // less + before < the number of positive rows <= M
  }
}

struct WBootRsArgs {
  const double* Y;        // [V x M]
  const double* P;        // [V x M]
  const double* W;        // [V x M] or [M]
  int64_t wstride;        // M or 0
  const double* params;   // [V x np]
  const double* peaks;    // [V x 3 F] or null
  const int* tab;         // [V or 1][3 M] (kind 1)
  const int64_t* vox;     // [V] or null
  double* Ys;             // [V x B x M]
  double* pk_out;         // [V B x 3 F] or null
  int* status;            // [V]
  int64_t V;
  unsigned long long seed, offset;
  double fill;            // the rows of a voxel in a non-zero status
  int M, B, np, F, csf_on, inflate;
};

__device__ __forceinline__ int wb_wave_sum_int(int x) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
  return x;
}

template <int KIND>
__global__ __launch_bounds__(256) void mfx_wboot_resample_kernel(WBootRsArgs a) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int M = a.M, B = a.B, F = a.F;
  const uint32_t k0 = (uint32_t)a.seed, k1 = (uint32_t)(a.seed >> 32);
  const int64_t row = (int64_t)blockIdx.x * 4 + wave;
  if (row < a.V * B) {
    const int64_t v = row / B;
    const int b = (int)(row - v * B);
    const double* __restrict__ pr = a.params + v * a.np;
    int n_act = 0;
    for (int k = 0; k < F; ++k) n_act += pr[1 + k] > 0.0;
    if (a.csf_on) n_act += pr[1 + 2 * F] > 0.0;
    const double* __restrict__ y = a.Y + v * M;
    const double* __restrict__ p = a.P + v * M;
    const double* __restrict__ w = a.W + v * a.wstride;
    double* __restrict__ o = a.Ys + row * M;
    // ---- pass 1: the status and M+
    bool badw = false, bad = false;
    int npos = 0;
    for (int m = lane; m < M; m += 64) {
      const double wm = w[m];
      badw |= !(wm >= 0.0) || !(wm <= WB_DBL_MAX);
      npos += wm > 0.0;
      bad |= !(fabs(y[m]) <= WB_DBL_MAX) || !(fabs(p[m]) <= WB_DBL_MAX);
    }
    badw = __ballot(badw) != 0ull;
    bad = __ballot(bad) != 0ull;
    const int Mp = wb_wave_sum_int(npos);
    const int st = badw ? 3 : (Mp == 0 ? 4 : (bad ? 2 : (Mp <= n_act ? 1 : 0)));
    if (st) {
      for (int m = lane; m < M; m += 64) o[m] = a.fill;
    } else {
      double sc = 1.0;
      if (a.inflate) {   // Mp > n_act here; the division, then the square root
        const double q = (double)Mp / (double)(Mp - n_act);
        sc = sqrt(q);
      }
      const int* __restrict__ gstart = a.tab + (a.wstride ? v * 3 * M : 0);
      const int* __restrict__ gcnt = gstart + M;
      const int* __restrict__ grows = gcnt + M;
      const unsigned long long base = a.offset + (unsigned long long)(a.vox ? a.vox[v] : v) * (unsigned long long)M;
      // ---- pass 2: the rule
      for (int m = lane; m < M; m += 64) {
        const double ym = y[m], pm = p[m], wm = w[m];
        const unsigned long long idx = base + (unsigned long long)m;
        uint32_t c[4] = {(uint32_t)idx, (uint32_t)(idx >> 32), (uint32_t)b, MFX_BOOT_STREAM};
        philox4x32_10(c, k0, k1);
        double out = ym;   // W_m = 0: as measured
        if (wm > 0.0) {
          if (KIND == MFX_BOOT_WILD) {
            const double r = ym - pm;
            const double ar = sc * r;
            const double t = (c[0] & 1u) ? -ar : ar;
            out = pm + t;
          } else {
            const int j = grows[gstart[m] + (int)mulhi32(c[0], (uint32_t)gcnt[m])];   // mulhi32(u, n) < n: inside the group's list
            const double sj = sqrt(w[j]), sm = sqrt(wm);
            const double r = y[j] - p[j];
            const double e = sj * r;
            const double ae = sc * e;
            const double d = ae / sm;
            out = pm + d;
          }
        }
        o[m] = out;
      }
    }
    if (a.pk_out)
      for (int i = lane; i < 3 * F; i += 64) a.pk_out[row * (3 * F) + i] = a.peaks[v * (3 * F) + i];
    if (b == 0 && lane == 0) a.status[v] = st;
  }
}

// the voxel's status = that of its first replicate row
__global__ void wboot_first_row_kernel(const int* __restrict__ rows, int64_t V, int B, int* __restrict__ vstat) {
  const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (v < V) vstat[v] = rows[v * B];
}
// NaN rows for the replicates of a voxel with unusable weights (the shared path's kernels skip it)
__global__ void wboot_nan_rows_kernel(const int* __restrict__ vstat, int64_t V, int64_t per_vox, double* __restrict__ params) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= V * per_vox) return;
  if (vstat[i / per_vox] != 0) params[i] = __builtin_nan("");
}

int wb_check_rule(const char* fn, int M, int F, int B, int kind) {
  if (M < 1) return mfx_fail(MFX_ERR_ARG, "%s: M should be positive, got %d", fn, M);
  if (M > WB_MAX_ROWS) return mfx_fail(MFX_ERR_UNSUPPORTED, "%s: more than %d measurements (got %d)", fn, WB_MAX_ROWS, M);
  if (F < 0) return mfx_fail(MFX_ERR_ARG, "%s: maxfasc should not be negative, got %d", fn, F);
  if (F > WB_MAXF) return mfx_fail(MFX_ERR_UNSUPPORTED, "%s: at most 3 fascicles (got %d)", fn, F);
  if (B < 1) return mfx_fail(MFX_ERR_ARG, "%s: B should be at least 1, got %d", fn, B);
  if (kind != MFX_BOOT_WILD && kind != MFX_BOOT_RESIDUAL)
    return mfx_fail(MFX_ERR_ARG, "%s: kind should be 0 (wild) or 1 (residual within groups), got %d", fn, kind);
  return MFX_OK;
}

int wb_check_fit(const char* fn, const mfx_plan* p, int64_t w_stride, int F, int csf_on, const void* sig_csf, int B, int kind,
                 const void* groups, int nprop, const void* props, int Q, const void* q) {
  if (!p) return mfx_fail(MFX_ERR_ARG, "%s: bad argument", fn);
  TablesDev T;
  PlanDev P;
  int device = 0;
  mfx_plan_view(p, &T, &P, &device);
  if (int rc = wb_check_rule(fn, P.M, F, B, kind)) return rc;
  if (B > MFX_BOOT_MAX_B)
    return mfx_fail(MFX_ERR_UNSUPPORTED, "%s: at most %d replicates are reduced on the device (got B = %d)", fn, MFX_BOOT_MAX_B, B);
  if (Q < 0) return mfx_fail(MFX_ERR_ARG, "%s: Q should not be negative, got %d", fn, Q);
  if (Q > MFX_BOOT_MAX_Q) return mfx_fail(MFX_ERR_UNSUPPORTED, "%s: at most %d quantiles (got %d)", fn, MFX_BOOT_MAX_Q, Q);
  if (w_stride != 0 && w_stride != P.M)
    return mfx_fail(MFX_ERR_ARG, "%s: w_stride should be M = %d or 0 (got %lld)", fn, P.M, (long long)w_stride);
  if (kind == MFX_BOOT_RESIDUAL && !groups) return mfx_fail(MFX_ERR_ARG, "%s: kind 1 needs groups", fn);
  if (nprop < 0 || (nprop > 0 && !props) || (Q > 0 && !q)) return mfx_fail(MFX_ERR_ARG, "%s: bad argument", fn);
  if (csf_on && !sig_csf) return mfx_fail(MFX_ERR_ARG, "%s: csf_on without sig_csf", fn);
  return MFX_OK;
}

// the resampling of V voxels; tab: scratch of 3 M ints per weight row (kind 1), filled here
int wb_launch_resample(int M, const double* d_Y, const double* d_P, const double* d_W, int64_t wstride, const double* d_params, int F,
                       int csf_on, const double* d_peaks, const int32_t* d_groups, int* d_tab, const int64_t* d_vox, int64_t V, int B,
                       int kind, int inflate, uint64_t seed, uint64_t offset, double fill, double* d_Ystar, double* d_peaks_out,
                       int32_t* d_status, hipStream_t st) {
  if ((V * B + 3) / 4 > 0x7fffffff || V > 0x7fffffff) return mfx_fail(MFX_ERR_ARG, "mfx_wboot: V B too large for one launch");
  if (kind == MFX_BOOT_RESIDUAL) {
    hipLaunchKernelGGL(wboot_table_kernel, dim3((unsigned)(wstride ? V : 1)), dim3(256), 0, st, d_groups, d_W, wstride, M, d_tab);
    HIPCHK(hipGetLastError());
  }
  WBootRsArgs a{};
  a.Y = d_Y; a.P = d_P; a.W = d_W; a.wstride = wstride; a.params = d_params; a.peaks = d_peaks; a.tab = d_tab; a.vox = d_vox;
  a.Ys = d_Ystar; a.pk_out = (d_peaks && F > 0) ? d_peaks_out : nullptr; a.status = d_status;
  a.V = V; a.seed = seed; a.offset = offset; a.fill = fill;
  a.M = M; a.B = B; a.np = boot_np(F, csf_on, 0); a.F = F; a.csf_on = csf_on; a.inflate = inflate;
  const unsigned grid = (unsigned)((V * B + 3) / 4);
  if (kind == MFX_BOOT_WILD) hipLaunchKernelGGL(mfx_wboot_resample_kernel<MFX_BOOT_WILD>, dim3(grid), dim3(256), 0, st, a);
  else hipLaunchKernelGGL(mfx_wboot_resample_kernel<MFX_BOOT_RESIDUAL>, dim3(grid), dim3(256), 0, st, a);
  HIPCHK(hipGetLastError());
  return MFX_OK;
}
inline size_t wb_tab_bytes(int kind, int M, int64_t wstride, int64_t V) {
  return kind == MFX_BOOT_RESIDUAL ? sizeof(int) * 3 * (size_t)M * (size_t)(wstride ? V : 1) : 0;
}

bool wb_shared_serves(const WArgs& a, int K, bool has_csf) {
  if (g_force_plain || has_csf || K != 2) return false;
  return a.T.N <= w_max_atoms_k2(a.P.M, a.P.any_bracket != 0);
}

// scratch bytes of the replicate fit per voxel (what the chunks of the bootstrap count beside the signals)
int64_t wb_rows_bytes(const WArgs& a, int K, bool has_csf, int64_t wstride, int B) {
  if (K == 0 && !has_csf) return 0;
  if (wb_shared_serves(a, K, has_csf)) return (int64_t)(sizeof(double) * w_gram_doubles(a.T.ldn));
  return (int64_t)B * ((wstride ? a.P.M : 0) * 8 + 3 * K * 8 + 8);
}

// The replicate fit of one class: V voxels of K fascicles (d_peaks [V x 3 K]), the CSF column d_xc or none, B signals
// each on the voxel's weights -> d_params [V x B x np] (np = 1 + 2 K + csf + 2), d_vstat [V] (mfx_wfit.h's status of the
// voxel's weights).  Only enqueues.
int wb_rows(const mfx_plan* p, const double* d_Ys, const double* d_W, int64_t wstride, const double* d_peaks, int K, const double* d_xc,
            int64_t V, int B, double* d_params, int32_t* d_vstat, int64_t budget, hipStream_t st) {
  WArgs a{};
  int device = 0;
  mfx_plan_view(p, &a.T, &a.P, &device);
  const int M = a.P.M, has_csf = d_xc != nullptr;
  const bool br = a.P.any_bracket != 0;
  const int np = boot_np(K, has_csf, 0);
  if (V > 0x7fffffff / B) return mfx_fail(MFX_ERR_UNSUPPORTED, "mfx_wboot: more than 2^31 replicate rows in one call");
  if (budget <= 0) budget = BOOT_DEFAULT_BYTES;
  const int64_t per_vox = std::max<int64_t>(1, wb_rows_bytes(a, K, has_csf, wstride, B));

  if (wb_shared_serves(a, K, has_csf)) {
    HIPCHK(hipMemsetAsync(d_params, 0, sizeof(double) * (size_t)V * B * np, st));
    StreamMem ok(st), sG(st);
    HIPCHK(ok.alloc(sizeof(int) * (size_t)V));
    hipLaunchKernelGGL(wfit_status_kernel, dim3(wb_grid(V)), dim3(256), 0, st, d_W, wstride, M, V, d_vstat, ok.as<int>(), (double*)nullptr, 0);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(wboot_nan_rows_kernel, dim3(wb_grid(V * B * np)), dim3(256), 0, st, d_vstat, V, (int64_t)B * np, d_params);
    HIPCHK(hipGetLastError());
    const int64_t Vc = std::max<int64_t>(1, std::min<int64_t>(V, budget / per_vox));
    const size_t gld = w_gram_doubles(a.T.ldn);
    HIPCHK(sG.alloc(sizeof(double) * gld * (size_t)Vc));
    const int MP = (M + W_MC - 1) & ~(W_MC - 1);
    const size_t lds = w_lds_bytes(a.T.ldn, MP, br);
    a.W = d_W; a.wstride = wstride; a.peaks_ld = 3 * K; a.num_params = np; a.maxfasc = K; a.G = sG.as<double>(); a.G_ld = gld; a.B = B;
    const void* kg = br ? (const void*)(mfx_wfit_k2_kernel<true, W_GRAM>) : (const void*)(mfx_wfit_k2_kernel<false, W_GRAM>);
    const void* kr = br ? (const void*)(mfx_wfit_k2_kernel<true, W_REP>) : (const void*)(mfx_wfit_k2_kernel<false, W_REP>);
    HIPCHK(hipFuncSetAttribute(kg, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    HIPCHK(hipFuncSetAttribute(kr, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    for (int64_t v0 = 0; v0 < V; v0 += Vc) {
      const int64_t nv = std::min(Vc, V - v0);
      a.Y = d_Ys + (size_t)v0 * B * M;
      a.W = d_W + (size_t)v0 * wstride;
      a.peaks = d_peaks + (size_t)v0 * 3 * K;
      a.vstat = d_vstat + v0;
      a.params = d_params + (size_t)v0 * B * np;
      if (br) {
        hipLaunchKernelGGL((mfx_wfit_k2_kernel<true, W_GRAM>), dim3((unsigned)nv), dim3(W_WG), lds, st, a);
        hipLaunchKernelGGL((mfx_wfit_k2_kernel<true, W_REP>), dim3((unsigned)(nv * B)), dim3(W_WG), lds, st, a);
      } else {
        hipLaunchKernelGGL((mfx_wfit_k2_kernel<false, W_GRAM>), dim3((unsigned)nv), dim3(W_WG), lds, st, a);
        hipLaunchKernelGGL((mfx_wfit_k2_kernel<false, W_REP>), dim3((unsigned)(nv * B)), dim3(W_WG), lds, st, a);
      }
      HIPCHK(hipGetLastError());
    }
    return MFX_OK;
  }

  // the plain path: weight rows and directions copied to the replicate rows of a voxel chunk, fit_w.hip's class launcher
  const int64_t Vc = std::max<int64_t>(1, std::min<int64_t>(V, budget / per_vox));
  StreamMem pk(st), wr(st), vrow(st);
  HIPCHK(pk.alloc(sizeof(double) * (size_t)Vc * B * 3 * std::max(K, 1)));
  if (wstride) HIPCHK(wr.alloc(sizeof(double) * (size_t)Vc * B * M));
  HIPCHK(vrow.alloc(sizeof(int) * (size_t)Vc * B));
  ScratchMark mark;
  const bool marked = mfx_scratch_mark(st, &mark);
  for (int64_t v0 = 0; v0 < V; v0 += Vc) {
    const int64_t nv = std::min(Vc, V - v0);
    if (K > 0) {
      hipLaunchKernelGGL(boot_expand_kernel, dim3(wb_grid(nv * B * 3 * K)), dim3(256), 0, st, d_peaks + (size_t)v0 * 3 * K, nv, B, 3 * K,
                         pk.as<double>());
      HIPCHK(hipGetLastError());
    }
    if (wstride) {
      hipLaunchKernelGGL(boot_expand_kernel, dim3(wb_grid(nv * B * M)), dim3(256), 0, st, d_W + (size_t)v0 * M, nv, B, M, wr.as<double>());
      HIPCHK(hipGetLastError());
    }
    if (int rc = mfx_wfit_class_dev(p, d_Ys + (size_t)v0 * B * M, wstride ? wr.as<double>() : d_W, wstride, pk.as<double>(), K, d_xc, K,
                                    has_csf, nv * B, d_params + (size_t)v0 * B * np, vrow.as<int32_t>(), st)) return rc;
    hipLaunchKernelGGL(wboot_first_row_kernel, dim3(wb_grid(nv)), dim3(256), 0, st, vrow.as<int>(), nv, B, d_vstat + v0);
    HIPCHK(hipGetLastError());
    if (marked) mfx_scratch_rewind(st, mark);
  }
  return MFX_OK;
}

// One class on device buffers (what mfx_wboot_fit_dev does after its checks; mfx_wboot_fit runs it per class chunk)
int wb_class_dev(const mfx_plan* p, const BootClass& r) {
  WArgs wa{};
  int device = 0;
  mfx_plan_view(p, &wa.T, &wa.P, &device);
  const int M = wa.P.M, N = wa.T.N, F = r.F, B = r.B;
  const double* xc = r.csf_on ? r.sig_csf : nullptr;
  hipStream_t st = r.st;
  BootChunkMem mem(r, M);
  StreamMem wst(st), tab(st);
  if (int rc = mem.alloc((int64_t)B * M * (int64_t)sizeof(double) + wb_rows_bytes(wa, F, r.csf_on != 0, r.wstride, B))) return rc;
  const int64_t Vc = mem.Vc;
  HIPCHK(wst.alloc(sizeof(int) * (size_t)Vc));   // mfx_wfit.h's status of the weights (the bootstrap's own says more)
  if (r.kind == MFX_BOOT_RESIDUAL) HIPCHK(tab.alloc(wb_tab_bytes(r.kind, M, r.wstride, Vc)));
  ScratchMark mark;
  const bool marked = mfx_scratch_mark(st, &mark);
  for (int64_t v0 = 0; v0 < r.V; v0 += Vc) {
    const int64_t nv = std::min(Vc, r.V - v0);
    const double* y = r.Y + (size_t)v0 * M;
    const double* w = r.W + (size_t)v0 * r.wstride;
    const double* pks = F > 0 ? r.peaks + (size_t)v0 * 3 * F : nullptr;
    const double* p0 = mem.p0(v0);
    if (!r.params0)
      if (int rc = mfx_wfit_class_dev(p, y, w, r.wstride, pks, F, xc, F, r.csf_on, nv, mem.par0.as<double>(), wst.as<int32_t>(), st)) return rc;
    if (!r.pred0)
      if (int rc = mfx_predict_dev(p, p0, pks, F, r.csf_on, 0, xc, nullptr, 0, nv, nullptr, nullptr, 0, 0, 0, 0, mem.pred.as<double>(),
                                   nullptr, mem.pst.as<int32_t>(), st)) return rc;
    // (zero rows for a voxel in a non-zero status: the fit never sees a NaN made here; the gather turns its rows into NaN)
    if (int rc = wb_launch_resample(M, y, mem.pr(v0), w, r.wstride, p0, F, r.csf_on, nullptr, r.groups, tab.as<int>(),
                                    r.vox ? r.vox + v0 : nullptr, nv, B, r.kind, r.inflate, r.seed,
                                    r.vox ? r.offset : r.offset + (uint64_t)v0 * (uint64_t)M, 0.0, mem.ys.as<double>(), nullptr,
                                    r.status + v0, st)) return rc;
    if (int rc = wb_rows(p, mem.ys.as<double>(), w, r.wstride, pks, F, xc, nv, B, mem.rows(v0), wst.as<int32_t>(), mem.budget(), st))
      return rc;
    if (int rc = mem.gather_reduce(v0, nv, N)) return rc;
    if (marked) mfx_scratch_rewind(st, mark);
  }
  return MFX_OK;
}

}  // namespace

extern "C" int mfx_wboot_abi_version(void) { return 1; }

extern "C" int mfx_wboot_rep_tile(void) { return WB_R; }

extern "C" void mfx_wboot_debug_set_force_plain(int enabled) { g_force_plain = enabled ? 1 : 0; }

extern "C" int mfx_wboot_resample_dev(int M, const double* d_Y, const double* d_P, const double* d_W, int64_t w_stride,
                                      const double* d_params, int maxfasc, int csf_on, const double* d_peaks, const int32_t* d_groups,
                                      const int64_t* d_vox, int64_t V, int B, int kind, int inflate, uint64_t seed, uint64_t offset,
                                      double* d_Ystar, double* d_peaks_out, int32_t* d_status, void* stream) {
  const char* fn = "mfx_wboot_resample_dev";
  if (mfx_device_count() <= 0) return mfx_no_device();
  if (V < 0 || (V > 0 && (!d_Y || !d_P || !d_W || !d_params || !d_Ystar || !d_status))) return mfx_fail(MFX_ERR_ARG, "%s: bad argument", fn);
  if (int rc = wb_check_rule(fn, M, maxfasc, B, kind)) return rc;
  if (w_stride != 0 && w_stride != M)
    return mfx_fail(MFX_ERR_ARG, "%s: w_stride should be M = %d or 0 (got %lld)", fn, M, (long long)w_stride);
  if (kind == MFX_BOOT_RESIDUAL && !d_groups) return mfx_fail(MFX_ERR_ARG, "%s: kind 1 needs groups", fn);
  if (d_peaks && maxfasc > 0 && !d_peaks_out) return mfx_fail(MFX_ERR_ARG, "%s: d_peaks without d_peaks_out", fn);
  if (V == 0) return MFX_OK;
  hipStream_t st = (hipStream_t)stream;
  StreamMem tab(st);
  if (kind == MFX_BOOT_RESIDUAL) HIPCHK(tab.alloc(wb_tab_bytes(kind, M, w_stride, V)));
  return wb_launch_resample(M, d_Y, d_P, d_W, w_stride, d_params, maxfasc, csf_on != 0, d_peaks, d_groups, tab.as<int>(), d_vox, V, B, kind,
                            inflate != 0, seed, offset, __builtin_nan(""), d_Ystar, d_peaks_out, d_status, st);
}

extern "C" int mfx_wboot_fit_rows_dev(const void* pv, const double* d_Ystar, const double* d_W, int64_t w_stride, const double* d_peaks,
                                      int maxfasc, int64_t V, int B, double* d_params, int32_t* d_status, void* stream) {
  const char* fn = "mfx_wboot_fit_rows_dev";
  if (mfx_device_count() <= 0) return mfx_no_device();
  const mfx_plan* p = (const mfx_plan*)pv;
  if (!p || V < 0 || maxfasc < 0 || (V > 0 && (!d_Ystar || !d_W || !d_params || !d_status || (maxfasc > 0 && !d_peaks))))
    return mfx_fail(MFX_ERR_ARG, "%s: bad argument", fn);
  if (B < 1) return mfx_fail(MFX_ERR_ARG, "%s: B should be at least 1, got %d", fn, B);
  if (maxfasc > WB_MAXF) return mfx_fail(MFX_ERR_UNSUPPORTED, "%s: at most 3 fascicles (got %d)", fn, maxfasc);
  TablesDev T;
  PlanDev P;
  int device = 0;
  mfx_plan_view(p, &T, &P, &device);
  if (w_stride != 0 && w_stride != P.M)
    return mfx_fail(MFX_ERR_ARG, "%s: w_stride should be M = %d or 0 (got %lld)", fn, P.M, (long long)w_stride);
  if (V == 0) return MFX_OK;
  if (int rc = mfx_require_device(device)) return rc;
  return wb_rows(p, d_Ystar, d_W, w_stride, d_peaks, maxfasc, nullptr, V, B, d_params, d_status, BOOT_DEFAULT_BYTES, (hipStream_t)stream);
}

extern "C" int mfx_wboot_fit_dev(const void* pv, const double* d_Y, const double* d_W, int64_t w_stride, const double* d_peaks, int maxfasc,
                                 int csf_on, const double* d_sig_csf, const double* d_params0, const double* d_pred0,
                                 const int32_t* d_groups, const int64_t* d_vox, int64_t V, int B, int kind, int inflate, uint64_t seed,
                                 uint64_t offset, const double* d_props, int nprop, const double* d_q, int Q, int64_t max_bytes,
                                 double* d_stats, int32_t* d_agree, int32_t* d_status, double* d_keep, void* stream) {
  const char* fn = "mfx_wboot_fit_dev";
  if (mfx_device_count() <= 0) return mfx_no_device();
  const mfx_plan* p = (const mfx_plan*)pv;
  csf_on = csf_on != 0;
  if (int rc = wb_check_fit(fn, p, w_stride, maxfasc, csf_on, d_sig_csf, B, kind, d_groups, nprop, d_props, Q, d_q)) return rc;
  if (V < 0 || (V > 0 && (!d_Y || !d_W || !d_stats || !d_status || (maxfasc > 0 && (!d_peaks || !d_agree)))))
    return mfx_fail(MFX_ERR_ARG, "%s: bad argument", fn);
  if (d_pred0 && !d_params0) return mfx_fail(MFX_ERR_ARG, "%s: a prediction needs the parameters it was made from", fn);
  if (V == 0) return MFX_OK;
  TablesDev T;
  PlanDev P;
  int device = 0;
  mfx_plan_view(p, &T, &P, &device);
  if (int rc = mfx_require_device(device)) return rc;
  BootClass r{};
  r.Y = d_Y; r.W = d_W; r.wstride = w_stride; r.peaks = d_peaks; r.F = maxfasc; r.csf_on = csf_on; r.sig_csf = d_sig_csf;
  r.params0 = d_params0; r.pred0 = d_pred0; r.groups = d_groups; r.vox = d_vox; r.V = V; r.B = B; r.kind = kind; r.inflate = inflate != 0;
  r.seed = seed; r.offset = offset; r.props = d_props; r.nprop = nprop; r.q = d_q; r.Q = Q; r.max_bytes = max_bytes;
  r.stats = d_stats; r.agree = d_agree; r.status = d_status; r.keep = d_keep; r.st = (hipStream_t)stream;
  return wb_class_dev(p, r);
}

extern "C" int mfx_wboot_fit(const void* pv, const double* Y, const double* W, int64_t w_stride, const int32_t* K, const uint8_t* csf,
                             const double* peaks, int maxfasc, int csf_on, const double* sig_csf, const double* params0,
                             const int32_t* groups, const int64_t* vox, int64_t V, int B, int kind, int inflate, uint64_t seed,
                             uint64_t offset, const double* props, int nprop, const double* q, int Q, int64_t max_bytes, double* stats,
                             int32_t* agree, int32_t* status, double* keep) {
  const char* fn = "mfx_wboot_fit";
  if (mfx_device_count() <= 0) return mfx_no_device();
  const mfx_plan* p = (const mfx_plan*)pv;
  csf_on = csf_on != 0;
  if (int rc = wb_check_fit(fn, p, w_stride, maxfasc, csf_on, sig_csf, B, kind, groups, nprop, props, Q, q)) return rc;
  if (V < 0 || (V > 0 && (!Y || !W || !K || !stats || !status || (maxfasc > 0 && (!peaks || !agree)))))
    return mfx_fail(MFX_ERR_ARG, "%s: bad argument", fn);
  for (int i = 0; i < Q; ++i)
    if (!(q[i] >= 0.0 && q[i] <= 1.0)) return mfx_fail(MFX_ERR_ARG, "%s: q[%d] = %g outside [0, 1]", fn, i, q[i]);
  TablesDev T;
  PlanDev P;
  int device = 0;
  mfx_plan_view(p, &T, &P, &device);
  BootBatch b{};
  b.fn = fn; b.device = device; b.M = P.M; b.N = T.N; b.Y = Y; b.W = W; b.w_stride = w_stride; b.K = K; b.csf = csf; b.peaks = peaks;
  b.F = maxfasc; b.csf_on = csf_on; b.sig_csf = sig_csf; b.params0 = params0; b.groups = groups; b.vox = vox; b.V = V;
  b.B = B; b.kind = kind; b.inflate = inflate != 0; b.seed = seed; b.offset = offset; b.props = props; b.nprop = nprop;
  b.q = q; b.Q = Q; b.max_bytes = max_bytes; b.stats = stats; b.agree = agree; b.status = status; b.keep = keep;
  return boot_run_mixed(b, [&](const BootClass& r) { return wb_class_dev(p, r); });
}
