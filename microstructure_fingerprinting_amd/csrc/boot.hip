// boot.hip -- the bootstrap (include/mfx_boot.h): replicate signals from the residuals of a voxel's own fit, the plain
// fit on the replicates (mfx_fit_batch_dev, unchanged), and the B parameter rows of every voxel reduced to statistics.
// The fit and the prediction are the entry points of mfx.h and mfx_predict.h; what is new here is three kernels and a
// small table.  The host side of a mixed batch is boot_shared.h's boot_run_mixed (binning and walking: class_batch.h; the
// column maps, the gather and the scatter: boot_batch.h), shared with wboot.hip, boot2d.hip and wboot2d.hip.
//
// boot_group_table_kernel     kind 1, once per call: for every row m the place of its group's row list in `rows`
//                        (start[m]: the number of rows of smaller groups), the group's size (cnt[m]) and the list
//                        itself (rows[start .. start + cnt): the group's rows ascending).  One workgroup, M^2 / 256
//                        comparisons per thread: nothing is searched per element later.
// mfx_boot_resample_kernel<KIND>   One wave per (voxel, replicate) row, 4 rows per workgroup.  Lane l
//                        owns the measurements l, l + 64, ...: one Philox block per element, the rule of mfx_boot.h
//                        line by line (every line one rounding), 8-byte stores that a wave issues 512 contiguous bytes
//                        at a time.  The scale a is a host-made table indexed by n_act (at most 5 active weights).
//                        A voxel whose y or p row is not finite (ballot) or that has no degree of freedom gets
//                        `fill` rows: NaN through mfx_boot_resample_dev, zeros inside mfx_boot_fit_dev.
// mfx_boot_gather_kernel  One wave per voxel, lane l owns the replicates l, l + 64, ...: the value table X, its validity
//                        mask and the agreement counts (summed over the wave in a fixed order; integers).
// mfx_boot_reduce_kernel  One wave per (voxel, column), boot_red_waves(B, Q) of them per workgroup (a wave beyond the
//                        work idles through the barriers).  Pass 1 packs the valid values in the order of b into the
//                        wave's LDS slice (ballot prefix, as robust.hip packs its residuals); pass 2 counts ranks -
//                        the rank of packed element i is #{j : x_j < x_i or (x_j == x_i and j < i)}, a total order, so
//                        exactly one element has each rank - and the lane that meets a wanted rank leaves the value
//                        in LDS; pass 3 does the serial sums (every lane the same LDS broadcasts, no shuffle) and the
//                        interpolation.  No sort, no atomics, one fixed result.
// LDS of the reduction: 8 B + 24 Q bytes per wave, at most 64 KB per workgroup: 4 waves up to B = 2000 or so, 1 wave at
// B = 4096 (32 KiB + the quantiles' 768 bytes).
#include "boot_shared.h"
#include "sos_shared.h"
#include "../../include/mfx_predict.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

namespace {

constexpr int BOOT_MAX_ROWS = 8192;
constexpr int BOOT_MAXF = 3;                      // mfx_fit_batch_dev's limit on maxfasc
constexpr int BOOT_MAX_ACT = BOOT_MAXF + 2;       // active weights of a row at the most
constexpr size_t BOOT_LDS_MAX = 64 * 1024;
constexpr double BOOT_DBL_MAX = 1.79769313486231570815e308;

__global__ __launch_bounds__(256) void boot_group_table_kernel(const int* __restrict__ groups, int M, int* __restrict__ start,
                                                              int* __restrict__ cnt, int* __restrict__ rows) {
  for (int m = threadIdx.x; m < M; m += 256) {
    const int g = groups[m];
    int less = 0, eq = 0, before = 0;
    for (int j = 0; j < M; ++j) {
      const int gj = groups[j];
      less += gj < g;
      eq += gj == g;
      before += (gj == g) && (j < m);
    }
    start[m] = less;
    cnt[m] = eq;
    rows[less + before] = m;   // less + before < less + eq <= M
  }
}

struct BootRsArgs {
  const double* Y;        // [V x M]
  const double* P;        // [V x M]
  const double* params;   // [V x np]
  const double* peaks;    // [V x 3 F] or null
  const int* gstart;      // [M] (kind 1)
  const int* gcnt;        // [M]
  const int* grows;       // [M]
  const int64_t* vox;     // [V] or null
  double* Ys;             // [V x B x M]
  double* pk_out;         // [V B x 3 F] or null
  int* status;            // [V]
  int64_t V;
  unsigned long long seed, offset;
  double fill;            // the rows of a voxel in a non-zero status
  double a_tab[BOOT_MAX_ACT + 1];   // the scale by n_act
  int M, B, np, F, csf_on, ear_on;
};

template <int KIND>
__global__ __launch_bounds__(256) void mfx_boot_resample_kernel(BootRsArgs a) {
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
    if (a.ear_on) n_act += pr[1 + 2 * F + a.csf_on] > 0.0;
    const double sc = a.a_tab[n_act];   // n_act <= F + 2 <= BOOT_MAX_ACT
    const double* __restrict__ y = a.Y + v * M;
    const double* __restrict__ p = a.P + v * M;
    double* __restrict__ o = a.Ys + row * M;
    const unsigned long long base = a.offset + (unsigned long long)(a.vox ? a.vox[v] : v) * (unsigned long long)M;
    bool bad = false;
    for (int m = lane; m < M; m += 64) {
      const double ym = y[m], pm = p[m];
      bad |= !(fabs(ym) <= BOOT_DBL_MAX) || !(fabs(pm) <= BOOT_DBL_MAX);
      const unsigned long long idx = base + (unsigned long long)m;
      uint32_t c[4] = {(uint32_t)idx, (uint32_t)(idx >> 32), (uint32_t)b, MFX_BOOT_STREAM};
      philox4x32_10(c, k0, k1);
      double out;
      if (KIND == MFX_BOOT_WILD) {
        const double r = ym - pm;
        const double ar = sc * r;
        const double t = (c[0] & 1u) ? -ar : ar;
        out = pm + t;
      } else {
        const int j = a.grows[a.gstart[m] + (int)mulhi32(c[0], (uint32_t)a.gcnt[m])];   // mulhi32(u, n) < n: inside the group's list
        const double r = y[j] - p[j];
        const double ar = sc * r;
        out = pm + ar;
      }
      o[m] = out;
    }
    bad = __ballot(bad) != 0ull;
    const int st = bad ? 2 : (M <= n_act ? 1 : 0);
    if (st)
      for (int m = lane; m < M; m += 64) o[m] = a.fill;
    if (a.pk_out)
      for (int i = lane; i < 3 * F; i += 64) a.pk_out[row * (3 * F) + i] = a.peaks[v * (3 * F) + i];
    if (b == 0 && lane == 0) a.status[v] = st;
  }
}

struct BootGaArgs {
  double* params;          // [V x B x np]
  const double* params0;   // [V x np]
  const double* props;     // [nprop x N]
  const int* status;       // [V] or null
  double* X;               // [V x B x C]
  uint8_t* valid;          // [V x B x C]
  int* agree;              // [V x F] or null
  int64_t V;
  int B, np, F, csf_on, ear_on, nprop, N, C;
};

__device__ __forceinline__ int wave_sum_int(int x) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
  return x;
}

__global__ __launch_bounds__(256) void mfx_boot_gather_kernel(BootGaArgs a) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int B = a.B, F = a.F, np = a.np, C = a.C, N = a.N;
  const int C0 = 2 + F + a.csf_on + a.ear_on;
  const double qnan = __longlong_as_double(0x7ff8000000000000LL);
  const int64_t v = (int64_t)blockIdx.x * 4 + wave;
  if (v < a.V) {
    const int st = a.status ? a.status[v] : 0;
    int ag[BOOT_MAXF] = {0, 0, 0};
    double id0[BOOT_MAXF] = {-1.0, -1.0, -1.0};
#pragma unroll
    for (int k = 0; k < BOOT_MAXF; ++k)
      if (k < F) id0[k] = a.params0[v * np + 1 + F + k];
    for (int b = lane; b < B; b += 64) {
      double* __restrict__ row = a.params + (v * B + b) * np;
      double* __restrict__ x = a.X + (v * B + b) * C;
      uint8_t* __restrict__ vd = a.valid + (v * B + b) * C;
      if (st) {
        for (int j = 0; j < np; ++j) row[j] = qnan;
        for (int c = 0; c < C; ++c) { x[c] = qnan; vd[c] = 0; }
        continue;
      }
      x[0] = row[0];
      for (int k = 0; k < F; ++k) x[1 + k] = row[1 + k];
      int col = 1 + F;
      if (a.csf_on) x[col++] = row[1 + 2 * F];
      if (a.ear_on) x[col++] = row[1 + 2 * F + a.csf_on];
      x[col++] = row[np - 2];
      for (int c = 0; c < C0; ++c) vd[c] = 1;
#pragma unroll
      for (int k = 0; k < BOOT_MAXF; ++k)
        if (k < F) {
          const double nu = row[1 + k], idd = row[1 + F + k];
          const bool ok = nu > 0.0 && idd >= 0.0 && idd < (double)N && idd == floor(idd);
          const int id = ok ? (int)idd : 0;
          for (int t = 0; t < a.nprop; ++t) {
            x[C0 + k * a.nprop + t] = ok ? a.props[(size_t)t * N + id] : qnan;
            vd[C0 + k * a.nprop + t] = ok ? 1 : 0;
          }
          ag[k] += (ok && idd == id0[k]) ? 1 : 0;
        }
    }
    if (a.agree) {
#pragma unroll
      for (int k = 0; k < BOOT_MAXF; ++k)
        if (k < F) {
          const int s = wave_sum_int(ag[k]);
          if (lane == 0) a.agree[v * F + k] = s;
        }
    }
  }
}

struct BootRdArgs {
  const double* X;        // [V x B x C]
  const uint8_t* valid;   // [V x B x C]
  const double* q;        // [Q]
  double* stats;          // [V x C x (5 + Q)]
  int64_t items;          // V C
  int B, C, Q;
};

inline size_t boot_red_wave_bytes(int B, int Q) { return sizeof(double) * ((size_t)B + 2 * (size_t)Q) + sizeof(int) * 2 * (size_t)Q; }
inline int boot_red_waves(int B, int Q) { return (int)std::max<size_t>(1, std::min<size_t>(4, BOOT_LDS_MAX / boot_red_wave_bytes(B, Q))); }

__global__ __launch_bounds__(256) void mfx_boot_reduce_kernel(BootRdArgs a) {
  extern __shared__ __attribute__((aligned(16))) double s_all[];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int nw = blockDim.x >> 6;
  const int B = a.B, C = a.C, Q = a.Q;
  const int64_t item = (int64_t)blockIdx.x * nw + wave;
  const bool live = item < a.items;   // wave-uniform; an idle wave only takes part in the barriers
  // the wave's slice: x [B], x_lo [Q], x_hi [Q] doubles, then lo [Q], hi [Q] ints (B + 2 Q doubles + Q doubles' worth)
  double* s_x = s_all + (size_t)wave * ((size_t)B + 3 * (size_t)Q);
  double* s_xlo = s_x + B;
  double* s_xhi = s_xlo + Q;
  int* s_lo = (int*)(s_xhi + Q);
  int* s_hi = s_lo + Q;
  const double qnan = __longlong_as_double(0x7ff8000000000000LL);
  const int64_t v = live ? item / C : 0;
  const int c = live ? (int)(item - v * C) : 0;

  // ---- pass 1: pack the valid values in the order of b; the wanted ranks
  int n = 0;
  if (live) {
    for (int base = 0; base < B; base += 64) {
      const int b = base + lane;
      bool in = false;
      double xb = 0.0;
      if (b < B) {
        const int64_t e = (v * B + b) * C + c;
        in = a.valid[e] != 0;
        xb = a.X[e];
      }
      const unsigned long long mk = __ballot(in);
      if (in) s_x[n + __popcll(mk & ((1ull << lane) - 1ull))] = xb;
      n += __popcll(mk);
    }
    if (lane < Q) {
      int lo = 0, hi = 0;
      if (n > 0) {
        const double pos = a.q[lane] * (double)(n - 1);
        const double fl = floor(pos);
        lo = (fl >= 0.0 && fl <= (double)(n - 1)) ? (int)fl : 0;
        hi = lo + 1 < n ? lo + 1 : n - 1;
      }
      s_lo[lane] = lo;
      s_hi[lane] = hi;
      s_xlo[lane] = qnan;
      s_xhi[lane] = qnan;
    }
  }
  __syncthreads();

  // ---- pass 2: rank counting; exactly one element has each rank
  if (live) {
    for (int i = lane; i < n; i += 64) {
      const double xi = s_x[i];
      int rank = 0;
      for (int j = 0; j < n; ++j) {
        const double xj = s_x[j];
        rank += (xj < xi || (xj == xi && j < i)) ? 1 : 0;
      }
      for (int t = 0; t < Q; ++t) {
        if (rank == s_lo[t]) s_xlo[t] = xi;
        if (rank == s_hi[t]) s_xhi[t] = xi;
      }
    }
  }
  __syncthreads();
  if (!live) return;

  // ---- pass 3: the serial sums in the order of b (every lane reads the same LDS words), the interpolation
  double* __restrict__ o = a.stats + item * (MFX_BOOT_NSTAT + Q);
  double mean = qnan, sd = qnan, mn = qnan, mx = qnan;
  if (n > 0) {
    double S = s_x[0];
    mn = S; mx = S;
    for (int i = 1; i < n; ++i) {
      const double x = s_x[i];
      S = S + x;
      mn = x < mn ? x : mn;
      mx = x > mx ? x : mx;
    }
    mean = S / (double)n;
    if (n > 1) {
      double T = 0.0;
      for (int i = 0; i < n; ++i) {
        const double d = s_x[i] - mean;
        const double dd = d * d;
        T = T + dd;
      }
      const double var = T / (double)(n - 1);
      sd = sqrt(var);
    }
  }
  if (lane == 0) { o[0] = (double)n; o[1] = mean; o[2] = sd; o[3] = mn; o[4] = mx; }
  if (lane < Q) {
    double val = qnan;
    if (n > 0) {
      const double pos = a.q[lane] * (double)(n - 1);
      const double frac = pos - (double)s_lo[lane];
      const double xl = s_xlo[lane], xh = s_xhi[lane];
      const double d = xh - xl;
      const double t = d * frac;
      val = xl + t;
    }
    o[MFX_BOOT_NSTAT + lane] = val;
  }
}

unsigned boot_grid(int64_t waves) { return (unsigned)((waves + 3) / 4); }   // 4 waves per workgroup; callers keep waves < 2^31

int boot_check_rule(const char* fn, int M, int F, int B, int kind) {
  if (M < 1) return mfx_fail(MFX_ERR_ARG, "%s: M should be positive, got %d", fn, M);
  if (M > BOOT_MAX_ROWS) return mfx_fail(MFX_ERR_UNSUPPORTED, "%s: more than %d measurements (got %d)", fn, BOOT_MAX_ROWS, M);
  if (F < 0 || F > BOOT_MAXF) return mfx_fail(MFX_ERR_ARG, "%s: maxfasc must be 0..%d (got %d)", fn, BOOT_MAXF, F);
  if (B < 1) return mfx_fail(MFX_ERR_ARG, "%s: B should be at least 1, got %d", fn, B);
  if (kind != MFX_BOOT_WILD && kind != MFX_BOOT_RESIDUAL)
    return mfx_fail(MFX_ERR_ARG, "%s: kind should be 0 (wild) or 1 (residual within groups), got %d", fn, kind);
  return MFX_OK;
}
int boot_check_reduce(const char* fn, int B, int Q) {
  if (B < 1) return mfx_fail(MFX_ERR_ARG, "%s: B should be at least 1, got %d", fn, B);
  if (B > MFX_BOOT_MAX_B)
    return mfx_fail(MFX_ERR_UNSUPPORTED, "%s: at most %d replicates are reduced on the device (got B = %d)", fn, MFX_BOOT_MAX_B, B);
  if (Q < 0) return mfx_fail(MFX_ERR_ARG, "%s: Q should not be negative, got %d", fn, Q);
  if (Q > MFX_BOOT_MAX_Q) return mfx_fail(MFX_ERR_UNSUPPORTED, "%s: at most %d quantiles (got %d)", fn, MFX_BOOT_MAX_Q, Q);
  return MFX_OK;
}

// the group table of a call: start, cnt, rows [M] ints each in one scratch block
int boot_launch_table(const int32_t* d_groups, int M, int* d_tab, hipStream_t st) {
  hipLaunchKernelGGL(boot_group_table_kernel, dim3(1), dim3(256), 0, st, d_groups, M, d_tab, d_tab + M, d_tab + 2 * (size_t)M);
  HIPCHK(hipGetLastError());
  return MFX_OK;
}

int boot_launch_resample(int M, const double* d_Y, const double* d_P, const double* d_params, int F, int csf_on, int ear_on,
                         const double* d_peaks, const int* d_tab, const int64_t* d_vox, int64_t V, int B, int kind, int inflate,
                         uint64_t seed, uint64_t offset, double fill, double* d_Ystar, double* d_peaks_out, int32_t* d_status,
                         hipStream_t st) {
  BootRsArgs a{};
  a.Y = d_Y; a.P = d_P; a.params = d_params; a.peaks = d_peaks;
  a.gstart = d_tab; a.gcnt = d_tab ? d_tab + M : nullptr; a.grows = d_tab ? d_tab + 2 * (size_t)M : nullptr;
  a.vox = d_vox; a.Ys = d_Ystar; a.pk_out = (d_peaks && F > 0) ? d_peaks_out : nullptr; a.status = d_status;
  a.V = V; a.seed = seed; a.offset = offset; a.fill = fill;
  a.M = M; a.B = B; a.np = boot_np(F, csf_on, ear_on); a.F = F; a.csf_on = csf_on; a.ear_on = ear_on;
  for (int n = 0; n <= BOOT_MAX_ACT; ++n) {   // division, then square root, each correctly rounded (host arithmetic)
    double s = 1.0;
    if (inflate && M > n) {
      const double q = (double)M / (double)(M - n);
      s = std::sqrt(q);
    }
    a.a_tab[n] = s;
  }
  if ((V * B + 3) / 4 > 0x7fffffff) return mfx_fail(MFX_ERR_ARG, "mfx_boot: V B too large for one launch");
  const unsigned grid = boot_grid(V * B);
  if (kind == MFX_BOOT_WILD) hipLaunchKernelGGL(mfx_boot_resample_kernel<MFX_BOOT_WILD>, dim3(grid), dim3(256), 0, st, a);
  else hipLaunchKernelGGL(mfx_boot_resample_kernel<MFX_BOOT_RESIDUAL>, dim3(grid), dim3(256), 0, st, a);
  HIPCHK(hipGetLastError());
  return MFX_OK;
}

int boot_launch_gather(double* d_params, const double* d_params0, int F, int csf_on, int ear_on, const double* d_props, int nprop,
                       int N, const int32_t* d_status, int64_t V, int B, double* d_X, uint8_t* d_valid, int32_t* d_agree,
                       hipStream_t st) {
  BootGaArgs a{};
  a.params = d_params; a.params0 = d_params0; a.props = d_props; a.status = d_status; a.X = d_X; a.valid = d_valid;
  a.agree = F > 0 ? d_agree : nullptr; a.V = V; a.B = B; a.np = boot_np(F, csf_on, ear_on); a.F = F; a.csf_on = csf_on;
  a.ear_on = ear_on; a.nprop = nprop; a.N = N; a.C = boot_ncol(F, csf_on, ear_on, nprop);
  if ((V + 3) / 4 > 0x7fffffff) return mfx_fail(MFX_ERR_ARG, "mfx_boot: V too large for one launch");
  hipLaunchKernelGGL(mfx_boot_gather_kernel, dim3(boot_grid(V)), dim3(256), 0, st, a);
  HIPCHK(hipGetLastError());
  return MFX_OK;
}

int boot_launch_reduce(const double* d_X, const uint8_t* d_valid, int64_t V, int B, int C, const double* d_q, int Q, double* d_stats,
                       hipStream_t st) {
  BootRdArgs a{};
  a.X = d_X; a.valid = d_valid; a.q = d_q; a.stats = d_stats; a.items = V * C; a.B = B; a.C = C; a.Q = Q;
  const int nw = boot_red_waves(B, Q);
  const int64_t blocks = (a.items + nw - 1) / nw;
  if (blocks > 0x7fffffff) return mfx_fail(MFX_ERR_ARG, "mfx_boot: V too large for one launch");
  // per wave B + 3 Q doubles (the 2 Q ints take Q doubles' room)
  hipLaunchKernelGGL(mfx_boot_reduce_kernel, dim3((unsigned)blocks), dim3(64 * nw), sizeof(double) * ((size_t)B + 3 * (size_t)Q) * nw, st, a);
  HIPCHK(hipGetLastError());
  return MFX_OK;
}

// One class on device buffers (what mfx_boot_fit_dev does after its checks; mfx_boot_fit runs it per class chunk).
int boot_class_dev(const mfx_plan* p, const BootClass& r) {
  TablesDev T;
  PlanDev P;
  int device = 0;
  mfx_plan_view(p, &T, &P, &device);
  const int M = P.M, N = T.N, F = r.F, B = r.B;
  hipStream_t st = r.st;
  BootChunkMem mem(r, M);
  StreamMem pk(st), tab(st);
  if (int rc = mem.alloc((int64_t)B * M * (int64_t)sizeof(double))) return rc;
  const int64_t Vc = mem.Vc;
  if (F > 0) HIPCHK(pk.alloc(sizeof(double) * (size_t)Vc * B * 3 * F));
  if (r.kind == MFX_BOOT_RESIDUAL) {
    HIPCHK(tab.alloc(sizeof(int) * 3 * (size_t)M));
    if (int rc = boot_launch_table(r.groups, M, tab.as<int>(), st)) return rc;
  }
  // the fit and the prediction take their scratch from the same arena: it is rewound behind the buffers above after
  // every chunk, so that it does not grow with the number of chunks
  ScratchMark mark;
  const bool marked = mfx_scratch_mark(st, &mark);
  for (int64_t v0 = 0; v0 < r.V; v0 += Vc) {
    const int64_t nv = std::min(Vc, r.V - v0);
    const double* y = r.Y + (size_t)v0 * M;
    const double* pks = F > 0 ? r.peaks + (size_t)v0 * 3 * F : nullptr;
    const double* p0 = mem.p0(v0);
    if (!r.params0) {
      HIPCHK(hipMemsetAsync(mem.par0.p, 0, sizeof(double) * (size_t)nv * mem.np, st));
      if (int rc = mfx_fit_batch_dev(p, y, pks, F, r.csf_on, r.ear_on, r.sig_csf, r.sig_ear, r.E, nv, mem.par0.as<double>(), st)) return rc;
    }
    if (!r.pred0)
      if (int rc = mfx_predict_dev(p, p0, pks, F, r.csf_on, r.ear_on, r.sig_csf, r.sig_ear, r.E, nv, nullptr, nullptr, 0, 0, 0, 0,
                                   mem.pred.as<double>(), nullptr, mem.pst.as<int32_t>(), st)) return rc;
    double* rows = mem.rows(v0);
    // (zero rows for a voxel in a non-zero status: the fit never sees a NaN made here; the gather turns its rows into NaN)
    if (int rc = boot_launch_resample(M, y, mem.pr(v0), p0, F, r.csf_on, r.ear_on, pks, tab.as<int>(), r.vox ? r.vox + v0 : nullptr, nv, B,
                                      r.kind, r.inflate, r.seed, r.vox ? r.offset : r.offset + (uint64_t)v0 * (uint64_t)M, 0.0,
                                      mem.ys.as<double>(), pk.as<double>(), r.status + v0, st)) return rc;
    HIPCHK(hipMemsetAsync(rows, 0, sizeof(double) * (size_t)nv * B * mem.np, st));   // classes without a column keep zero rows (mf.py:387-388)
    if (int rc = mfx_fit_batch_dev(p, mem.ys.as<double>(), F > 0 ? pk.as<double>() : nullptr, F, r.csf_on, r.ear_on, r.sig_csf, r.sig_ear,
                                   r.E, nv * B, rows, st)) return rc;
    if (int rc = mem.gather_reduce(v0, nv, N)) return rc;
    if (marked) mfx_scratch_rewind(st, mark);
  }
  return MFX_OK;
}

int boot_check_fit(const char* fn, const mfx_plan* p, int F, int csf_on, int ear_on, const double* sig_csf, const double* sig_ear, int E,
                   int B, int kind, const void* groups, int nprop, const void* props, int Q, const void* q) {
  TablesDev T;
  PlanDev P;
  int device = 0;
  mfx_plan_view(p, &T, &P, &device);
  if (int rc = boot_check_rule(fn, P.M, F, B, kind)) return rc;
  if (int rc = boot_check_reduce(fn, B, Q)) return rc;
  if (kind == MFX_BOOT_RESIDUAL && !groups) return mfx_fail(MFX_ERR_ARG, "%s: kind 1 needs groups", fn);
  if (nprop < 0 || (nprop > 0 && !props) || (Q > 0 && !q)) return mfx_fail(MFX_ERR_ARG, "%s: bad argument", fn);
  if (csf_on && !sig_csf) return mfx_fail(MFX_ERR_ARG, "%s: csf_on without sig_csf", fn);
  if (ear_on && (!sig_ear || E < 1)) return mfx_fail(MFX_ERR_ARG, "%s: ear_on without sig_ear", fn);
  return MFX_OK;
}

}  // namespace

extern "C" int mfx_boot_abi_version(void) { return 1; }

extern "C" int mfx_boot_resample_dev(int M, const double* d_Y, const double* d_P, const double* d_params, int maxfasc, int csf_on,
                                     int ear_on, const double* d_peaks, const int32_t* d_groups, const int64_t* d_vox, int64_t V, int B,
                                     int kind, int inflate, uint64_t seed, uint64_t offset, double* d_Ystar, double* d_peaks_out,
                                     int32_t* d_status, void* stream) {
  const char* fn = "mfx_boot_resample_dev";
  if (mfx_device_count() <= 0) return mfx_no_device();
  if (V < 0 || (V > 0 && (!d_Y || !d_P || !d_params || !d_Ystar || !d_status))) return mfx_fail(MFX_ERR_ARG, "%s: bad argument", fn);
  if (int rc = boot_check_rule(fn, M, maxfasc, B, kind)) return rc;
  if (kind == MFX_BOOT_RESIDUAL && !d_groups) return mfx_fail(MFX_ERR_ARG, "%s: kind 1 needs groups", fn);
  if (d_peaks && maxfasc > 0 && !d_peaks_out) return mfx_fail(MFX_ERR_ARG, "%s: d_peaks without d_peaks_out", fn);
  if (V == 0) return MFX_OK;
  hipStream_t st = (hipStream_t)stream;
  StreamMem tab(st);
  if (kind == MFX_BOOT_RESIDUAL) {
    HIPCHK(tab.alloc(sizeof(int) * 3 * (size_t)M));
    if (int rc = boot_launch_table(d_groups, M, tab.as<int>(), st)) return rc;
  }
  return boot_launch_resample(M, d_Y, d_P, d_params, maxfasc, csf_on != 0, ear_on != 0, d_peaks, tab.as<int>(), d_vox, V, B, kind,
                              inflate != 0, seed, offset, __builtin_nan(""), d_Ystar, d_peaks_out, d_status, st);
}

extern "C" int mfx_boot_gather_dev(double* d_params, const double* d_params0, int maxfasc, int csf_on, int ear_on, const double* d_props,
                                   int nprop, int N, const int32_t* d_status, int64_t V, int B, double* d_X, uint8_t* d_valid,
                                   int32_t* d_agree, void* stream) {
  const char* fn = "mfx_boot_gather_dev";
  if (mfx_device_count() <= 0) return mfx_no_device();
  if (V < 0 || nprop < 0 || (nprop > 0 && (!d_props || N < 1)) || (V > 0 && (!d_params || !d_params0 || !d_X || !d_valid)))
    return mfx_fail(MFX_ERR_ARG, "%s: bad argument", fn);
  if (maxfasc < 0 || maxfasc > BOOT_MAXF) return mfx_fail(MFX_ERR_ARG, "%s: maxfasc must be 0..%d (got %d)", fn, BOOT_MAXF, maxfasc);
  if (B < 1) return mfx_fail(MFX_ERR_ARG, "%s: B should be at least 1, got %d", fn, B);
  if (V == 0) return MFX_OK;
  return boot_launch_gather(d_params, d_params0, maxfasc, csf_on != 0, ear_on != 0, d_props, nprop, N, d_status, V, B, d_X, d_valid,
                            d_agree, (hipStream_t)stream);
}

extern "C" int mfx_boot_reduce_dev(const double* d_X, const uint8_t* d_valid, int64_t V, int B, int C, const double* d_q, int Q,
                                   double* d_stats, void* stream) {
  const char* fn = "mfx_boot_reduce_dev";
  if (mfx_device_count() <= 0) return mfx_no_device();
  if (V < 0 || C < 1 || (Q > 0 && !d_q) || (V > 0 && (!d_X || !d_valid || !d_stats))) return mfx_fail(MFX_ERR_ARG, "%s: bad argument", fn);
  if (int rc = boot_check_reduce(fn, B, Q)) return rc;
  if (V == 0) return MFX_OK;
  return boot_launch_reduce(d_X, d_valid, V, B, C, d_q, Q, d_stats, (hipStream_t)stream);
}

extern "C" int mfx_boot_fit_dev(const mfx_plan* p, const double* d_Y, const double* d_peaks, int maxfasc, int csf_on, int ear_on,
                                const double* d_sig_csf, const double* d_sig_ear, int E, const double* d_params0, const double* d_pred0,
                                const int32_t* d_groups, const int64_t* d_vox, int64_t V, int B, int kind, int inflate, uint64_t seed,
                                uint64_t offset, const double* d_props, int nprop, const double* d_q, int Q, int64_t max_bytes,
                                double* d_stats, int32_t* d_agree, int32_t* d_status, double* d_keep, void* stream) {
  const char* fn = "mfx_boot_fit_dev";
  if (mfx_device_count() <= 0) return mfx_no_device();
  if (!p || V < 0 || (V > 0 && (!d_Y || !d_stats || !d_status || (maxfasc > 0 && (!d_peaks || !d_agree)))))
    return mfx_fail(MFX_ERR_ARG, "%s: bad argument", fn);
  if (d_pred0 && !d_params0) return mfx_fail(MFX_ERR_ARG, "%s: a prediction needs the parameters it was made from", fn);
  csf_on = csf_on != 0; ear_on = ear_on != 0;
  if (int rc = boot_check_fit(fn, p, maxfasc, csf_on, ear_on, d_sig_csf, d_sig_ear, E, B, kind, d_groups, nprop, d_props, Q, d_q)) return rc;
  if (V == 0) return MFX_OK;
  TablesDev T;
  PlanDev P;
  int device = 0;
  mfx_plan_view(p, &T, &P, &device);
  if (int rc = mfx_require_device(device)) return rc;
  BootClass r{};
  r.Y = d_Y; r.peaks = d_peaks; r.F = maxfasc; r.csf_on = csf_on; r.ear_on = ear_on; r.sig_csf = d_sig_csf; r.sig_ear = d_sig_ear; r.E = E;
  r.params0 = d_params0; r.pred0 = d_pred0; r.groups = d_groups; r.vox = d_vox; r.V = V; r.B = B; r.kind = kind; r.inflate = inflate != 0;
  r.seed = seed; r.offset = offset; r.props = d_props; r.nprop = nprop; r.q = d_q; r.Q = Q; r.max_bytes = max_bytes;
  r.stats = d_stats; r.agree = d_agree; r.status = d_status; r.keep = d_keep; r.st = (hipStream_t)stream;
  return boot_class_dev(p, r);
}

extern "C" int mfx_boot_fit(const mfx_plan* p, const double* Y, const int32_t* K, const uint8_t* csf, const uint8_t* ear,
                            const double* peaks, int maxfasc, int csf_on, int ear_on, const double* sig_csf, const double* sig_ear, int E,
                            const double* params0, const int32_t* groups, const int64_t* vox, int64_t V, int B, int kind, int inflate,
                            uint64_t seed, uint64_t offset, const double* props, int nprop, const double* q, int Q, int64_t max_bytes,
                            double* stats, int32_t* agree, int32_t* status, double* keep) {
  const char* fn = "mfx_boot_fit";
  if (mfx_device_count() <= 0) return mfx_no_device();
  if (!p || V < 0 || (V > 0 && (!Y || !K || !stats || !status || (maxfasc > 0 && (!peaks || !agree)))))
    return mfx_fail(MFX_ERR_ARG, "%s: bad argument", fn);
  csf_on = csf_on != 0; ear_on = ear_on != 0;
  if (int rc = boot_check_fit(fn, p, maxfasc, csf_on, ear_on, sig_csf, sig_ear, E, B, kind, groups, nprop, props, Q, q)) return rc;
  for (int i = 0; i < Q; ++i)
    if (!(q[i] >= 0.0 && q[i] <= 1.0)) return mfx_fail(MFX_ERR_ARG, "%s: q[%d] = %g outside [0, 1]", fn, i, q[i]);
  TablesDev T;
  PlanDev P;
  int device = 0;
  mfx_plan_view(p, &T, &P, &device);
  const int F = maxfasc;
  // K, then the EAR flag, then the CSF flag of every voxel; the first offending voxel is the one reported
  for (int64_t v = 0; v < V; ++v) {
    if (K[v] < 0 || K[v] > F) return mfx_fail(MFX_ERR_ARG, "%s: K[%lld] = %d outside 0..%d", fn, (long long)v, K[v], F);
    if (ear && ear[v] && !ear_on) return mfx_fail(MFX_ERR_ARG, "%s: voxels flagged EAR need ear_on and sig_ear", fn);
    if (csf && csf[v] && !csf_on) return mfx_fail(MFX_ERR_ARG, "%s: voxels flagged CSF need csf_on and sig_csf", fn);
  }
  BootBatch b{};
  b.fn = fn; b.device = device; b.M = P.M; b.N = T.N; b.Y = Y; b.K = K; b.csf = csf; b.ear = ear; b.peaks = peaks;
  b.F = F; b.csf_on = csf_on; b.ear_on = ear_on; b.sig_csf = sig_csf; b.sig_ear = sig_ear; b.E = E;
  b.params0 = params0; b.groups = groups; b.vox = vox; b.V = V; b.B = B; b.kind = kind; b.inflate = inflate != 0;
  b.seed = seed; b.offset = offset; b.props = props; b.nprop = nprop; b.q = q; b.Q = Q; b.max_bytes = max_bytes;
  b.stats = stats; b.agree = agree; b.status = status; b.keep = keep;
  return boot_run_mixed(b, [&](const BootClass& r) { return boot_class_dev(p, r); });
}
