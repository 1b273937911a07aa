// predict.hip -- the forward model (include/mfx_predict.h): fit parameters -> DW-MRI signal, with optional
// sum-of-squares magnitude noise and an optional residual against measured data, in one pass.
//
// mfx_predict_kernel     One wave per voxel (four per workgroup, voxels dealt round-robin over the waves of the grid).
//                        The voxel's parameter row is decoded once per wave from wave-uniform addresses; lane l then
//                        owns the protocol rows l, l + 64, ...: it builds the row descriptor of each present fascicle
//                        once (mfx_row_desc, as mfx_rotate_cols_kernel does, so a predicted column has that kernel's
//                        bits), adds the compartments in the order f0, f1, ..., csf, ear and stores 64 consecutive
//                        doubles per wave instruction.  The atoms' knot tables are read through L2; the knot
//                        abscissae and the plan's rows, which every voxel reads again, are staged in LDS once per
//                        workgroup when they fit (see the kernel).  Measured, the kernel is bound by the latency of
//                        locating each row's knot interval, not yet by the V M 8 bytes it writes.
//                        Residual: the lanes keep partial sums over their rows, a fixed xor butterfly over the 64 lanes
//                        adds them - the order depends on M alone, not on the grid.  R2 needs the means first, so a
//                        second sweep re-reads the row this wave has just written (L2 hits) and Y.
// mfx_sos_noise_kernel   one element per thread, grid-stride.
//
// The noise generator, the magnitude of one element and the wave's fixed-order sum are those of sos_shared.h, which
// predict2d.hip shares.
#include "mfx_host.h"
#include "sos_shared.h"
#include "../../include/mfx_predict.h"

#include <algorithm>
#include <cmath>

namespace {

constexpr int PRED_WG = 256;
constexpr int PRED_WAVES = PRED_WG / 64;
constexpr size_t PRED_LDS_MAX = 40 * 1024;        // knots and plan rows are kept in LDS up to this size; beyond it they are read through L2
constexpr int PRED_MAXF = 3;                      // mfx_fit_batch_dev's limit on maxfasc

struct PredArgs {
  const double* params;   // [V x np]
  const double* peaks;    // [V x 3 maxfasc]
  const double* sig_csf;  // [M]
  const double* sig_ear;  // [M x E]
  const double* Y;        // [V x M] or null
  const double* sigma;    // per sigma_mode (ncoils > 0)
  double* out;            // [V x M]
  double* stats;          // [V x 2] (Y given)
  int* status;            // [2]
  int64_t V;
  unsigned long long seed, offset;
  int np, maxfasc, csf_on, ear_on, E, sigma_mode, ncoils;
  int lds;                // knots and plan rows staged in LDS (predict_lds_bytes)
};

template <bool NOISE, bool RESID>
__device__ __forceinline__ void predict_voxels(const TablesDev& T, const PlanDev& P, const PredArgs& a) {
  const int lane = threadIdx.x & 63;
  const int M = P.M, N = T.N, F = a.maxfasc;
  const int64_t nwaves = (int64_t)gridDim.x * PRED_WAVES;
  const double qnan = __longlong_as_double(0x7ff8000000000000LL);
  for (int64_t v = (int64_t)blockIdx.x * PRED_WAVES + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6); v < a.V; v += nwaves) {
    const double* __restrict__ pr = a.params + v * a.np;
    const double M0 = pr[0];
    int bad = 0;
    double w[PRED_MAXF], d[PRED_MAXF][3];
    int id[PRED_MAXF];
#pragma unroll
    for (int k = 0; k < PRED_MAXF; ++k) {
      w[k] = 0.0; id[k] = 0; d[k][0] = d[k][1] = d[k][2] = 0.0;
      if (k < F) {
        const double wk = M0 * pr[1 + k];
        if (!(wk >= 0.0) || isinf(wk)) bad |= MFX_PRED_ST_WEIGHT;
        else if (wk > 0.0) {   // a zero weight: direction and ID are not looked at
          const double idd = pr[1 + F + k];
          if (!(idd >= 0.0 && idd < (double)N && idd == floor(idd))) bad |= MFX_PRED_ST_ID;
          else {
            const double* __restrict__ pk = a.peaks + v * (3 * F) + 3 * k;
            w[k] = wk; id[k] = (int)idd; d[k][0] = pk[0]; d[k][1] = pk[1]; d[k][2] = pk[2];
            if (lane == 0) mfx_check_dir(P, pk, (int)v);
          }
        }
      }
    }
    double wc = 0.0, we = 0.0;
    int ide = 0;
    if (a.csf_on) {
      const double x = M0 * pr[1 + 2 * F];
      if (!(x >= 0.0) || isinf(x)) bad |= MFX_PRED_ST_WEIGHT; else wc = x;
    }
    if (a.ear_on) {
      const int ie = 1 + 2 * F + a.csf_on;
      const double x = M0 * pr[ie];
      if (!(x >= 0.0) || isinf(x)) bad |= MFX_PRED_ST_WEIGHT;
      else if (x > 0.0) {
        const double idd = pr[ie + 1];
        if (!(idd >= 0.0 && idd < (double)a.E && idd == floor(idd))) bad |= MFX_PRED_ST_ID;
        else { we = x; ide = (int)idd; }
      }
    }
    if (bad && lane == 0) {
      atomicOr(a.status, bad);
      a.status[1] = (int)v;
    }
    double sg = 0.0;
    if (NOISE && a.sigma_mode != MFX_SIGMA_ELEMENT) sg = a.sigma[a.sigma_mode == MFX_SIGMA_VOXEL ? v : 0];
    double* __restrict__ o = a.out + v * M;
    const double* __restrict__ y = RESID ? a.Y + v * M : nullptr;
    double rss = 0.0, sy = 0.0, so = 0.0;
    for (int m = lane; m < M; m += 64) {
      double acc = 0.0;
      if (bad) acc = qnan;
      else {
#pragma unroll
        for (int k = 0; k < PRED_MAXF; ++k)
          if (w[k] > 0.0) {
            const RowDesc rd = mfx_row_desc(T, P, m, d[k][0], d[k][1], d[k][2]);
            acc = acc + w[k] * mfx_eval_br(T.tab, T.ldn, rd, P.tG[m], P.dG[m], id[k]);
          }
        if (wc > 0.0) acc = acc + wc * a.sig_csf[m];
        if (we > 0.0) acc = acc + we * a.sig_ear[(size_t)m * a.E + ide];
        if (NOISE) {
          const unsigned long long i = (unsigned long long)(v * M + m);
          acc = sos_value(acc, a.sigma_mode == MFX_SIGMA_ELEMENT ? a.sigma[i] : sg, a.ncoils, a.seed, a.offset + i);
        }
      }
      o[m] = acc;
      if (RESID) {
        const double yy = y[m], r = yy - acc;
        rss = rss + r * r; sy = sy + yy; so = so + acc;
      }
    }
    if (RESID) {
      rss = wave_sum(rss);
      const double my = wave_sum(sy) / M, mo = wave_sum(so) / M;
      double syy = 0.0, soo = 0.0, syo = 0.0;
#pragma unroll 4
      for (int m = lane; m < M; m += 64) {   // o[m] was stored by this very lane
        const double dy = y[m] - my, dd = o[m] - mo;
        syy = syy + dy * dy; soo = soo + dd * dd; syo = syo + dy * dd;
      }
      syy = wave_sum(syy); soo = wave_sum(soo); syo = wave_sum(syo);
      if (lane == 0) {
        double R2 = 0.0;   // mf.py:449-450
        if (M > 1 && syy > 0.0 && soo > 0.0) {
          double r = syo / sqrt(syy) / sqrt(soo);
          r = fmin(1.0, fmax(-1.0, r));   // np.corrcoef clips
          R2 = r * r;
        }
        a.stats[2 * v] = rss;
        a.stats[2 * v + 1] = bad ? qnan : R2;
      }
    }
  }
}

template <bool NOISE, bool RESID>
__global__ __launch_bounds__(PRED_WG) void mfx_predict_kernel(TablesDev T, PlanDev P, PredArgs a) {
  // What every voxel reads again - the knot abscissae of the shells and the plan's rows - goes to LDS once per
  // workgroup (a.lds: the host found that it fits).  Locating a row's knot interval is a chain of dependent loads
  // (plan row -> shell offsets -> binary search -> knot), and from L2 that chain, not the V M 8 bytes written, set
  // the kernel's time.  Same values, same comparisons, same arithmetic: the results do not change.
  extern __shared__ double s_mem[];
  if (a.lds) {
    const int M = P.M, S1 = T.S + 1;
    double* s_x = s_mem;
    double* s_g = s_x + T.P;
    double* s_tG = s_g + 3 * M;
    double* s_dG = s_tG + M;
    int* s_lo = (int*)(s_dG + M);
    int* s_hi = s_lo + M;
    int* s_off = s_hi + M;
    for (int i = threadIdx.x; i < T.P; i += PRED_WG) s_x[i] = T.x[i];
    for (int i = threadIdx.x; i < 3 * M; i += PRED_WG) s_g[i] = P.g[i];
    for (int i = threadIdx.x; i < M; i += PRED_WG) {
      s_tG[i] = P.tG[i]; s_dG[i] = P.dG[i]; s_lo[i] = P.s_lo[i]; s_hi[i] = P.s_hi[i];
    }
    for (int i = threadIdx.x; i < S1; i += PRED_WG) s_off[i] = T.off[i];
    __syncthreads();
    TablesDev TL = T;
    PlanDev PL = P;
    TL.x = s_x; TL.off = s_off;
    PL.g = s_g; PL.tG = s_tG; PL.dG = s_dG; PL.s_lo = s_lo; PL.s_hi = s_hi;
    predict_voxels<NOISE, RESID>(TL, PL, a);
  } else {
    predict_voxels<NOISE, RESID>(T, P, a);
  }
}

__global__ __launch_bounds__(256) void mfx_sos_noise_kernel(const double* S0, int64_t n, const double* __restrict__ sigma,
                                                            int sigma_mode, int ncoils, unsigned long long seed,
                                                            unsigned long long offset, double* out) {   // out may be S0
  const int64_t step = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += step)
    out[i] = sos_value(S0[i], sigma[sigma_mode == MFX_SIGMA_ELEMENT ? i : 0], ncoils, seed, offset + (unsigned long long)i);
}

int pred_num_params(int maxfasc, int csf_on, int ear_on) { return 1 + 2 * maxfasc + (csf_on ? 1 : 0) + (ear_on ? 2 : 0) + 2; }

// what both prediction entry points check before anything else
int pred_check_args(const char* fn, const mfx_plan* p, const void* params, const void* peaks, int maxfasc, int csf_on, int ear_on,
                    const void* sig_csf, const void* sig_ear, int E, int64_t V, const void* Y, const void* sigma, int sigma_mode,
                    int ncoils, const void* out, const void* stats) {
  if (!p || V < 0 || (V > 0 && (!params || !out))) return mfx_fail(MFX_ERR_ARG, "%s: bad argument", fn);
  if (maxfasc < 0 || maxfasc > PRED_MAXF) return mfx_fail(MFX_ERR_ARG, "%s: maxfasc must be 0..%d", fn, PRED_MAXF);
  if (V > 0 && maxfasc > 0 && !peaks) return mfx_fail(MFX_ERR_ARG, "%s: peaks is null but maxfasc = %d", fn, maxfasc);
  if (csf_on && !sig_csf) return mfx_fail(MFX_ERR_ARG, "%s: csf_on without sig_csf", fn);
  if (ear_on && (!sig_ear || E < 1)) return mfx_fail(MFX_ERR_ARG, "%s: ear_on without sig_ear [M x E], E >= 1", fn);
  if (ncoils < 0) return mfx_fail(MFX_ERR_ARG, "%s: ncoils must not be negative", fn);
  if (ncoils > 0 && (!sigma || sigma_mode < MFX_SIGMA_SCALAR || sigma_mode > MFX_SIGMA_ELEMENT))
    return mfx_fail(MFX_ERR_ARG, "%s: noise needs sigma and a sigma_mode of 0, 1 or 2", fn);
  if (V > 0 && Y && !stats) return mfx_fail(MFX_ERR_ARG, "%s: Y without stats", fn);
  return MFX_OK;
}

int sos_check_args(const char* fn, const void* S0, int64_t n, const void* sigma, int sigma_mode, int ncoils, const void* out) {
  if (n < 0 || (n > 0 && (!S0 || !sigma || !out))) return mfx_fail(MFX_ERR_ARG, "%s: bad argument", fn);
  if (ncoils < 1) return mfx_fail(MFX_ERR_ARG, "%s: ncoils must be at least 1", fn);
  if (sigma_mode != MFX_SIGMA_SCALAR && sigma_mode != MFX_SIGMA_ELEMENT)
    return mfx_fail(MFX_ERR_ARG, "%s: sigma_mode must be 0 (scalar) or 2 (one per element)", fn);
  return MFX_OK;
}

unsigned grid_for(int64_t items, int per_block) {   // memory-bound, grid-stride: a few workgroups per CU
  const int64_t blocks = (items + per_block - 1) / per_block;
  return (unsigned)std::min<int64_t>(blocks, 256 * 16);
}

}  // namespace

extern "C" int mfx_predict_abi_version(void) { return 1; }

extern "C" int mfx_predict_dev(const mfx_plan* p, const double* d_params, const double* d_peaks, int maxfasc, int csf_on,
                               int ear_on, const double* d_sig_csf, const double* d_sig_ear, int E, int64_t V,
                               const double* d_Y, const double* d_sigma, int sigma_mode, int ncoils, uint64_t seed,
                               uint64_t offset, double* d_out, double* d_stats, int32_t* d_status, void* stream) {
  if (mfx_device_count() <= 0) return mfx_no_device();
  if (int rc = pred_check_args("mfx_predict_dev", p, d_params, d_peaks, maxfasc, csf_on, ear_on, d_sig_csf, d_sig_ear, E, V, d_Y,
                               d_sigma, sigma_mode, ncoils, d_out, d_stats)) return rc;
  if (V > 0 && !d_status) return mfx_fail(MFX_ERR_ARG, "mfx_predict_dev: d_status is null");
  if (V == 0) return MFX_OK;
  if (V > 0x7fffffff) return mfx_fail(MFX_ERR_ARG, "mfx_predict_dev: V too large for one call");
  TablesDev T;
  PlanDev P;
  int device = 0;
  mfx_plan_view(p, &T, &P, &device);
  if (int rc = mfx_require_device(device)) return rc;
  PredArgs a{};
  a.params = d_params; a.peaks = d_peaks; a.sig_csf = d_sig_csf; a.sig_ear = d_sig_ear; a.Y = d_Y; a.sigma = d_sigma;
  a.out = d_out; a.stats = d_stats; a.status = d_status; a.V = V; a.seed = seed; a.offset = offset;
  a.np = pred_num_params(maxfasc, csf_on, ear_on); a.maxfasc = maxfasc; a.csf_on = csf_on ? 1 : 0; a.ear_on = ear_on ? 1 : 0;
  a.E = ear_on ? E : 0; a.sigma_mode = sigma_mode; a.ncoils = ncoils;
  // x [P], g [3M], tG [M], dG [M] doubles; s_lo [M], s_hi [M], off [S + 1] ints
  size_t lds = sizeof(double) * ((size_t)T.P + 5 * (size_t)P.M) + sizeof(int) * (2 * (size_t)P.M + T.S + 1);
  a.lds = lds <= PRED_LDS_MAX ? 1 : 0;
  if (!a.lds) lds = 0;
  const dim3 grid(grid_for(V, PRED_WAVES)), wg(PRED_WG);
  hipStream_t st = (hipStream_t)stream;
  if (ncoils > 0 && d_Y) hipLaunchKernelGGL((mfx_predict_kernel<true, true>), grid, wg, lds, st, T, P, a);
  else if (ncoils > 0) hipLaunchKernelGGL((mfx_predict_kernel<true, false>), grid, wg, lds, st, T, P, a);
  else if (d_Y) hipLaunchKernelGGL((mfx_predict_kernel<false, true>), grid, wg, lds, st, T, P, a);
  else hipLaunchKernelGGL((mfx_predict_kernel<false, false>), grid, wg, lds, st, T, P, a);
  HIPCHK(hipGetLastError());
  return MFX_OK;
}

extern "C" int mfx_predict(const mfx_plan* p, const double* params, const double* peaks, int maxfasc, int csf_on, int ear_on,
                           const double* sig_csf, const double* sig_ear, int E, int64_t V, const double* Y,
                           const double* sigma, int sigma_mode, int ncoils, uint64_t seed, uint64_t offset, double* out,
                           double* stats) {
  const char* fn = "mfx_predict";
  if (int rc = pred_check_args(fn, p, params, peaks, maxfasc, csf_on, ear_on, sig_csf, sig_ear, E, V, Y, sigma, sigma_mode,
                               ncoils, out, stats)) return rc;
  if (V == 0) return MFX_OK;
  TablesDev T;
  PlanDev P;
  int device = 0;
  mfx_plan_view(p, &T, &P, &device);
  const int np = pred_num_params(maxfasc, csf_on, ear_on), M = P.M;
  for (int64_t v = 0; v < V; ++v) {   // the argument errors the device entry point can only flag
    const double* pr = params + v * np;
    for (int c = 0; c < maxfasc + (csf_on ? 1 : 0) + (ear_on ? 1 : 0); ++c) {
      const bool fasc = c < maxfasc, csf = !fasc && csf_on && c == maxfasc;
      const int iw = fasc ? 1 + c : (csf ? 1 + 2 * maxfasc : 1 + 2 * maxfasc + (csf_on ? 1 : 0));
      const double w = pr[0] * pr[iw];
      if (!(w >= 0.0) || std::isinf(w))
        return mfx_fail(MFX_ERR_ARG, "%s: voxel %lld: weight M0 * nu = %g of compartment %d is negative or not finite", fn,
                        (long long)v, w, c);
      if (w > 0.0 && !csf) {
        const double id = pr[fasc ? 1 + maxfasc + c : iw + 1];
        const int lim = fasc ? T.N : E;
        if (!(id >= 0.0 && id < (double)lim && id == std::floor(id)))
          return mfx_fail(MFX_ERR_ARG, "%s: voxel %lld: atom index %g of compartment %d is not an integer in [0, %d)", fn,
                          (long long)v, id, c, lim);
      }
    }
  }
  if (int rc = mfx_require_device(device)) return rc;
  const size_t VM = (size_t)V * M;
  const size_t n_sigma = ncoils > 0 ? (sigma_mode == MFX_SIGMA_SCALAR ? 1 : (sigma_mode == MFX_SIGMA_VOXEL ? (size_t)V : VM)) : 0;
  DevMem dpar, dpk, dcsf, dear, dY, dsig, dout, dstats, dst;
  HIPCHK(dpar.alloc(sizeof(double) * V * np));
  HIPCHK(dpk.alloc(sizeof(double) * V * 3 * maxfasc));
  HIPCHK(dcsf.alloc(sizeof(double) * M));
  HIPCHK(dear.alloc(sizeof(double) * M * (ear_on ? E : 0)));
  HIPCHK(dY.alloc(Y ? sizeof(double) * VM : 0));
  HIPCHK(dsig.alloc(sizeof(double) * n_sigma));
  HIPCHK(dout.alloc(sizeof(double) * VM));
  HIPCHK(dstats.alloc(sizeof(double) * 2 * V));
  HIPCHK(dst.alloc(2 * sizeof(int)));
  HIPCHK(hipMemcpy(dpar.p, params, sizeof(double) * V * np, hipMemcpyHostToDevice));
  if (maxfasc > 0) HIPCHK(hipMemcpy(dpk.p, peaks, sizeof(double) * V * 3 * maxfasc, hipMemcpyHostToDevice));
  if (csf_on) HIPCHK(hipMemcpy(dcsf.p, sig_csf, sizeof(double) * M, hipMemcpyHostToDevice));
  if (ear_on) HIPCHK(hipMemcpy(dear.p, sig_ear, sizeof(double) * M * E, hipMemcpyHostToDevice));
  if (Y) HIPCHK(hipMemcpy(dY.p, Y, sizeof(double) * VM, hipMemcpyHostToDevice));
  if (n_sigma) HIPCHK(hipMemcpy(dsig.p, sigma, sizeof(double) * n_sigma, hipMemcpyHostToDevice));
  HIPCHK(hipMemset(dst.p, 0, 2 * sizeof(int)));
  if (int rc = mfx_predict_dev(p, dpar.as<double>(), maxfasc > 0 ? dpk.as<double>() : nullptr, maxfasc, csf_on, ear_on,
                               csf_on ? dcsf.as<double>() : nullptr, ear_on ? dear.as<double>() : nullptr, E, V,
                               Y ? dY.as<double>() : nullptr, n_sigma ? dsig.as<double>() : nullptr, sigma_mode, ncoils, seed,
                               offset, dout.as<double>(), dstats.as<double>(), dst.as<int32_t>(), nullptr)) return rc;
  if (int rc = mfx_plan_status(p, nullptr)) return rc;   // waits; a direction that is not a unit vector
  int st[2] = {0, 0};
  HIPCHK(hipMemcpy(st, dst.p, sizeof(st), hipMemcpyDeviceToHost));
  if (st[0]) return mfx_fail(MFX_ERR_ARG, "%s: the kernel flagged status 0x%x in voxel %d", fn, st[0], st[1]);
  HIPCHK(hipMemcpy(out, dout.p, sizeof(double) * VM, hipMemcpyDeviceToHost));
  if (Y) HIPCHK(hipMemcpy(stats, dstats.p, sizeof(double) * 2 * V, hipMemcpyDeviceToHost));
  return MFX_OK;
}

extern "C" int mfx_sos_noise_dev(const double* d_S0, int64_t n, const double* d_sigma, int sigma_mode, int ncoils, uint64_t seed,
                                 uint64_t offset, double* d_out, int device, void* stream) {
  if (mfx_device_count() <= 0) return mfx_no_device();
  if (int rc = sos_check_args("mfx_sos_noise_dev", d_S0, n, d_sigma, sigma_mode, ncoils, d_out)) return rc;
  if (n == 0) return MFX_OK;
  if (int rc = mfx_require_device(device)) return rc;
  hipLaunchKernelGGL(mfx_sos_noise_kernel, dim3(grid_for(n, 256)), dim3(256), 0, (hipStream_t)stream, d_S0, n, d_sigma,
                     sigma_mode, ncoils, (unsigned long long)seed, (unsigned long long)offset, d_out);
  HIPCHK(hipGetLastError());
  return MFX_OK;
}

extern "C" int mfx_sos_noise(const double* S0, int64_t n, const double* sigma, int sigma_mode, int ncoils, uint64_t seed,
                             uint64_t offset, double* out, int device) {
  if (int rc = sos_check_args("mfx_sos_noise", S0, n, sigma, sigma_mode, ncoils, out)) return rc;
  if (n == 0) return MFX_OK;
  if (int rc = mfx_require_device(device)) return rc;
  const size_t ns = sigma_mode == MFX_SIGMA_ELEMENT ? (size_t)n : 1;
  DevMem dS, dsig;
  HIPCHK(dS.alloc(sizeof(double) * n));
  HIPCHK(dsig.alloc(sizeof(double) * ns));
  HIPCHK(hipMemcpy(dS.p, S0, sizeof(double) * n, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(dsig.p, sigma, sizeof(double) * ns, hipMemcpyHostToDevice));
  if (int rc = mfx_sos_noise_dev(dS.as<double>(), n, dsig.as<double>(), sigma_mode, ncoils, seed, offset, dS.as<double>(), device,
                                 nullptr)) return rc;
  HIPCHK(hipMemcpy(out, dS.p, sizeof(double) * n, hipMemcpyDeviceToHost));   // (waits for the kernel on the default stream)
  return MFX_OK;
}
