// predict2d.hip -- the forward model of 2-D (AxCaliber-like) protocols (include/mfx_predict2d.h): fit parameters ->
// signal, with optional sum-of-squares magnitude noise and an optional residual against measured data, in one pass.
//
// mfx_rot2d_plan_kernel (rotate2d.hip) runs over the V maxfasc directions as it is, fit2d_rec_kernel (fit2d_shared.h)
// turns its records into the 32-byte records the fits read; the kernel here reads the same records.
//
// mfx_predict2d_kernel   One wave per voxel (four per workgroup, voxels dealt round-robin over the waves of the grid).
//                        The voxel's parameter row is decoded once per wave from wave-uniform addresses; lane l then
//                        owns the protocol rows l, l + 64, ...: per row and present fascicle k it reads the F2Rec of
//                        (voxel, k, row) - consecutive lanes read consecutive 32-byte records - and the row's two
//                        table operands of atom ID_k, and evaluates f2_value, the one expression mfx_rot2d_rotate and
//                        the fits share: a predicted column has rotate_cols' bits.  The compartments are added in the
//                        order f0, f1, f2, csf, every step one rounded operation (-ffp-contract=off), and 64
//                        consecutive doubles are stored per wave instruction.
//                        Residual: the lanes keep partial sums over their rows, a fixed xor butterfly over the 64 lanes
//                        adds them - the order depends on M alone, not on the grid.  R2 needs the means first, so a
//                        second sweep re-reads the row this wave has just written (L2 hits) and Y.
#include "fit2d_shared.h"
#include "sos_shared.h"
#include "../../include/mfx_predict.h"
#include "../../include/mfx_predict2d.h"

#include <algorithm>
#include <cmath>

namespace {

constexpr int P2_WG = 256;
constexpr int P2_WAVES = P2_WG / 64;
constexpr int P2_MAXF = 3;   // mfx_fit2d_batch's limit on maxfasc

struct P2Args {
  const double* base;     // the handle's knot values (Rot2dDev::ky): the records' offsets are relative to it
  const F2Rec* rec;       // [V KR x M]
  const int* pstat;       // [V KR x 4] the directions' records of the plan
  const double* params;   // [V x np]
  const double* sig_csf;  // [M]
  const double* Y;        // [V x M] or null
  const double* sigma;    // per sigma_mode (ncoils > 0)
  double* out;            // [V x M]
  double* stats;          // [V x 2] (Y given)
  int* status;            // [2]
  int* dstat;             // [V x 5]
  int64_t V;
  unsigned long long seed, offset;
  int M, N, np, maxfasc, KR, csf_on, sigma_mode, ncoils;
};

template <bool NOISE, bool RESID>
__global__ __launch_bounds__(P2_WG) void mfx_predict2d_kernel(P2Args a) {
  const int lane = threadIdx.x & 63;
  const int M = a.M, N = a.N, F = a.maxfasc;
  const int64_t nwaves = (int64_t)gridDim.x * P2_WAVES;
  const double qnan = __longlong_as_double(0x7ff8000000000000LL);
  for (int64_t v = (int64_t)blockIdx.x * P2_WAVES + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6); v < a.V; v += nwaves) {
    const double* __restrict__ pr = a.params + v * a.np;
    const double M0 = pr[0];
    int bad = 0;
    int drec[5] = {0, 0, 0, 0, 0};   // the lowest present fascicle whose direction fails
    double w[P2_MAXF];
    int id[P2_MAXF];
#pragma unroll
    for (int k = 0; k < P2_MAXF; ++k) {
      w[k] = 0.0; id[k] = 0;
      if (k < F) {
        const double wk = M0 * pr[1 + k];
        if (!(wk >= 0.0) || isinf(wk)) bad |= MFX_PRED_ST_WEIGHT;
        else if (wk > 0.0) {   // a zero weight: direction and ID are not looked at
          const double idd = pr[1 + F + k];
          if (!(idd >= 0.0 && idd < (double)N && idd == floor(idd)) || k >= a.KR) bad |= MFX_PRED_ST_ID;
          else {
            w[k] = wk; id[k] = (int)idd;
            const int* __restrict__ s = a.pstat + 4 * (v * a.KR + k);
            if (s[0] != MFX_ROT2D_OK && drec[0] == 0) { drec[0] = s[0]; drec[1] = s[1]; drec[2] = s[2]; drec[3] = s[3]; drec[4] = k; }
          }
        }
      }
    }
    double wc = 0.0;
    if (a.csf_on) {
      const double x = M0 * pr[1 + 2 * F];
      if (!(x >= 0.0) || isinf(x)) bad |= MFX_PRED_ST_WEIGHT; else wc = x;
    }
    if (lane == 0) {
      if (bad) {
        atomicOr(a.status, bad);
        a.status[1] = (int)v;
      }
#pragma unroll
      for (int q = 0; q < 5; ++q) a.dstat[5 * v + q] = drec[q];
    }
    const bool nanrow = bad != 0 || drec[0] != 0;
    double sg = 0.0;
    if (NOISE && a.sigma_mode != MFX_SIGMA_ELEMENT) sg = a.sigma[a.sigma_mode == MFX_SIGMA_VOXEL ? v : 0];
    double* __restrict__ o = a.out + v * M;
    const double* __restrict__ y = RESID ? a.Y + v * M : nullptr;
    const F2Rec* __restrict__ rv = a.rec + (size_t)v * a.KR * M;
    double rss = 0.0, sy = 0.0, so = 0.0;
    for (int m = lane; m < M; m += 64) {
      double acc = 0.0;
      if (nanrow) acc = qnan;
      else {
#pragma unroll
        for (int k = 0; k < P2_MAXF; ++k)
          if (w[k] > 0.0) {
            const F2Rec r = rv[(size_t)k * M + m];
            acc = acc + w[k] * f2_value(a.base, r, id[k]);
          }
        if (wc > 0.0) acc = acc + wc * a.sig_csf[m];
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
        a.stats[2 * v + 1] = nanrow ? qnan : R2;
      }
    }
  }
}

// what both entry points check before anything else
int p2_check_args(const char* fn, const mfx_rot2d* h, const void* params, const void* peaks, int maxfasc, int csf_on,
                  const void* sig_csf, int64_t V, const void* Y, const void* sigma, int sigma_mode, int ncoils, const void* out,
                  const void* stats, const void* dir_status) {
  if (!h || V < 0 || (V > 0 && (!params || !out || !dir_status))) return mfx_fail(MFX_ERR_ARG, "%s: bad argument", fn);
  if (maxfasc < 0) return mfx_fail(MFX_ERR_ARG, "%s: maxfasc must not be negative", fn);
  if (maxfasc > P2_MAXF) return mfx_fail(MFX_ERR_UNSUPPORTED, "%s: at most %d fascicles (got %d)", fn, P2_MAXF, maxfasc);
  if (h->d.M > R2_MAX_ROWS) return mfx_fail(MFX_ERR_UNSUPPORTED, "%s: more than %d protocol rows", fn, R2_MAX_ROWS);
  if (V > 0 && maxfasc > 0 && !peaks) return mfx_fail(MFX_ERR_ARG, "%s: peaks is null but maxfasc = %d", fn, maxfasc);
  if (csf_on && !sig_csf) return mfx_fail(MFX_ERR_ARG, "%s: csf_on without sig_csf", fn);
  if (ncoils < 0) return mfx_fail(MFX_ERR_ARG, "%s: ncoils must not be negative", fn);
  if (ncoils > 0 && (!sigma || sigma_mode < MFX_SIGMA_SCALAR || sigma_mode > MFX_SIGMA_ELEMENT))
    return mfx_fail(MFX_ERR_ARG, "%s: noise needs sigma and a sigma_mode of 0, 1 or 2", fn);
  if (V > 0 && Y && !stats) return mfx_fail(MFX_ERR_ARG, "%s: Y without stats", fn);
  return MFX_OK;
}

unsigned p2_grid(int64_t V) {   // memory-bound, grid-stride: a few workgroups per CU
  return (unsigned)std::min<int64_t>((V + P2_WAVES - 1) / P2_WAVES, 256 * 16);
}

}  // namespace

// The kernel on prepared records (rot2d_shared.h): d_rec [V KR x M] and d_pstat [V KR x 4] are those of the V KR directions,
// KR fascicle slots per voxel (fascicle k of a parameter row reads slot k; KR <= maxfasc).  Only enqueues.
int mfx_predict2d_launch(const mfx_rot2d* h, const void* d_rec, const int* d_pstat, int KR, const double* d_params, int maxfasc,
                         int csf_on, const double* d_sig_csf, int64_t V, const double* d_Y, const double* d_sigma, int sigma_mode,
                         int ncoils, uint64_t seed, uint64_t offset, double* d_out, double* d_stats, int32_t* d_status,
                         int32_t* d_dir_status, hipStream_t st) {
  if (V <= 0) return MFX_OK;
  P2Args a{};
  a.base = h->d.ky; a.rec = (const F2Rec*)d_rec; a.pstat = d_pstat; a.params = d_params; a.sig_csf = d_sig_csf; a.Y = d_Y;
  a.sigma = d_sigma; a.out = d_out; a.stats = d_stats; a.status = d_status; a.dstat = d_dir_status; a.V = V;
  a.seed = seed; a.offset = offset; a.M = h->d.M; a.N = h->d.N; a.np = 1 + 2 * maxfasc + (csf_on ? 1 : 0) + 2;
  a.maxfasc = maxfasc; a.KR = KR; a.csf_on = csf_on ? 1 : 0; a.sigma_mode = sigma_mode; a.ncoils = ncoils;
  const dim3 grid(p2_grid(V)), wg(P2_WG);
  if (ncoils > 0 && d_Y) hipLaunchKernelGGL((mfx_predict2d_kernel<true, true>), grid, wg, 0, st, a);
  else if (ncoils > 0) hipLaunchKernelGGL((mfx_predict2d_kernel<true, false>), grid, wg, 0, st, a);
  else if (d_Y) hipLaunchKernelGGL((mfx_predict2d_kernel<false, true>), grid, wg, 0, st, a);
  else hipLaunchKernelGGL((mfx_predict2d_kernel<false, false>), grid, wg, 0, st, a);
  HIPCHK(hipGetLastError());
  return MFX_OK;
}

extern "C" int mfx_predict2d_abi_version(void) { return 1; }

extern "C" int mfx_predict2d_dev(void* hv, const double* d_params, const double* d_peaks, int maxfasc, int csf_on,
                                 const double* d_sig_csf, int64_t V, const double* d_Y, const double* d_sigma, int sigma_mode,
                                 int ncoils, uint64_t seed, uint64_t offset, double* d_out, double* d_stats, int32_t* d_status,
                                 int32_t* d_dir_status, void* stream) {
  const char* fn = "mfx_predict2d_dev";
  if (mfx_device_count() <= 0) return mfx_no_device();
  const mfx_rot2d* h = (const mfx_rot2d*)hv;
  if (int rc = p2_check_args(fn, h, d_params, d_peaks, maxfasc, csf_on, d_sig_csf, V, d_Y, d_sigma, sigma_mode, ncoils, d_out,
                             d_stats, d_dir_status)) return rc;
  if (V > 0 && !d_status) return mfx_fail(MFX_ERR_ARG, "%s: d_status is null", fn);
  if (V == 0) return MFX_OK;
  if (int rc = f2_limits(fn, h, maxfasc, V)) return rc;
  if (int rc = mfx_require_device(h->device)) return rc;
  hipStream_t st = (hipStream_t)stream;
  F2Dirs dirs(st);
  if (int rc = dirs.enqueue(h, d_peaks, V * maxfasc, st)) return rc;
  return mfx_predict2d_launch(h, dirs.rec.p, dirs.pstat.as<int>(), maxfasc, d_params, maxfasc, csf_on, d_sig_csf, V, d_Y, d_sigma,
                              sigma_mode, ncoils, seed, offset, d_out, d_stats, d_status, d_dir_status, st);
}

extern "C" int mfx_predict2d(void* hv, const double* params, const double* peaks, int maxfasc, int csf_on, const double* sig_csf,
                             int64_t V, const double* Y, const double* sigma, int sigma_mode, int ncoils, uint64_t seed,
                             uint64_t offset, double* out, double* stats, int32_t* dir_status) {
  const char* fn = "mfx_predict2d";
  if (mfx_device_count() <= 0) return mfx_no_device();
  const mfx_rot2d* h = (const mfx_rot2d*)hv;
  if (int rc = p2_check_args(fn, h, params, peaks, maxfasc, csf_on, sig_csf, V, Y, sigma, sigma_mode, ncoils, out, stats,
                             dir_status)) return rc;
  if (V == 0) return MFX_OK;
  csf_on = csf_on != 0;
  const int np = 1 + 2 * maxfasc + csf_on + 2, M = h->d.M, N = h->d.N;
  for (int64_t v = 0; v < V; ++v) {   // the argument errors the device entry point can only flag
    const double* pr = params + v * np;
    for (int c = 0; c < maxfasc + csf_on; ++c) {
      const bool fasc = c < maxfasc;
      const double w = pr[0] * pr[fasc ? 1 + c : 1 + 2 * maxfasc];
      if (!(w >= 0.0) || std::isinf(w))
        return mfx_fail(MFX_ERR_ARG, "%s: voxel %lld: weight M0 * nu = %g of compartment %d is negative or not finite", fn,
                        (long long)v, w, c);
      if (w > 0.0 && fasc) {
        const double id = pr[1 + maxfasc + c];
        if (!(id >= 0.0 && id < (double)N && id == std::floor(id)))
          return mfx_fail(MFX_ERR_ARG, "%s: voxel %lld: atom index %g of compartment %d is not an integer in [0, %d)", fn,
                          (long long)v, id, c, N);
      }
    }
  }
  if (int rc = mfx_require_device(h->device)) return rc;
  const size_t VM = (size_t)V * M;
  const size_t n_sigma = ncoils > 0 ? (sigma_mode == MFX_SIGMA_SCALAR ? 1 : (sigma_mode == MFX_SIGMA_VOXEL ? (size_t)V : VM)) : 0;
  DevMem dpar, dpk, dcsf, dY, dsig, dout, dstats, dst, dds;
  HIPCHK(dpar.alloc(sizeof(double) * V * np));
  HIPCHK(dpk.alloc(sizeof(double) * V * 3 * maxfasc));
  HIPCHK(dcsf.alloc(sizeof(double) * M));
  HIPCHK(dY.alloc(Y ? sizeof(double) * VM : 0));
  HIPCHK(dsig.alloc(sizeof(double) * n_sigma));
  HIPCHK(dout.alloc(sizeof(double) * VM));
  HIPCHK(dstats.alloc(sizeof(double) * 2 * V));
  HIPCHK(dst.alloc(2 * sizeof(int)));
  HIPCHK(dds.alloc(sizeof(int32_t) * 5 * V));
  HIPCHK(hipMemcpy(dpar.p, params, sizeof(double) * V * np, hipMemcpyHostToDevice));
  if (maxfasc > 0) HIPCHK(hipMemcpy(dpk.p, peaks, sizeof(double) * V * 3 * maxfasc, hipMemcpyHostToDevice));
  if (csf_on) HIPCHK(hipMemcpy(dcsf.p, sig_csf, sizeof(double) * M, hipMemcpyHostToDevice));
  if (Y) HIPCHK(hipMemcpy(dY.p, Y, sizeof(double) * VM, hipMemcpyHostToDevice));
  if (n_sigma) HIPCHK(hipMemcpy(dsig.p, sigma, sizeof(double) * n_sigma, hipMemcpyHostToDevice));
  HIPCHK(hipMemset(dst.p, 0, 2 * sizeof(int)));
  if (int rc = mfx_predict2d_dev(hv, dpar.as<double>(), maxfasc > 0 ? dpk.as<double>() : nullptr, maxfasc, csf_on,
                                 csf_on ? dcsf.as<double>() : nullptr, V, Y ? dY.as<double>() : nullptr,
                                 n_sigma ? dsig.as<double>() : nullptr, sigma_mode, ncoils, seed, offset, dout.as<double>(),
                                 dstats.as<double>(), dst.as<int32_t>(), dds.as<int32_t>(), nullptr)) return rc;
  HIPCHK(hipStreamSynchronize(nullptr));
  int st[2] = {0, 0};
  HIPCHK(hipMemcpy(st, dst.p, sizeof(st), hipMemcpyDeviceToHost));
  if (st[0]) return mfx_fail(MFX_ERR_ARG, "%s: the kernel flagged status 0x%x in voxel %d", fn, st[0], st[1]);
  HIPCHK(hipMemcpy(out, dout.p, sizeof(double) * VM, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(dir_status, dds.p, sizeof(int32_t) * 5 * V, hipMemcpyDeviceToHost));
  if (Y) HIPCHK(hipMemcpy(stats, dstats.p, sizeof(double) * 2 * V, hipMemcpyDeviceToHost));
  return MFX_OK;
}
