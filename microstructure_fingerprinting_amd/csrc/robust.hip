// robust.hip -- robust fits (include/mfx_robust.h): measurement weights from the residuals of a fit, and the loop
// fit -> predict -> reweight -> weighted fit on device-resident data.  The fits and the prediction are the class
// launchers of mfx_api.hip (unweighted), fit_w.hip (weighted) and predict.hip; what is new here is one kernel.  The loop
// itself is mfx_rob_iterate (mfx_host.h) over the three steps below; the host side of a mixed batch is class_batch.h.
//
// mfx_robust_weights_kernel   One wave per voxel, ROB_WAVES(M) voxels per workgroup (a wave beyond the batch idles
//                        through the barriers).  Lane l owns the rows l, l + 64, ...
//   pass 1  a_m = |fl(y_m - p_m)| of the rows of B = {W0 > 0}, packed in row order into the wave's LDS slice (ballot
//           prefix: the packed position of a row is the number of rows of B before it, so the packed index orders
//           ties as the row index does); the flags of states 3 and 1.
//   pass 2  rank counting: the rank of packed element i is #{j : a_j < a_i or (a_j == a_i and j < i)} - a total order,
//           so exactly one element has rank (n0 - 1) / 2 and one has rank n0 / 2.  Every lane counts the ranks of its
//           elements against all n0 (the a_j are LDS broadcasts), n0^2 / 64 comparisons per lane; the two order
//           statistics reach all lanes through a ballot and a shuffle.  No sort, no atomics, one fixed result.
//   pass 3  s, thr, psi and the weights in the order of operations of mfx_robust.h (the build has -ffp-contract=off,
//           every line below is one rounding); W, scale, state, changed with plain vector stores.
// LDS: 8 M bytes per wave, at most 64 KB per workgroup: 4 waves up to M = 2048, 3 up to 2730, 2 up to 4096, 1 up to
// 8192 rows.
#include "mfx_host.h"
#include "../../include/mfx_predict.h"
#include "../../include/mfx_robust.h"

#include <algorithm>
#include <cstring>
#include <vector>

namespace {

constexpr int ROB_MAX_ROWS = 8192;            // the weighted fit's limit; 8 M bytes of LDS per wave
constexpr size_t ROB_LDS_MAX = 64 * 1024;
constexpr double ROB_DBL_MAX = 1.79769313486231570815e308;

inline int rob_waves(int M) { return (int)std::max<size_t>(1, std::min<size_t>(4, ROB_LDS_MAX / (sizeof(double) * (size_t)M))); }

struct RobArgs {
  const double* Y;       // [V x M]
  const double* P;       // [V x M]
  const double* W0;      // [V x M], [M] or null
  int64_t w0_stride;     // M or 0
  const double* Wprev;   // [V x M] or null; may be W
  double* W;             // [V x M]
  double* scale;         // [V]
  int* state;            // [V]
  int* changed;          // [V] or null
  int64_t V;
  int M, loss;
  double c;
};

__global__ __launch_bounds__(256) void mfx_robust_weights_kernel(RobArgs a) {
  extern __shared__ double s_all[];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int nw = blockDim.x >> 6;
  const int M = a.M;
  const int64_t v = (int64_t)blockIdx.x * nw + wave;
  const bool live = v < a.V;   // wave-uniform; an idle wave only takes part in the barrier
  double* s_a = s_all + (size_t)wave * M;
  const double* __restrict__ y = a.Y + (live ? v : 0) * M;
  const double* __restrict__ p = a.P + (live ? v : 0) * M;
  const double* w0 = a.W0 ? a.W0 + (live ? v : 0) * a.w0_stride : nullptr;
  const double qnan = __longlong_as_double(0x7ff8000000000000LL);

  // ---- pass 1: pack a over B, flag unusable base weights and residuals that are not finite
  int n0 = 0;
  bool badw = false, bada = false;
  if (live) {
    for (int base = 0; base < M; base += 64) {
      const int m = base + lane;
      bool inB = false;
      double am = 0.0;
      if (m < M) {
        const double w = w0 ? w0[m] : 1.0;
        badw |= !(w >= 0.0) || !(w <= ROB_DBL_MAX);
        inB = w > 0.0;
        const double r = y[m] - p[m];
        am = fabs(r);
        bada |= inB && !(am <= ROB_DBL_MAX);
      }
      const unsigned long long mk = __ballot(inB);
      if (inB) s_a[n0 + __popcll(mk & ((1ull << lane) - 1ull))] = am;
      n0 += __popcll(mk);
    }
    badw = __ballot(badw) != 0ull;
    bada = __ballot(bada) != 0ull;
  }
  __syncthreads();
  if (!live) return;

  int st = 0;
  if (badw || n0 == 0) st = 3;
  else if (bada) st = 1;

  // ---- pass 2: the order statistics of rank k1 = (n0 - 1) / 2 and k2 = n0 / 2 by rank counting
  double s = qnan;
  if (st == 0) {
    const int k1 = (n0 - 1) >> 1, k2 = n0 >> 1;
    double v1 = 0.0, v2 = 0.0;
    bool h1 = false, h2 = false;
    for (int i = lane; i < n0; i += 64) {
      const double ai = s_a[i];
      int rank = 0;
      for (int j = 0; j < n0; ++j) {
        const double aj = s_a[j];
        rank += (aj < ai || (aj == ai && j < i)) ? 1 : 0;
      }
      if (rank == k1) { v1 = ai; h1 = true; }
      if (rank == k2) { v2 = ai; h2 = true; }
    }
    const unsigned long long b1 = __ballot(h1), b2 = __ballot(h2);   // one lane each
    const double lo = __shfl(v1, __ffsll((long long)b1) - 1, 64);
    const double hi = __shfl(v2, __ffsll((long long)b2) - 1, 64);
    if (n0 & 1) s = lo;
    else {
      const double sum = lo + hi;
      s = sum / 2.0;
    }
    if (s == 0.0) st = 2;
  }

  // ---- pass 3: the weights
  const double thr = a.c * s;
  const double* wp = a.Wprev ? a.Wprev + v * M : nullptr;
  double* wo = a.W + v * M;
  bool chg = false;
  for (int m = lane; m < M; m += 64) {
    const double w = w0 ? w0[m] : 1.0;
    double out = w;   // a non-zero state: the base weights as they are
    if (st == 0) {
      if (w > 0.0) {
        const double r = y[m] - p[m];
        const double am = fabs(r);
        double psi;
        if (a.loss == MFX_ROBUST_CUTOFF) psi = am <= thr ? 1.0 : 0.0;
        else if (a.loss == MFX_ROBUST_HUBER) psi = am <= thr ? 1.0 : thr / am;
        else {
          const double u = am / thr;
          const double uu = u * u;
          const double t = 1.0 - uu;
          psi = u < 1.0 ? t * t : 0.0;
        }
        out = w0 ? w * psi : psi;
      } else {
        out = 0.0;
      }
    }
    if (wp) chg |= __double_as_longlong(wp[m]) != __double_as_longlong(out);   // (read before the store: Wprev may be W)
    wo[m] = out;
  }
  chg = __ballot(chg) != 0ull;
  if (lane == 0) {
    a.scale[v] = s;
    a.state[v] = st;
    if (a.changed) a.changed[v] = chg ? 1 : 0;
  }
}

// W = W0 spread to [V x M] (ones without W0): the weights before the first iteration
__global__ __launch_bounds__(256) void rob_spread_kernel(const double* __restrict__ W0, int64_t w0_stride, int M, int64_t V,
                                                        double* __restrict__ W) {
  const int64_t n = V * M, step = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += step) {
    const int64_t v = i / M;
    W[i] = W0 ? W0[v * w0_stride + (i - v * M)] : 1.0;
  }
}

// *out = number of non-zero flags, by one workgroup in a fixed order
__global__ __launch_bounds__(256) void rob_count_kernel(const int* __restrict__ flags, int64_t V, int* __restrict__ out) {
  __shared__ int s_n[256];
  int n = 0;
  for (int64_t i = threadIdx.x; i < V; i += 256) n += flags[i] != 0;
  s_n[threadIdx.x] = n;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) s_n[threadIdx.x] += s_n[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) *out = s_n[0];
}

int rob_check_rule(const char* fn, int loss, double c, int M) {
  if (loss != MFX_ROBUST_CUTOFF && loss != MFX_ROBUST_HUBER && loss != MFX_ROBUST_TUKEY)
    return mfx_fail(MFX_ERR_ARG, "%s: loss should be 0 (cutoff), 1 (huber) or 2 (tukey), got %d", fn, loss);
  if (!(c >= 1.0) || !(c <= ROB_DBL_MAX)) return mfx_fail(MFX_ERR_ARG, "%s: c should be a finite number >= 1, got %g", fn, c);
  if (M < 1) return mfx_fail(MFX_ERR_ARG, "%s: M should be positive, got %d", fn, M);
  if (M > ROB_MAX_ROWS) return mfx_fail(MFX_ERR_UNSUPPORTED, "%s: more than %d measurements (got %d)", fn, ROB_MAX_ROWS, M);
  return MFX_OK;
}

int rob_launch_weights(int M, const double* d_Y, const double* d_P, const double* d_W0, int64_t w0_stride, int loss, double c,
                       int64_t V, const double* d_Wprev, double* d_W, double* d_scale, int32_t* d_state, int32_t* d_changed,
                       hipStream_t st) {
  RobArgs a{};
  a.Y = d_Y; a.P = d_P; a.W0 = d_W0; a.w0_stride = d_W0 ? w0_stride : 0; a.Wprev = d_Wprev; a.W = d_W;
  a.scale = d_scale; a.state = d_state; a.changed = d_changed; a.V = V; a.M = M; a.loss = loss; a.c = c;
  const int nw = rob_waves(M);
  const int64_t blocks = (V + nw - 1) / nw;
  if (blocks > 0x7fffffff) return mfx_fail(MFX_ERR_ARG, "mfx_robust: V too large for one launch");
  hipLaunchKernelGGL(mfx_robust_weights_kernel, dim3((unsigned)blocks), dim3(64 * nw), sizeof(double) * (size_t)M * nw, st, a);
  HIPCHK(hipGetLastError());
  return MFX_OK;
}

unsigned rob_grid(int64_t items) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>((items + 255) / 256, 256 * 16)); }

// One class on device buffers: V voxels of K fascicles (d_peaksK [V x 3 K]; d_peaksF [V x 3 maxfasc], the same
// directions in the layout of the parameter rows, for the prediction), with the CSF column d_xc or without (null);
// d_params [V x np] (np = 1 + 2 maxfasc + csf_on + 2); d_sig_csf [M] is the CSF signal of the batch (csf_on), which the
// prediction of every class needs.  The loop is rob_first_fit, then per iteration rob_reweight and the weighted fit
// (rob_refit); all three only enqueue.
struct RobClass {
  const mfx_plan* p;
  const double *Y, *W0;
  int64_t w0_stride;
  const double *peaksK, *peaksF;
  int K;
  const double *xc, *sig_csf;
  int maxfasc, csf_on, loss;
  double c;
  int64_t V;
  double *params, *W, *scale;
  int32_t *state, *status, *nchanged;
  hipStream_t st;
};

// fit 0 (unweighted without W0, else weighted on W0), W = W0 spread (ones), scale and state zero
int rob_first_fit(const RobClass& r) {
  TablesDev T;
  PlanDev P;
  int device = 0;
  mfx_plan_view(r.p, &T, &P, &device);
  const int M = P.M, np = 1 + 2 * r.maxfasc + r.csf_on + 2;
  if (int rc = mfx_rob_spread(r.W0, r.w0_stride, M, r.V, r.W, r.st)) return rc;
  HIPCHK(hipMemsetAsync(r.scale, 0, sizeof(double) * (size_t)r.V, r.st));
  HIPCHK(hipMemsetAsync(r.state, 0, sizeof(int32_t) * (size_t)r.V, r.st));
  if (r.W0) return mfx_wfit_class_dev(r.p, r.Y, r.W0, r.w0_stride, r.peaksK, r.K, r.xc, r.maxfasc, r.csf_on, r.V, r.params, r.status, r.st);
  HIPCHK(hipMemsetAsync(r.params, 0, sizeof(double) * (size_t)r.V * np, r.st));
  HIPCHK(hipMemsetAsync(r.status, 0, sizeof(int32_t) * (size_t)r.V, r.st));
  return mfx_fit_class_plain_dev(r.p, r.Y, r.peaksK, r.K, r.xc, r.maxfasc, r.csf_on, r.V, r.params, r.st);
}

// iteration `it` up to its fit: prediction -> weights in place on W -> nchanged[it].  Its scratch is given back before
// it returns - the fit that follows comes behind it on the stream and may use the same addresses - so the stream's
// arena rewinds between the steps and does not grow with the number of iterations.
int rob_reweight(const RobClass& r, int it) {
  TablesDev T;
  PlanDev P;
  int device = 0;
  mfx_plan_view(r.p, &T, &P, &device);
  const int M = P.M;
  StreamMem pred(r.st), chg(r.st), pst(r.st);
  HIPCHK(pred.alloc(sizeof(double) * (size_t)r.V * M));
  HIPCHK(chg.alloc(sizeof(int) * (size_t)r.V));
  HIPCHK(pst.alloc(2 * sizeof(int)));
  HIPCHK(hipMemsetAsync(pst.p, 0, 2 * sizeof(int), r.st));   // a row the fit could not serve is flagged there and predicted as NaN: state 1
  if (int rc = mfx_predict_dev(r.p, r.params, r.maxfasc > 0 ? r.peaksF : nullptr, r.maxfasc, r.csf_on, 0, r.csf_on ? r.sig_csf : nullptr,
                               nullptr, 0, r.V, nullptr, nullptr, 0, 0, 0, 0, pred.as<double>(), nullptr, pst.as<int32_t>(), r.st)) return rc;
  if (int rc = rob_launch_weights(M, r.Y, pred.as<double>(), r.W0, r.w0_stride, r.loss, r.c, r.V, r.W, r.W, r.scale, r.state, chg.as<int>(),
                                  r.st)) return rc;
  return mfx_rob_count(chg.as<int>(), r.V, r.nchanged + it, r.st);
}

// the weighted fit on the current W
int rob_refit(const RobClass& r) {
  TablesDev T;
  PlanDev P;
  int device = 0;
  mfx_plan_view(r.p, &T, &P, &device);
  return mfx_wfit_class_dev(r.p, r.Y, r.W, P.M, r.peaksK, r.K, r.xc, r.maxfasc, r.csf_on, r.V, r.params, r.status, r.st);
}

// the loop's steps for mfx_rob_iterate (mfx_host.h); the steps give their scratch back themselves
struct RobSteps {
  const RobClass& r;
  int first_fit() const { return rob_first_fit(r); }
  int reweight(int it) const { return rob_reweight(r, it); }
  int refit() const { return rob_refit(r); }
  void step_done() const {}
};

}  // namespace

// what robust2d.hip shares of this file (mfx_host.h)
int mfx_rob_check_rule(const char* fn, int loss, double c, int M) { return rob_check_rule(fn, loss, c, M); }

int mfx_rob_launch_weights(int M, const double* d_Y, const double* d_P, const double* d_W0, int64_t w0_stride, int loss, double c,
                           int64_t V, const double* d_Wprev, double* d_W, double* d_scale, int32_t* d_state, int32_t* d_changed,
                           hipStream_t st) {
  return rob_launch_weights(M, d_Y, d_P, d_W0, w0_stride, loss, c, V, d_Wprev, d_W, d_scale, d_state, d_changed, st);
}

int mfx_rob_spread(const double* d_W0, int64_t w0_stride, int M, int64_t V, double* d_W, hipStream_t st) {
  hipLaunchKernelGGL(rob_spread_kernel, dim3(rob_grid(V * M)), dim3(256), 0, st, d_W0, w0_stride, M, V, d_W);
  HIPCHK(hipGetLastError());
  return MFX_OK;
}

int mfx_rob_count(const int* d_flags, int64_t V, int* d_out, hipStream_t st) {
  hipLaunchKernelGGL(rob_count_kernel, dim3(1), dim3(256), 0, st, d_flags, V, d_out);
  HIPCHK(hipGetLastError());
  return MFX_OK;
}

extern "C" int mfx_robust_abi_version(void) { return 1; }

extern "C" int mfx_robust_weights_dev(int M, const double* d_Y, const double* d_P, const double* d_W0, int64_t w0_stride, int loss,
                                      double c, int64_t V, const double* d_Wprev, double* d_W, double* d_scale, int32_t* d_state,
                                      int32_t* d_changed, void* stream) {
  const char* fn = "mfx_robust_weights_dev";
  if (mfx_device_count() <= 0) return mfx_no_device();
  if (V < 0 || (V > 0 && (!d_Y || !d_P || !d_W || !d_scale || !d_state))) return mfx_fail(MFX_ERR_ARG, "%s: bad argument", fn);
  if (int rc = rob_check_rule(fn, loss, c, M)) return rc;
  if (d_W0 && w0_stride != 0 && w0_stride != M)
    return mfx_fail(MFX_ERR_ARG, "%s: w0_stride should be M = %d or 0 (got %lld)", fn, M, (long long)w0_stride);
  if (V == 0) return MFX_OK;
  return rob_launch_weights(M, d_Y, d_P, d_W0, w0_stride, loss, c, V, d_Wprev, d_W, d_scale, d_state, d_changed, (hipStream_t)stream);
}

extern "C" int mfx_rfit_batch_dev(const void* pv, const double* d_Y, const double* d_W0, int64_t w0_stride, const double* d_peaks,
                                  int maxfasc, int loss, double c, int n_iter, int64_t V, double* d_params, double* d_W,
                                  double* d_scale, int32_t* d_state, int32_t* d_status, int32_t* d_nchanged, void* stream) {
  const char* fn = "mfx_rfit_batch_dev";
  if (mfx_device_count() <= 0) return mfx_no_device();
  const mfx_plan* p = (const mfx_plan*)pv;
  if (!p || V < 0 || maxfasc < 0 || n_iter < 0 ||
      (V > 0 && (!d_Y || !d_params || !d_W || !d_scale || !d_state || !d_status || (maxfasc > 0 && !d_peaks) || (n_iter > 0 && !d_nchanged))))
    return mfx_fail(MFX_ERR_ARG, "%s: bad argument", fn);
  if (maxfasc > 3) return mfx_fail(MFX_ERR_UNSUPPORTED, "%s: at most 3 fascicles (got %d)", fn, maxfasc);
  TablesDev T;
  PlanDev P;
  int device = 0;
  mfx_plan_view(p, &T, &P, &device);
  if (int rc = rob_check_rule(fn, loss, c, P.M)) return rc;
  if (d_W0 && w0_stride != 0 && w0_stride != P.M)
    return mfx_fail(MFX_ERR_ARG, "%s: w0_stride should be M = %d or 0 (got %lld)", fn, P.M, (long long)w0_stride);
  if (V > 0x7fffffff) return mfx_fail(MFX_ERR_ARG, "%s: V too large for one launch", fn);
  if (int rc = mfx_require_device(device)) return rc;
  hipStream_t st = (hipStream_t)stream;
  if (V == 0) {
    if (n_iter > 0) HIPCHK(hipMemsetAsync(d_nchanged, 0, sizeof(int32_t) * (size_t)n_iter, st));
    return MFX_OK;
  }
  const RobClass r{p, d_Y, d_W0, d_W0 ? w0_stride : 0, d_peaks, d_peaks, maxfasc, nullptr, nullptr, maxfasc, 0, loss, c, V,
                   d_params, d_W, d_scale, d_state, d_status, d_nchanged, st};
  return mfx_rob_iterate(RobSteps{r}, n_iter, nullptr);
}

extern "C" int mfx_rfit_batch(const void* pv, const double* Y, const double* W0, int64_t w0_stride, const int32_t* K,
                              const uint8_t* csf, const double* peaks, int maxfasc, int csf_on, const double* sig_csf, int loss,
                              double c, int n_iter, int64_t V, double* params, double* W_out, double* scale, int32_t* state,
                              int32_t* status, int64_t* n_changed, int32_t* n_iter_used) {
  const char* fn = "mfx_rfit_batch";
  if (mfx_device_count() <= 0) return mfx_no_device();
  const mfx_plan* p = (const mfx_plan*)pv;
  if (!p || V < 0 || maxfasc < 0 || n_iter < 0 || !n_iter_used || (n_iter > 0 && !n_changed) ||
      (V > 0 && (!Y || !K || !params || !W_out || !scale || !state || !status || (maxfasc > 0 && !peaks))))
    return mfx_fail(MFX_ERR_ARG, "%s: bad argument", fn);
  if (maxfasc > 3) return mfx_fail(MFX_ERR_UNSUPPORTED, "%s: at most 3 fascicles (got %d)", fn, maxfasc);
  csf_on = csf_on != 0;
  TablesDev T;
  PlanDev P;
  int device = 0;
  mfx_plan_view(p, &T, &P, &device);
  const int M = P.M, np = 1 + 2 * maxfasc + csf_on + 2;
  if (int rc = rob_check_rule(fn, loss, c, M)) return rc;
  if (W0 && w0_stride != 0 && w0_stride != M)
    return mfx_fail(MFX_ERR_ARG, "%s: w0_stride should be M = %d or 0 (got %lld)", fn, M, (long long)w0_stride);
  if (!W0) w0_stride = 0;
  if (csf_on && !sig_csf) return mfx_fail(MFX_ERR_ARG, "%s: csf_on without sig_csf", fn);   // (the prediction of every class needs it)
  // bin by class (K, CSF flag) before any device call
  MfxClassBins bins;
  if (int rc = mfx_class_bins(fn, K, csf, maxfasc, csf_on && sig_csf, V, &bins)) return rc;
  *n_iter_used = 0;
  for (int it = 0; it < n_iter; ++it) n_changed[it] = 0;
  if (V == 0) return MFX_OK;
  if (int rc = mfx_require_device(device)) return rc;
  DevBuf<double> dxc, dW0s;
  DevBuf<int32_t> dnc;
  if (sig_csf) HIPCHK(dxc.upload(sig_csf, M));
  if (W0 && w0_stride == 0) HIPCHK(dW0s.upload(W0, M));   // the shared vector is uploaded once
  HIPCHK(dnc.alloc_n((size_t)std::max(n_iter, 1)));
  const size_t chunk = mfx_rfit_upload_chunk(M);   // voxels per upload: Y, W0, W, prediction
  return mfx_class_walk(bins, chunk, [&](int k, int cf, const int64_t* ix, size_t nv) -> int {
    DevBuf<double> dY, dW0, dW, dpK, dpF, dpr, dsc;
    DevBuf<int32_t> dstt, dst;
    HIPCHK(dY.upload_rows(Y, ix, nv, M, M));
    if (w0_stride) HIPCHK(dW0.upload_rows(W0, ix, nv, M, M));
    HIPCHK(mfx_upload_peaks(dpK, peaks, ix, nv, maxfasc, k));
    HIPCHK(mfx_upload_peaks(dpF, peaks, ix, nv, maxfasc, maxfasc));   // whole rows, the layout of the parameter rows
    HIPCHK(dW.alloc_n(nv * M));
    HIPCHK(dpr.alloc_n(nv * np));
    HIPCHK(dsc.alloc_n(nv));
    HIPCHK(dstt.alloc_n(nv));
    HIPCHK(dst.alloc_n(nv));
    const double* w0d = !W0 ? nullptr : (w0_stride ? dW0.get() : dW0s.get());
    const RobClass r{p, dY.get(), w0d, w0_stride, dpK.get(), dpF.get(), k, cf ? dxc.get() : nullptr, dxc.get(), maxfasc, csf_on, loss, c,
                     (int64_t)nv, dpr.get(), dW.get(), dsc.get(), dstt.get(), dst.get(), dnc.get(), nullptr};
    const MfxRobHostCount host{dnc.get(), W0 != nullptr, n_changed, n_iter_used};
    if (int rc = mfx_rob_iterate(RobSteps{r}, n_iter, &host)) return rc;
    HIPCHK(hipStreamSynchronize(nullptr));
    HIPCHK(dpr.download_rows(params, ix, nv, np));
    HIPCHK(dW.download_rows(W_out, ix, nv, M));
    HIPCHK(dsc.download_rows(scale, ix, nv, 1));
    HIPCHK(dstt.download_rows(state, ix, nv, 1));
    HIPCHK(dst.download_rows(status, ix, nv, 1));
    return MFX_OK;
  });
}
