// robust2d.hip -- robust fits of voxels of a 2-D (AxCaliber-like) protocol (include/mfx_robust2d.h): the loop
// fit -> predict -> reweight -> weighted fit of robust.hip on a handle of rotate2d.hip, on device-resident data.
// Nothing here computes: the fits are the class launchers of fit2d.hip (unweighted) and w2d.hip (weighted) on prepared
// directions, the prediction is the kernel of predict2d.hip on the same records, the rule is mfx_robust_weights_kernel
// of robust.hip.  What this file adds is the order of the launches - and that the plan of the class's directions and
// the kernels' 32-byte records (F2Dirs) are made once per class chunk, not once per fit and prediction.
#include "fit2d_shared.h"
#include "../../include/mfx_robust.h"
#include "../../include/mfx_robust2d.h"

#include <algorithm>
#include <cstring>
#include <vector>

namespace {

thread_local int64_t g_last_plan_dirs = 0;

const char* NO_DEVICE = "no HIP device available (this library has no CPU path)";

int r2d_require_device(int device) {
  const int n = mfx_device_count();
  if (n <= 0) return mfx_fail(MFX_ERR_NO_DEVICE, "%s", NO_DEVICE);
  if (device < 0 || device >= n) return mfx_fail(MFX_ERR_ARG, "device %d out of range (have %d)", device, n);
  HIPCHK(hipSetDevice(device));
  return MFX_OK;
}

// One class on device buffers: V voxels of K fascicles (d_peaksK [V x 3 K]), with the CSF column d_xc or without
// (null); d_params [V x np] (np = 1 + 2 maxfasc + csf_on + 2); d_sig_csf [M] is the CSF signal of the batch (csf_on),
// which the prediction of every class needs.  rec / pstat: the prepared directions of the class.
struct Rob2Class {
  const mfx_rot2d* h;
  const void* rec;
  const int* pstat;
  const double *Y, *W0;
  int64_t w0_stride;
  int K;
  const double *xc, *sig_csf;
  int maxfasc, csf_on, loss;
  double c;
  int64_t V;
  double *params, *W, *scale;
  int32_t *state, *vstat, *wstat, *nchanged;
  hipStream_t st;
};

// fit 0 (unweighted without W0, else weighted on W0), W = W0 spread (ones), scale and state zero
int r2d_first_fit(const Rob2Class& r) {
  const int M = r.h->d.M;
  if (int rc = mfx_rob_spread(r.W0, r.w0_stride, M, r.V, r.W, r.st)) return rc;
  HIPCHK(hipMemsetAsync(r.scale, 0, sizeof(double) * (size_t)r.V, r.st));
  HIPCHK(hipMemsetAsync(r.state, 0, sizeof(int32_t) * (size_t)r.V, r.st));
  if (r.W0)
    return mfx_wfit2d_class_prepared(r.h, r.Y, r.W0, r.w0_stride, r.rec, r.pstat, r.K, r.xc, r.maxfasc, r.csf_on, r.V, r.params,
                                     r.vstat, r.wstat, r.st);
  HIPCHK(hipMemsetAsync(r.wstat, 0, sizeof(int32_t) * (size_t)r.V, r.st));
  return mfx_fit2d_class_prepared(r.h, r.Y, r.rec, r.pstat, r.K, r.xc, r.maxfasc, r.csf_on, r.V, r.params, r.vstat, r.st);
}

// iteration `it` up to its fit: prediction -> weights in place on W -> nchanged[it].  Its scratch is given back before
// it returns - the fit that follows comes behind it on the stream and may use the same addresses.
int r2d_reweight(const Rob2Class& r, int it) {
  const int M = r.h->d.M;
  StreamMem pred(r.st), chg(r.st), pst(r.st);
  HIPCHK(pred.alloc(sizeof(double) * (size_t)r.V * M));
  HIPCHK(chg.alloc(sizeof(int) * (size_t)r.V));
  HIPCHK(pst.alloc(sizeof(int) * (2 + 5 * (size_t)r.V)));   // the prediction's status word and its own direction records
  HIPCHK(hipMemsetAsync(pst.p, 0, 2 * sizeof(int), r.st));   // a row the fit could not serve is flagged there and predicted as NaN: state 1
  if (int rc = mfx_predict2d_launch(r.h, r.rec, r.pstat, r.K, r.params, r.maxfasc, r.csf_on, r.csf_on ? r.sig_csf : nullptr, r.V, nullptr,
                                    nullptr, 0, 0, 0, 0, pred.as<double>(), nullptr, pst.as<int32_t>(), pst.as<int32_t>() + 2, r.st))
    return rc;
  if (int rc = mfx_rob_launch_weights(M, r.Y, pred.as<double>(), r.W0, r.w0_stride, r.loss, r.c, r.V, r.W, r.W, r.scale, r.state,
                                      chg.as<int>(), r.st)) return rc;
  return mfx_rob_count(chg.as<int>(), r.V, r.nchanged + it, r.st);
}

// the weighted fit on the current W
int r2d_refit(const Rob2Class& r) {
  return mfx_wfit2d_class_prepared(r.h, r.Y, r.W, r.h->d.M, r.rec, r.pstat, r.K, r.xc, r.maxfasc, r.csf_on, r.V, r.params, r.vstat,
                                   r.wstat, r.st);
}

// The directions' records stay allocated over the loop; every step behind them starts at the same place of the stream's
// arena (mfx_host.h), so the arena does not grow with the number of iterations.
struct StepScratch {
  hipStream_t st;
  ScratchMark mk;
  bool marked;
  explicit StepScratch(hipStream_t s) : st(s), marked(mfx_scratch_mark(s, &mk)) {}
  void done() const { if (marked) mfx_scratch_rewind(st, mk); }
};

struct PlanCount {   // the diagnostic of mfx_robust2d_debug_last_plan_directions, kept on every exit path
  PlanCount() { mfx_rot2d_plan_count_reset(); g_last_plan_dirs = 0; }
  ~PlanCount() { g_last_plan_dirs = mfx_rot2d_plan_count(); }
};

}  // namespace

extern "C" int mfx_robust2d_abi_version(void) { return 1; }

extern "C" int64_t mfx_robust2d_debug_last_plan_directions(void) { return g_last_plan_dirs; }

extern "C" int mfx_rfit2d_batch_dev(void* hv, const double* d_Y, const double* d_W0, int64_t w0_stride, const double* d_peaks,
                                    int maxfasc, int loss, double c, int n_iter, int64_t V, double* d_params, double* d_W,
                                    double* d_scale, int32_t* d_state, int32_t* d_dir_status, int32_t* d_wstatus,
                                    int32_t* d_nchanged, void* stream) {
  const char* fn = "mfx_rfit2d_batch_dev";
  if (mfx_device_count() <= 0) return mfx_fail(MFX_ERR_NO_DEVICE, "%s", NO_DEVICE);
  const mfx_rot2d* h = (const mfx_rot2d*)hv;
  if (!h || V < 0 || maxfasc < 0 || n_iter < 0 ||
      (V > 0 && (!d_Y || !d_params || !d_W || !d_scale || !d_state || !d_dir_status || !d_wstatus || (maxfasc > 0 && !d_peaks) ||
                 (n_iter > 0 && !d_nchanged))))
    return mfx_fail(MFX_ERR_ARG, "%s: bad argument", fn);
  if (maxfasc > 3) return mfx_fail(MFX_ERR_UNSUPPORTED, "%s: at most 3 fascicles (got %d)", fn, maxfasc);
  const int M = h->d.M;
  if (int rc = mfx_rob_check_rule(fn, loss, c, M)) return rc;
  if (d_W0 && w0_stride != 0 && w0_stride != M)
    return mfx_fail(MFX_ERR_ARG, "%s: w0_stride should be M = %d or 0 (got %lld)", fn, M, (long long)w0_stride);
  if (int rc = f2_limits(fn, h, maxfasc, V)) return rc;
  if (int rc = r2d_require_device(h->device)) return rc;
  PlanCount count;
  hipStream_t st = (hipStream_t)stream;
  if (V == 0) {
    if (n_iter > 0) HIPCHK(hipMemsetAsync(d_nchanged, 0, sizeof(int32_t) * (size_t)n_iter, st));
    return MFX_OK;
  }
  F2Dirs dirs(st);
  if (int rc = dirs.enqueue(h, d_peaks, V * maxfasc, st)) return rc;
  const StepScratch step(st);
  const Rob2Class r{h, dirs.rec.p, dirs.pstat.as<int>(), d_Y, d_W0, d_W0 ? w0_stride : 0, maxfasc, nullptr, nullptr, maxfasc, 0, loss, c,
                    V, d_params, d_W, d_scale, d_state, d_dir_status, d_wstatus, d_nchanged, st};
  if (int rc = r2d_first_fit(r)) return rc;
  step.done();
  for (int it = 0; it < n_iter; ++it) {
    if (int rc = r2d_reweight(r, it)) return rc;
    step.done();
    if (int rc = r2d_refit(r)) return rc;
    step.done();
  }
  return MFX_OK;
}

extern "C" int mfx_rfit2d_batch(void* hv, const double* Y, const double* W0, int64_t w0_stride, const int32_t* K, const uint8_t* csf,
                                const double* peaks, int maxfasc, int csf_on, const double* sig_csf, int loss, double c, int n_iter,
                                int64_t V, double* params, double* W_out, double* scale, int32_t* state, int32_t* dir_status,
                                int32_t* wstatus, int64_t* n_changed, int32_t* n_iter_used) {
  const char* fn = "mfx_rfit2d_batch";
  if (mfx_device_count() <= 0) return mfx_fail(MFX_ERR_NO_DEVICE, "%s", NO_DEVICE);
  const mfx_rot2d* h = (const mfx_rot2d*)hv;
  if (!h || V < 0 || maxfasc < 0 || n_iter < 0 || !n_iter_used || (n_iter > 0 && !n_changed) ||
      (V > 0 && (!Y || !K || !params || !W_out || !scale || !state || !dir_status || !wstatus || (maxfasc > 0 && !peaks))))
    return mfx_fail(MFX_ERR_ARG, "%s: bad argument", fn);
  if (maxfasc > 3) return mfx_fail(MFX_ERR_UNSUPPORTED, "%s: at most 3 fascicles (got %d)", fn, maxfasc);
  csf_on = csf_on != 0;
  const int M = h->d.M, np = 1 + 2 * maxfasc + csf_on + 2;
  if (int rc = mfx_rob_check_rule(fn, loss, c, M)) return rc;
  if (W0 && w0_stride != 0 && w0_stride != M)
    return mfx_fail(MFX_ERR_ARG, "%s: w0_stride should be M = %d or 0 (got %lld)", fn, M, (long long)w0_stride);
  if (!W0) w0_stride = 0;
  if (csf_on && !sig_csf) return mfx_fail(MFX_ERR_ARG, "%s: csf_on without sig_csf", fn);   // (the prediction of every class needs it)
  // bin by class (K, CSF flag) before any device call
  std::vector<std::vector<int64_t>> bins((size_t)2 * (maxfasc + 1));
  for (int64_t v = 0; v < V; ++v) {
    const int cf = csf && csf[v];
    if (K[v] < 0 || K[v] > maxfasc) return mfx_fail(MFX_ERR_ARG, "%s: K[%lld] = %d outside 0..%d", fn, (long long)v, K[v], maxfasc);
    if (cf && (!csf_on || !sig_csf)) return mfx_fail(MFX_ERR_ARG, "%s: voxels flagged CSF need csf_on and sig_csf", fn);
    bins[(size_t)2 * K[v] + cf].push_back(v);
  }
  *n_iter_used = 0;
  for (int it = 0; it < n_iter; ++it) n_changed[it] = 0;
  if (int rc = f2_limits(fn, h, maxfasc, V)) return rc;
  if (int rc = r2d_require_device(h->device)) return rc;
  PlanCount count;
  if (V == 0) return MFX_OK;
  DevMem dxc, dW0s, dnc;
  if (sig_csf) {
    HIPCHK(dxc.alloc(sizeof(double) * M));
    HIPCHK(hipMemcpy(dxc.p, sig_csf, sizeof(double) * M, hipMemcpyHostToDevice));
  }
  if (W0 && w0_stride == 0) {   // the shared vector is uploaded once
    HIPCHK(dW0s.alloc(sizeof(double) * M));
    HIPCHK(hipMemcpy(dW0s.p, W0, sizeof(double) * M, hipMemcpyHostToDevice));
  }
  HIPCHK(dnc.alloc(sizeof(int32_t) * (size_t)std::max(n_iter, 1)));
  for (size_t b = 0; b < bins.size(); ++b) {
    const std::vector<int64_t>& all = bins[b];
    const int k = (int)(b >> 1), cf = (int)(b & 1);
    // voxels per upload from a byte budget: Y, W0, W, the prediction and the weighted fit's s and y' (8 M bytes each), the
    // plan's records (28 K M) and the kernels' records (32 K M)
    const size_t per_vox = (size_t)M * (sizeof(double) * 6 + (size_t)k * (28 + sizeof(F2Rec)));
    const size_t chunk = std::max<size_t>(1, ((size_t)256 << 20) / per_vox);
    for (size_t c0 = 0; c0 < all.size(); c0 += chunk) {
      const size_t nv = std::min(chunk, all.size() - c0);
      const int64_t* ix = all.data() + c0;
      const size_t kk = (size_t)std::max(k, 1);
      std::vector<double> Yc(nv * M), Wc(nv * M), pcK(nv * 3 * kk), prm(nv * np), scc(nv);
      std::vector<int32_t> vsc(nv * 5), wsc(nv), stt(nv);
      for (size_t q = 0; q < nv; ++q) {
        std::memcpy(&Yc[q * M], Y + (size_t)ix[q] * M, sizeof(double) * M);
        if (w0_stride) std::memcpy(&Wc[q * M], W0 + (size_t)ix[q] * M, sizeof(double) * M);
        if (k > 0) std::memcpy(&pcK[q * 3 * k], peaks + (size_t)ix[q] * 3 * maxfasc, sizeof(double) * 3 * k);
      }
      DevMem dY, dW0, dW, dpK, dpr, dsc, dstt, dvs, dws;
      HIPCHK(dY.alloc(sizeof(double) * Yc.size()));
      HIPCHK(dW0.alloc(w0_stride ? sizeof(double) * Wc.size() : 0));
      HIPCHK(dW.alloc(sizeof(double) * Wc.size()));
      HIPCHK(dpK.alloc(sizeof(double) * pcK.size()));
      HIPCHK(dpr.alloc(sizeof(double) * prm.size()));
      HIPCHK(dsc.alloc(sizeof(double) * nv));
      HIPCHK(dstt.alloc(sizeof(int32_t) * nv));
      HIPCHK(dvs.alloc(sizeof(int32_t) * 5 * nv));
      HIPCHK(dws.alloc(sizeof(int32_t) * nv));
      HIPCHK(hipMemcpy(dY.p, Yc.data(), sizeof(double) * Yc.size(), hipMemcpyHostToDevice));
      if (w0_stride) HIPCHK(hipMemcpy(dW0.p, Wc.data(), sizeof(double) * Wc.size(), hipMemcpyHostToDevice));
      HIPCHK(hipMemcpy(dpK.p, pcK.data(), sizeof(double) * pcK.size(), hipMemcpyHostToDevice));
      const double* w0d = !W0 ? nullptr : (w0_stride ? dW0.as<double>() : dW0s.as<double>());
      // the chunk's directions, once: every fit and every prediction below reads these records
      F2Dirs dirs(nullptr);
      if (int rc = dirs.enqueue(h, dpK.as<double>(), (int64_t)nv * k, nullptr)) return rc;
      // one iteration at a time: the count of changed voxels decides whether the chunk goes on.  An iteration that
      // changed nothing leaves its fit out when the parameters already are those of a weighted fit on these weights
      // (any iteration but the first one after an unweighted fit); every later iteration would repeat it bit for bit.
      int used = 0;
      const StepScratch step(nullptr);
      const Rob2Class r{h, dirs.rec.p, dirs.pstat.as<int>(), dY.as<double>(), w0d, w0_stride, k, cf ? dxc.as<double>() : nullptr,
                        dxc.as<double>(), maxfasc, csf_on, loss, c, (int64_t)nv, dpr.as<double>(), dW.as<double>(), dsc.as<double>(),
                        dstt.as<int32_t>(), dvs.as<int32_t>(), dws.as<int32_t>(), dnc.as<int32_t>(), nullptr};
      if (int rc = r2d_first_fit(r)) return rc;
      step.done();
      for (int it = 0; it < n_iter; ++it) {
        if (int rc = r2d_reweight(r, it)) return rc;
        step.done();
        int32_t nc = 0;
        HIPCHK(hipMemcpy(&nc, dnc.as<int32_t>() + it, sizeof(int32_t), hipMemcpyDeviceToHost));   // (waits for the default stream)
        n_changed[it] += nc;
        used = it + 1;
        if (nc == 0 && (it > 0 || W0)) break;
        if (int rc = r2d_refit(r)) return rc;
        step.done();
      }
      *n_iter_used = std::max<int32_t>(*n_iter_used, used);
      HIPCHK(hipStreamSynchronize(nullptr));
      HIPCHK(hipMemcpy(prm.data(), dpr.p, sizeof(double) * prm.size(), hipMemcpyDeviceToHost));
      HIPCHK(hipMemcpy(Wc.data(), dW.p, sizeof(double) * Wc.size(), hipMemcpyDeviceToHost));
      HIPCHK(hipMemcpy(scc.data(), dsc.p, sizeof(double) * nv, hipMemcpyDeviceToHost));
      HIPCHK(hipMemcpy(stt.data(), dstt.p, sizeof(int32_t) * nv, hipMemcpyDeviceToHost));
      HIPCHK(hipMemcpy(vsc.data(), dvs.p, sizeof(int32_t) * 5 * nv, hipMemcpyDeviceToHost));
      HIPCHK(hipMemcpy(wsc.data(), dws.p, sizeof(int32_t) * nv, hipMemcpyDeviceToHost));
      for (size_t q = 0; q < nv; ++q) {
        std::memcpy(params + (size_t)ix[q] * np, &prm[q * np], sizeof(double) * np);
        std::memcpy(W_out + (size_t)ix[q] * M, &Wc[q * M], sizeof(double) * M);
        std::memcpy(dir_status + (size_t)ix[q] * 5, &vsc[q * 5], sizeof(int32_t) * 5);
        scale[ix[q]] = scc[q];
        state[ix[q]] = stt[q];
        wstatus[ix[q]] = wsc[q];
      }
    }
  }
  return MFX_OK;
}
