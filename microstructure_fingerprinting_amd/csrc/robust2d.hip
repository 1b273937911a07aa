// robust2d.hip -- robust fits of voxels of a 2-D (AxCaliber-like) protocol (include/mfx_robust2d.h): the loop
// fit -> predict -> reweight -> weighted fit of robust.hip on a handle of rotate2d.hip, on device-resident data.
// Nothing here computes: the fits are the class launchers of fit2d.hip (unweighted) and w2d.hip (weighted) on prepared
// directions, the prediction is the kernel of predict2d.hip on the same records, the rule is mfx_robust_weights_kernel
// of robust.hip.  What this file adds is the order of the launches - and that the plan of the class's directions and
// the kernels' 32-byte records (F2Dirs) are made once per class chunk, not once per fit and prediction.  The loop itself is
// mfx_rob_iterate (mfx_host.h) over the three steps below; the host side of a mixed batch is class_batch.h.
#include "fit2d_shared.h"
#include "../../include/mfx_robust.h"
#include "../../include/mfx_robust2d.h"

#include <algorithm>
#include <cstring>
#include <vector>

namespace {

thread_local int64_t g_last_plan_dirs = 0;

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

// the loop's steps for mfx_rob_iterate (mfx_host.h)
struct Rob2Steps {
  const Rob2Class& r;
  const StepScratch& step;
  int first_fit() const { return r2d_first_fit(r); }
  int reweight(int it) const { return r2d_reweight(r, it); }
  int refit() const { return r2d_refit(r); }
  void step_done() const { step.done(); }
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
  if (mfx_device_count() <= 0) return mfx_no_device();
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
  if (int rc = mfx_require_device(h->device)) return rc;
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
  return mfx_rob_iterate(Rob2Steps{r, step}, n_iter, nullptr);
}

extern "C" int mfx_rfit2d_batch(void* hv, const double* Y, const double* W0, int64_t w0_stride, const int32_t* K, const uint8_t* csf,
                                const double* peaks, int maxfasc, int csf_on, const double* sig_csf, int loss, double c, int n_iter,
                                int64_t V, double* params, double* W_out, double* scale, int32_t* state, int32_t* dir_status,
                                int32_t* wstatus, int64_t* n_changed, int32_t* n_iter_used) {
  const char* fn = "mfx_rfit2d_batch";
  if (mfx_device_count() <= 0) return mfx_no_device();
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
  MfxClassBins bins;
  if (int rc = mfx_class_bins(fn, K, csf, maxfasc, csf_on && sig_csf, V, &bins)) return rc;
  *n_iter_used = 0;
  for (int it = 0; it < n_iter; ++it) n_changed[it] = 0;
  if (int rc = f2_limits(fn, h, maxfasc, V)) return rc;
  if (int rc = mfx_require_device(h->device)) return rc;
  PlanCount count;
  if (V == 0) return MFX_OK;
  DevBuf<double> dxc, dW0s;
  DevBuf<int32_t> dnc;
  if (sig_csf) HIPCHK(dxc.upload(sig_csf, M));
  if (W0 && w0_stride == 0) HIPCHK(dW0s.upload(W0, M));   // the shared vector is uploaded once
  HIPCHK(dnc.alloc_n((size_t)std::max(n_iter, 1)));
  // voxels per upload from a byte budget: Y, W0, W, the prediction and the weighted fit's s and y' (8 M bytes each), the
  // plan's records (28 K M) and the kernels' records (32 K M)
  static_assert(sizeof(F2Rec) == MFX_F2REC_BYTES, "mfx_rfit2d_upload_chunk counts 32 bytes per record");
  const auto chunk_of = [M](int k) { return mfx_rfit2d_upload_chunk(M, k); };
  return mfx_class_walk(bins, chunk_of, [&](int k, int cf, const int64_t* ix, size_t nv) -> int {
    DevBuf<double> dY, dW0, dW, dpK, dpr, dsc;
    DevBuf<int32_t> dstt, dvs, dws;
    HIPCHK(dY.upload_rows(Y, ix, nv, M, M));
    if (w0_stride) HIPCHK(dW0.upload_rows(W0, ix, nv, M, M));
    HIPCHK(mfx_upload_peaks(dpK, peaks, ix, nv, maxfasc, k));
    HIPCHK(dW.alloc_n(nv * M));
    HIPCHK(dpr.alloc_n(nv * np));
    HIPCHK(dsc.alloc_n(nv));
    HIPCHK(dstt.alloc_n(nv));
    HIPCHK(dvs.alloc_n(nv * 5));
    HIPCHK(dws.alloc_n(nv));
    const double* w0d = !W0 ? nullptr : (w0_stride ? dW0.get() : dW0s.get());
    // the chunk's directions, once: every fit and every prediction below reads these records
    F2Dirs dirs(nullptr);
    if (int rc = dirs.enqueue(h, dpK.get(), (int64_t)nv * k, nullptr)) return rc;
    const StepScratch step(nullptr);
    const Rob2Class r{h, dirs.rec.p, dirs.pstat.as<int>(), dY.get(), w0d, w0_stride, k, cf ? dxc.get() : nullptr, dxc.get(), maxfasc, csf_on,
                      loss, c, (int64_t)nv, dpr.get(), dW.get(), dsc.get(), dstt.get(), dvs.get(), dws.get(), dnc.get(), nullptr};
    const MfxRobHostCount host{dnc.get(), W0 != nullptr, n_changed, n_iter_used};
    if (int rc = mfx_rob_iterate(Rob2Steps{r, step}, n_iter, &host)) return rc;
    HIPCHK(hipStreamSynchronize(nullptr));
    HIPCHK(dpr.download_rows(params, ix, nv, np));
    HIPCHK(dW.download_rows(W_out, ix, nv, M));
    HIPCHK(dvs.download_rows(dir_status, ix, nv, 5));
    HIPCHK(dsc.download_rows(scale, ix, nv, 1));
    HIPCHK(dstt.download_rows(state, ix, nv, 1));
    HIPCHK(dws.download_rows(wstatus, ix, nv, 1));
    return MFX_OK;
  });
}
