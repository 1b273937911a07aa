// boot_shared.h -- what boot.hip, wboot.hip, boot2d.hip and wboot2d.hip share on the device side of the bootstrap:
//   BootClass          the arguments of one class on device buffers (what a *_fit_dev entry point runs after its checks and
//                      a mixed entry point runs per class chunk); fields a family does not use are null or zero
//   BootChunkMem       the front and the tail of a *_class_dev loop: the chunk size within the byte budget, the scratch
//                      buffers every family needs, the gather-then-reduce tail.  The middle of the loop - the family's own
//                      fit, its prediction, the resampling, the replicate fit - stays in its file.
//   boot_run_mixed     the host side of the four mixed entry points: per-batch uploads, the walk over the classes
//                      (class_batch.h), per chunk the uploads, the class run, the downloads and the scatter (boot_batch.h)
//   boot_expand_kernel rows [V x w] -> [V B x w]
#pragma once
#include "mfx_host.h"
#include "boot_batch.h"

namespace {

constexpr int64_t BOOT_DEFAULT_BYTES = (int64_t)256 << 20;

// rows [V x w] -> [V B x w]
__global__ void boot_expand_kernel(const double* __restrict__ src, int64_t V, int B, int w, double* __restrict__ dst) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= V * B * w) return;
  const int64_t row = i / w;
  dst[i] = src[(row / B) * w + (i - row * w)];
}

struct BootClass {
  const double *Y, *W;           // [V x M]; weights [V x M] or [M], or null
  int64_t wstride;               // M or 0
  const double* peaks;           // [V x 3 F] or null
  int F, csf_on, ear_on;
  const double *sig_csf, *sig_ear;
  int E;
  const double *params0, *pred0;   // the own fit [V x np] and its prediction [V x M], or null: made here
  const int32_t* groups;
  const int64_t* vox;
  int64_t V;
  int B, kind, inflate;
  uint64_t seed, offset;
  const double* props;
  int nprop;
  const double* q;
  int Q;
  int64_t max_bytes;
  double* stats;
  int32_t *agree, *status, *dir_status;   // dir_status [V x 5]: the 2-D families
  double* keep;
  hipStream_t st;
};

struct BootChunkMem {
  const BootClass& r;
  int M, np, C;
  int64_t Vc = 0;   // voxels per chunk
  StreamMem ys, prm, X, vd, par0, pred, pst;
  BootChunkMem(const BootClass& r_, int M_)
      : r(r_), M(M_), np(boot_np(r_.F, r_.csf_on, r_.ear_on)), C(boot_ncol(r_.F, r_.csf_on, r_.ear_on, r_.nprop)), ys(r_.st), prm(r_.st),
        X(r_.st), vd(r_.st), par0(r_.st), pred(r_.st), pst(r_.st) {}
  int64_t budget() const { return r.max_bytes > 0 ? r.max_bytes : BOOT_DEFAULT_BYTES; }
  // per_vox: the bytes a voxel takes in a chunk (its replicate signals and what the family's replicate fit adds)
  int alloc(int64_t per_vox) {
    const int B = r.B;
    Vc = std::max<int64_t>(1, std::min<int64_t>(r.V, budget() / per_vox));
    Vc = std::min<int64_t>(Vc, 0x7fffffff / B);   // the replicate rows of a chunk are one launch of the fit
    HIPCHK(ys.alloc(sizeof(double) * (size_t)Vc * B * M));
    if (!r.keep) HIPCHK(prm.alloc(sizeof(double) * (size_t)Vc * B * np));
    HIPCHK(X.alloc(sizeof(double) * (size_t)Vc * B * C));
    HIPCHK(vd.alloc((size_t)Vc * B * C));
    if (!r.params0) HIPCHK(par0.alloc(sizeof(double) * (size_t)Vc * np));
    if (!r.pred0) {
      HIPCHK(pred.alloc(sizeof(double) * (size_t)Vc * M));
      HIPCHK(pst.alloc(2 * sizeof(int)));
      HIPCHK(hipMemsetAsync(pst.p, 0, 2 * sizeof(int), r.st));   // a row the fit could not serve is flagged there and predicted as NaN: status 2
    }
    return MFX_OK;
  }
  // of the chunk that begins at voxel v0: the own fit's rows, their prediction, the replicate rows
  const double* p0(int64_t v0) const { return r.params0 ? r.params0 + (size_t)v0 * np : par0.as<double>(); }
  const double* pr(int64_t v0) const { return r.pred0 ? r.pred0 + (size_t)v0 * M : pred.as<double>(); }
  double* rows(int64_t v0) const { return r.keep ? r.keep + (size_t)v0 * r.B * np : prm.as<double>(); }
  // the value table of the chunk's replicate rows and its statistics (N: atoms of the property tables)
  int gather_reduce(int64_t v0, int64_t nv, int N) const {
    if (int rc = mfx_boot_gather_dev(rows(v0), p0(v0), r.F, r.csf_on, r.ear_on, r.props, r.nprop, N, r.status + v0, nv, r.B, X.as<double>(),
                                     vd.as<uint8_t>(), r.agree ? r.agree + (size_t)v0 * r.F : nullptr, r.st)) return rc;
    return mfx_boot_reduce_dev(X.as<double>(), vd.as<uint8_t>(), nv, r.B, C, r.q, r.Q, r.stats + (size_t)v0 * C * (MFX_BOOT_NSTAT + r.Q), r.st);
  }
};

// The caller's host arrays of a mixed batch, after the entry point's own checks.
struct BootBatch {
  const char* fn;
  int device, M, N;
  const double *Y, *W;     // W [V x M] (w_stride = M), one shared [M] vector (w_stride = 0), or null: no weights
  int64_t w_stride;
  const int32_t* K;
  const uint8_t *csf, *ear;   // ear null: no voxel has the EAR columns
  const double* peaks;
  int F, csf_on, ear_on;
  const double *sig_csf, *sig_ear;
  int E;
  const double* params0;
  const int32_t* groups;
  const int64_t* vox;
  int64_t V;
  int B, kind, inflate;
  uint64_t seed, offset;
  const double* props;
  int nprop;
  const double* q;
  int Q;
  int64_t max_bytes;
  double* stats;
  int32_t *agree, *status, *dir_status;   // dir_status [V x 5] or null
  double* keep;
};

// run(const BootClass&): one class chunk on device buffers, on the default stream.  The voxels without and with the EAR
// columns are binned on their own by (K, CSF flag), each before any device call; without `ear` the second pass is empty.
template <class Run>
int boot_run_mixed(const BootBatch& b, Run run) {
  const int M = b.M, F = b.F, B = b.B, Q = b.Q, NS = MFX_BOOT_NSTAT + b.Q;
  std::vector<int64_t> sub[2];
  for (int64_t v = 0; v < b.V; ++v) sub[(b.ear && b.ear[v]) ? 1 : 0].push_back(v);
  MfxClassBins bins[2];
  for (int e = 0; e < 2; ++e) {
    std::vector<int32_t> Ks(sub[e].size());
    std::vector<uint8_t> cs(sub[e].size());
    for (size_t i = 0; i < sub[e].size(); ++i) { Ks[i] = b.K[sub[e][i]]; cs[i] = b.csf ? b.csf[sub[e][i]] : 0; }
    if (int rc = mfx_class_bins(b.fn, Ks.data(), cs.data(), F, b.csf_on && b.sig_csf, (int64_t)sub[e].size(), &bins[e])) return rc;
    for (auto& bin : bins[e]) for (auto& i : bin) i = sub[e][(size_t)i];   // positions in the sub-list -> batch positions
  }
  if (b.V == 0) return MFX_OK;
  if (int rc = mfx_require_device(b.device)) return rc;
  DevBuf<double> dxc, dxe, dprops, dq, dWs;
  DevBuf<int32_t> dgr;
  if (b.csf_on) HIPCHK(dxc.upload(b.sig_csf, M));
  if (b.ear_on) HIPCHK(dxe.upload(b.sig_ear, (size_t)M * b.E));
  if (b.nprop > 0) HIPCHK(dprops.upload(b.props, (size_t)b.nprop * b.N));
  if (Q > 0) HIPCHK(dq.upload(b.q, Q));
  if (b.kind == MFX_BOOT_RESIDUAL) HIPCHK(dgr.upload(b.groups, M));
  if (b.W && b.w_stride == 0) HIPCHK(dWs.upload(b.W, M));   // the shared vector is uploaded once and read with stride 0
  const int64_t budget = b.max_bytes > 0 ? b.max_bytes : BOOT_DEFAULT_BYTES;
  for (int e = 0; e < 2; ++e) {
    const int rc = mfx_class_walk(bins[e], boot_upload_chunk(budget, B, M), [&](int k, int cf, const int64_t* ix, size_t nv) -> int {
      const BootColMap map(F, b.csf_on, b.ear_on, b.nprop, k, cf, e);
      DevBuf<double> dY, dW, dpk, dp0, dst, dkeep;
      DevBuf<int32_t> dag, dstat, ddir;
      DevBuf<int64_t> dvox;
      HIPCHK(dY.upload_rows(b.Y, ix, nv, M, M));
      if (b.W && b.w_stride) HIPCHK(dW.upload_rows(b.W, ix, nv, M, M));
      HIPCHK(mfx_upload_peaks(dpk, b.peaks, ix, nv, F, k));
      if (b.params0) {
        const std::vector<double> rows = boot_gather_params0(map, b.params0, ix, nv);
        HIPCHK(dp0.upload(rows.data(), rows.size()));
      }
      HIPCHK(dvox.upload(boot_vox_keys(b.vox, ix, nv).data(), nv));
      HIPCHK(dst.alloc_n(nv * map.Cc * NS));
      HIPCHK(dag.alloc_n(nv * (size_t)std::max(k, 1)));
      HIPCHK(dstat.alloc_n(nv));
      if (b.dir_status) HIPCHK(ddir.alloc_n(nv * 5));
      if (b.keep) HIPCHK(dkeep.alloc_n(nv * B * map.npc));
      BootClass r{};
      r.Y = dY.get(); r.W = b.W ? (b.w_stride ? dW.get() : dWs.get()) : nullptr; r.wstride = b.w_stride;
      r.peaks = k > 0 ? dpk.get() : nullptr; r.F = k; r.csf_on = cf; r.ear_on = e;
      r.sig_csf = cf ? dxc.get() : nullptr; r.sig_ear = e ? dxe.get() : nullptr; r.E = e ? b.E : 0;
      r.params0 = b.params0 ? dp0.get() : nullptr; r.groups = dgr.get(); r.vox = dvox.get(); r.V = (int64_t)nv;
      r.B = B; r.kind = b.kind; r.inflate = b.inflate; r.seed = b.seed; r.offset = b.offset;
      r.props = dprops.get(); r.nprop = b.nprop; r.q = dq.get(); r.Q = Q; r.max_bytes = budget;
      r.stats = dst.get(); r.agree = dag.get(); r.status = dstat.get(); r.dir_status = ddir.get(); r.keep = dkeep.get();
      if (int rc2 = run(r)) return rc2;
      HIPCHK(hipStreamSynchronize(nullptr));
      std::vector<double> hs(dst.n), hk(dkeep.n);
      std::vector<int32_t> ha(dag.n), hst(nv);
      HIPCHK(dst.download(hs.data()));
      HIPCHK(dag.download(ha.data()));
      HIPCHK(dstat.download(hst.data()));
      if (b.dir_status) HIPCHK(ddir.download_rows(b.dir_status, ix, nv, 5));
      if (b.keep) HIPCHK(dkeep.download(hk.data()));
      boot_scatter(map, ix, nv, B, Q, hs.data(), ha.data(), hst.data(), b.keep ? hk.data() : nullptr, b.stats, b.agree, b.status, b.keep);
      return MFX_OK;
    });
    if (rc) return rc;
  }
  return MFX_OK;
}

}  // namespace
