// wboot2d.hip -- the bootstrap of 2-D (AxCaliber-like) protocols conditional on a fit's measurement weights
// (include/mfx_wboot2d.h): the own weighted fit (w2d.hip's class launcher), its prediction (predict2d.hip's kernel), the
// resampling rule of wboot.hip and the value table and statistics of boot.hip through their public entry points, and
// between them the WEIGHTED REPLICATE FIT: B signals per voxel on one set of weights and directions.
//
// The replicate fit (wb2_rows).  One and two fascicles without a CSF column run the WGT = true instantiations of
// boot2d_kernels.h (described there; only this file instantiates them): per voxel the directions' records and status
// (F2Dirs, fit2d_status_kernel), s = sqrt(W), sum W and the weights' status (w2d_prep_kernel of fit2d_kernels.h, the
// arithmetic of the plain weighted fit), the norms |fl(s_m d)|^2 and for K = 2 the weighted cross-Gram into scratch
// G [NP x NP]; per replicate y'* = fl(s_m y*_m) (boot2d_wsig_kernel), fl(s_m d) . y'* in replicate tiles, |y'*|^2, then
// one workgroup per (voxel, replicate) that scans G and runs the exact stage.  Scratch per voxel:
// 8 (M + 1 + B M + NP^2 + K NP (B + 1) + B) + 4 bytes; the voxels go in chunks within the byte budget.  Every other class,
// and everything under mfx_wboot2d_debug_set_force_plain(1), takes the plain path: weight rows and directions are copied
// to the replicate rows of a voxel chunk (a shared [M] vector stays shared) and w2d.hip's class launcher runs on them
// untouched.  The host side of a mixed batch, the per-class arguments and the front and tail of the class loop are
// boot_shared.h's, as in boot.hip.
#include "boot2d_kernels.h"
#include "boot_shared.h"
#include "../../include/mfx_wboot2d.h"
#include "../../include/mfx_wboot.h"
#include "../../include/mfx_w2d.h"

#include <algorithm>
#include <cstring>
#include <vector>

namespace {

thread_local int g_force_plain = 0;

constexpr int WB2_MAXF = 3;

unsigned wb2_grid(int64_t n) { return (unsigned)((n + 255) / 256); }

// the voxel's records = those of its first replicate row: the directions' [5] and the weights' [1]
__global__ void wboot2d_first_row_kernel(const int* __restrict__ rows, const int* __restrict__ wrows, int64_t V, int B,
                                         int* __restrict__ vstat, int* __restrict__ wstat) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= V * 5) return;
  vstat[i] = rows[(i / 5) * B * 5 + i % 5];
  if (i % 5 == 0) wstat[i / 5] = wrows[(i / 5) * B];
}
// NaN rows for the replicates of a voxel the shared path's kernels skip: a failing direction, unusable weights
__global__ void wboot2d_nan_rows_kernel(const int* __restrict__ vstat, const int* __restrict__ wstat, int64_t V, int64_t per_vox,
                                        double* __restrict__ params) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= V * per_vox) return;
  const int64_t v = i / per_vox;
  if (vstat[5 * v] != 0 || wstat[v] != 0) params[i] = __builtin_nan("");
}
// A failing direction makes the status 2, whatever the resampling rule said (it is tested first); the signals of a voxel
// in a non-zero status (NaN rows of the resampling rule) become zero rows for the fit.
__global__ void wboot2d_mask_kernel(int* __restrict__ status, const int* __restrict__ vstat, int64_t V, int64_t per_vox,
                                    double* __restrict__ Ys) {
  const int64_t v = blockIdx.x;
  const bool dirfail = vstat[5 * v] != 0;
  const int st = status[v];
  if (st == 0 && !dirfail) return;
  for (int64_t i = threadIdx.x; i < per_vox; i += blockDim.x) Ys[v * per_vox + i] = 0.0;
  if (dirfail && st != 2 && threadIdx.x == 0) status[v] = 2;
}

// the largest dictionary of the shared path's two-fascicle kernels: the plain weighted kernel must serve it too (its
// arithmetic is what the replicates repeat), and the scan kernel's LDS must hold its statistics
int wb2_max_atoms(const mfx_rot2d* h) {
  int n = f2_max_atoms_k2(true);
  while (n > 0 && b2_k2_lds_bytes((n + 15) & ~15, h->d.M) > F2_LDS_MAX) n -= 16;
  return std::max(n, 0);
}

bool wb2_shared_serves(const mfx_rot2d* h, int K, bool has_csf) {
  if (g_force_plain || has_csf) return false;
  if (K == 1) return true;
  return K == 2 && h->d.N <= wb2_max_atoms(h);
}

// scratch bytes of the replicate fit per voxel (what the chunks of the bootstrap count beside the signals)
int64_t wb2_rows_bytes(const mfx_rot2d* h, int K, bool has_csf, int64_t wstride, int B) {
  const int64_t M = h->d.M, NP = (h->d.N + 15) & ~15;
  if (wb2_shared_serves(h, K, has_csf))
    return 8 * (M + 1 + (int64_t)B * M + (K == 2 ? NP * NP : 0) + K * NP * ((int64_t)B + 1) + B) + 4;
  // the plain path: records and plan of B K directions, the copied weight rows, s and y' of the class launcher
  return (int64_t)B * (K * (M * (int64_t)(sizeof(F2Rec) + sizeof(int) + 3 * sizeof(double)) + 24 + 16) + 20 + (wstride ? 8 * M : 0) +
                       16 * M + 24);
}

// The replicate fit of one class: V voxels of K fascicles (d_peaks [V x 3 K]), the CSF column d_xc or none, B signals
// each on the voxel's weights -> d_params [V x B x np] (np = 1 + 2 K + csf + 2), d_vstat [V x 5], d_wstat [V].  dirs: the
// prepared directions of the V voxels (null: prepared here).  Only enqueues.
int wb2_rows(const mfx_rot2d* h, const double* d_Ys, const double* d_W, int64_t wstride, const double* d_peaks, const F2Dirs* dirs,
             int K, const double* d_xc, int64_t V, int B, double* d_params, int32_t* d_vstat, int32_t* d_wstat, int64_t budget,
             hipStream_t st) {
  const int M = h->d.M, N = h->d.N, NP = (N + 15) & ~15, has_csf = d_xc != nullptr;
  const int np = boot_np(K, has_csf, 0);
  if (int rc = f2_limits("mfx_wboot2d", h, K, V)) return rc;
  if (V > 0x7fffffff / B) return mfx_fail(MFX_ERR_UNSUPPORTED, "mfx_wboot2d: more than 2^31 replicate rows in one call");
  if (budget <= 0) budget = BOOT_DEFAULT_BYTES;
  const int64_t per_vox = std::max<int64_t>(1, wb2_rows_bytes(h, K, has_csf, wstride, B));

  if (wb2_shared_serves(h, K, has_csf)) {
    HIPCHK(hipMemsetAsync(d_params, 0, sizeof(double) * (size_t)V * B * np, st));
    F2Dirs own(st);
    if (!dirs) {
      if (int rc = own.enqueue(h, d_peaks, V * K, st)) return rc;
      dirs = &own;
    }
    hipLaunchKernelGGL(fit2d_status_kernel, dim3(wb2_grid(V)), dim3(256), 0, st, dirs->pstat.as<int>(), K, V, d_vstat, (int*)nullptr,
                       (double*)nullptr, np);
    HIPCHK(hipGetLastError());
    const int64_t Vc = std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(V, MFX_WB2_VOX_PER_LAUNCH), budget / per_vox));
    StreamMem sS(st), ssw(st), sYs(st), sa2(st), say(st), sysq(st), sG(st);
    HIPCHK(sS.alloc(sizeof(double) * (size_t)Vc * M));
    HIPCHK(ssw.alloc(sizeof(double) * (size_t)Vc));
    HIPCHK(sYs.alloc(sizeof(double) * (size_t)Vc * B * M));
    HIPCHK(sa2.alloc(sizeof(double) * (size_t)Vc * K * NP));
    HIPCHK(say.alloc(sizeof(double) * (size_t)Vc * B * K * NP));
    HIPCHK(sysq.alloc(sizeof(double) * (size_t)Vc * B));
    if (K == 2) HIPCHK(sG.alloc(sizeof(double) * (size_t)Vc * NP * NP));
    const size_t lds2 = b2_k2_lds_bytes(NP, M);
    if (K == 2 && lds2 > 64 * 1024)
      HIPCHK(hipFuncSetAttribute((const void*)boot2d_k2_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds2));
    for (int64_t v0 = 0; v0 < V; v0 += Vc) {
      const int64_t nv = std::min(Vc, V - v0);
      const double* w = d_W + (size_t)v0 * wstride;
      const double* ystar = d_Ys + (size_t)v0 * B * M;
      int32_t* vstat = d_vstat + 5 * v0;
      int32_t* wstat = d_wstat + v0;
      double* rows = d_params + (size_t)v0 * B * np;
      // s, sum W and the weights' status by the plain weighted fit's own kernel (no y': the replicates have their own)
      hipLaunchKernelGGL(w2d_prep_kernel, dim3((unsigned)nv), dim3(64), 0, st, (const double*)nullptr, w, wstride, M, vstat, sS.as<double>(),
                         (double*)nullptr, ssw.as<double>(), wstat, (int*)nullptr, (double*)nullptr, 0);
      HIPCHK(hipGetLastError());
      hipLaunchKernelGGL(wboot2d_nan_rows_kernel, dim3(wb2_grid(nv * B * np)), dim3(256), 0, st, vstat, wstat, nv, (int64_t)B * np, rows);
      HIPCHK(hipGetLastError());
      hipLaunchKernelGGL(boot2d_wsig_kernel, dim3(wb2_grid(nv * B * M)), dim3(256), 0, st, ystar, sS.as<double>(), vstat, wstat, nv, B, M,
                         sYs.as<double>());
      HIPCHK(hipGetLastError());
      WB2Args a{};
      a.M = M; a.N = N; a.NP = NP; a.B = B; a.base = h->d.ky;
      a.rec = dirs->rec.as<F2Rec>() + (size_t)v0 * K * M;
      a.Y = ystar;
      a.vstat = vstat;
      a.a2 = sa2.as<double>(); a.ay = say.as<double>(); a.ysq = sysq.as<double>(); a.G = sG.as<double>();
      a.params = rows; a.num_params = np; a.maxfasc = K;
      a.Ys = sYs.as<double>(); a.W = w; a.wstride = wstride; a.S = sS.as<double>(); a.sumw = ssw.as<double>(); a.wstat = wstat;
      const dim3 gs((unsigned)((K * NP + B2_ST_WG - 1) / B2_ST_WG), (unsigned)((B + B2_R - 1) / B2_R), (unsigned)nv);
      if (K == 1) {
        hipLaunchKernelGGL((boot2d_stats_kernel<1, true>), gs, dim3(B2_ST_WG), 0, st, a);
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL((boot2d_ysq_kernel<1, true>), dim3(wb2_grid(nv * B)), dim3(256), 0, st, a, nv * B);
        HIPCHK(hipGetLastError());
        const size_t lds = (2 * F2_K1_WG + 8 + (size_t)M) * sizeof(double);
        hipLaunchKernelGGL(boot2d_k1_kernel<true>, dim3((unsigned)(nv * B)), dim3(F2_K1_WG), lds, st, a);
        HIPCHK(hipGetLastError());
      } else {
        hipLaunchKernelGGL((boot2d_stats_kernel<2, true>), gs, dim3(B2_ST_WG), 0, st, a);
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL((boot2d_ysq_kernel<2, true>), dim3(wb2_grid(nv * B)), dim3(256), 0, st, a, nv * B);
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL(boot2d_gram_kernel<true>, dim3((unsigned)nv), dim3(F2_WG), b2_gram_lds_bytes(true), st, a, sG.as<double>());
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL(boot2d_k2_kernel<true>, dim3((unsigned)(nv * B)), dim3(F2_WG), lds2, st, a);
        HIPCHK(hipGetLastError());
      }
    }
    return MFX_OK;
  }

  // the plain path: weight rows and directions copied to the replicate rows of a voxel chunk, w2d.hip's class launcher
  const int64_t Vc = std::max<int64_t>(1, std::min<int64_t>(V, budget / per_vox));
  StreamMem pk(st), wr(st), vrow(st), wrow(st);
  HIPCHK(pk.alloc(sizeof(double) * (size_t)Vc * B * 3 * std::max(K, 1)));
  if (wstride) HIPCHK(wr.alloc(sizeof(double) * (size_t)Vc * B * M));
  HIPCHK(vrow.alloc(sizeof(int) * (size_t)Vc * B * 5));
  HIPCHK(wrow.alloc(sizeof(int) * (size_t)Vc * B));
  ScratchMark mark;
  const bool marked = mfx_scratch_mark(st, &mark);
  for (int64_t v0 = 0; v0 < V; v0 += Vc) {
    const int64_t nv = std::min(Vc, V - v0);
    {
      F2Dirs rows(st);
      if (K > 0) {
        hipLaunchKernelGGL(boot_expand_kernel, dim3(wb2_grid(nv * B * 3 * K)), dim3(256), 0, st, d_peaks + (size_t)v0 * 3 * K, nv, B,
                           3 * K, pk.as<double>());
        HIPCHK(hipGetLastError());
      }
      if (wstride) {
        hipLaunchKernelGGL(boot_expand_kernel, dim3(wb2_grid(nv * B * M)), dim3(256), 0, st, d_W + (size_t)v0 * M, nv, B, M,
                           wr.as<double>());
        HIPCHK(hipGetLastError());
      }
      if (int rc = rows.enqueue(h, pk.as<double>(), nv * B * K, st)) return rc;
      if (int rc = mfx_wfit2d_class_prepared(h, d_Ys + (size_t)v0 * B * M, wstride ? wr.as<double>() : d_W, wstride, rows.rec.p,
                                             rows.pstat.as<int>(), K, d_xc, K, has_csf, nv * B, d_params + (size_t)v0 * B * np,
                                             vrow.as<int32_t>(), wrow.as<int32_t>(), st)) return rc;
      hipLaunchKernelGGL(wboot2d_first_row_kernel, dim3(wb2_grid(nv * 5)), dim3(256), 0, st, vrow.as<int>(), wrow.as<int>(), nv, B,
                         d_vstat + 5 * v0, d_wstat + v0);
      HIPCHK(hipGetLastError());
    }
    if (marked) mfx_scratch_rewind(st, mark);
  }
  return MFX_OK;
}

int wb2_stride_check(const char* fn, const mfx_rot2d* h, int64_t w_stride) {
  if (w_stride != 0 && w_stride != h->d.M)
    return mfx_fail(MFX_ERR_ARG, "%s: w_stride should be M = %d or 0 (got %lld)", fn, h->d.M, (long long)w_stride);
  return MFX_OK;
}

int wb2_check(const char* fn, const mfx_rot2d* h, int64_t w_stride, int F, int csf_on, const void* sig_csf, int B, int kind,
              const void* groups, int nprop, const void* props, int Q, const void* q) {
  if (!h) return mfx_fail(MFX_ERR_ARG, "%s: bad argument", fn);
  if (F < 0) return mfx_fail(MFX_ERR_ARG, "%s: maxfasc should not be negative, got %d", fn, F);
  if (F > WB2_MAXF) return mfx_fail(MFX_ERR_UNSUPPORTED, "%s: at most 3 fascicles (got %d)", fn, F);
  if (B < 1) return mfx_fail(MFX_ERR_ARG, "%s: B should be at least 1, got %d", fn, B);
  if (B > MFX_BOOT_MAX_B)
    return mfx_fail(MFX_ERR_UNSUPPORTED, "%s: at most %d replicates are reduced on the device (got B = %d)", fn, MFX_BOOT_MAX_B, B);
  if (Q < 0) return mfx_fail(MFX_ERR_ARG, "%s: Q should not be negative, got %d", fn, Q);
  if (Q > MFX_BOOT_MAX_Q) return mfx_fail(MFX_ERR_UNSUPPORTED, "%s: at most %d quantiles (got %d)", fn, MFX_BOOT_MAX_Q, Q);
  if (int rc = wb2_stride_check(fn, h, w_stride)) return rc;
  if (kind != MFX_BOOT_WILD && kind != MFX_BOOT_RESIDUAL)
    return mfx_fail(MFX_ERR_ARG, "%s: kind should be 0 (wild) or 1 (residual within groups), got %d", fn, kind);
  if (kind == MFX_BOOT_RESIDUAL && !groups) return mfx_fail(MFX_ERR_ARG, "%s: kind 1 needs groups", fn);
  if (nprop < 0 || (nprop > 0 && !props) || (Q > 0 && !q)) return mfx_fail(MFX_ERR_ARG, "%s: bad argument", fn);
  if (csf_on && !sig_csf) return mfx_fail(MFX_ERR_ARG, "%s: csf_on without sig_csf", fn);
  return MFX_OK;
}

// One class on device buffers (what mfx_wboot2d_fit_dev does after its checks; mfx_wboot2d_fit runs it per class chunk)
int wb2_class_dev(const mfx_rot2d* h, const BootClass& r) {
  const int M = h->d.M, N = h->d.N, F = r.F, B = r.B;
  const double* xc = r.csf_on ? r.sig_csf : nullptr;
  hipStream_t st = r.st;
  BootChunkMem mem(r, M);
  StreamMem dst(st), wst(st);
  if (int rc = mem.alloc((int64_t)B * M * (int64_t)sizeof(double) + wb2_rows_bytes(h, F, r.csf_on != 0, r.wstride, B))) return rc;
  const int64_t Vc = mem.Vc;
  HIPCHK(wst.alloc(sizeof(int) * (size_t)Vc));   // mfx_w2d.h's status of the weights (the bootstrap's own says more)
  if (!r.pred0) HIPCHK(dst.alloc(sizeof(int) * 5 * (size_t)Vc));   // the prediction's own record of the directions
  ScratchMark mark;
  const bool marked = mfx_scratch_mark(st, &mark);
  for (int64_t v0 = 0; v0 < r.V; v0 += Vc) {
    const int64_t nv = std::min(Vc, r.V - v0);
    {
      const double* y = r.Y + (size_t)v0 * M;
      const double* w = r.W + (size_t)v0 * r.wstride;
      const double* pks = F > 0 ? r.peaks + (size_t)v0 * 3 * F : nullptr;
      int32_t* vstat = r.dir_status + 5 * v0;
      // the directions of the chunk, prepared once: the own fit, the prediction and the replicate fit read them
      F2Dirs dirs(st);
      if (int rc = dirs.enqueue(h, pks, nv * F, st)) return rc;
      const double* p0 = mem.p0(v0);
      if (!r.params0)
        if (int rc = mfx_wfit2d_class_prepared(h, y, w, r.wstride, dirs.rec.p, dirs.pstat.as<int>(), F, xc, F, r.csf_on, nv,
                                               mem.par0.as<double>(), vstat, wst.as<int32_t>(), st)) return rc;
      if (!r.pred0)
        if (int rc = mfx_predict2d_launch(h, dirs.rec.p, dirs.pstat.as<int>(), F, p0, F, r.csf_on, xc, nv, nullptr, nullptr, 0, 0, 0, 0,
                                          mem.pred.as<double>(), nullptr, mem.pst.as<int32_t>(), dst.as<int32_t>(), st)) return rc;
      double* ys = mem.ys.as<double>();
      if (int rc = mfx_wboot_resample_dev(M, y, mem.pr(v0), w, r.wstride, p0, F, r.csf_on, nullptr, r.groups, r.vox ? r.vox + v0 : nullptr,
                                          nv, B, r.kind, r.inflate, r.seed, r.vox ? r.offset : r.offset + (uint64_t)v0 * (uint64_t)M, ys,
                                          nullptr, r.status + v0, st)) return rc;
      // the voxels' records (the replicate fit writes them again, the same); a failing direction comes first in the
      // status, and no NaN signal reaches a fit kernel
      if (F == 0) {
        HIPCHK(hipMemsetAsync(vstat, 0, sizeof(int32_t) * 5 * (size_t)nv, st));
      } else {
        hipLaunchKernelGGL(fit2d_status_kernel, dim3(wb2_grid(nv)), dim3(256), 0, st, dirs.pstat.as<int>(), F, nv, vstat, (int*)nullptr,
                           (double*)nullptr, mem.np);
        HIPCHK(hipGetLastError());
      }
      hipLaunchKernelGGL(wboot2d_mask_kernel, dim3((unsigned)nv), dim3(256), 0, st, r.status + v0, vstat, nv, (int64_t)B * M, ys);
      HIPCHK(hipGetLastError());
      if (int rc = wb2_rows(h, ys, w, r.wstride, pks, &dirs, F, xc, nv, B, mem.rows(v0), vstat, wst.as<int32_t>(), mem.budget(), st))
        return rc;
      if (int rc = mem.gather_reduce(v0, nv, N)) return rc;
    }
    if (marked) mfx_scratch_rewind(st, mark);
  }
  return MFX_OK;
}

}  // namespace

extern "C" int mfx_wboot2d_abi_version(void) { return 1; }

extern "C" int mfx_wboot2d_rep_tile(void) { return B2_R; }

extern "C" int mfx_wboot2d_max_atoms(void* hv) { return hv ? wb2_max_atoms((const mfx_rot2d*)hv) : 0; }

extern "C" void mfx_wboot2d_debug_set_force_plain(int enabled) { g_force_plain = enabled ? 1 : 0; }

extern "C" int mfx_wboot2d_fit_rows_dev(void* hv, const double* d_Ystar, const double* d_W, int64_t w_stride, const double* d_peaks,
                                        int maxfasc, int64_t V, int B, double* d_params, int32_t* d_status, int32_t* d_wstatus,
                                        void* stream) {
  const char* fn = "mfx_wboot2d_fit_rows_dev";
  if (mfx_device_count() <= 0) return mfx_no_device();
  const mfx_rot2d* h = (const mfx_rot2d*)hv;
  if (!h || V < 0 || maxfasc < 0 || (V > 0 && (!d_Ystar || !d_W || !d_params || !d_status || !d_wstatus || (maxfasc > 0 && !d_peaks))))
    return mfx_fail(MFX_ERR_ARG, "%s: bad argument", fn);
  if (B < 1) return mfx_fail(MFX_ERR_ARG, "%s: B should be at least 1, got %d", fn, B);
  if (maxfasc > WB2_MAXF) return mfx_fail(MFX_ERR_UNSUPPORTED, "%s: at most 3 fascicles (got %d)", fn, maxfasc);
  if (int rc = wb2_stride_check(fn, h, w_stride)) return rc;
  if (V == 0) return MFX_OK;
  if (int rc = mfx_require_device(h->device)) return rc;
  return wb2_rows(h, d_Ystar, d_W, w_stride, d_peaks, nullptr, maxfasc, nullptr, V, B, d_params, d_status, d_wstatus, BOOT_DEFAULT_BYTES,
                  (hipStream_t)stream);
}

extern "C" int mfx_wboot2d_fit_dev(void* hv, const double* d_Y, const double* d_W, int64_t w_stride, const double* d_peaks, int maxfasc,
                                   int csf_on, const double* d_sig_csf, const double* d_params0, const double* d_pred0,
                                   const int32_t* d_groups, const int64_t* d_vox, int64_t V, int B, int kind, int inflate, uint64_t seed,
                                   uint64_t offset, const double* d_props, int nprop, const double* d_q, int Q, int64_t max_bytes,
                                   double* d_stats, int32_t* d_agree, int32_t* d_status, int32_t* d_dir_status, double* d_keep,
                                   void* stream) {
  const char* fn = "mfx_wboot2d_fit_dev";
  if (mfx_device_count() <= 0) return mfx_no_device();
  const mfx_rot2d* h = (const mfx_rot2d*)hv;
  csf_on = csf_on != 0;
  if (int rc = wb2_check(fn, h, w_stride, maxfasc, csf_on, d_sig_csf, B, kind, d_groups, nprop, d_props, Q, d_q)) return rc;
  if (V < 0 || (V > 0 && (!d_Y || !d_W || !d_stats || !d_status || !d_dir_status || (maxfasc > 0 && (!d_peaks || !d_agree)))))
    return mfx_fail(MFX_ERR_ARG, "%s: bad argument", fn);
  if (d_pred0 && !d_params0) return mfx_fail(MFX_ERR_ARG, "%s: a prediction needs the parameters it was made from", fn);
  if (V == 0) return MFX_OK;
  if (int rc = f2_limits(fn, h, maxfasc, V)) return rc;
  if (int rc = mfx_require_device(h->device)) return rc;
  BootClass r{};
  r.Y = d_Y; r.W = d_W; r.wstride = w_stride; r.peaks = d_peaks; r.F = maxfasc; r.csf_on = csf_on; r.sig_csf = d_sig_csf;
  r.params0 = d_params0; r.pred0 = d_pred0; r.groups = d_groups; r.vox = d_vox; r.V = V; r.B = B; r.kind = kind; r.inflate = inflate != 0;
  r.seed = seed; r.offset = offset; r.props = d_props; r.nprop = nprop; r.q = d_q; r.Q = Q; r.max_bytes = max_bytes;
  r.stats = d_stats; r.agree = d_agree; r.status = d_status; r.dir_status = d_dir_status; r.keep = d_keep; r.st = (hipStream_t)stream;
  return wb2_class_dev(h, r);
}

extern "C" int mfx_wboot2d_fit(void* hv, const double* Y, const double* W, int64_t w_stride, const int32_t* K, const uint8_t* csf,
                               const double* peaks, int maxfasc, int csf_on, const double* sig_csf, const double* params0,
                               const int32_t* groups, const int64_t* vox, int64_t V, int B, int kind, int inflate, uint64_t seed,
                               uint64_t offset, const double* props, int nprop, const double* q, int Q, int64_t max_bytes, double* stats,
                               int32_t* agree, int32_t* status, int32_t* dir_status, double* keep) {
  const char* fn = "mfx_wboot2d_fit";
  if (mfx_device_count() <= 0) return mfx_no_device();
  const mfx_rot2d* h = (const mfx_rot2d*)hv;
  csf_on = csf_on != 0;
  if (int rc = wb2_check(fn, h, w_stride, maxfasc, csf_on, sig_csf, B, kind, groups, nprop, props, Q, q)) return rc;
  if (V < 0 || (V > 0 && (!Y || !W || !K || !stats || !status || !dir_status || (maxfasc > 0 && (!peaks || !agree)))))
    return mfx_fail(MFX_ERR_ARG, "%s: bad argument", fn);
  for (int i = 0; i < Q; ++i)
    if (!(q[i] >= 0.0 && q[i] <= 1.0)) return mfx_fail(MFX_ERR_ARG, "%s: q[%d] = %g outside [0, 1]", fn, i, q[i]);
  BootBatch b{};
  b.fn = fn; b.device = h->device; b.M = h->d.M; b.N = h->d.N; b.Y = Y; b.W = W; b.w_stride = w_stride; b.K = K; b.csf = csf; b.peaks = peaks;
  b.F = maxfasc; b.csf_on = csf_on; b.sig_csf = sig_csf; b.params0 = params0; b.groups = groups; b.vox = vox; b.V = V;
  b.B = B; b.kind = kind; b.inflate = inflate != 0; b.seed = seed; b.offset = offset; b.props = props; b.nprop = nprop;
  b.q = q; b.Q = Q; b.max_bytes = max_bytes; b.stats = stats; b.agree = agree; b.status = status; b.dir_status = dir_status; b.keep = keep;
  return boot_run_mixed(b, [&](const BootClass& r) { return wb2_class_dev(h, r); });
}
