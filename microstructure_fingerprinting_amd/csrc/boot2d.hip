// boot2d.hip -- the bootstrap of 2-D (AxCaliber-like) protocols (include/mfx_boot2d.h): the own fit (fit2d.hip's class
// launcher), its prediction (predict2d.hip's kernel), the resampling rule, value table and statistics of boot.hip through
// their public entry points, and between them the REPLICATE FIT: B signals per voxel on one set of directions.
//
// The replicate fit (b2_rows).  One and two fascicles without a CSF column run the kernels of boot2d_kernels.h: the
// directions' records and status once per voxel (F2Dirs, fit2d_status_kernel), the column statistics in replicate tiles,
// for K = 2 the cross-Gram once per voxel into scratch G [NP x NP], then one workgroup per (voxel, replicate) that scans G
// and runs the exact stage.  A voxel's Gram is formed once, whatever B.  Scratch per voxel: 8 (NP^2 + K NP (B + 1) + B)
// bytes; the voxels go in chunks within the byte budget.  Every other class, and everything under
// mfx_boot2d_debug_set_force_plain(1), takes the plain path: the directions are copied to the replicate rows of a voxel
// chunk and fit2d.hip's class launcher runs on them untouched (records of B rows per voxel: chunks keep records and plan
// within the budget; the explicit solver behind it sizes its dictionaries' block itself, mfx_solve_dense_chunks).
// The host side of a mixed batch, the per-class arguments and the front and tail of the class loop are boot_shared.h's,
// as in boot.hip.
#include "boot2d_kernels.h"
#include "boot_shared.h"
#include "../../include/mfx_boot2d.h"
#include "../../include/mfx_fit2d.h"

#include <algorithm>
#include <cstring>
#include <vector>

namespace {

thread_local int g_force_plain = 0;

constexpr int B2_MAXF = 3;

// the voxel's record = the record of its first replicate row
__global__ void boot2d_first_row_kernel(const int* __restrict__ rows, int64_t V, int B, int* __restrict__ vstat) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= V * 5) return;
  vstat[i] = rows[(i / 5) * B * 5 + i % 5];
}
// the signals of a voxel in a non-zero status (NaN rows of the resampling rule) or with a failing direction become zero
// rows for the fit; a failing direction makes the status 2 where the prediction did not (a fascicle of weight 0)
__global__ void boot2d_mask_kernel(int* __restrict__ status, const int* __restrict__ vstat, int64_t V, int64_t per_vox,
                                   double* __restrict__ Ys) {
  const int64_t v = blockIdx.x;
  const bool dirfail = vstat[5 * v] != 0;
  const int st = status[v];
  if (st == 0 && !dirfail) return;
  for (int64_t i = threadIdx.x; i < per_vox; i += blockDim.x) Ys[v * per_vox + i] = 0.0;
  if (st == 0 && threadIdx.x == 0) status[v] = 2;
}

unsigned b2_grid(int64_t n) { return (unsigned)((n + 255) / 256); }

bool b2_shared_serves(const mfx_rot2d* h, int K, bool has_csf) {
  if (g_force_plain || has_csf) return false;
  const int N = h->d.N, NP = (N + 15) & ~15;
  if (K == 1) return true;
  return K == 2 && N <= f2_max_atoms_k2(false) && b2_k2_lds_bytes(NP, h->d.M) <= F2_LDS_MAX;
}

// scratch bytes of the replicate fit per voxel (what the chunks of the bootstrap count beside the signals)
int64_t b2_rows_bytes(const mfx_rot2d* h, int K, bool has_csf, int B) {
  const int64_t M = h->d.M, NP = (h->d.N + 15) & ~15;
  if (K == 0 && !has_csf) return 0;
  if (b2_shared_serves(h, K, has_csf)) return 8 * ((K == 2 ? NP * NP : 0) + K * NP * ((int64_t)B + 1) + B);
  return (int64_t)B * (K * (M * (int64_t)(sizeof(F2Rec) + sizeof(int) + 3 * sizeof(double)) + 24 + 16) + 20);
}

// The replicate fit of one class: V voxels of K fascicles (d_peaks [V x 3 K]), the CSF column d_xc or none, B signals
// each -> d_params [V x B x np] (np = 1 + 2 K + csf + 2), d_vstat [V x 5].  dirs: the prepared directions of the V
// voxels (null: prepared here).  Only enqueues.
int b2_rows(const mfx_rot2d* h, const double* d_Ys, const double* d_peaks, const F2Dirs* dirs, int K, const double* d_xc, int64_t V,
            int B, double* d_params, int32_t* d_vstat, int64_t budget, hipStream_t st) {
  const int M = h->d.M, N = h->d.N, NP = (N + 15) & ~15, has_csf = d_xc != nullptr;
  const int np = boot_np(K, has_csf, 0);
  if (int rc = f2_limits("mfx_boot2d", h, K, V)) return rc;
  if (V > 0x7fffffff / B) return mfx_fail(MFX_ERR_UNSUPPORTED, "mfx_boot2d: more than 2^31 replicate rows in one call");
  HIPCHK(hipMemsetAsync(d_params, 0, sizeof(double) * (size_t)V * B * np, st));
  if (K == 0 && !has_csf) {   // mf.py:387: nothing to fit, zero rows
    HIPCHK(hipMemsetAsync(d_vstat, 0, sizeof(int32_t) * 5 * (size_t)V, st));
    return MFX_OK;
  }
  if (budget <= 0) budget = BOOT_DEFAULT_BYTES;
  const int64_t per_vox = std::max<int64_t>(1, b2_rows_bytes(h, K, has_csf, B));

  if (b2_shared_serves(h, K, has_csf)) {
    F2Dirs own(st);
    if (!dirs) {
      if (int rc = own.enqueue(h, d_peaks, V * K, st)) return rc;
      dirs = &own;
    }
    hipLaunchKernelGGL(fit2d_status_kernel, dim3(b2_grid(V)), dim3(256), 0, st, dirs->pstat.as<int>(), K, V, d_vstat, (int*)nullptr,
                       (double*)nullptr, np);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(boot2d_nan_rows_kernel, dim3(b2_grid(V * B * np)), dim3(256), 0, st, d_vstat, V, (int64_t)B * np, d_params);
    HIPCHK(hipGetLastError());
    const int64_t Vc = std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(V, MFX_B2_VOX_PER_LAUNCH), budget / per_vox));
    StreamMem sa2(st), say(st), sysq(st), sG(st);
    HIPCHK(sa2.alloc(sizeof(double) * (size_t)Vc * K * NP));
    HIPCHK(say.alloc(sizeof(double) * (size_t)Vc * B * K * NP));
    HIPCHK(sysq.alloc(sizeof(double) * (size_t)Vc * B));
    if (K == 2) HIPCHK(sG.alloc(sizeof(double) * (size_t)Vc * NP * NP));
    const size_t lds2 = b2_k2_lds_bytes(NP, M);
    if (K == 2 && lds2 > 64 * 1024)
      HIPCHK(hipFuncSetAttribute((const void*)boot2d_k2_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds2));
    for (int64_t v0 = 0; v0 < V; v0 += Vc) {
      const int64_t nv = std::min(Vc, V - v0);
      B2Args a{};
      a.M = M; a.N = N; a.NP = NP; a.B = B; a.base = h->d.ky;
      a.rec = dirs->rec.as<F2Rec>() + (size_t)v0 * K * M;
      a.Y = d_Ys + (size_t)v0 * B * M;
      a.vstat = d_vstat + 5 * v0;
      a.a2 = sa2.as<double>(); a.ay = say.as<double>(); a.ysq = sysq.as<double>(); a.G = sG.as<double>();
      a.params = d_params + (size_t)v0 * B * np; a.num_params = np; a.maxfasc = K;
      const dim3 gs((unsigned)((K * NP + B2_ST_WG - 1) / B2_ST_WG), (unsigned)((B + B2_R - 1) / B2_R), (unsigned)nv);
      if (K == 1) {
        hipLaunchKernelGGL((boot2d_stats_kernel<1, false>), gs, dim3(B2_ST_WG), 0, st, a);
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL((boot2d_ysq_kernel<1, false>), dim3(b2_grid(nv * B)), dim3(256), 0, st, a, nv * B);
        HIPCHK(hipGetLastError());
        const size_t lds = (2 * F2_K1_WG + 8 + (size_t)M) * sizeof(double);
        hipLaunchKernelGGL(boot2d_k1_kernel<false>, dim3((unsigned)(nv * B)), dim3(F2_K1_WG), lds, st, a);
        HIPCHK(hipGetLastError());
      } else {
        hipLaunchKernelGGL((boot2d_stats_kernel<2, false>), gs, dim3(B2_ST_WG), 0, st, a);
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL((boot2d_ysq_kernel<2, false>), dim3(b2_grid(nv * B)), dim3(256), 0, st, a, nv * B);
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL(boot2d_gram_kernel<false>, dim3((unsigned)nv), dim3(F2_WG), b2_gram_lds_bytes(), st, a, sG.as<double>());
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL(boot2d_k2_kernel<false>, dim3((unsigned)(nv * B)), dim3(F2_WG), lds2, st, a);
        HIPCHK(hipGetLastError());
      }
    }
    return MFX_OK;
  }

  // the plain path: the directions copied to the replicate rows of a voxel chunk, fit2d.hip's class launcher on them
  const int64_t Vc = std::max<int64_t>(1, std::min<int64_t>(V, budget / per_vox));
  StreamMem pk(st), vrow(st);
  HIPCHK(pk.alloc(sizeof(double) * (size_t)Vc * B * 3 * std::max(K, 1)));
  HIPCHK(vrow.alloc(sizeof(int) * (size_t)Vc * B * 5));
  ScratchMark mark;
  const bool marked = mfx_scratch_mark(st, &mark);
  for (int64_t v0 = 0; v0 < V; v0 += Vc) {
    const int64_t nv = std::min(Vc, V - v0);
    {
      F2Dirs rows(st);
      if (K > 0) {
        hipLaunchKernelGGL(boot_expand_kernel, dim3(b2_grid(nv * B * 3 * K)), dim3(256), 0, st, d_peaks + (size_t)v0 * 3 * K, nv, B, 3 * K,
                           pk.as<double>());
        HIPCHK(hipGetLastError());
      }
      if (int rc = rows.enqueue(h, pk.as<double>(), nv * B * K, st)) return rc;
      if (int rc = mfx_fit2d_class_prepared(h, d_Ys + (size_t)v0 * B * M, rows.rec.p, rows.pstat.as<int>(), K, d_xc, K, has_csf, nv * B,
                                            d_params + (size_t)v0 * B * np, vrow.as<int32_t>(), st)) return rc;
      hipLaunchKernelGGL(boot2d_first_row_kernel, dim3(b2_grid(nv * 5)), dim3(256), 0, st, vrow.as<int>(), nv, B, d_vstat + 5 * v0);
      HIPCHK(hipGetLastError());
    }
    if (marked) mfx_scratch_rewind(st, mark);
  }
  return MFX_OK;
}

int b2_check(const char* fn, const mfx_rot2d* h, int F, int csf_on, const void* sig_csf, int B, int kind, const void* groups, int nprop,
             const void* props, int Q, const void* q) {
  if (!h) return mfx_fail(MFX_ERR_ARG, "%s: bad argument", fn);
  if (F < 0) return mfx_fail(MFX_ERR_ARG, "%s: maxfasc should not be negative, got %d", fn, F);
  if (F > B2_MAXF) return mfx_fail(MFX_ERR_UNSUPPORTED, "%s: at most 3 fascicles (got %d)", fn, F);
  if (B < 1) return mfx_fail(MFX_ERR_ARG, "%s: B should be at least 1, got %d", fn, B);
  if (B > MFX_BOOT_MAX_B)
    return mfx_fail(MFX_ERR_UNSUPPORTED, "%s: at most %d replicates are reduced on the device (got B = %d)", fn, MFX_BOOT_MAX_B, B);
  if (Q < 0) return mfx_fail(MFX_ERR_ARG, "%s: Q should not be negative, got %d", fn, Q);
  if (Q > MFX_BOOT_MAX_Q) return mfx_fail(MFX_ERR_UNSUPPORTED, "%s: at most %d quantiles (got %d)", fn, MFX_BOOT_MAX_Q, Q);
  if (kind != MFX_BOOT_WILD && kind != MFX_BOOT_RESIDUAL)
    return mfx_fail(MFX_ERR_ARG, "%s: kind should be 0 (wild) or 1 (residual within groups), got %d", fn, kind);
  if (kind == MFX_BOOT_RESIDUAL && !groups) return mfx_fail(MFX_ERR_ARG, "%s: kind 1 needs groups", fn);
  if (nprop < 0 || (nprop > 0 && !props) || (Q > 0 && !q)) return mfx_fail(MFX_ERR_ARG, "%s: bad argument", fn);
  if (csf_on && !sig_csf) return mfx_fail(MFX_ERR_ARG, "%s: csf_on without sig_csf", fn);
  return MFX_OK;
}

// One class on device buffers (what mfx_boot2d_fit_dev does after its checks; mfx_boot2d_fit runs it per class chunk)
int b2_class_dev(const mfx_rot2d* h, const BootClass& r) {
  const int M = h->d.M, N = h->d.N, F = r.F, B = r.B;
  const double* xc = r.csf_on ? r.sig_csf : nullptr;
  hipStream_t st = r.st;
  BootChunkMem mem(r, M);
  StreamMem dst(st);
  if (int rc = mem.alloc((int64_t)B * M * (int64_t)sizeof(double) + b2_rows_bytes(h, F, r.csf_on != 0, B))) return rc;
  const int64_t Vc = mem.Vc;
  if (!r.pred0) HIPCHK(dst.alloc(sizeof(int) * 5 * (size_t)Vc));   // the prediction's own record of the directions
  ScratchMark mark;
  const bool marked = mfx_scratch_mark(st, &mark);
  for (int64_t v0 = 0; v0 < r.V; v0 += Vc) {
    const int64_t nv = std::min(Vc, r.V - v0);
    {
      const double* y = r.Y + (size_t)v0 * M;
      const double* pks = F > 0 ? r.peaks + (size_t)v0 * 3 * F : nullptr;
      int32_t* vstat = r.dir_status + 5 * v0;
      // the directions of the chunk, prepared once: the own fit, the prediction and the replicate fit read them
      F2Dirs dirs(st);
      if (int rc = dirs.enqueue(h, pks, nv * F, st)) return rc;
      const double* p0 = mem.p0(v0);
      if (!r.params0)
        if (int rc = mfx_fit2d_class_prepared(h, y, dirs.rec.p, dirs.pstat.as<int>(), F, xc, F, r.csf_on, nv, mem.par0.as<double>(), vstat, st))
          return rc;
      if (!r.pred0)
        if (int rc = mfx_predict2d_launch(h, dirs.rec.p, dirs.pstat.as<int>(), F, p0, F, r.csf_on, xc, nv, nullptr, nullptr, 0, 0, 0, 0,
                                          mem.pred.as<double>(), nullptr, mem.pst.as<int32_t>(), dst.as<int32_t>(), st)) return rc;
      double* ys = mem.ys.as<double>();
      if (int rc = mfx_boot_resample_dev(M, y, mem.pr(v0), p0, F, r.csf_on, 0, nullptr, r.groups, r.vox ? r.vox + v0 : nullptr, nv, B, r.kind,
                                         r.inflate, r.seed, r.vox ? r.offset : r.offset + (uint64_t)v0 * (uint64_t)M, ys, nullptr,
                                         r.status + v0, st)) return rc;
      // the voxels' records (the replicate fit writes them again, the same); then no NaN signal reaches a fit kernel
      if (F == 0 && !r.csf_on) {
        HIPCHK(hipMemsetAsync(vstat, 0, sizeof(int32_t) * 5 * (size_t)nv, st));
      } else {
        hipLaunchKernelGGL(fit2d_status_kernel, dim3(b2_grid(nv)), dim3(256), 0, st, dirs.pstat.as<int>(), F, nv, vstat, (int*)nullptr,
                           (double*)nullptr, mem.np);
        HIPCHK(hipGetLastError());
      }
      hipLaunchKernelGGL(boot2d_mask_kernel, dim3((unsigned)nv), dim3(256), 0, st, r.status + v0, vstat, nv, (int64_t)B * M, ys);
      HIPCHK(hipGetLastError());
      if (int rc = b2_rows(h, ys, pks, &dirs, F, xc, nv, B, mem.rows(v0), vstat, mem.budget(), st)) return rc;
      if (int rc = mem.gather_reduce(v0, nv, N)) return rc;
    }
    if (marked) mfx_scratch_rewind(st, mark);
  }
  return MFX_OK;
}

}  // namespace

extern "C" int mfx_boot2d_abi_version(void) { return 1; }

extern "C" int mfx_boot2d_rep_tile(void) { return B2_R; }

extern "C" void mfx_boot2d_debug_set_force_plain(int enabled) { g_force_plain = enabled ? 1 : 0; }

extern "C" int mfx_boot2d_fit_rows_dev(void* hv, const double* d_Ystar, const double* d_peaks, int maxfasc, int64_t V, int B,
                                       double* d_params, int32_t* d_status, void* stream) {
  const char* fn = "mfx_boot2d_fit_rows_dev";
  if (mfx_device_count() <= 0) return mfx_no_device();
  const mfx_rot2d* h = (const mfx_rot2d*)hv;
  if (!h || V < 0 || maxfasc < 0 || (V > 0 && (!d_Ystar || !d_params || !d_status || (maxfasc > 0 && !d_peaks))))
    return mfx_fail(MFX_ERR_ARG, "%s: bad argument", fn);
  if (B < 1) return mfx_fail(MFX_ERR_ARG, "%s: B should be at least 1, got %d", fn, B);
  if (maxfasc > B2_MAXF) return mfx_fail(MFX_ERR_UNSUPPORTED, "%s: at most 3 fascicles (got %d)", fn, maxfasc);
  if (V == 0) return MFX_OK;
  if (int rc = mfx_require_device(h->device)) return rc;
  return b2_rows(h, d_Ystar, d_peaks, nullptr, maxfasc, nullptr, V, B, d_params, d_status, BOOT_DEFAULT_BYTES, (hipStream_t)stream);
}

extern "C" int mfx_boot2d_fit_dev(void* hv, const double* d_Y, const double* d_peaks, int maxfasc, int csf_on, const double* d_sig_csf,
                                  const double* d_params0, const double* d_pred0, const int32_t* d_groups, const int64_t* d_vox,
                                  int64_t V, int B, int kind, int inflate, uint64_t seed, uint64_t offset, const double* d_props,
                                  int nprop, const double* d_q, int Q, int64_t max_bytes, double* d_stats, int32_t* d_agree,
                                  int32_t* d_status, int32_t* d_dir_status, double* d_keep, void* stream) {
  const char* fn = "mfx_boot2d_fit_dev";
  if (mfx_device_count() <= 0) return mfx_no_device();
  const mfx_rot2d* h = (const mfx_rot2d*)hv;
  csf_on = csf_on != 0;
  if (int rc = b2_check(fn, h, maxfasc, csf_on, d_sig_csf, B, kind, d_groups, nprop, d_props, Q, d_q)) return rc;
  if (V < 0 || (V > 0 && (!d_Y || !d_stats || !d_status || !d_dir_status || (maxfasc > 0 && (!d_peaks || !d_agree)))))
    return mfx_fail(MFX_ERR_ARG, "%s: bad argument", fn);
  if (d_pred0 && !d_params0) return mfx_fail(MFX_ERR_ARG, "%s: a prediction needs the parameters it was made from", fn);
  if (V == 0) return MFX_OK;
  if (int rc = f2_limits(fn, h, maxfasc, V)) return rc;
  if (int rc = mfx_require_device(h->device)) return rc;
  BootClass r{};
  r.Y = d_Y; r.peaks = d_peaks; r.F = maxfasc; r.csf_on = csf_on; r.sig_csf = d_sig_csf; r.params0 = d_params0; r.pred0 = d_pred0;
  r.groups = d_groups; r.vox = d_vox; r.V = V; r.B = B; r.kind = kind; r.inflate = inflate != 0; r.seed = seed; r.offset = offset;
  r.props = d_props; r.nprop = nprop; r.q = d_q; r.Q = Q; r.max_bytes = max_bytes;
  r.stats = d_stats; r.agree = d_agree; r.status = d_status; r.dir_status = d_dir_status; r.keep = d_keep; r.st = (hipStream_t)stream;
  return b2_class_dev(h, r);
}

extern "C" int mfx_boot2d_fit(void* hv, const double* Y, const int32_t* K, const uint8_t* csf, const double* peaks, int maxfasc,
                              int csf_on, const double* sig_csf, const double* params0, const int32_t* groups, const int64_t* vox,
                              int64_t V, int B, int kind, int inflate, uint64_t seed, uint64_t offset, const double* props, int nprop,
                              const double* q, int Q, int64_t max_bytes, double* stats, int32_t* agree, int32_t* status,
                              int32_t* dir_status, double* keep) {
  const char* fn = "mfx_boot2d_fit";
  if (mfx_device_count() <= 0) return mfx_no_device();
  const mfx_rot2d* h = (const mfx_rot2d*)hv;
  csf_on = csf_on != 0;
  if (int rc = b2_check(fn, h, maxfasc, csf_on, sig_csf, B, kind, groups, nprop, props, Q, q)) return rc;
  if (V < 0 || (V > 0 && (!Y || !K || !stats || !status || !dir_status || (maxfasc > 0 && (!peaks || !agree)))))
    return mfx_fail(MFX_ERR_ARG, "%s: bad argument", fn);
  for (int i = 0; i < Q; ++i)
    if (!(q[i] >= 0.0 && q[i] <= 1.0)) return mfx_fail(MFX_ERR_ARG, "%s: q[%d] = %g outside [0, 1]", fn, i, q[i]);
  BootBatch b{};
  b.fn = fn; b.device = h->device; b.M = h->d.M; b.N = h->d.N; b.Y = Y; b.K = K; b.csf = csf; b.peaks = peaks;
  b.F = maxfasc; b.csf_on = csf_on; b.sig_csf = sig_csf; b.params0 = params0; b.groups = groups; b.vox = vox; b.V = V;
  b.B = B; b.kind = kind; b.inflate = inflate != 0; b.seed = seed; b.offset = offset; b.props = props; b.nprop = nprop;
  b.q = q; b.Q = Q; b.max_bytes = max_bytes; b.stats = stats; b.agree = agree; b.status = status; b.dir_status = dir_status; b.keep = keep;
  return boot_run_mixed(b, [&](const BootClass& r) { return b2_class_dev(h, r); });
}
