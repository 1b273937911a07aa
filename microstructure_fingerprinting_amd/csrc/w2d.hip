// w2d.hip -- measurement weights for voxels of a 2-D (AxCaliber-like) protocol (include/mfx_w2d.h): the fit of fit2d.hip
// and the soft fits and objective profiles of soft2d.hip with a weight W[v, m] >= 0 per voxel and measurement.  Per voxel
// the reference chain on rows scaled by s = sqrt(W): rotate_atom_2Dprotocol per fascicle -> rows times s ->
// solve_exhaustive_posweights on (s A, s y) -> params packing with MSE = min_obj / sum W and the weighted R2; F_W of the
// posterior and the profile is the F of mfx_soft2d.h on (s A, s y).
//
// Every dictionary entry is fl(s_m * d) with d the entry of fit2d_shared.h (f2_value / r2_value on the 32-byte records),
// bit for bit the entry mfx_rot2d_rotate returns: for W = 1 the kernels see the unweighted columns (s = 1).
//
// The fitting kernels are the WGT = true instantiations of fit2d_kernels.h (mfx_fit2d_k2_kernel, mfx_fit2d_k1_kernel,
// fit2d_mat_kernel) and soft2d_kernels.h (mfx_soft2d_k2_kernel<MODE>, mfx_soft2d_k1_kernel<MODE>); what the weights add to
// each is listed there.  w2d_prep_kernel (fit2d_kernels.h; the replicate fit of wboot2d.hip runs it too), once per call,
// one wave per voxel: the weights' status (uniform over the voxel), s [V x M], y' = s y [V x M] and sum W into the stream's
// scratch arena; NaN row of a flagged voxel (fit).  s and y' live in memory, not LDS: the kernels' LDS footprint stays
// independent of M.  This file's own:
// w2d_repack_kernel      behind the explicit solver of mfx_api.hip, which ran per voxel on the materialised (s A, y'): puts
//                        the weighted MSE and R2 into the row.
// The explicit fallback's chunk loop is mfx_solve_dense_chunks (mfx_host.h); the host side of a mixed batch is class_batch.h
// and DevBuf (mfx_host.h).
#include "fit2d_kernels.h"
#include "soft2d_kernels.h"
#include "../../include/mfx_w2d.h"

#include <algorithm>
#include <cstring>
#include <vector>

namespace {

thread_local int g_force_explicit = 0;

// The explicit solver packed the row for (s A, y'): MSE = min_obj / M and the unweighted R2 of the scaled signals.  One
// wave per voxel puts the weighted figures in: MSE (M / sum W), and the weighted R2 of y and y_rec = D w + w_csf x_csf on
// the unscaled columns, with w_k = nu_k M0 from the row.
__global__ __launch_bounds__(64) void w2d_repack_kernel(W2Args a, const int* __restrict__ ok, int64_t v0, int K, int has_csf,
                                                       const double* __restrict__ xc) {
  extern __shared__ double s_yrec[];
  const int64_t v = v0 + blockIdx.x;
  if (!ok[v]) return;
  const int M = a.M, lane = threadIdx.x;
  const double* __restrict__ yv = a.Y + (size_t)v * M;
  const double* __restrict__ wv = a.W + (size_t)v * a.wstride;
  double* row = a.params + (size_t)v * a.num_params;
  const double M0 = row[0];
  const double sc = (fabs(M0) > 0) ? M0 : 1.0;
  for (int m = lane; m < M; m += 64) {
    double yr = 0.0;
    for (int k = 0; k < K; ++k)
      yr += f2_elem(a,(size_t)(v * K + k) * M + m, (int)row[1 + a.maxfasc + k]) * (row[1 + k] * sc);
    if (has_csf) yr += xc[m] * (row[2 * a.maxfasc + 1] * sc);
    s_yrec[m] = yr;
  }
  __syncthreads();
  const double r2 = f2_r2w(yv, wv, s_yrec, M, lane);
  if (lane == 0) {
    row[a.num_params - 2] = row[a.num_params - 2] * ((double)M / a.sumw[v]);
    row[a.num_params - 1] = r2;
  }
}

// what every class launch shares beside the prepared directions (F2Dirs: the plan of the V K directions and the kernels'
// records): the voxels' direction records and the prepared weights.  Scratch of the stream's arena, released with the object.
struct W2Weights {
  StreamMem prep, ok;
  explicit W2Weights(hipStream_t st) : prep(st), ok(st) {}
  // fills a.M .. a.vstat; d_params non-null: the fit (NaN rows are written, wstat is the caller's d_wstat)
  int enqueue(const mfx_rot2d* h, const double* d_Y, const double* d_W, int64_t wstride, const void* d_rec, const int* d_pstat, int K,
              int64_t V, int32_t* d_vstat, int32_t* d_wstat, double* d_params, int np, W2Args& a, hipStream_t st) {
    const int M = h->d.M;
    hipLaunchKernelGGL(fit2d_status_kernel, dim3((unsigned)((V + 255) / 256)), dim3(256), 0, st, d_pstat, K, V, d_vstat,
                       (int*)nullptr, d_params, np);
    HIPCHK(hipGetLastError());
    // s [V x M], y' [V x M], sum W [V], and the weights' status where the caller has no array for it
    const size_t vm = (size_t)V * M;
    HIPCHK(prep.alloc(sizeof(double) * (2 * vm + (size_t)V) + sizeof(int) * (size_t)V + 64));
    HIPCHK(ok.alloc(sizeof(int) * (size_t)V));
    double* S = prep.as<double>();
    double* Ys = S + vm;
    double* sumw = Ys + vm;
    int* wstat = d_wstat ? d_wstat : (int*)(sumw + V);
    hipLaunchKernelGGL(w2d_prep_kernel, dim3((unsigned)V), dim3(64), 0, st, d_Y, d_W, wstride, M, d_vstat, S, Ys, sumw, wstat, ok.as<int>(),
                       d_params, np);
    HIPCHK(hipGetLastError());
    a.M = M; a.N = h->d.N; a.base = h->d.ky; a.rec = (const F2Rec*)d_rec;
    a.Y = d_Y; a.W = d_W; a.wstride = wstride; a.S = S; a.Ys = Ys; a.sumw = sumw; a.wstat = wstat; a.vstat = d_vstat;
    return MFX_OK;
  }
};

// directions, then weights: what the entry points that get directions run
struct W2Scratch {
  F2Dirs dirs;
  W2Weights w;
  StreamMem& ok;
  explicit W2Scratch(hipStream_t st) : dirs(st), w(st), ok(w.ok) {}
  int enqueue(const mfx_rot2d* h, const double* d_Y, const double* d_W, int64_t wstride, const double* d_peaks, int K, int64_t V,
              int32_t* d_vstat, int32_t* d_wstat, double* d_params, int np, W2Args& a, hipStream_t st) {
    if (int rc = dirs.enqueue(h, d_peaks, V * K, st)) return rc;
    return w.enqueue(h, d_Y, d_W, wstride, dirs.rec.p, dirs.pstat.as<int>(), K, V, d_vstat, d_wstat, d_params, np, a, st);
  }
};

int w2_limits(const char* fn, const mfx_rot2d* h, int K, int64_t V) {
  if (V > 0x3fffffff / std::max(K, 1)) return mfx_fail(MFX_ERR_UNSUPPORTED, "%s: more than 2^30 directions in one call", fn);
  if (((size_t)2 * h->d.K + h->d.C + 2) * (size_t)h->d.N > 0x7fffffff)
    return mfx_fail(MFX_ERR_UNSUPPORTED, "%s: tables of more than 2^31 doubles", fn);
  return MFX_OK;
}

int w2_class_fit(const mfx_rot2d* h, W2Args& a, const int* ok, int K, const double* d_xc, int maxfasc, int csf_on, int64_t V,
                 double* d_params, hipStream_t st);

// One fit class on device buffers: V voxels of K fascicles each (d_peaks [V x 3 K], contiguous), with the CSF column d_xc
// or without (null) -> d_params [V x np] (np = 1 + 2 maxfasc + csf_on + 2), d_vstat [V x 5], d_wstat [V].  Only enqueues.
int w2_class_dev(const mfx_rot2d* h, const double* d_Y, const double* d_W, int64_t wstride, const double* d_peaks, int K,
                 const double* d_xc, int maxfasc, int csf_on, int64_t V, double* d_params, int32_t* d_vstat, int32_t* d_wstat,
                 hipStream_t st) {
  const int np = 1 + 2 * maxfasc + csf_on + 2;
  if (int rc = w2_limits("mfx_wfit2d", h, K, V)) return rc;
  HIPCHK(hipMemsetAsync(d_params, 0, sizeof(double) * (size_t)V * np, st));
  W2Scratch sc(st);
  W2Args a{};
  if (int rc = sc.enqueue(h, d_Y, d_W, wstride, d_peaks, K, V, d_vstat, d_wstat, d_params, np, a, st)) return rc;
  return w2_class_fit(h, a, sc.ok.as<int>(), K, d_xc, maxfasc, csf_on, V, d_params, st);
}

// the fit of a class behind the prepared weights
int w2_class_fit(const mfx_rot2d* h, W2Args& a, const int* ok, int K, const double* d_xc, int maxfasc, int csf_on, int64_t V,
                 double* d_params, hipStream_t st) {
  const int M = h->d.M, N = h->d.N, has_csf = d_xc != nullptr;
  const int np = 1 + 2 * maxfasc + csf_on + 2;
  if (K == 0 && !has_csf) return MFX_OK;   // mf.py:387: nothing to fit, a zero row (NaN where the weights are unusable)
  a.params = d_params; a.num_params = np; a.maxfasc = maxfasc;
  if (!g_force_explicit && !has_csf && K == 2 && f2_lds_bytes((N + 15) & ~15, true) <= F2_LDS_MAX) {
    const size_t lds = f2_lds_bytes((N + 15) & ~15, true);
    HIPCHK(hipFuncSetAttribute((const void*)mfx_fit2d_k2_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(mfx_fit2d_k2_kernel<true>, dim3((unsigned)V), dim3(F2_WG), lds, st, a);
    HIPCHK(hipGetLastError());
    return MFX_OK;
  }
  if (!g_force_explicit && !has_csf && K == 1) {
    const size_t lds = (2 * F2_K1_WG + 8 + (size_t)M) * sizeof(double);
    hipLaunchKernelGGL(mfx_fit2d_k1_kernel<true>, dim3((unsigned)V), dim3(F2_K1_WG), lds, st, a);
    HIPCHK(hipGetLastError());
    return MFX_OK;
  }
  // every other class: the scaled dictionaries in voxel chunks, explicit solver per voxel on (s A, y'), then the weighted
  // figures into the chunk's rows (mfx_solve_dense_chunks, mfx_host.h)
  return mfx_solve_dense_chunks(
      M, K, N, has_csf, sizeof(double) * M * ((size_t)K * N + has_csf), V, maxfasc, csf_on, d_params, ok, st,
      [&](int64_t v0, int64_t nv, int64_t, double* dA, const double** y) -> int {
        hipLaunchKernelGGL(fit2d_mat_kernel<true>, dim3((unsigned)nv, (unsigned)((M + 7) / 8)), dim3(256), 0, st, a, ok, v0, K, has_csf, d_xc, dA);
        HIPCHK(hipGetLastError());
        *y = a.Ys + (size_t)v0 * M;
        return MFX_OK;
      },
      [&](int64_t v0, int64_t nv) -> int {
        hipLaunchKernelGGL(w2d_repack_kernel, dim3((unsigned)nv), dim3(64), sizeof(double) * M, st, a, ok, v0, K, has_csf, d_xc);
        HIPCHK(hipGetLastError());
        return MFX_OK;
      });
}

template <int MODE>
int w2_soft_launch(const W2Args& a, int K, int64_t V, hipStream_t st) {
  if (K == 2) {
    const size_t lds = s2_lds_bytes(MODE, (a.N + 15) & ~15, true);
    HIPCHK(hipFuncSetAttribute((const void*)mfx_soft2d_k2_kernel<MODE, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL((mfx_soft2d_k2_kernel<MODE, true>), dim3((unsigned)V), dim3(F2_WG), lds, st, a);
  } else {
    hipLaunchKernelGGL((mfx_soft2d_k1_kernel<MODE, true>), dim3((unsigned)V), dim3(S2_K1_WG), 0, st, a);
  }
  HIPCHK(hipGetLastError());
  return MFX_OK;
}

int w2_stride_check(const char* fn, const mfx_rot2d* h, int64_t w_stride) {
  if (w_stride != 0 && w_stride != h->d.M)
    return mfx_fail(MFX_ERR_ARG, "%s: w_stride should be M = %d or 0 (got %lld)", fn, h->d.M, (long long)w_stride);
  return MFX_OK;
}

// every check of the posterior's and the profile's entry points that needs no device: the arguments, the class, the LDS limit
int w2_soft_check(const char* fn, int mode, const mfx_rot2d* h, const void* Y, const void* W, int64_t w_stride, const void* peaks, int K,
                  const void* T, const void* shift, int64_t V, const void* out, const void* log_sum, const void* status,
                  const void* dir_status) {
  const bool post = mode == S2_POST;
  if (!h || V < 0 || (V > 0 && (!Y || !W || !peaks || !out || !dir_status || (post && (!T || !shift || !log_sum || !status)))))
    return mfx_fail(MFX_ERR_ARG, "%s: bad argument", fn);
  if (int rc = w2_stride_check(fn, h, w_stride)) return rc;
  if (K != 1 && K != 2)
    return mfx_fail(MFX_ERR_UNSUPPORTED, "%s: K must be 1 or 2 (got %d): three fascicles and voxels without one are out of scope", fn, K);
  if (int rc = w2_limits(fn, h, K, V)) return rc;
  if (K == 2 && s2_lds_bytes(mode, (h->d.N + 15) & ~15, true) > S2_LDS_MAX)
    return mfx_fail(MFX_ERR_UNSUPPORTED, "%s: N = %d atoms exceed the %d that fit in LDS", fn, h->d.N, s2_max_atoms(mode, true));
  return MFX_OK;
}

// shared body of the posterior's and the profile's device entry points: only enqueues
int w2_soft_enqueue(const char* fn, int mode, const mfx_rot2d* h, const double* d_Y, const double* d_W, int64_t w_stride,
                    const double* d_peaks, int K, const double* d_T, const double* d_shift, int64_t V, double* d_out, double* d_log_sum,
                    int32_t* d_status, int32_t* d_partner, int32_t* d_dir_status, hipStream_t st) {
  if (mfx_device_count() <= 0) return mfx_no_device();
  if (int rc = w2_soft_check(fn, mode, h, d_Y, d_W, w_stride, d_peaks, K, d_T, d_shift, V, d_out, d_log_sum, d_status, d_dir_status)) return rc;
  if (V == 0) return MFX_OK;
  if (int rc = mfx_require_device(h->device)) return rc;
  W2Scratch sc(st);
  W2Args a{};
  if (int rc = sc.enqueue(h, d_Y, d_W, w_stride, d_peaks, K, V, d_dir_status, nullptr, nullptr, 0, a, st)) return rc;
  a.temp = d_T; a.shift = d_shift; a.out = d_out; a.log_sum = d_log_sum; a.status = d_status; a.partner = d_partner;
  return mode == S2_POST ? w2_soft_launch<S2_POST>(a, K, V, st) : w2_soft_launch<S2_PROF>(a, K, V, st);
}

// shared body of the posterior's and the profile's host entry points
int w2_soft_host(const char* fn, int mode, const mfx_rot2d* h, const double* Y, const double* W, int64_t w_stride, const double* peaks,
                 int K, const double* T, const double* shift, int64_t V, double* out, double* log_sum, int32_t* status, int32_t* partner,
                 int32_t* dir_status) {
  if (mfx_device_count() <= 0) return mfx_no_device();
  if (int rc = w2_soft_check(fn, mode, h, Y, W, w_stride, peaks, K, T, shift, V, out, log_sum, status, dir_status)) return rc;
  if (V == 0) return MFX_OK;
  if (int rc = mfx_require_device(h->device)) return rc;
  const bool post = mode == S2_POST;
  const size_t M = h->d.M, nout = (size_t)V * K * h->d.N, nw = w_stride ? (size_t)V * M : M;
  DevMem dY, dW, dpk, dT, dsh, dout, dls, dst, dpar, dds;
  HIPCHK(dY.alloc(sizeof(double) * V * M));
  HIPCHK(dW.alloc(sizeof(double) * nw));
  HIPCHK(dpk.alloc(sizeof(double) * V * 3 * K));
  HIPCHK(dT.alloc(sizeof(double) * V));
  HIPCHK(dsh.alloc(sizeof(double) * V));
  HIPCHK(dout.alloc(sizeof(double) * nout));
  HIPCHK(dls.alloc(sizeof(double) * V));
  HIPCHK(dst.alloc(sizeof(int32_t) * V));
  HIPCHK(dpar.alloc(partner ? sizeof(int32_t) * nout : 0));
  HIPCHK(dds.alloc(sizeof(int32_t) * 5 * V));
  HIPCHK(hipMemcpy(dY.p, Y, sizeof(double) * V * M, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(dW.p, W, sizeof(double) * nw, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(dpk.p, peaks, sizeof(double) * V * 3 * K, hipMemcpyHostToDevice));
  if (post) {
    HIPCHK(hipMemcpy(dT.p, T, sizeof(double) * V, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(dsh.p, shift, sizeof(double) * V, hipMemcpyHostToDevice));
  }
  if (int rc = w2_soft_enqueue(fn, mode, h, dY.as<double>(), dW.as<double>(), w_stride, dpk.as<double>(), K, dT.as<double>(), dsh.as<double>(),
                               V, dout.as<double>(), dls.as<double>(), dst.as<int32_t>(), partner ? dpar.as<int32_t>() : nullptr,
                               dds.as<int32_t>(), nullptr))
    return rc;
  HIPCHK(hipStreamSynchronize(nullptr));
  HIPCHK(hipMemcpy(out, dout.p, sizeof(double) * nout, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(dir_status, dds.p, sizeof(int32_t) * 5 * V, hipMemcpyDeviceToHost));
  if (post) {
    HIPCHK(hipMemcpy(log_sum, dls.p, sizeof(double) * V, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(status, dst.p, sizeof(int32_t) * V, hipMemcpyDeviceToHost));
  }
  if (partner) HIPCHK(hipMemcpy(partner, dpar.p, sizeof(int32_t) * nout, hipMemcpyDeviceToHost));
  return MFX_OK;
}

}  // namespace

// the weighted fit of one class on prepared directions (rot2d_shared.h)
int mfx_wfit2d_class_prepared(const mfx_rot2d* h, const double* d_Y, const double* d_W, int64_t wstride, const void* d_rec,
                              const int* d_pstat, int K, const double* d_xc, int maxfasc, int csf_on, int64_t V, double* d_params,
                              int32_t* d_vstat, int32_t* d_wstat, hipStream_t st) {
  const int np = 1 + 2 * maxfasc + csf_on + 2;
  if (int rc = w2_limits("mfx_wfit2d", h, K, V)) return rc;
  HIPCHK(hipMemsetAsync(d_params, 0, sizeof(double) * (size_t)V * np, st));
  W2Weights w(st);
  W2Args a{};
  if (int rc = w.enqueue(h, d_Y, d_W, wstride, d_rec, d_pstat, K, V, d_vstat, d_wstat, d_params, np, a, st)) return rc;
  return w2_class_fit(h, a, w.ok.as<int>(), K, d_xc, maxfasc, csf_on, V, d_params, st);
}

extern "C" int mfx_w2d_abi_version(void) { return 1; }

extern "C" void mfx_w2d_debug_set_force_explicit(int enabled) { g_force_explicit = enabled ? 1 : 0; }

extern "C" int mfx_w2d_max_atoms(void* hv, int what) {
  if (!hv) return 0;
  if (what == 0) return f2_max_atoms_k2(true);
  if (what == 1) return s2_max_atoms(S2_POST, true);
  if (what == 2) return s2_max_atoms(S2_PROF, true);
  return 0;
}

extern "C" int mfx_wfit2d_batch_dev(void* hv, const double* d_Y, const double* d_W, int64_t w_stride, const double* d_peaks, int maxfasc,
                                    int64_t V, double* d_params, int32_t* d_status, int32_t* d_wstatus, void* stream) {
  const char* fn = "mfx_wfit2d_batch_dev";
  if (mfx_device_count() <= 0) return mfx_no_device();
  const mfx_rot2d* h = (const mfx_rot2d*)hv;
  if (!h || V < 0 || maxfasc < 0 || (V > 0 && (!d_Y || !d_W || !d_params || !d_status || !d_wstatus || (maxfasc > 0 && !d_peaks))))
    return mfx_fail(MFX_ERR_ARG, "%s: bad argument", fn);
  if (maxfasc > 3) return mfx_fail(MFX_ERR_UNSUPPORTED, "%s: at most 3 fascicles (got %d)", fn, maxfasc);
  if (int rc = w2_stride_check(fn, h, w_stride)) return rc;
  if (V == 0) return MFX_OK;
  if (int rc = mfx_require_device(h->device)) return rc;
  return w2_class_dev(h, d_Y, d_W, w_stride, d_peaks, maxfasc, nullptr, maxfasc, 0, V, d_params, d_status, d_wstatus, (hipStream_t)stream);
}

extern "C" int mfx_wfit2d_batch(void* hv, const double* Y, const double* W, int64_t w_stride, const int32_t* K, const uint8_t* csf,
                                const double* peaks, int maxfasc, int csf_on, const double* sig_csf, int64_t V, double* params,
                                int32_t* status, int32_t* wstatus) {
  const char* fn = "mfx_wfit2d_batch";
  if (mfx_device_count() <= 0) return mfx_no_device();
  const mfx_rot2d* h = (const mfx_rot2d*)hv;
  if (!h || V < 0 || maxfasc < 0 || (V > 0 && (!Y || !W || !K || !params || !status || !wstatus || (maxfasc > 0 && !peaks))))
    return mfx_fail(MFX_ERR_ARG, "%s: bad argument", fn);
  if (maxfasc > 3) return mfx_fail(MFX_ERR_UNSUPPORTED, "%s: at most 3 fascicles (got %d)", fn, maxfasc);
  if (int rc = w2_stride_check(fn, h, w_stride)) return rc;
  csf_on = csf_on != 0;
  const int M = h->d.M, np = 1 + 2 * maxfasc + csf_on + 2;
  // bin by class (K, CSF flag) before any device call
  MfxClassBins bins;
  if (int rc = mfx_class_bins(fn, K, csf, maxfasc, csf_on && sig_csf, V, &bins)) return rc;
  if (V == 0) return MFX_OK;
  if (int rc = mfx_require_device(h->device)) return rc;
  DevBuf<double> dxc, dWs;
  if (sig_csf) HIPCHK(dxc.upload(sig_csf, M));
  if (w_stride == 0) HIPCHK(dWs.upload(W, M));   // the shared vector is uploaded once and read with stride 0
  return mfx_class_walk(bins, SIZE_MAX, [&](int k, int c, const int64_t* ix, size_t nv) -> int {   // a bin at a time
    DevBuf<double> dY, dW, dpk, dpr;
    DevBuf<int32_t> dst, dws;
    HIPCHK(dY.upload_rows(Y, ix, nv, M, M));
    if (w_stride) HIPCHK(dW.upload_rows(W, ix, nv, M, M));
    HIPCHK(mfx_upload_peaks(dpk, peaks, ix, nv, maxfasc, k));
    HIPCHK(dpr.alloc_n(nv * np));
    HIPCHK(dst.alloc_n(nv * 5));
    HIPCHK(dws.alloc_n(nv));
    if (int rc = w2_class_dev(h, dY.get(), w_stride ? dW.get() : dWs.get(), w_stride, dpk.get(), k, c ? dxc.get() : nullptr, maxfasc, csf_on,
                              (int64_t)nv, dpr.get(), dst.get(), dws.get(), nullptr)) return rc;
    HIPCHK(hipStreamSynchronize(nullptr));
    HIPCHK(dpr.download_rows(params, ix, nv, np));
    HIPCHK(dst.download_rows(status, ix, nv, 5));
    HIPCHK(dws.download_rows(wstatus, ix, nv, 1));
    return MFX_OK;
  });
}

extern "C" int mfx_wpost2d_dev(void* hv, const double* d_Y, const double* d_W, int64_t w_stride, const double* d_peaks, int K,
                               const double* d_T, const double* d_shift, int64_t V, double* d_w, double* d_log_sum, int32_t* d_status,
                               int32_t* d_dir_status, void* stream) {
  return w2_soft_enqueue("mfx_wpost2d_dev", S2_POST, (const mfx_rot2d*)hv, d_Y, d_W, w_stride, d_peaks, K, d_T, d_shift, V, d_w, d_log_sum,
                         d_status, nullptr, d_dir_status, (hipStream_t)stream);
}

extern "C" int mfx_wpost2d(void* hv, const double* Y, const double* W, int64_t w_stride, const double* peaks, int K, const double* T,
                           const double* shift, int64_t V, double* w, double* log_sum, int32_t* status, int32_t* dir_status) {
  return w2_soft_host("mfx_wpost2d", S2_POST, (const mfx_rot2d*)hv, Y, W, w_stride, peaks, K, T, shift, V, w, log_sum, status, nullptr,
                      dir_status);
}

extern "C" int mfx_wprofile2d_dev(void* hv, const double* d_Y, const double* d_W, int64_t w_stride, const double* d_peaks, int K, int64_t V,
                                  double* d_obj, int32_t* d_partner, int32_t* d_dir_status, void* stream) {
  return w2_soft_enqueue("mfx_wprofile2d_dev", S2_PROF, (const mfx_rot2d*)hv, d_Y, d_W, w_stride, d_peaks, K, nullptr, nullptr, V, d_obj,
                         nullptr, nullptr, d_partner, d_dir_status, (hipStream_t)stream);
}

extern "C" int mfx_wprofile2d(void* hv, const double* Y, const double* W, int64_t w_stride, const double* peaks, int K, int64_t V,
                              double* obj, int32_t* partner, int32_t* dir_status) {
  return w2_soft_host("mfx_wprofile2d", S2_PROF, (const mfx_rot2d*)hv, Y, W, w_stride, peaks, K, nullptr, nullptr, V, obj, nullptr, nullptr,
                      partner, dir_status);
}
