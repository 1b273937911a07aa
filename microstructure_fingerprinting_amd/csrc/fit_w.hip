// fit_w.hip -- weighted fit (include/mfx_wfit.h): mfx_fit_batch with a weight W[v, m] >= 0 per voxel and measurement.
// Per voxel the reference chain on rows scaled by s = sqrt(W): interp_PGSE_from_multishell (mf_utils.py:1693-1956) per
// fascicle -> rows times s -> solve_exhaustive_posweights (mf_utils.py:115-607) on (s A, s y) -> params packing
// (mf.py:420-450) with MSE = min_obj / sum W and the weighted R2.
//
// Every dictionary entry is fl(s_m * d) with d the expression of mfx_device.h (mfx_eval / mfx_eval_br on mfx_row_desc)
// that mfx_rotate and the unweighted kernels evaluate, so for W = 1 the kernels here see the unweighted columns bit
// for bit (s = 1).  The one new operation of operand generation is that product.
//
// phase 0 (all kernels)  s = sqrt(W) and y' = s y of the voxel, the (direction, row) knot descriptors -> LDS.
// mfx_wfit_k2_kernel   K = 2, no extra column: one 4-wave workgroup per voxel, fit2d.hip's blocked skeleton.
//   phase 1  column statistics |a|^2, a.y' of both scaled dictionaries, one thread per atom, serial over the rows: the
//            sums the exact stage forms (only the cross terms differ between ranking and exact arithmetic).
//   phase 2  the cross-Gram D_0^T diag(W) D_1 in 128 x 128 blocks on v_mfma_f64_16x16x4_f64, accumulated over the rows
//            in chunks of 8: the 16 accumulator tiles of a wave persist across the chunks, both operands of a chunk
//            are generated (scaled) into double-buffered LDS tiles, the next chunk's before the MFMAs of the current
//            one.  Rows beyond the protocol have s = 0 on the all-zero table row.  Then fit_k2.hip's un-normalised
//            scan on the accumulator tiles: a slot keeps its best pair and is short-listed by interval (4 M eps, not
//            below MFX_A12_REL); pairs with 1 - c^2 <= MFX_DET_REL and two positive weights go to the list unranked.
//   phase 3  fit_k2.hip's exact stage on fl(s_m d): serial sums in the reference's row order, nnls2_exact, strict
//            '<' in (i1, i2) order, the family expansion, an exhaustive exact pass on short-list overflow.
// mfx_wfit_k1_kernel   K = 1, no extra column: one thread per atom, serial statistics, the reference's _1 rule.
// every other class    scaled dictionaries and y' materialised by wfit_mat_kernel in voxel chunks, the explicit solver
//                      of mfx_api.hip per voxel on (s A, s y), then wfit_repack_kernel puts the weighted MSE and R2
//                      into the row (the chunk loop is mfx_solve_dense_chunks of mfx_host.h).
// The host side of a mixed batch (mfx_wfit_batch) is class_batch.h and DevBuf (mfx_host.h).
// A voxel whose weights are unusable is skipped by every kernel (wfit_status_kernel wrote its NaN row and code).
// The fused kernels, their argument block and their LDS sizes live in wfit_kernels.h, which wboot.hip includes too.
#include "wfit_kernels.h"
#include "../../include/mfx_wfit.h"

#include <algorithm>
#include <cstring>
#include <vector>

namespace {

thread_local int g_force_explicit = 0;

// the voxels' scaled dictionaries [nv][M][Ntot] (K blocks of N columns, then the scaled CSF column) and scaled signals
// [nv][M]; grid (voxel, block of 8 rows)
__global__ __launch_bounds__(256) void wfit_mat_kernel(WArgs a, int64_t v0, int K, int has_csf, const double* __restrict__ xc,
                                                      double* __restrict__ A, double* __restrict__ Ys) {
  __shared__ RowDesc s_rd[3 * 8];
  __shared__ double s_s[8];
  const int64_t v = v0 + blockIdx.x;
  if (a.vstat[v] != 0) return;
  const int M = a.P.M, N = a.T.N, Ntot = K * N + has_csf;
  const int m0 = blockIdx.y * 8;
  const double* __restrict__ pk = a.peaks + (size_t)v * a.peaks_ld;
  const double* __restrict__ wv = a.W + (size_t)v * a.wstride;
  if ((int)threadIdx.x < 8 * K) {
    const int k = threadIdx.x / 8, m = m0 + threadIdx.x % 8;
    if (m < M) s_rd[threadIdx.x] = mfx_row_desc(a.T, a.P, m, pk[3 * k], pk[3 * k + 1], pk[3 * k + 2]);
  } else if (threadIdx.x >= 32 && threadIdx.x < 40) {
    const int m = m0 + threadIdx.x - 32;
    if (m < M) {
      const double s = sqrt(wv[m]);
      s_s[threadIdx.x - 32] = s;
      Ys[(size_t)blockIdx.x * M + m] = s * a.Y[(size_t)v * M + m];
    }
  }
  if (blockIdx.y == 0 && (int)threadIdx.x < K) mfx_check_dir(a.P, pk + 3 * threadIdx.x, (int)v);
  __syncthreads();
  for (int r = 0; r < 8; ++r) {
    const int m = m0 + r;
    if (m >= M) break;
    const double s = s_s[r], tG = a.P.tG[m], dG = a.P.dG[m];
    double* dst = A + ((size_t)blockIdx.x * M + m) * Ntot;
    for (int k = 0; k < K; ++k) {
      const RowDesc rd = s_rd[k * 8 + r];
      for (int n = threadIdx.x; n < N; n += 256) dst[k * N + n] = s * mfx_eval_br(a.T.tab, a.T.ldn, rd, tG, dG, n);
    }
    if (has_csf && threadIdx.x == 0) dst[K * N] = s * xc[m];
  }
}

// the explicit solver packed the row for (s A, s y): MSE = min_obj / M and the unweighted R2 of the scaled signals.
// One wave per voxel puts the weighted figures in: MSE M / sum W, and the weighted R2 of y and y_rec = D w + w_csf x_csf
// on the unscaled columns, with w_k = nu_k M0 from the row.
__global__ __launch_bounds__(64) void wfit_repack_kernel(WArgs a, int64_t v0, int K, int has_csf, const double* __restrict__ xc) {
  extern __shared__ double s_yrec[];
  const int64_t v = v0 + blockIdx.x;
  if (a.vstat[v] != 0) return;
  const int M = a.P.M, lane = threadIdx.x;
  const double* __restrict__ pk = a.peaks + (size_t)v * a.peaks_ld;
  const double* __restrict__ yv = a.Y + (size_t)v * M;
  const double* __restrict__ wv = a.W + (size_t)v * a.wstride;
  double* row = a.params + (size_t)v * a.num_params;
  const double M0 = row[0];
  const double sc = (fabs(M0) > 0) ? M0 : 1.0;
  for (int m = lane; m < M; m += 64) {
    double yr = 0.0;
    for (int k = 0; k < K; ++k) {
      const RowDesc rd = mfx_row_desc(a.T, a.P, m, pk[3 * k], pk[3 * k + 1], pk[3 * k + 2]);
      yr += mfx_eval_br(a.T.tab, a.T.ldn, rd, a.P.tG[m], a.P.dG[m], (int)row[1 + a.maxfasc + k]) * (row[1 + k] * sc);
    }
    if (has_csf) yr += xc[m] * (row[2 * a.maxfasc + 1] * sc);
    s_yrec[m] = yr;
  }
  __syncthreads();
  const double r2 = w_r2(yv, wv, s_yrec, M, lane);
  const double sw = w_sumw(wv, M, lane);
  if (lane == 0) {
    row[a.num_params - 2] = row[a.num_params - 2] * M / sw;
    row[a.num_params - 1] = r2;
  }
}

// One class on device buffers: V voxels of K fascicles each (d_peaks [V x 3 K], contiguous), with the CSF column d_xc
// or without (null) -> d_params [V x np] (np = 1 + 2 maxfasc + csf_on + 2), d_vstat [V].  Only enqueues.
int w_class_dev(const mfx_plan* p, const double* d_Y, const double* d_W, int64_t wstride, const double* d_peaks, int K,
                const double* d_xc, int maxfasc, int csf_on, int64_t V, double* d_params, int32_t* d_vstat, hipStream_t st) {
  WArgs a{};
  int device = 0;
  mfx_plan_view(p, &a.T, &a.P, &device);
  const int M = a.P.M, N = a.T.N, has_csf = d_xc != nullptr;
  const bool br = a.P.any_bracket != 0;
  const int np = 1 + 2 * maxfasc + csf_on + 2;
  if (V > 0x7fffffff) return mfx_fail(MFX_ERR_ARG, "mfx_wfit: V too large for one launch");
  HIPCHK(hipMemsetAsync(d_params, 0, sizeof(double) * (size_t)V * np, st));
  StreamMem ok(st);
  HIPCHK(ok.alloc(sizeof(int) * (size_t)V));
  hipLaunchKernelGGL(wfit_status_kernel, dim3((unsigned)((V + 255) / 256)), dim3(256), 0, st, d_W, wstride, M, V, d_vstat, ok.as<int>(),
                     d_params, np);
  HIPCHK(hipGetLastError());
  if (K == 0 && !has_csf) return MFX_OK;   // mf.py:387: nothing to fit, a zero row
  a.Y = d_Y; a.W = d_W; a.wstride = wstride; a.peaks = d_peaks; a.peaks_ld = 3 * K;
  a.vstat = d_vstat; a.params = d_params; a.num_params = np; a.maxfasc = maxfasc;
  const int MP = (M + W_MC - 1) & ~(W_MC - 1);
  if (!g_force_explicit && !has_csf && K == 2 && N <= w_max_atoms_k2(M, br)) {
    const size_t lds = w_lds_bytes(a.T.ldn, MP, br);
    if (br) {
      HIPCHK(hipFuncSetAttribute((const void*)(mfx_wfit_k2_kernel<true, W_PLAIN>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
      hipLaunchKernelGGL((mfx_wfit_k2_kernel<true, W_PLAIN>), dim3((unsigned)V), dim3(W_WG), lds, st, a);
    } else {
      HIPCHK(hipFuncSetAttribute((const void*)(mfx_wfit_k2_kernel<false, W_PLAIN>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
      hipLaunchKernelGGL((mfx_wfit_k2_kernel<false, W_PLAIN>), dim3((unsigned)V), dim3(W_WG), lds, st, a);
    }
    HIPCHK(hipGetLastError());
    return MFX_OK;
  }
  if (!g_force_explicit && !has_csf && K == 1 && w_k1_lds_bytes(M, MP, br) <= W_LDS_MAX) {
    const size_t lds = w_k1_lds_bytes(M, MP, br);
    if (br) {
      HIPCHK(hipFuncSetAttribute((const void*)mfx_wfit_k1_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
      hipLaunchKernelGGL(mfx_wfit_k1_kernel<true>, dim3((unsigned)V), dim3(W_K1_WG), lds, st, a);
    } else {
      HIPCHK(hipFuncSetAttribute((const void*)mfx_wfit_k1_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
      hipLaunchKernelGGL(mfx_wfit_k1_kernel<false>, dim3((unsigned)V), dim3(W_K1_WG), lds, st, a);
    }
    HIPCHK(hipGetLastError());
    return MFX_OK;
  }
  // every other class: the scaled dictionaries in voxel chunks, explicit solver per voxel (mfx_solve_dense_chunks,
  // mfx_host.h).  A chunk's block holds the dictionaries [nvc x M x Ntot] and behind them the scaled signals s y
  // [nvc x M], both written by wfit_mat_kernel; wfit_repack_kernel follows every chunk.
  if ((size_t)M * sizeof(double) > 64 * 1024) return mfx_fail(MFX_ERR_UNSUPPORTED, "mfx_wfit: more than 8192 measurements");
  const size_t Ntot = (size_t)K * N + has_csf;
  return mfx_solve_dense_chunks(
      M, K, N, has_csf, sizeof(double) * M * (Ntot + 1), V, maxfasc, csf_on, d_params, ok.as<int>(), st,
      [&](int64_t v0, int64_t nv, int64_t nvc, double* dA, const double** y) -> int {
        double* dYs = dA + (size_t)nvc * M * Ntot;
        hipLaunchKernelGGL(wfit_mat_kernel, dim3((unsigned)nv, (unsigned)((M + 7) / 8)), dim3(256), 0, st, a, v0, K, has_csf, d_xc, dA, dYs);
        HIPCHK(hipGetLastError());
        *y = dYs;
        return MFX_OK;
      },
      [&](int64_t v0, int64_t nv) -> int {
        hipLaunchKernelGGL(wfit_repack_kernel, dim3((unsigned)nv), dim3(64), sizeof(double) * M, st, a, v0, K, has_csf, d_xc);
        HIPCHK(hipGetLastError());
        return MFX_OK;
      });
}

}  // namespace

int mfx_wfit_class_dev(const mfx_plan* p, const double* d_Y, const double* d_W, int64_t wstride, const double* d_peaks, int K,
                       const double* d_xc, int maxfasc, int csf_on, int64_t V, double* d_params, int32_t* d_vstat, hipStream_t st) {
  return w_class_dev(p, d_Y, d_W, wstride, d_peaks, K, d_xc, maxfasc, csf_on, V, d_params, d_vstat, st);
}

extern "C" int mfx_wfit_abi_version(void) { return 1; }

extern "C" void mfx_wfit_debug_set_force_explicit(int enabled) { g_force_explicit = enabled ? 1 : 0; }

extern "C" int mfx_wfit_max_atoms(const void* pv, int K) {
  if (!pv) return 0;
  WArgs a{};
  int device = 0;
  mfx_plan_view((const mfx_plan*)pv, &a.T, &a.P, &device);
  const bool br = a.P.any_bracket != 0;
  const int MP = (a.P.M + W_MC - 1) & ~(W_MC - 1);
  if (K == 2) return w_max_atoms_k2(a.P.M, br);
  if (K == 1) return w_k1_lds_bytes(a.P.M, MP, br) <= W_LDS_MAX ? 1 << 20 : 0;   // one thread per atom: no limit of its own
  return 0;
}

extern "C" int mfx_wfit_batch_dev(const void* pv, const double* d_Y, const double* d_W, int64_t w_stride, const double* d_peaks,
                                  int maxfasc, int64_t V, double* d_params, int32_t* d_status, void* stream) {
  if (mfx_device_count() <= 0) return mfx_no_device();
  const mfx_plan* p = (const mfx_plan*)pv;
  if (!p || V < 0 || maxfasc < 0 || (V > 0 && (!d_Y || !d_W || !d_params || !d_status || (maxfasc > 0 && !d_peaks))))
    return mfx_fail(MFX_ERR_ARG, "mfx_wfit_batch_dev: bad argument");
  if (maxfasc > 3) return mfx_fail(MFX_ERR_UNSUPPORTED, "mfx_wfit_batch_dev: at most 3 fascicles (got %d)", maxfasc);
  WArgs a{};
  int device = 0;
  mfx_plan_view(p, &a.T, &a.P, &device);
  if (w_stride != 0 && w_stride != a.P.M)
    return mfx_fail(MFX_ERR_ARG, "mfx_wfit_batch_dev: w_stride should be M = %d or 0 (got %lld)", a.P.M, (long long)w_stride);
  if (V == 0) return MFX_OK;
  if (int rc = mfx_require_device(device)) return rc;
  return w_class_dev(p, d_Y, d_W, w_stride, d_peaks, maxfasc, nullptr, maxfasc, 0, V, d_params, d_status, (hipStream_t)stream);
}

extern "C" int mfx_wfit_batch(const void* pv, const double* Y, const double* W, int64_t w_stride, const int32_t* K,
                              const uint8_t* csf, const double* peaks, int maxfasc, int csf_on, const double* sig_csf, int64_t V,
                              double* params, int32_t* status) {
  const char* fn = "mfx_wfit_batch";
  if (mfx_device_count() <= 0) return mfx_no_device();
  const mfx_plan* p = (const mfx_plan*)pv;
  if (!p || V < 0 || maxfasc < 0 || (V > 0 && (!Y || !W || !K || !params || !status || (maxfasc > 0 && !peaks))))
    return mfx_fail(MFX_ERR_ARG, "%s: bad argument", fn);
  if (maxfasc > 3) return mfx_fail(MFX_ERR_UNSUPPORTED, "%s: at most 3 fascicles (got %d)", fn, maxfasc);
  csf_on = csf_on != 0;
  WArgs va{};
  int device = 0;
  mfx_plan_view(p, &va.T, &va.P, &device);
  const int M = va.P.M, np = 1 + 2 * maxfasc + csf_on + 2;
  if (w_stride != 0 && w_stride != M)
    return mfx_fail(MFX_ERR_ARG, "%s: w_stride should be M = %d or 0 (got %lld)", fn, M, (long long)w_stride);
  // bin by class (K, CSF flag) before any device call
  MfxClassBins bins;
  if (int rc = mfx_class_bins(fn, K, csf, maxfasc, csf_on && sig_csf, V, &bins)) return rc;
  if (V == 0) return MFX_OK;
  if (int rc = mfx_require_device(device)) return rc;
  DevBuf<double> dxc, dWs;
  if (sig_csf) HIPCHK(dxc.upload(sig_csf, M));
  if (w_stride == 0) HIPCHK(dWs.upload(W, M));   // the shared vector is uploaded once
  const size_t chunk = mfx_wfit_upload_chunk(M);   // voxels per upload
  return mfx_class_walk(bins, chunk, [&](int k, int c, const int64_t* ix, size_t nv) -> int {
    DevBuf<double> dY, dW, dpk, dpr;
    DevBuf<int32_t> dst;
    HIPCHK(dY.upload_rows(Y, ix, nv, M, M));
    if (w_stride) HIPCHK(dW.upload_rows(W, ix, nv, M, M));
    HIPCHK(mfx_upload_peaks(dpk, peaks, ix, nv, maxfasc, k));
    HIPCHK(dpr.alloc_n(nv * np));
    HIPCHK(dst.alloc_n(nv));
    if (int rc = w_class_dev(p, dY.get(), w_stride ? dW.get() : dWs.get(), w_stride, dpk.get(), k, c ? dxc.get() : nullptr, maxfasc, csf_on,
                             (int64_t)nv, dpr.get(), dst.get(), nullptr)) return rc;
    HIPCHK(hipStreamSynchronize(nullptr));
    HIPCHK(dpr.download_rows(params, ix, nv, np));
    HIPCHK(dst.download_rows(status, ix, nv, 1));
    return MFX_OK;
  });
}
