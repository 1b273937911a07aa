// fit2d.hip -- batched fit of voxels measured with a 2-D (AxCaliber-like) protocol (include/mfx_fit2d.h): per voxel the
// reference chain rotate_atom_2Dprotocol (mf_utils.py:1440-1690) per fascicle -> solve_exhaustive_posweights
// (mf_utils.py:115-607) -> params packing (mf.py:420-450).
//
// mfx_rot2d_plan_kernel (rotate2d.hip) runs over the V K directions as it is: per (direction, row) an operation, an
// abscissa and S_par.  fit2d_rec_kernel turns them once into the 32-byte records the kernels here read (operation, S_par,
// x - kx, the offsets of the row's two table operands); every dictionary entry is r2_value of rot2d_shared.h on such a
// record, the expression mfx_rot2d_eval_kernel evaluates: the fit sees bit for bit the columns mfx_rot2d_rotate returns.
//
// The kernels are those of fit2d_kernels.h (described there), instantiated here without measurement weights (WGT = false)
// and by w2d.hip with them: mfx_fit2d_k2_kernel (K = 2, no extra column), mfx_fit2d_k1_kernel (K = 1, no extra column) and,
// for every other class, fit2d_mat_kernel, which materialises the dictionaries (the same expression) in voxel chunks for
// the explicit solver of mfx_api.hip per voxel on the device (the chunk loop is mfx_solve_dense_chunks of mfx_host.h).  This
// file holds the class launcher and the entry points; the host side of a mixed batch - binning by class, the rows' gather,
// upload, download and scatter - is class_batch.h and DevBuf (mfx_host.h).
#include "fit2d_kernels.h"
#include "../../include/mfx_fit2d.h"

#include <algorithm>
#include <cstring>
#include <vector>

namespace {

thread_local int g_force_explicit = 0;

// One class on device buffers: V voxels of K fascicles each (d_peaks [V x 3 K], contiguous), with the CSF column d_xc
// or without (null) -> d_params [V x np] (np = 1 + 2 maxfasc + csf_on + 2), d_vstat [V x 5].  Only enqueues: the
// directions' plan and records (F2Dirs), then the fit on them.
int f2_class_dev(const mfx_rot2d* h, const double* d_Y, const double* d_peaks, int K, const double* d_xc, int maxfasc,
                 int csf_on, int64_t V, double* d_params, int32_t* d_vstat, hipStream_t st) {
  if (int rc = f2_limits("mfx_fit2d", h, K, V)) return rc;
  if (K == 0 && !d_xc) return mfx_fit2d_class_prepared(h, d_Y, nullptr, nullptr, K, d_xc, maxfasc, csf_on, V, d_params, d_vstat, st);
  F2Dirs dirs(st);
  if (int rc = dirs.enqueue(h, d_peaks, V * K, st)) return rc;
  return mfx_fit2d_class_prepared(h, d_Y, dirs.rec.p, dirs.pstat.as<int>(), K, d_xc, maxfasc, csf_on, V, d_params, d_vstat, st);
}

}  // namespace

// the fit of one class on prepared directions (rot2d_shared.h)
int mfx_fit2d_class_prepared(const mfx_rot2d* h, const double* d_Y, const void* d_rec, const int* d_pstat, int K, const double* d_xc,
                             int maxfasc, int csf_on, int64_t V, double* d_params, int32_t* d_vstat, hipStream_t st) {
  const int M = h->d.M, N = h->d.N, has_csf = d_xc != nullptr;
  const int np = 1 + 2 * maxfasc + csf_on + 2;
  if (int rc = f2_limits("mfx_fit2d", h, K, V)) return rc;
  HIPCHK(hipMemsetAsync(d_params, 0, sizeof(double) * (size_t)V * np, st));
  if (K == 0 && !has_csf) {   // mf.py:387: nothing to fit, a zero row
    HIPCHK(hipMemsetAsync(d_vstat, 0, sizeof(int32_t) * 5 * (size_t)V, st));
    return MFX_OK;
  }
  StreamMem ok(st);
  HIPCHK(ok.alloc(sizeof(int) * (size_t)V));
  hipLaunchKernelGGL(fit2d_status_kernel, dim3((unsigned)((V + 255) / 256)), dim3(256), 0, st, d_pstat, K, V, d_vstat,
                     ok.as<int>(), d_params, np);
  HIPCHK(hipGetLastError());
  F2Args a{};
  a.M = M; a.N = N; a.base = h->d.ky; a.rec = (const F2Rec*)d_rec;
  a.Y = d_Y; a.vstat = d_vstat; a.params = d_params; a.num_params = np; a.maxfasc = maxfasc;
  if (!g_force_explicit && !has_csf && K == 2 && f2_lds_bytes((N + 15) & ~15, false) <= F2_LDS_MAX) {
    const size_t lds = f2_lds_bytes((N + 15) & ~15, false);
    HIPCHK(hipFuncSetAttribute((const void*)mfx_fit2d_k2_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(mfx_fit2d_k2_kernel<false>, dim3((unsigned)V), dim3(F2_WG), lds, st, a);
    HIPCHK(hipGetLastError());
    return MFX_OK;
  }
  if (!g_force_explicit && !has_csf && K == 1) {
    const size_t lds = (2 * F2_K1_WG + 8 + (size_t)M) * sizeof(double);
    hipLaunchKernelGGL(mfx_fit2d_k1_kernel<false>, dim3((unsigned)V), dim3(F2_K1_WG), lds, st, a);
    HIPCHK(hipGetLastError());
    return MFX_OK;
  }
  // every other class: the dictionaries in voxel chunks, explicit solver per voxel (mfx_solve_dense_chunks, mfx_host.h)
  const int* okp = ok.as<int>();
  return mfx_solve_dense_chunks(
      M, K, N, has_csf, sizeof(double) * M * ((size_t)K * N + has_csf), V, maxfasc, csf_on, d_params, okp, st,
      [&](int64_t v0, int64_t nv, int64_t, double* dA, const double** y) -> int {
        hipLaunchKernelGGL(fit2d_mat_kernel<false>, dim3((unsigned)nv, (unsigned)((M + 7) / 8)), dim3(256), 0, st, a, okp, v0, K, has_csf, d_xc,
                           dA);
        HIPCHK(hipGetLastError());
        *y = d_Y + (size_t)v0 * M;
        return MFX_OK;
      },
      [](int64_t, int64_t) -> int { return MFX_OK; });
}

extern "C" int mfx_fit2d_abi_version(void) { return 1; }

extern "C" void mfx_fit2d_debug_set_force_explicit(int enabled) { g_force_explicit = enabled ? 1 : 0; }

extern "C" int mfx_fit2d_max_atoms(void* hv, int K) {
  if (!hv) return 0;
  if (K == 2) return f2_max_atoms_k2(false);
  if (K == 1) return 1 << 20;   // one thread per atom: no limit of its own
  return 0;
}

extern "C" int mfx_fit2d_batch_dev(void* hv, const double* d_Y, const double* d_peaks, int maxfasc, int64_t V, double* d_params,
                                   int32_t* d_status, void* stream) {
  if (mfx_device_count() <= 0) return mfx_no_device();
  const mfx_rot2d* h = (const mfx_rot2d*)hv;
  if (!h || V < 0 || maxfasc < 0 || (V > 0 && (!d_Y || !d_params || !d_status || (maxfasc > 0 && !d_peaks))))
    return mfx_fail(MFX_ERR_ARG, "mfx_fit2d_batch_dev: bad argument");
  if (maxfasc > 3) return mfx_fail(MFX_ERR_UNSUPPORTED, "mfx_fit2d_batch_dev: at most 3 fascicles (got %d)", maxfasc);
  if (V == 0) return MFX_OK;
  if (int rc = mfx_require_device(h->device)) return rc;
  return f2_class_dev(h, d_Y, d_peaks, maxfasc, nullptr, maxfasc, 0, V, d_params, d_status, (hipStream_t)stream);
}

extern "C" int mfx_fit2d_batch(void* hv, const double* Y, const int32_t* K, const uint8_t* csf, const double* peaks, int maxfasc,
                               int csf_on, const double* sig_csf, int64_t V, double* params, int32_t* status) {
  const char* fn = "mfx_fit2d_batch";
  if (mfx_device_count() <= 0) return mfx_no_device();
  const mfx_rot2d* h = (const mfx_rot2d*)hv;
  if (!h || V < 0 || maxfasc < 0 || (V > 0 && (!Y || !K || !params || !status || (maxfasc > 0 && !peaks))))
    return mfx_fail(MFX_ERR_ARG, "%s: bad argument", fn);
  if (maxfasc > 3) return mfx_fail(MFX_ERR_UNSUPPORTED, "%s: at most 3 fascicles (got %d)", fn, maxfasc);
  csf_on = csf_on != 0;
  const int M = h->d.M, np = 1 + 2 * maxfasc + csf_on + 2;
  // bin by class (K, CSF flag) before any device call
  MfxClassBins bins;
  if (int rc = mfx_class_bins(fn, K, csf, maxfasc, csf_on && sig_csf, V, &bins)) return rc;
  if (V == 0) return MFX_OK;
  if (int rc = mfx_require_device(h->device)) return rc;
  DevBuf<double> dxc;
  if (sig_csf) HIPCHK(dxc.upload(sig_csf, M));
  return mfx_class_walk(bins, SIZE_MAX, [&](int k, int c, const int64_t* ix, size_t nv) -> int {   // a bin at a time
    DevBuf<double> dY, dpk, dpr;
    DevBuf<int32_t> dst;
    HIPCHK(dY.upload_rows(Y, ix, nv, M, M));
    HIPCHK(mfx_upload_peaks(dpk, peaks, ix, nv, maxfasc, k));
    HIPCHK(dpr.alloc_n(nv * np));
    HIPCHK(dst.alloc_n(nv * 5));
    if (int rc = f2_class_dev(h, dY.get(), dpk.get(), k, c ? dxc.get() : nullptr, maxfasc, csf_on, (int64_t)nv, dpr.get(), dst.get(), nullptr))
      return rc;
    HIPCHK(hipStreamSynchronize(nullptr));
    HIPCHK(dpr.download_rows(params, ix, nv, np));
    HIPCHK(dst.download_rows(status, ix, nv, 5));
    return MFX_OK;
  });
}
