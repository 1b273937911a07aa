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
// the explicit solver of mfx_api.hip per voxel on the device.  This file holds the class launcher and the entry points.
#include "fit2d_kernels.h"
#include "../../include/mfx_fit2d.h"

#include <algorithm>
#include <cstring>
#include <vector>

namespace {

thread_local int g_force_explicit = 0;

const char* NO_DEVICE = "no HIP device available (this library has no CPU path)";

int f2_require_device(int device) {
  const int n = mfx_device_count();
  if (n <= 0) return mfx_fail(MFX_ERR_NO_DEVICE, "%s", NO_DEVICE);
  if (device < 0 || device >= n) return mfx_fail(MFX_ERR_ARG, "device %d out of range (have %d)", device, n);
  HIPCHK(hipSetDevice(device));
  return MFX_OK;
}

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
  // every other class: materialise the dictionaries in voxel chunks within a byte budget, explicit solver per voxel
  const size_t Ntot = (size_t)K * N + has_csf, per_vox = sizeof(double) * M * Ntot;
  size_t free_b = 0, total_b = 0, scratch_b = 0;
  HIPCHK(hipMemGetInfo(&free_b, &total_b));
  if (int rc = mfx_solve_dense_scratch_bytes(M, K, N, has_csf, &scratch_b)) return rc;
  const size_t budget = std::min<size_t>(free_b / 4, (size_t)1 << 30);
  const int64_t nvc = std::max<int64_t>(1, std::min<int64_t>(V, (int64_t)(budget / per_vox)));
  StreamMem dA(st), dS(st);
  HIPCHK(dA.alloc(per_vox * nvc));
  HIPCHK(dS.alloc(scratch_b));
  for (int64_t v0 = 0; v0 < V; v0 += nvc) {
    const int64_t nv = std::min(nvc, V - v0);
    hipLaunchKernelGGL(fit2d_mat_kernel<false>, dim3((unsigned)nv, (unsigned)((M + 7) / 8)), dim3(256), 0, st, a, ok.as<int>(), v0, K, has_csf, d_xc,
                       dA.as<double>());
    HIPCHK(hipGetLastError());
    for (int64_t q = 0; q < nv; ++q) {
      const int64_t v = v0 + q;
      if (int rc = mfx_solve_dense_dev(dA.as<double>() + (size_t)q * M * Ntot, M, K, N, has_csf, d_Y + (size_t)v * M, maxfasc, csf_on,
                                       d_params + (size_t)v * np, ok.as<int>() + v, dS.p, st)) return rc;
    }
  }
  return MFX_OK;
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
  if (mfx_device_count() <= 0) return mfx_fail(MFX_ERR_NO_DEVICE, "%s", NO_DEVICE);
  const mfx_rot2d* h = (const mfx_rot2d*)hv;
  if (!h || V < 0 || maxfasc < 0 || (V > 0 && (!d_Y || !d_params || !d_status || (maxfasc > 0 && !d_peaks))))
    return mfx_fail(MFX_ERR_ARG, "mfx_fit2d_batch_dev: bad argument");
  if (maxfasc > 3) return mfx_fail(MFX_ERR_UNSUPPORTED, "mfx_fit2d_batch_dev: at most 3 fascicles (got %d)", maxfasc);
  if (V == 0) return MFX_OK;
  if (int rc = f2_require_device(h->device)) return rc;
  return f2_class_dev(h, d_Y, d_peaks, maxfasc, nullptr, maxfasc, 0, V, d_params, d_status, (hipStream_t)stream);
}

extern "C" int mfx_fit2d_batch(void* hv, const double* Y, const int32_t* K, const uint8_t* csf, const double* peaks, int maxfasc,
                               int csf_on, const double* sig_csf, int64_t V, double* params, int32_t* status) {
  const char* fn = "mfx_fit2d_batch";
  if (mfx_device_count() <= 0) return mfx_fail(MFX_ERR_NO_DEVICE, "%s", NO_DEVICE);
  const mfx_rot2d* h = (const mfx_rot2d*)hv;
  if (!h || V < 0 || maxfasc < 0 || (V > 0 && (!Y || !K || !params || !status || (maxfasc > 0 && !peaks))))
    return mfx_fail(MFX_ERR_ARG, "%s: bad argument", fn);
  if (maxfasc > 3) return mfx_fail(MFX_ERR_UNSUPPORTED, "%s: at most 3 fascicles (got %d)", fn, maxfasc);
  csf_on = csf_on != 0;
  const int M = h->d.M, np = 1 + 2 * maxfasc + csf_on + 2;
  // bin by class (K, CSF flag) before any device call
  std::vector<std::vector<int64_t>> bins((size_t)2 * (maxfasc + 1));
  for (int64_t v = 0; v < V; ++v) {
    const int c = csf && csf[v];
    if (K[v] < 0 || K[v] > maxfasc) return mfx_fail(MFX_ERR_ARG, "%s: K[%lld] = %d outside 0..%d", fn, (long long)v, K[v], maxfasc);
    if (c && (!csf_on || !sig_csf)) return mfx_fail(MFX_ERR_ARG, "%s: voxels flagged CSF need csf_on and sig_csf", fn);
    bins[(size_t)2 * K[v] + c].push_back(v);
  }
  if (V == 0) return MFX_OK;
  if (int rc = f2_require_device(h->device)) return rc;
  DevMem dxc;
  if (sig_csf) {
    HIPCHK(dxc.alloc(sizeof(double) * M));
    HIPCHK(hipMemcpy(dxc.p, sig_csf, sizeof(double) * M, hipMemcpyHostToDevice));
  }
  for (size_t b = 0; b < bins.size(); ++b) {
    const std::vector<int64_t>& ix = bins[b];
    if (ix.empty()) continue;
    const int k = (int)(b >> 1), c = (int)(b & 1);
    const size_t nv = ix.size();
    std::vector<double> Yc(nv * M), pc(nv * 3 * (size_t)std::max(k, 1)), prm(nv * np);
    std::vector<int32_t> stc(nv * 5);
    for (size_t q = 0; q < nv; ++q) {
      std::memcpy(&Yc[q * M], Y + (size_t)ix[q] * M, sizeof(double) * M);
      if (k > 0) std::memcpy(&pc[q * 3 * k], peaks + (size_t)ix[q] * 3 * maxfasc, sizeof(double) * 3 * k);
    }
    DevMem dY, dpk, dpr, dst;
    HIPCHK(dY.alloc(sizeof(double) * Yc.size()));
    HIPCHK(dpk.alloc(sizeof(double) * pc.size()));
    HIPCHK(dpr.alloc(sizeof(double) * prm.size()));
    HIPCHK(dst.alloc(sizeof(int32_t) * stc.size()));
    HIPCHK(hipMemcpy(dY.p, Yc.data(), sizeof(double) * Yc.size(), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(dpk.p, pc.data(), sizeof(double) * pc.size(), hipMemcpyHostToDevice));
    if (int rc = f2_class_dev(h, dY.as<double>(), dpk.as<double>(), k, c ? dxc.as<double>() : nullptr, maxfasc, csf_on, (int64_t)nv,
                              dpr.as<double>(), dst.as<int32_t>(), nullptr)) return rc;
    HIPCHK(hipStreamSynchronize(nullptr));
    HIPCHK(hipMemcpy(prm.data(), dpr.p, sizeof(double) * prm.size(), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(stc.data(), dst.p, sizeof(int32_t) * stc.size(), hipMemcpyDeviceToHost));
    for (size_t q = 0; q < nv; ++q) {
      std::memcpy(params + (size_t)ix[q] * np, &prm[q * np], sizeof(double) * np);
      std::memcpy(status + (size_t)ix[q] * 5, &stc[q * 5], sizeof(int32_t) * 5);
    }
  }
  return MFX_OK;
}
