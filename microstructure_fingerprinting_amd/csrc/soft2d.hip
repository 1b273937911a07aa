// soft2d.hip -- soft fits and objective profiles of voxels measured with a 2-D (AxCaliber-like) protocol
// (include/mfx_soft2d.h): per atom of each fascicle the sum over every partner atom of exp(-(F - shift) / T), normalised
// per voxel, or the smallest F any partner reaches, on the rotated dictionaries of rotate2d.hip, never written to memory.
//
// The kernels are mfx_soft2d_k2_kernel<MODE, WGT> and mfx_soft2d_k1_kernel<MODE, WGT> of soft2d_kernels.h (described
// there), instantiated here without measurement weights (WGT = false) and by w2d.hip with them.  This file holds the
// checks, the launcher and the entry points.
#include "soft2d_kernels.h"
#include "../../include/mfx_soft2d.h"
#include "../../include/mfx_profile.h"   // mfx_profile_cut

#include <algorithm>
#include <cstring>
#include <vector>

namespace {

template <int MODE>
int s2_launch(const S2Args& a, int K, int64_t V, hipStream_t st) {
  if (K == 2) {
    const size_t lds = s2_lds_bytes(MODE, (a.N + 15) & ~15, false);
    HIPCHK(hipFuncSetAttribute((const void*)mfx_soft2d_k2_kernel<MODE, false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL((mfx_soft2d_k2_kernel<MODE, false>), dim3((unsigned)V), dim3(F2_WG), lds, st, a);
  } else {
    hipLaunchKernelGGL((mfx_soft2d_k1_kernel<MODE, false>), dim3((unsigned)V), dim3(S2_K1_WG), 0, st, a);
  }
  HIPCHK(hipGetLastError());
  return MFX_OK;
}

// every check of the entry points that needs no device: the arguments, the class, the LDS limit
int s2_check(const char* fn, int mode, const mfx_rot2d* h, const void* Y, const void* peaks, int K, const void* T, const void* shift,
             int64_t V, const void* out, const void* log_sum, const void* status, const void* dir_status) {
  const bool post = mode == S2_POST;
  if (!h || V < 0 || (V > 0 && (!Y || !peaks || !out || !dir_status || (post && (!T || !shift || !log_sum || !status)))))
    return mfx_fail(MFX_ERR_ARG, "%s: bad argument", fn);
  if (K != 1 && K != 2)
    return mfx_fail(MFX_ERR_UNSUPPORTED, "%s: K must be 1 or 2 (got %d): three fascicles and voxels without one are out of scope", fn, K);
  if (V > 0x3fffffff / K) return mfx_fail(MFX_ERR_UNSUPPORTED, "%s: more than 2^30 directions in one call", fn);
  if (((size_t)2 * h->d.K + h->d.C + 2) * (size_t)h->d.N > 0x7fffffff)
    return mfx_fail(MFX_ERR_UNSUPPORTED, "%s: tables of more than 2^31 doubles", fn);
  if (K == 2 && s2_lds_bytes(mode, (h->d.N + 15) & ~15, false) > S2_LDS_MAX)
    return mfx_fail(MFX_ERR_UNSUPPORTED, "%s: N = %d atoms exceed the %d that fit in LDS", fn, h->d.N, s2_max_atoms(mode, false));
  if (mfx_profile_cut() != MFX_SOFT2D_CUT) return mfx_fail(MFX_ERR_HIP, "%s: built with a cut other than the profile's", fn);
  return MFX_OK;
}

// shared body of the device entry points: only enqueues
int s2_enqueue(const char* fn, int mode, const mfx_rot2d* h, const double* d_Y, const double* d_peaks, int K, const double* d_T,
               const double* d_shift, int64_t V, double* d_out, double* d_log_sum, int32_t* d_status, int32_t* d_partner,
               int32_t* d_dir_status, hipStream_t st) {
  if (mfx_device_count() <= 0) return mfx_no_device();
  if (int rc = s2_check(fn, mode, h, d_Y, d_peaks, K, d_T, d_shift, V, d_out, d_log_sum, d_status, d_dir_status)) return rc;
  if (V == 0) return MFX_OK;
  if (int rc = mfx_require_device(h->device)) return rc;
  const int M = h->d.M;
  PlanMem pm(st);
  StreamMem pstat(st), rec(st);
  HIPCHK(pstat.alloc(sizeof(int) * 4 * (size_t)V * K));
  if (int rc = pm.alloc(V * K, M, pstat.as<int>())) return rc;
  if (int rc = mfx_rot2d_plan_enqueue(h, d_peaks, V * K, pm.pl, st)) return rc;
  hipLaunchKernelGGL(fit2d_status_kernel, dim3((unsigned)((V + 255) / 256)), dim3(256), 0, st, pstat.as<int>(), K, V, d_dir_status,
                     (int*)nullptr, (double*)nullptr, 0);
  HIPCHK(hipGetLastError());
  const size_t nrec = (size_t)V * K * M;
  HIPCHK(rec.alloc(nrec * sizeof(F2Rec) + 64));
  hipLaunchKernelGGL(fit2d_rec_kernel, dim3((unsigned)((nrec + 255) / 256)), dim3(256), 0, st, h->d, pm.pl, (int64_t)nrec, rec.as<F2Rec>());
  HIPCHK(hipGetLastError());
  S2Args a{};
  a.M = M; a.N = h->d.N; a.base = h->d.ky; a.rec = rec.as<F2Rec>();
  a.Y = d_Y; a.vstat = d_dir_status; a.temp = d_T; a.shift = d_shift;
  a.out = d_out; a.log_sum = d_log_sum; a.status = d_status; a.partner = d_partner;
  return mode == S2_POST ? s2_launch<S2_POST>(a, K, V, st) : s2_launch<S2_PROF>(a, K, V, st);
}

// shared body of the host entry points
int s2_host(const char* fn, int mode, const mfx_rot2d* h, const double* Y, const double* peaks, int K, const double* T,
            const double* shift, int64_t V, double* out, double* log_sum, int32_t* status, int32_t* partner, int32_t* dir_status) {
  if (mfx_device_count() <= 0) return mfx_no_device();
  if (int rc = s2_check(fn, mode, h, Y, peaks, K, T, shift, V, out, log_sum, status, dir_status)) return rc;
  if (V == 0) return MFX_OK;
  if (int rc = mfx_require_device(h->device)) return rc;
  const bool post = mode == S2_POST;
  const size_t M = h->d.M, nout = (size_t)V * K * h->d.N;
  DevMem dY, dpk, dT, dsh, dout, dls, dst, dpar, dds;
  HIPCHK(dY.alloc(sizeof(double) * V * M));
  HIPCHK(dpk.alloc(sizeof(double) * V * 3 * K));
  HIPCHK(dT.alloc(sizeof(double) * V));
  HIPCHK(dsh.alloc(sizeof(double) * V));
  HIPCHK(dout.alloc(sizeof(double) * nout));
  HIPCHK(dls.alloc(sizeof(double) * V));
  HIPCHK(dst.alloc(sizeof(int32_t) * V));
  HIPCHK(dpar.alloc(partner ? sizeof(int32_t) * nout : 0));
  HIPCHK(dds.alloc(sizeof(int32_t) * 5 * V));
  HIPCHK(hipMemcpy(dY.p, Y, sizeof(double) * V * M, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(dpk.p, peaks, sizeof(double) * V * 3 * K, hipMemcpyHostToDevice));
  if (post) {
    HIPCHK(hipMemcpy(dT.p, T, sizeof(double) * V, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(dsh.p, shift, sizeof(double) * V, hipMemcpyHostToDevice));
  }
  if (int rc = s2_enqueue(fn, mode, h, dY.as<double>(), dpk.as<double>(), K, dT.as<double>(), dsh.as<double>(), V, dout.as<double>(),
                          dls.as<double>(), dst.as<int32_t>(), partner ? dpar.as<int32_t>() : nullptr, dds.as<int32_t>(), nullptr))
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

extern "C" int mfx_soft2d_abi_version(void) { return 1; }

extern "C" int mfx_soft2d_max_atoms(void* hv, int what) {
  if (!hv || (what != S2_POST && what != S2_PROF)) return 0;
  return s2_max_atoms(what, false);
}

extern "C" int mfx_post2d_dev(void* hv, const double* d_Y, const double* d_peaks, int K, const double* d_T, const double* d_shift,
                              int64_t V, double* d_w, double* d_log_sum, int32_t* d_status, int32_t* d_dir_status, void* stream) {
  return s2_enqueue("mfx_post2d_dev", S2_POST, (const mfx_rot2d*)hv, d_Y, d_peaks, K, d_T, d_shift, V, d_w, d_log_sum, d_status,
                    nullptr, d_dir_status, (hipStream_t)stream);
}

extern "C" int mfx_post2d(void* hv, const double* Y, const double* peaks, int K, const double* T, const double* shift, int64_t V,
                          double* w, double* log_sum, int32_t* status, int32_t* dir_status) {
  return s2_host("mfx_post2d", S2_POST, (const mfx_rot2d*)hv, Y, peaks, K, T, shift, V, w, log_sum, status, nullptr, dir_status);
}

extern "C" int mfx_profile2d_dev(void* hv, const double* d_Y, const double* d_peaks, int K, int64_t V, double* d_obj,
                                 int32_t* d_partner, int32_t* d_dir_status, void* stream) {
  return s2_enqueue("mfx_profile2d_dev", S2_PROF, (const mfx_rot2d*)hv, d_Y, d_peaks, K, nullptr, nullptr, V, d_obj, nullptr, nullptr,
                    d_partner, d_dir_status, (hipStream_t)stream);
}

extern "C" int mfx_profile2d(void* hv, const double* Y, const double* peaks, int K, int64_t V, double* obj, int32_t* partner,
                             int32_t* dir_status) {
  return s2_host("mfx_profile2d", S2_PROF, (const mfx_rot2d*)hv, Y, peaks, K, nullptr, nullptr, V, obj, nullptr, nullptr, partner,
                 dir_status);
}
