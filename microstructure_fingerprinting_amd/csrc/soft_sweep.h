// soft_sweep.h -- what the objective profiles (profile.hip) and the soft fits (posterior.hip) share.
//
// Both families score every atom pair of a voxel, s = ||y||^2 - F (the single-active cases included, with CSF the
// projected three-unknown form), in kernels of one shape (the phases of fit_k2.hip), and differ in what they keep of the
// scores: a minimum per atom, a sum of exponentials per atom.  Here:
//   device  SweepArgs (the leading kernel arguments), the cut, the three scoring helpers and the verdict on a voxel's weights.
//           __device__ __forceinline__: nothing becomes a call.
//   host    the LDS byte count of the kernels' common front (sweep_front), the configuration table and its chooser
//           (sweep_pick, sweep_max_atoms, sweep_dispatch, sweep_launch_k2, sweep_launch), the record of the last form
//           launched (sweep_record, sweep_last_form: the debug hooks of both headers), the argument checks of the entry
//           points in their order (sweep_enqueue_head, SweepHostIn::stage) and the host staging on DevBuf.
// The sweep's front end inside the kernels (phases 0 and 1, the chunk generator, the A operand, the operands of a pair)
// is still written out in both files: moved into functions here, it changed the register allocation of every kernel
// (DESIGN.md 4.15).
//
// Arithmetic: the closed forms use fma() like the fit's ranking math.  The build has -ffp-contract=off; the order of
// every operation here is part of the result.
#pragma once
#include "mfx_host.h"

#include <algorithm>
#include <type_traits>

#define MFX_PROFILE_CUT 1e-8   // pairs with 1 - c^2 <= this are scored as their better single atom (the fit's MFX_DET_REL)

namespace {

constexpr size_t SWEEP_LDS_MAX = 160 * 1024;
constexpr int SWEEP_K1_WG = 256;

// the leading arguments of every kernel of the two families; ProfArgs and PostArgs add their outputs behind them
struct SweepArgs {
  TablesDev T;
  PlanDev P;
  const double* Y;      // [V x M]
  const double* peaks;  // [V x 3 K]
  const double* xc;     // [M] the CSF column (CSF variants)
};

// weights of a voxel: 3 one is negative or not finite, 4 none is positive, 0 usable.  Every thread reads all M weights
// (the address does not depend on the lane), so the answer is workgroup-uniform without a barrier.
__device__ __forceinline__ int sweep_weights_status(const double* __restrict__ wv, int M) {
  bool bad = false, pos = false;
  for (int m = 0; m < M; ++m) {
    const double w = wv[m];
    bad |= !(w >= 0.0) || !(w <= 1.79769313486231570815e308);
    pos |= w > 0.0;
  }
  return bad ? 3 : (pos ? 0 : 4);
}
// the profile's verdict, status != 0, with the scan written out again: testing the status against 0, or one scan behind
// both verdicts, moves instructions (and in places registers) in every weighted kernel of profile.hip
__device__ __forceinline__ bool sweep_weights_unusable(const double* __restrict__ wv, int M) {
  bool bad = false, pos = false;
  for (int m = 0; m < M; ++m) {
    const double w = wv[m];
    bad |= !(w >= 0.0) || !(w <= 1.79769313486231570815e308);
    pos |= w > 0.0;
  }
  return bad || !pos;
}

// score s = ||y||^2 - F of one atom pair as the fraction p / q (q > 0 whenever p > 0).  p1 = max(Y1, 0)^2 and
// p2 likewise are the single atoms' numerators (denominators A11, A22).
__device__ __forceinline__ void sweep_pair_frac(double A11, double A22, double A12, double Y1, double Y2, double p1, double p2,
                                                double& p, double& q) {
  const double d1 = fma(-A12, Y2, A22 * Y1);   // w1 Det, mf_utils.py:425
  const double d2 = fma(-A12, Y1, A11 * Y2);   // w2 Det
  const double pd = A11 * A22;
  const double Det = fma(-A12, A12, pd);
  const double num = fma(Y2, d2, Y1 * d1);     // Y1 w1 + Y2 w2, times Det
  const bool both = (d1 > 0.0) & (d2 > 0.0) & (Det > MFX_PROFILE_CUT * pd);
  const bool first = p1 * A22 >= p2 * A11;     // the better single atom (ties: the row's)
  p = both ? num : (first ? p1 : p2);
  q = both ? Det : (first ? A11 : A22);
}

// the same with the weights (CSF form): i11 = 1 / A11 (0 for a null atom), returns the score
__device__ __forceinline__ double sweep_pair_w(double A11, double A22, double A12, double Y1, double Y2, double i11, double i22,
                                               double& w1, double& w2) {
  const double d1 = fma(-A12, Y2, A22 * Y1);
  const double d2 = fma(-A12, Y1, A11 * Y2);
  const double pd = A11 * A22;
  const double Det = fma(-A12, A12, pd);
  const bool both = (d1 > 0.0) & (d2 > 0.0) & (Det > MFX_PROFILE_CUT * pd);
  const double u1 = fmax(Y1, 0.0) * i11, u2 = fmax(Y2, 0.0) * i22;   // single-atom weights
  const double s1 = Y1 * u1, s2 = Y2 * u2;
  const bool first = s1 >= s2;
  const double iD = both ? 1.0 / Det : 0.0;
  w1 = both ? d1 * iD : (first ? u1 : 0.0);
  w2 = both ? d2 * iD : (first ? 0.0 : u2);
  return both ? fma(Y2, d2, Y1 * d1) * iD : (first ? s1 : s2);
}

// statistics of an atom with the CSF column x projected out: A' = A - X^2 / xx, Y' = Y - X xy / xx; an atom
// parallel to x (A' within the cut of 0) becomes a null atom
__device__ __forceinline__ void sweep_primed(double A, double Yv, double X, double ixx, double xy, double& Ap, double& Yp,
                                             double& iAp) {
  const double xs = X * ixx;
  Ap = fma(-xs, X, A);
  Yp = fma(-xs, xy, Yv);
  const bool ok = Ap > MFX_PROFILE_CUT * A;
  Ap = ok ? Ap : 0.0;
  Yp = ok ? Yp : 0.0;
  iAp = ok ? 1.0 / Ap : 0.0;
}

// ---- K = 2: the common front of the kernels' LDS carve-up, as the host counts it.  Offsets in doubles from the start of
// LDS, in the order of the arrays; `own`: where the kernel's own doubles begin.  Behind those the ints: s_r0, then r1 and
// own_i counted in ints from s_r0.  The kernels carve the same arrays in the same order.
struct SweepFront {
  int y, x, w, t0, t1, tG, dG, A11, Y1, A22, Y2, X1, X2, own;
  int r1, own_i;
};
constexpr SweepFront sweep_front(int MP, int NP, bool bracket, bool csf, bool wgt, int nbuf, int tiles) {
  SweepFront f{};
  f.y = nbuf * tiles * MP * 16;           // sB [NBUF][TILES][MP][16]
  f.x = f.y + MP;                         // s_y [MP]
  f.w = f.x + (csf ? MP : 0);             // s_x [MP] (CSF)
  f.t0 = f.w + (wgt ? MP : 0);            // s_w [MP] sqrt(W) (WGT)
  f.t1 = f.t0 + 2 * MP;                   // s_t0 [2][MP]
  f.tG = f.t1 + (bracket ? 2 * MP : 0);   // s_t1 [2][MP] (bracket only)
  f.dG = f.tG + (bracket ? MP : 0);       // s_tG [MP]
  f.A11 = f.dG + (bracket ? MP : 0);      // s_dG [MP]
  f.Y1 = f.A11 + NP;                      // [NP] each: |d|^2 and d.y of both dictionaries
  f.A22 = f.Y1 + NP;
  f.Y2 = f.A22 + NP;
  f.X1 = f.Y2 + NP;
  f.X2 = f.X1 + (csf ? NP : 0);           // [NP] each: d.x (CSF)
  f.own = f.X2 + (csf ? NP : 0);
  f.r1 = 2 * MP;                          // s_r0 [2][MP]
  f.own_i = f.r1 + (bracket ? 2 * MP : 0);   // s_r1 [2][MP] (bracket only)
  return f;
}
// bytes of the front with own_dbl doubles and own_int ints of the kernel's own
inline size_t sweep_lds_bytes(int ksteps, int NP, bool bracket, bool csf, bool wgt, int nbuf, int tiles, size_t own_dbl, size_t own_int) {
  const SweepFront f = sweep_front(ksteps * 4, NP, bracket, csf, wgt, nbuf, tiles);
  return ((size_t)f.own + own_dbl) * 8 + ((size_t)f.own_i + own_int) * 4;
}

// the K = 1 kernels: y, x, t0, t1 [M] each, sqrt(W) [M] (WGT), then r0, r1 [M] ints and own_int ints of the kernel's own
inline size_t sweep_k1_lds_bytes(int M, bool wgt, size_t own_int) {
  return (size_t)M * ((wgt ? 5 : 4) * sizeof(double) + 2 * sizeof(int)) + own_int * sizeof(int);
}

// ---- host: configurations.  NW waves per workgroup, TILES 16-atom column tiles per D_1 chunk, NBUF LDS buffers for the
// chunks (as fit_k2.hip): (8, 2, 2) for exact-G protocols of M <= 200 without CSF where it fits; (4, 1, 2) and
// (4, 1, 1) - one wave per SIMD with the whole register file - for the CSF form (whose scan keeps twice the per-row
// operands), G-bracketed rows and larger dictionaries; the last entry for longer protocols (M <= 560).
struct SweepCfg { int ks, nw, tiles, nbuf; };
constexpr SweepCfg SWEEP_CFG[4] = {{50, 8, 2, 2}, {50, 4, 1, 2}, {50, 4, 1, 1}, {140, 4, 1, 1}};

// index into SWEEP_CFG, -1: none fits.  lds(cfg, NP): the family's LDS bytes.  M <= 200: the first three in order.
template <class Lds>
int sweep_pick(int M, bool br, bool csf, int NP, Lds lds) {
  if (M <= 200) {
    for (int c = (csf || br) ? 1 : 0; c < 3; ++c)   // the CSF scan and bracketed rows do not fit the 256 registers of the 8-wave form
      if (lds(SWEEP_CFG[c], NP) <= SWEEP_LDS_MAX) return c;
    return -1;
  }
  return lds(SWEEP_CFG[3], NP) <= SWEEP_LDS_MAX ? 3 : -1;
}
template <class Lds>
int sweep_max_atoms(int M, bool br, bool csf, Lds lds) {
  int n = 0;
  while (n < (1 << 20) && sweep_pick(M, br, csf, n + 16, lds) >= 0) n += 16;
  return n;
}

// the form of the calling thread's last K = 2 launch of this family (this header is included once per family, so each
// has its own record), for mfx_*_debug_last_config: written by the launch functors, where the template arguments are
// known, before the launch itself
struct SweepForm { int ks, nw, tiles, nbuf, br, csf, land, wgt; };
thread_local SweepForm g_sweep_last_form = {};
thread_local bool g_sweep_launched = false;
inline void sweep_record(int ks, int nw, int tiles, int nbuf, bool br, bool csf, bool land, bool wgt) {
  g_sweep_last_form = {ks, nw, tiles, nbuf, br, csf, land, wgt};
  g_sweep_launched = true;
}
// form[8] = (KSTEPS, NW, TILES, NBUF, BR, CSF, LAND, WGT); 0 (and form untouched) before the thread's first launch
inline int sweep_last_form(int* form) {
  if (!g_sweep_launched) return 0;
  if (form) {
    const SweepForm& f = g_sweep_last_form;
    const int v[8] = {f.ks, f.nw, f.tiles, f.nbuf, f.br, f.csf, f.land, f.wgt};
    std::copy(v, v + 8, form);
  }
  return 1;
}

// launch.run<KS, BR, CSF, NW, TILES, NBUF>() of configuration cfg
template <bool BR, bool CSF, class Launch>
int sweep_dispatch_cfg(const char* family, int cfg, const Launch& launch) {
  switch (cfg) {
    case 0:
      if constexpr (!CSF && !BR) return launch.template run<50, BR, CSF, 8, 2, 2>();
      return mfx_fail(MFX_ERR_ARG, "%s: no such configuration", family);
    case 1: return launch.template run<50, BR, CSF, 4, 1, 2>();
    case 2: return launch.template run<50, BR, CSF, 4, 1, 1>();
    default: return launch.template run<140, BR, CSF, 4, 1, 1>();
  }
}
template <class Launch>
int sweep_dispatch(const char* family, int cfg, bool br, bool csf, const Launch& launch) {
  if (br) return csf ? sweep_dispatch_cfg<true, true>(family, cfg, launch) : sweep_dispatch_cfg<true, false>(family, cfg, launch);
  return csf ? sweep_dispatch_cfg<false, true>(family, cfg, launch) : sweep_dispatch_cfg<false, false>(family, cfg, launch);
}
// the K = 2 launcher: the configuration that fits, or the family's limit in the message
template <class Lds, class Launch>
int sweep_launch_k2(const char* fn, const char* family, const SweepArgs& a, bool csf, Lds lds, const Launch& launch) {
  const int M = a.P.M;
  const bool br = a.P.any_bracket != 0;
  const int cfg = sweep_pick(M, br, csf, a.T.ldn, lds);
  if (cfg < 0)
    return mfx_fail(MFX_ERR_UNSUPPORTED, "%s: N = %d atoms exceed the %d that fit in LDS for this protocol (M = %d)", fn, a.T.N,
                    sweep_max_atoms(M, br, csf, lds), M);
  return sweep_dispatch(family, cfg, br, csf, launch);
}
// one kernel launch; big_lds: the kernel may need more dynamic LDS than the default limit
template <class Kern, class KArgs>
int sweep_launch(Kern kern, const KArgs& ka, int nvox, int wg, size_t lds, bool big_lds, hipStream_t st) {
  if (big_lds) HIPCHK(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(kern, dim3((unsigned)nvox), dim3(wg), lds, st, ka);
  HIPCHK(hipGetLastError());
  return MFX_OK;
}
// the limit a *_max_atoms entry point reports: the plan's protocol, 0 beyond M = 560
template <class MaxAtoms>
int sweep_plan_max_atoms(const mfx_plan* p, MaxAtoms max_atoms) {
  if (!p) return 0;
  TablesDev T;
  PlanDev P;
  int device = 0;
  mfx_plan_view(p, &T, &P, &device);
  if (P.M > 560) return 0;
  return max_atoms(P.M, P.any_bracket != 0);
}

// ---- host: argument checks.  outs: every output (and family-specific input) pointer is given.
inline int sweep_check_args(const char* fn, const mfx_plan* p, const void* Y, const void* peaks, int K, int csf_on, const void* sig_csf,
                            int64_t V, bool outs) {
  if (!p || V < 0 || (V > 0 && (!Y || !peaks || !outs))) return mfx_fail(MFX_ERR_ARG, "%s: bad argument", fn);
  if (K != 1 && K != 2)
    return mfx_fail(MFX_ERR_UNSUPPORTED, "%s: K must be 1 or 2 (got %d): three fascicles and voxels without one are out of scope", fn, K);
  if (csf_on && !sig_csf) return mfx_fail(MFX_ERR_ARG, "%s: csf_on without sig_csf", fn);
  if (V > 0x7fffffff) return mfx_fail(MFX_ERR_ARG, "%s: V too large for one call", fn);
  return MFX_OK;
}
// W [V x M] (w_stride = M) or [M] (w_stride = 0); the device and the host entry points word it differently
inline int sweep_check_weights(const char* fn, bool host, const void* W, int64_t w_stride, int M, int64_t V) {
  if (host) {
    if (!W || (w_stride != 0 && w_stride != M))
      return mfx_fail(MFX_ERR_ARG, "%s: W should be given with w_stride M = %d or 0 (got %lld)", fn, M, (long long)w_stride);
    return MFX_OK;
  }
  if (V > 0 && !W) return mfx_fail(MFX_ERR_ARG, "%s: bad argument", fn);
  if (w_stride != 0 && w_stride != M)
    return mfx_fail(MFX_ERR_ARG, "%s: w_stride should be M = %d or 0 (got %lld)", fn, M, (long long)w_stride);
  return MFX_OK;
}
// head of a device entry point: the checks in their order, then the shared arguments into *a (a ProfArgsW / PostArgsW).
// *run = false: V == 0, nothing to launch.
template <class ArgsW>
int sweep_enqueue_head(const char* fn, const mfx_plan* p, const double* d_Y, const double* d_peaks, int K, int csf_on,
                       const double* d_sig_csf, int64_t V, bool outs, bool wgt, const double* d_W, int64_t w_stride, ArgsW* a, bool* run) {
  *run = false;
  if (mfx_device_count() <= 0) return mfx_no_device();
  if (int rc = sweep_check_args(fn, p, d_Y, d_peaks, K, csf_on, d_sig_csf, V, outs)) return rc;
  int device = 0;
  mfx_plan_view(p, &a->T, &a->P, &device);
  if (a->P.M > 560) return mfx_fail(MFX_ERR_UNSUPPORTED, "%s: supports M <= 560 (got %d)", fn, a->P.M);
  if (wgt)
    if (int rc = sweep_check_weights(fn, false, d_W, w_stride, a->P.M, V)) return rc;
  if (V == 0) return MFX_OK;
  if (int rc = mfx_require_device(device)) return rc;
  a->Y = d_Y; a->peaks = d_peaks; a->xc = csf_on ? d_sig_csf : nullptr;
  a->W = d_W; a->wstride = w_stride;
  *run = true;
  return MFX_OK;
}

// head of a host entry point: the checks in their order, then the inputs on the device.  device_first: the device count
// is looked at before the plan.  *run = false: V == 0.
struct SweepHostIn {
  DevBuf<double> Y, peaks, x, W;   // x only with csf_on, W only with wgt (null otherwise)
  size_t M = 0, N = 0;
  int stage(const char* fn, const mfx_plan* p, const double* hY, const double* hpeaks, int K, int csf_on, const double* sig_csf,
            int64_t V, bool outs, bool device_first, bool wgt, const double* hW, int64_t w_stride, bool* run) {
    *run = false;
    if (device_first && mfx_device_count() <= 0) return mfx_no_device();
    if (int rc = sweep_check_args(fn, p, hY, hpeaks, K, csf_on, sig_csf, V, outs)) return rc;
    if (V == 0) return MFX_OK;
    TablesDev Td;
    PlanDev P;
    int device = 0;
    mfx_plan_view(p, &Td, &P, &device);
    if (wgt)
      if (int rc = sweep_check_weights(fn, true, hW, w_stride, P.M, V)) return rc;
    if (int rc = mfx_require_device(device)) return rc;
    M = P.M; N = Td.N;
    HIPCHK(Y.upload(hY, (size_t)V * M));
    HIPCHK(peaks.upload(hpeaks, (size_t)V * 3 * K));
    if (csf_on) HIPCHK(x.upload(sig_csf, M));
    if (wgt) HIPCHK(W.upload(hW, w_stride ? (size_t)V * M : M));
    *run = true;
    return MFX_OK;
  }
};

}  // namespace
