// fit2d_shared.h -- what fit2d.hip (the fit of 2-D protocols), soft2d.hip (their soft fits and objective profiles) and
// w2d.hip (both with measurement weights) share beside the kernel texts of fit2d_kernels.h and soft2d_kernels.h:
// the 32-byte record of a (direction, row), the kernel that derives the records from the plan records of rotate2d.hip, the
// prepared directions of a call (F2Dirs; predict2d.hip and robust2d.hip use them too), the expression that turns a record
// into a dictionary entry, the kernel that folds the directions' status into the voxel's,
// the weighted kernels' arguments, and the geometry of the blocked cross-Gram (128 x 128 atoms per
// workgroup, rows accumulated in chunks of 8).  Every translation unit gets its own copy (anonymous namespace).
#pragma once
#include "rot2d_shared.h"

#include <algorithm>

namespace {

constexpr int F2_WG = 256;                 // 4 waves, one per SIMD and workgroup
constexpr int F2_NW = 4;
constexpr int F2_BLK = 128;                // atoms per side of a workgroup's Gram block (2 x 2 waves of 64 x 64)
constexpr int F2_MC = 8;                   // protocol rows per chunk (2 k-steps)
constexpr int F2_TS = F2_MC * 16 + 16;     // doubles per LDS tile: 16 atoms x F2_MC rows, padded (bank spread of the writers)
constexpr int F2_NT = 2 * F2_BLK / 16;     // tiles per buffer: 8 of D_0, 8 of D_1
constexpr int F2_REC = 2 * 2 * F2_MC;      // staged records: [chunk parity][side][row]

// What the kernels read of a direction, per (direction, row): the operation, S_par, the abscissa's distance to the knot
// below it, and the offsets (in doubles, relative to the knot values `base` = Rot2dDev::ky; the handle's tables sit in one
// allocation) of the row's two operands: slope and knot value, or the constant row twice, or any readable row for the
// reference's zero.  fit2d_rec_kernel derives them from the plan records once, so that an entry is two loads and r2_value.
struct __attribute__((aligned(16))) F2Rec {
  double s, dx;
  int o, a, b, pad;
};

// entry (record, atom n): the expression of mfx_rot2d_eval_kernel
__device__ __forceinline__ double f2_value(const double* __restrict__ base, const F2Rec& r, int n) {
  return r2_value(r.o, r.s, base[r.a + n], r.dx, base[r.b + n]);
}

// records of B directions from their plan records; a failing direction gets harmless ones (its voxel is skipped)
__global__ void fit2d_rec_kernel(Rot2dDev D, Rot2dPlan pl, int64_t n, F2Rec* __restrict__ rec) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  F2Rec r;
  r.s = 0.0; r.dx = 0.0; r.o = R2_OP_ZERO; r.a = 0; r.b = 0; r.pad = 0;
  if (pl.status[4 * (i / D.M)] == MFX_ROT2D_OK) {
    const int o = pl.op[i];
    r.s = pl.spar[i];
    if (o >= 1 && o < D.K) {
      r.o = o;
      r.a = (int)((D.slope - D.ky) + (int64_t)o * D.N);
      r.b = (o - 1) * D.N;
      r.dx = pl.x[i] - D.kx[o - 1];
    } else if (o <= -2 && -2 - o < D.C) {
      r.o = o;
      r.a = r.b = (int)((D.cst - D.ky) + (int64_t)(-2 - o) * D.N);
    }
  }
  rec[i] = r;
}

// what a call of B = V K directions may hold: the records are indexed with ints, the tables' offsets too
inline int f2_limits(const char* fn, const mfx_rot2d* h, int K, int64_t V) {
  if (V > 0x3fffffff / std::max(K, 1)) return mfx_fail(MFX_ERR_UNSUPPORTED, "%s: more than 2^30 directions in one call", fn);
  if (((size_t)2 * h->d.K + h->d.C + 2) * (size_t)h->d.N > 0x7fffffff)
    return mfx_fail(MFX_ERR_UNSUPPORTED, "%s: tables of more than 2^31 doubles", fn);
  return MFX_OK;
}

// The prepared directions of a call: the plan of B directions, their status records [B x 4] and the kernels' records
// [B x M], scratch of the stream's arena released with the object.  Made once, they serve every fit and every prediction
// on these directions (the class launchers of rot2d_shared.h take them).
struct F2Dirs {
  PlanMem pm;
  StreamMem pstat, rec;
  explicit F2Dirs(hipStream_t st) : pm(st), pstat(st), rec(st) {}
  int enqueue(const mfx_rot2d* h, const double* d_dirs, int64_t B, hipStream_t st) {
    const int M = h->d.M;
    HIPCHK(pstat.alloc(sizeof(int) * 4 * (size_t)std::max<int64_t>(B, 1)));
    if (int rc = pm.alloc(B, M, pstat.as<int>())) return rc;
    if (B > 0)
      if (int rc = mfx_rot2d_plan_enqueue(h, d_dirs, B, pm.pl, st)) return rc;
    const size_t nrec = (size_t)B * M;
    HIPCHK(rec.alloc(nrec * sizeof(F2Rec) + 64));
    if (nrec > 0) {
      hipLaunchKernelGGL(fit2d_rec_kernel, dim3((unsigned)((nrec + 255) / 256)), dim3(256), 0, st, h->d, pm.pl, (int64_t)nrec, rec.as<F2Rec>());
      HIPCHK(hipGetLastError());
    }
    return MFX_OK;
  }
};

// voxel record from the directions' records: the lowest failing fascicle (the record of mfx_fit2d.h).  ok (may be null):
// 1 where no direction fails; params (may be null): the NaN row of a voxel with a failing direction
__global__ void fit2d_status_kernel(const int* __restrict__ pstat, int K, int64_t V, int* __restrict__ vstat, int* __restrict__ ok,
                                    double* __restrict__ params, int np) {
  const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= V) return;
  int rec[5] = {0, 0, 0, 0, 0};
  for (int k = 0; k < K; ++k) {
    const int* s = pstat + 4 * (v * K + k);
    if (s[0] != MFX_ROT2D_OK) { rec[0] = s[0]; rec[1] = s[1]; rec[2] = s[2]; rec[3] = s[3]; rec[4] = k; break; }
  }
  for (int q = 0; q < 5; ++q) vstat[5 * v + q] = rec[q];
  if (ok) ok[v] = rec[0] == 0;
  if (params && rec[0] != 0)
    for (int q = 0; q < np; ++q) params[v * np + q] = __builtin_nan("");
}

// The arguments of the weighted (WGT) kernels of fit2d_kernels.h and soft2d_kernels.h: those of the unweighted ones and what
// w2d_prep_kernel (fit2d_kernels.h) prepared of the weights.
struct W2Args {
  int M, N;
  const double* base;
  const F2Rec* rec;      // [V K x M]
  const double* Y;       // [V x M]
  const double* W;       // [V x M] or [M]
  int64_t wstride;       // M or 0
  const double* S;       // [V x M] sqrt(W)               (w2d_prep_kernel)
  const double* Ys;      // [V x M] y' = sqrt(W) y        (w2d_prep_kernel)
  const double* sumw;    // [V] sum_m W                   (w2d_prep_kernel)
  const int* wstat;      // [V] 0 usable, 1 a negative or non-finite weight, 2 no positive weight
  const int* vstat;      // [V x 5]
  // fit
  double* params;        // [V x num_params]
  int num_params, maxfasc;
  // posterior / profile
  const double* temp;    // [V] (posterior)
  const double* shift;   // [V] (posterior)
  double* out;           // [V x K x N]: w or obj
  double* log_sum;       // [V] (posterior)
  int* status;           // [V] (posterior)
  int* partner;          // [V x K x N] or null (profile)
};

}  // namespace
