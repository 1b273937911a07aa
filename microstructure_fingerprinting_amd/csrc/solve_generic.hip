// solve_generic.hip -- explicit-dictionary solver: solve_exhaustive_posweights(A, y, dicsizes)
// (mf_utils.py:115-214) for ONE problem with arbitrary sub-dictionary sizes.
//
// The fused fit kernels never see an explicit dictionary; this path backs the drop-in mf_utils entry
// point (and reproduces the reference's own solver tests).  The launches:
//   1. mfx_gram_kernel     G = A^T A and A^T y, every entry summed sequentially over the rows exactly as
//                          the reference's precompute loops (mf_utils.py:307-325, 503-535)  -> HBM
//   2. mfx_tuple_scan      all prod(sizes) index tuples, one thread per tuple (grid-stride); scores a tuple
//                          by the NNLS optimum of its tiny Gram system, with a bound on that score's rounding
//                          error (mfx_tuple_score_err); the best upper bound of every block -> HBM, the best
//                          lower bound of all (atomicMax)
//   3. mfx_tuple_collect   the blocks whose best lies within 1e-9*||y||^2 of the best of all (the finalize
//                          stage's tie window) score their tuples again and append EVERY tuple inside the
//                          window to a candidate list (atomic counter); every other block exits at once.
//                          Two tuples whose scores differ by rounding only - the same columns in two
//                          orders, (i, j) and (j, i) of two identical sub-dictionaries - both reach the
//                          finalize stage, whatever block they sit in.
//   4. mfx_tuple_overflow  only when the list overflowed (more than MFX_SCAN_CAP tuples inside the window:
//                          massive exact ties), exits at once otherwise: every block keeps, of its tuples
//                          inside the window, the first in the reference's scan order - the first hit of
//                          all tuples inside the window is among them.
//   5. mfx_tuple_finalize  the listed candidates are re-evaluated with the
//                          reference's exact per-tuple arithmetic (_1/_2 closed forms, _3 Cramer +
//                          explicit residual, _4up active-set optimum + explicit residual), first-hit
//                          rule in the reference's scan order, outputs written.
// HBM-bound gather work; meant for correctness and convenience, not for the 1e5-voxel loop.
#pragma once
#include "fit_small.hip"  // mfx_np_sumsq
#include "nnls_small.h"

#define MFX_GK 8  // max sub-dictionaries supported by the explicit solver
#define MFX_SCAN_CAP 16384   // candidate list entries of the plain scan (>= the largest grid of the scan: the overflow pass
                             // stores one entry per block in the same arrays)

struct SolveArgs {
  const double* A;  // [M x lda] device copy
  long lda;
  int M, Kp, Ntot;
  long sizes[MFX_GK], start[MFX_GK];
  const double* y;  // [M]
  double* G;        // [Ntot x Ntot]
  double* Aty;      // [Ntot]
  double* ysq;      // [2]: sequential, pairwise
  long ntuples;
  double* blk_score;  // [list_cap] candidate list: score ...
  long* blk_tuple;    // [list_cap] ... and tuple number (after an overflow: one entry per scan block, tuple -1 = none)
  int nblocks;        // grid of the scan
  int list_cap;       // min(ntuples, MFX_SCAN_CAP) >= nblocks
  double* blk_max;    // [nblocks] best score of every scan block
  unsigned long long* smax;   // [1] bits of the best score of all tuples (a non-negative double)
  int* ncand;         // [1] tuples appended to the list; negative once it has overflowed
  // three-dictionary fast path (solve_k3.hip); all null / 0 otherwise
  const int* nblocks_dev;   // device-side number of entries in blk_score / blk_tuple (< 0: use nblocks); the plain scan: ncand
  const int* scan_enable;   // the full scan below runs only when this device flag is set
  int gram_ranking_only;    // G was summed on the matrix pipe: the finalize stage re-sums what it needs sequentially
  const int* run_if;        // null, or a device flag: every kernel of the launch sequence exits at once while it is 0 (fit_k3.hip
                            // enqueues this path for every voxel of a batch as the fallback of a candidate-list overflow)
  // outputs
  double* w;       // [Kp]
  long* sub;       // [Kp]
  double* minobj;  // [1]
  double* yrec;    // [M]
};

#ifndef MFX_SOLVE_BODIES_ONLY
__global__ void mfx_gram_kernel(SolveArgs a) {
  if (a.run_if && !*a.run_if) return;
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long nn = (long)a.Ntot * a.Ntot;
  if (idx < nn) {
    const int p = (int)(idx / a.Ntot), q = (int)(idx - (long)p * a.Ntot);
    double s = 0.0;
    for (int k = 0; k < a.M; ++k) s += a.A[k * a.lda + p] * a.A[k * a.lda + q];
    a.G[idx] = s;
  } else if (idx < nn + a.Ntot) {
    const int p = (int)(idx - nn);
    double s = 0.0;
    for (int k = 0; k < a.M; ++k) s += a.y[k] * a.A[k * a.lda + p];
    a.Aty[p] = s;
  } else if (idx == nn + a.Ntot) {
    double s = 0.0;
    for (int k = 0; k < a.M; ++k) s += a.y[k] * a.y[k];
    a.ysq[0] = s;
  } else if (idx == nn + a.Ntot + 1) {
    a.ysq[1] = mfx_np_sumsq(a.y, a.M);
    *a.smax = 0ull;   // the scan's running maximum and candidate counter start from zero in every launch sequence
    *a.ncand = 0;
  }
}
#endif

// decode tuple number t (itertools.product order: last index fastest) into absolute column indices
__device__ __forceinline__ void mfx_decode(const SolveArgs& a, long t, int col[MFX_GK]) {
  for (int k = a.Kp - 1; k >= 0; --k) {
    const long s = a.sizes[k];
    col[k] = (int)(a.start[k] + t % s);
    t /= s;
  }
}

// general feasible-support NNLS score for n <= MFX_GK columns (n >= 5 only; smaller n use closed forms)
__device__ inline double mfx_score_general(int n, const double* g /* n x n */, const double* y) {
  double best = 0.0;
  for (int mask = 1; mask < (1 << n); ++mask) {
    int idx[MFX_GK], c = 0;
    for (int k = 0; k < n; ++k)
      if (mask & (1 << k)) idx[c++] = k;
    double Am[MFX_GK][MFX_GK + 1];
    for (int p = 0; p < c; ++p) {
      for (int q = 0; q < c; ++q) Am[p][q] = g[idx[p] * n + idx[q]];
      Am[p][MFX_GK] = y[idx[p]];
    }
    bool ok = true;
    for (int p = 0; p < c && ok; ++p) {
      if (!(Am[p][p] > 1e-13 * g[idx[p] * n + idx[p]])) { ok = false; break; }
      for (int r = p + 1; r < c; ++r) {
        const double f = Am[r][p] / Am[p][p];
        for (int q = p; q < c; ++q) Am[r][q] -= f * Am[p][q];
        Am[r][MFX_GK] -= f * Am[p][MFX_GK];
      }
    }
    if (!ok) continue;
    double ws[MFX_GK], sc = 0.0;
    for (int p = c - 1; p >= 0; --p) {
      double t = Am[p][MFX_GK];
      for (int q = p + 1; q < c; ++q) t -= Am[p][q] * ws[q];
      ws[p] = t / Am[p][p];
    }
    for (int p = 0; p < c; ++p) { if (!(ws[p] >= 0.0)) ok = false; sc += ws[p] * y[idx[p]]; }
    if (ok && sc > best) best = sc;
  }
  return best;
}

__device__ inline double mfx_tuple_score(const SolveArgs& a, const int col[MFX_GK]) {
  const int n = a.Kp, N = a.Ntot;
  const double* G = a.G;
  if (n == 1) return score1(G[(long)col[0] * N + col[0]], a.Aty[col[0]]);
  if (n == 2)
    return score2(G[(long)col[0] * N + col[0]], G[(long)col[0] * N + col[1]], G[(long)col[1] * N + col[1]], a.Aty[col[0]],
                  a.Aty[col[1]]);
  if (n == 3)
    return score3(G[(long)col[0] * N + col[0]], G[(long)col[0] * N + col[1]], G[(long)col[0] * N + col[2]],
                  G[(long)col[1] * N + col[1]], G[(long)col[1] * N + col[2]], G[(long)col[2] * N + col[2]], a.Aty[col[0]],
                  a.Aty[col[1]], a.Aty[col[2]]);
  if (n == 4) {
    double g[10], y[4];
    int q = 0;
    for (int p = 0; p < 4; ++p) {
      y[p] = a.Aty[col[p]];
      for (int r = p; r < 4; ++r) g[q++] = G[(long)col[p] * N + col[r]];
    }
    return score4(g, y);
  }
  double g[MFX_GK * MFX_GK], y[MFX_GK];
  for (int p = 0; p < n; ++p) {
    y[p] = a.Aty[col[p]];
    for (int r = 0; r < n; ++r) g[p * n + r] = G[(long)col[p] * N + col[r]];
  }
  return mfx_score_general(n, g, y);
}

// ||y||^2 as the reference's kernel for this number of sub-dictionaries sums it: np.sum(y**2) in _1/_4up, sequential in _2/_3
__device__ __forceinline__ double mfx_ref_ysq(const SolveArgs& a) { return (a.Kp == 1 || a.Kp >= 4) ? a.ysq[1] : a.ysq[0]; }

// Bound on the rounding error of mfx_tuple_score for two and three sub-dictionaries.  score2 / score3 solve the tuple's
// Gram system by cofactors: with d = Det / prod |a_k|^2 the relative determinant of the system a branch solves, the
// rounding of the cofactors, of Det and of the Gram's own sums moves the score by a few eps |y|^2 / d.  A CSF column
// almost inside the span of two fascicle atoms gives d = 1e-5 .. 1e-7 on ordinary voxels: the score is then good to
// 1e-11 .. 1e-9 |y|^2 only, and a tuple that the reference's explicit residual prefers could fall out of a fixed window
// of 1e-9 |y|^2 under the best score.  MFX_SCORE_ERR: 16 eps (measured on the CSF fits of tests/_twin2d_cases.py: at
// most 3.5 eps |y|^2 / d).  The smallest d over the branches the score may have taken counts (a branch below its own
// cut - 1e-8, 1e-12 - is never taken).  Other tuple sizes: 0, as before.
#define MFX_SCORE_ERR (16.0 * 2.220446049250313e-16)
// the signal-independent part: the smallest relative determinant over the branches (1 where none counts)
__device__ inline double mfx_tuple_rel(const SolveArgs& a, const int col[MFX_GK]) {
  const int n = a.Kp, N = a.Ntot;
  const double* G = a.G;
  auto g = [&](int p, int q) { return G[(long)col[p] * N + col[q]]; };
  double rel = 1.0;
  auto pair = [&](int p, int q) {
    const double pd = g(p, p) * g(q, q), det = pd - g(p, q) * g(p, q);
    if (det > 1e-8 * pd) rel = fmin(rel, det / pd);
  };
  pair(0, 1);
  if (n == 3) {
    pair(0, 2);
    pair(1, 2);
    const double a11 = g(0, 0), a12 = g(0, 1), a13 = g(0, 2), a22 = g(1, 1), a23 = g(1, 2), a33 = g(2, 2);
    const double det = a11 * (a22 * a33 - a23 * a23) + a12 * (a13 * a23 - a12 * a33) + a13 * (a12 * a23 - a13 * a22);
    const double pd = a11 * a22 * a33;
    if (det > 1e-12 * pd) rel = fmin(rel, det / pd);
  }
  return rel;
}
__device__ inline double mfx_tuple_score_err(const SolveArgs& a, const int col[MFX_GK]) {
  if (a.Kp != 2 && a.Kp != 3) return 0.0;
  return MFX_SCORE_ERR * mfx_ref_ysq(a) / mfx_tuple_rel(a, col);
}

// lower edge of the tie window: *a.smax holds the best LOWER bound (score - error) of all tuples; a tuple is listed when
// its upper bound (score + error) reaches this edge
__device__ __forceinline__ double mfx_tie_threshold(const SolveArgs& a) {
  return __longlong_as_double((long long)*a.smax) - 1e-9 * mfx_ref_ysq(a);
}
// what the list stores for a tuple inside the window: its upper bound, not above the best lower bound - so that the
// finalize stage, which takes its window from the largest stored value, keeps every listed tuple
__device__ __forceinline__ double mfx_listed_score(const SolveArgs& a, double ub) {
  return fmin(ub, __longlong_as_double((long long)*a.smax));
}

// pass 1: the best score of every block and of all tuples.  Nothing is selected here: which tuples reach the finalize
// stage is decided against the maximum of ALL tuples, in mfx_tuple_collect.
__device__ inline void mfx_tuple_scan_body(const SolveArgs& a) {
  __shared__ double s_sc[256], s_lb[256];
  if (a.run_if && !*a.run_if) return;
  if (a.scan_enable && !*a.scan_enable) return;   // (three-dictionary fast path: only after a candidate-list overflow)
  double best = 0.0, lb = 0.0;   // the block's best upper and lower bound
  for (long t = (long)blockIdx.x * 256 + threadIdx.x; t < a.ntuples; t += (long)gridDim.x * 256) {
    int col[MFX_GK];
    mfx_decode(a, t, col);
    const double s = mfx_tuple_score(a, col);
    if (!(s > 0.0)) continue;
    const double e = mfx_tuple_score_err(a, col);
    best = fmax(best, s + e);
    lb = fmax(lb, s - e);
  }
  s_sc[threadIdx.x] = best;
  s_lb[threadIdx.x] = lb;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int i = 1; i < 256; ++i) { best = fmax(best, s_sc[i]); lb = fmax(lb, s_lb[i]); }
    a.blk_max[blockIdx.x] = best;
    if (lb > 0.0) atomicMax(a.smax, (unsigned long long)__double_as_longlong(lb));
  }
}

// reference scan-order key of a tuple: _3 iterates i3 -> i1 -> i2 (mf_utils.py:540-547), every other
// kernel in itertools/lexicographic order
__device__ __forceinline__ long mfx_order_key(const SolveArgs& a, long t) {
  if (a.Kp != 3) return t;
  const long i3 = t % a.sizes[2], i2 = (t / a.sizes[2]) % a.sizes[1], i1 = t / (a.sizes[2] * a.sizes[1]);
  return (i3 * a.sizes[0] + i1) * a.sizes[1] + i2;
}

// pass 2: every tuple inside the tie window goes to the candidate list.  Same grid as pass 1 (a block sees the tuples it
// scored there, and scores them to the same bits: the build does not contract floating point); a block whose best lies
// below the window has none and exits.  More than list_cap candidates: the counter's sign bit is set and stays.
__device__ inline void mfx_tuple_collect_body(const SolveArgs& a) {
  if (a.run_if && !*a.run_if) return;
  if (a.scan_enable && !*a.scan_enable) return;
  const double thr = mfx_tie_threshold(a);
  const double bm = a.blk_max[blockIdx.x];
  if (!(bm > 0.0) || bm < thr) return;
  for (long t = (long)blockIdx.x * 256 + threadIdx.x; t < a.ntuples; t += (long)gridDim.x * 256) {
    int col[MFX_GK];
    mfx_decode(a, t, col);
    const double s = mfx_tuple_score(a, col);
    if (!(s > 0.0)) continue;
    const double ub = s + mfx_tuple_score_err(a, col);
    if (ub < thr) continue;
    if (*(volatile int*)a.ncand < 0) return;   // overflowed: mfx_tuple_overflow takes over
    const int slot = atomicAdd(a.ncand, 1);
    if (slot >= 0 && slot < a.list_cap) {
      a.blk_score[slot] = mfx_listed_score(a, ub);
      a.blk_tuple[slot] = t;
    } else {
      atomicOr(a.ncand, (int)0x80000000);
      return;
    }
  }
}

// pass 3, only after an overflow of the list (exits at once otherwise): one entry per block - of the block's tuples
// inside the tie window the first in the reference's scan order.  The first hit among ALL tuples inside the window is
// the first of its own block, so it is kept; the finalize stage reads nblocks entries (nblocks_dev < 0).
__device__ inline void mfx_tuple_overflow_body(const SolveArgs& a) {
  __shared__ double s_sc[256];
  __shared__ long s_key[256], s_t[256];
  if (a.run_if && !*a.run_if) return;
  if (a.scan_enable && !*a.scan_enable) return;
  if (*a.ncand >= 0) return;
  const double thr = mfx_tie_threshold(a);
  const double bm = a.blk_max ? a.blk_max[blockIdx.x] : INFINITY;   // (no per-block maxima of this partition: every block looks)
  double bs = 0.0;
  long bkey = -1, bt = -1;
  if (bm > 0.0 && !(bm < thr)) {   // (uniform over the block)
    for (long t = (long)blockIdx.x * 256 + threadIdx.x; t < a.ntuples; t += (long)gridDim.x * 256) {
      int col[MFX_GK];
      mfx_decode(a, t, col);
      const double s = mfx_tuple_score(a, col);
      if (!(s > 0.0)) continue;
      const double ub = s + mfx_tuple_score_err(a, col);
      if (ub < thr) continue;
      const long key = mfx_order_key(a, t);
      if (bt < 0 || key < bkey) { bs = mfx_listed_score(a, ub); bkey = key; bt = t; }
    }
  }
  s_sc[threadIdx.x] = bs;
  s_key[threadIdx.x] = bkey;
  s_t[threadIdx.x] = bt;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int i = 1; i < 256; ++i)
      if (s_t[i] >= 0 && (bt < 0 || s_key[i] < bkey)) { bs = s_sc[i]; bkey = s_key[i]; bt = s_t[i]; }
    a.blk_score[blockIdx.x] = bs;
    a.blk_tuple[blockIdx.x] = bt;
  }
}

__device__ inline void mfx_tuple_finalize_body(const SolveArgs& a) {
  if (a.run_if && !*a.run_if) return;
  __shared__ double s_res[256];
  __shared__ long s_key[256], s_tt[256];
  __shared__ double s_w[256][MFX_GK];
  __shared__ double s_max;
  const int tid = threadIdx.x;
  const int n = a.Kp, N = a.Ntot, M = a.M;
  const double y_sq = (n == 1 || n >= 4) ? a.ysq[1] : a.ysq[0];  // np.sum(y**2) in _1/_4up, sequential in _2/_3
  const int nb = (a.nblocks_dev && *a.nblocks_dev >= 0) ? *a.nblocks_dev : a.nblocks;
  {
    double mx = 0.0;
    for (int b = tid; b < nb; b += 256) mx = fmax(mx, a.blk_score[b]);
    s_res[tid] = mx;
    __syncthreads();
    if (tid == 0) {
      for (int i = 1; i < 256; ++i) mx = fmax(mx, s_res[i]);
      s_max = mx;
    }
  }
  __syncthreads();
  const double thr = s_max - 1e-9 * y_sq;
  double bres = INFINITY, bw[MFX_GK];
  long bkey = -1, btt = -1;
  for (int k = 0; k < MFX_GK; ++k) bw[k] = 0.0;
  for (int b = tid; b < nb; b += 256) {
    const long t = a.blk_tuple[b];
    if (t < 0 || a.blk_score[b] < thr) continue;
    int col[MFX_GK];
    mfx_decode(a, t, col);
    double w[MFX_GK], res;
    for (int k = 0; k < MFX_GK; ++k) w[k] = 0.0;
    const double* G = a.G;
    if (n == 1) {
      nnls1_exact(y_sq, G[(long)col[0] * N + col[0]], a.Aty[col[0]], w[0], res);
    } else if (n == 2) {
      nnls2_exact(y_sq, G[(long)col[0] * N + col[0]], G[(long)col[0] * N + col[1]], G[(long)col[1] * N + col[1]],
                  a.Aty[col[0]], a.Aty[col[1]], w[0], w[1], res);
    } else if (n == 3) {
      auto explicit_res = [&](const double* ww) {
        double rr = 0.0;
        for (int k = 0; k < M; ++k) {
          const double t3 = (ww[0] * a.A[k * a.lda + col[0]] + ww[1] * a.A[k * a.lda + col[1]] + ww[2] * a.A[k * a.lda + col[2]] - a.y[k]);
          rr += t3 * t3;
        }
        return rr;
      };
      if (a.gram_ranking_only) {
        // the Gram came from the matrix pipe: the reference's sequential sums (mf_utils.py:503-535) for this triple
        double g11 = 0, g12 = 0, g13 = 0, g22 = 0, g23 = 0, g33 = 0, y1 = 0, y2 = 0, y3 = 0;
        for (int k = 0; k < M; ++k) {
          const double d1 = a.A[k * a.lda + col[0]], d2 = a.A[k * a.lda + col[1]], d3 = a.A[k * a.lda + col[2]], yk = a.y[k];
          g11 += d1 * d1; g22 += d2 * d2; g33 += d3 * d3; g12 += d1 * d2; g13 += d1 * d3; g23 += d2 * d3;
          y1 += yk * d1; y2 += yk * d2; y3 += yk * d3;
        }
        nnls3_cramer(y_sq, g11, g12, g13, g22, g23, g33, y1, y2, y3, explicit_res, w, res);
      } else
      nnls3_cramer(y_sq, G[(long)col[0] * N + col[0]], G[(long)col[0] * N + col[1]], G[(long)col[0] * N + col[2]],
                   G[(long)col[1] * N + col[1]], G[(long)col[1] * N + col[2]], G[(long)col[2] * N + col[2]], a.Aty[col[0]],
                   a.Aty[col[1]], a.Aty[col[2]], explicit_res, w, res);
    } else {
      // _4up: NNLS optimum from the Gram (feasible-support enumeration), residual explicitly.
      // The columns are taken in a canonical order - by |d|^2, then d.y, then position - for the elimination and for the
      // residual's sum: two tuples that hold the SAME columns in another order (identical peak directions make two
      // sub-dictionaries bit-identical: (i, j, ..) and (j, i, ..)) then go through the same operations and tie exactly,
      // as they do in the reference's Lawson-Hanson solve, and the first of them in scan order wins below.  In tuple order
      // their residuals differed in the last bits and rounding picked the winner.
      // (every K' >= 4 result's last bits follow this order, not only a mirrored tuple's)
      int ord[MFX_GK], tcol[MFX_GK];
      double dd[MFX_GK], dy[MFX_GK];
      for (int p = 0; p < n; ++p) { ord[p] = p; tcol[p] = col[p]; dd[p] = G[(long)col[p] * N + col[p]]; dy[p] = a.Aty[col[p]]; }
      for (int p = 1; p < n; ++p)
        for (int q = p; q > 0; --q) {
          const int u = ord[q - 1], v = ord[q];
          if (dd[u] < dd[v] || (dd[u] == dd[v] && dy[u] <= dy[v])) break;
          ord[q] = u; ord[q - 1] = v;
        }
      for (int p = 0; p < n; ++p) col[p] = tcol[ord[p]];      // canonical order from here to the residual
      double g[MFX_GK * MFX_GK], yy[MFX_GK];
      for (int p = 0; p < n; ++p) {
        yy[p] = a.Aty[col[p]];
        for (int r = 0; r < n; ++r) g[p * n + r] = G[(long)col[p] * N + col[r]];
      }
      double best = 0.0;
      for (int mask = 1; mask < (1 << n); ++mask) {
        int idx[MFX_GK], c = 0;
        for (int k = 0; k < n; ++k)
          if (mask & (1 << k)) idx[c++] = k;
        double Am[MFX_GK][MFX_GK + 1];
        for (int p = 0; p < c; ++p) {
          for (int q = 0; q < c; ++q) Am[p][q] = g[idx[p] * n + idx[q]];
          Am[p][MFX_GK] = yy[idx[p]];
        }
        bool ok = true;
        for (int p = 0; p < c && ok; ++p) {
          if (!(Am[p][p] > 1e-13 * g[idx[p] * n + idx[p]])) { ok = false; break; }
          for (int r = p + 1; r < c; ++r) {
            const double f = Am[r][p] / Am[p][p];
            for (int q = p; q < c; ++q) Am[r][q] -= f * Am[p][q];
            Am[r][MFX_GK] -= f * Am[p][MFX_GK];
          }
        }
        if (!ok) continue;
        double ws[MFX_GK], sc = 0.0;
        for (int p = c - 1; p >= 0; --p) {
          double tt = Am[p][MFX_GK];
          for (int q = p + 1; q < c; ++q) tt -= Am[p][q] * ws[q];
          ws[p] = tt / Am[p][p];
        }
        for (int p = 0; p < c; ++p) { if (!(ws[p] >= 0.0)) ok = false; sc += ws[p] * yy[idx[p]]; }
        if (ok && sc > best) {
          best = sc;
          for (int k = 0; k < n; ++k) w[k] = 0.0;
          for (int p = 0; p < c; ++p) w[idx[p]] = ws[p];
        }
      }
      double rr = 0.0;
      for (int k = 0; k < M; ++k) {
        double tt = -a.y[k];
        for (int p = 0; p < n; ++p) tt += w[p] * a.A[k * a.lda + col[p]];
        rr += tt * tt;
      }
      res = rr;
      double wt[MFX_GK];
      for (int p = 0; p < n; ++p) wt[p] = w[p];
      for (int p = 0; p < n; ++p) w[ord[p]] = wt[p];          // back to tuple order
    }
    const long key = mfx_order_key(a, t);
    if (res < bres || (res == bres && key < bkey)) {
      bres = res; bkey = key; btt = t;
      for (int k = 0; k < MFX_GK; ++k) bw[k] = w[k];
    }
  }
  s_res[tid] = bres;
  s_key[tid] = bkey;
  s_tt[tid] = btt;
  for (int k = 0; k < MFX_GK; ++k) s_w[tid][k] = bw[k];
  __syncthreads();
  if (tid == 0) {
    // initial state of the reference: min_obj = ||y||^2, w = 0, every index 0; strict '<'
    double br = y_sq;
    long bk = -1, bt = -1;
    int bi = -1;
    for (int i = 0; i < 256; ++i) {
      if (s_key[i] < 0) continue;
      if (s_res[i] < br || (s_res[i] == br && bk >= 0 && s_key[i] < bk)) { br = s_res[i]; bk = s_key[i]; bt = s_tt[i]; bi = i; }
    }
    int col[MFX_GK];
    mfx_decode(a, bt < 0 ? 0 : bt, col);
    for (int k = 0; k < n; ++k) {
      a.w[k] = (bi >= 0) ? s_w[bi][k] : 0.0;
      a.sub[k] = col[k] - a.start[k];
    }
    a.minobj[0] = br;
    s_tt[0] = bt < 0 ? 0 : bt;
    s_key[0] = bi;
  }
  __syncthreads();
  if (a.yrec) {  // y_recons = A[:, tot] @ w   (w * column for one sub-dictionary, mf_utils.py:277); the batched solver may leave it out
    int col[MFX_GK];
    mfx_decode(a, s_tt[0], col);
    for (int k = tid; k < M; k += 256) {
      double t = 0.0;
      if (n == 1) t = a.w[0] * a.A[k * a.lda + col[0]];
      else
        for (int p = 0; p < n; ++p) t += a.A[k * a.lda + col[p]] * a.w[p];
      a.yrec[k] = t;
    }
  }
}

// The kernels of the one-problem launch sequence.  The bodies above are __device__ functions so that the batched solver
// (solve_batch.hip, which defines MFX_SOLVE_BODIES_ONLY and has kernels of its own) runs them per signal on a view.
#ifndef MFX_SOLVE_BODIES_ONLY
__global__ __launch_bounds__(256) void mfx_tuple_scan(SolveArgs a) { mfx_tuple_scan_body(a); }
__global__ __launch_bounds__(256) void mfx_tuple_collect(SolveArgs a) { mfx_tuple_collect_body(a); }
__global__ __launch_bounds__(256) void mfx_tuple_overflow(SolveArgs a) { mfx_tuple_overflow_body(a); }
__global__ __launch_bounds__(256) void mfx_tuple_finalize(SolveArgs a) { mfx_tuple_finalize_body(a); }
#endif


// ---- params packing for the voxel loop's generic classes (mf.py:420-450) from the solver's outputs: one 64-thread workgroup
struct PackArgs {
  const int* run_if;   // null, or a device flag: the kernel exits at once while it is 0
  const double* w; const long* sub; const double* minobj; const double* yrec; const double* y;
  int M, K, has_csf, E, maxfasc, csf_on, ear_on, num_params;
  double* out;   // the voxel's params row
};
// (one wave: the 64 lanes of the calling wave)
__device__ __forceinline__ void mfx_pack_params_body(const PackArgs& a) {
  const int lane = threadIdx.x & 63, M = a.M;
  const int Kp = a.K + a.has_csf + (a.E > 0);
  double sy = 0.0, sr = 0.0;
  for (int m = lane; m < M; m += 64) { sy += a.y[m]; sr += a.yrec[m]; }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { sy += __shfl_xor(sy, o); sr += __shfl_xor(sr, o); }
  sy /= M; sr /= M;
  double cyy = 0.0, crr = 0.0, cyr = 0.0;
  for (int m = lane; m < M; m += 64) {
    const double da = a.y[m] - sy, db = a.yrec[m] - sr;
    cyy += da * da; crr += db * db; cyr += da * db;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { cyy += __shfl_xor(cyy, o); crr += __shfl_xor(crr, o); cyr += __shfl_xor(cyr, o); }
  double r2 = 0.0;
  if (M > 1 && cyy > 0.0 && crr > 0.0) {
    const double f = (double)(M - 1);
    double r = (cyr / f) / sqrt(cyy / f) / sqrt(crr / f);
    r = r > 1.0 ? 1.0 : (r < -1.0 ? -1.0 : r);
    r2 = r * r;
  }
  if (lane == 0) {
    double M0 = 0.0;
    for (int k = 0; k < Kp; ++k) M0 += a.w[k];
    for (int k = 0; k < a.K; ++k) {
      a.out[1 + k] = (fabs(M0) > 0) ? a.w[k] / M0 : a.w[k];
      a.out[1 + a.maxfasc + k] = (double)a.sub[k];
    }
    a.out[0] = M0;
    const int i_csf = 2 * a.maxfasc + 1, i_ear = 2 * a.maxfasc + a.csf_on + 1;
    if (a.has_csf) a.out[i_csf] = (fabs(M0) > 0) ? a.w[a.K] / M0 : a.w[a.K];
    if (a.E > 0) {
      a.out[i_ear] = (fabs(M0) > 0) ? a.w[a.K + a.has_csf] / M0 : a.w[a.K + a.has_csf];
      a.out[i_ear + 1] = (double)a.sub[a.K + a.has_csf];
    }
    a.out[a.num_params - 2] = a.minobj[0] / M;
    a.out[a.num_params - 1] = r2;
  }
}
#ifndef MFX_SOLVE_BODIES_ONLY
__global__ __launch_bounds__(64) void mfx_pack_params_kernel(PackArgs a) {
  if (a.run_if && !*a.run_if) return;
  mfx_pack_params_body(a);
}
#endif
