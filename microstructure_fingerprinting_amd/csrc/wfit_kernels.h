// wfit_kernels.h -- the fused kernels of the weighted fit (include/mfx_wfit.h; fit_w.hip's header comment describes
// their phases), their argument block, the staging of a voxel's scaling and knot descriptors, the weighted R2 and the
// LDS sizes.  Included by fit_w.hip (the weighted fit) and by wboot.hip (the replicate weighted fit of
// include/mfx_wboot.h), as fit2d_kernels.h serves fit2d.hip and boot2d.hip.
//
// The two-fascicle kernel has three instantiations that share every line of arithmetic:
//   W_PLAIN  one workgroup per voxel, all phases: the weighted fit.
//   W_GRAM   one workgroup per voxel, phases 0 and 2 without the scan: the 16 accumulator tiles of every (row block,
//            column block) go to scratch G as they stand, element r of tile (ti, tj) of thread tid at
//            G[vox][((blk 16 + ti 4 + tj) 4 + r) 256 + tid] (coalesced; blk = rb nblk + cb).
//   W_REP    one workgroup per (voxel, replicate): the signal is row vox B + b of Y, weights, directions and status
//            are the voxel's.  Phases 0, 1 and 3 run as in W_PLAIN; phase 2 reads its accumulator tiles from G instead
//            of forming them, so the scan sees the bits W_PLAIN's MFMAs leave, and the row is W_PLAIN's row.
#pragma once
#include "mfx_host.h"
#include "fit_small.hip"   // mfx_np_sumsq

namespace {

constexpr int W_PLAIN = 0, W_GRAM = 1, W_REP = 2;
constexpr int W_WG = 256;               // 4 waves, one per SIMD and workgroup
constexpr int W_NW = 4;
constexpr int W_BLK = 128;               // atoms per side of a workgroup's Gram block (2 x 2 waves of 64 x 64)
constexpr int W_MC = 8;                  // protocol rows per chunk (2 k-steps)
constexpr int W_TS = W_MC * 16 + 16;     // doubles per LDS tile: 16 atoms x W_MC rows, padded
constexpr int W_NT = 2 * W_BLK / 16;     // tiles per buffer: 8 of D_0, 8 of D_1
constexpr int W_MAXC = 256;              // short-list entries
constexpr size_t W_LDS_MAX = 160 * 1024;
constexpr int W_K1_WG = 256;
constexpr int W_MAX_ROWS = 4096;         // y_rec scratch of the K = 2 kernel lives in its idle operand tiles


struct WArgs {
  TablesDev T;
  PlanDev P;
  const double* Y;       // [V x M]
  const double* W;       // [V x M] or [M]
  int64_t wstride;       // M or 0
  const double* peaks;   // [V x peaks_ld]
  int peaks_ld;
  const int* vstat;      // [V]
  double* params;        // [V x num_params]
  int num_params, maxfasc;
  double* G;             // W_GRAM, W_REP: accumulator tiles of the voxels' Grams, G_ld doubles a voxel
  size_t G_ld;
  int B;                 // W_REP: replicates per voxel (Y and params have V B rows)
};

// the voxel's scaling, scaled signal and knot descriptors in LDS: MP = M padded to the chunk, K directions
struct WDesc {
  double *s, *y, *t0, *t1, *tG, *dG;
  int *r0, *r1;
  int MP;
};
__host__ __device__ inline size_t w_desc_doubles(int K, int MP, bool br) {
  return (size_t)2 * MP + (size_t)K * MP + (br ? (size_t)K * MP + 2 * (size_t)MP : 0) + ((size_t)K * MP * (br ? 2 : 1)) / 2;
}
template <bool BR>
__device__ __forceinline__ double* w_desc_carve(double* p, int K, int MP, WDesc& d) {
  d.MP = MP;
  d.s = p; p += MP;
  d.y = p; p += MP;
  d.t0 = p; p += K * MP;
  d.t1 = p; d.tG = p; d.dG = p;
  if (BR) { p += K * MP; d.tG = p; p += MP; d.dG = p; p += MP; }
  d.r0 = (int*)p;
  d.r1 = d.r0 + (BR ? K * MP : 0);
  return p + (K * MP * (BR ? 2 : 1)) / 2;   // MP is a multiple of 8
}
// phase 0 (the caller puts a barrier behind it)
template <bool BR>
__device__ __forceinline__ void w_stage(const WArgs& a, const WDesc& d, int K, size_t yrow, size_t vox, int tid, int nthr) {
  const int M = a.P.M, MP = d.MP;
  const double* __restrict__ yv = a.Y + yrow * M;   // the signal's row (a replicate's), weights and directions of the voxel
  const double* __restrict__ wv = a.W + vox * a.wstride;
  const double* __restrict__ pk = a.peaks + vox * a.peaks_ld;
  for (int m = tid; m < MP; m += nthr) {
    const double s = (m < M) ? sqrt(wv[m]) : 0.0;
    d.s[m] = s;
    d.y[m] = (m < M) ? s * yv[m] : 0.0;
    if (BR) { d.tG[m] = (m < M) ? a.P.tG[m] : 0.0; d.dG[m] = (m < M) ? a.P.dG[m] : 1.0; }
  }
  for (int idx = tid; idx < K * MP; idx += nthr) {
    const int k = idx / MP, m = idx - k * MP;
    RowDesc rd;
    rd.r0 = a.T.P; rd.t0 = 0.0; rd.r1 = -1; rd.t1 = 0.0;   // padded rows -> the all-zero table row
    if (m < M) rd = mfx_row_desc(a.T, a.P, m, pk[3 * k], pk[3 * k + 1], pk[3 * k + 2]);
    d.r0[idx] = rd.r0;
    d.t0[idx] = rd.t0;
    if (BR) { d.r1[idx] = rd.r1; d.t1[idx] = rd.t1; }
  }
  if (tid < K) mfx_check_dir(a.P, pk + 3 * tid, (int)vox);
}
// the unscaled entry (direction k, row m, atom n): the expression of mfx_rotate
template <bool BR>
__device__ __forceinline__ double w_elem(const WArgs& a, const WDesc& d, int k, int m, int n) {
  const int q = k * d.MP + m;
  if (BR) {
    RowDesc rd;
    rd.r0 = d.r0[q]; rd.t0 = d.t0[q]; rd.r1 = d.r1[q]; rd.t1 = d.t1[q];
    return mfx_eval_br(a.T.tab, a.T.ldn, rd, d.tG[m], d.dG[m], n);
  }
  return mfx_eval(a.T.tab, a.T.ldn, d.r0[q], d.t0[q], n);
}

// status of every voxel from its weights; NaN row for an unusable voxel, ok[v] = 0
__global__ void wfit_status_kernel(const double* __restrict__ W, int64_t wstride, int M, int64_t V, int* __restrict__ vstat,
                                   int* __restrict__ ok, double* __restrict__ params, int np) {
  const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= V) return;
  const double* wv = W + v * wstride;
  bool bad = false, pos = false;
  for (int m = 0; m < M; ++m) {
    const double w = wv[m];
    bad |= !(w >= 0.0) || !(w <= 1.79769313486231570815e308);
    pos |= w > 0.0;
  }
  const int code = bad ? 1 : (pos ? 0 : 2);
  vstat[v] = code;
  ok[v] = code == 0;
  if (code != 0)
    for (int q = 0; q < np; ++q) params[v * np + q] = __builtin_nan("");
}

// squared weighted Pearson correlation of y and y_rec by the 64 lanes of one wave (weights wv, weighted means);
// 0 with fewer than two positive weights or a vanishing weighted variance
__device__ __forceinline__ double w_r2(const double* __restrict__ yv, const double* __restrict__ wv, const double* yrec, int M,
                                       int lane) {
  double sw = 0.0, sy = 0.0, sr = 0.0, np = 0.0;
  for (int m = lane; m < M; m += 64) {
    const double w = wv[m];
    sw += w;
    sy += w * yv[m];
    sr += w * yrec[m];
    np += (w > 0.0) ? 1.0 : 0.0;
  }
  sw = wave_sum(sw);
  sy = wave_sum(sy) / sw;
  sr = wave_sum(sr) / sw;
  np = wave_sum(np);
  double cyy = 0.0, crr = 0.0, cyr = 0.0;
  for (int m = lane; m < M; m += 64) {
    const double w = wv[m], da = yv[m] - sy, db = yrec[m] - sr;
    cyy += w * (da * da);
    crr += w * (db * db);
    cyr += w * (da * db);
  }
  cyy = wave_sum(cyy) / sw;
  crr = wave_sum(crr) / sw;
  cyr = wave_sum(cyr) / sw;
  double r2 = 0.0;
  if (np > 1.5 && cyy > 0.0 && crr > 0.0) {
    double r = cyr / sqrt(cyy) / sqrt(crr);
    r = r > 1.0 ? 1.0 : (r < -1.0 ? -1.0 : r);
    r2 = r * r;
  }
  return r2;
}
// sum of the voxel's weights by one wave
__device__ __forceinline__ double w_sumw(const double* __restrict__ wv, int M, int lane) {
  double sw = 0.0;
  for (int m = lane; m < M; m += 64) sw += wv[m];
  return wave_sum(sw);
}

size_t w_lds_bytes(int NP, int MP, bool br) {
  return ((size_t)2 * W_NT * W_TS + 4 * (size_t)NP + 32 + w_desc_doubles(2, MP, br)) * sizeof(double) + W_MAXC * sizeof(Cand) +
         4 * sizeof(int);
}

template <bool BR, int MODE>
__global__ __launch_bounds__(W_WG, 2) void mfx_wfit_k2_kernel(WArgs a) {
  extern __shared__ double smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lg = lane >> 4, lc = lane & 15;
  const int wr = wave >> 1, wc = wave & 1;
  const int M = a.P.M, N = a.T.N;
  const int NP = a.T.ldn;          // atoms padded to a multiple of 16 (padded atoms are zero columns of the table)
  const int MP = (M + W_MC - 1) & ~(W_MC - 1);
  const int ntiles = NP >> 4;
  const size_t row = blockIdx.x;   // the parameter row: the voxel, or (voxel, replicate) in W_REP
  const size_t vox = MODE == W_REP ? row / (size_t)a.B : row;
  const size_t yrow = MODE == W_GRAM ? vox * (size_t)a.B : row;   // (W_GRAM reads no signal: a row that exists)
  if (a.vstat[vox] != 0) return;   // unusable weights: wfit_status_kernel wrote the row (workgroup-uniform)

  // ---- LDS carve-up (w_lds_bytes mirrors it)
  double* sT = smem;                                    // [2][W_NT][W_TS]: tiles 0..7 the D_0 block, 8..15 the D_1 block
  double2* s_st = (double2*)(sT + 2 * W_NT * W_TS);     // [2][NP] column statistics {|a|^2, a.y'} of D_0, then of D_1
  double* s_red = (double*)(s_st + 2 * NP);             // [32] scratch
  WDesc D;
  double* p_end = w_desc_carve<BR>(s_red + 32, 2, MP, D);
  Cand* s_cand = (Cand*)p_end;                          // [W_MAXC]
  int* s_cnt = (int*)(s_cand + W_MAXC);                 // [4]

  const double* __restrict__ yv = a.Y + yrow * M;
  const double* __restrict__ wv = a.W + vox * a.wstride;

  // ---- phase 0: s, y', descriptors
  w_stage<BR>(a, D, 2, yrow, vox, tid, W_WG);
  __syncthreads();
  const double* s_s = D.s;
  const double* s_y = D.y;
  auto elem = [&](int k, int m, int n) -> double { return s_s[m] * w_elem<BR>(a, D, k, m, n); };   // the scaled entry

  // ---- phase 1: ||y'||^2 and the column statistics, sequential over the measurements (mf_utils.py:307-325)
  if constexpr (MODE != W_GRAM) {   // (the bodies under the mode switches keep the indentation they had in fit_w.hip)
  if (tid == 0) {
    s_cnt[0] = 0;
    double s = 0.0;
    for (int m = 0; m < M; ++m) s += s_y[m] * s_y[m];
    s_red[31] = s;
  }
  double my_s[2] = {0.0, 0.0};
  int my_n[2] = {0, 0};
  for (int col = tid; col < 2 * NP; col += W_WG) {
    const int k = col >= NP, n = col - k * NP;
    double a2 = 0.0, ay = 0.0;
    if (n < N) {
#pragma unroll 4
      for (int m = 0; m < M; ++m) {
        const double d = elem(k, m, n);
        a2 += d * d;
        ay += s_y[m] * d;
      }
    }
    s_st[col] = double2{a2, ay};
    const double s = (n < N && ay > 0.0) ? (ay * ay) / a2 : 0.0;
    if (s > my_s[k]) { my_s[k] = s; my_n[k] = n; }   // columns are visited in increasing n per thread
  }
  __syncthreads();
  // ||y'||^2 stays in s_red[31] and the running best lower bound on the score in s_red[30]
  {
    const double eps_abs = 1e-9 * s_red[31];
    // best single atom of each dictionary (first index on ties): they stand for every pair whose optimum has one
    // active atom (mf_utils.py:357-379); phase 3 expands the winner's family exactly (as fit_k2.hip)
    double* s_bs = s_red;            // [2][8] per-wave bests
    int* s_bn = (int*)(s_red + 16);  // [2][8]
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      double s = my_s[k];
      int n = my_n[k];
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const double s2 = __shfl_xor(s, o);
        const int n2 = __shfl_xor(n, o);
        const bool take = (s2 > s) || (s2 == s && n2 < n);
        s = take ? s2 : s;
        n = take ? n2 : n;
      }
      if (lane == 0) { s_bs[k * 8 + wave] = s; s_bn[k * 8 + wave] = n; }
    }
    __syncthreads();
    double best1 = 0.0;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      double s = s_bs[k * 8];
      int n = s_bn[k * 8];
      for (int w = 1; w < W_NW; ++w) {
        const double s2 = s_bs[k * 8 + w];
        const int n2 = s_bn[k * 8 + w];
        if (s2 > s || (s2 == s && n2 < n)) { s = s2; n = n2; }
      }
      best1 = fmax(best1, s);
      if (tid == 0 && s > 0.0) {
        const int slot = s_cnt[0]++;
        s_cand[slot].score = s + eps_abs;
        s_cand[slot].i = k ? 0 : n;
        s_cand[slot].j = k ? n : 0;
      }
    }
    __syncthreads();   // (s_red[0..23] read by everybody)
    if (tid == 0) { s_red[30] = best1; s_cnt[1] = s_cnt[0]; }   // the single-atom representatives (0..2)
  }
  __syncthreads();
  }

  // ---- phase 2: cross-Gram blocks accumulated over the rows in chunks, then the pair scan
  const int nblk = (NP + W_BLK - 1) / W_BLK;
  const int nchunks = MP / W_MC;
  // generation: thread -> one atom of one side (waves 0, 1: D_0; waves 2, 3: D_1), the W_MC rows of the chunk
  const int gk = wave >> 1;
  const int gc = tid & (W_BLK - 1);
  double* const gdst0 = sT + (gk * 8 + (gc >> 4)) * W_TS + (gc & 15);

  for (int rb = 0; rb < nblk; ++rb) {
    const int nta = min(max(ntiles - (rb * 8 + wr * 4), 0), 4);   // valid row tiles of this wave (wave-uniform)
    for (int cb = 0; cb < nblk; ++cb) {
      const int ntb = min(max(ntiles - (cb * 8 + wc * 4), 0), 4);
      const int gn = (gk ? cb : rb) * W_BLK + gc;   // this thread's atom
      const int gnc = gn < NP ? gn : NP - 1;        // (a readable column; atoms beyond the dictionary are written as zeros)
      auto gen_chunk = [&](int ch, int buf) {
        double* dst = gdst0 + (size_t)buf * (W_NT * W_TS);
#pragma unroll
        for (int r = 0; r < W_MC; ++r) {
          const double v = elem(gk, ch * W_MC + r, gnc);   // rows beyond the protocol: s = 0 on the zero table row
          dst[r * 16] = gn < N ? v : 0.0;
        }
      };
      d4 acc[4][4];
#pragma unroll
      for (int ti = 0; ti < 4; ++ti)
#pragma unroll
        for (int tj = 0; tj < 4; ++tj) acc[ti][tj] = d4{0, 0, 0, 0};

      // element r of tile (ti, tj) of this thread in the voxel's stored tiles (W_GRAM writes, W_REP reads)
      double* const gacc = MODE == W_PLAIN ? nullptr : a.G + vox * a.G_ld + (size_t)(rb * nblk + cb) * (16 * 4 * W_WG) + tid;
      if constexpr (MODE == W_REP) {
#pragma unroll
        for (int ti = 0; ti < 4; ++ti)
#pragma unroll
          for (int tj = 0; tj < 4; ++tj)
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[ti][tj][r] = gacc[((ti * 4 + tj) * 4 + r) * W_WG];
      } else {
      gen_chunk(0, 0);
      __syncthreads();
      for (int ch = 0; ch < nchunks; ++ch) {
        const int buf = ch & 1;
        if (ch + 1 < nchunks) gen_chunk(ch + 1, buf ^ 1);
        if (nta > 0 && ntb > 0) {
          const double* tA = sT + (size_t)buf * (W_NT * W_TS) + (wr * 4) * W_TS + lg * 16 + lc;
          const double* tB = sT + (size_t)buf * (W_NT * W_TS) + (8 + wc * 4) * W_TS + lg * 16 + lc;
#pragma unroll
          for (int kk = 0; kk < W_MC / 4; ++kk) {
            double av[4], bv[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) { av[t] = tA[t * W_TS + kk * 64]; bv[t] = tB[t * W_TS + kk * 64]; }
#pragma unroll
            for (int ti = 0; ti < 4; ++ti)
#pragma unroll
              for (int tj = 0; tj < 4; ++tj)
                acc[ti][tj] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[ti], bv[tj], acc[ti][tj], 0, 0, 0);
          }
        }
        __syncthreads();
      }
      }
      if constexpr (MODE == W_GRAM) {
#pragma unroll
        for (int ti = 0; ti < 4; ++ti)
#pragma unroll
          for (int tj = 0; tj < 4; ++tj)
#pragma unroll
            for (int r = 0; r < 4; ++r) gacc[((ti * 4 + tj) * 4 + r) * W_WG] = acc[ti][tj][r];
        continue;
      }

      // pair scan of the accumulator tiles, fit_k2.hip's un-normalised scan (mf_utils.py:348-356 ranked here; the
      // single-active cases are the two single-atom representatives).  A slot is one row of the lane over this block's
      // columns of the lane; pass 0: the slots' lower bounds (and the ill-conditioned pairs); pass 1: the list
      double llb = 0.0;
      const double eps_abs = 1e-9 * s_red[31];
      // an MFMA-summed cross term against the serial sum: at most M eps |a1||a2| whatever the order; 4 x that, not below fit_k2's
      const double a12_rel = fmax(MFX_A12_REL, 4.0 * M * 2.220446049250313e-16);
      double glb_run = s_red[30];
#pragma unroll 1
      for (int pass = 0; pass < 2; ++pass) {
        mfx_static_for<0, 4>([&](auto tic) {
          constexpr int ti = decltype(tic)::value;
          if (ti < nta) {
#pragma unroll 1
            for (int r = 0; r < 4; ++r) {
              const int i = rb * W_BLK + wr * 64 + ti * 16 + lg + 4 * r;
              const double A11 = s_st[i].x, Y1 = s_st[i].y;
              double p = 0.0, q = 1.0;
              int bj = -1;
#pragma unroll 1
              for (int tj = 0; tj < ntb; ++tj) {
                const int j = cb * W_BLK + wc * 64 + tj * 16 + lc;
                const double A22 = s_st[NP + j].x, Y2 = s_st[NP + j].y;
                auto row = [&](const d4& v) { return r == 0 ? v[0] : (r == 1 ? v[1] : (r == 2 ? v[2] : v[3])); };
                const double A12 = tj == 0 ? row(acc[ti][0]) : (tj == 1 ? row(acc[ti][1]) : (tj == 2 ? row(acc[ti][2]) : row(acc[ti][3])));
                const double d1 = fma(-A12, Y2, A22 * Y1);
                const double d2 = fma(-A12, Y1, A11 * Y2);
                const double pd = A11 * A22;
                const double Det = fma(-A12, A12, pd);
                const double num = fma(Y2, d2, Y1 * d1);
                const bool pos = (d1 > 0.0) & (d2 > 0.0) & (j < N) & (i < N);
                const bool wellc = Det > MFX_DET_REL * pd;
                // nearly collinear pairs cannot be ranked as a fraction; with two positive weights they go to the exact
                // stage unranked, never as single atoms (rare: a branch)
                if (pass == 0 && pos && !wellc) {
                  const int slot = atomicAdd(&s_cnt[0], 1);
                  if (slot < W_MAXC) { s_cand[slot].score = 1e300; s_cand[slot].i = i; s_cand[slot].j = j; }
                }
                const bool both = pos & wellc;
                const double pn = both ? num : 0.0;
                const double qn = both ? Det : 1.0;
                const bool better = pn * q > p * qn;
                p = better ? pn : p;
                q = better ? qn : q;
                bj = better ? j : bj;
              }
              if (bj >= 0) {
                const double sc = p / q;
                const double er = sc * (a12_rel * (A11 * s_st[NP + bj].x) / q);
                if (pass == 0) {
                  llb = fmax(llb, sc - er);
                } else if (sc > 0.0 && sc + er + eps_abs >= glb_run) {
                  const int slot = atomicAdd(&s_cnt[0], 1);
                  if (slot < W_MAXC) { s_cand[slot].score = sc + er + eps_abs; s_cand[slot].i = i; s_cand[slot].j = bj; }   // upper bound
                }
              }
            }
          }
        });
        if (pass == 0) {
          llb = wave_max(llb);
          if (lane == 0) s_red[wave] = llb;
          __syncthreads();
          double rlb = s_red[0];
#pragma unroll
          for (int w = 1; w < W_NW; ++w) rlb = fmax(rlb, s_red[w]);
          glb_run = fmax(glb_run, rlb);
        }
      }
      __syncthreads();
      if (tid == 0) s_red[30] = glb_run;   // (read again behind the next block's barriers)
    }
  }

  if constexpr (MODE == W_GRAM) return;
  // ---- phase 3: exact re-evaluation of the short list (reference arithmetic and order) on the scaled entries
  __syncthreads();
  const double y_sq = s_red[31], glb_run = s_red[30];
  auto exact_pair = [&](int i, int j, double& w0, double& w1, double& res) {
    double a11 = 0.0, a22 = 0.0, a12 = 0.0, y1 = 0.0, y2 = 0.0;
#pragma unroll 4
    for (int m = 0; m < M; ++m) {
      const double d1 = elem(0, m, i), d2 = elem(1, m, j), ym = s_y[m];
      a11 += d1 * d1;
      a22 += d2 * d2;
      a12 += d1 * d2;
      y1 += ym * d1;
      y2 += ym * d2;
    }
    nnls2_exact(y_sq, a11, a12, a22, y1, y2, w0, w1, res);
  };
  // lexicographic (res, idx) minimum over the workgroup; idx = i N + j is the reference's scan order
  double* s_rres = sT;                   // [8] per-wave partials (the operand buffers are idle now)
  long* s_ridx = (long*)(s_rres + 8);    // [8]
  double* s_rw = (double*)(s_ridx + 8);  // [8][2]
  double* s_win = s_rw + 16;             // winner: res, w0, w1, (long) idx
  auto block_argmin = [&](double res, long idx, double w0, double w1) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const double r2 = __shfl_xor(res, o), u0 = __shfl_xor(w0, o), u1 = __shfl_xor(w1, o);
      const long i2 = __shfl_xor(idx, o);
      const bool take = (r2 < res) || (r2 == res && i2 < idx);
      res = take ? r2 : res; idx = take ? i2 : idx; w0 = take ? u0 : w0; w1 = take ? u1 : w1;
    }
    __syncthreads();
    if (lane == 0) { s_rres[wave] = res; s_ridx[wave] = idx; s_rw[2 * wave] = w0; s_rw[2 * wave + 1] = w1; }
    __syncthreads();
    if (tid == 0) {
      // fold into the current winner (strict '<' on res, ties -> earlier pair in scan order)
      double br = s_win[0], b0 = s_win[1], b1 = s_win[2];
      long bi = ((long*)s_win)[3];
      for (int w = 0; w < W_NW; ++w) {
        const double r = s_rres[w];
        const long ix = s_ridx[w];
        if (ix < 0) continue;
        if (r < br || (r == br && bi >= 0 && ix < bi)) { br = r; bi = ix; b0 = s_rw[2 * w]; b1 = s_rw[2 * w + 1]; }
      }
      s_win[0] = br; s_win[1] = b0; s_win[2] = b1; ((long*)s_win)[3] = bi;
    }
    __syncthreads();
  };
  const int nappend = s_cnt[0];
  const int ncand = nappend > W_MAXC ? W_MAXC : nappend;
  __syncthreads();   // everyone has read s_cnt / is done with the operand buffers
  if (tid == 0) {    // mf_utils.py:327, 382: start from min_obj = y_sq at pair (0,0) with w = 0, strict '<'
    s_win[0] = y_sq; s_win[1] = 0.0; s_win[2] = 0.0; ((long*)s_win)[3] = -1;
  }
  {
    double res = INFINITY, w0 = 0.0, w1 = 0.0;
    long idx = -1;
    if (nappend <= W_MAXC) {
      // A scan candidate is the best pair of its slot - row i, the columns j = lc (mod 16) of one wave's half of one
      // column block; the whole row i over the columns j = lc (mod 16) (a superset of the slot) is evaluated exactly
      // for every listed candidate that still reaches the final lower bound.  The first entries are the single-atom
      // representatives of phase 1: themselves only.
      const int NJ = (N + 15) >> 4, nsingle = s_cnt[1];
      for (int q = tid; q < ncand * NJ; q += W_WG) {
        const int c = q / NJ, u = q - c * NJ;
        if (!(s_cand[c].score >= glb_run)) continue;
        const int ci = s_cand[c].i, cj = s_cand[c].j;
        const int jj = (c < nsingle) ? cj : (cj & 15) + 16 * u;
        if ((c < nsingle && u > 0) || jj >= N) continue;
        double r, u0, u1;
        exact_pair(ci, jj, u0, u1, r);
        const long ix = (long)ci * N + jj;
        if (r < res || (r == res && ix < idx)) { res = r; idx = ix; w0 = u0; w1 = u1; }
      }
    } else {
      // the short list overflowed (massive near-ties): last resort, every pair through the reference arithmetic
      const long npairs = (long)N * N;
      for (long pr = tid; pr < npairs; pr += W_WG) {
        double r, u0, u1;
        exact_pair((int)(pr / N), (int)(pr % N), u0, u1, r);
        if (r < res || (r == res && pr < idx)) { res = r; idx = pr; w0 = u0; w1 = u1; }
      }
    }
    block_argmin(res, idx, w0, w1);
  }
  // near-zero second weight: every pair sharing the active atom fits equally well up to rounding; the reference returns
  // the first pair of that row / column attaining the minimum of its own rounded residual: the whole family exactly
  for (int pass = 0; pass < 2; ++pass) {
    const double bw0 = s_win[1], bw1 = s_win[2];
    const long bidx = ((long*)s_win)[3];
    if (bidx < 0) break;
    const int bi = (int)(bidx / N), bj2 = (int)(bidx - (long)bi * N);
    const bool row_family = (pass == 0) && (bw1 <= 1e-7 * bw0);
    const bool col_family = (pass == 1) && (bw0 <= 1e-7 * bw1);
    if (!row_family && !col_family) continue;
    double res = INFINITY, w0 = 0.0, w1 = 0.0;
    long idx = -1;
    for (int n = tid; n < N; n += W_WG) {
      double r, u0, u1;
      const int i = row_family ? bi : n, j = row_family ? n : bj2;
      exact_pair(i, j, u0, u1, r);
      const long ix = (long)i * N + j;
      if (r < res || (r == res && ix < idx)) { res = r; idx = ix; w0 = u0; w1 = u1; }
    }
    block_argmin(res, idx, w0, w1);
  }
  if (wave == 0) {
    const double best = s_win[0], w0 = s_win[1], w1 = s_win[2];
    const long bidx = ((long*)s_win)[3];
    const int bi = bidx < 0 ? 0 : (int)(bidx / N);
    const int bjx = bidx < 0 ? 0 : (int)(bidx - (long)bi * N);
    // params packing, mf.py:420-450, with the weighted MSE and R2
    const double M0 = w0 + w1;
    const double nu0 = (fabs(M0) > 0) ? w0 / M0 : w0;
    const double nu1 = (fabs(M0) > 0) ? w1 / M0 : w1;
    // y_rec = D[:, tot] @ w on the unscaled columns
    double* s_yrec = s_win + 8;   // [M] scratch inside the idle operand buffers
    for (int m = lane; m < M; m += 64) s_yrec[m] = w_elem<BR>(a, D, 0, m, bi) * w0 + w_elem<BR>(a, D, 1, m, bjx) * w1;
    const double r2 = w_r2(yv, wv, s_yrec, M, lane);
    const double sw = w_sumw(wv, M, lane);
    double* out = a.params + row * a.num_params;
    if (lane == 0) {
      out[0] = M0;
      out[1] = nu0;
      out[2] = nu1;
      out[1 + a.maxfasc] = (double)bi;
      out[2 + a.maxfasc] = (double)bjx;
      out[a.num_params - 2] = best / sw;
      out[a.num_params - 1] = r2;
    }
  }
}
static_assert(2 * W_NT * W_TS >= W_MAX_ROWS + 48, "y_rec scratch of the K = 2 kernel");

size_t w_k1_lds_bytes(int M, int MP, bool br) {
  return (2 * (size_t)W_K1_WG + 8 + (size_t)M + w_desc_doubles(1, MP, br)) * sizeof(double);
}

// K = 1, no extra column: one workgroup per voxel, one thread per atom; solve_exhaustive_posweights_1 (mf_utils.py:225-286)
template <bool BR>
__global__ __launch_bounds__(W_K1_WG) void mfx_wfit_k1_kernel(WArgs a) {
  extern __shared__ double smem[];
  const int tid = threadIdx.x;
  const int M = a.P.M, N = a.T.N;
  const int MP = (M + W_MC - 1) & ~(W_MC - 1);
  const size_t vox = blockIdx.x;
  if (a.vstat[vox] != 0) return;
  double* s_res = smem;                         // [WG]
  long* s_key = (long*)(s_res + W_K1_WG);       // [WG]
  double* s_misc = (double*)(s_key + W_K1_WG);  // [8]
  double* s_yrec = s_misc + 8;                  // [M]
  WDesc D;
  w_desc_carve<BR>(s_yrec + M, 1, MP, D);
  const double* __restrict__ yv = a.Y + vox * M;
  const double* __restrict__ wv = a.W + vox * a.wstride;
  w_stage<BR>(a, D, 1, vox, vox, tid, W_K1_WG);
  __syncthreads();
  const double* s_s = D.s;
  const double* s_y = D.y;
  if (tid == 0) s_misc[0] = mfx_np_sumsq(s_y, M);   // _1 uses np.sum(y**2)
  __syncthreads();
  const double y_sq = s_misc[0];
  // thread-local best in the reference's scan order; key < 0 = the reference's initial state
  double bres = y_sq, bw = 0.0;
  long bkey = -1;
  for (int i = tid; i < N; i += W_K1_WG) {
    double a11 = 0.0, Y1 = 0.0;
#pragma unroll 4
    for (int m = 0; m < M; ++m) {
      const double d = s_s[m] * w_elem<BR>(a, D, 0, m, i);
      a11 += d * d;
      Y1 += s_y[m] * d;
    }
    double w, r;
    nnls1_exact(y_sq, a11, Y1, w, r);
    if (r < bres || (r == bres && bkey >= 0 && i < bkey)) { bres = r; bkey = i; bw = w; }
  }
  s_res[tid] = bres;
  s_key[tid] = bkey;
  __syncthreads();
  for (int o = W_K1_WG / 2; o > 0; o >>= 1) {
    if (tid < o) {
      const double r1 = s_res[tid], r2 = s_res[tid + o];
      const long k1 = s_key[tid], k2 = s_key[tid + o];
      if (r2 < r1 || (r2 == r1 && k1 >= 0 && k2 < k1)) { s_res[tid] = r2; s_key[tid] = k2; }
    }
    __syncthreads();
  }
  if (bres == s_res[0] && bkey == s_key[0]) { s_misc[2] = bres; s_misc[3] = bw; ((long*)s_misc)[4] = bkey; }
  __syncthreads();
  const double res = s_misc[2], w = s_misc[3];
  const long key = ((long*)s_misc)[4];
  const int ia = key < 0 ? 0 : (int)key;
  if (tid < 64) {
    const int lane = tid;
    for (int m = lane; m < M; m += 64) s_yrec[m] = w * w_elem<BR>(a, D, 0, m, ia);
    const double r2 = w_r2(yv, wv, s_yrec, M, lane);
    const double sw = w_sumw(wv, M, lane);
    if (lane == 0) {   // params packing, mf.py:420-450
      double* out = a.params + vox * a.num_params;
      out[0] = w;
      out[1] = (fabs(w) > 0) ? w / w : w;
      out[1 + a.maxfasc] = (double)ia;
      out[a.num_params - 2] = res / sw;
      out[a.num_params - 1] = r2;
    }
  }
}

int w_max_atoms_k2(int M, bool br) {
  if (M > W_MAX_ROWS) return 0;
  const int MP = (M + W_MC - 1) & ~(W_MC - 1);
  int n = 0;
  while (n < (1 << 20) && w_lds_bytes(n + 16, MP, br) <= W_LDS_MAX) n += 16;
  return n;
}

// doubles of scratch G per voxel for dictionaries padded to NP atoms: every 128 x 128 block's tiles in full
inline size_t w_gram_doubles(int NP) {
  const size_t nblk = ((size_t)NP + W_BLK - 1) / W_BLK;
  return nblk * nblk * (16 * 4 * W_WG);
}

}  // namespace
