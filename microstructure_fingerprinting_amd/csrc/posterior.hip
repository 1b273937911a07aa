// posterior.hip -- soft fits (include/mfx_post.h): per atom of each fascicle the sum over every partner atom of
// exp(-(F - shift) / T), normalised per voxel, and the log of the whole sum.
//
// mfx_post_k2_kernel   one workgroup per voxel; phases 0-2 are those of mfx_profile_k2_kernel (profile.hip), restated
//                      here: knot descriptors and y in LDS, column statistics of both rotated dictionaries (one thread
//                      per atom), the cross-Gram D_0^T D_1 on v_mfma_f64_16x16x4_f64 with the wave's 16 atoms of D_0 in
//                      registers and D_1 generated chunk by chunk into LDS.  The scoring helpers, the cut, the weights'
//                      status and the host plumbing are soft_sweep.h's, shared with profile.hip (F is the profile's value
//                      by definition).  The scan keeps a sum of exponentials per row and per column where the profile
//                      keeps a minimum:
//                        per pair  the score ||y||^2 - F (p / q, or the CSF value), t = exp((score - (||y||^2 - shift)) / T):
//                                  one division and one FP64 exp per pair.  FP64 MFMA and VALU instructions do not
//                                  overlap on a SIMD, so the scan adds to the matrix work: about 2 900 cycles of
//                                  VALU beside 6 400 of MFMA per wave and pair of tiles.
//                        rows      4 running sums per lane and sweep (C/D layout: col = lane & 15, row = (lane >> 4) +
//                                  4 reg), folded over the 16 lanes of a row once per sweep, one lane stores;
//                        columns   added in the lane over its 4 rows, over the 4 lane groups by two shuffles, then one
//                                  entry per wave and column in a two-half LDS slab; the chunk's first CW threads add
//                                  the waves' entries in wave order into an [NP] LDS array behind the barrier that ends
//                                  the chunk anyway.
//                      No indices, no tie rules, no fraction compare, no global atomics.  Z is the index-order sum of the
//                      row sums; the division by Z and log_sum happen in the kernel's last phase.
// mfx_post_k1_kernel   one workgroup per voxel, one thread per atom (mfx_profile_k1_kernel's scoring).
//
// The status codes come from the kernels themselves: T and shift are checked in phase 0 (code 1, workgroup-uniform
// exit), then the weights (codes 3 and 4), an exponent above 700 raises an LDS flag and Z is tested in the last phase
// (code 2).
#include "soft_sweep.h"
#include "../../include/mfx_post.h"
#include "../../include/mfx_wsoft.h"

namespace {

constexpr double POST_EXP_MAX = 700.0;   // exponents above this make the shift unusable (status 2)

struct PostArgs : SweepArgs {
  const double* temp;   // [V]
  const double* shift;  // [V]
  double* w;            // [V x K x N]
  double* log_sum;      // [V]
  int* status;          // [V]
};
// the weighted variants (include/mfx_wsoft.h) take two more arguments; the unweighted kernels keep PostArgs as it is
struct PostArgsW : PostArgs {
  const double* W;      // [V x M] (wstride = M) or [M] (wstride = 0)
  long long wstride;
};
template <bool WGT> using PostArgsT = std::conditional_t<WGT, PostArgsW, PostArgs>;

__device__ __forceinline__ bool post_finite(double x) { return fabs(x) <= 1.79769313486231570815e308; }   // false for NaN

// a voxel without a result: its rows and log_sum become NaN, its status `code` (every thread of the workgroup takes part)
__device__ __forceinline__ void post_nan_rows(const PostArgs& a, size_t vox, int K, int N, int code, int tid, int wg) {
  const double nan = __builtin_nan("");
  for (int n = tid; n < K * N; n += wg) a.w[vox * K * N + n] = nan;
  if (tid == 0) { a.log_sum[vox] = nan; a.status[vox] = code; }
}

// the K = 2 kernel's own LDS behind the common front of soft_sweep.h, for the host.  Doubles: the row sums R0 and the running column sums R1, [NP]
// each, and the waves' column sums of one chunk, [2][NW][CW]; ints: the flag (and one of padding).
constexpr int post_own_dbl(int NP, int nw, int cw) { return 2 * NP + 2 * nw * cw; }
constexpr int POST_OWN_INT = 2;

// NW waves per workgroup, TILES 16-atom column tiles per D_1 chunk, NBUF LDS buffers for the chunks: the profile's
// configurations (profile.hip).  WGT: rows scaled by s = sqrt(W) as they are generated (include/mfx_wsoft.h): one more
// [MP] array in LDS, y and x stored scaled, every generated entry multiplied by s_w[m]; all else is the same code.
template <int KSTEPS, bool BRACKET, bool CSF, int NW, int TILES, int NBUF, bool WGT = false>
__global__ __launch_bounds__(NW * 64, NW == 8 ? 2 : 1) void mfx_post_k2_kernel(PostArgsT<WGT> a) {
  constexpr int WG = NW * 64;
  constexpr int MP = KSTEPS * 4;              // padded measurement count
  constexpr int MPS = MP;                     // rows of one LDS D_1 tile
  constexpr int CW = 16 * TILES;              // atoms per chunk
  constexpr int RS = WG / CW;                 // row stride of one generating thread
  extern __shared__ double smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lg = lane >> 4, lc = lane & 15;
  const int M = a.P.M, N = a.T.N, ldn = a.T.ldn;
  const int NP = ldn;  // atoms padded to a multiple of 16 (padded atoms are zero columns)
  const int ntiles = NP >> 4;
  const double2* __restrict__ tab = a.T.tab;
  const size_t vox = blockIdx.x;

  // ---- LDS carve-up (post_lds_bytes below mirrors it)
  double* sB = smem;                              // [NBUF][TILES][MPS][16]
  double* s_y = sB + NBUF * TILES * MPS * 16;     // [MP]
  double* s_x = s_y + MP;                         // [MP] (CSF)
  double* s_w = s_x + (CSF ? MP : 0);             // [MP] sqrt(W) (WGT)
  double* s_t0 = s_w + (WGT ? MP : 0);            // [2][MP]
  double* s_t1 = s_t0 + 2 * MP;                   // [2][MP] (bracket only)
  double* s_tG = s_t1 + (BRACKET ? 2 * MP : 0);   // [MP]
  double* s_dG = s_tG + (BRACKET ? MP : 0);       // [MP]
  double* s_A11 = s_dG + (BRACKET ? MP : 0);      // [NP] each: |d|^2 and d.y of both dictionaries
  double* s_Y1 = s_A11 + NP;
  double* s_A22 = s_Y1 + NP;
  double* s_Y2 = s_A22 + NP;
  double* s_X1 = s_Y2 + NP;                       // [NP] each: d.x (CSF)
  double* s_X2 = s_X1 + (CSF ? NP : 0);
  double* s_rs = s_X2 + (CSF ? NP : 0);           // [NP] row sums R0 (written once per atom)
  double* s_cs = s_rs + NP;                       // [NP] running column sums R1
  double* s_sl = s_cs + NP;                       // [2][NW][CW] the waves' column sums of one chunk
  double* s_end = s_sl + 2 * NW * CW;
  int* s_r0 = (int*)s_end;                        // [2][MP]
  int* s_r1 = s_r0 + 2 * MP;                      // [2][MP] (bracket only)
  int* s_flag = s_r1 + (BRACKET ? 2 * MP : 0);    // [2] an exponent above POST_EXP_MAX was met

  // ---- phase 0: temperature and shift (status 1 leaves here, workgroup-uniform), y, x, descriptors
  const double* __restrict__ yv = a.Y + vox * M;
  const double* __restrict__ pk = a.peaks + vox * 6;
  const double Tv = a.temp[vox], shift = a.shift[vox];
  if (tid < 2) mfx_check_dir(a.P, pk + 3 * tid, (int)vox);
  if (!(Tv > 0.0) || !post_finite(Tv) || !post_finite(shift)) {
    post_nan_rows(a, vox, 2, N, 1, tid, WG);
    return;
  }
  if constexpr (WGT) {   // status 3 / 4 leave here, workgroup-uniform
    if (const int code = sweep_weights_status(a.W + vox * a.wstride, M)) {
      post_nan_rows(a, vox, 2, N, code, tid, WG);
      return;
    }
  }
  const double iT = 1.0 / Tv;
  for (int m = tid; m < MP; m += WG) {
    if constexpr (WGT) {
      const double s = (m < M) ? sqrt(a.W[vox * a.wstride + m]) : 0.0;
      s_w[m] = s;
      s_y[m] = (m < M) ? s * yv[m] : 0.0;
      if constexpr (CSF) s_x[m] = (m < M) ? s * a.xc[m] : 0.0;
    } else {
      s_y[m] = (m < M) ? yv[m] : 0.0;
      if constexpr (CSF) s_x[m] = (m < M) ? a.xc[m] : 0.0;
    }
  }
  for (int idx = tid; idx < 2 * MP; idx += WG) {
    const int k = idx / MP, m = idx - k * MP;
    RowDesc rd;
    rd.r0 = a.T.P; rd.t0 = 0.0; rd.r1 = -1; rd.t1 = 0.0;  // padded rows -> the all-zero table row
    if (m < M) rd = mfx_row_desc(a.T, a.P, m, pk[3 * k], pk[3 * k + 1], pk[3 * k + 2]);
    s_r0[idx] = rd.r0;
    s_t0[idx] = rd.t0;
    if (BRACKET) {
      s_r1[idx] = rd.r1;
      s_t1[idx] = rd.t1;
      if (k == 0) { s_tG[m] = (m < M) ? a.P.tG[m] : 0.0; s_dG[m] = (m < M) ? a.P.dG[m] : 1.0; }
    }
  }
  for (int n = tid; n < NP; n += WG) { s_rs[n] = 0.0; s_cs[n] = 0.0; }
  if (tid == 0) s_flag[0] = 0;
  __syncthreads();

  auto elem = [&](int k, int m, int n) -> double {
    if (BRACKET) {
      RowDesc rd;
      rd.r0 = s_r0[k * MP + m]; rd.t0 = s_t0[k * MP + m];
      rd.r1 = s_r1[k * MP + m]; rd.t1 = s_t1[k * MP + m];
      if constexpr (WGT) return s_w[m] * mfx_eval_br(tab, ldn, rd, s_tG[m], s_dG[m], n);
      else return mfx_eval_br(tab, ldn, rd, s_tG[m], s_dG[m], n);
    } else {
      if constexpr (WGT) return s_w[m] * mfx_eval(tab, ldn, s_r0[k * MP + m], s_t0[k * MP + m], n);
      else return mfx_eval(tab, ldn, s_r0[k * MP + m], s_t0[k * MP + m], n);
    }
  };

  // ---- phase 1: column statistics, sequential over the measurements; ||y||^2, x.x, x.y likewise (every thread)
  double y_sq = 0.0, xx = 0.0, xy = 0.0;
  for (int m = 0; m < M; ++m) {
    y_sq += s_y[m] * s_y[m];
    if constexpr (CSF) { xx += s_x[m] * s_x[m]; xy += s_x[m] * s_y[m]; }
  }
  for (int col = tid; col < 2 * NP; col += WG) {
    const int k = col >= NP, n = col - k * NP;
    double a2 = 0.0, ay = 0.0, ax = 0.0;
    if (n < N) {
#pragma unroll 4
      for (int m = 0; m < M; ++m) {
        const double d = elem(k, m, n);
        a2 += d * d;
        ay += s_y[m] * d;
        if constexpr (CSF) ax += s_x[m] * d;
      }
    }
    (k ? s_A22 : s_A11)[n] = a2;
    (k ? s_Y2 : s_Y1)[n] = ay;
    if constexpr (CSF) (k ? s_X2 : s_X1)[n] = ax;
  }
  const double ixx = (CSF && xx > 0.0) ? 1.0 / xx : 0.0;
  const double sx = xy * xy * ixx;   // what x alone explains: ||y||^2 - ||y'||^2
  const double c0 = y_sq - shift;    // exponent of a pair: (score - c0) / T = -(F - shift) / T

  auto gen_chunk = [&](int ch, int buf) {
    const int c = tid % CW, m0 = tid / CW;
    const int n = ch * CW + c;
    double* dst = sB + (size_t)buf * (TILES * MPS * 16) + (c >> 4) * (MPS * 16) + (c & 15);
    if (n < NP) {
      if constexpr (BRACKET) {   // not unrolled: a bracketed entry holds two table loads and six descriptors
#pragma unroll 1
        for (int m = m0; m < MP; m += RS) dst[m * 16] = elem(1, m, n);
      } else {
#pragma unroll 4
        for (int m = m0; m < MP; m += RS) dst[m * 16] = elem(1, m, n);
      }
    } else {
      for (int m = m0; m < MP; m += RS) dst[m * 16] = 0.0;
    }
  };

  const int nchunks = (ntiles + TILES - 1) / TILES;
  const int nrounds = (ntiles + NW - 1) / NW;
  // largest exponent this lane met over the pairs of two real atoms
  double emax = -POST_EXP_MAX;

  for (int round = 0; round < nrounds; ++round) {
    const int rt = round * NW + wave;
    const bool rt_valid = rt < ntiles;  // wave-uniform
    const int rtc = rt_valid ? rt : 0;
    // A operand: this wave's 16 atoms of D_0, all KSTEPS k-steps, in registers
    double afr[KSTEPS];
#pragma unroll
    for (int kk = 0; kk < KSTEPS; ++kk) {
      afr[kk] = rt_valid ? elem(0, 4 * kk + lg, rtc * 16 + lc) : 0.0;
      if (BRACKET && (kk & 3) == 3) __builtin_amdgcn_sched_barrier(0);   // keeps the loads of a long protocol from piling up in registers
    }
    __syncthreads();   // statistics complete (round 0); the previous sweep's last slab half folded before it is written again
    gen_chunk(0, 0);
    __syncthreads();

    // per-row operands of the scan (row r of the lane: atom i = 16 rt + lg + 4 r)
    double A11r[4], Y1r[4], p1r[4];   // CSF: the primed statistics
    double X1s[4], X1r[4], A11u[4], Y1u[4], i11p[4], i11u[4];   // CSF only: X1 / xx, X1, the plain statistics, inverses
    const int nrow = rt_valid ? N - (rtc * 16 + lg) : 0;   // row r of the lane is an atom iff 4 r < nrow
    double rs[4];   // running row sums of this sweep
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int i = rtc * 16 + lg + 4 * r;
      const double A = s_A11[i], Yv = s_Y1[i];
      if constexpr (CSF) {
        const double X = s_X1[i];
        A11u[r] = A; Y1u[r] = Yv; X1r[r] = X; X1s[r] = X * ixx;
        i11u[r] = A > 0.0 ? 1.0 / A : 0.0;
        sweep_primed(A, Yv, X, ixx, xy, A11r[r], Y1r[r], i11p[r]);
        p1r[r] = 0.0;
      } else {
        A11r[r] = A; Y1r[r] = Yv;
        const double yp = fmax(Yv, 0.0);
        p1r[r] = yp * yp;
      }
      rs[r] = 0.0;
    }

    for (int ch = 0; ch < nchunks; ++ch) {
      const int buf = (NBUF == 2) ? (ch & 1) : 0;
      if constexpr (NBUF == 2) {
        if (ch + 1 < nchunks) gen_chunk(ch + 1, buf ^ 1);
      } else if (ch > 0) {
        gen_chunk(ch, 0);   // single buffer: generate, barrier, consume, barrier
        __syncthreads();
      }
      double cs[TILES];   // this lane's column sums of the chunk (a wave without a row tile contributes zeros)
#pragma unroll
      for (int t = 0; t < TILES; ++t) cs[t] = 0.0;
      if (rt_valid) {
        const double* b0p = sB + (size_t)buf * (TILES * MPS * 16) + lg * 16 + lc;
        const double* b1p = b0p + (TILES == 2 ? MPS * 16 : 0);
        d4 acc0 = {0, 0, 0, 0}, acc1 = {0, 0, 0, 0};
#pragma unroll
        for (int kk = 0; kk < KSTEPS; ++kk) {
          const double b0 = b0p[kk * 64];
          acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(afr[kk], b0, acc0, 0, 0, 0);
          if constexpr (TILES == 2) {
            const double b1 = b1p[kk * 64];
            acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(afr[kk], b1, acc1, 0, 0, 0);
          }
        }
#pragma unroll
        for (int t = 0; t < TILES; ++t) {
          const d4 acc = t ? acc1 : acc0;
          const int j = ch * CW + t * 16 + lc;
          const bool colok = j < N;
          const int jq = colok ? j : 0;
          // a padded column is a null atom
          double A22 = colok ? s_A22[jq] : 0.0, Y2 = colok ? s_Y2[jq] : 0.0;
          double p2 = 0.0, X2 = 0.0, A22u = 0.0, Y2u = 0.0, i22p = 0.0, i22u = 0.0;
          if constexpr (CSF) {
            X2 = colok ? s_X2[jq] : 0.0; A22u = A22; Y2u = Y2;
            i22u = A22 > 0.0 ? 1.0 / A22 : 0.0;
            sweep_primed(A22u, Y2u, X2, ixx, xy, A22, Y2, i22p);
          } else {
            const double yp = fmax(Y2, 0.0);
            p2 = yp * yp;
          }
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            double s;
            if constexpr (CSF) {
              // x projected out: the two-variable form on the primed quantities, then the sign of w_x decides
              double w1, w2, v1, v2;
              const double A12p = fma(-X1s[r], X2, acc[r]);
              const double sp = sweep_pair_w(A11r[r], A22, A12p, Y1r[r], Y2, i11p[r], i22p, w1, w2);
              const double wxn = fma(-w2, X2, fma(-w1, X1r[r], xy));   // w_x times x.x
              const double su = sweep_pair_w(A11u[r], A22u, acc[r], Y1u[r], Y2u, i11u[r], i22u, v1, v2);
              s = (wxn >= 0.0) ? sx + sp : su;
            } else {
              double p, q;
              sweep_pair_frac(A11r[r], A22, acc[r], Y1r[r], Y2, p1r[r], p2, p, q);
              s = q > 0.0 ? p / q : 0.0;
            }
            const bool ok = (4 * r < nrow) & colok;
            const double e = fma(s - c0, iT, 0.0);
            emax = fmax(emax, ok ? e : emax);
            const double tv = ok ? exp(e) : 0.0;   // padded atoms contribute nothing
            rs[r] += tv;    // increasing j per lane
            cs[t] += tv;    // increasing i with r
          }
        }
      }
      // column sums: over the four lane groups (rows lg + 4 r), then one slab entry per wave and column
#pragma unroll
      for (int t = 0; t < TILES; ++t) {
        cs[t] += __shfl_xor(cs[t], 16);
        cs[t] += __shfl_xor(cs[t], 32);
        if (lg == 0) s_sl[((ch & 1) * NW + wave) * CW + t * 16 + lc] = cs[t];
      }
      __syncthreads();
      // over the waves in wave order into the running column sum.  The slab has two halves: the waves that run ahead
      // write the other one, and this half is rewritten only behind the next barrier.
      if (tid < CW) {
        const int j = ch * CW + tid;
        if (j < NP) {
          double c = s_cs[j];
          for (int w = 0; w < NW; ++w) c += s_sl[((ch & 1) * NW + w) * CW + tid];
          s_cs[j] = c;
        }
      }
    }
    // row sums of this sweep: over the 16 lanes of the row (a butterfly: every lane ends with the same value)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      double v = rs[r];
#pragma unroll
      for (int o = 1; o < 16; o <<= 1) v += __shfl_xor(v, o);
      if (lc == 0 && 4 * r < nrow) s_rs[rtc * 16 + lg + 4 * r] = v;
    }
  }
  if (emax > POST_EXP_MAX) s_flag[0] = 1;
  __syncthreads();

  // ---- last phase: Z in index order (every thread, the same value), status, normalisation, log_sum
  double Z = 0.0;
  for (int i = 0; i < N; ++i) Z += s_rs[i];
  if (s_flag[0] != 0 || !(Z > 0.0) || !post_finite(Z)) {
    post_nan_rows(a, vox, 2, N, 2, tid, WG);
    return;
  }
  for (int n = tid; n < N; n += WG) {
    a.w[(vox * 2 + 0) * N + n] = s_rs[n] / Z;
    a.w[(vox * 2 + 1) * N + n] = s_cs[n] / Z;
  }
  if (tid == 0) {
    a.log_sum[vox] = log(Z) - shift / Tv;
    a.status[vox] = 0;
  }
}

// K = 1: one workgroup per voxel, one thread per atom; the unnormalised t(i) wait in the output row for Z
template <bool CSF, bool WGT = false>
__global__ __launch_bounds__(SWEEP_K1_WG) void mfx_post_k1_kernel(PostArgsT<WGT> a) {
  extern __shared__ double smem[];
  const int tid = threadIdx.x;
  const int M = a.P.M, N = a.T.N, ldn = a.T.ldn;
  const size_t vox = blockIdx.x;
  double* s_y = smem;          // [M]
  double* s_x = s_y + M;       // [M]
  double* s_t0 = s_x + M;      // [M]
  double* s_t1 = s_t0 + M;     // [M]
  double* s_w = s_t1 + M;      // [M] sqrt(W) (WGT)
  int* s_r0 = (int*)(s_w + (WGT ? M : 0));  // [M]
  int* s_r1 = s_r0 + M;        // [M]
  int* s_flag = s_r1 + M;      // [2]
  const double* __restrict__ yv = a.Y + vox * M;
  const double* __restrict__ pk = a.peaks + vox * 3;
  const double Tv = a.temp[vox], shift = a.shift[vox];
  if (tid == 0) mfx_check_dir(a.P, pk, (int)vox);
  if (!(Tv > 0.0) || !post_finite(Tv) || !post_finite(shift)) {
    post_nan_rows(a, vox, 1, N, 1, tid, SWEEP_K1_WG);
    return;
  }
  if constexpr (WGT) {
    if (const int code = sweep_weights_status(a.W + vox * a.wstride, M)) {
      post_nan_rows(a, vox, 1, N, code, tid, SWEEP_K1_WG);
      return;
    }
  }
  const double iT = 1.0 / Tv;
  for (int m = tid; m < M; m += SWEEP_K1_WG) {
    if constexpr (WGT) {
      const double s = sqrt(a.W[vox * a.wstride + m]);
      s_w[m] = s;
      s_y[m] = s * yv[m];
      s_x[m] = CSF ? s * a.xc[m] : 0.0;
    } else {
      s_y[m] = yv[m];
      s_x[m] = CSF ? a.xc[m] : 0.0;
    }
    const RowDesc rd = mfx_row_desc(a.T, a.P, m, pk[0], pk[1], pk[2]);
    s_r0[m] = rd.r0; s_t0[m] = rd.t0; s_r1[m] = rd.r1; s_t1[m] = rd.t1;
  }
  if (tid == 0) s_flag[0] = 0;
  __syncthreads();
  double y_sq = 0.0, xx = 0.0, xy = 0.0;
  for (int m = 0; m < M; ++m) {
    y_sq += s_y[m] * s_y[m];
    if constexpr (CSF) { xx += s_x[m] * s_x[m]; xy += s_x[m] * s_y[m]; }
  }
  const double ixx = (CSF && xx > 0.0) ? 1.0 / xx : 0.0;
  const double c0 = y_sq - shift;
  double* wrow = a.w + vox * N;
  bool over = false;
  for (int n = tid; n < N; n += SWEEP_K1_WG) {
    double a2 = 0.0, ay = 0.0, ax = 0.0;
    for (int m = 0; m < M; ++m) {
      RowDesc rd;
      rd.r0 = s_r0[m]; rd.t0 = s_t0[m]; rd.r1 = s_r1[m]; rd.t1 = s_t1[m];
      double d = mfx_eval_br(a.T.tab, ldn, rd, a.P.tG[m], a.P.dG[m], n);
      if constexpr (WGT) d = s_w[m] * d;
      a2 += d * d;
      ay += s_y[m] * d;
      if constexpr (CSF) ax += s_x[m] * d;
    }
    const double yp = fmax(ay, 0.0);
    double s = a2 > 0.0 ? yp * yp / a2 : 0.0;
    if constexpr (CSF) {
      double Ap, Yp, iAp;
      sweep_primed(a2, ay, ax, ixx, xy, Ap, Yp, iAp);
      const double w1 = fmax(Yp, 0.0) * iAp;
      if (fma(-w1, ax, xy) >= 0.0) s = xy * xy * ixx + Yp * w1;
    }
    const double e = fma(s - c0, iT, 0.0);
    over |= e > POST_EXP_MAX;
    wrow[n] = exp(e);
  }
  if (over) s_flag[0] = 1;
  __syncthreads();   // the row is written and visible to the workgroup
  double Z = 0.0;
  for (int i = 0; i < N; ++i) Z += wrow[i];   // index order, every thread the same value
  __syncthreads();   // every thread has read the unnormalised row before it is overwritten
  if (s_flag[0] != 0 || !(Z > 0.0) || !post_finite(Z)) {
    post_nan_rows(a, vox, 1, N, 2, tid, SWEEP_K1_WG);
    return;
  }
  for (int n = tid; n < N; n += SWEEP_K1_WG) wrow[n] = wrow[n] / Z;
  if (tid == 0) {
    a.log_sum[vox] = log(Z) - shift / Tv;
    a.status[vox] = 0;
  }
}

size_t post_lds_bytes(int ksteps, bool bracket, bool csf, int NP, int nw, int tiles, int nbuf, bool wgt) {
  return sweep_lds_bytes(ksteps, NP, bracket, csf, wgt, nbuf, tiles, post_own_dbl(NP, nw, 16 * tiles), POST_OWN_INT);
}
// the family's LDS bytes of a configuration, for sweep_pick and sweep_max_atoms
auto post_lds(bool br, bool csf, bool wgt) {
  return [=](const SweepCfg& c, int NP) { return post_lds_bytes(c.ks, br, csf, NP, c.nw, c.tiles, c.nbuf, wgt); };
}
int post_max_atoms(int M, bool br, bool csf, bool wgt = false) { return sweep_max_atoms(M, br, csf, post_lds(br, csf, wgt)); }

template <bool WGT>
struct PostLaunch {
  const PostArgsW& a;
  int nvox;
  hipStream_t st;
  template <int KS, bool BR, bool CSF, int NW, int TILES, int NBUF>
  int run() const {
    const PostArgsT<WGT> ka = a;   // the unweighted kernels take the PostArgs part
    sweep_record(KS, NW, TILES, NBUF, BR, CSF, false, WGT);
    return sweep_launch(mfx_post_k2_kernel<KS, BR, CSF, NW, TILES, NBUF, WGT>, ka, nvox, NW * 64,
                        post_lds_bytes(KS, BR, CSF, a.T.ldn, NW, TILES, NBUF, WGT), true, st);
  }
};

template <bool WGT>
int post_launch_k2(const PostArgsW& a, int nvox, bool csf, hipStream_t st, const char* fn) {
  return sweep_launch_k2(fn, "posterior", a, csf, post_lds(a.P.any_bracket != 0, csf, WGT), PostLaunch<WGT>{a, nvox, st});
}

template <bool WGT>
int post_launch_k1(const PostArgsW& a, int nvox, bool csf, hipStream_t st) {
  const size_t lds = sweep_k1_lds_bytes(a.P.M, WGT, POST_OWN_INT);
  const PostArgsT<WGT> ka = a;
  if (csf) return sweep_launch(mfx_post_k1_kernel<true, WGT>, ka, nvox, SWEEP_K1_WG, lds, false, st);
  return sweep_launch(mfx_post_k1_kernel<false, WGT>, ka, nvox, SWEEP_K1_WG, lds, false, st);
}

// shared body of the device entry points; wgt: d_W [V x M] (w_stride = M) or [M] (w_stride = 0) scales the rows
int post_enqueue(const char* fn, const mfx_plan* p, const double* d_Y, const double* d_peaks, int K, int csf_on,
                 const double* d_sig_csf, const double* d_T, const double* d_shift, int64_t V, double* d_w, double* d_log_sum,
                 int32_t* d_status, void* stream, bool wgt = false, const double* d_W = nullptr, int64_t w_stride = 0) {
  PostArgsW a{};
  bool run = false;
  if (int rc = sweep_enqueue_head(fn, p, d_Y, d_peaks, K, csf_on, d_sig_csf, V, d_T && d_shift && d_w && d_log_sum && d_status, wgt,
                                  d_W, w_stride, &a, &run)) return rc;
  if (!run) return MFX_OK;
  a.temp = d_T; a.shift = d_shift; a.w = d_w; a.log_sum = d_log_sum; a.status = d_status;
  hipStream_t st = (hipStream_t)stream;
  if (K == 2) return wgt ? post_launch_k2<true>(a, (int)V, csf_on != 0, st, fn) : post_launch_k2<false>(a, (int)V, csf_on != 0, st, fn);
  return wgt ? post_launch_k1<true>(a, (int)V, csf_on != 0, st) : post_launch_k1<false>(a, (int)V, csf_on != 0, st);
}

// shared body of the host entry points; the device count always comes before the plan
int post_host(const char* fn, const mfx_plan* p, const double* Y, const double* peaks, int K, int csf_on, const double* sig_csf,
              const double* T, const double* shift, int64_t V, double* w, double* log_sum, int32_t* status, bool wgt = false,
              const double* W = nullptr, int64_t w_stride = 0) {
  SweepHostIn in;
  bool run = false;
  if (int rc = in.stage(fn, p, Y, peaks, K, csf_on, sig_csf, V, T && shift && w && log_sum && status, true, wgt, W, w_stride, &run))
    return rc;
  if (!run) return MFX_OK;
  DevBuf<double> dT, dsh, dw, dls;
  DevBuf<int32_t> dst;
  HIPCHK(dT.upload(T, (size_t)V));
  HIPCHK(dsh.upload(shift, (size_t)V));
  HIPCHK(dw.alloc_n((size_t)V * K * in.N));
  HIPCHK(dls.alloc_n((size_t)V));
  HIPCHK(dst.alloc_n((size_t)V));
  if (int rc = post_enqueue(fn, p, in.Y.get(), in.peaks.get(), K, csf_on, in.x.get(), dT.get(), dsh.get(), V, dw.get(), dls.get(),
                            dst.get(), nullptr, wgt, in.W.get(), w_stride)) return rc;
  if (int rc = mfx_plan_status(p, nullptr)) return rc;   // waits; a direction that is not a unit vector
  HIPCHK(dw.download(w));
  HIPCHK(dls.download(log_sum));
  HIPCHK(dst.download(status));
  return MFX_OK;
}

}  // namespace

extern "C" int mfx_post_abi_version(void) { return 2; }

extern "C" int mfx_post_debug_last_config(int* form) { return sweep_last_form(form); }

extern "C" int mfx_post_max_atoms(const mfx_plan* p, int csf_on) {
  return sweep_plan_max_atoms(p, [=](int M, bool br) { return post_max_atoms(M, br, csf_on != 0); });
}

extern "C" int mfx_post_dev(const mfx_plan* p, const double* d_Y, const double* d_peaks, int K, int csf_on,
                            const double* d_sig_csf, const double* d_T, const double* d_shift, int64_t V, double* d_w,
                            double* d_log_sum, int32_t* d_status, void* stream) {
  return post_enqueue("mfx_post_dev", p, d_Y, d_peaks, K, csf_on, d_sig_csf, d_T, d_shift, V, d_w, d_log_sum, d_status, stream);
}

extern "C" int mfx_post(const mfx_plan* p, const double* Y, const double* peaks, int K, int csf_on, const double* sig_csf,
                        const double* T, const double* shift, int64_t V, double* w, double* log_sum, int32_t* status) {
  return post_host("mfx_post", p, Y, peaks, K, csf_on, sig_csf, T, shift, V, w, log_sum, status);
}

// ---- include/mfx_wsoft.h: the weighted forms (the profile's are in profile.hip)
int mfx_wsoft_prof_max_atoms(int M, bool br, bool csf, bool land);   // profile.hip

extern "C" int mfx_wsoft_abi_version(void) { return 1; }

extern "C" int mfx_wsoft_max_atoms(const mfx_plan* p, int csf_on, int what) {
  if (what < 0 || what > 2) return 0;
  return sweep_plan_max_atoms(p, [=](int M, bool br) {
    return what == 0 ? post_max_atoms(M, br, csf_on != 0, true) : mfx_wsoft_prof_max_atoms(M, br, csf_on != 0, what == 2);
  });
}

extern "C" int mfx_wpost_dev(const mfx_plan* p, const double* d_Y, const double* d_W, int64_t w_stride, const double* d_peaks, int K,
                             int csf_on, const double* d_sig_csf, const double* d_T, const double* d_shift, int64_t V, double* d_w,
                             double* d_log_sum, int32_t* d_status, void* stream) {
  return post_enqueue("mfx_wpost_dev", p, d_Y, d_peaks, K, csf_on, d_sig_csf, d_T, d_shift, V, d_w, d_log_sum, d_status, stream, true,
                      d_W, w_stride);
}

extern "C" int mfx_wpost(const mfx_plan* p, const double* Y, const double* W, int64_t w_stride, const double* peaks, int K, int csf_on,
                         const double* sig_csf, const double* T, const double* shift, int64_t V, double* w, double* log_sum,
                         int32_t* status) {
  return post_host("mfx_wpost", p, Y, peaks, K, csf_on, sig_csf, T, shift, V, w, log_sum, status, true, W, w_stride);
}
