// profile.hip -- objective profiles (include/mfx_profile.h): per atom of each fascicle the best objective any partner
// reaches with it, or the objective of every atom pair of a voxel.
//
// mfx_profile_k2_kernel   one workgroup per voxel, the structure of fit_k2.hip's phases 0-2: knot descriptors and y in
//                         LDS, column statistics of both rotated dictionaries (one thread per atom), then the cross-Gram
//                         D_0^T D_1 on v_mfma_f64_16x16x4_f64 with the wave's 16 atoms of D_0 in registers and D_1
//                         generated chunk by chunk into LDS.  Unlike the fit's scan, EVERY pair is scored here - the
//                         single-active cases included, and with CSF the projected three-unknown form - and what is kept
//                         is a minimum per row and per column, not one candidate list:
//                           rows     a wave owns its 16 atoms for a whole sweep over the chunks, so their minima live in
//                                    registers (C/D layout: col = lane & 15, row = (lane >> 4) + 4 reg) and are folded
//                                    over the 16 lanes of a row once per sweep;
//                           columns  folded in the lane over its 4 rows, over the 4 lane groups by shuffles, then over
//                                    the waves through a small LDS slab behind the barrier that ends the chunk anyway,
//                                    into per-atom arrays in LDS.  No global atomics, no N x N store.
//                         FP64 MFMA and VALU instructions do not overlap on a SIMD (fit_k2.hip), so the scan's
//                         instruction count is its cost: without CSF a pair's score ||y||^2 - F is kept as a fraction
//                         p / q, fractions are compared by cross-multiplication, and the division happens once per
//                         reported atom.  The CSF form needs the pair's weights (the sign of w_x decides which value
//                         holds) and divides per pair; it is the slow variant.
//                         LAND = true: the same Gram and scoring, every pair's value stored [N x N], no minima kept.
//                         All variants take the plain chunk loop of fit_k2.hip (the next chunk is generated before the
//                         MFMAs of the current one where two LDS buffers fit); its pipelined k-loop is not ported.
// mfx_profile_k1_kernel   one workgroup per voxel, one thread per atom: ||y||^2 - max(Y, 0)^2 / A (and the CSF form).
//
// The scoring helpers, the cut, the weights' scan and the host plumbing are soft_sweep.h's, shared with posterior.hip,
// whose K = 2 kernel restates phases 0-2 of this one.
//
// Error of a pair's value: each of the six Gram quantities carries at most M eps |a||b|, carried through
// (z1^2 - 2 c z1 z2 + z2^2) / (1 - c^2); tests hold the kernel to 16 M eps ||y||^2 / (1 - c^2).
#include "soft_sweep.h"
#include "../../include/mfx_profile.h"
#include "../../include/mfx_wsoft.h"

namespace {

struct ProfArgs : SweepArgs {
  double* obj;          // profile: [V x K x N]; landscape: [V x N x N]
  int* partner;         // [V x K x N] or null
};
// the weighted variants (include/mfx_wsoft.h) take two more arguments; the unweighted kernels keep ProfArgs as it is
struct ProfArgsW : ProfArgs {
  const double* W;      // [V x M] (wstride = M) or [M] (wstride = 0)
  long long wstride;
};
template <bool WGT> using ProfArgsT = std::conditional_t<WGT, ProfArgsW, ProfArgs>;

// a voxel with unusable weights: NaN values, partner -1 (every thread of the workgroup takes part)
__device__ __forceinline__ void prof_nan_rows(const ProfArgs& a, size_t vox, size_t n_out, int tid, int wg) {
  const double nan = __builtin_nan("");
  for (size_t n = tid; n < n_out; n += wg) {
    a.obj[vox * n_out + n] = nan;
    if (a.partner) a.partner[vox * n_out + n] = -1;
  }
}

// the K = 2 kernel's own LDS behind the common front of soft_sweep.h (none of it in the landscape form), for the host.  Doubles: the running column
// best as a fraction, [NP] each, and the waves' column bests of one chunk, [2][NW][CW] each; ints: their atom indices.
constexpr int prof_own_dbl(bool land, int NP, int nw, int cw) { return land ? 0 : 2 * NP + 2 * 2 * nw * cw; }
constexpr int prof_own_int(bool land, int NP, int nw, int cw) { return land ? 0 : NP + 2 * nw * cw; }

// NW waves per workgroup, TILES 16-atom column tiles per D_1 chunk, NBUF LDS buffers for the chunks (as fit_k2.hip):
// (8, 2, 2) for exact-G protocols of M <= 200 without CSF where it fits; (4, 1, 2) and (4, 1, 1) - one wave per SIMD with the whole register
// file - for the CSF form (whose scan keeps twice the per-row operands), G-bracketed rows, larger dictionaries and long protocols.
// WGT: rows scaled by s = sqrt(W) as they are generated (include/mfx_wsoft.h): one more [MP] array in LDS, y and x stored scaled,
// every generated entry multiplied by s_w[m]; all else is the same code.
template <int KSTEPS, bool BRACKET, bool CSF, bool LAND, int NW, int TILES, int NBUF, bool WGT = false>
__global__ __launch_bounds__(NW * 64, NW == 8 ? 2 : 1) void mfx_profile_k2_kernel(ProfArgsT<WGT> a) {
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

  // ---- LDS carve-up (prof_lds_bytes below mirrors it)
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
  double* s_cp = s_X2 + (CSF ? NP : 0);           // [NP] each: running column best as a fraction (profile)
  double* s_cq = s_cp + (LAND ? 0 : NP);
  double* s_sp = s_cq + (LAND ? 0 : NP);          // [2][NW][CW] each: the waves' column bests of one chunk
  double* s_sq = s_sp + (LAND ? 0 : 2 * NW * CW);
  double* s_end = s_sq + (LAND ? 0 : 2 * NW * CW);
  int* s_r0 = (int*)s_end;                        // [2][MP]
  int* s_r1 = s_r0 + 2 * MP;                      // [2][MP] (bracket only)
  int* s_ci = s_r1 + (BRACKET ? 2 * MP : 0);      // [NP]
  int* s_si = s_ci + (LAND ? 0 : NP);             // [2][NW][CW]

  // ---- phase 0: y, x, descriptors
  const double* __restrict__ yv = a.Y + vox * M;
  const double* __restrict__ pk = a.peaks + vox * 6;
  if constexpr (WGT) {   // unusable weights leave here, workgroup-uniform
    if (sweep_weights_unusable(a.W + vox * a.wstride, M)) {
      if (tid < 2) mfx_check_dir(a.P, pk + 3 * tid, (int)vox);
      prof_nan_rows(a, vox, (size_t)(LAND ? N : 2) * N, tid, WG);
      return;
    }
  }
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
  if (tid < 2) mfx_check_dir(a.P, pk + 3 * tid, (int)vox);
  if constexpr (!LAND) {
    for (int n = tid; n < NP; n += WG) { s_cp[n] = 0.0; s_cq[n] = 1.0; s_ci[n] = 0; }
  }
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
  double* const out_land = LAND ? a.obj + vox * (size_t)N * N : nullptr;

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
    bool rowok[4];
    double bp[4], bq[4];
    int bj[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int i = rtc * 16 + lg + 4 * r;
      rowok[r] = rt_valid && (i < N);
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
      bp[r] = 0.0; bq[r] = 1.0; bj[r] = 0;
    }

    for (int ch = 0; ch < nchunks; ++ch) {
      const int buf = (NBUF == 2) ? (ch & 1) : 0;
      if constexpr (NBUF == 2) {
        if (ch + 1 < nchunks) gen_chunk(ch + 1, buf ^ 1);
      } else if (ch > 0) {
        gen_chunk(ch, 0);   // single buffer: generate, barrier, consume, barrier
        __syncthreads();
      }
      double cp[TILES], cq[TILES];
      int ci[TILES];
#pragma unroll
      for (int t = 0; t < TILES; ++t) { cp[t] = 0.0; cq[t] = 1.0; ci[t] = 0; }
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
          double A22 = s_A22[jq], Y2 = s_Y2[jq];
          double p2 = 0.0, X2 = 0.0, A22u = 0.0, Y2u = 0.0, i22p = 0.0, i22u = 0.0;
          if constexpr (CSF) {
            X2 = s_X2[jq]; A22u = A22; Y2u = Y2;
            i22u = A22 > 0.0 ? 1.0 / A22 : 0.0;
            sweep_primed(A22u, Y2u, X2, ixx, xy, A22, Y2, i22p);
          } else {
            const double yp = fmax(Y2, 0.0);
            p2 = yp * yp;
          }
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            double p, q;
            if constexpr (CSF) {
              // x projected out: the two-variable form on the primed quantities, then the sign of w_x decides
              double w1, w2, v1, v2;
              const double A12p = fma(-X1s[r], X2, acc[r]);
              const double sp = sweep_pair_w(A11r[r], A22, A12p, Y1r[r], Y2, i11p[r], i22p, w1, w2);
              const double wxn = fma(-w2, X2, fma(-w1, X1r[r], xy));   // w_x times x.x
              const double su = sweep_pair_w(A11u[r], A22u, acc[r], Y1u[r], Y2u, i11u[r], i22u, v1, v2);
              p = (wxn >= 0.0) ? sx + sp : su;
              q = 1.0;
            } else {
              sweep_pair_frac(A11r[r], A22, acc[r], Y1r[r], Y2, p1r[r], p2, p, q);
            }
            const bool ok = rowok[r] & colok;
            if constexpr (LAND) {
              if (ok) out_land[(size_t)(rtc * 16 + lg + 4 * r) * N + j] = y_sq - (q > 0.0 ? p / q : 0.0);
            } else {
              p = ok ? p : 0.0;   // padded atoms never win (strict comparisons)
              const bool brow = p * bq[r] > bp[r] * q;   // increasing j per lane: the first best stays
              bp[r] = brow ? p : bp[r];
              bq[r] = brow ? q : bq[r];
              bj[r] = brow ? j : bj[r];
              const bool bcol = p * cq[t] > cp[t] * q;   // increasing i with r
              cp[t] = bcol ? p : cp[t];
              cq[t] = bcol ? q : cq[t];
              ci[t] = bcol ? rtc * 16 + lg + 4 * r : ci[t];
            }
          }
        }
      }
      if constexpr (!LAND) {
        // column bests: over the four lane groups (rows lg + 4 r), then one slab entry per wave and column
#pragma unroll
        for (int t = 0; t < TILES; ++t) {
#pragma unroll
          for (int o = 16; o <= 32; o <<= 1) {
            const double p2 = __shfl_xor(cp[t], o), q2 = __shfl_xor(cq[t], o);
            const int i2 = __shfl_xor(ci[t], o);
            const double l = p2 * cq[t], rgt = cp[t] * q2;
            const bool take = (l > rgt) || (l == rgt && i2 < ci[t]);
            cp[t] = take ? p2 : cp[t];
            cq[t] = take ? q2 : cq[t];
            ci[t] = take ? i2 : ci[t];
          }
          if (lg == 0) {
            const int s = ((ch & 1) * NW + wave) * CW + t * 16 + lc;
            s_sp[s] = cp[t]; s_sq[s] = cq[t]; s_si[s] = ci[t];
          }
        }
      }
      __syncthreads();
      if constexpr (!LAND) {
        // over the waves (increasing atom index: the first best stays) into the running column best.  The slab has two
        // halves: the waves that run ahead write the other one, and this half is rewritten only behind the next barrier.
        if (tid < CW) {
          const int j = ch * CW + tid;
          if (j < NP) {
            double p = s_cp[j], q = s_cq[j];
            int i = s_ci[j];
            for (int w = 0; w < NW; ++w) {
              const int s = ((ch & 1) * NW + w) * CW + tid;
              const double p2 = s_sp[s], q2 = s_sq[s];
              const bool take = p2 * q > p * q2;
              p = take ? p2 : p;
              q = take ? q2 : q;
              i = take ? s_si[s] : i;
            }
            s_cp[j] = p; s_cq[j] = q; s_ci[j] = i;
          }
        }
      }
    }
    if constexpr (!LAND) {
      // row bests of this sweep: one division per (lane, row), then over the 16 lanes of the row (ties: lowest j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        double v = bp[r] / bq[r];
        int j = bj[r];
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) {
          const double v2 = __shfl_xor(v, o);
          const int j2 = __shfl_xor(j, o);
          const bool take = (v2 > v) || (v2 == v && j2 < j);
          v = take ? v2 : v;
          j = take ? j2 : j;
        }
        const int i = rtc * 16 + lg + 4 * r;
        if (lc == 0 && rowok[r]) {
          a.obj[(vox * 2 + 0) * N + i] = y_sq - v;
          if (a.partner) a.partner[(vox * 2 + 0) * N + i] = j;
        }
      }
    }
  }
  if constexpr (!LAND) {
    __syncthreads();
    for (int j = tid; j < N; j += WG) {
      a.obj[(vox * 2 + 1) * N + j] = y_sq - s_cp[j] / s_cq[j];
      if (a.partner) a.partner[(vox * 2 + 1) * N + j] = s_ci[j];
    }
  }
}

// K = 1: one workgroup per voxel, one thread per atom
template <bool CSF, bool WGT = false>
__global__ __launch_bounds__(SWEEP_K1_WG) void mfx_profile_k1_kernel(ProfArgsT<WGT> a) {
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
  const double* __restrict__ yv = a.Y + vox * M;
  const double* __restrict__ pk = a.peaks + vox * 3;
  if constexpr (WGT) {
    if (sweep_weights_unusable(a.W + vox * a.wstride, M)) {
      if (tid == 0) mfx_check_dir(a.P, pk, (int)vox);
      prof_nan_rows(a, vox, (size_t)N, tid, SWEEP_K1_WG);
      return;
    }
  }
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
  if (tid == 0) mfx_check_dir(a.P, pk, (int)vox);
  __syncthreads();
  double y_sq = 0.0, xx = 0.0, xy = 0.0;
  for (int m = 0; m < M; ++m) {
    y_sq += s_y[m] * s_y[m];
    if constexpr (CSF) { xx += s_x[m] * s_x[m]; xy += s_x[m] * s_y[m]; }
  }
  const double ixx = (CSF && xx > 0.0) ? 1.0 / xx : 0.0;
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
    a.obj[vox * N + n] = y_sq - s;
    if (a.partner) a.partner[vox * N + n] = -1;
  }
}

size_t prof_lds_bytes(int ksteps, bool bracket, bool csf, bool land, int NP, int nw, int tiles, int nbuf, bool wgt) {
  return sweep_lds_bytes(ksteps, NP, bracket, csf, wgt, nbuf, tiles, prof_own_dbl(land, NP, nw, 16 * tiles),
                         prof_own_int(land, NP, nw, 16 * tiles));
}
// the family's LDS bytes of a configuration, for sweep_pick and sweep_max_atoms
auto prof_lds(bool br, bool csf, bool land, bool wgt) {
  return [=](const SweepCfg& c, int NP) { return prof_lds_bytes(c.ks, br, csf, land, NP, c.nw, c.tiles, c.nbuf, wgt); };
}
int prof_max_atoms(int M, bool br, bool csf, bool land, bool wgt = false) { return sweep_max_atoms(M, br, csf, prof_lds(br, csf, land, wgt)); }

template <bool LAND, bool WGT>
struct ProfLaunch {
  const ProfArgsW& a;
  int nvox;
  hipStream_t st;
  template <int KS, bool BR, bool CSF, int NW, int TILES, int NBUF>
  int run() const {
    const ProfArgsT<WGT> ka = a;   // the unweighted kernels take the ProfArgs part
    sweep_record(KS, NW, TILES, NBUF, BR, CSF, LAND, WGT);
    return sweep_launch(mfx_profile_k2_kernel<KS, BR, CSF, LAND, NW, TILES, NBUF, WGT>, ka, nvox, NW * 64,
                        prof_lds_bytes(KS, BR, CSF, LAND, a.T.ldn, NW, TILES, NBUF, WGT), true, st);
  }
};

template <bool WGT>
int prof_launch_k2(const ProfArgsW& a, int nvox, bool csf, bool land, hipStream_t st, const char* fn) {
  if (a.P.M > 560) return mfx_fail(MFX_ERR_UNSUPPORTED, "%s: the K = 2 kernel supports M <= 560 (got %d)", fn, a.P.M);
  const auto lds = prof_lds(a.P.any_bracket != 0, csf, land, WGT);
  if (land) return sweep_launch_k2(fn, "profile", a, csf, lds, ProfLaunch<true, WGT>{a, nvox, st});
  return sweep_launch_k2(fn, "profile", a, csf, lds, ProfLaunch<false, WGT>{a, nvox, st});
}

template <bool WGT>
int prof_launch_k1(const ProfArgsW& a, int nvox, bool csf, hipStream_t st) {
  const size_t lds = sweep_k1_lds_bytes(a.P.M, WGT, 0);
  const ProfArgsT<WGT> ka = a;
  if (csf) return sweep_launch(mfx_profile_k1_kernel<true, WGT>, ka, nvox, SWEEP_K1_WG, lds, false, st);
  return sweep_launch(mfx_profile_k1_kernel<false, WGT>, ka, nvox, SWEEP_K1_WG, lds, false, st);
}

// shared body of the device entry points; wgt: d_W [V x M] (w_stride = M) or [M] (w_stride = 0) scales the rows
int prof_enqueue(const char* fn, const mfx_plan* p, const double* d_Y, const double* d_peaks, int K, int csf_on,
                 const double* d_sig_csf, int64_t V, double* d_obj, int32_t* d_partner, bool land, void* stream, bool wgt = false,
                 const double* d_W = nullptr, int64_t w_stride = 0) {
  ProfArgsW a{};
  bool run = false;
  if (int rc = sweep_enqueue_head(fn, p, d_Y, d_peaks, K, csf_on, d_sig_csf, V, d_obj != nullptr, wgt, d_W, w_stride, &a, &run)) return rc;
  if (!run) return MFX_OK;
  a.obj = d_obj; a.partner = d_partner;
  hipStream_t st = (hipStream_t)stream;
  if (K == 2)
    return wgt ? prof_launch_k2<true>(a, (int)V, csf_on != 0, land, st, fn) : prof_launch_k2<false>(a, (int)V, csf_on != 0, land, st, fn);
  return wgt ? prof_launch_k1<true>(a, (int)V, csf_on != 0, st) : prof_launch_k1<false>(a, (int)V, csf_on != 0, st);
}

// shared body of the host entry points: out [V x rows x N] with rows = K (profile) or N (landscape).  The device count
// comes before the plan only in the weighted forms.
int prof_host(const char* fn, const mfx_plan* p, const double* Y, const double* peaks, int K, int csf_on, const double* sig_csf,
              int64_t V, double* obj, int32_t* partner, bool land, bool wgt = false, const double* W = nullptr, int64_t w_stride = 0) {
  SweepHostIn in;
  bool run = false;
  if (int rc = in.stage(fn, p, Y, peaks, K, csf_on, sig_csf, V, obj != nullptr, wgt, wgt, W, w_stride, &run)) return rc;
  if (!run) return MFX_OK;
  const size_t nout = (size_t)V * (land ? in.N : (size_t)K) * in.N;
  DevBuf<double> dobj;
  DevBuf<int32_t> dpar;   // stays null without partner
  HIPCHK(dobj.alloc_n(nout));
  if (partner) HIPCHK(dpar.alloc_n(nout));
  if (int rc = prof_enqueue(fn, p, in.Y.get(), in.peaks.get(), K, csf_on, in.x.get(), V, dobj.get(), dpar.get(), land, nullptr, wgt,
                            in.W.get(), w_stride)) return rc;
  if (int rc = mfx_plan_status(p, nullptr)) return rc;   // waits; a direction that is not a unit vector
  HIPCHK(dobj.download(obj));
  if (partner) HIPCHK(dpar.download(partner));
  return MFX_OK;
}

}  // namespace

extern "C" int mfx_profile_abi_version(void) { return 2; }

extern "C" int mfx_profile_debug_last_config(int* form) { return sweep_last_form(form); }

extern "C" double mfx_profile_cut(void) { return MFX_PROFILE_CUT; }

extern "C" int mfx_profile_max_atoms(const mfx_plan* p, int csf_on, int landscape) {
  return sweep_plan_max_atoms(p, [=](int M, bool br) { return prof_max_atoms(M, br, csf_on != 0, landscape != 0); });
}

extern "C" int mfx_profile_dev(const mfx_plan* p, const double* d_Y, const double* d_peaks, int K, int csf_on,
                               const double* d_sig_csf, int64_t V, double* d_obj, int32_t* d_partner, void* stream) {
  return prof_enqueue("mfx_profile_dev", p, d_Y, d_peaks, K, csf_on, d_sig_csf, V, d_obj, d_partner, false, stream);
}

extern "C" int mfx_profile(const mfx_plan* p, const double* Y, const double* peaks, int K, int csf_on, const double* sig_csf,
                           int64_t V, double* obj, int32_t* partner) {
  return prof_host("mfx_profile", p, Y, peaks, K, csf_on, sig_csf, V, obj, partner, false);
}

extern "C" int mfx_pair_objectives_dev(const mfx_plan* p, const double* d_Y, const double* d_peaks, int csf_on,
                                       const double* d_sig_csf, int64_t V, double* d_out, void* stream) {
  return prof_enqueue("mfx_pair_objectives_dev", p, d_Y, d_peaks, 2, csf_on, d_sig_csf, V, d_out, nullptr, true, stream);
}

extern "C" int mfx_pair_objectives(const mfx_plan* p, const double* Y, const double* peaks, int csf_on, const double* sig_csf,
                                   int64_t V, double* out) {
  return prof_host("mfx_pair_objectives", p, Y, peaks, 2, csf_on, sig_csf, V, out, nullptr, true);
}

// ---- include/mfx_wsoft.h: the weighted forms (the posterior's are in posterior.hip)
int mfx_wsoft_prof_max_atoms(int M, bool br, bool csf, bool land) { return prof_max_atoms(M, br, csf, land, true); }

extern "C" int mfx_wprofile_dev(const mfx_plan* p, const double* d_Y, const double* d_W, int64_t w_stride, const double* d_peaks, int K,
                                int csf_on, const double* d_sig_csf, int64_t V, double* d_obj, int32_t* d_partner, void* stream) {
  return prof_enqueue("mfx_wprofile_dev", p, d_Y, d_peaks, K, csf_on, d_sig_csf, V, d_obj, d_partner, false, stream, true, d_W, w_stride);
}

extern "C" int mfx_wprofile(const mfx_plan* p, const double* Y, const double* W, int64_t w_stride, const double* peaks, int K,
                            int csf_on, const double* sig_csf, int64_t V, double* obj, int32_t* partner) {
  return prof_host("mfx_wprofile", p, Y, peaks, K, csf_on, sig_csf, V, obj, partner, false, true, W, w_stride);
}

extern "C" int mfx_wpair_objectives_dev(const mfx_plan* p, const double* d_Y, const double* d_W, int64_t w_stride, const double* d_peaks,
                                        int csf_on, const double* d_sig_csf, int64_t V, double* d_out, void* stream) {
  return prof_enqueue("mfx_wpair_objectives_dev", p, d_Y, d_peaks, 2, csf_on, d_sig_csf, V, d_out, nullptr, true, stream, true, d_W,
                      w_stride);
}

extern "C" int mfx_wpair_objectives(const mfx_plan* p, const double* Y, const double* W, int64_t w_stride, const double* peaks,
                                    int csf_on, const double* sig_csf, int64_t V, double* out) {
  return prof_host("mfx_wpair_objectives", p, Y, peaks, 2, csf_on, sig_csf, V, out, nullptr, true, true, W, w_stride);
}
