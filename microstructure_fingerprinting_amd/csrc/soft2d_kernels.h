// soft2d_kernels.h -- the kernels of the soft fits and objective profiles of voxels of a 2-D protocol, without measurement
// weights (soft2d.hip instantiates <MODE, false>) and with them (w2d.hip, <MODE, true>).  No translation unit of its own.
//
// WGT: F_W is the F below on rows scaled by s = sqrt(W) (include/mfx_w2d.h): every entry fl(s_m * d), y' = s y, both from
// w2d_prep_kernel (fit2d_kernels.h) through W2Args.  What WGT adds: the weights' status, tested after T (posterior 3 / 4); s_m of a
// chunk's rows staged in LDS beside the rows' records and store_chunk's multiply by it, as in mfx_fit2d_k2_kernel; the
// serial sums of phase 1 over fl(s_m d) and y'.  The chunk loop and the pair walk are one text.
//
// mfx_soft2d_k2_kernel<MODE, WGT>   K = 2: one 4-wave workgroup per voxel on the skeleton of mfx_fit2d_k2_kernel (fit2d_kernels.h).
//   phase 1  ||y||^2 and the column statistics |d|^2, d.y of both dictionaries: one thread per atom, serial over the rows.
//   phase 2  the cross-Gram D_0^T D_1 in 128 x 128 blocks on v_mfma_f64_16x16x4_f64, accumulated over the rows in chunks
//            of 8: the 16 accumulator tiles of a wave (64 x 64 atoms) persist across the chunks, both operands of a chunk
//            are generated into double-buffered LDS tiles from the staged 32-byte records.  The loop is the fit's, word
//            for word; nothing depends on M beyond R2_MAX_ROWS.
//            What happens to a finished block is new.  Every pair is scored through post_pair_frac (posterior.hip's,
//            restated: F is the profile's value by definition) and one division:
//              posterior  t = exp((score - (||y||^2 - shift)) / T), one FP64 exp per pair.  A row's partial sum runs over
//                         the lane's four columns (ascending), then over the 16 lanes of the row; a column's over the
//                         lane's 16 rows (ascending), then over the four lane groups.  Each wave leaves its 64 row and
//                         64 column partials in an LDS slab; behind a barrier one thread per atom adds the block's two
//                         halves, in order, to R0[N] / R1[N] in LDS.  Blocks are walked in order, so every sum has one
//                         fixed order.  Then Z (the row sums in index order), the division and log_sum.
//              profile    the same walk with running maxima of the score and their partner indices; strict comparisons
//                         in ascending index order, and the lower index on equality wherever two lanes meet: a tie goes
//                         to the lowest index.
//            Both modes are ONE kernel template with a compile-time mode.  Register budget: 256 per lane
//            (__launch_bounds__(256, 2)), accumulators in architectural VGPRs, no spill.
// mfx_soft2d_k1_kernel<MODE, WGT>   K = 1: one workgroup per voxel, one thread per atom, serial statistics.
// A voxel with a failing direction (fit2d_status_kernel wrote its record) gets NaN rows from the kernel itself.
#pragma once
#include "fit2d_shared.h"

#include <type_traits>

// profile.hip's MFX_PROFILE_CUT restated as a compile-time constant; the entry points of soft2d.hip refuse to launch unless
// it equals mfx_profile_cut()
#define MFX_SOFT2D_CUT 1e-8

namespace {

constexpr int S2_POST = 0, S2_PROF = 1;
constexpr size_t S2_LDS_MAX = 160 * 1024;
constexpr int S2_K1_WG = 256;
constexpr double S2_EXP_MAX = 700.0;   // exponents above this make the shift unusable (status 2)
constexpr int S2_NO_PARTNER = 0x7fffffff;

struct S2Args {
  int M, N;
  const double* base;
  const F2Rec* rec;     // [V K x M]
  const double* Y;      // [V x M]
  const int* vstat;     // [V x 5]
  const double* temp;   // [V] (posterior)
  const double* shift;  // [V] (posterior)
  double* out;          // [V x K x N]: w or obj
  double* log_sum;      // [V] (posterior)
  int* status;          // [V] (posterior)
  int* partner;         // [V x K x N] or null (profile)
};
template <bool WGT> using S2ArgsT = std::conditional_t<WGT, W2Args, S2Args>;

// score s = ||y||^2 - F of one atom pair as the fraction p / q (posterior.hip: post_pair_frac; profile.hip: prof_pair_frac)
__device__ __forceinline__ void s2_pair_frac(double A11, double A22, double A12, double Y1, double Y2, double p1, double p2,
                                             double& p, double& q) {
  const double d1 = fma(-A12, Y2, A22 * Y1);
  const double d2 = fma(-A12, Y1, A11 * Y2);
  const double pd = A11 * A22;
  const double Det = fma(-A12, A12, pd);
  const double num = fma(Y2, d2, Y1 * d1);
  const bool both = (d1 > 0.0) & (d2 > 0.0) & (Det > MFX_SOFT2D_CUT * pd);
  const bool first = p1 * A22 >= p2 * A11;
  p = both ? num : (first ? p1 : p2);
  q = both ? Det : (first ? A11 : A22);
}

__device__ __forceinline__ bool s2_finite(double x) { return fabs(x) <= 1.79769313486231570815e308; }   // false for NaN

// a voxel without a result: NaN rows (partner -1), NaN log_sum and the status code (every thread of the workgroup takes part)
template <int MODE, class Args>
__device__ __forceinline__ void s2_nan_rows(const Args& a, size_t vox, int K, int code, int tid, int wg) {
  const double nan = __builtin_nan("");
  const size_t n_out = (size_t)K * a.N;
  for (size_t n = tid; n < n_out; n += wg) {
    a.out[vox * n_out + n] = nan;
    if (MODE == S2_PROF && a.partner) a.partner[vox * n_out + n] = -1;
  }
  if (MODE == S2_POST && tid == 0) { a.log_sum[vox] = nan; a.status[vox] = code; }
}

// wgt: plus the staged s of two chunks
size_t s2_lds_bytes(int mode, int NP, bool wgt) {
  const size_t dbl = (size_t)2 * F2_NT * F2_TS + 4 * (size_t)NP + 2 * (size_t)NP + 4 * F2_BLK + 8 + (wgt ? 2 * F2_MC : 0);
  const size_t ints = (mode == S2_PROF ? 2 * (size_t)NP + 4 * F2_BLK : 0) + 4;
  return dbl * sizeof(double) + F2_REC * sizeof(F2Rec) + ints * sizeof(int);
}

int s2_max_atoms(int mode, bool wgt) {
  int n = 0;
  while (n < (1 << 20) && s2_lds_bytes(mode, n + 16, wgt) <= S2_LDS_MAX) n += 16;
  return n;
}

template <int MODE, bool WGT>
__global__ __launch_bounds__(F2_WG, 2) void mfx_soft2d_k2_kernel(S2ArgsT<WGT> a) {
  constexpr bool POST = MODE == S2_POST;
  extern __shared__ double smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lg = lane >> 4, lc = lane & 15;
  const int wr = wave >> 1, wc = wave & 1;
  const int M = a.M, N = a.N;
  const int NP = (N + 15) & ~15;   // atoms padded to a multiple of 16 (padded atoms are zero columns)
  const int ntiles = NP >> 4;
  const size_t vox = blockIdx.x;
  if (a.vstat[5 * vox] != 0) {     // a failing direction (workgroup-uniform)
    s2_nan_rows<MODE>(a, vox, 2, 5, tid, F2_WG);
    return;
  }
  if constexpr (POST) {
    const double Tv = a.temp[vox], shift = a.shift[vox];
    if (!(Tv > 0.0) || !s2_finite(Tv) || !s2_finite(shift)) {
      s2_nan_rows<MODE>(a, vox, 2, 1, tid, F2_WG);
      return;
    }
  }
  if constexpr (WGT) {
    if (a.wstat[vox] != 0) {       // unusable weights (workgroup-uniform): 3 a bad weight, 4 none positive
      s2_nan_rows<MODE>(a, vox, 2, 2 + a.wstat[vox], tid, F2_WG);
      return;
    }
  }

  // ---- LDS carve-up (s2_lds_bytes mirrors it)
  double* sT = smem;                                    // [2][F2_NT][F2_TS]: tiles 0..7 the D_0 block, 8..15 the D_1 block
  double2* s_st = (double2*)(sT + 2 * F2_NT * F2_TS);   // [2][NP] column statistics {|d|^2, d.y} of D_0, then of D_1
  double* s_R = (double*)(s_st + 2 * NP);               // [2][NP] running row (R0) and column (R1) sums / best scores
  double* s_sl = s_R + 2 * NP;                          // [4][F2_BLK] the waves' partials of one block: rows by wc, columns by wr
  double* s_red = s_sl + 4 * F2_BLK;                    // [8]: [0] ||y||^2, [1] ||y||^2 - shift, [2] 1 / T
  double* s_sc = s_red + 8;                             // [2][F2_MC] staged s of two chunks (WGT)
  F2Rec* s_rec = (F2Rec*)(s_sc + (WGT ? 2 * F2_MC : 0));   // [F2_REC] staged records of two chunks
  int* s_Ri = (int*)(s_rec + F2_REC);                   // [2][NP] partners of the running bests (profile)
  int* s_sli = s_Ri + (POST ? 0 : 2 * NP);              // [4][F2_BLK] (profile)
  int* s_flag = s_sli + (POST ? 0 : 4 * F2_BLK);        // [4]: [0] an exponent above S2_EXP_MAX was met

  const double* __restrict__ ys = a.Y + vox * M;        // the signal; WGT: y' = s y
  const double* __restrict__ sv = nullptr;              // s (WGT)
  if constexpr (WGT) { ys = a.Ys + vox * M; sv = a.S + vox * M; }
  const size_t rec0 = 2 * vox * M;                      // records of direction k: + k M

  // ---- phase 1: ||y||^2 and the column statistics, sequential over the measurements
  if (tid == 0) {
    s_flag[0] = 0;
    double s = 0.0;
    for (int m = 0; m < M; ++m) s += ys[m] * ys[m];
    s_red[0] = s;
    if constexpr (POST) {   // exponent of a pair: (score - c0) / T = -(F - shift) / T; the scan reads both from LDS (no register lives
      s_red[1] = s - a.shift[vox];   // through the chunk loop for them)
      s_red[2] = 1.0 / a.temp[vox];
    }
  }
  for (int col = tid; col < 2 * NP; col += F2_WG) {
    const int k = col >= NP, n = col - k * NP;
    double a2 = 0.0, ay = 0.0;
    if (n < N) {
#pragma unroll 4
      for (int m = 0; m < M; ++m) {
        const F2Rec r = a.rec[rec0 + (size_t)k * M + m];
        const double sm = WGT ? sv[m] : 1.0;   // s_m (WGT)
        double d = f2_value(a.base, r, n);
        if constexpr (WGT) d = sm * d;   // fl(s_m d)
        a2 += d * d;
        ay += ys[m] * d;
      }
    }
    s_st[col] = double2{a2, ay};
    s_R[col] = POST ? 0.0 : -1.0;          // a score is never negative: the first real pair wins
    if constexpr (!POST) s_Ri[col] = S2_NO_PARTNER;
  }
  __syncthreads();
  bool over = false;                       // this lane met an exponent above S2_EXP_MAX on a pair of two real atoms

  // ---- phase 2: cross-Gram blocks accumulated over the rows in chunks (mfx_fit2d_k2_kernel's loop), then the block's pairs
  const int nblk = (NP + F2_BLK - 1) / F2_BLK;
  const int nchunks = (M + F2_MC - 1) / F2_MC;
  const int gk = wave >> 1;
  const int gc = tid & (F2_BLK - 1);
  double* const gdst0 = sT + (gk * 8 + (gc >> 4)) * F2_TS + (gc & 15);
  auto stage_rec = [&](int ch) {
    if (tid < 2 * F2_MC) {
      const int side = tid / F2_MC, r = tid % F2_MC, m = ch * F2_MC + r;
      const int q = ((ch & 1) * 2 + side) * F2_MC + r;
      const bool in = m < M;                      // rows beyond the protocol: S_par = 0 on the reference's zero -> entry 0
      F2Rec rc = a.rec[rec0 + (size_t)side * M + (in ? m : 0)];
      if (!in) { rc.s = 0.0; rc.dx = 0.0; rc.o = R2_OP_ZERO; rc.a = 0; rc.b = 0; }
      s_rec[q] = rc;
    } else if (WGT && tid < 3 * F2_MC) {   // s of the chunk's rows (0 beyond the protocol), by chunk parity
      const int r = tid - 2 * F2_MC, m = ch * F2_MC + r;
      s_sc[(ch & 1) * F2_MC + r] = m < M ? sv[m] : 0.0;
    }
  };

  for (int rb = 0; rb < nblk; ++rb) {
    const int nta = min(max(ntiles - (rb * 8 + wr * 4), 0), 4);   // valid row tiles of this wave (wave-uniform)
    for (int cb = 0; cb < nblk; ++cb) {
      const int ntb = min(max(ntiles - (cb * 8 + wc * 4), 0), 4);
      const int gn = (gk ? cb : rb) * F2_BLK + gc;   // this thread's atom
      const double* gbase = a.base + (gn < N ? gn : 0);
      double va[F2_MC], vb[F2_MC];
      auto load_chunk = [&](int ch) {
        const int q0 = ((ch & 1) * 2 + gk) * F2_MC;
#pragma unroll
        for (int r = 0; r < F2_MC; ++r) {
          va[r] = gbase[s_rec[q0 + r].a];
          vb[r] = gbase[s_rec[q0 + r].b];
        }
      };
      auto store_chunk = [&](int ch, int buf) {
        const int q0 = ((ch & 1) * 2 + gk) * F2_MC;
        double* dst = gdst0 + (size_t)buf * (F2_NT * F2_TS);
#pragma unroll
        for (int r = 0; r < F2_MC; ++r) {
          const double sm = WGT ? s_sc[(ch & 1) * F2_MC + r] : 1.0;   // s_m (WGT)
          double v = r2_value(s_rec[q0 + r].o, s_rec[q0 + r].s, va[r], s_rec[q0 + r].dx, vb[r]);
          if constexpr (WGT) v = sm * v;
          dst[r * 16] = gn < N ? v : 0.0;   // atoms beyond the dictionary: zero columns
        }
      };
      d4 acc[4][4];
#pragma unroll
      for (int ti = 0; ti < 4; ++ti)
#pragma unroll
        for (int tj = 0; tj < 4; ++tj) acc[ti][tj] = d4{0, 0, 0, 0};

      if constexpr (WGT) {   // an index the compiler cannot see through: see mfx_fit2d_k2_kernel
        int ch0 = 0;
        asm volatile("" : "+s"(ch0));
        stage_rec(ch0);
        stage_rec(ch0 + 1);
      } else {
        stage_rec(0);
        stage_rec(1);
      }
      __syncthreads();
      load_chunk(0);
      store_chunk(0, 0);
      __syncthreads();
      for (int ch = 0; ch < nchunks; ++ch) {
        const int buf = ch & 1;
        const bool more = ch + 1 < nchunks;
        if (ch + 2 < nchunks) stage_rec(ch + 2);   // into the parity of chunk ch, whose records nobody reads any more
        if (more) load_chunk(ch + 1);
        if (nta > 0 && ntb > 0) {
          const double* tA = sT + (size_t)buf * (F2_NT * F2_TS) + (wr * 4) * F2_TS + lg * 16 + lc;
          const double* tB = sT + (size_t)buf * (F2_NT * F2_TS) + (8 + wc * 4) * F2_TS + lg * 16 + lc;
#pragma unroll
          for (int kk = 0; kk < F2_MC / 4; ++kk) {
            double av[4], bv[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) { av[t] = tA[t * F2_TS + kk * 64]; bv[t] = tB[t * F2_TS + kk * 64]; }
#pragma unroll
            for (int ti = 0; ti < 4; ++ti)
#pragma unroll
              for (int tj = 0; tj < 4; ++tj)
                acc[ti][tj] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[ti], bv[tj], acc[ti][tj], 0, 0, 0);
          }
        }
        if (more) store_chunk(ch + 1, buf ^ 1);
        __syncthreads();
      }

      // ---- the block's pairs.  C/D layout of a tile: column lc, rows lg + 4 r.  Row i of the lane: its columns
      // j = lc (mod 16) of this wave's half of the block, ascending; column j: the lane's 16 rows, ascending.
      double cs[4];   // per column tile: the lane's column sum / best score
      int ci[4];      // (profile) and its row
#pragma unroll
      for (int t = 0; t < 4; ++t) { cs[t] = POST ? 0.0 : -1.0; ci[t] = S2_NO_PARTNER; }
      mfx_static_for<0, 4>([&](auto tic) {
        constexpr int ti = decltype(tic)::value;
#pragma unroll 1
        for (int r = 0; r < 4; ++r) {
          const int il = wr * 64 + ti * 16 + lg + 4 * r;   // row within the block
          const int i = rb * F2_BLK + il;
          double rv = POST ? 0.0 : -1.0;
          int rj = S2_NO_PARTNER;
          if (ti < nta) {   // wave-uniform; i < NP
            const double A11 = s_st[i].x, Y1 = s_st[i].y;
            const double yp1 = fmax(Y1, 0.0), p1 = yp1 * yp1;
            mfx_static_for<0, 4>([&](auto tjc) {
              constexpr int tj = decltype(tjc)::value;
              if (tj < ntb) {   // wave-uniform; j < NP
                const int j = cb * F2_BLK + wc * 64 + tj * 16 + lc;
                const double A22 = s_st[NP + j].x, Y2 = s_st[NP + j].y;
                const double yp2 = fmax(Y2, 0.0), p2 = yp2 * yp2;
                const d4& v = acc[ti][tj];
                const double A12 = r == 0 ? v[0] : (r == 1 ? v[1] : (r == 2 ? v[2] : v[3]));
                double p, q;
                s2_pair_frac(A11, A22, A12, Y1, Y2, p1, p2, p, q);
                const double s = q > 0.0 ? p / q : 0.0;
                const bool ok = (i < N) & (j < N);   // padded atoms contribute nothing
                if constexpr (POST) {
                  const double e = (s - s_red[1]) * s_red[2];
                  over |= ok & (e > S2_EXP_MAX);
                  const double tv = ok ? exp(e) : 0.0;
                  rv += tv;
                  cs[tj] += tv;
                  __builtin_amdgcn_sched_barrier(0);   // one pair's exp at a time: four interleaved ones do not fit the register budget
                } else {
                  const double sc = ok ? s : -1.0;
                  const bool brow = sc > rv;        // ascending j: the first best stays
                  rv = brow ? sc : rv;
                  rj = brow ? j : rj;
                  const bool bcol = sc > cs[tj];    // ascending i
                  cs[tj] = bcol ? sc : cs[tj];
                  ci[tj] = bcol ? i : ci[tj];
                }
              }
            });
          }
          // over the 16 lanes of the row (a butterfly: every lane ends with the same value)
#pragma unroll
          for (int o = 1; o < 16; o <<= 1) {
            const double v2 = __shfl_xor(rv, o);
            if constexpr (POST) {
              rv += v2;
            } else {
              const int j2 = __shfl_xor(rj, o);
              const bool take = (v2 > rv) || (v2 == rv && j2 < rj);
              rv = take ? v2 : rv;
              rj = take ? j2 : rj;
            }
          }
          if (lc == 0) {
            s_sl[wc * F2_BLK + il] = rv;
            if constexpr (!POST) s_sli[wc * F2_BLK + il] = rj;
          }
        }
      });
      // columns: over the four lane groups (rows lg + 4 r), then one slab entry per wave and column
#pragma unroll
      for (int t = 0; t < 4; ++t) {
#pragma unroll
        for (int o = 16; o <= 32; o <<= 1) {
          const double v2 = __shfl_xor(cs[t], o);
          if constexpr (POST) {
            cs[t] += v2;
          } else {
            const int i2 = __shfl_xor(ci[t], o);
            const bool take = (v2 > cs[t]) || (v2 == cs[t] && i2 < ci[t]);
            cs[t] = take ? v2 : cs[t];
            ci[t] = take ? i2 : ci[t];
          }
        }
        if (lg == 0) {
          const int jl = wc * 64 + t * 16 + lc;
          s_sl[(2 + wr) * F2_BLK + jl] = cs[t];
          if constexpr (!POST) s_sli[(2 + wr) * F2_BLK + jl] = ci[t];
        }
      }
      __syncthreads();
      // the block's two halves, in order, into the running results: threads 0..127 the rows, 128..255 the columns (an
      // entry of s_R belongs to one thread for the whole kernel; the slab is rewritten behind the next block's barriers)
      {
        const int side = tid >> 7, l = tid & (F2_BLK - 1);
        const int n = (side ? cb : rb) * F2_BLK + l;
        if (n < NP) {
          const double h0 = s_sl[(2 * side) * F2_BLK + l], h1 = s_sl[(2 * side + 1) * F2_BLK + l];
          double cur = s_R[side * NP + n];
          if constexpr (POST) {
            cur += h0;
            cur += h1;
          } else {
            int ix = s_Ri[side * NP + n];
            if (h0 > cur) { cur = h0; ix = s_sli[(2 * side) * F2_BLK + l]; }       // ascending partner index: the first best stays
            if (h1 > cur) { cur = h1; ix = s_sli[(2 * side + 1) * F2_BLK + l]; }
            s_Ri[side * NP + n] = ix;
          }
          s_R[side * NP + n] = cur;
        }
      }
    }
  }
  if constexpr (POST) {
    if (over) s_flag[0] = 1;
  }
  __syncthreads();

  // ---- last phase
  if constexpr (POST) {
    // Z in index order (every thread, the same value), status, normalisation, log_sum
    double Z = 0.0;
    for (int i = 0; i < N; ++i) Z += s_R[i];
    if (s_flag[0] != 0 || !(Z > 0.0) || !s2_finite(Z)) {
      s2_nan_rows<MODE>(a, vox, 2, 2, tid, F2_WG);
      return;
    }
    for (int n = tid; n < N; n += F2_WG) {
      a.out[(vox * 2 + 0) * N + n] = s_R[n] / Z;
      a.out[(vox * 2 + 1) * N + n] = s_R[NP + n] / Z;
    }
    if (tid == 0) {
      a.log_sum[vox] = log(Z) - a.shift[vox] / a.temp[vox];
      a.status[vox] = 0;
    }
  } else {
    const double y_sq = s_red[0];
    for (int n = tid; n < N; n += F2_WG) {
      a.out[(vox * 2 + 0) * N + n] = y_sq - s_R[n];
      a.out[(vox * 2 + 1) * N + n] = y_sq - s_R[NP + n];
      if (a.partner) {
        a.partner[(vox * 2 + 0) * N + n] = s_Ri[n];
        a.partner[(vox * 2 + 1) * N + n] = s_Ri[NP + n];
      }
    }
  }
}

// K = 1: one workgroup per voxel, one thread per atom; the unnormalised t(i) wait in the output row for Z
template <int MODE, bool WGT>
__global__ __launch_bounds__(S2_K1_WG) void mfx_soft2d_k1_kernel(S2ArgsT<WGT> a) {
  constexpr bool POST = MODE == S2_POST;
  __shared__ double s_ysq;
  __shared__ int s_over;
  const int tid = threadIdx.x;
  const int M = a.M, N = a.N;
  const size_t vox = blockIdx.x;
  if (a.vstat[5 * vox] != 0) {
    s2_nan_rows<MODE>(a, vox, 1, 5, tid, S2_K1_WG);
    return;
  }
  double Tv = 1.0, shift = 0.0;
  if constexpr (POST) {
    Tv = a.temp[vox];
    shift = a.shift[vox];
    if (!(Tv > 0.0) || !s2_finite(Tv) || !s2_finite(shift)) {
      s2_nan_rows<MODE>(a, vox, 1, 1, tid, S2_K1_WG);
      return;
    }
  }
  if constexpr (WGT) {
    if (a.wstat[vox] != 0) {
      s2_nan_rows<MODE>(a, vox, 1, 2 + a.wstat[vox], tid, S2_K1_WG);
      return;
    }
  }
  const double* __restrict__ ys = a.Y + vox * M;        // the signal; WGT: y' = s y
  const double* __restrict__ sv = nullptr;              // s (WGT)
  if constexpr (WGT) { ys = a.Ys + vox * M; sv = a.S + vox * M; }
  if (tid == 0) {
    s_over = 0;
    double s = 0.0;
    for (int m = 0; m < M; ++m) s += ys[m] * ys[m];
    s_ysq = s;
  }
  __syncthreads();
  const double y_sq = s_ysq, c0 = y_sq - shift, iT = 1.0 / Tv;
  double* row = a.out + vox * N;
  bool over = false;
  for (int n = tid; n < N; n += S2_K1_WG) {
    double a2 = 0.0, ay = 0.0;
#pragma unroll 4
    for (int m = 0; m < M; ++m) {
      const F2Rec r = a.rec[vox * M + m];
      const double sm = WGT ? sv[m] : 1.0;   // s_m (WGT)
      double d = f2_value(a.base, r, n);
      if constexpr (WGT) d = sm * d;   // fl(s_m d)
      a2 += d * d;
      ay += ys[m] * d;
    }
    const double yp = fmax(ay, 0.0);
    const double s = a2 > 0.0 ? yp * yp / a2 : 0.0;
    if constexpr (POST) {
      const double e = (s - c0) * iT;
      over |= e > S2_EXP_MAX;
      row[n] = exp(e);
    } else {
      row[n] = y_sq - s;
      if (a.partner) a.partner[vox * N + n] = -1;
    }
  }
  if constexpr (POST) {
    if (over) s_over = 1;
    __syncthreads();   // the row is written and visible to the workgroup
    double Z = 0.0;
    for (int i = 0; i < N; ++i) Z += row[i];   // index order, every thread the same value
    __syncthreads();   // every thread has read the unnormalised row before it is overwritten
    if (s_over != 0 || !(Z > 0.0) || !s2_finite(Z)) {
      s2_nan_rows<MODE>(a, vox, 1, 2, tid, S2_K1_WG);
      return;
    }
    for (int n = tid; n < N; n += S2_K1_WG) row[n] = row[n] / Z;
    if (tid == 0) {
      a.log_sum[vox] = log(Z) - shift / Tv;
      a.status[vox] = 0;
    }
  }
}

}  // namespace
