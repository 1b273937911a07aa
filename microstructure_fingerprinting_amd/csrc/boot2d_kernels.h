// boot2d_kernels.h -- the kernels of the replicate fit of 2-D protocols (include/mfx_boot2d.h): B signals per voxel on ONE
// set of directions.  What the plain kernels of fit2d_kernels.h form per row - both rotated dictionaries, their column
// norms, the cross-Gram D_0^T D_1 - belongs to the directions and is formed once per voxel here; only D^T y* and |y*|^2
// belong to a replicate.  Every sum a result depends on is formed by the arithmetic of the plain kernels, in their order,
// so a replicate's row is the row mfx_fit2d_batch_dev returns for that signal, bit for bit.  No translation unit of its own:
// boot2d.hip instantiates WGT = false, wboot2d.hip (include/mfx_wboot2d.h) WGT = true.
//
// WGT: the replicate fit on a voxel's measurement weights, the arithmetic of the WGT kernels of fit2d_kernels.h.  Once per
// voxel w2d_prep_kernel gives s = sqrt(W), sum W and the weights' status; boot2d_wsig_kernel forms y'* = fl(s_m y*_m) for every
// replicate row.  The kernels then read y'* where the unweighted ones read y*, every generated entry is fl(s_m d) (one
// multiply by the wave-uniform s_m in the statistics kernel and the exact stage; s of a chunk staged in LDS by chunk parity
// and one multiply in store_chunk of the Gram kernel, the chunk loop of mfx_fit2d_k2_kernel<true>), and the packing is the
// weighted one: MSE = min_obj / sum W, f2_r2w on the unscaled y* and W.  A voxel with unusable weights is skipped like one
// with a failing direction.  The WGT = false instantiations are the kernels as they were.
//
// boot2d_stats_kernel<K>  column statistics: one thread per atom (and side), serial over the rows in row order, one rounded
//                     multiply and one rounded add per step - phase 1 of mfx_fit2d_k2_kernel, the atom loop of
//                     mfx_fit2d_k1_kernel.  Every generated entry feeds |d|^2 once and the d.y* sums of a tile of B2_R
//                     replicates held in registers (the signals' addresses are wave-uniform).  grid (column blocks,
//                     replicate tiles, voxels); -> a2 [V][K][NP], ay [V][B][K][NP].
// boot2d_ysq_kernel<K>  |y*|^2 -> ysq [V][B], one thread per replicate row: the serial sum for K = 2, mfx_np_sumsq for K = 1, as
//                     the plain kernels (apart from the statistics kernel, whose registers belong to the replicate tile).
// boot2d_k1_kernel    K = 1, per (voxel, replicate): the tail of mfx_fit2d_k1_kernel on the stored statistics - nnls1_exact,
//                     the reference's scan-order arg-min, y_rec, f2_r2, the packing.
// boot2d_gram_kernel  K = 2, per voxel: the chunk loop of mfx_fit2d_k2_kernel<false> (fit2d_kernels.h, phase 2; its text is
//                     repeated here once and must stay the same MFMA sequence) - records staged two chunks ahead, double-
//                     buffered operand tiles, 4 x 4 v_mfma_f64_16x16x4_f64 accumulator tiles per wave - with the
//                     accumulator blocks stored to scratch G [V][NP][NP] instead of being scanned.  It needs neither the
//                     candidate list nor the column statistics in LDS.
// boot2d_k2_kernel    K = 2, per (voxel, replicate): every lane reads from G the accumulator elements the plain kernel holds
//                     for it, pair by pair as the scan meets them (a block's 128 registers per lane held the kernel to two
//                     waves per SIMD and 70 ms on the workload of DESIGN 4.23; read from L2 twice, three waves and 58 ms),
//                     and the rest of mfx_fit2d_k2_kernel<false> follows as it stands: the
//                     pair scan with its slot geometry, block order and running bound, the 4 M eps interval, the unranked
//                     hand-over of ill-conditioned pairs, the single atoms' entries, the exact stage (serial sums,
//                     nnls2_exact, strict '<' in (i1, i2) order), both family expansions, the overflow pass, the epilogue.
//                     The short list of a replicate is therefore the list the plain kernel forms for it.
// A voxel with a failing direction is skipped by every kernel (boot2d_nan_rows_kernel writes its NaN rows).
#pragma once
#include "fit2d_kernels.h"

namespace {

constexpr int B2_R = 8;          // replicates per register tile of the statistics kernel
constexpr int B2_ST_WG = 256;

struct B2Args {
  int M, N, NP, B;
  const double* base;
  const F2Rec* rec;      // [V K x M], per voxel
  const double* Y;       // [V x B x M] replicate signals
  const int* vstat;      // [V x 5], per voxel
  double* a2;            // [V][K][NP]
  double* ay;            // [V][B][K][NP]
  double* ysq;           // [V][B]
  const double* G;       // [V][NP][NP] (K = 2)
  double* params;        // [V x B x num_params]
  int num_params, maxfasc;
};
// WGT: the same and what w2d_prep_kernel and boot2d_wsig_kernel prepared of the weights
struct WB2Args {
  int M, N, NP, B;
  const double* base;
  const F2Rec* rec;      // [V K x M], per voxel
  const double* Y;       // [V x B x M] replicate signals, unscaled (the weighted R2 reads them)
  const int* vstat;      // [V x 5], per voxel
  double* a2;            // [V][K][NP]  |fl(s_m d)|^2
  double* ay;            // [V][B][K][NP]  fl(s_m d) . y'*
  double* ysq;           // [V][B]  |y'*|^2
  const double* G;       // [V][NP][NP] (K = 2)
  double* params;        // [V x B x num_params]
  int num_params, maxfasc;
  const double* Ys;      // [V x B x M] y'* = fl(s_m y*_m)  (boot2d_wsig_kernel)
  const double* W;       // [V x M] or [M]
  int64_t wstride;       // M or 0
  const double* S;       // [V x M] sqrt(W)                 (w2d_prep_kernel)
  const double* sumw;    // [V] sum_m W                     (w2d_prep_kernel)
  const int* wstat;      // [V] 0 usable, 1 a negative or non-finite weight, 2 no positive weight
};
template <bool WGT> using B2ArgsT = std::conditional_t<WGT, WB2Args, B2Args>;

// a voxel no kernel works on: a failing direction, or (WGT) unusable weights
template <class Args>
__device__ __forceinline__ bool b2_skip(const Args& a, size_t vox) {
  if constexpr (std::is_same_v<Args, WB2Args>) return a.vstat[5 * vox] != 0 || a.wstat[vox] != 0;
  else return a.vstat[5 * vox] != 0;
}
// the signals of the fit: y* or (WGT) y'*
template <class Args>
__device__ __forceinline__ const double* b2_fit_signals(const Args& a) {
  if constexpr (std::is_same_v<Args, WB2Args>) return a.Ys;
  else return a.Y;
}

// NaN rows for the replicates of a voxel with a failing direction (what fit2d_status_kernel writes per row of the plain fit)
__global__ void boot2d_nan_rows_kernel(const int* __restrict__ vstat, int64_t V, int64_t per_vox, double* __restrict__ params) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= V * per_vox) return;
  if (vstat[5 * (i / per_vox)] != 0) params[i] = __builtin_nan("");
}

// y'* = fl(s_m y*_m) for every replicate row of the chunk (WGT), one rounded multiply each; zero rows for a skipped voxel
__global__ void boot2d_wsig_kernel(const double* __restrict__ Y, const double* __restrict__ S, const int* __restrict__ vstat,
                                   const int* __restrict__ wstat, int64_t V, int B, int M, double* __restrict__ Ys) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= V * B * M) return;
  const int64_t row = i / M, v = row / B;
  const int m = (int)(i - row * M);
  Ys[i] = (vstat[5 * v] != 0 || wstat[v] != 0) ? 0.0 : S[v * M + m] * Y[i];
}

template <int K, bool WGT>
__global__ __launch_bounds__(B2_ST_WG) void boot2d_stats_kernel(B2ArgsT<WGT> a) {
  const int M = a.M, N = a.N, NP = a.NP, B = a.B;
  const size_t vox = blockIdx.z;
  if (b2_skip(a, vox)) return;
  const double* __restrict__ sv = nullptr;   // s (WGT), wave-uniform addresses
  if constexpr (WGT) sv = a.S + vox * M;
  const int b0 = blockIdx.y * B2_R;
  const int nb = min(B2_R, B - b0);
  const double* __restrict__ ys[B2_R];   // rows beyond the tile read the tile's last signal and are not stored
#pragma unroll
  for (int r = 0; r < B2_R; ++r) ys[r] = b2_fit_signals(a) + (vox * B + (size_t)(b0 + min(r, nb - 1))) * M;
  const int col = blockIdx.x * B2_ST_WG + threadIdx.x;
  if (col < K * NP) {
    const int k = col >= NP, n = col - k * NP;
    const F2Rec* __restrict__ rec = a.rec + (vox * K + k) * (size_t)M;
    double s2 = 0.0, sy[B2_R];
#pragma unroll
    for (int r = 0; r < B2_R; ++r) sy[r] = 0.0;
    if (n < N) {
#pragma unroll 2
      for (int m = 0; m < M; ++m) {
        const F2Rec rc = rec[m];
        const double d = WGT ? sv[m] * f2_value(a.base, rc, n) : f2_value(a.base, rc, n);   // WGT: fl(s_m d)
        s2 += d * d;
#pragma unroll
        for (int r = 0; r < B2_R; ++r) sy[r] += ys[r][m] * d;
      }
    }
    if (blockIdx.y == 0) a.a2[(vox * K + k) * NP + n] = s2;
#pragma unroll
    for (int r = 0; r < B2_R; ++r)
      if (r < nb) a.ay[((vox * B + b0 + r) * K + k) * NP + n] = sy[r];
  }
}

// |y*|^2 per replicate row, one thread each: the serial sum for K = 2, np.sum's pairwise order for K = 1, as the plain kernels
template <int K, bool WGT>
__global__ void boot2d_ysq_kernel(B2ArgsT<WGT> a, int64_t rows) {
  const int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= rows || b2_skip(a, (size_t)(row / a.B))) return;
  const int M = a.M;
  const double* __restrict__ y = b2_fit_signals(a) + row * M;   // WGT: |y'*|^2
  double s;
  if (K == 1) {
    s = mfx_np_sumsq(y, M);   // _1 uses np.sum(y**2)
  } else {
    s = 0.0;
    for (int m = 0; m < M; ++m) s += y[m] * y[m];
  }
  a.ysq[row] = s;
}

// K = 1: the tail of mfx_fit2d_k1_kernel<WGT>; grid = V B rows
template <bool WGT>
__global__ __launch_bounds__(F2_K1_WG) void boot2d_k1_kernel(B2ArgsT<WGT> a) {
  extern __shared__ double smem[];
  const int tid = threadIdx.x;
  const int M = a.M, N = a.N, NP = a.NP;
  const size_t row = blockIdx.x, vox = row / a.B;
  if (b2_skip(a, vox)) return;
  double* s_res = smem;                         // [WG]
  long* s_key = (long*)(s_res + F2_K1_WG);      // [WG]
  double* s_misc = (double*)(s_key + F2_K1_WG); // [8]
  double* s_yrec = s_misc + 8;                  // [M]
  const double* __restrict__ yv = a.Y + row * M;   // unscaled (WGT: only the weighted R2 reads it)
  const double* __restrict__ va2 = a.a2 + vox * NP;
  const double* __restrict__ vay = a.ay + row * NP;
  const F2Rec* __restrict__ rec = a.rec + vox * M;
  const double y_sq = a.ysq[row];
  // thread-local best in the reference's scan order; key < 0 = the reference's initial state
  double bres = y_sq, bw = 0.0;
  long bkey = -1;
  for (int i = tid; i < N; i += F2_K1_WG) {
    double w, r;
    nnls1_exact(y_sq, va2[i], vay[i], w, r);
    if (r < bres || (r == bres && bkey >= 0 && i < bkey)) { bres = r; bkey = i; bw = w; }
  }
  s_res[tid] = bres;
  s_key[tid] = bkey;
  __syncthreads();
  for (int o = F2_K1_WG / 2; o > 0; o >>= 1) {
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
    for (int m = lane; m < M; m += 64) s_yrec[m] = w * f2_value(a.base, rec[m], ia);
    double r2;
    if constexpr (WGT) r2 = f2_r2w(yv, a.W + vox * a.wstride, s_yrec, M, lane);
    else r2 = f2_r2(yv, s_yrec, M, lane);
    if (lane == 0) {   // params packing, mf.py:420-450
      double* out = a.params + row * a.num_params;
      out[0] = w;
      out[1] = (fabs(w) > 0) ? w / w : w;
      out[1 + a.maxfasc] = (double)ia;
      if constexpr (WGT) out[a.num_params - 2] = res / a.sumw[vox];   // MSE = min_obj / sum W
      else out[a.num_params - 2] = res / M;
      out[a.num_params - 1] = r2;
    }
  }
}

size_t b2_gram_lds_bytes(bool wgt = false) {   // wgt: plus the staged s of two chunks
  return ((size_t)2 * F2_NT * F2_TS + (wgt ? 2 * F2_MC : 0)) * sizeof(double) + F2_REC * sizeof(F2Rec);
}

// K = 2, per voxel: the cross-Gram of the padded dictionaries.  The chunk loop is that of mfx_fit2d_k2_kernel<WGT>
// (fit2d_kernels.h, "phase 2"): keep the two texts in step.  WGT: s of a chunk's rows staged beside the records, one
// multiply in store_chunk.
template <bool WGT>
__global__ __launch_bounds__(F2_WG, 2) void boot2d_gram_kernel(B2ArgsT<WGT> a, double* __restrict__ G) {
  extern __shared__ double smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lg = lane >> 4, lc = lane & 15;
  const int wr = wave >> 1, wc = wave & 1;
  const int M = a.M, N = a.N, NP = a.NP;
  const int ntiles = NP >> 4;
  const size_t vox = blockIdx.x;
  if (b2_skip(a, vox)) return;
  double* sT = smem;                                      // [2][F2_NT][F2_TS]: tiles 0..7 the D_0 block, 8..15 the D_1 block
  double* s_sc = sT + 2 * F2_NT * F2_TS;                  // [2][F2_MC] staged s of two chunks (WGT)
  F2Rec* s_rec = (F2Rec*)(s_sc + (WGT ? 2 * F2_MC : 0));  // [F2_REC] staged records of two chunks
  const double* __restrict__ sv = nullptr;                // s (WGT)
  if constexpr (WGT) sv = a.S + vox * M;
  const size_t rec0 = 2 * vox * M;
  double* __restrict__ Gv = G + vox * (size_t)NP * NP;

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
          double v = r2_value(s_rec[q0 + r].o, s_rec[q0 + r].s, va[r], s_rec[q0 + r].dx, vb[r]);
          if constexpr (WGT) v = s_sc[(ch & 1) * F2_MC + r] * v;   // fl(s_m d)
          dst[r * 16] = gn < N ? v : 0.0;   // atoms beyond the dictionary: zero columns
        }
      };
      d4 acc[4][4];
#pragma unroll
      for (int ti = 0; ti < 4; ++ti)
#pragma unroll
        for (int tj = 0; tj < 4; ++tj) acc[ti][tj] = d4{0, 0, 0, 0};

      stage_rec(0);
      stage_rec(1);
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

      // the block's accumulator tiles, in the scan's geometry: row i = .. + lg + 4 r, column j = .. + lc; i, j < NP
#pragma unroll
      for (int ti = 0; ti < 4; ++ti)
#pragma unroll
        for (int tj = 0; tj < 4; ++tj)
          if (ti < nta && tj < ntb) {
            const int j = cb * F2_BLK + wc * 64 + tj * 16 + lc;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int i = rb * F2_BLK + wr * 64 + ti * 16 + lg + 4 * r;
              Gv[(size_t)i * NP + j] = acc[ti][tj][r];
            }
          }
      __syncthreads();
    }
  }
}

// LDS of the scan kernel: the column statistics, the scratch words, the short list, the reduction scratch and y_rec [M]
size_t b2_k2_lds_bytes(int NP, int M) {
  return ((size_t)4 * NP + 32 + 48 + (size_t)M) * sizeof(double) + F2_MAXC * sizeof(Cand) + 4 * sizeof(int);
}

// K = 2, per (voxel, replicate): mfx_fit2d_k2_kernel<WGT> behind its chunk loop, on the stored statistics and Gram
template <bool WGT>
__global__ __launch_bounds__(F2_WG) void boot2d_k2_kernel(B2ArgsT<WGT> a) {
  extern __shared__ double smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lg = lane >> 4, lc = lane & 15;
  const int wr = wave >> 1, wc = wave & 1;
  const int M = a.M, N = a.N, NP = a.NP;
  const int ntiles = NP >> 4;
  const size_t row = blockIdx.x, vox = row / a.B;
  if (b2_skip(a, vox)) return;

  double2* s_st = (double2*)smem;                // [2][NP] column statistics {|d|^2, d.y*} of D_0, then of D_1
  double* s_red = (double*)(s_st + 2 * NP);      // [32] scratch
  double* s_wk = s_red + 32;                     // [48 + M] reduction scratch, winner, y_rec
  Cand* s_cand = (Cand*)(s_wk + 48 + M);         // [F2_MAXC]
  int* s_cnt = (int*)(s_cand + F2_MAXC);         // [4]

  const double* __restrict__ yv = a.Y + row * M;              // unscaled (WGT: only the weighted R2 reads it)
  const double* __restrict__ ys = b2_fit_signals(a) + row * M;   // the signal of the fit (WGT: y'*)
  const double* __restrict__ sv = nullptr;                    // s (WGT)
  if constexpr (WGT) sv = a.S + vox * M;
  const double* __restrict__ Gv = a.G + vox * (size_t)NP * NP;
  const size_t rec0 = 2 * vox * M;               // records of direction k: + k M
  auto elem_raw = [&](int k, int m, int n) -> double { return f2_value(a.base, a.rec[rec0 + (size_t)k * M + m], n); };
  auto elem = [&](int k, int m, int n) -> double {   // WGT: fl(s_m d)
    if constexpr (WGT) return sv[m] * elem_raw(k, m, n);
    else return elem_raw(k, m, n);
  };

  // ---- the stored statistics; the best single-atom score of either dictionary is the scan's first bound
  if (tid == 0) { s_cnt[0] = 0; s_red[31] = a.ysq[row]; }
  double my_s = 0.0;
  for (int col = tid; col < 2 * NP; col += F2_WG) {
    const int k = col >= NP, n = col - k * NP;
    const double a2 = a.a2[(vox * 2 + k) * NP + n], ay = a.ay[(row * 2 + k) * NP + n];
    s_st[col] = double2{a2, ay};
    const double s = (n < N && ay > 0.0) ? (ay * ay) / a2 : 0.0;
    my_s = fmax(my_s, s);   // a maximum: exact in any order
  }
  my_s = wave_max(my_s);
  if (lane == 0) s_red[wave] = my_s;
  __syncthreads();
  {
    double best1 = s_red[0];
    for (int w = 1; w < F2_NW; ++w) best1 = fmax(best1, s_red[w]);
    __syncthreads();
    if (tid == 0) s_red[30] = best1;
  }
  __syncthreads();

  // ---- the pair scan, block by block in the plain kernel's order, the accumulator elements read from G
  const int nblk = (NP + F2_BLK - 1) / F2_BLK;
  for (int rb = 0; rb < nblk; ++rb) {
    const int nta = min(max(ntiles - (rb * 8 + wr * 4), 0), 4);
    for (int cb = 0; cb < nblk; ++cb) {
      const int ntb = min(max(ntiles - (cb * 8 + wc * 4), 0), 4);
      double llb = 0.0;
      const double eps_abs = 1e-9 * s_red[31];
      const double a12_rel = fmax(MFX_A12_REL, 4.0 * M * 2.220446049250313e-16);
      double glb_run = s_red[30];
#pragma unroll 1
      for (int pass = 0; pass < 2; ++pass) {
        mfx_static_for<0, 4>([&](auto tic) {
          constexpr int ti = decltype(tic)::value;
          if (ti < nta) {
#pragma unroll 1
            for (int r = 0; r < 4; ++r) {
              const int i = rb * F2_BLK + wr * 64 + ti * 16 + lg + 4 * r;
              const double A11 = s_st[i].x, Y1 = s_st[i].y;
              double p = 0.0, q = 1.0;
              int bj = -1;
#pragma unroll 1
              for (int tj = 0; tj < ntb; ++tj) {
                const int j = cb * F2_BLK + wc * 64 + tj * 16 + lc;
                const double A22 = s_st[NP + j].x, Y2 = s_st[NP + j].y;
                const double A12 = Gv[(size_t)i * NP + j];   // the accumulator element (ti, tj, r) of this lane; i, j < NP
                const double d1 = fma(-A12, Y2, A22 * Y1);
                const double d2 = fma(-A12, Y1, A11 * Y2);
                const double pd = A11 * A22;
                const double Det = fma(-A12, A12, pd);
                const double num = fma(Y2, d2, Y1 * d1);
                const bool pos = (d1 > 0.0) & (d2 > 0.0) & (j < N) & (i < N);
                const bool wellc = Det > MFX_DET_REL * pd;
                if (pass == 0 && pos && !wellc) {
                  const int slot = atomicAdd(&s_cnt[0], 1);
                  if (slot < F2_MAXC) { s_cand[slot].score = 1e300; s_cand[slot].i = i; s_cand[slot].j = j; }
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
                  if (slot < F2_MAXC) { s_cand[slot].score = sc + er + eps_abs; s_cand[slot].i = i; s_cand[slot].j = bj; }   // upper bound
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
          for (int w = 1; w < F2_NW; ++w) rlb = fmax(rlb, s_red[w]);
          glb_run = fmax(glb_run, rlb);
        }
      }
      __syncthreads();
      if (tid == 0) s_red[30] = glb_run;
      __syncthreads();   // (the plain kernel's chunk loop has barriers between this store and the next block's read)
    }
  }

  // every single atom of either dictionary whose score reaches the final bound (see mfx_fit2d_k2_kernel)
  __syncthreads();
  {
    const double thr = s_red[30], eps_abs = 1e-9 * s_red[31];
    for (int col = tid; col < 2 * NP; col += F2_WG) {
      const int k = col >= NP, n = col - k * NP;
      const double a2 = s_st[col].x, ay = s_st[col].y;
      const double s = (n < N && ay > 0.0) ? (ay * ay) / a2 : 0.0;
      if (s > 0.0 && s + eps_abs >= thr) {
        const int slot = atomicAdd(&s_cnt[0], 1);
        if (slot < F2_MAXC) { s_cand[slot].score = s + eps_abs; s_cand[slot].i = k ? 0 : n; s_cand[slot].j = (k ? n : 0) | F2_SINGLE; }
      }
    }
  }

  // ---- the exact stage (reference arithmetic and order), as mfx_fit2d_k2_kernel's phase 3
  __syncthreads();
  const double y_sq = s_red[31], glb_run = s_red[30];
  auto exact_pair = [&](int i, int j, double& w0, double& w1, double& res) {
    double a11 = 0.0, a22 = 0.0, a12 = 0.0, y1 = 0.0, y2 = 0.0;
#pragma unroll 4
    for (int m = 0; m < M; ++m) {
      const double d1 = elem(0, m, i), d2 = elem(1, m, j), ym = ys[m];
      a11 += d1 * d1;
      a22 += d2 * d2;
      a12 += d1 * d2;
      y1 += ym * d1;
      y2 += ym * d2;
    }
    nnls2_exact(y_sq, a11, a12, a22, y1, y2, w0, w1, res);
  };
  double* s_rres = s_wk;                 // [8] per-wave partials
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
      double br = s_win[0], b0 = s_win[1], b1 = s_win[2];
      long bi = ((long*)s_win)[3];
      for (int w = 0; w < F2_NW; ++w) {
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
  const int ncand = nappend > F2_MAXC ? F2_MAXC : nappend;
  __syncthreads();
  if (tid == 0) {    // mf_utils.py:327, 382: start from min_obj = y_sq at pair (0,0) with w = 0, strict '<'
    s_win[0] = y_sq; s_win[1] = 0.0; s_win[2] = 0.0; ((long*)s_win)[3] = -1;
  }
  {
    double res = INFINITY, w0 = 0.0, w1 = 0.0;
    long idx = -1;
    if (nappend <= F2_MAXC) {
      const int NJ = (N + 15) >> 4;
      for (int q = tid; q < ncand * NJ; q += F2_WG) {
        const int c = q / NJ, u = q - c * NJ;
        if (!(s_cand[c].score >= glb_run)) continue;
        const int ci = s_cand[c].i, cj = s_cand[c].j & ~F2_SINGLE;
        const bool single = (s_cand[c].j & F2_SINGLE) != 0;
        const int jj = single ? cj : (cj & 15) + 16 * u;
        if ((single && u > 0) || jj >= N) continue;
        double r, u0, u1;
        exact_pair(ci, jj, u0, u1, r);
        const long ix = (long)ci * N + jj;
        if (r < res || (r == res && ix < idx)) { res = r; idx = ix; w0 = u0; w1 = u1; }
      }
    } else {
      // the short list overflowed (massive near-ties): last resort, every pair through the reference arithmetic
      const long npairs = (long)N * N;
      for (long pr = tid; pr < npairs; pr += F2_WG) {
        double r, u0, u1;
        exact_pair((int)(pr / N), (int)(pr % N), u0, u1, r);
        if (r < res || (r == res && pr < idx)) { res = r; idx = pr; w0 = u0; w1 = u1; }
      }
    }
    block_argmin(res, idx, w0, w1);
  }
  // near-zero second weight: the whole family of the active atom exactly (see mfx_fit2d_k2_kernel)
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
    for (int n = tid; n < N; n += F2_WG) {
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
    // params packing, mf.py:420-450
    const double M0 = w0 + w1;
    const double nu0 = (fabs(M0) > 0) ? w0 / M0 : w0;
    const double nu1 = (fabs(M0) > 0) ? w1 / M0 : w1;
    double* s_yrec = s_win + 8;   // [M]: s_wk holds 48 + M doubles
    for (int m = lane; m < M; m += 64) s_yrec[m] = elem_raw(0, m, bi) * w0 + elem_raw(1, m, bjx) * w1;   // unscaled columns
    double r2;
    if constexpr (WGT) r2 = f2_r2w(yv, a.W + vox * a.wstride, s_yrec, M, lane);
    else r2 = f2_r2(yv, s_yrec, M, lane);
    double* out = a.params + row * a.num_params;
    if (lane == 0) {
      out[0] = M0;
      out[1] = nu0;
      out[2] = nu1;
      out[1 + a.maxfasc] = (double)bi;
      out[2 + a.maxfasc] = (double)bjx;
      if constexpr (WGT) out[a.num_params - 2] = best / a.sumw[vox];   // MSE = min_obj / sum W
      else out[a.num_params - 2] = best / M;
      out[a.num_params - 1] = r2;
    }
  }
}

}  // namespace
