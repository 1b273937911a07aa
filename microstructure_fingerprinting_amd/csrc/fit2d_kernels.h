// fit2d_kernels.h -- the kernels that fit voxels of a 2-D protocol, without measurement weights (fit2d.hip instantiates
// WGT = false) and with them (w2d.hip, WGT = true).  No translation unit of its own.
//
// WGT: the reference chain on rows scaled by s = sqrt(W) (include/mfx_w2d.h).  Every dictionary entry is fl(s_m * d) with d
// the unweighted entry, y' = s y, MSE = min_obj / sum W and the weighted R2 on the unscaled columns; s, y' and sum W come
// from w2d_prep_kernel (below) through W2Args.  For W = 1 the weighted kernels see the unweighted columns (s = 1) and
// return the unweighted rows bit for bit.  What WGT adds to a kernel is listed at its head; everything else - the chunk
// loop, the scan, the 4 M eps interval, the unranked hand-over, the family expansion, the overflow pass - is one text.
//
// mfx_fit2d_k2_kernel<WGT>   K = 2, no extra column: one 4-wave workgroup per voxel, the phases of fit_k2.hip.
//   phase 1  column statistics |d|^2, d.y of both dictionaries, one thread per atom, serial over the rows (the sums the
//            exact stage forms: only the cross terms differ between ranking and exact arithmetic).
//   phase 2  the cross-Gram D_0^T D_1 in 128 x 128 blocks on v_mfma_f64_16x16x4_f64.  The fused kernels of fit_k2.hip
//            hold a column block over ALL rows in registers and stop at 560 rows; here the block is ACCUMULATED over the
//            rows in chunks of 8: the 16 accumulator tiles of a wave (64 x 64 atoms, 128 VGPRs) persist across the
//            chunks, and both operands of a chunk (8 rows x 128 atoms of either dictionary) are generated into LDS,
//            double buffered - the table loads of the next chunk are issued before the MFMAs of the current one and
//            turned into entries behind them.  The rows' records are staged in LDS two chunks ahead (16 threads, one
//            record each), so the loop reads nothing but table values from memory and has no per-row branch.  Nothing
//            depends on M beyond R2_MAX_ROWS.  After the last chunk the 2x2 NNLS closed form of mf_utils.py:341-379 is
//            scanned on the accumulator tiles with fit_k2.hip's un-normalised scan (division-free); a slot - one row of
//            the lane over the lane's columns of the block - keeps its best pair and is short-listed by interval; pairs
//            with 1 - c^2 <= MFX_DET_REL and two positive weights go to the short list unranked.  The register budget
//            is 256 per lane (two workgroups per CU where LDS allows): accumulators in arch VGPRs, no spill.
//   phase 3  fit_k2.hip's exact stage: the slot row of every short-listed candidate through serial sums in the
//            reference's row order and nnls2_exact (the reference's branch order), strict '<' in (i1, i2) order, the
//            family expansion for a vanishing second weight, the params row.
//   WGT      the weights' status beside the directions'; s_m of a chunk's rows staged in LDS beside the rows' records, two
//            chunks ahead, by 8 threads that are idle in stage_rec, and store_chunk's multiply by it; the serial sums of
//            phase 1 and the exact stage over fl(s_m d) and y'; the epilogue.
// mfx_fit2d_k1_kernel<WGT>   K = 1, no extra column: one thread per atom, serial statistics, the reference's _1 rule
//                            (WGT: on fl(s_m d) and y', |y'|^2 in np.sum's pairwise order).
// fit2d_mat_kernel<WGT>      every other class: the dictionaries (WGT: scaled) materialised in voxel chunks for the explicit
//                            solver of mfx_api.hip.
// A voxel with a failing direction is skipped by every kernel (fit2d_status_kernel wrote its NaN row and record).
#pragma once
#include "fit2d_shared.h"   // F2Rec, fit2d_rec_kernel, f2_value, W2Args, the Gram block geometry
#include "fit_small.hip"    // mfx_np_sumsq

#include <type_traits>

namespace {

constexpr int F2_MAXC = 512;               // short-list entries
constexpr int F2_SINGLE = 1 << 30;         // in Cand::j: a single atom's entry - the pair itself, no slot row
constexpr size_t F2_LDS_MAX = 160 * 1024;
constexpr int F2_K1_WG = 256;

struct F2Args {
  int M, N;
  const double* base;
  const F2Rec* rec;    // [B x M]
  const double* Y;     // [V x M]
  const int* vstat;    // [V x 5]
  double* params;      // [V x num_params]
  int num_params, maxfasc;
};
template <bool WGT> using F2ArgsT = std::conditional_t<WGT, W2Args, F2Args>;

// the unscaled entry (record i, atom n)
template <class Args>
__device__ __forceinline__ double f2_elem(const Args& a, size_t i, int n) {
  const F2Rec r = a.rec[i];
  return f2_value(a.base, r, n);
}

// the voxels' dictionaries [nv][M][Ntot]: K blocks of N columns, then the CSF column (WGT: every row times s_m); grid
// (voxel, block of 8 rows)
template <bool WGT>
__global__ __launch_bounds__(256) void fit2d_mat_kernel(F2ArgsT<WGT> a, const int* __restrict__ ok, int64_t v0, int K, int has_csf,
                                                       const double* __restrict__ xc, double* __restrict__ A) {
  const int64_t v = v0 + blockIdx.x;
  if (!ok[v]) return;
  const int M = a.M, N = a.N, Ntot = K * N + has_csf;
  const double* __restrict__ sv = nullptr;   // s (WGT)
  if constexpr (WGT) sv = a.S + (size_t)v * M;
  for (int r = 0; r < 8; ++r) {
    const int m = blockIdx.y * 8 + r;
    if (m >= M) break;
    const double s = WGT ? sv[m] : 1.0;
    double* dst = A + ((size_t)blockIdx.x * M + m) * Ntot;
    for (int k = 0; k < K; ++k) {
      const size_t i = (size_t)(v * K + k) * M + m;
      for (int n = threadIdx.x; n < N; n += 256) {
        const double d = f2_elem(a, i, n);
        dst[k * N + n] = WGT ? s * d : d;
      }
    }
    if (has_csf && threadIdx.x == 0) dst[K * N] = WGT ? s * xc[m] : xc[m];
  }
}

// R^2 = corrcoef(y, y_rec)[0, 1]^2 (mf.py:449-450) by the 64 lanes of one wave; y_rec [M] in LDS
__device__ __forceinline__ double f2_r2(const double* __restrict__ yv, const double* s_yrec, int M, int lane) {
  double sy = 0.0, sr = 0.0;
  for (int m = lane; m < M; m += 64) { sy += yv[m]; sr += s_yrec[m]; }
  sy = wave_sum(sy) / M;
  sr = wave_sum(sr) / M;
  double cyy = 0.0, crr = 0.0, cyr = 0.0;
  for (int m = lane; m < M; m += 64) {
    const double da = yv[m] - sy, db = s_yrec[m] - sr;
    cyy += da * da;
    crr += db * db;
    cyr += da * db;
  }
  cyy = wave_sum(cyy);
  crr = wave_sum(crr);
  cyr = wave_sum(cyr);
  double r2 = 0.0;
  if (M > 1 && cyy > 0.0 && crr > 0.0) {
    const double f = (double)(M - 1);
    double r = (cyr / f) / sqrt(cyy / f) / sqrt(crr / f);
    r = r > 1.0 ? 1.0 : (r < -1.0 ? -1.0 : r);
    r2 = r * r;
  }
  return r2;
}

// Squared weighted Pearson correlation of y and y_rec by the 64 lanes of one wave (weights wv, weighted means).  The
// common normaliser of the three moments cancels; it is n_pos - 1 (n_pos the number of positive weights), so that a 0/1
// mask gives np.corrcoef's arithmetic on the kept rows and W = 1 that of f2_r2, operation for operation.
// 0 with fewer than two positive weights or a vanishing weighted variance.
__device__ __forceinline__ double f2_r2w(const double* __restrict__ yv, const double* __restrict__ wv, const double* s_yrec, int M,
                                         int lane) {
  double sw = 0.0, sy = 0.0, sr = 0.0, np = 0.0;
  for (int m = lane; m < M; m += 64) {
    const double w = wv[m];
    sw += w;
    sy += w * yv[m];
    sr += w * s_yrec[m];
    np += (w > 0.0) ? 1.0 : 0.0;
  }
  sw = wave_sum(sw);
  sy = wave_sum(sy) / sw;
  sr = wave_sum(sr) / sw;
  np = wave_sum(np);
  double cyy = 0.0, crr = 0.0, cyr = 0.0;
  for (int m = lane; m < M; m += 64) {
    const double w = wv[m], da = yv[m] - sy, db = s_yrec[m] - sr;
    cyy += w * (da * da);
    crr += w * (db * db);
    cyr += w * (da * db);
  }
  cyy = wave_sum(cyy);
  crr = wave_sum(crr);
  cyr = wave_sum(cyr);
  double r2 = 0.0;
  if (np > 1.5 && cyy > 0.0 && crr > 0.0) {
    const double f = np - 1.0;
    double r = (cyr / f) / sqrt(cyy / f) / sqrt(crr / f);
    r = r > 1.0 ? 1.0 : (r < -1.0 ? -1.0 : r);
    r2 = r * r;
  }
  return r2;
}

// One wave per voxel: the weights are tested over the whole voxel first (the result is uniform), then s, y' and sum W are
// written.  A voxel with a failing direction is left alone (weight status 0: the direction is reported); a voxel with
// unusable weights gets zeros in s and y' (nobody reads them), its code, and with params its NaN row.  ok (may be null):
// 1 where the fit runs.  Y and Ys null: no y' (the replicate fit of boot2d_kernels.h forms y'* per replicate row).
__global__ __launch_bounds__(64) void w2d_prep_kernel(const double* __restrict__ Y, const double* __restrict__ W, int64_t wstride, int M,
                                                      const int* __restrict__ vstat, double* __restrict__ S, double* __restrict__ Ys,
                                                      double* __restrict__ sumw, int* __restrict__ wstat, int* __restrict__ ok,
                                                      double* __restrict__ params, int np) {
  const size_t v = blockIdx.x;
  const int lane = threadIdx.x;
  if (vstat[5 * v] != 0) {
    if (lane == 0) { wstat[v] = 0; sumw[v] = 0.0; if (ok) ok[v] = 0; }
    return;
  }
  const double* __restrict__ wv = W + v * wstride;
  const double* __restrict__ yv = Y + v * M;
  int bad = 0, pos = 0;
  double sw = 0.0;
  for (int m = lane; m < M; m += 64) {
    const double w = wv[m];
    bad |= !(w >= 0.0) || !(w <= 1.79769313486231570815e308);
    pos |= w > 0.0;
    sw += w;
  }
  bad = __any(bad);
  pos = __any(pos);
  sw = wave_sum(sw);
  const int code = bad ? 1 : (pos ? 0 : 2);
  for (int m = lane; m < M; m += 64) {
    const double s = code == 0 ? sqrt(wv[m]) : 0.0;
    S[v * M + m] = s;
    if (Ys) Ys[v * M + m] = s * yv[m];
  }
  if (params && code != 0)
    for (int q = lane; q < np; q += 64) params[v * np + q] = __builtin_nan("");
  if (lane == 0) { wstat[v] = code; sumw[v] = sw; if (ok) ok[v] = code == 0; }
}

// wgt: plus the staged s of two chunks
size_t f2_lds_bytes(int NP, bool wgt) {
  return ((size_t)2 * F2_NT * F2_TS + 4 * (size_t)NP + 32 + (wgt ? 2 * F2_MC : 0)) * sizeof(double) + F2_REC * sizeof(F2Rec) +
         F2_MAXC * sizeof(Cand) + 4 * sizeof(int);
}

int f2_max_atoms_k2(bool wgt) {
  int n = 0;
  while (n < (1 << 20) && f2_lds_bytes(n + 16, wgt) <= F2_LDS_MAX) n += 16;
  return n;
}

template <bool WGT>
__global__ __launch_bounds__(F2_WG, 2) void mfx_fit2d_k2_kernel(F2ArgsT<WGT> a) {
  extern __shared__ double smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lg = lane >> 4, lc = lane & 15;
  const int wr = wave >> 1, wc = wave & 1;
  const int M = a.M, N = a.N;
  const int NP = (N + 15) & ~15;   // atoms padded to a multiple of 16 (padded atoms are zero columns)
  const int ntiles = NP >> 4;
  const size_t vox = blockIdx.x;
  // a failing direction, unusable weights: the row is written by fit2d_status_kernel / w2d_prep_kernel (workgroup-uniform)
  if constexpr (WGT) {
    if (a.vstat[5 * vox] != 0 || a.wstat[vox] != 0) return;
  } else {
    if (a.vstat[5 * vox] != 0) return;
  }

  // ---- LDS carve-up (f2_lds_bytes mirrors it)
  double* sT = smem;                             // [2][F2_NT][F2_TS]: tiles 0..7 the D_0 block, 8..15 the D_1 block
  double2* s_st = (double2*)(sT + 2 * F2_NT * F2_TS);   // [2][NP] column statistics {|d|^2, d.y} of D_0, then of D_1
  double* s_red = (double*)(s_st + 2 * NP);      // [32] scratch
  double* s_sc = s_red + 32;                     // [2][F2_MC] staged s of two chunks (WGT)
  F2Rec* s_rec = (F2Rec*)(s_sc + (WGT ? 2 * F2_MC : 0));   // [F2_REC] staged records of two chunks
  Cand* s_cand = (Cand*)(s_rec + F2_REC);        // [F2_MAXC]
  int* s_cnt = (int*)(s_cand + F2_MAXC);         // [4]

  const double* __restrict__ yv = a.Y + vox * M;          // unscaled (WGT: only the weighted R2 reads it)
  const double* __restrict__ ys = yv;                     // y' = s y, the signal of the fit
  const double* __restrict__ sv = nullptr;                // s (WGT)
  const double* __restrict__ wv = nullptr;                // W (WGT)
  if constexpr (WGT) { ys = a.Ys + vox * M; sv = a.S + vox * M; wv = a.W + vox * a.wstride; }
  const size_t rec0 = 2 * vox * M;               // records of direction k: + k M
  auto elem_raw = [&](int k, int m, int n) -> double { return f2_elem(a, rec0 + (size_t)k * M + m, n); };
  auto elem = [&](int k, int m, int n) -> double {   // WGT: fl(s_m d)
    if constexpr (WGT) return sv[m] * elem_raw(k, m, n);
    else return elem_raw(k, m, n);
  };

  // ---- phase 1: ||y'||^2 and the column statistics, sequential over the measurements (mf_utils.py:307-325)
  if (tid == 0) {
    s_cnt[0] = 0;
    double s = 0.0;
    for (int m = 0; m < M; ++m) s += ys[m] * ys[m];
    s_red[31] = s;
  }
  double my_s[2] = {0.0, 0.0};
  int my_n[2] = {0, 0};
  for (int col = tid; col < 2 * NP; col += F2_WG) {
    const int k = col >= NP, n = col - k * NP;
    double a2 = 0.0, ay = 0.0;
    if (n < N) {
#pragma unroll 4
      for (int m = 0; m < M; ++m) {
        const double d = elem(k, m, n);
        a2 += d * d;
        ay += ys[m] * d;
      }
    }
    s_st[col] = double2{a2, ay};
    const double s = (n < N && ay > 0.0) ? (ay * ay) / a2 : 0.0;
    if (s > my_s[k]) { my_s[k] = s; my_n[k] = n; }   // columns are visited in increasing n per thread
  }
  __syncthreads();
  // ||y||^2 stays in s_red[31] and the running best lower bound on the score in s_red[30] (one value for the workgroup):
  // they live through the whole of phase 2, whose registers belong to the accumulators
  {
    // best single-atom score of either dictionary: no pair below it matters (a pair whose optimum has one active atom,
    // mf_utils.py:357-379, scores as that atom).  The single atoms themselves join the candidates behind phase 2.
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
      for (int w = 1; w < F2_NW; ++w) {
        const double s2 = s_bs[k * 8 + w];
        const int n2 = s_bn[k * 8 + w];
        if (s2 > s || (s2 == s && n2 < n)) { s = s2; n = n2; }
      }
      best1 = fmax(best1, s);
    }
    __syncthreads();   // (s_red[0..23] read by everybody)
    if (tid == 0) s_red[30] = best1;
  }
  __syncthreads();

  // ---- phase 2: cross-Gram blocks accumulated over the rows in chunks, then the pair scan
  const int nblk = (NP + F2_BLK - 1) / F2_BLK;
  const int nchunks = (M + F2_MC - 1) / F2_MC;
  // generation: thread -> one atom of one side (waves 0, 1: D_0; waves 2, 3: D_1), the rows of the chunk.  The rows'
  // records are staged in LDS two chunks ahead by 2 F2_MC threads (one per side and row), by chunk parity: every lane reads
  // them at one address, no record is read from memory inside the loop.
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

      if constexpr (WGT) {
        // The first two chunks are staged through an index the compiler cannot see through: with the literal 0 and 1 it
        // hoists the staging threads' two addresses of s out of the block loops and keeps them in registers through
        // the chunk loop, which the posterior's budget (255 VGPRs) does not hold.  The unweighted kernels stage no s and
        // keep the literals: their object code is what it was before the weighted forms joined them.
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
            // tiles beyond the dictionary are zero columns and run along: the workgroup waits for its fullest wave at
            // the barrier anyway
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

      // pair scan of the accumulator tiles, fit_k2.hip's un-normalised scan (mf_utils.py:348-356 ranked here; the
      // single-active cases are the two single-atom representatives).  A slot is one row of the lane (16 per lane) over
      // this block's columns of the lane; its best pair is short-listed by interval against the best lower bound so far.
      // The slots are walked one at a time, twice - lower bounds first, the list after the workgroup's bound is known -
      // rather than held in registers side by side: beside a block's MFMAs (M / 4 x 16 per wave) the scan is small.
      // pass 0: the slots' lower bounds (and the ill-conditioned pairs); pass 1: the list
      double llb = 0.0;
      const double eps_abs = 1e-9 * s_red[31];
      // an MFMA-summed cross term against the serial sum: at most M eps |d1||d2| whatever the order; 4 x that, not below fit_k2's
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
      if (tid == 0) s_red[30] = glb_run;   // (read again behind the next block's barriers)
    }
  }

  // The single atoms stand for every pair whose optimum has one active atom; phase 3 expands the winner's family exactly.
  // The best one alone does not stand for the others: of two near-duplicate atoms whose scores differ by rounding the
  // reference takes the one whose ROUNDED residual is smaller and, when those tie, the first - not the one that scores
  // higher.  EVERY atom of either dictionary whose score reaches the final bound joins the list, by the rule of every
  // other entry; none does once a pair beats them all by more than the window.
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

  // ---- phase 3: exact re-evaluation of the short list (reference arithmetic and order), as fit_k2.hip
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
  __syncthreads();   // everyone has read s_cnt / is done with the operand buffers
  if (tid == 0) {    // mf_utils.py:327, 382: start from min_obj = y_sq at pair (0,0) with w = 0, strict '<'
    s_win[0] = y_sq; s_win[1] = 0.0; s_win[2] = 0.0; ((long*)s_win)[3] = -1;
  }
  {
    double res = INFINITY, w0 = 0.0, w1 = 0.0;
    long idx = -1;
    if (nappend <= F2_MAXC) {
      // A scan candidate is the best pair of its slot - row i, the columns j = lc (mod 16) of one wave's half of one
      // column block; a second pair of the slot within rounding distance of the optimum was never listed.  The whole
      // row i over the columns j = lc (mod 16) (a superset of the slot) is therefore evaluated exactly for every listed
      // candidate that still reaches the final lower bound.  A single atom's entry (F2_SINGLE) is itself only.
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
    // y_rec = A[:, tot] @ w
    double* s_yrec = s_win + 8;   // [M] scratch inside the idle operand buffers (2 F2_NT F2_TS = 4608 doubles >= R2_MAX_ROWS + 48)
    for (int m = lane; m < M; m += 64) s_yrec[m] = elem_raw(0, m, bi) * w0 + elem_raw(1, m, bjx) * w1;   // unscaled columns
    double r2;
    if constexpr (WGT) r2 = f2_r2w(yv, wv, s_yrec, M, lane);
    else r2 = f2_r2(yv, s_yrec, M, lane);
    double* out = a.params + vox * a.num_params;
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
static_assert(2 * F2_NT * F2_TS >= R2_MAX_ROWS + 48, "y_rec scratch of the K = 2 kernel");

// K = 1, no extra column: one workgroup per voxel, one thread per atom; solve_exhaustive_posweights_1 (mf_utils.py:225-286),
// WGT: on (s D, y')
template <bool WGT>
__global__ __launch_bounds__(F2_K1_WG) void mfx_fit2d_k1_kernel(F2ArgsT<WGT> a) {
  extern __shared__ double smem[];
  const int tid = threadIdx.x;
  const int M = a.M, N = a.N;
  const size_t vox = blockIdx.x;
  if constexpr (WGT) {
    if (a.vstat[5 * vox] != 0 || a.wstat[vox] != 0) return;
  } else {
    if (a.vstat[5 * vox] != 0) return;
  }
  double* s_res = smem;                         // [WG]
  long* s_key = (long*)(s_res + F2_K1_WG);      // [WG]
  double* s_misc = (double*)(s_key + F2_K1_WG); // [8]
  double* s_yrec = s_misc + 8;                  // [M]
  const double* __restrict__ yv = a.Y + vox * M;
  const double* __restrict__ ys = yv;           // y' = s y
  const double* __restrict__ sv = nullptr;      // s (WGT)
  const double* __restrict__ wv = nullptr;      // W (WGT)
  if constexpr (WGT) { ys = a.Ys + vox * M; sv = a.S + vox * M; wv = a.W + vox * a.wstride; }
  auto elem_raw = [&](int m, int n) -> double { return f2_elem(a, vox * M + m, n); };
  auto elem = [&](int m, int n) -> double {   // WGT: fl(s_m d)
    if constexpr (WGT) return sv[m] * elem_raw(m, n);
    else return elem_raw(m, n);
  };
  if (tid == 0) s_misc[0] = mfx_np_sumsq(ys, M);   // _1 uses np.sum(y**2)
  __syncthreads();
  const double y_sq = s_misc[0];
  // thread-local best in the reference's scan order; key < 0 = the reference's initial state
  double bres = y_sq, bw = 0.0;
  long bkey = -1;
  for (int i = tid; i < N; i += F2_K1_WG) {
    double a11 = 0.0, Y1 = 0.0;
#pragma unroll 4
    for (int m = 0; m < M; ++m) {
      const double d = elem(m, i);
      a11 += d * d;
      Y1 += ys[m] * d;
    }
    double w, r;
    nnls1_exact(y_sq, a11, Y1, w, r);
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
    for (int m = lane; m < M; m += 64) s_yrec[m] = w * elem_raw(m, ia);
    double r2;
    if constexpr (WGT) r2 = f2_r2w(yv, wv, s_yrec, M, lane);
    else r2 = f2_r2(yv, s_yrec, M, lane);
    if (lane == 0) {   // params packing, mf.py:420-450
      double* out = a.params + vox * a.num_params;
      out[0] = w;
      out[1] = (fabs(w) > 0) ? w / w : w;
      out[1 + a.maxfasc] = (double)ia;
      if constexpr (WGT) out[a.num_params - 2] = res / a.sumw[vox];
      else out[a.num_params - 2] = res / M;
      out[a.num_params - 1] = r2;
    }
  }
}

}  // namespace
