// w2d.hip -- measurement weights for voxels of a 2-D (AxCaliber-like) protocol (include/mfx_w2d.h): the fit of fit2d.hip
// and the soft fits and objective profiles of soft2d.hip with a weight W[v, m] >= 0 per voxel and measurement.  Per voxel
// the reference chain on rows scaled by s = sqrt(W): rotate_atom_2Dprotocol per fascicle -> rows times s ->
// solve_exhaustive_posweights on (s A, s y) -> params packing with MSE = min_obj / sum W and the weighted R2; F_W of the
// posterior and the profile is the F of mfx_soft2d.h on (s A, s y).
//
// Every dictionary entry is fl(s_m * d) with d the entry of fit2d_shared.h (f2_value / r2_value on the 32-byte records),
// bit for bit the entry mfx_rot2d_rotate returns: for W = 1 the kernels here see the unweighted columns (s = 1).  The one
// new operation of operand generation is that product.
//
// w2d_prep_kernel        once per call, one wave per voxel: the weights' status (uniform over the voxel), s [V x M],
//                        y' = s y [V x M] and sum W into the stream's scratch arena; NaN row of a flagged voxel (fit).  s
//                        and y' live in memory, not LDS: the kernels' LDS footprint stays independent of M.
// mfx_wfit2d_k2_kernel   K = 2, no extra column: mfx_fit2d_k2_kernel's three phases.  s_m of a chunk's rows is staged in
//                        LDS beside the rows' records, two chunks ahead, by 8 threads that are idle in stage_rec;
//                        store_chunk multiplies each generated entry by it.  Phase 1 and the exact stage form their
//                        serial sums over fl(s_m d) and y' in the reference's row order.  The scan, the 4 M eps interval,
//                        the unranked hand-over, the family expansion and the overflow pass are unchanged.
// mfx_wfit2d_k1_kernel   K = 1: one thread per atom, |y'|^2 in np.sum's pairwise order.
// every other fit class  w2d_mat_kernel materialises the scaled dictionaries in voxel chunks, the explicit solver of
//                        mfx_api.hip runs per voxel on (s A, y'), w2d_repack_kernel puts the weighted MSE and R2 in.
// mfx_wsoft2d_k2_kernel<MODE>, mfx_wsoft2d_k1_kernel<MODE>   mfx_soft2d_k2_kernel / k1 with the same two changes.
#include "fit2d_shared.h"
#include "../../include/mfx_w2d.h"
#include "../../include/mfx_profile.h"   // mfx_profile_cut
#include "fit_small.hip"                 // mfx_np_sumsq

#include <algorithm>
#include <cstring>
#include <vector>

// profile.hip's MFX_PROFILE_CUT restated as a compile-time constant; the entry points refuse to launch unless it equals
// mfx_profile_cut()
#define MFX_W2D_CUT 1e-8

namespace {

constexpr int W2_MAXC = 512;               // short-list entries
constexpr size_t W2_LDS_MAX = 160 * 1024;
constexpr int W2_K1_WG = 256;
constexpr int W2_POST = 0, W2_PROF = 1;
constexpr double W2_EXP_MAX = 700.0;       // exponents above this make the shift unusable (status 2)
constexpr int W2_NO_PARTNER = 0x7fffffff;

thread_local int g_force_explicit = 0;

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

// the unscaled entry (record i, atom n)
__device__ __forceinline__ double w2_elem(const W2Args& a, size_t i, int n) {
  const F2Rec r = a.rec[i];
  return f2_value(a.base, r, n);
}

// voxel record from the directions' records: the lowest failing fascicle (the record of mfx_fit2d.h); with params, the NaN
// row of such a voxel
__global__ void w2d_status_kernel(const int* __restrict__ pstat, int K, int64_t V, int* __restrict__ vstat, double* __restrict__ params,
                                  int np) {
  const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= V) return;
  int rec[5] = {0, 0, 0, 0, 0};
  for (int k = 0; k < K; ++k) {
    const int* s = pstat + 4 * (v * K + k);
    if (s[0] != MFX_ROT2D_OK) { rec[0] = s[0]; rec[1] = s[1]; rec[2] = s[2]; rec[3] = s[3]; rec[4] = k; break; }
  }
  for (int q = 0; q < 5; ++q) vstat[5 * v + q] = rec[q];
  if (params && rec[0] != 0)
    for (int q = 0; q < np; ++q) params[v * np + q] = __builtin_nan("");
}

// One wave per voxel: the weights are tested over the whole voxel first (the result is uniform), then s, y' and sum W are
// written.  A voxel with a failing direction is left alone (weight status 0: the direction is reported); a voxel with
// unusable weights gets zeros in s and y' (nobody reads them), its code, and with params its NaN row.  ok (may be null):
// 1 where the fit runs.
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
    Ys[v * M + m] = s * yv[m];
  }
  if (params && code != 0)
    for (int q = lane; q < np; q += 64) params[v * np + q] = __builtin_nan("");
  if (lane == 0) { wstat[v] = code; sumw[v] = sw; if (ok) ok[v] = code == 0; }
}

// Squared weighted Pearson correlation of y and y_rec by the 64 lanes of one wave (weights wv, weighted means).  The
// common normaliser of the three moments cancels; it is n_pos - 1 (n_pos the number of positive weights), so that a 0/1
// mask gives np.corrcoef's arithmetic on the kept rows and W = 1 that of fit2d.hip's f2_r2, operation for operation.
// 0 with fewer than two positive weights or a vanishing weighted variance.
__device__ __forceinline__ double w2_r2(const double* __restrict__ yv, const double* __restrict__ wv, const double* s_yrec, int M,
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

// mfx_fit2d_k2_kernel's LDS plus the staged s of two chunks
size_t w2_fit_lds_bytes(int NP) {
  return ((size_t)2 * F2_NT * F2_TS + 4 * (size_t)NP + 32 + 2 * F2_MC) * sizeof(double) + F2_REC * sizeof(F2Rec) + W2_MAXC * sizeof(Cand) +
         4 * sizeof(int);
}

__global__ __launch_bounds__(F2_WG, 2) void mfx_wfit2d_k2_kernel(W2Args a) {
  extern __shared__ double smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lg = lane >> 4, lc = lane & 15;
  const int wr = wave >> 1, wc = wave & 1;
  const int M = a.M, N = a.N;
  const int NP = (N + 15) & ~15;   // atoms padded to a multiple of 16 (padded atoms are zero columns)
  const int ntiles = NP >> 4;
  const size_t vox = blockIdx.x;
  if (a.vstat[5 * vox] != 0 || a.wstat[vox] != 0) return;   // a failing direction, unusable weights: the row is written (workgroup-uniform)

  // ---- LDS carve-up (w2_fit_lds_bytes mirrors it)
  double* sT = smem;                             // [2][F2_NT][F2_TS]: tiles 0..7 the D_0 block, 8..15 the D_1 block
  double2* s_st = (double2*)(sT + 2 * F2_NT * F2_TS);   // [2][NP] column statistics {|d|^2, d.y} of D_0, then of D_1
  double* s_red = (double*)(s_st + 2 * NP);      // [32] scratch
  double* s_sc = s_red + 32;                     // [2][F2_MC] staged s of two chunks
  F2Rec* s_rec = (F2Rec*)(s_sc + 2 * F2_MC);     // [F2_REC] staged records of two chunks
  Cand* s_cand = (Cand*)(s_rec + F2_REC);        // [W2_MAXC]
  int* s_cnt = (int*)(s_cand + W2_MAXC);         // [4]

  const double* __restrict__ yv = a.Y + vox * M;          // unscaled: the weighted R2
  const double* __restrict__ ys = a.Ys + vox * M;         // y' = s y
  const double* __restrict__ sv = a.S + vox * M;
  const double* __restrict__ wv = a.W + vox * a.wstride;
  const size_t rec0 = 2 * vox * M;               // records of direction k: + k M
  auto elem_raw = [&](int k, int m, int n) -> double { return w2_elem(a, rec0 + (size_t)k * M + m, n); };
  auto elem = [&](int k, int m, int n) -> double { return sv[m] * elem_raw(k, m, n); };   // fl(s_m d)

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
      for (int w = 1; w < F2_NW; ++w) {
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
    } else if (tid < 3 * F2_MC) {   // s of the chunk's rows (0 beyond the protocol), by chunk parity
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
          const double v = s_sc[(ch & 1) * F2_MC + r] * r2_value(s_rec[q0 + r].o, s_rec[q0 + r].s, va[r], s_rec[q0 + r].dx, vb[r]);
          dst[r * 16] = gn < N ? v : 0.0;   // atoms beyond the dictionary: zero columns
        }
      };
      d4 acc[4][4];
#pragma unroll
      for (int ti = 0; ti < 4; ++ti)
#pragma unroll
        for (int tj = 0; tj < 4; ++tj) acc[ti][tj] = d4{0, 0, 0, 0};

      // The first two chunks are staged through an index the compiler cannot see through: with the literal 0 and 1 it
      // hoists the staging threads' two addresses of s out of the block loops and keeps them in registers through
      // the chunk loop, which the posterior's budget (255 VGPRs) does not hold.
      int ch0 = 0;
      asm volatile("" : "+s"(ch0));
      stage_rec(ch0);
      stage_rec(ch0 + 1);
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
                  if (slot < W2_MAXC) { s_cand[slot].score = 1e300; s_cand[slot].i = i; s_cand[slot].j = j; }
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
                  if (slot < W2_MAXC) { s_cand[slot].score = sc + er + eps_abs; s_cand[slot].i = i; s_cand[slot].j = bj; }   // upper bound
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
  const int ncand = nappend > W2_MAXC ? W2_MAXC : nappend;
  __syncthreads();   // everyone has read s_cnt / is done with the operand buffers
  if (tid == 0) {    // mf_utils.py:327, 382: start from min_obj = y_sq at pair (0,0) with w = 0, strict '<'
    s_win[0] = y_sq; s_win[1] = 0.0; s_win[2] = 0.0; ((long*)s_win)[3] = -1;
  }
  {
    double res = INFINITY, w0 = 0.0, w1 = 0.0;
    long idx = -1;
    if (nappend <= W2_MAXC) {
      // A scan candidate is the best pair of its slot - row i, the columns j = lc (mod 16) of one wave's half of one
      // column block; a second pair of the slot within rounding distance of the optimum was never listed.  The whole
      // row i over the columns j = lc (mod 16) (a superset of the slot) is therefore evaluated exactly for every listed
      // candidate that still reaches the final lower bound.  The first entries are the single-atom representatives of
      // phase 1: themselves only.
      const int NJ = (N + 15) >> 4, nsingle = s_cnt[1];
      for (int q = tid; q < ncand * NJ; q += F2_WG) {
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
    const double r2 = w2_r2(yv, wv, s_yrec, M, lane);
    double* out = a.params + vox * a.num_params;
    if (lane == 0) {
      out[0] = M0;
      out[1] = nu0;
      out[2] = nu1;
      out[1 + a.maxfasc] = (double)bi;
      out[2 + a.maxfasc] = (double)bjx;
      out[a.num_params - 2] = best / a.sumw[vox];
      out[a.num_params - 1] = r2;
    }
  }
}
static_assert(2 * F2_NT * F2_TS >= R2_MAX_ROWS + 48, "y_rec scratch of the K = 2 kernel");

// K = 1, no extra column: one workgroup per voxel, one thread per atom; solve_exhaustive_posweights_1 (mf_utils.py:225-286)
// on (s D, y')
__global__ __launch_bounds__(W2_K1_WG) void mfx_wfit2d_k1_kernel(W2Args a) {
  extern __shared__ double smem[];
  const int tid = threadIdx.x;
  const int M = a.M, N = a.N;
  const size_t vox = blockIdx.x;
  if (a.vstat[5 * vox] != 0 || a.wstat[vox] != 0) return;
  double* s_res = smem;                         // [WG]
  long* s_key = (long*)(s_res + W2_K1_WG);      // [WG]
  double* s_misc = (double*)(s_key + W2_K1_WG); // [8]
  double* s_yrec = s_misc + 8;                  // [M]
  const double* __restrict__ yv = a.Y + vox * M;
  const double* __restrict__ ys = a.Ys + vox * M;
  const double* __restrict__ sv = a.S + vox * M;
  const double* __restrict__ wv = a.W + vox * a.wstride;
  auto elem_raw = [&](int m, int n) -> double { return w2_elem(a, vox * M + m, n); };
  auto elem = [&](int m, int n) -> double { return sv[m] * elem_raw(m, n); };   // fl(s_m d)
  if (tid == 0) s_misc[0] = mfx_np_sumsq(ys, M);   // _1 uses np.sum(y**2)
  __syncthreads();
  const double y_sq = s_misc[0];
  // thread-local best in the reference's scan order; key < 0 = the reference's initial state
  double bres = y_sq, bw = 0.0;
  long bkey = -1;
  for (int i = tid; i < N; i += W2_K1_WG) {
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
  for (int o = W2_K1_WG / 2; o > 0; o >>= 1) {
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
    const double r2 = w2_r2(yv, wv, s_yrec, M, lane);
    if (lane == 0) {   // params packing, mf.py:420-450
      double* out = a.params + vox * a.num_params;
      out[0] = w;
      out[1] = (fabs(w) > 0) ? w / w : w;
      out[1 + a.maxfasc] = (double)ia;
      out[a.num_params - 2] = res / a.sumw[vox];
      out[a.num_params - 1] = r2;
    }
  }
}

// the voxels' scaled dictionaries [nv][M][Ntot]: K blocks of N columns, then the scaled CSF column; grid (voxel, block of 8
// rows)
__global__ __launch_bounds__(256) void w2d_mat_kernel(W2Args a, const int* __restrict__ ok, int64_t v0, int K, int has_csf,
                                                     const double* __restrict__ xc, double* __restrict__ A) {
  const int64_t v = v0 + blockIdx.x;
  if (!ok[v]) return;
  const int M = a.M, N = a.N, Ntot = K * N + has_csf;
  const double* __restrict__ sv = a.S + (size_t)v * M;
  for (int r = 0; r < 8; ++r) {
    const int m = blockIdx.y * 8 + r;
    if (m >= M) break;
    const double s = sv[m];
    double* dst = A + ((size_t)blockIdx.x * M + m) * Ntot;
    for (int k = 0; k < K; ++k) {
      const size_t i = (size_t)(v * K + k) * M + m;
      for (int n = threadIdx.x; n < N; n += 256) dst[k * N + n] = s * w2_elem(a, i, n);
    }
    if (has_csf && threadIdx.x == 0) dst[K * N] = s * xc[m];
  }
}

// The explicit solver packed the row for (s A, y'): MSE = min_obj / M and the unweighted R2 of the scaled signals.  One
// wave per voxel puts the weighted figures in: MSE (M / sum W), and the weighted R2 of y and y_rec = D w + w_csf x_csf on
// the unscaled columns, with w_k = nu_k M0 from the row.
__global__ __launch_bounds__(64) void w2d_repack_kernel(W2Args a, const int* __restrict__ ok, int64_t v0, int K, int has_csf,
                                                       const double* __restrict__ xc) {
  extern __shared__ double s_yrec[];
  const int64_t v = v0 + blockIdx.x;
  if (!ok[v]) return;
  const int M = a.M, lane = threadIdx.x;
  const double* __restrict__ yv = a.Y + (size_t)v * M;
  const double* __restrict__ wv = a.W + (size_t)v * a.wstride;
  double* row = a.params + (size_t)v * a.num_params;
  const double M0 = row[0];
  const double sc = (fabs(M0) > 0) ? M0 : 1.0;
  for (int m = lane; m < M; m += 64) {
    double yr = 0.0;
    for (int k = 0; k < K; ++k)
      yr += w2_elem(a, (size_t)(v * K + k) * M + m, (int)row[1 + a.maxfasc + k]) * (row[1 + k] * sc);
    if (has_csf) yr += xc[m] * (row[2 * a.maxfasc + 1] * sc);
    s_yrec[m] = yr;
  }
  __syncthreads();
  const double r2 = w2_r2(yv, wv, s_yrec, M, lane);
  if (lane == 0) {
    row[a.num_params - 2] = row[a.num_params - 2] * ((double)M / a.sumw[v]);
    row[a.num_params - 1] = r2;
  }
}

// ---- posterior and profile

// score s = ||y'||^2 - F_W of one atom pair as the fraction p / q (soft2d.hip: s2_pair_frac)
__device__ __forceinline__ void w2_pair_frac(double A11, double A22, double A12, double Y1, double Y2, double p1, double p2,
                                             double& p, double& q) {
  const double d1 = fma(-A12, Y2, A22 * Y1);
  const double d2 = fma(-A12, Y1, A11 * Y2);
  const double pd = A11 * A22;
  const double Det = fma(-A12, A12, pd);
  const double num = fma(Y2, d2, Y1 * d1);
  const bool both = (d1 > 0.0) & (d2 > 0.0) & (Det > MFX_W2D_CUT * pd);
  const bool first = p1 * A22 >= p2 * A11;
  p = both ? num : (first ? p1 : p2);
  q = both ? Det : (first ? A11 : A22);
}

__device__ __forceinline__ bool w2_finite(double x) { return fabs(x) <= 1.79769313486231570815e308; }   // false for NaN

// a voxel without a result: NaN rows (partner -1), NaN log_sum and the status code (every thread of the workgroup takes part)
template <int MODE>
__device__ __forceinline__ void w2_nan_rows(const W2Args& a, size_t vox, int K, int code, int tid, int wg) {
  const double nan = __builtin_nan("");
  const size_t n_out = (size_t)K * a.N;
  for (size_t n = tid; n < n_out; n += wg) {
    a.out[vox * n_out + n] = nan;
    if (MODE == W2_PROF && a.partner) a.partner[vox * n_out + n] = -1;
  }
  if (MODE == W2_POST && tid == 0) { a.log_sum[vox] = nan; a.status[vox] = code; }
}

// mfx_soft2d_k2_kernel's LDS plus the staged s of two chunks
size_t w2_soft_lds_bytes(int mode, int NP) {
  const size_t dbl = (size_t)2 * F2_NT * F2_TS + 4 * (size_t)NP + 2 * (size_t)NP + 4 * F2_BLK + 8 + 2 * F2_MC;
  const size_t ints = (mode == W2_PROF ? 2 * (size_t)NP + 4 * F2_BLK : 0) + 4;
  return dbl * sizeof(double) + F2_REC * sizeof(F2Rec) + ints * sizeof(int);
}

template <int MODE>
__global__ __launch_bounds__(F2_WG, 2) void mfx_wsoft2d_k2_kernel(W2Args a) {
  constexpr bool POST = MODE == W2_POST;
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
    w2_nan_rows<MODE>(a, vox, 2, 5, tid, F2_WG);
    return;
  }
  if constexpr (POST) {
    const double Tv = a.temp[vox], shift = a.shift[vox];
    if (!(Tv > 0.0) || !w2_finite(Tv) || !w2_finite(shift)) {
      w2_nan_rows<MODE>(a, vox, 2, 1, tid, F2_WG);
      return;
    }
  }

  if (a.wstat[vox] != 0) {         // unusable weights (workgroup-uniform): 3 a bad weight, 4 none positive
    w2_nan_rows<MODE>(a, vox, 2, 2 + a.wstat[vox], tid, F2_WG);
    return;
  }

  // ---- LDS carve-up (w2_soft_lds_bytes mirrors it)
  double* sT = smem;                                    // [2][F2_NT][F2_TS]: tiles 0..7 the D_0 block, 8..15 the D_1 block
  double2* s_st = (double2*)(sT + 2 * F2_NT * F2_TS);   // [2][NP] column statistics {|d|^2, d.y} of D_0, then of D_1
  double* s_R = (double*)(s_st + 2 * NP);               // [2][NP] running row (R0) and column (R1) sums / best scores
  double* s_sl = s_R + 2 * NP;                          // [4][F2_BLK] the waves' partials of one block: rows by wc, columns by wr
  double* s_red = s_sl + 4 * F2_BLK;                    // [8]: [0] ||y||^2, [1] ||y||^2 - shift, [2] 1 / T
  double* s_sc = s_red + 8;                             // [2][F2_MC] staged s of two chunks
  F2Rec* s_rec = (F2Rec*)(s_sc + 2 * F2_MC);            // [F2_REC] staged records of two chunks
  int* s_Ri = (int*)(s_rec + F2_REC);                   // [2][NP] partners of the running bests (profile)
  int* s_sli = s_Ri + (POST ? 0 : 2 * NP);              // [4][F2_BLK] (profile)
  int* s_flag = s_sli + (POST ? 0 : 4 * F2_BLK);        // [4]: [0] an exponent above W2_EXP_MAX was met

  const double* __restrict__ ys = a.Ys + vox * M;       // y' = s y
  const double* __restrict__ sv = a.S + vox * M;
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
        const double d = sv[m] * f2_value(a.base, r, n);   // fl(s_m d)
        a2 += d * d;
        ay += ys[m] * d;
      }
    }
    s_st[col] = double2{a2, ay};
    s_R[col] = POST ? 0.0 : -1.0;          // a score is never negative: the first real pair wins
    if constexpr (!POST) s_Ri[col] = W2_NO_PARTNER;
  }
  __syncthreads();
  bool over = false;                       // this lane met an exponent above W2_EXP_MAX on a pair of two real atoms

  // ---- phase 2: cross-Gram blocks accumulated over the rows in chunks (fit2d.hip's loop), then the block's pairs
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
    } else if (tid < 3 * F2_MC) {   // s of the chunk's rows (0 beyond the protocol), by chunk parity
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
          const double v = s_sc[(ch & 1) * F2_MC + r] * r2_value(s_rec[q0 + r].o, s_rec[q0 + r].s, va[r], s_rec[q0 + r].dx, vb[r]);
          dst[r * 16] = gn < N ? v : 0.0;   // atoms beyond the dictionary: zero columns
        }
      };
      d4 acc[4][4];
#pragma unroll
      for (int ti = 0; ti < 4; ++ti)
#pragma unroll
        for (int tj = 0; tj < 4; ++tj) acc[ti][tj] = d4{0, 0, 0, 0};

      // The first two chunks are staged through an index the compiler cannot see through: with the literal 0 and 1 it
      // hoists the staging threads' two addresses of s out of the block loops and keeps them in registers through
      // the chunk loop, which the posterior's budget (255 VGPRs) does not hold.
      int ch0 = 0;
      asm volatile("" : "+s"(ch0));
      stage_rec(ch0);
      stage_rec(ch0 + 1);
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
      for (int t = 0; t < 4; ++t) { cs[t] = POST ? 0.0 : -1.0; ci[t] = W2_NO_PARTNER; }
      mfx_static_for<0, 4>([&](auto tic) {
        constexpr int ti = decltype(tic)::value;
#pragma unroll 1
        for (int r = 0; r < 4; ++r) {
          const int il = wr * 64 + ti * 16 + lg + 4 * r;   // row within the block
          const int i = rb * F2_BLK + il;
          double rv = POST ? 0.0 : -1.0;
          int rj = W2_NO_PARTNER;
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
                w2_pair_frac(A11, A22, A12, Y1, Y2, p1, p2, p, q);
                const double s = q > 0.0 ? p / q : 0.0;
                const bool ok = (i < N) & (j < N);   // padded atoms contribute nothing
                if constexpr (POST) {
                  const double e = (s - s_red[1]) * s_red[2];
                  over |= ok & (e > W2_EXP_MAX);
                  const double tv = ok ? exp(e) : 0.0;
                  rv += tv;
                  cs[tj] += tv;
                  __builtin_amdgcn_sched_barrier(0);   // one pair's exp at a time: four interleaved ones do not fit the register budget
                } else {
                  const double sv = ok ? s : -1.0;
                  const bool brow = sv > rv;        // ascending j: the first best stays
                  rv = brow ? sv : rv;
                  rj = brow ? j : rj;
                  const bool bcol = sv > cs[tj];    // ascending i
                  cs[tj] = bcol ? sv : cs[tj];
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
    if (s_flag[0] != 0 || !(Z > 0.0) || !w2_finite(Z)) {
      w2_nan_rows<MODE>(a, vox, 2, 2, tid, F2_WG);
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
template <int MODE>
__global__ __launch_bounds__(W2_K1_WG) void mfx_wsoft2d_k1_kernel(W2Args a) {
  constexpr bool POST = MODE == W2_POST;
  __shared__ double s_ysq;
  __shared__ int s_over;
  const int tid = threadIdx.x;
  const int M = a.M, N = a.N;
  const size_t vox = blockIdx.x;
  if (a.vstat[5 * vox] != 0) {
    w2_nan_rows<MODE>(a, vox, 1, 5, tid, W2_K1_WG);
    return;
  }
  double Tv = 1.0, shift = 0.0;
  if constexpr (POST) {
    Tv = a.temp[vox];
    shift = a.shift[vox];
    if (!(Tv > 0.0) || !w2_finite(Tv) || !w2_finite(shift)) {
      w2_nan_rows<MODE>(a, vox, 1, 1, tid, W2_K1_WG);
      return;
    }
  }
  if (a.wstat[vox] != 0) {
    w2_nan_rows<MODE>(a, vox, 1, 2 + a.wstat[vox], tid, W2_K1_WG);
    return;
  }
  const double* __restrict__ ys = a.Ys + vox * M;
  const double* __restrict__ sv = a.S + vox * M;
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
  for (int n = tid; n < N; n += W2_K1_WG) {
    double a2 = 0.0, ay = 0.0;
#pragma unroll 4
    for (int m = 0; m < M; ++m) {
      const F2Rec r = a.rec[vox * M + m];
      const double d = sv[m] * f2_value(a.base, r, n);   // fl(s_m d)
      a2 += d * d;
      ay += ys[m] * d;
    }
    const double yp = fmax(ay, 0.0);
    const double s = a2 > 0.0 ? yp * yp / a2 : 0.0;
    if constexpr (POST) {
      const double e = (s - c0) * iT;
      over |= e > W2_EXP_MAX;
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
    if (s_over != 0 || !(Z > 0.0) || !w2_finite(Z)) {
      w2_nan_rows<MODE>(a, vox, 1, 2, tid, W2_K1_WG);
      return;
    }
    for (int n = tid; n < N; n += W2_K1_WG) row[n] = row[n] / Z;
    if (tid == 0) {
      a.log_sum[vox] = log(Z) - shift / Tv;
      a.status[vox] = 0;
    }
  }
}

const char* NO_DEVICE = "no HIP device available (this library has no CPU path)";

int w2_require_device(int device) {
  const int n = mfx_device_count();
  if (n <= 0) return mfx_fail(MFX_ERR_NO_DEVICE, "%s", NO_DEVICE);
  if (device < 0 || device >= n) return mfx_fail(MFX_ERR_ARG, "device %d out of range (have %d)", device, n);
  HIPCHK(hipSetDevice(device));
  return MFX_OK;
}

int w2_fit_max_atoms() {
  int n = 0;
  while (n < (1 << 20) && w2_fit_lds_bytes(n + 16) <= W2_LDS_MAX) n += 16;
  return n;
}

int w2_soft_max_atoms(int mode) {
  int n = 0;
  while (n < (1 << 20) && w2_soft_lds_bytes(mode, n + 16) <= W2_LDS_MAX) n += 16;
  return n;
}

// what every class launch shares: the plan of the V K directions, the voxels' direction records, the kernels' records and
// the prepared weights.  Scratch of the stream's arena, released with the object.
struct W2Scratch {
  PlanMem pm;
  StreamMem pstat, rec, prep, ok;
  explicit W2Scratch(hipStream_t st) : pm(st), pstat(st), rec(st), prep(st), ok(st) {}
  // fills a.M .. a.vstat; d_params non-null: the fit (NaN rows are written, wstat is the caller's d_wstat)
  int enqueue(const mfx_rot2d* h, const double* d_Y, const double* d_W, int64_t wstride, const double* d_peaks, int K, int64_t V,
              int32_t* d_vstat, int32_t* d_wstat, double* d_params, int np, W2Args& a, hipStream_t st) {
    const int M = h->d.M;
    HIPCHK(pstat.alloc(sizeof(int) * 4 * (size_t)V * std::max(K, 1)));
    if (int rc = pm.alloc(V * K, M, pstat.as<int>())) return rc;
    if (K > 0)
      if (int rc = mfx_rot2d_plan_enqueue(h, d_peaks, V * K, pm.pl, st)) return rc;
    hipLaunchKernelGGL(w2d_status_kernel, dim3((unsigned)((V + 255) / 256)), dim3(256), 0, st, pstat.as<int>(), K, V, d_vstat, d_params, np);
    HIPCHK(hipGetLastError());
    const size_t nrec = (size_t)V * K * M;
    HIPCHK(rec.alloc(nrec * sizeof(F2Rec) + 64));
    if (nrec > 0) {
      hipLaunchKernelGGL(fit2d_rec_kernel, dim3((unsigned)((nrec + 255) / 256)), dim3(256), 0, st, h->d, pm.pl, (int64_t)nrec, rec.as<F2Rec>());
      HIPCHK(hipGetLastError());
    }
    // s [V x M], y' [V x M], sum W [V], and the weights' status where the caller has no array for it
    const size_t vm = (size_t)V * M;
    HIPCHK(prep.alloc(sizeof(double) * (2 * vm + (size_t)V) + sizeof(int) * (size_t)V + 64));
    HIPCHK(ok.alloc(sizeof(int) * (size_t)V));
    double* S = prep.as<double>();
    double* Ys = S + vm;
    double* sumw = Ys + vm;
    int* wstat = d_wstat ? d_wstat : (int*)(sumw + V);
    hipLaunchKernelGGL(w2d_prep_kernel, dim3((unsigned)V), dim3(64), 0, st, d_Y, d_W, wstride, M, d_vstat, S, Ys, sumw, wstat, ok.as<int>(),
                       d_params, np);
    HIPCHK(hipGetLastError());
    a.M = M; a.N = h->d.N; a.base = h->d.ky; a.rec = rec.as<F2Rec>();
    a.Y = d_Y; a.W = d_W; a.wstride = wstride; a.S = S; a.Ys = Ys; a.sumw = sumw; a.wstat = wstat; a.vstat = d_vstat;
    return MFX_OK;
  }
};

int w2_limits(const char* fn, const mfx_rot2d* h, int K, int64_t V) {
  if (V > 0x3fffffff / std::max(K, 1)) return mfx_fail(MFX_ERR_UNSUPPORTED, "%s: more than 2^30 directions in one call", fn);
  if (((size_t)2 * h->d.K + h->d.C + 2) * (size_t)h->d.N > 0x7fffffff)
    return mfx_fail(MFX_ERR_UNSUPPORTED, "%s: tables of more than 2^31 doubles", fn);
  return MFX_OK;
}

// One fit class on device buffers: V voxels of K fascicles each (d_peaks [V x 3 K], contiguous), with the CSF column d_xc
// or without (null) -> d_params [V x np] (np = 1 + 2 maxfasc + csf_on + 2), d_vstat [V x 5], d_wstat [V].  Only enqueues.
int w2_class_dev(const mfx_rot2d* h, const double* d_Y, const double* d_W, int64_t wstride, const double* d_peaks, int K,
                 const double* d_xc, int maxfasc, int csf_on, int64_t V, double* d_params, int32_t* d_vstat, int32_t* d_wstat,
                 hipStream_t st) {
  const int M = h->d.M, N = h->d.N, has_csf = d_xc != nullptr;
  const int np = 1 + 2 * maxfasc + csf_on + 2;
  if (int rc = w2_limits("mfx_wfit2d", h, K, V)) return rc;
  HIPCHK(hipMemsetAsync(d_params, 0, sizeof(double) * (size_t)V * np, st));
  W2Scratch sc(st);
  W2Args a{};
  if (int rc = sc.enqueue(h, d_Y, d_W, wstride, d_peaks, K, V, d_vstat, d_wstat, d_params, np, a, st)) return rc;
  if (K == 0 && !has_csf) return MFX_OK;   // mf.py:387: nothing to fit, a zero row (NaN where the weights are unusable)
  a.params = d_params; a.num_params = np; a.maxfasc = maxfasc;
  if (!g_force_explicit && !has_csf && K == 2 && w2_fit_lds_bytes((N + 15) & ~15) <= W2_LDS_MAX) {
    const size_t lds = w2_fit_lds_bytes((N + 15) & ~15);
    HIPCHK(hipFuncSetAttribute((const void*)mfx_wfit2d_k2_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(mfx_wfit2d_k2_kernel, dim3((unsigned)V), dim3(F2_WG), lds, st, a);
    HIPCHK(hipGetLastError());
    return MFX_OK;
  }
  if (!g_force_explicit && !has_csf && K == 1) {
    const size_t lds = (2 * W2_K1_WG + 8 + (size_t)M) * sizeof(double);
    hipLaunchKernelGGL(mfx_wfit2d_k1_kernel, dim3((unsigned)V), dim3(W2_K1_WG), lds, st, a);
    HIPCHK(hipGetLastError());
    return MFX_OK;
  }
  // every other class: materialise the scaled dictionaries in voxel chunks within a byte budget, explicit solver per voxel
  const size_t Ntot = (size_t)K * N + has_csf, per_vox = sizeof(double) * M * Ntot;
  size_t free_b = 0, total_b = 0, scratch_b = 0;
  HIPCHK(hipMemGetInfo(&free_b, &total_b));
  if (int rc = mfx_solve_dense_scratch_bytes(M, K, N, has_csf, &scratch_b)) return rc;
  const size_t budget = std::min<size_t>(free_b / 4, (size_t)1 << 30);
  const int64_t nvc = std::max<int64_t>(1, std::min<int64_t>(V, (int64_t)(budget / per_vox)));
  StreamMem dA(st), dS(st);
  HIPCHK(dA.alloc(per_vox * nvc));
  HIPCHK(dS.alloc(scratch_b));
  const int* ok = sc.ok.as<int>();
  for (int64_t v0 = 0; v0 < V; v0 += nvc) {
    const int64_t nv = std::min(nvc, V - v0);
    hipLaunchKernelGGL(w2d_mat_kernel, dim3((unsigned)nv, (unsigned)((M + 7) / 8)), dim3(256), 0, st, a, ok, v0, K, has_csf, d_xc,
                       dA.as<double>());
    HIPCHK(hipGetLastError());
    for (int64_t q = 0; q < nv; ++q) {
      const int64_t v = v0 + q;
      if (int rc = mfx_solve_dense_dev(dA.as<double>() + (size_t)q * M * Ntot, M, K, N, has_csf, a.Ys + (size_t)v * M, maxfasc, csf_on,
                                       d_params + (size_t)v * np, ok + v, dS.p, st)) return rc;
    }
    hipLaunchKernelGGL(w2d_repack_kernel, dim3((unsigned)nv), dim3(64), sizeof(double) * M, st, a, ok, v0, K, has_csf, d_xc);
    HIPCHK(hipGetLastError());
  }
  return MFX_OK;
}

template <int MODE>
int w2_soft_launch(const W2Args& a, int K, int64_t V, hipStream_t st) {
  if (K == 2) {
    const size_t lds = w2_soft_lds_bytes(MODE, (a.N + 15) & ~15);
    HIPCHK(hipFuncSetAttribute((const void*)mfx_wsoft2d_k2_kernel<MODE>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(mfx_wsoft2d_k2_kernel<MODE>, dim3((unsigned)V), dim3(F2_WG), lds, st, a);
  } else {
    hipLaunchKernelGGL(mfx_wsoft2d_k1_kernel<MODE>, dim3((unsigned)V), dim3(W2_K1_WG), 0, st, a);
  }
  HIPCHK(hipGetLastError());
  return MFX_OK;
}

int w2_stride_check(const char* fn, const mfx_rot2d* h, int64_t w_stride) {
  if (w_stride != 0 && w_stride != h->d.M)
    return mfx_fail(MFX_ERR_ARG, "%s: w_stride should be M = %d or 0 (got %lld)", fn, h->d.M, (long long)w_stride);
  return MFX_OK;
}

// every check of the posterior's and the profile's entry points that needs no device: the arguments, the class, the LDS limit
int w2_soft_check(const char* fn, int mode, const mfx_rot2d* h, const void* Y, const void* W, int64_t w_stride, const void* peaks, int K,
                  const void* T, const void* shift, int64_t V, const void* out, const void* log_sum, const void* status,
                  const void* dir_status) {
  const bool post = mode == W2_POST;
  if (!h || V < 0 || (V > 0 && (!Y || !W || !peaks || !out || !dir_status || (post && (!T || !shift || !log_sum || !status)))))
    return mfx_fail(MFX_ERR_ARG, "%s: bad argument", fn);
  if (int rc = w2_stride_check(fn, h, w_stride)) return rc;
  if (K != 1 && K != 2)
    return mfx_fail(MFX_ERR_UNSUPPORTED, "%s: K must be 1 or 2 (got %d): three fascicles and voxels without one are out of scope", fn, K);
  if (int rc = w2_limits(fn, h, K, V)) return rc;
  if (K == 2 && w2_soft_lds_bytes(mode, (h->d.N + 15) & ~15) > W2_LDS_MAX)
    return mfx_fail(MFX_ERR_UNSUPPORTED, "%s: N = %d atoms exceed the %d that fit in LDS", fn, h->d.N, w2_soft_max_atoms(mode));
  if (mfx_profile_cut() != MFX_W2D_CUT) return mfx_fail(MFX_ERR_HIP, "%s: built with a cut other than the profile's", fn);
  return MFX_OK;
}

// shared body of the posterior's and the profile's device entry points: only enqueues
int w2_soft_enqueue(const char* fn, int mode, const mfx_rot2d* h, const double* d_Y, const double* d_W, int64_t w_stride,
                    const double* d_peaks, int K, const double* d_T, const double* d_shift, int64_t V, double* d_out, double* d_log_sum,
                    int32_t* d_status, int32_t* d_partner, int32_t* d_dir_status, hipStream_t st) {
  if (mfx_device_count() <= 0) return mfx_fail(MFX_ERR_NO_DEVICE, "%s", NO_DEVICE);
  if (int rc = w2_soft_check(fn, mode, h, d_Y, d_W, w_stride, d_peaks, K, d_T, d_shift, V, d_out, d_log_sum, d_status, d_dir_status)) return rc;
  if (V == 0) return MFX_OK;
  if (int rc = w2_require_device(h->device)) return rc;
  W2Scratch sc(st);
  W2Args a{};
  if (int rc = sc.enqueue(h, d_Y, d_W, w_stride, d_peaks, K, V, d_dir_status, nullptr, nullptr, 0, a, st)) return rc;
  a.temp = d_T; a.shift = d_shift; a.out = d_out; a.log_sum = d_log_sum; a.status = d_status; a.partner = d_partner;
  return mode == W2_POST ? w2_soft_launch<W2_POST>(a, K, V, st) : w2_soft_launch<W2_PROF>(a, K, V, st);
}

// shared body of the posterior's and the profile's host entry points
int w2_soft_host(const char* fn, int mode, const mfx_rot2d* h, const double* Y, const double* W, int64_t w_stride, const double* peaks,
                 int K, const double* T, const double* shift, int64_t V, double* out, double* log_sum, int32_t* status, int32_t* partner,
                 int32_t* dir_status) {
  if (mfx_device_count() <= 0) return mfx_fail(MFX_ERR_NO_DEVICE, "%s", NO_DEVICE);
  if (int rc = w2_soft_check(fn, mode, h, Y, W, w_stride, peaks, K, T, shift, V, out, log_sum, status, dir_status)) return rc;
  if (V == 0) return MFX_OK;
  if (int rc = w2_require_device(h->device)) return rc;
  const bool post = mode == W2_POST;
  const size_t M = h->d.M, nout = (size_t)V * K * h->d.N, nw = w_stride ? (size_t)V * M : M;
  DevMem dY, dW, dpk, dT, dsh, dout, dls, dst, dpar, dds;
  HIPCHK(dY.alloc(sizeof(double) * V * M));
  HIPCHK(dW.alloc(sizeof(double) * nw));
  HIPCHK(dpk.alloc(sizeof(double) * V * 3 * K));
  HIPCHK(dT.alloc(sizeof(double) * V));
  HIPCHK(dsh.alloc(sizeof(double) * V));
  HIPCHK(dout.alloc(sizeof(double) * nout));
  HIPCHK(dls.alloc(sizeof(double) * V));
  HIPCHK(dst.alloc(sizeof(int32_t) * V));
  HIPCHK(dpar.alloc(partner ? sizeof(int32_t) * nout : 0));
  HIPCHK(dds.alloc(sizeof(int32_t) * 5 * V));
  HIPCHK(hipMemcpy(dY.p, Y, sizeof(double) * V * M, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(dW.p, W, sizeof(double) * nw, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(dpk.p, peaks, sizeof(double) * V * 3 * K, hipMemcpyHostToDevice));
  if (post) {
    HIPCHK(hipMemcpy(dT.p, T, sizeof(double) * V, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(dsh.p, shift, sizeof(double) * V, hipMemcpyHostToDevice));
  }
  if (int rc = w2_soft_enqueue(fn, mode, h, dY.as<double>(), dW.as<double>(), w_stride, dpk.as<double>(), K, dT.as<double>(), dsh.as<double>(),
                               V, dout.as<double>(), dls.as<double>(), dst.as<int32_t>(), partner ? dpar.as<int32_t>() : nullptr,
                               dds.as<int32_t>(), nullptr))
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

extern "C" int mfx_w2d_abi_version(void) { return 1; }

extern "C" void mfx_w2d_debug_set_force_explicit(int enabled) { g_force_explicit = enabled ? 1 : 0; }

extern "C" int mfx_w2d_max_atoms(void* hv, int what) {
  if (!hv) return 0;
  if (what == 0) return w2_fit_max_atoms();
  if (what == 1) return w2_soft_max_atoms(W2_POST);
  if (what == 2) return w2_soft_max_atoms(W2_PROF);
  return 0;
}

extern "C" int mfx_wfit2d_batch_dev(void* hv, const double* d_Y, const double* d_W, int64_t w_stride, const double* d_peaks, int maxfasc,
                                    int64_t V, double* d_params, int32_t* d_status, int32_t* d_wstatus, void* stream) {
  const char* fn = "mfx_wfit2d_batch_dev";
  if (mfx_device_count() <= 0) return mfx_fail(MFX_ERR_NO_DEVICE, "%s", NO_DEVICE);
  const mfx_rot2d* h = (const mfx_rot2d*)hv;
  if (!h || V < 0 || maxfasc < 0 || (V > 0 && (!d_Y || !d_W || !d_params || !d_status || !d_wstatus || (maxfasc > 0 && !d_peaks))))
    return mfx_fail(MFX_ERR_ARG, "%s: bad argument", fn);
  if (maxfasc > 3) return mfx_fail(MFX_ERR_UNSUPPORTED, "%s: at most 3 fascicles (got %d)", fn, maxfasc);
  if (int rc = w2_stride_check(fn, h, w_stride)) return rc;
  if (V == 0) return MFX_OK;
  if (int rc = w2_require_device(h->device)) return rc;
  return w2_class_dev(h, d_Y, d_W, w_stride, d_peaks, maxfasc, nullptr, maxfasc, 0, V, d_params, d_status, d_wstatus, (hipStream_t)stream);
}

extern "C" int mfx_wfit2d_batch(void* hv, const double* Y, const double* W, int64_t w_stride, const int32_t* K, const uint8_t* csf,
                                const double* peaks, int maxfasc, int csf_on, const double* sig_csf, int64_t V, double* params,
                                int32_t* status, int32_t* wstatus) {
  const char* fn = "mfx_wfit2d_batch";
  if (mfx_device_count() <= 0) return mfx_fail(MFX_ERR_NO_DEVICE, "%s", NO_DEVICE);
  const mfx_rot2d* h = (const mfx_rot2d*)hv;
  if (!h || V < 0 || maxfasc < 0 || (V > 0 && (!Y || !W || !K || !params || !status || !wstatus || (maxfasc > 0 && !peaks))))
    return mfx_fail(MFX_ERR_ARG, "%s: bad argument", fn);
  if (maxfasc > 3) return mfx_fail(MFX_ERR_UNSUPPORTED, "%s: at most 3 fascicles (got %d)", fn, maxfasc);
  if (int rc = w2_stride_check(fn, h, w_stride)) return rc;
  csf_on = csf_on != 0;
  const int M = h->d.M, np = 1 + 2 * maxfasc + csf_on + 2;
  // bin by class (K, CSF flag) before any device call
  std::vector<std::vector<int64_t>> bins((size_t)2 * (maxfasc + 1));
  for (int64_t v = 0; v < V; ++v) {
    const int c = csf && csf[v];
    if (K[v] < 0 || K[v] > maxfasc) return mfx_fail(MFX_ERR_ARG, "%s: K[%lld] = %d outside 0..%d", fn, (long long)v, K[v], maxfasc);
    if (c && (!csf_on || !sig_csf)) return mfx_fail(MFX_ERR_ARG, "%s: voxels flagged CSF need csf_on and sig_csf", fn);
    bins[(size_t)2 * K[v] + c].push_back(v);
  }
  if (V == 0) return MFX_OK;
  if (int rc = w2_require_device(h->device)) return rc;
  DevMem dxc, dWs;
  if (sig_csf) {
    HIPCHK(dxc.alloc(sizeof(double) * M));
    HIPCHK(hipMemcpy(dxc.p, sig_csf, sizeof(double) * M, hipMemcpyHostToDevice));
  }
  if (w_stride == 0) {   // the shared vector is uploaded once and read with stride 0
    HIPCHK(dWs.alloc(sizeof(double) * M));
    HIPCHK(hipMemcpy(dWs.p, W, sizeof(double) * M, hipMemcpyHostToDevice));
  }
  for (size_t b = 0; b < bins.size(); ++b) {
    const std::vector<int64_t>& ix = bins[b];
    if (ix.empty()) continue;
    const int k = (int)(b >> 1), c = (int)(b & 1);
    const size_t nv = ix.size();
    std::vector<double> Yc(nv * M), Wc(w_stride ? nv * M : 0), pc(nv * 3 * (size_t)std::max(k, 1)), prm(nv * np);
    std::vector<int32_t> stc(nv * 5), wsc(nv);
    for (size_t q = 0; q < nv; ++q) {
      std::memcpy(&Yc[q * M], Y + (size_t)ix[q] * M, sizeof(double) * M);
      if (w_stride) std::memcpy(&Wc[q * M], W + (size_t)ix[q] * M, sizeof(double) * M);
      if (k > 0) std::memcpy(&pc[q * 3 * k], peaks + (size_t)ix[q] * 3 * maxfasc, sizeof(double) * 3 * k);
    }
    DevMem dY, dW, dpk, dpr, dst, dws;
    HIPCHK(dY.alloc(sizeof(double) * Yc.size()));
    HIPCHK(dW.alloc(sizeof(double) * Wc.size()));
    HIPCHK(dpk.alloc(sizeof(double) * pc.size()));
    HIPCHK(dpr.alloc(sizeof(double) * prm.size()));
    HIPCHK(dst.alloc(sizeof(int32_t) * stc.size()));
    HIPCHK(dws.alloc(sizeof(int32_t) * wsc.size()));
    HIPCHK(hipMemcpy(dY.p, Yc.data(), sizeof(double) * Yc.size(), hipMemcpyHostToDevice));
    if (w_stride) HIPCHK(hipMemcpy(dW.p, Wc.data(), sizeof(double) * Wc.size(), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(dpk.p, pc.data(), sizeof(double) * pc.size(), hipMemcpyHostToDevice));
    if (int rc = w2_class_dev(h, dY.as<double>(), w_stride ? dW.as<double>() : dWs.as<double>(), w_stride, dpk.as<double>(), k,
                              c ? dxc.as<double>() : nullptr, maxfasc, csf_on, (int64_t)nv, dpr.as<double>(), dst.as<int32_t>(),
                              dws.as<int32_t>(), nullptr)) return rc;
    HIPCHK(hipStreamSynchronize(nullptr));
    HIPCHK(hipMemcpy(prm.data(), dpr.p, sizeof(double) * prm.size(), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(stc.data(), dst.p, sizeof(int32_t) * stc.size(), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(wsc.data(), dws.p, sizeof(int32_t) * wsc.size(), hipMemcpyDeviceToHost));
    for (size_t q = 0; q < nv; ++q) {
      std::memcpy(params + (size_t)ix[q] * np, &prm[q * np], sizeof(double) * np);
      std::memcpy(status + (size_t)ix[q] * 5, &stc[q * 5], sizeof(int32_t) * 5);
      wstatus[ix[q]] = wsc[q];
    }
  }
  return MFX_OK;
}

extern "C" int mfx_wpost2d_dev(void* hv, const double* d_Y, const double* d_W, int64_t w_stride, const double* d_peaks, int K,
                               const double* d_T, const double* d_shift, int64_t V, double* d_w, double* d_log_sum, int32_t* d_status,
                               int32_t* d_dir_status, void* stream) {
  return w2_soft_enqueue("mfx_wpost2d_dev", W2_POST, (const mfx_rot2d*)hv, d_Y, d_W, w_stride, d_peaks, K, d_T, d_shift, V, d_w, d_log_sum,
                         d_status, nullptr, d_dir_status, (hipStream_t)stream);
}

extern "C" int mfx_wpost2d(void* hv, const double* Y, const double* W, int64_t w_stride, const double* peaks, int K, const double* T,
                           const double* shift, int64_t V, double* w, double* log_sum, int32_t* status, int32_t* dir_status) {
  return w2_soft_host("mfx_wpost2d", W2_POST, (const mfx_rot2d*)hv, Y, W, w_stride, peaks, K, T, shift, V, w, log_sum, status, nullptr,
                      dir_status);
}

extern "C" int mfx_wprofile2d_dev(void* hv, const double* d_Y, const double* d_W, int64_t w_stride, const double* d_peaks, int K, int64_t V,
                                  double* d_obj, int32_t* d_partner, int32_t* d_dir_status, void* stream) {
  return w2_soft_enqueue("mfx_wprofile2d_dev", W2_PROF, (const mfx_rot2d*)hv, d_Y, d_W, w_stride, d_peaks, K, nullptr, nullptr, V, d_obj,
                         nullptr, nullptr, d_partner, d_dir_status, (hipStream_t)stream);
}

extern "C" int mfx_wprofile2d(void* hv, const double* Y, const double* W, int64_t w_stride, const double* peaks, int K, int64_t V,
                              double* obj, int32_t* partner, int32_t* dir_status) {
  return w2_soft_host("mfx_wprofile2d", W2_PROF, (const mfx_rot2d*)hv, Y, W, w_stride, peaks, K, nullptr, nullptr, V, obj, nullptr, nullptr,
                      partner, dir_status);
}
