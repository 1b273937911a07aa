// solve_soft.hip -- soft answers of the batched explicit-dictionary solver (include/mfx_solve_soft.h): per-atom
// objective profiles and posterior weights of V signals against the ONE dictionary of a mfx_solve handle.
//
// The handle owns G = A^T A (solve_batch.hip); sb_prep_kernel forms A^T y and ||y||^2 per signal (solve_shared.h: the
// solver's own kernel, the same bits).  The score of a pair, s = ||y||^2 - F, comes from the functions of soft_sweep.h
// (sweep_pair_frac; with a third column x sweep_primed and sweep_pair_w, the sign of w_x deciding as in posterior.hip).
// Per chunk of signals (scratch of the stream's arena, within the byte budget):
//   ss_tile_kernel<K3, MODE>   the geometry of sb_tile_kernel: a workgroup keeps a 64 x 64 tile of the cross block of G
//                      in LDS [row][column] (35 KiB with the waves' column results; no rel table), a lane is a column,
//                      wave w has rows w, w + 4, .., g11 / g13 of the rows in LDS and g22 / g23 / g33 in registers, and
//                      sweeps blockIdx.y, += gridDim.y over the chunk's signals.  With a third column the row operands of a signal (the primed
//                      statistics and inverses: two divisions a row) are formed once by the first 64 threads into LDS.
//                      MODE 0 / 1  the minimum pass: the maximum of s per row (wave butterfly, four rows sharing its
//                                  first exchanges; with the column index in MODE 1) and per column (over a wave's rows, then the four waves through LDS),
//                                  into the (signal, tile) partials
//                      MODE 2      the exponential pass: t = exp(fma(s - c0, 1 / T, 0)), c0 = ||y||^2 - shift, summed
//                                  the same way; a padded column adds an exact 0; an exponent above 700 raises the
//                                  signal's flag (a plain store of 1)
//   ss_prof_final_kernel  profile: one thread per atom combines the partials over the tiles in tile order (strictly
//                      greater wins: the lowest index on a tie), obj = ||y||^2 - max s
//   ss_post_head_kernel   posterior, one workgroup per signal: min F = ||y||^2 - max of the row partials (when the
//                      minimum pass ran), the shift (given, or min F), c0, 1 / T, the status (5 / 1 / 0), the flag zeroed
//   ss_post_reduce_kernel posterior, one workgroup per signal: R0 and R1 from the partials in tile order, Z over R0 in
//                      index order, normalisation, log_sum = log Z - shift / T, status 2 from the flag or a bad Z
//   ss_k1_prof_kernel, ss_k1_post_kernel   one sub-dictionary: one thread per (signal, atom)
// Every partial is written by exactly one thread and read after the kernel: no atomics at all.
#include "solve_shared.h"   // the handle, SbArgs, sb_prep_kernel, sb_args
#include "soft_sweep.h"     // the pair-scoring functions, MFX_PROFILE_CUT
#include "../../include/mfx_solve_soft.h"

#include <algorithm>
#include <cmath>

namespace {

constexpr double SS_EXP_MAX = 700.0;   // exponents above this make the shift unusable (status 2)
constexpr int SS_NONE = 0x7fffffff;    // index of "no pair yet"

struct SsArgs {
  const double* G;
  int N, n1, n2, tiles_r, tiles_c;
  long P;                  // partials of one signal: tiles_c * n1 row entries, then tiles_r * n2 column entries
  int Vc;
  const double* Aty;       // [Vc x N]
  const double* ysq;       // [Vc x 2]
  const int* skip;         // [Vc] signals the tile kernel passes over
  double* pval;            // [Vc x P]
  int* pidx;               // [Vc x P] (MODE 1)
  const double* c0;        // [Vc] (MODE 2)
  const double* iT;        // [Vc] (MODE 2)
  int* flag;               // [Vc] (MODE 2)
};

__device__ __forceinline__ bool ss_finite(double x) { return fabs(x) <= 1.79769313486231570815e308; }   // false for NaN
__device__ __forceinline__ double ss_nan() { return __longlong_as_double(0x7ff8000000000000LL); }
__device__ __forceinline__ double ss_ninf() { return __longlong_as_double((long long)0xfff0000000000000ULL); }

// one exchange of a row reduction: MODE 2 adds the partner's value, MODE 0 / 1 keep the greater one (MODE 1: with its
// index, the lower index on equal values)
template <int MODE>
__device__ __forceinline__ void ss_join(double& v, int& i, double ov, int oi) {
  if constexpr (MODE == 2) {
    v += ov;
  } else {
    const bool take = ov > v || (MODE == 1 && ov == v && oi < i);
    v = take ? ov : v;
    i = take ? oi : i;
  }
}
// the exchange at distance `off` for two rows at once: the lanes whose bit `off` is clear keep row a and send row b, the
// others keep b and send a; afterwards each half holds what a plain butterfly step leaves there for its row
template <int MODE>
__device__ __forceinline__ void ss_fold(bool hi, double a, int ai, double b, int bi, int off, double& v, int& i) {
  v = hi ? b : a;
  i = hi ? bi : ai;
  const double sv = hi ? a : b;
  const int si = hi ? ai : bi;
  ss_join<MODE>(v, i, __shfl_xor(sv, off), MODE == 1 ? __shfl_xor(si, off) : SS_NONE);
}

template <bool K3, int MODE>
__global__ __launch_bounds__(256) void ss_tile_kernel(SsArgs a) {
  __shared__ double s_g12[SB_T * SB_T];          // [row][column]
  __shared__ double s_g11[SB_T], s_g13[SB_T];
  __shared__ double s_row[K3 ? 5 * SB_T : 1];    // (K3) per signal: A11', Y1', 1 / A11', 1 / A11, X1 / xx of the rows
  __shared__ double s_cv[SB_WAVES * SB_T];       // the waves' column results
  __shared__ int s_ci[MODE == 1 ? SB_WAVES * SB_T : 1];
  const int tile = blockIdx.x, tr = tile / a.tiles_c, tc = tile - tr * a.tiles_c;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n1 = a.n1, n2 = a.n2, N = a.N;
  const int c3 = n1 + n2;   // (K3) the third column
  const int r0 = tr * SB_T, nr = min(SB_T, n1 - r0);   // the tile's rows r0 .. r0 + nr inside sub-dictionary 0
  const int j = tc * SB_T + lane;                       // the lane's column inside sub-dictionary 1
  const bool cv = j < n2;
  const int jc = n1 + (cv ? j : n2 - 1);                // its column of A (clamped: cv says whether it exists)
  const double* __restrict__ G = a.G;
  for (int r = wave; r < nr; r += SB_WAVES) s_g12[r * SB_T + lane] = G[(long)(r0 + r) * N + jc];
  if (threadIdx.x < nr) {
    s_g11[threadIdx.x] = G[(long)(r0 + threadIdx.x) * N + r0 + threadIdx.x];
    s_g13[threadIdx.x] = K3 ? G[(long)(r0 + threadIdx.x) * N + c3] : 0.0;
  }
  const double g22 = G[(long)jc * N + jc];
  const double g23 = K3 ? G[(long)jc * N + c3] : 0.0;
  const double g33 = K3 ? G[(long)c3 * N + c3] : 0.0;
  const double ixx = (K3 && g33 > 0.0) ? 1.0 / g33 : 0.0;
  const double i22u = (K3 && g22 > 0.0) ? 1.0 / g22 : 0.0;
  __syncthreads();
  const int nk = nr > wave ? (nr - wave + SB_WAVES - 1) / SB_WAVES : 0;   // rows of this wave: r = wave + 4 k, k < nk <= 16
  const bool b5 = (lane & 32) != 0, b4 = (lane & 16) != 0;
  // the row whose result this lane keeps: trip (lane & 15), row bit5 + 2 bit4 of the trip (beyond the tile from trip 4 on)
  const int myrow = wave + SB_WAVES * (4 * (lane & 15) + (b5 ? 1 : 0) + (b4 ? 2 : 0));
  for (int v = blockIdx.y; v < a.Vc; v += gridDim.y) {
    if (a.skip[v]) continue;           // (uniform over the workgroup)
    const double* __restrict__ aty = a.Aty + (size_t)v * N;
    const double y2 = aty[jc];
    const double xy = K3 ? aty[c3] : 0.0;
    const double sx = xy * xy * ixx;   // what x alone explains: ||y||^2 - ||y'||^2
    double A22p = 0.0, Y2p = 0.0, i22p = 0.0, p2 = 0.0;
    if constexpr (K3) {
      sweep_primed(g22, y2, g23, ixx, xy, A22p, Y2p, i22p);
      if (threadIdx.x < nr) {
        const double A = s_g11[threadIdx.x], X = s_g13[threadIdx.x];
        double Ap, Yp, iAp;
        sweep_primed(A, aty[r0 + threadIdx.x], X, ixx, xy, Ap, Yp, iAp);
        s_row[threadIdx.x] = Ap;
        s_row[SB_T + threadIdx.x] = Yp;
        s_row[2 * SB_T + threadIdx.x] = iAp;
        s_row[3 * SB_T + threadIdx.x] = A > 0.0 ? 1.0 / A : 0.0;
        s_row[4 * SB_T + threadIdx.x] = X * ixx;
      }
    } else {
      const double yp = fmax(y2, 0.0);
      p2 = yp * yp;
    }
    __syncthreads();   // the row operands are there; the previous signal's column results have been read
    double c0 = 0.0, iT = 0.0, emax = -SS_EXP_MAX;
    if constexpr (MODE == 2) { c0 = a.c0[v]; iT = a.iT[v]; }
    double keep = MODE == 2 ? 0.0 : ss_ninf(), cb = keep;   // this lane's row result, its column result over the wave's rows
    int keep_i = SS_NONE, cb_i = SS_NONE;
    // Four rows a trip.  Every row is reduced over the 64 lanes by the butterfly 32, 16, 8, 4, 2, 1; of the four rows'
    // first two exchanges only one half and one quarter of the lanes need the result, so the rows share them (ss_fold):
    // 7 exchanges for four rows, not 24, and the same operands in the same order as four plain butterflies.
#pragma unroll 1
    for (int g = 0; 4 * g < nk; ++g) {
      double t[4];
      int ti[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int k = 4 * g + q;
        const bool rv = k < nk;                               // (uniform over the wave) the row exists
        const int r = wave + SB_WAVES * (rv ? k : 4 * g);     // (a row that does not: the trip's first one, masked below)
        const double g11 = s_g11[r], g12 = s_g12[r * SB_T + lane], y1 = aty[r0 + r];
        double s;
        if constexpr (K3) {
          // x projected out: the two-variable form on the primed quantities, then the sign of w_x decides
          const double X1 = s_g13[r];
          double w1, w2, v1, v2;
          const double A12p = fma(-s_row[4 * SB_T + r], g23, g12);
          const double sp = sweep_pair_w(s_row[r], A22p, A12p, s_row[SB_T + r], Y2p, s_row[2 * SB_T + r], i22p, w1, w2);
          const double wxn = fma(-w2, g23, fma(-w1, X1, xy));   // w_x times x.x
          const double su = sweep_pair_w(g11, g22, g12, y1, y2, s_row[3 * SB_T + r], i22u, v1, v2);
          s = (wxn >= 0.0) ? sx + sp : su;
        } else {
          const double yp = fmax(y1, 0.0);
          double p, pq;
          sweep_pair_frac(g11, g22, g12, y1, y2, yp * yp, p2, p, pq);
          s = pq > 0.0 ? p / pq : 0.0;
        }
        const bool ok = rv && cv;
        if constexpr (MODE == 2) {
          const double e = fma(s - c0, iT, 0.0);
          emax = fmax(emax, ok ? e : emax);
          t[q] = ok ? exp(e) : 0.0;     // a padded column contributes nothing
          ti[q] = SS_NONE;
          if (rv) cb += t[q];           // increasing r
        } else {
          t[q] = ok ? s : ss_ninf();
          ti[q] = ok ? j : SS_NONE;
          if (ok && s > cb) { cb = s; cb_i = r0 + r; }   // increasing r: the lowest row on a tie
        }
      }
      double u0, u1, w;
      int i0, i1, wi;
      ss_fold<MODE>(b5, t[0], ti[0], t[1], ti[1], 32, u0, i0);   // lanes 0..31: row 0, lanes 32..63: row 1
      ss_fold<MODE>(b5, t[2], ti[2], t[3], ti[3], 32, u1, i1);   // rows 2 and 3
      ss_fold<MODE>(b4, u0, i0, u1, i1, 16, w, wi);              // lane bits (5, 4) -> row bit5 + 2 bit4 of the trip
#pragma unroll
      for (int o = 8; o > 0; o >>= 1) ss_join<MODE>(w, wi, __shfl_xor(w, o), MODE == 1 ? __shfl_xor(wi, o) : SS_NONE);
      if ((lane & 15) == g) { keep = w; keep_i = wi; }
    }
    double* __restrict__ pv = a.pval + (size_t)v * a.P;
    int* __restrict__ pi = MODE == 1 ? a.pidx + (size_t)v * a.P : nullptr;
    if (myrow < nr) {
      pv[(long)tc * n1 + r0 + myrow] = keep;
      if (MODE == 1) pi[(long)tc * n1 + r0 + myrow] = keep_i;
    }
    if (MODE == 2 && emax > SS_EXP_MAX) a.flag[v] = 1;
    s_cv[wave * SB_T + lane] = cb;
    if (MODE == 1) s_ci[wave * SB_T + lane] = cb_i;
    __syncthreads();
    if (wave == 0 && cv) {   // over the waves in wave order
      double c = s_cv[lane];
      int ci = MODE == 1 ? s_ci[lane] : SS_NONE;
      for (int w = 1; w < SB_WAVES; ++w) {
        const double o = s_cv[w * SB_T + lane];
        if constexpr (MODE == 2) {
          c += o;
        } else {
          const int oi = MODE == 1 ? s_ci[w * SB_T + lane] : SS_NONE;
          const bool take = o > c || (MODE == 1 && o == c && oi < ci);
          c = take ? o : c;
          ci = take ? oi : ci;
        }
      }
      const long at = (long)a.tiles_c * n1 + (long)tr * n2 + j;
      pv[at] = c;
      if (MODE == 1) pi[at] = ci;
    }
  }
}

// ---- profile: grid (ceil(max(n1, n2) / 256), Vc), thread t is atom t of both sub-dictionaries
struct SsProfOut { double* obj0; double* obj1; int* partner0; int* partner1; int* status; };
__global__ __launch_bounds__(256) void ss_prof_final_kernel(SsArgs a, SsProfOut o) {
  const int v = blockIdx.y, t = blockIdx.x * 256 + threadIdx.x;
  const int st = a.skip[v] ? 5 : 0;
  if (t == 0) o.status[v] = st;
  const double ysq = a.ysq[2 * (size_t)v];
  const double* __restrict__ pv = a.pval + (size_t)v * a.P;
  const int* __restrict__ pi = a.pidx + (size_t)v * a.P;
  if (t < a.n1) {
    double best = ss_ninf();
    int bi = -1;
    if (!st)
      for (int tc = 0; tc < a.tiles_c; ++tc) {   // the tiles' columns ascend: strictly greater keeps the lowest index
        const double s = pv[(long)tc * a.n1 + t];
        if (s > best) { best = s; bi = pi[(long)tc * a.n1 + t]; }
      }
    o.obj0[(size_t)v * a.n1 + t] = st ? ss_nan() : ysq - best;
    if (o.partner0) o.partner0[(size_t)v * a.n1 + t] = bi;
  }
  if (t < a.n2) {
    const long base = (long)a.tiles_c * a.n1;
    double best = ss_ninf();
    int bi = -1;
    if (!st)
      for (int tr = 0; tr < a.tiles_r; ++tr) {
        const double s = pv[base + (long)tr * a.n2 + t];
        if (s > best) { best = s; bi = pi[base + (long)tr * a.n2 + t]; }
      }
    o.obj1[(size_t)v * a.n2 + t] = st ? ss_nan() : ysq - best;
    if (o.partner1) o.partner1[(size_t)v * a.n2 + t] = bi;
  }
}

// ---- posterior
struct SsPostArgs {
  const double* T; const double* shift;   // [Vc]; shift null: the signal's own min F
  const int* pst;                         // [Vc] sb_prep_kernel's status
  int have_min;                           // the minimum pass ran: the row partials hold the maxima of s
  double* c0; double* iT; double* shf;    // [Vc] scratch
  int* flag;                              // [Vc] scratch
  double* w0; double* w1; double* log_sum; double* minF; int* status;
};
// one workgroup per signal
__global__ __launch_bounds__(256) void ss_post_head_kernel(SsArgs a, SsPostArgs p) {
  __shared__ double s_m[256];
  const int v = blockIdx.x, tid = threadIdx.x;
  const int bad = p.pst[v];
  double m = ss_ninf();
  if (p.have_min && !bad) {
    const double* __restrict__ pv = a.pval + (size_t)v * a.P;
    const long nrow = (long)a.tiles_c * a.n1;
    for (long k = tid; k < nrow; k += 256) m = fmax(m, pv[k]);
  }
  s_m[tid] = m;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) s_m[tid] = fmax(s_m[tid], s_m[tid + o]);
    __syncthreads();
  }
  if (tid == 0) {
    const double ysq = a.ysq[2 * (size_t)v];
    const double minF = (bad || !p.have_min) ? ss_nan() : ysq - s_m[0];
    if (p.minF && p.have_min) p.minF[v] = minF;
    const double Tv = p.T[v];
    const double sh = p.shift ? p.shift[v] : minF;
    const int st = bad ? 5 : ((!(Tv > 0.0) || !ss_finite(Tv) || !ss_finite(sh)) ? 1 : 0);
    p.status[v] = st;
    p.shf[v] = sh;
    p.c0[v] = ysq - sh;        // exponent of a pair: (score - c0) / T = -(F - shift) / T
    p.iT[v] = 1.0 / Tv;
    p.flag[v] = 0;
  }
}
__device__ __forceinline__ void ss_nan_rows(const SsArgs& a, const SsPostArgs& p, int v, int tid) {
  for (int n = tid; n < a.n1; n += 256) p.w0[(size_t)v * a.n1 + n] = ss_nan();
  if (p.w1)
    for (int n = tid; n < a.n2; n += 256) p.w1[(size_t)v * a.n2 + n] = ss_nan();
  if (tid == 0) p.log_sum[v] = ss_nan();
}
// one workgroup per signal; the unnormalised sums wait in the output rows for Z
__global__ __launch_bounds__(256) void ss_post_reduce_kernel(SsArgs a, SsPostArgs p) {
  const int v = blockIdx.x, tid = threadIdx.x;
  if (p.status[v]) { ss_nan_rows(a, p, v, tid); return; }
  const double* __restrict__ pv = a.pval + (size_t)v * a.P;
  double* w0 = p.w0 + (size_t)v * a.n1;
  double* w1 = p.w1 + (size_t)v * a.n2;
  for (int i = tid; i < a.n1; i += 256) {
    double s = 0.0;
    for (int tc = 0; tc < a.tiles_c; ++tc) s += pv[(long)tc * a.n1 + i];
    w0[i] = s;
  }
  const long base = (long)a.tiles_c * a.n1;
  for (int j = tid; j < a.n2; j += 256) {
    double s = 0.0;
    for (int tr = 0; tr < a.tiles_r; ++tr) s += pv[base + (long)tr * a.n2 + j];
    w1[j] = s;
  }
  __syncthreads();
  double Z = 0.0;   // in index order (every thread, the same value)
  for (int i = 0; i < a.n1; ++i) Z += ((volatile double*)w0)[i];
  __syncthreads();
  if (p.flag[v] != 0 || !(Z > 0.0) || !ss_finite(Z)) {
    ss_nan_rows(a, p, v, tid);
    if (tid == 0) p.status[v] = 2;
    return;
  }
  for (int i = tid; i < a.n1; i += 256) w0[i] = w0[i] / Z;
  for (int j = tid; j < a.n2; j += 256) w1[j] = w1[j] / Z;
  if (tid == 0) p.log_sum[v] = log(Z) - p.shf[v] / p.T[v];
}

// ---- one sub-dictionary: s(i) = max(Y_i, 0)^2 / A_ii
__device__ __forceinline__ double ss_k1_score(const double* __restrict__ G, int N, const double* __restrict__ aty, int i) {
  const double A = G[(long)i * N + i];
  const double yp = fmax(aty[i], 0.0);
  return A > 0.0 ? yp * yp / A : 0.0;
}
__global__ __launch_bounds__(256) void ss_k1_prof_kernel(SsArgs a, SsProfOut o) {
  const int v = blockIdx.y, t = blockIdx.x * 256 + threadIdx.x;
  const int st = a.skip[v] ? 5 : 0;
  if (t == 0) o.status[v] = st;
  if (t >= a.n1) return;
  o.obj0[(size_t)v * a.n1 + t] = st ? ss_nan() : a.ysq[2 * (size_t)v] - ss_k1_score(a.G, a.N, a.Aty + (size_t)v * a.N, t);
  if (o.partner0) o.partner0[(size_t)v * a.n1 + t] = -1;
}
// one workgroup per signal
__global__ __launch_bounds__(256) void ss_k1_post_kernel(SsArgs a, SsPostArgs p) {
  __shared__ double s_m[256];
  __shared__ int s_over;
  const int v = blockIdx.x, tid = threadIdx.x;
  const int bad = p.pst[v];
  const double* __restrict__ aty = a.Aty + (size_t)v * a.N;
  if (tid == 0) s_over = 0;
  double m = ss_ninf();
  if (!bad)
    for (int i = tid; i < a.n1; i += 256) m = fmax(m, ss_k1_score(a.G, a.N, aty, i));
  s_m[tid] = m;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) s_m[tid] = fmax(s_m[tid], s_m[tid + o]);
    __syncthreads();
  }
  const double ysq = a.ysq[2 * (size_t)v];
  const double minF = bad ? ss_nan() : ysq - s_m[0];
  if (tid == 0 && p.minF) p.minF[v] = minF;
  const double Tv = p.T[v];
  const double sh = p.shift ? p.shift[v] : minF;
  const int st = bad ? 5 : ((!(Tv > 0.0) || !ss_finite(Tv) || !ss_finite(sh)) ? 1 : 0);
  if (st) {
    ss_nan_rows(a, p, v, tid);
    if (tid == 0) p.status[v] = st;
    return;
  }
  const double c0 = ysq - sh, iT = 1.0 / Tv;
  double* w0 = p.w0 + (size_t)v * a.n1;
  bool over = false;
  for (int i = tid; i < a.n1; i += 256) {
    const double e = fma(ss_k1_score(a.G, a.N, aty, i) - c0, iT, 0.0);
    over |= e > SS_EXP_MAX;
    w0[i] = exp(e);
  }
  if (over) s_over = 1;
  __syncthreads();
  double Z = 0.0;   // in index order (every thread, the same value)
  for (int i = 0; i < a.n1; ++i) Z += ((volatile double*)w0)[i];
  __syncthreads();
  if (s_over != 0 || !(Z > 0.0) || !ss_finite(Z)) {
    ss_nan_rows(a, p, v, tid);
    if (tid == 0) p.status[v] = 2;
    return;
  }
  for (int i = tid; i < a.n1; i += 256) w0[i] = w0[i] / Z;
  if (tid == 0) {
    p.log_sum[v] = log(Z) - sh / Tv;
    p.status[v] = 0;
  }
}

// ---- host
bool ss_served(const mfx_solve* h) { return h->Kp == 1 || h->Kp == 2 || (h->Kp == 3 && h->sizes[2] == 1); }
int ss_unserved(const char* fn, const mfx_solve* h) {
  std::string s;
  for (int k = 0; k < h->Kp; ++k) s += (k ? ", " : "") + std::to_string(h->sizes[k]);
  return mfx_fail(MFX_ERR_UNSUPPORTED,
                  "%s: sub-dictionaries of sizes [%s] are not served: one or two sub-dictionaries, or three whose last has "
                  "one column (three general sub-dictionaries and four or more are out of scope)", fn, s.c_str());
}
long ss_partials(const mfx_solve* h) {
  return h->Kp == 1 ? 0 : h->tiles_c * h->sizes[0] + h->tiles_r * h->sizes[1];
}
int64_t ss_bytes_per_signal(const mfx_solve* h, int what) {
  return 8 * ((int64_t)h->Ntot + 8) + (what == MFX_SOLVE_SOFT_PROFILE ? 12 : 8) * (int64_t)ss_partials(h);
}

// the chunk's scratch and the arguments both calls share
struct SsChunk {
  StreamMem Aty, ysq, smax, ncand, pst, pval, pidx, c0, iT, shf, flag;
  explicit SsChunk(hipStream_t st) : Aty(st), ysq(st), smax(st), ncand(st), pst(st), pval(st), pidx(st), c0(st), iT(st), shf(st), flag(st) {}
  SbArgs b{};
  SsArgs a{};
  int alloc(const mfx_solve* h, int64_t Vc, bool idx, bool post) {
    const size_t n = (size_t)Vc, P = (size_t)ss_partials(h);
    HIPCHK(Aty.alloc(sizeof(double) * n * h->Ntot));
    HIPCHK(ysq.alloc(sizeof(double) * 2 * n));
    HIPCHK(smax.alloc(sizeof(unsigned long long) * n));
    HIPCHK(ncand.alloc(sizeof(int) * n));
    HIPCHK(pst.alloc(sizeof(int) * n));
    if (P) HIPCHK(pval.alloc(sizeof(double) * n * P));
    if (P && idx) HIPCHK(pidx.alloc(sizeof(int) * n * P));
    if (post) {
      HIPCHK(c0.alloc(sizeof(double) * n));
      HIPCHK(iT.alloc(sizeof(double) * n));
      HIPCHK(shf.alloc(sizeof(double) * n));
      HIPCHK(flag.alloc(sizeof(int) * n));
    }
    b = sb_args(h);
    b.Aty = Aty.as<double>(); b.ysq = ysq.as<double>(); b.smax = smax.as<unsigned long long>(); b.ncand = ncand.as<int>();
    b.status = pst.as<int>();
    a.G = b.G; a.N = h->Ntot; a.n1 = (int)h->sizes[0]; a.n2 = h->Kp > 1 ? (int)h->sizes[1] : 0;
    a.tiles_r = (int)h->tiles_r; a.tiles_c = (int)h->tiles_c; a.P = (long)P;
    a.Aty = b.Aty; a.ysq = b.ysq; a.skip = b.status;
    a.pval = pval.as<double>(); a.pidx = pidx.as<int>();
    a.c0 = c0.as<double>(); a.iT = iT.as<double>(); a.flag = flag.as<int>();
    return MFX_OK;
  }
  // A^T y, ||y||^2 and the non-finite test of the signals Y [nv x M]
  int prep(const mfx_solve* h, const double* Y, int nv, hipStream_t st) {
    b.Y = Y; b.Vc = nv; a.Vc = nv;
    hipLaunchKernelGGL(sb_prep_kernel, dim3((unsigned)((h->Ntot + 255) / 256 + 1), (unsigned)nv), dim3(256), 0, st, b);
    HIPCHK(hipGetLastError());
    return MFX_OK;
  }
};

template <int MODE>
int ss_tiles(const mfx_solve* h, const SsArgs& a, hipStream_t st) {
  const long ntiles = h->tiles_r * h->tiles_c;
  // enough workgroups to fill the device: the signals of the chunk are dealt to gridDim.y sweeps of every tile
  const unsigned ny = (unsigned)std::max<long>(1, std::min<long>(a.Vc, (2048 + ntiles - 1) / ntiles));
  const dim3 g((unsigned)ntiles, ny);
  if (h->Kp == 3) hipLaunchKernelGGL((ss_tile_kernel<true, MODE>), g, dim3(256), 0, st, a);
  else hipLaunchKernelGGL((ss_tile_kernel<false, MODE>), g, dim3(256), 0, st, a);
  HIPCHK(hipGetLastError());
  return MFX_OK;
}

// the checks both device entry points share, in their order; *run = false: V == 0
int ss_head(const char* fn, const mfx_solve* h, int64_t V, bool ptrs, bool second, bool* run) {
  *run = false;
  if (mfx_device_count() <= 0) return mfx_no_device();
  if (!h || V < 0) return mfx_fail(MFX_ERR_ARG, "%s: bad argument", fn);
  if (!ss_served(h)) return ss_unserved(fn, h);
  if (V > 0 && !ptrs) return mfx_fail(MFX_ERR_ARG, "%s: bad argument", fn);
  if (h->Kp == 1 && second) return mfx_fail(MFX_ERR_ARG, "%s: one sub-dictionary has no second set of outputs", fn);
  if (V == 0) return MFX_OK;
  if (int rc = mfx_require_device(h->device)) return rc;
  *run = true;
  return MFX_OK;
}
int64_t ss_chunk(const mfx_solve* h, int what, int64_t V, int64_t max_bytes) {
  if (max_bytes <= 0) max_bytes = SB_DEFAULT_BYTES;
  return std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(V, MFX_SS_SIGNALS_PER_LAUNCH), max_bytes / ss_bytes_per_signal(h, what)));
}

}  // namespace

extern "C" int mfx_solve_soft_abi_version(void) { return 1; }

extern "C" int mfx_solve_soft_served(const void* hv) {
  const mfx_solve* h = (const mfx_solve*)hv;
  if (!h) return mfx_fail(MFX_ERR_ARG, "mfx_solve_soft_served: bad argument");
  return ss_served(h) ? MFX_OK : ss_unserved("mfx_solve_soft_served", h);
}

extern "C" int64_t mfx_solve_soft_bytes_per_signal(const void* hv, int what) {
  const mfx_solve* h = (const mfx_solve*)hv;
  if (!h || !ss_served(h) || (what != MFX_SOLVE_SOFT_PROFILE && what != MFX_SOLVE_SOFT_POST)) return -1;
  return ss_bytes_per_signal(h, what);
}

extern "C" int mfx_solve_profile_dev(void* hv, const double* d_Y, int64_t V, int64_t max_bytes, double* d_obj0, double* d_obj1,
                                     int32_t* d_partner0, int32_t* d_partner1, int32_t* d_status, void* stream) {
  const mfx_solve* h = (const mfx_solve*)hv;
  bool run;
  const bool two = h && h->Kp > 1;
  const bool ptrs = d_Y && d_obj0 && d_status && (!two || (d_obj1 && !d_partner0 == !d_partner1));
  if (int rc = ss_head("mfx_solve_profile_dev", h, V, ptrs, d_obj1 || d_partner1, &run)) return rc;
  if (!run) return MFX_OK;
  hipStream_t st = (hipStream_t)stream;
  const int64_t Vc = ss_chunk(h, MFX_SOLVE_SOFT_PROFILE, V, max_bytes);
  SsChunk c(st);
  if (int rc = c.alloc(h, Vc, true, false)) return rc;
  const int n1 = c.a.n1, n2 = c.a.n2;
  for (int64_t v0 = 0; v0 < V; v0 += Vc) {
    const int nv = (int)std::min<int64_t>(Vc, V - v0);
    if (int rc = c.prep(h, d_Y + (size_t)v0 * h->M, nv, st)) return rc;
    SsProfOut o{d_obj0 + (size_t)v0 * n1, two ? d_obj1 + (size_t)v0 * n2 : nullptr, d_partner0 ? d_partner0 + (size_t)v0 * n1 : nullptr,
                (two && d_partner1) ? d_partner1 + (size_t)v0 * n2 : nullptr, d_status + v0};
    if (!two) {
      hipLaunchKernelGGL(ss_k1_prof_kernel, dim3((unsigned)((n1 + 255) / 256), (unsigned)nv), dim3(256), 0, st, c.a, o);
    } else {
      if (int rc = ss_tiles<1>(h, c.a, st)) return rc;
      hipLaunchKernelGGL(ss_prof_final_kernel, dim3((unsigned)((std::max(n1, n2) + 255) / 256), (unsigned)nv), dim3(256), 0, st, c.a, o);
    }
    HIPCHK(hipGetLastError());
  }
  return MFX_OK;
}

extern "C" int mfx_solve_profile(void* hv, const double* Y, int64_t V, int64_t max_bytes, double* obj0, double* obj1,
                                 int32_t* partner0, int32_t* partner1, int32_t* status) {
  const mfx_solve* h = (const mfx_solve*)hv;
  bool run;
  const bool two = h && h->Kp > 1;
  const bool ptrs = Y && obj0 && status && (!two || (obj1 && !partner0 == !partner1));
  if (int rc = ss_head("mfx_solve_profile", h, V, ptrs, obj1 || partner1, &run)) return rc;
  if (!run) return MFX_OK;
  const size_t n = (size_t)V, n1 = (size_t)h->sizes[0], n2 = two ? (size_t)h->sizes[1] : 0;
  DevBuf<double> dY, do0, do1;
  DevBuf<int32_t> dp0, dp1, dst;
  HIPCHK(dY.upload(Y, n * h->M));
  HIPCHK(do0.alloc_n(n * n1));
  HIPCHK(dst.alloc_n(n));
  if (two) HIPCHK(do1.alloc_n(n * n2));
  if (partner0) HIPCHK(dp0.alloc_n(n * n1));
  if (partner1) HIPCHK(dp1.alloc_n(n * n2));
  if (int rc = mfx_solve_profile_dev(hv, dY.get(), V, max_bytes, do0.get(), two ? do1.get() : nullptr, partner0 ? dp0.get() : nullptr,
                                     partner1 ? dp1.get() : nullptr, dst.get(), nullptr)) return rc;
  HIPCHK(hipStreamSynchronize(nullptr));
  HIPCHK(do0.download(obj0));
  HIPCHK(dst.download(status));
  if (two) HIPCHK(do1.download(obj1));
  if (partner0) HIPCHK(dp0.download(partner0));
  if (partner1) HIPCHK(dp1.download(partner1));
  return MFX_OK;
}

extern "C" int mfx_solve_post_dev(void* hv, const double* d_Y, int64_t V, const double* d_T, const double* d_shift, int64_t max_bytes,
                                  double* d_w0, double* d_w1, double* d_log_sum, double* d_minF, int32_t* d_status, void* stream) {
  const mfx_solve* h = (const mfx_solve*)hv;
  bool run;
  const bool two = h && h->Kp > 1;
  const bool ptrs = d_Y && d_T && d_w0 && d_log_sum && d_status && (!two || d_w1);
  if (int rc = ss_head("mfx_solve_post_dev", h, V, ptrs, d_w1 != nullptr, &run)) return rc;
  if (!run) return MFX_OK;
  hipStream_t st = (hipStream_t)stream;
  const int64_t Vc = ss_chunk(h, MFX_SOLVE_SOFT_POST, V, max_bytes);
  SsChunk c(st);
  if (int rc = c.alloc(h, Vc, false, true)) return rc;
  const int n1 = c.a.n1, n2 = c.a.n2;
  for (int64_t v0 = 0; v0 < V; v0 += Vc) {
    const int nv = (int)std::min<int64_t>(Vc, V - v0);
    if (int rc = c.prep(h, d_Y + (size_t)v0 * h->M, nv, st)) return rc;
    SsPostArgs p{};
    p.T = d_T + v0; p.shift = d_shift ? d_shift + v0 : nullptr; p.pst = c.b.status;
    p.have_min = (!d_shift || d_minF) ? 1 : 0;
    p.c0 = c.c0.as<double>(); p.iT = c.iT.as<double>(); p.shf = c.shf.as<double>(); p.flag = c.flag.as<int>();
    p.w0 = d_w0 + (size_t)v0 * n1; p.w1 = two ? d_w1 + (size_t)v0 * n2 : nullptr;
    p.log_sum = d_log_sum + v0; p.minF = d_minF ? d_minF + v0 : nullptr; p.status = d_status + v0;
    if (!two) {
      hipLaunchKernelGGL(ss_k1_post_kernel, dim3((unsigned)nv), dim3(256), 0, st, c.a, p);
      HIPCHK(hipGetLastError());
      continue;
    }
    c.a.skip = c.b.status;
    if (p.have_min)
      if (int rc = ss_tiles<0>(h, c.a, st)) return rc;
    hipLaunchKernelGGL(ss_post_head_kernel, dim3((unsigned)nv), dim3(256), 0, st, c.a, p);
    HIPCHK(hipGetLastError());
    c.a.skip = p.status;   // the exponential pass: only the signals whose T and shift are usable
    if (int rc = ss_tiles<2>(h, c.a, st)) return rc;
    hipLaunchKernelGGL(ss_post_reduce_kernel, dim3((unsigned)nv), dim3(256), 0, st, c.a, p);
    HIPCHK(hipGetLastError());
  }
  return MFX_OK;
}

extern "C" int mfx_solve_post(void* hv, const double* Y, int64_t V, const double* T, const double* shift, int64_t max_bytes,
                              double* w0, double* w1, double* log_sum, double* minF, int32_t* status) {
  const mfx_solve* h = (const mfx_solve*)hv;
  bool run;
  const bool two = h && h->Kp > 1;
  const bool ptrs = Y && T && w0 && log_sum && status && (!two || w1);
  if (int rc = ss_head("mfx_solve_post", h, V, ptrs, w1 != nullptr, &run)) return rc;
  if (!run) return MFX_OK;
  const size_t n = (size_t)V, n1 = (size_t)h->sizes[0], n2 = two ? (size_t)h->sizes[1] : 0;
  DevBuf<double> dY, dT, dsh, dw0, dw1, dls, dmf;
  DevBuf<int32_t> dst;
  HIPCHK(dY.upload(Y, n * h->M));
  HIPCHK(dT.upload(T, n));
  if (shift) HIPCHK(dsh.upload(shift, n));
  HIPCHK(dw0.alloc_n(n * n1));
  if (two) HIPCHK(dw1.alloc_n(n * n2));
  HIPCHK(dls.alloc_n(n));
  if (minF) HIPCHK(dmf.alloc_n(n));
  HIPCHK(dst.alloc_n(n));
  if (int rc = mfx_solve_post_dev(hv, dY.get(), V, dT.get(), shift ? dsh.get() : nullptr, max_bytes, dw0.get(), two ? dw1.get() : nullptr,
                                  dls.get(), minF ? dmf.get() : nullptr, dst.get(), nullptr)) return rc;
  HIPCHK(hipStreamSynchronize(nullptr));
  HIPCHK(dw0.download(w0));
  if (two) HIPCHK(dw1.download(w1));
  HIPCHK(dls.download(log_sum));
  if (minF) HIPCHK(dmf.download(minF));
  HIPCHK(dst.download(status));
  return MFX_OK;
}
