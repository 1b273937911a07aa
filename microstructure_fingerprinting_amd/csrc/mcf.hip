// mcf.hip -- MCF signal synthesis (include/mfx_mcf.h; reference mcf.py:83-426).
//
// One work item is one (atom, protocol row).  With p = D T / L^2, q = gamma T L G_perp and tau = delta / T,
// the reference forms R = expm(-(p Lam - i q B) tau) diag(d) expm(-(p Lam + i q B) tau) and keeps |R[0,0]|.
// Lam is diagonal and B real symmetric, so with X = expm(A), A = -tau (p Lam + i q B), the left factor is
// conj(X): one matrix exponential per encoding block instead of two, and only products of X with vectors
// afterwards.  X is computed the way scipy.linalg.expm does for large norms: Pade [13/13] on A / 2^s
// (Higham 2005, the m = 13 branch of Al-Mohy & Higham 2009) and s squarings, in FP64, padded to 64 x 64.
//
// One 256-thread workgroup owns one item at a time (persistent grid, one workgroup per CU):
//   - complex 64 x 64 products on v_mfma_f64_16x16x4_f64: both operands staged in LDS (4 planes of
//     64 x 65 doubles, 133 KiB), wave w computes rows 16w..16w+15 (four 16 x 16 tiles, real and imaginary
//     accumulators: 32 doubles per lane);
//   - the Pade solve (V - U) X = (V + U): Gauss-Jordan with partial pivoting on the same 4 LDS planes;
//   - the matrices that live across products (A, A^2, A^4, A^6 and two temporaries, 384 KiB per
//     workgroup) stay in a global workspace that only this workgroup touches (L2-resident).
#include "mfx_host.h"
#include "../../include/mfx_mcf.h"

#include <cmath>
#include <vector>

namespace {

constexpr int MCF_N = 64;                   // padded matrix size
constexpr int MCF_LD = 65;                  // LDS row stride in doubles (breaks the column-read bank pattern)
constexpr int MCF_PLANE = MCF_N * MCF_LD;   // one LDS plane
constexpr int MCF_MAT = 2 * MCF_N * MCF_N;  // one planar complex matrix in the workspace: [re 4096][im 4096]
constexpr int MCF_NMAT = 6;
constexpr int MCF_THREADS = 256;
constexpr int MCF_VEC = 8 * MCF_N;          // LDS vectors after the planes: 4 complex vectors
constexpr size_t MCF_LDS_BYTES = (size_t)(4 * MCF_PLANE + MCF_VEC + 8) * sizeof(double);
constexpr double MCF_THETA13 = 5.371920351148152;   // Higham 2005, Table 2.3 (scipy's theta_13)

typedef double mcf_d4 __attribute__((ext_vector_type(4)));

struct McfRow {        // per protocol row, direction-resolved on the host
  double T;            // total encoding time (Delta + delta, or the DDE sum)
  double tmix;         // DDE mixing time
  double Gperp[2], Gpar[2], Del[2], del[2];
  int kind;            // 0: E = 1 (no gradient), 1: E = E_par (no perpendicular gradient), 2: matrix work
  int pad;
};

struct McfArgs {
  const double* lam;      // [64] zero padded
  const double* B;        // [64 x 64] zero padded
  const double* colsum;   // [64] sum_{i != j} |B_ij|
  const McfRow* rows;     // [n_seq]
  const int* act;         // [n_act] rows of kind 2
  int n_act, n_seq, M, nblk;
  long n_atoms;
  const double* L;
  const double* diff;
  double gamma;
  double* E;              // [n_seq x n_atoms]
  double* work;           // [gridDim.x x MCF_NMAT x MCF_MAT]
};

__device__ __forceinline__ double mcf_bpar(const McfRow& r, int b, double gamma) {
  const double t = gamma * r.del[b] * r.Gpar[b];
  return t * t * (r.Del[b] - r.del[b] / 3.0);
}
__device__ __forceinline__ double mcf_epar(const McfRow& r, int nblk, double gamma, double D) {
  double b = mcf_bpar(r, 0, gamma);
  if (nblk == 2) b = b + mcf_bpar(r, 1, gamma);
  return exp(-b * D);
}

// closed-form items: rows without gradient (E = 1) or without a perpendicular component (E = E_par)
__global__ void mfx_mcf_closed_kernel(McfArgs a) {
  const long n = (long)a.n_seq * a.n_atoms;
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (long)gridDim.x * blockDim.x) {
    const int r = (int)(e / a.n_atoms);
    const long at = e - (long)r * a.n_atoms;
    const McfRow row = a.rows[r];
    if (row.kind == 0) a.E[e] = 1.0;
    else if (row.kind == 1) a.E[e] = mcf_epar(row, a.nblk, a.gamma, a.diff[at]);
  }
}

// C = X Y (complex 64 x 64, planar).  Both operands are staged in LDS first, so C may alias X or Y.
__device__ __noinline__ void mcf_gemm(double* __restrict__ S, double* C, const double* X, const double* Y) {
  const int tid = threadIdx.x;
  __syncthreads();   // previous writes of the workspace visible, previous LDS readers done
  for (int e = tid; e < MCF_N * MCF_N; e += MCF_THREADS) {
    const int r = e >> 6, c = e & 63;
    S[0 * MCF_PLANE + r * MCF_LD + c] = X[e];
    S[1 * MCF_PLANE + r * MCF_LD + c] = X[MCF_N * MCF_N + e];
    S[2 * MCF_PLANE + r * MCF_LD + c] = Y[e];
    S[3 * MCF_PLANE + r * MCF_LD + c] = Y[MCF_N * MCF_N + e];
  }
  __syncthreads();
  const int wave = tid >> 6, lane = tid & 63;
  const int arow = 16 * wave + (lane & 15), kq = lane >> 4, bcol = lane & 15;
  mcf_d4 cr[4], ci[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) { cr[t] = mcf_d4{0.0, 0.0, 0.0, 0.0}; ci[t] = cr[t]; }
  const double* Xr = S;
  const double* Xi = S + MCF_PLANE;
  const double* Yr = S + 2 * MCF_PLANE;
  const double* Yi = S + 3 * MCF_PLANE;
#pragma unroll 2
  for (int k4 = 0; k4 < MCF_N / 4; ++k4) {
    const int k = 4 * k4 + kq;
    const double ar = Xr[arow * MCF_LD + k];
    const double ai = Xi[arow * MCF_LD + k];
    const double nai = -ai;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const double br = Yr[k * MCF_LD + 16 * t + bcol];
      const double bi = Yi[k * MCF_LD + 16 * t + bcol];
      cr[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(ar, br, cr[t], 0, 0, 0);
      cr[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(nai, bi, cr[t], 0, 0, 0);
      ci[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(ar, bi, ci[t], 0, 0, 0);
      ci[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(ai, br, ci[t], 0, 0, 0);
    }
  }
  // C/D layout of the f64 16x16x4 MFMA: col = lane & 15, row = (lane >> 4) + 4 * reg
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int r = 16 * wave + (lane >> 4) + 4 * j, c = 16 * t + (lane & 15);
      C[r * MCF_N + c] = cr[t][j];
      C[MCF_N * MCF_N + r * MCF_N + c] = ci[t][j];
    }
}

// D = (acc ? acc : 0) + c6 P6 + c4 P4 + c2 P2 + c0 I   (left to right, as scipy's pade13 sums)
__device__ __noinline__ void mcf_comb(double* D, const double* acc, const double* P6, const double* P4, const double* P2, double c6,
                         double c4, double c2, double c0) {
  __syncthreads();
  for (int e = threadIdx.x; e < MCF_MAT; e += MCF_THREADS) {
    double v = c6 * P6[e];
    if (acc) v = acc[e] + v;
    v = v + c4 * P4[e];
    v = v + c2 * P2[e];
    if (c0 != 0.0 && e < MCF_N * MCF_N && (e >> 6) == (e & 63)) v = v + c0;
    D[e] = v;
  }
}

// X = (V - U)^-1 (V + U): Gauss-Jordan with partial pivoting (|re| + |im|, as LAPACK's izamax) in LDS.
__device__ __noinline__ void mcf_solve(double* __restrict__ S, double* X, const double* U, const double* V) {
  const int tid = threadIdx.x;
  double* Qr = S;
  double* Qi = S + MCF_PLANE;
  double* Pr = S + 2 * MCF_PLANE;
  double* Pi = S + 3 * MCF_PLANE;
  double* fr = S + 4 * MCF_PLANE;   // elimination factors of the current column
  double* fi = fr + MCF_N;
  double* piv = S + 4 * MCF_PLANE + MCF_VEC;
  __syncthreads();
  for (int e = tid; e < MCF_N * MCF_N; e += MCF_THREADS) {
    const int r = e >> 6, c = e & 63;
    const double ur = U[e], ui = U[MCF_N * MCF_N + e], vr = V[e], vi = V[MCF_N * MCF_N + e];
    Qr[r * MCF_LD + c] = -ur + vr;
    Qi[r * MCF_LD + c] = -ui + vi;
    Pr[r * MCF_LD + c] = ur + vr;
    Pi[r * MCF_LD + c] = ui + vi;
  }
  __syncthreads();
  for (int k = 0; k < MCF_N; ++k) {
    if (tid < 64) {   // pivot search on wave 0: largest |re| + |im| in rows k..63, lowest row on ties
      double v = (tid >= k) ? fabs(Qr[tid * MCF_LD + k]) + fabs(Qi[tid * MCF_LD + k]) : -1.0;
      int idx = tid;
#pragma unroll
      for (int off = 32; off >= 1; off >>= 1) {
        const double ov = __shfl_xor(v, off);
        const int oi = __shfl_xor(idx, off);
        if (ov > v || (ov == v && oi < idx)) { v = ov; idx = oi; }
      }
      if (tid == 0) piv[0] = (double)idx;
    }
    __syncthreads();
    const int pr = (int)piv[0];
    if (pr != k) {   // swap rows k and pr of Q and P (128 complex entries)
      for (int c = tid; c < 2 * MCF_N; c += MCF_THREADS) {
        double* mr = c < MCF_N ? Qr : Pr;
        double* mi = c < MCF_N ? Qi : Pi;
        const int cc = c & 63;
        const double tr = mr[k * MCF_LD + cc], ti = mi[k * MCF_LD + cc];
        mr[k * MCF_LD + cc] = mr[pr * MCF_LD + cc];
        mi[k * MCF_LD + cc] = mi[pr * MCF_LD + cc];
        mr[pr * MCF_LD + cc] = tr;
        mi[pr * MCF_LD + cc] = ti;
      }
      __syncthreads();
    }
    if (tid < MCF_N) {   // f_i = Q[i][k] / Q[k][k]
      const double ar = Qr[tid * MCF_LD + k], ai = Qi[tid * MCF_LD + k];
      const double br = Qr[k * MCF_LD + k], bi = Qi[k * MCF_LD + k];
      const double den = br * br + bi * bi;
      fr[tid] = (ar * br + ai * bi) / den;
      fi[tid] = (ai * br - ar * bi) / den;
    }
    __syncthreads();
    // rows i != k: Q[i][c] -= f_i Q[k][c] (c > k), P[i][c] -= f_i P[k][c] (all c)
    for (int e = tid; e < MCF_N * 2 * MCF_N; e += MCF_THREADS) {
      const int i = e >> 7, c = e & 127;
      if (i == k) continue;
      double* mr;
      double* mi;
      int cc;
      if (c < MCF_N) { if (c <= k) continue; mr = Qr; mi = Qi; cc = c; }
      else { mr = Pr; mi = Pi; cc = c - MCF_N; }
      const double kr = mr[k * MCF_LD + cc], ki = mi[k * MCF_LD + cc];
      const double gr = fr[i], gi = fi[i];
      mr[i * MCF_LD + cc] = mr[i * MCF_LD + cc] - (gr * kr - gi * ki);
      mi[i * MCF_LD + cc] = mi[i * MCF_LD + cc] - (gr * ki + gi * kr);
    }
    __syncthreads();
  }
  for (int e = tid; e < MCF_N * MCF_N; e += MCF_THREADS) {
    const int r = e >> 6, c = e & 63;
    const double ar = Pr[r * MCF_LD + c], ai = Pi[r * MCF_LD + c];
    const double br = Qr[r * MCF_LD + r], bi = Qi[r * MCF_LD + r];
    const double den = br * br + bi * bi;
    X[e] = (ar * br + ai * bi) / den;
    X[MCF_N * MCF_N + e] = (ai * br - ar * bi) / den;
  }
}

// W0 = expm(-tau (p Lam + i q B)) (workspace W0..W5, LDS S)
__device__ void mcf_expm(const McfArgs& a, double* S, double* W, double p, double q, double tau) {
  double* W0 = W;
  double* W1 = W + MCF_MAT;
  double* W2 = W + 2 * MCF_MAT;
  double* W3 = W + 3 * MCF_MAT;
  double* W4 = W + 4 * MCF_MAT;
  double* W5 = W + 5 * MCF_MAT;
  // exact 1-norm of A (each thread computes it; no synchronisation needed) -> number of squarings
  double nrm = 0.0;
  for (int j = 0; j < a.M; ++j) {
    const double dr = (p * a.lam[j]) * tau, di = (q * a.B[j * MCF_N + j]) * tau;
    const double cs = sqrt(dr * dr + di * di) + fabs(q * tau) * a.colsum[j];
    nrm = fmax(nrm, cs);
  }
  int s = 0;
  if (nrm > MCF_THETA13) s = (int)ceil(log2(nrm / MCF_THETA13));
  if (!(s >= 0)) s = 0;
  if (s > 100) s = 100;
  const double sc = ldexp(1.0, -s);
  __syncthreads();   // the previous item's readers of W0 are done
  for (int e = threadIdx.x; e < MCF_N * MCF_N; e += MCF_THREADS) {
    const int r = e >> 6, c = e & 63;
    double re = 0.0, im = 0.0;
    if (r < a.M && c < a.M) {
      if (r == c) re = -((p * a.lam[r]) * tau) * sc;
      im = -((q * a.B[e]) * tau) * sc;
    }
    W0[e] = re;
    W0[MCF_N * MCF_N + e] = im;
  }
  const double b[14] = {64764752532480000., 32382376266240000., 7771770303897600., 1187353796428800.,
                        129060195264000., 10559470521600., 670442572800., 33522128640.,
                        1323241920., 40840800., 960960., 16380., 182., 1.};
  mcf_gemm(S, W1, W0, W0);                                    // A2
  mcf_gemm(S, W2, W1, W1);                                    // A4
  mcf_gemm(S, W3, W2, W1);                                    // A6
  mcf_comb(W4, nullptr, W3, W2, W1, b[13], b[11], b[9], 0.0);
  mcf_gemm(S, W5, W3, W4);
  mcf_comb(W5, W5, W3, W2, W1, b[7], b[5], b[3], b[1]);
  mcf_gemm(S, W4, W0, W5);                                    // U
  mcf_comb(W5, nullptr, W3, W2, W1, b[12], b[10], b[8], 0.0);
  mcf_gemm(S, W0, W3, W5);
  mcf_comb(W0, W0, W3, W2, W1, b[6], b[4], b[2], b[0]);      // V
  mcf_solve(S, W0, W4, W0);
  for (int i = 0; i < s; ++i) mcf_gemm(S, W0, W0, W0);
  __syncthreads();
}

__global__ void __launch_bounds__(MCF_THREADS) mfx_mcf_kernel(McfArgs a) {
  extern __shared__ double S[];
  double* W = a.work + (size_t)blockIdx.x * MCF_NMAT * MCF_MAT;
  double* vr = S + 4 * MCF_PLANE + 2 * MCF_N;   // (the first two vectors are the solve's factors)
  double* vi = vr + MCF_N;
  double* wr = vi + MCF_N;
  double* wi = wr + MCF_N;
  const int tid = threadIdx.x;
  const long n_items = (long)a.n_act * a.n_atoms;
  for (long it = blockIdx.x; it < n_items; it += gridDim.x) {
    const long at = it / a.n_act;
    const int r = a.act[it - at * a.n_act];
    const McfRow row = a.rows[r];
    const double Lx = a.L[at], D = a.diff[at];
    const double L2 = Lx * Lx;
    const double p = D * row.T / L2;
    const double* X = W;
    double R00r = 0.0, R00i = 0.0;
    for (int b = 0; b < a.nblk; ++b) {
      const double q = a.gamma * row.T * Lx * row.Gperp[b];
      const double tau = row.del[b] / row.T;
      mcf_expm(a, S, W, p, q, tau);
      const double dd = row.Del[b] - row.del[b];
      if (a.nblk == 1) {
        // R[0,0] = sum_k conj(X[0,k]) d_k X[k,0]
        if (tid == 0) {
          for (int k = 0; k < MCF_N; ++k) {
            const double d = exp(-(a.lam[k] * D) * dd / L2);
            const double xr = X[k], xi = X[MCF_N * MCF_N + k];
            const double yr = X[k * MCF_N], yi = X[MCF_N * MCF_N + k * MCF_N];
            R00r += d * (xr * yr + xi * yi);
            R00i += d * (xr * yi - xi * yr);
          }
        }
      } else if (b == 0) {
        // v = conj(X1) diag(d1) X1[:,0], then w = diag(d_mix) v
        if (tid < MCF_N) {
          double sr = 0.0, si = 0.0;
          for (int j = 0; j < MCF_N; ++j) {
            const double d = exp(-(a.lam[j] * D) * dd / L2);
            const double xr = X[tid * MCF_N + j], xi = -X[MCF_N * MCF_N + tid * MCF_N + j];
            const double yr = d * X[j * MCF_N], yi = d * X[MCF_N * MCF_N + j * MCF_N];
            sr += xr * yr - xi * yi;
            si += xr * yi + xi * yr;
          }
          const double dm = exp(-(a.lam[tid] * D) * row.tmix / L2);
          vr[tid] = dm * sr;
          vi[tid] = dm * si;
        }
      } else {
        // u = X2 w, R[0,0] = sum_j conj(X2[0,j]) d2_j u_j
        if (tid < MCF_N) {
          double sr = 0.0, si = 0.0;
          for (int j = 0; j < MCF_N; ++j) {
            const double xr = X[tid * MCF_N + j], xi = X[MCF_N * MCF_N + tid * MCF_N + j];
            sr += xr * vr[j] - xi * vi[j];
            si += xr * vi[j] + xi * vr[j];
          }
          wr[tid] = sr;
          wi[tid] = si;
        }
        __syncthreads();
        if (tid == 0) {
          for (int j = 0; j < MCF_N; ++j) {
            const double d = exp(-(a.lam[j] * D) * dd / L2);
            const double xr = X[j], xi = -X[MCF_N * MCF_N + j];
            R00r += d * (xr * wr[j] - xi * wi[j]);
            R00i += d * (xr * wi[j] + xi * wr[j]);
          }
        }
      }
    }
    if (tid == 0) a.E[(long)r * a.n_atoms + at] = hypot(R00r, R00i) * mcf_epar(row, a.nblk, a.gamma, D);
  }
}

int mcf_run(const double* lam, const double* B, int M, const double* seq, int64_t n_seq, const double* L,
            const double* diff, int64_t n_atoms, const double* envdir, double gamma, double* E_out, bool dde) {
  const char* fn = dde ? "mfx_mcf_dde" : "mfx_mcf_pgse";
  if (!lam || !B || !seq || !L || !diff || !envdir || !E_out)
    return mfx_fail(MFX_ERR_ARG, "%s: null argument", fn);
  if (M < 1 || M > MCF_N) return mfx_fail(MFX_ERR_ARG, "%s: need 1 <= M <= %d (got %d)", fn, MCF_N, M);
  if (n_seq < 0 || n_atoms < 0) return mfx_fail(MFX_ERR_ARG, "%s: negative n_seq or n_atoms", fn);
  if (n_seq > (1 << 24) || n_atoms > (1LL << 31) || n_seq * n_atoms > (1LL << 40))
    return mfx_fail(MFX_ERR_UNSUPPORTED, "%s: more than 2^24 rows, 2^31 atoms or 2^40 items", fn);
  for (int64_t a = 0; a < n_atoms; ++a)
    if (!(L[a] > 0.0) || !(diff[a] > 0.0) || !std::isfinite(L[a]) || !std::isfinite(diff[a]))
      return mfx_fail(MFX_ERR_ARG, "%s: atom %lld: L and diff must be positive and finite", fn, (long long)a);
  const double en = std::sqrt(envdir[0] * envdir[0] + envdir[1] * envdir[1] + envdir[2] * envdir[2]);
  if (!(en > 0.0) || !std::isfinite(en)) return mfx_fail(MFX_ERR_ARG, "%s: envdir must be a non-zero finite vector", fn);
  if (!std::isfinite(gamma)) return mfx_fail(MFX_ERR_ARG, "%s: gamma must be finite", fn);
  const double e[3] = {envdir[0] / en, envdir[1] / en, envdir[2] / en};
  // rows: parallel / perpendicular gradient components as the reference's loop forms them
  const int ncol = dde ? 14 : 7, nblk = dde ? 2 : 1;
  std::vector<McfRow> rows((size_t)n_seq);
  std::vector<int> act;
  for (int64_t i = 0; i < n_seq; ++i) {
    const double* s = seq + (size_t)i * ncol;
    McfRow& r = rows[(size_t)i];
    r = McfRow{};
    bool any_g = false, any_perp = false;
    for (int b = 0; b < nblk; ++b) {
      const double* g = s + 7 * b;   // [gx gy gz G Delta delta tau_mix|TE]
      const double G = g[3];
      const double dot = g[0] * e[0] + g[1] * e[1] + g[2] * e[2];
      double par[3], perp[3];
      for (int c = 0; c < 3; ++c) { par[c] = dot * e[c]; perp[c] = g[c] - par[c]; }
      r.Gpar[b] = G * std::sqrt(par[0] * par[0] + par[1] * par[1] + par[2] * par[2]);
      r.Gperp[b] = G * std::sqrt(perp[0] * perp[0] + perp[1] * perp[1] + perp[2] * perp[2]);
      r.Del[b] = g[4];
      r.del[b] = g[5];
      any_g = any_g || G != 0.0;
      any_perp = any_perp || r.Gperp[b] != 0.0;
    }
    if (dde) { r.tmix = s[6]; r.T = s[4] + s[5] + s[6] + s[11] + s[12]; }
    else r.T = s[4] + s[5];
    r.kind = !any_g ? 0 : (!any_perp ? 1 : 2);
    if (r.kind == 2) {
      if (!(r.T > 0.0) || !std::isfinite(r.T))
        return mfx_fail(MFX_ERR_ARG, "%s: row %lld: total encoding time must be positive", fn, (long long)i);
      act.push_back((int)i);
    }
  }
  if (n_seq == 0 || n_atoms == 0) return MFX_OK;
  {
    int dev = 0;
    if (mfx_device_count() <= 0) return mfx_no_device();
    HIPCHK(hipGetDevice(&dev));
    HIPCHK(hipSetDevice(dev));
  }
  std::vector<double> hlam(MCF_N, 0.0), hB((size_t)MCF_N * MCF_N, 0.0), hcs(MCF_N, 0.0);
  for (int i = 0; i < M; ++i) {
    hlam[i] = lam[i];
    for (int j = 0; j < M; ++j) hB[(size_t)i * MCF_N + j] = B[(size_t)i * M + j];
  }
  for (int j = 0; j < M; ++j)
    for (int i = 0; i < M; ++i)
      if (i != j) hcs[j] += std::fabs(hB[(size_t)i * MCF_N + j]);
  const int64_t n_items = (int64_t)act.size() * n_atoms;
  int ncu = 0, dev = 0;
  HIPCHK(hipGetDevice(&dev));
  HIPCHK(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev));
  const int nblocks = (int)std::min<int64_t>(n_items, std::max(1, ncu));
  DevMem dlam, dB, dcs, drows, dact, dL, dD, dE, dW;
  HIPCHK(dlam.alloc(sizeof(double) * MCF_N));
  HIPCHK(dB.alloc(sizeof(double) * hB.size()));
  HIPCHK(dcs.alloc(sizeof(double) * MCF_N));
  HIPCHK(drows.alloc(sizeof(McfRow) * rows.size()));
  HIPCHK(dact.alloc(sizeof(int) * act.size()));
  HIPCHK(dL.alloc(sizeof(double) * n_atoms));
  HIPCHK(dD.alloc(sizeof(double) * n_atoms));
  HIPCHK(dE.alloc(sizeof(double) * n_seq * n_atoms));
  if (nblocks > 0) HIPCHK(dW.alloc(sizeof(double) * (size_t)nblocks * MCF_NMAT * MCF_MAT));
  HIPCHK(hipMemcpy(dlam.p, hlam.data(), sizeof(double) * MCF_N, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(dB.p, hB.data(), sizeof(double) * hB.size(), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(dcs.p, hcs.data(), sizeof(double) * MCF_N, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(drows.p, rows.data(), sizeof(McfRow) * rows.size(), hipMemcpyHostToDevice));
  if (!act.empty()) HIPCHK(hipMemcpy(dact.p, act.data(), sizeof(int) * act.size(), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(dL.p, L, sizeof(double) * n_atoms, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(dD.p, diff, sizeof(double) * n_atoms, hipMemcpyHostToDevice));
  McfArgs a{};
  a.lam = dlam.as<double>(); a.B = dB.as<double>(); a.colsum = dcs.as<double>();
  a.rows = drows.as<McfRow>(); a.act = dact.as<int>(); a.n_act = (int)act.size(); a.n_seq = (int)n_seq;
  a.M = M; a.nblk = nblk; a.n_atoms = n_atoms; a.L = dL.as<double>(); a.diff = dD.as<double>(); a.gamma = gamma;
  a.E = dE.as<double>(); a.work = dW.as<double>();
  hipStream_t st = nullptr;
  if (int rc = mfx_prof_begin(st)) return rc;
  const int64_t n_all = n_seq * n_atoms;
  hipLaunchKernelGGL(mfx_mcf_closed_kernel, dim3((unsigned)std::min<int64_t>((n_all + 255) / 256, 4096)), dim3(256), 0, st, a);
  HIPCHK(hipGetLastError());
  if (nblocks > 0) {
    HIPCHK(hipFuncSetAttribute((const void*)mfx_mcf_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)MCF_LDS_BYTES));
    hipLaunchKernelGGL(mfx_mcf_kernel, dim3(nblocks), dim3(MCF_THREADS), MCF_LDS_BYTES, st, a);
    HIPCHK(hipGetLastError());
  }
  if (int rc = mfx_prof_end(st)) return rc;
  HIPCHK(hipMemcpy(E_out, dE.p, sizeof(double) * n_all, hipMemcpyDeviceToHost));
  return MFX_OK;
}

}  // namespace

extern "C" int mfx_mcf_abi_version(void) { return 1; }

extern "C" int mfx_mcf_pgse(const double* lam, const double* B, int M, const double* seq, int64_t n_seq, const double* L,
                            const double* diff, int64_t n_atoms, const double* envdir, double gamma, double* E_out) {
  return mcf_run(lam, B, M, seq, n_seq, L, diff, n_atoms, envdir, gamma, E_out, false);
}

extern "C" int mfx_mcf_dde(const double* lam, const double* B, int M, const double* seq, int64_t n_seq, const double* L,
                           const double* diff, int64_t n_atoms, const double* envdir, double gamma, double* E_out) {
  return mcf_run(lam, B, M, seq, n_seq, L, diff, n_atoms, envdir, gamma, E_out, true);
}
