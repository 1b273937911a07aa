// solve_batch.hip -- the batched explicit-dictionary solver (include/mfx_solve.h): V signals against ONE dictionary.
//
// mfx_solve_exhaustive (mfx_api.hip, solve_generic.hip) serves one problem per call; of its work only A^T y and ||y||^2
// depend on the signal.  A handle here owns, on the device:
//   A    [M x Ntot]     the dictionary, compacted
//   G    [Ntot x Ntot]  A^T A, every entry summed sequentially over the rows (mfx_gram_kernel's order: the same bits)
//   rel  [n1 x n2]      tiled classes only: mfx_tuple_rel of every pair - the signal-independent part of the score's
//                       error bound, which becomes MFX_SCORE_ERR * ysq / rel
// and a batch runs, per chunk of signals (scratch of the stream's arena, within the byte budget):
//   1. sb_prep_kernel      A^T y [Vc x Ntot] and ||y||^2 [Vc x 2] in the one-problem path's order, the status of every
//                          signal (1: a non-finite value; such a signal is not scanned), the scan's counters zeroed
//   2. scan + collect      TILED (two sub-dictionaries, or three whose last has one column): sb_tile_kernel.  A
//                          workgroup keeps a 64 x 64 tile of the cross block of G and of rel in LDS (16 pairs a
//                          thread), the diagonals and, for the third column, g13 / g23 / g33 beside it or in registers,
//                          and sweeps the chunk's signals over it: per signal it loads A^T y's slices and ysq, nothing else.
//                          Every pair goes through score2 / score3 and the error bound of mfx_tuple_score(_err): the
//                          same bits.  Pass 1 leaves the best upper bound of every (signal, tile, wave) cell and the
//                          signal's best lower bound (atomicMax); pass 2 revisits the cells that reach the signal's tie
//                          threshold and appends every tuple inside the window to the signal's list (mfx_listed_score,
//                          MFX_SCAN_CAP, overflow flag: mfx_tuple_collect's rule).  WHICH tuples are listed depends on
//                          the scores alone, not on how tuples are dealt to blocks, and the finalize stage decides by
//                          (residual, scan-order key), not by the list's order: the tiling is free.
//                          GENERIC (every other class, and everything under mfx_solve_debug_set_force_generic(1)): the
//                          bodies of mfx_tuple_scan / mfx_tuple_collect on a per-signal view, blockIdx.y = signal.
//   3. sb_overflow_kernel  a signal whose list overflowed: mfx_tuple_overflow's rule on the one-problem path's block
//                          partition (the outcome depends on it); the blocks loop over the chunk's signals and pass
//                          every signal that did not overflow.
//   4. sb_finalize_kernel  one workgroup per signal: the body of mfx_tuple_finalize; NaN rows for status 1.
// The three-dictionary matrix-pipe screen (solve_k3.hip) is not used here.
#include "solve_shared.h"   // the handle, SbArgs, sb_prep_kernel, sb_args
#include "../../include/mfx_solve.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>
#include <vector>

namespace {

thread_local int g_force_generic = 0;

// the one-problem solver's view of signal v
__device__ __forceinline__ SolveArgs sb_view(const SbArgs& b, int v) {
  SolveArgs a{};
  a.A = b.A; a.lda = b.Ntot; a.M = b.M; a.Kp = b.Kp; a.Ntot = b.Ntot;
  for (int k = 0; k < MFX_GK; ++k) { a.sizes[k] = b.sizes[k]; a.start[k] = b.start[k]; }
  a.y = b.Y + (size_t)v * b.M;
  a.G = const_cast<double*>(b.G);
  a.Aty = b.Aty + (size_t)v * b.Ntot;
  a.ysq = b.ysq + 2 * (size_t)v;
  a.ntuples = b.ntuples;
  a.blk_score = b.lst_score + (size_t)v * b.list_cap;
  a.blk_tuple = b.lst_tuple + (size_t)v * b.list_cap;
  a.nblocks = b.nblocks; a.list_cap = b.list_cap;
  a.blk_max = b.cell_is_blk_max ? b.cell + (size_t)v * b.ncell : nullptr;
  a.smax = b.smax + v;
  a.ncand = b.ncand + v;
  a.nblocks_dev = a.ncand;
  a.w = b.w + (size_t)v * b.Kp;
  a.sub = b.sub + (size_t)v * b.Kp;
  a.minobj = b.obj + v;
  a.yrec = b.yrec ? b.yrec + (size_t)v * b.M : nullptr;
  return a;
}

// ---- once per handle
__global__ void sb_gram_kernel(const double* __restrict__ A, int M, int Ntot, double* __restrict__ G) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long)Ntot * Ntot) return;
  const int p = (int)(idx / Ntot), q = (int)(idx - (long)p * Ntot);
  double s = 0.0;
  for (int k = 0; k < M; ++k) s += A[(long)k * Ntot + p] * A[(long)k * Ntot + q];
  G[idx] = s;
}
// rel [n1 x n2] of the pair (i, j), with the only third column where there is one
__global__ void sb_rel_kernel(SbArgs b, double* __restrict__ rel) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long n2 = b.sizes[1];
  if (idx >= b.sizes[0] * n2) return;
  SolveArgs a{};
  a.Kp = b.Kp; a.Ntot = b.Ntot; a.G = const_cast<double*>(b.G);
  int col[MFX_GK];
  col[0] = (int)(idx / n2);
  col[1] = (int)(b.start[1] + idx % n2);
  col[2] = (int)b.start[2];
  rel[idx] = mfx_tuple_rel(a, col);
}

// ---- the tiled scan (COLLECT = false) and collect (COLLECT = true); K3: a third sub-dictionary of one column.
// Lane = column of the tile, wave w = rows w, w + 4, ..: what belongs to a row (g11, g13, A^T y of the row) is uniform over
// the wave, what belongs to the column (g22, g23, A^T y of the column) is one register a lane.  The tile of the cross
// block and of rel sits in LDS [row][column] (a wave reads 64 consecutive doubles: no bank conflict), so the loop over
// the rows stays rolled and the registers few.
constexpr size_t SB_TILE_LDS = sizeof(double) * (2 * SB_T * SB_T + 2 * SB_T);
template <bool K3, bool COLLECT>
__global__ __launch_bounds__(256) void sb_tile_kernel(SbArgs b) {
  extern __shared__ double sb_lds[];
  double* s_g12 = sb_lds;                  // [SB_T x SB_T]
  double* s_rl = s_g12 + SB_T * SB_T;      // [SB_T x SB_T]
  double* s_g11 = s_rl + SB_T * SB_T;      // [SB_T]
  double* s_g13 = s_g11 + SB_T;            // [SB_T]
  const int tile = blockIdx.x, tr = tile / b.tiles_c, tc = tile - tr * b.tiles_c;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n1 = (int)b.sizes[0], n2 = (int)b.sizes[1], N = b.Ntot;
  const int c3 = n1 + n2;   // (K3) the third column
  const int r0 = tr * SB_T, nr = min(SB_T, n1 - r0);   // the tile's rows r0 .. r0 + nr inside sub-dictionary 0
  const int j = tc * SB_T + lane;                       // the lane's column inside sub-dictionary 1
  const bool cv = j < n2;
  const int jc = n1 + (cv ? j : n2 - 1);                // its column of A (clamped: cv says whether it exists)
  const double* __restrict__ G = b.G;
  for (int r = wave; r < nr; r += SB_WAVES) {
    s_g12[r * SB_T + lane] = G[(long)(r0 + r) * N + jc];
    s_rl[r * SB_T + lane] = b.rel[(long)(r0 + r) * n2 + (jc - n1)];
  }
  if (threadIdx.x < nr) {
    s_g11[threadIdx.x] = G[(long)(r0 + threadIdx.x) * N + r0 + threadIdx.x];
    s_g13[threadIdx.x] = K3 ? G[(long)(r0 + threadIdx.x) * N + c3] : 0.0;
  }
  const double g22 = G[(long)jc * N + jc];
  const double g23 = K3 ? G[(long)jc * N + c3] : 0.0;
  const double g33 = K3 ? G[(long)c3 * N + c3] : 0.0;
  __syncthreads();
  const int cell = tile * SB_WAVES + wave;
  for (int v = blockIdx.y; v < b.Vc; v += gridDim.y) {
    if (b.status[v]) continue;
    const double ysq = b.ysq[2 * (size_t)v];   // two and three sub-dictionaries: the sequential sum (mfx_ref_ysq)
    double smaxv = 0.0, thr = 0.0;
    if (COLLECT) {
      smaxv = __longlong_as_double((long long)b.smax[v]);
      thr = smaxv - 1e-9 * ysq;                // mfx_tie_threshold
      const double bm = b.cell[(size_t)v * b.ncell + cell];
      if (!(bm > 0.0) || bm < thr) continue;   // (uniform over the wave)
    }
    const double* __restrict__ aty = b.Aty + (size_t)v * N;
    const double y2 = aty[jc];
    const double y3 = K3 ? aty[c3] : 0.0;
    const double eb = MFX_SCORE_ERR * ysq;     // mfx_tuple_score_err: MFX_SCORE_ERR * ysq / rel, left to right
    double best = 0.0, lb = 0.0;
    if (cv) {
#pragma unroll 1
      for (int r = wave; r < nr; r += SB_WAVES) {
        const double g11 = s_g11[r], g12 = s_g12[r * SB_T + lane], y1 = aty[r0 + r];
        const double s = K3 ? score3(g11, g12, s_g13[r], g22, g23, g33, y1, y2, y3) : score2(g11, g12, g22, y1, y2);
        if (!(s > 0.0)) continue;
        const double e = eb / s_rl[r * SB_T + lane];
        if (!COLLECT) {
          best = fmax(best, s + e);
          lb = fmax(lb, s - e);
        } else {
          const double ub = s + e;
          if (ub < thr) continue;
          int* nc = b.ncand + v;
          if (*(volatile int*)nc < 0) break;   // overflowed: sb_overflow_kernel takes over
          const int slot = atomicAdd(nc, 1);
          if (slot >= 0 && slot < b.list_cap) {
            b.lst_score[(size_t)v * b.list_cap + slot] = fmin(ub, smaxv);            // mfx_listed_score
            b.lst_tuple[(size_t)v * b.list_cap + slot] = (long)(r0 + r) * n2 + j;    // (a third column of one: the same number)
          } else {
            atomicOr(nc, (int)0x80000000);
            break;
          }
        }
      }
    }
    if (!COLLECT) {
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) { best = fmax(best, __shfl_xor(best, o)); lb = fmax(lb, __shfl_xor(lb, o)); }
      if (lane == 0) {
        b.cell[(size_t)v * b.ncell + cell] = best;
        if (lb > 0.0) atomicMax(b.smax + v, (unsigned long long)__double_as_longlong(lb));
      }
    }
  }
}

// ---- the generic route: the one-problem scan with a signal dimension
__global__ __launch_bounds__(256) void sb_scan_kernel(SbArgs b) {
  if (b.status[blockIdx.y]) return;
  const SolveArgs a = sb_view(b, blockIdx.y);
  mfx_tuple_scan_body(a);
}
__global__ __launch_bounds__(256) void sb_collect_kernel(SbArgs b) {
  if (b.status[blockIdx.y]) return;
  const SolveArgs a = sb_view(b, blockIdx.y);
  mfx_tuple_collect_body(a);
}
// grid: the one-problem partition; the blocks pass every signal whose list did not overflow
__global__ __launch_bounds__(256) void sb_overflow_kernel(SbArgs b) {
  for (int v = 0; v < b.Vc; ++v) {
    if (b.status[v] || b.ncand[v] >= 0) continue;   // (uniform over the block)
    const SolveArgs a = sb_view(b, v);
    mfx_tuple_overflow_body(a);
    __syncthreads();   // (the body's shared arrays serve the next signal)
  }
}
__global__ __launch_bounds__(256) void sb_finalize_kernel(SbArgs b) {
  const int v = blockIdx.x;
  if (b.status[v]) {   // a non-finite signal: NaN row, no index
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    for (int k = threadIdx.x; k < b.Kp; k += 256) { b.w[(size_t)v * b.Kp + k] = nan; b.sub[(size_t)v * b.Kp + k] = -1; }
    if (threadIdx.x == 0) b.obj[v] = nan;
    if (b.yrec)
      for (int k = threadIdx.x; k < b.M; k += 256) b.yrec[(size_t)v * b.M + k] = nan;
    return;
  }
  const SolveArgs a = sb_view(b, v);
  mfx_tuple_finalize_body(a);
}

bool sb_tiled(const mfx_solve* h) { return h->tiled_class && !g_force_generic; }
int sb_ncell(const mfx_solve* h) { return sb_tiled(h) ? (int)(h->tiles_r * h->tiles_c * SB_WAVES) : h->nblocks; }
// scratch of one signal: A^T y, ysq [2], smax, ncand (padded), the cells, the candidate list
int64_t sb_bytes_per_signal(const mfx_solve* h) {
  return 8 * ((int64_t)h->Ntot + 4) + 8 * (int64_t)sb_ncell(h) + 16 * (int64_t)h->list_cap;
}

}  // namespace

extern "C" int mfx_solve_abi_version(void) { return 1; }

extern "C" void mfx_solve_debug_set_force_generic(int enabled) { g_force_generic = enabled ? 1 : 0; }

extern "C" int mfx_solve_create(const double* A, int64_t lda, int M, const int64_t* dicsizes, int Kp, int device, void** out) {
  if (!A || !dicsizes || !out || M < 1 || Kp < 1) return mfx_fail(MFX_ERR_ARG, "mfx_solve_create: bad argument");
  *out = nullptr;
  if (Kp > MFX_GK) return mfx_fail(MFX_ERR_UNSUPPORTED, "at most %d sub-dictionaries are supported (got %d)", MFX_GK, Kp);
  if (mfx_device_count() <= 0) return mfx_no_device();
  std::unique_ptr<mfx_solve> h(new mfx_solve());
  long Ntot = 0, ntup = 1;
  for (int k = 0; k < Kp; ++k) {
    if (dicsizes[k] < 1) return mfx_fail(MFX_ERR_ARG, "All entries of dicsizes should be > 0");
    h->sizes[k] = dicsizes[k];
    h->start[k] = Ntot;
    Ntot += dicsizes[k];
    if (ntup > (1L << 40) / dicsizes[k]) return mfx_fail(MFX_ERR_UNSUPPORTED, "too many index tuples for the explicit solver");
    ntup *= dicsizes[k];
  }
  if (lda < Ntot) return mfx_fail(MFX_ERR_ARG, "lda (%lld) < number of columns (%ld)", (long long)lda, Ntot);
  if (Ntot > 30000) return mfx_fail(MFX_ERR_UNSUPPORTED, "explicit solver supports up to 30000 columns (got %ld)", Ntot);
  if (int rc = mfx_require_device(device)) return rc;
  h->device = device; h->M = M; h->Kp = Kp; h->Ntot = (int)Ntot; h->ntuples = ntup;
  h->nblocks = (int)std::min<long>(8192, (ntup + 255) / 256);
  h->list_cap = (int)std::min<long>(ntup, MFX_SCAN_CAP);
  h->tiled_class = Kp == 2 || (Kp == 3 && dicsizes[2] == 1);
  if (h->tiled_class) {
    h->tiles_r = (h->sizes[0] + SB_T - 1) / SB_T;
    h->tiles_c = (h->sizes[1] + SB_T - 1) / SB_T;
  }
  std::vector<double> Ac((size_t)M * Ntot);
  for (int k = 0; k < M; ++k) std::memcpy(&Ac[(size_t)k * Ntot], A + (size_t)k * lda, sizeof(double) * Ntot);
  HIPCHK(h->A.alloc(sizeof(double) * Ac.size()));
  HIPCHK(h->G.alloc(sizeof(double) * (size_t)Ntot * Ntot));
  HIPCHK(hipMemcpy(h->A.p, Ac.data(), sizeof(double) * Ac.size(), hipMemcpyHostToDevice));
  const long nn = Ntot * Ntot;
  hipLaunchKernelGGL(sb_gram_kernel, dim3((unsigned)((nn + 255) / 256)), dim3(256), 0, nullptr, h->A.as<double>(), M, (int)Ntot,
                     h->G.as<double>());
  HIPCHK(hipGetLastError());
  if (h->tiled_class) {
    // (the tile's LDS is beyond the 64 KiB a kernel gets without asking)
    HIPCHK(hipFuncSetAttribute((const void*)sb_tile_kernel<false, false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)SB_TILE_LDS));
    HIPCHK(hipFuncSetAttribute((const void*)sb_tile_kernel<false, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)SB_TILE_LDS));
    HIPCHK(hipFuncSetAttribute((const void*)sb_tile_kernel<true, false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)SB_TILE_LDS));
    HIPCHK(hipFuncSetAttribute((const void*)sb_tile_kernel<true, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)SB_TILE_LDS));
    const long np = h->sizes[0] * h->sizes[1];
    HIPCHK(h->rel.alloc(sizeof(double) * (size_t)np));
    hipLaunchKernelGGL(sb_rel_kernel, dim3((unsigned)((np + 255) / 256)), dim3(256), 0, nullptr, sb_args(h.get()), h->rel.as<double>());
    HIPCHK(hipGetLastError());
  }
  HIPCHK(hipDeviceSynchronize());   // the handle serves any stream from here on
  *out = h.release();
  return MFX_OK;
}

extern "C" void mfx_solve_destroy(void* hv) {
  mfx_solve* h = (mfx_solve*)hv;
  if (!h) return;
  (void)hipSetDevice(h->device);
  delete h;
}

extern "C" int64_t mfx_solve_num_columns(const void* hv) { return hv ? ((const mfx_solve*)hv)->Ntot : -1; }

extern "C" int64_t mfx_solve_bytes_per_signal(const void* hv) { return hv ? sb_bytes_per_signal((const mfx_solve*)hv) : -1; }

extern "C" int mfx_solve_batch_dev(void* hv, const double* d_Y, int64_t V, int64_t max_bytes, double* d_w, int64_t* d_sub,
                                   double* d_obj, double* d_yrec, int32_t* d_status, void* stream) {
  if (mfx_device_count() <= 0) return mfx_no_device();
  const mfx_solve* h = (const mfx_solve*)hv;
  if (!h || V < 0 || (V > 0 && (!d_Y || !d_w || !d_sub || !d_obj || !d_status)))
    return mfx_fail(MFX_ERR_ARG, "mfx_solve_batch_dev: bad argument");
  if (V == 0) return MFX_OK;
  if (int rc = mfx_require_device(h->device)) return rc;
  hipStream_t st = (hipStream_t)stream;
  const bool tiled = sb_tiled(h);
  const int ncell = sb_ncell(h);
  if (max_bytes <= 0) max_bytes = SB_DEFAULT_BYTES;
  const int64_t Vc = std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(V, 65535), max_bytes / sb_bytes_per_signal(h)));
  const int N = h->Ntot;
  StreamMem sAty(st), sysq(st), ssmax(st), sncand(st), scell(st), slsc(st), sltu(st);
  HIPCHK(sAty.alloc(sizeof(double) * (size_t)Vc * N));
  HIPCHK(sysq.alloc(sizeof(double) * 2 * (size_t)Vc));
  HIPCHK(ssmax.alloc(sizeof(unsigned long long) * (size_t)Vc));
  HIPCHK(sncand.alloc(sizeof(int) * (size_t)Vc));
  HIPCHK(scell.alloc(sizeof(double) * (size_t)Vc * ncell));
  HIPCHK(slsc.alloc(sizeof(double) * (size_t)Vc * h->list_cap));
  HIPCHK(sltu.alloc(sizeof(long) * (size_t)Vc * h->list_cap));
  SbArgs b = sb_args(h);
  b.Aty = sAty.as<double>(); b.ysq = sysq.as<double>(); b.smax = ssmax.as<unsigned long long>(); b.ncand = sncand.as<int>();
  b.cell = scell.as<double>(); b.ncell = ncell; b.cell_is_blk_max = tiled ? 0 : 1;
  b.lst_score = slsc.as<double>(); b.lst_tuple = sltu.as<long>();
  const long ntiles = h->tiles_r * h->tiles_c;
  for (int64_t v0 = 0; v0 < V; v0 += Vc) {
    const int nv = (int)std::min<int64_t>(Vc, V - v0);
    b.Y = d_Y + (size_t)v0 * h->M; b.Vc = nv;
    b.w = d_w + (size_t)v0 * h->Kp; b.sub = (long*)d_sub + (size_t)v0 * h->Kp; b.obj = d_obj + v0;
    b.yrec = d_yrec ? d_yrec + (size_t)v0 * h->M : nullptr;
    b.status = d_status + v0;
    hipLaunchKernelGGL(sb_prep_kernel, dim3((unsigned)((N + 255) / 256 + 1), (unsigned)nv), dim3(256), 0, st, b);
    HIPCHK(hipGetLastError());
    if (tiled) {
      // enough workgroups to fill the device: the signals of the chunk are dealt to gridDim.y sweeps of every tile
      const unsigned ny = (unsigned)std::max<long>(1, std::min<long>(nv, (2048 + ntiles - 1) / ntiles));
      const dim3 g((unsigned)ntiles, ny);
      if (h->Kp == 3) {
        hipLaunchKernelGGL((sb_tile_kernel<true, false>), g, dim3(256), SB_TILE_LDS, st, b);
        hipLaunchKernelGGL((sb_tile_kernel<true, true>), g, dim3(256), SB_TILE_LDS, st, b);
      } else {
        hipLaunchKernelGGL((sb_tile_kernel<false, false>), g, dim3(256), SB_TILE_LDS, st, b);
        hipLaunchKernelGGL((sb_tile_kernel<false, true>), g, dim3(256), SB_TILE_LDS, st, b);
      }
    } else {
      hipLaunchKernelGGL(sb_scan_kernel, dim3(h->nblocks, (unsigned)nv), dim3(256), 0, st, b);
      hipLaunchKernelGGL(sb_collect_kernel, dim3(h->nblocks, (unsigned)nv), dim3(256), 0, st, b);
    }
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(sb_overflow_kernel, dim3(h->nblocks), dim3(256), 0, st, b);
    hipLaunchKernelGGL(sb_finalize_kernel, dim3((unsigned)nv), dim3(256), 0, st, b);
    HIPCHK(hipGetLastError());
  }
  return MFX_OK;
}

extern "C" int mfx_solve_batch(void* hv, const double* Y, int64_t V, int64_t max_bytes, double* w, int64_t* sub, double* obj,
                               double* yrec, int32_t* status) {
  if (mfx_device_count() <= 0) return mfx_no_device();
  const mfx_solve* h = (const mfx_solve*)hv;
  if (!h || V < 0 || (V > 0 && (!Y || !w || !sub || !obj || !status))) return mfx_fail(MFX_ERR_ARG, "mfx_solve_batch: bad argument");
  if (V == 0) return MFX_OK;
  if (int rc = mfx_require_device(h->device)) return rc;
  const size_t M = h->M, Kp = h->Kp, n = (size_t)V;
  DevBuf<double> dY, dw, dobj, dyrec;
  DevBuf<int64_t> dsub;
  DevBuf<int32_t> dst;
  HIPCHK(dY.upload(Y, n * M));
  HIPCHK(dw.alloc_n(n * Kp));
  HIPCHK(dsub.alloc_n(n * Kp));
  HIPCHK(dobj.alloc_n(n));
  HIPCHK(dst.alloc_n(n));
  if (yrec) HIPCHK(dyrec.alloc_n(n * M));
  if (int rc = mfx_solve_batch_dev(hv, dY.get(), V, max_bytes, dw.get(), dsub.get(), dobj.get(), yrec ? dyrec.get() : nullptr,
                                   dst.get(), nullptr)) return rc;
  HIPCHK(hipStreamSynchronize(nullptr));
  HIPCHK(dw.download(w));
  HIPCHK(dsub.download(sub));
  HIPCHK(dobj.download(obj));
  HIPCHK(dst.download(status));
  if (yrec) HIPCHK(dyrec.download(yrec));
  return MFX_OK;
}
