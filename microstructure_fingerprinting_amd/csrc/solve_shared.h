// solve_shared.h -- what the batched explicit solver (solve_batch.hip, include/mfx_solve.h) and its soft answers
// (solve_soft.hip, include/mfx_solve_soft.h) share: the handle, the tile geometry, the arguments of a chunk of signals
// and the kernel that forms A^T y and ||y||^2 per signal - one definition, so that both read the same bits.
#pragma once
#define MFX_SOLVE_BODIES_ONLY
#include "mfx_host.h"
#include "solve_generic.hip"

#define SB_T 64        // tile edge: a lane per column, the rows dealt to the waves
#define SB_WAVES 4     // cells per tile: wave w has rows w, w + 4, ..

struct mfx_solve {
  int device = 0;
  int M = 0, Kp = 0, Ntot = 0;
  long sizes[MFX_GK] = {}, start[MFX_GK] = {};
  long ntuples = 0;
  int nblocks = 0, list_cap = 0;
  bool tiled_class = false;
  long tiles_r = 0, tiles_c = 0;
  DevMem A, G, rel;
};

namespace {

constexpr int64_t SB_DEFAULT_BYTES = (int64_t)256 << 20;

struct SbArgs {
  // the handle
  const double* A; const double* G; const double* rel;
  int M, Kp, Ntot;
  long sizes[MFX_GK], start[MFX_GK];
  long ntuples;
  int nblocks, list_cap;
  int tiles_c;
  // the chunk
  const double* Y;        // [Vc x M]
  int Vc;
  double* Aty;            // [Vc x Ntot]
  double* ysq;            // [Vc x 2]
  unsigned long long* smax;   // [Vc]
  int* ncand;             // [Vc]
  double* cell;           // [Vc x ncell] best upper bound of a scan block (generic) or of a (tile, wave) (tiled)
  int ncell;
  int cell_is_blk_max;    // the cells are the one-problem partition's block maxima (generic route)
  double* lst_score;      // [Vc x list_cap]
  long* lst_tuple;        // [Vc x list_cap]
  // the chunk's outputs
  double* w; long* sub; double* obj; double* yrec; int* status;
};

// ---- per chunk: blocks x < gridDim.x - 1 sum A^T y, the last one of every signal sums ||y||^2 and looks for non-finite values
__global__ __launch_bounds__(256) void sb_prep_kernel(SbArgs b) {
  const int v = blockIdx.y;
  const double* y = b.Y + (size_t)v * b.M;
  if (blockIdx.x + 1 < gridDim.x) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= b.Ntot) return;
    double s = 0.0;
    for (int k = 0; k < b.M; ++k) s += y[k] * b.A[(long)k * b.Ntot + p];
    b.Aty[(size_t)v * b.Ntot + p] = s;
    return;
  }
  int bad = 0;
  for (int k = threadIdx.x; k < b.M; k += 256) bad |= !isfinite(y[k]);
  bad = __syncthreads_or(bad);
  if (threadIdx.x == 0) {
    double s = 0.0;
    for (int k = 0; k < b.M; ++k) s += y[k] * y[k];
    b.ysq[2 * (size_t)v] = s;
    b.status[v] = bad ? 1 : 0;
  } else if (threadIdx.x == 64) {
    b.ysq[2 * (size_t)v + 1] = mfx_np_sumsq(y, b.M);
    b.smax[v] = 0ull;
    b.ncand[v] = 0;
  }
}

SbArgs sb_args(const mfx_solve* h) {
  SbArgs b{};
  b.A = h->A.as<double>(); b.G = h->G.as<double>(); b.rel = h->rel.as<double>();
  b.M = h->M; b.Kp = h->Kp; b.Ntot = h->Ntot;
  for (int k = 0; k < MFX_GK; ++k) { b.sizes[k] = h->sizes[k]; b.start[k] = h->start[k]; }
  b.ntuples = h->ntuples; b.nblocks = h->nblocks; b.list_cap = h->list_cap;
  b.tiles_c = (int)h->tiles_c;
  return b;
}

}  // namespace
