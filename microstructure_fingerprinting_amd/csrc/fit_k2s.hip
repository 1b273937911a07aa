// fit_k2s.hip -- two-fascicle voxels, protocols of up to 256 measurements (exact-G or G-bracketed rows):
// split-FP16 MFMA SCREENING of all atom pairs followed by the exact FP64 evaluation of the short list.
// Same inputs, outputs and results as mfx_fit_k2_kernel (fit_k2.hip), which stays the path for longer
// protocols and the fallback for the rare voxel whose short list overflows.
//
// Why: the 2*N1*N2*M cross-Gram of solve_exhaustive_posweights_2 (mf_utils.py:307-325) only RANKS the
// pairs; the reference's answer is decided by the few pairs within rounding distance of the best one.
// So the Gram is computed here from operands split into two FP16 halves (mfx_split16),
//        a = hi + lo (+ r),  |r| <= 2^-21 |a|,      c~ = hi.hi + hi.lo + lo.hi
// on v_mfma_f32_32x32x16_f16 (3 instructions per 32x32x16 block, 32x the FP64 MFMA rate), with unit-norm
// columns so that c~ is the cosine of the pair up to |c~ - c| <= DC (MFX_S_DC below: 1.5e-5, a bound under one measured
// assumption about the matrix pipe's FP32 summation; 13x the largest error measured).
// For a pair whose optimum has two positive weights the score S = |y|^2 - residual obeys dS/dc = -2 w1 w2
// with w1 w2 <= |y|^2 / 2 (c >= 0), so |S(c~) - S(c)| <= DC |y|^2 =: m.  Every pair with S(c~) >= thr is
// appended to a ring in LDS, thr = (largest S(c~) seen) - 2m, which can only drop pairs that are not the
// optimum; nearly collinear pairs (1 - c~^2 < 1e-3), where S(c) is ill-conditioned, go through an
// interval upper bound instead.  The survivors (typically < 20 of 611 524) are evaluated by the same
// exact stage as in fit_k2.hip (reference arithmetic and order, strict-'<' first hit, family expansion).
// A ring entry that is overwritten while it could still matter raises a flag and the voxel is redone
// by the FP64 kernel (host side, mfx_api.hip), so the result never depends on the ring size.
//
// Structure: one 512-thread workgroup per voxel, 8 waves = 8 row tiles of 32 atoms of D1 per round; a
// wave keeps its tile (hi and lo, K = 16*KS) in 8*KS VGPRs; D2 is generated 32 atoms at a time into a
// double-buffered LDS image laid out in MFMA fragment order (ds_read_b128, conflict-free), waves 0-3 and
// 4-7 alternating between the MFMAs of a chunk and VALU work (pair screen + generation) half-step by
// half-step; a last round with one row tile left is shared by all waves.  Everything that only ranks reads
// an FP32 copy of the table, two adjacent atoms per 16-byte load (the vector-memory pipe, not the matrix
// pipe, is what this kernel saturates next to VALU issue: DESIGN.md 4.0/4.1).
//
// XC = true: the same sweep for the class with one fixed extra column ([N, N, 1]: two fascicles + CSF), the column projected
// out through a spare measurement row; it writes per-voxel short lists for fit_k2x.hip's exact stage instead of running
// one (see the comment at the kernel and DESIGN.md 4.3b).
#pragma once
#include "fit_k2.hip"

typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef _Float16 h4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef int i32x4 __attribute__((ext_vector_type(4)));

// Bound on |c~ - c| (cosine units).  A statement under ONE measured assumption:
//   operands: every rotated entry is one FP32 fma of FP32 table values (<= 3 roundings): |da| <= 2.4e-7 |a|  -> 4.8e-7
//   split:    a = hi + lo + r, |r| <= 2^-21 |a|; dropped lo.lo + r.b + a.r <= 2^-19 |a b| per term           -> 1.9e-6
//   matrix pipe: ASSUMPTION - one v_mfma_f32_32x32x16_f16 returns its 17 addends' sum (16 exact products + accumulator)
//             within kappa 2^-24 (|c| + sum |a_k b_k|), kappa <= 5.1: the largest value tools/micro/mfma_sum_model.hip
//             finds over 15 adversarial operand families, 1.6e7 cases (profiles/r03_micro_mfma_sum_model.txt: 5.02;
//             2.0 on positive dictionary-like operands; the pipe does NOT round once - 12-46 % of the results differ
//             from the correctly rounded sum); 39 dependent instructions, every partial sum <= sum |a_i b_i| <= |a||b|
//             (Cauchy-Schwarz), the hi.lo / lo.hi addends 2^-10 of it:  39 x 5.1 x 2^-24 x 1.002                -> 1.19e-5
//   total 1.43e-5 <= MFX_S_DC.  (Measured: worst 1.14e-6 over 46 M adversarial pairs, tools/micro/split_mfma_error.hip;
//   and every voxel audits one pseudo-random pair of its own, k2s_shared.h.)
//   The 16-row form of the shared last row tile (k2s_round.h) runs v_mfma_f32_16x16x32_f16: 33 addends per instruction,
//   3 (KS + 1) / 2 dependent instructions (21 at KS = 13).  The same families through that instruction: kappa_16 = 5.20
//   (profiles/tail16_micro_mfma_sum_model.txt), and 21 x 5.20 = 109 <= 39 x 5.1 = 199 (kappa_16 <= 9.4 would do; likewise
//   24 x 5.20 <= 48 x 5.1 at KS = 16): the statement holds unchanged and that tile screens with the same DC.  Measured with
//   the kernel's split and order at K = 208: worst |c~ - c| 1.16e-6 (1.18e-6 at K = 256; profiles/tail16_micro_split_mfma_error.txt).
#ifndef MFX_S_DC
#define MFX_S_DC 1.5e-5
#endif
// The matrix-pipe term grows with the number of dependent instructions, 3 per k-step: longer protocols (KS = 16: up to 256
// measurements here, KS = 24 / 35: the wide kernel) get the margin the same statement gives for them, with the same 5 % of head
// room: 1.05 (2.38e-6 + 3 KS x 3.046e-7) = 1.79e-5, 2.55e-5, 3.61e-5.  (The audit of the wide kernel at 302 / 551 measurements:
// largest |c~ - c| 9.9e-7 / 1.19e-6.)
template <int KS>
__host__ __device__ constexpr double mfx_s_dc() { return KS <= 13 ? (double)MFX_S_DC : 1.05 * (2.38e-6 + 3.0 * KS * 3.046e-7); }
#define MFX_S_DENMIN 1e-3   // below this 1 - c~^2 the pair goes through the interval bound
#define MFX_S_BOUND 0x40000000   // ring entry flag (in .j): .score is an upper bound (interval bound, single atom), not S(c~)
#define MFX_S_GUARD 0.25    // run-time guard: an exactly evaluated pair whose screening score was off by more than this
                            // fraction of the margin DC |y|^2 sends the voxel to the FP64 kernel (and is counted)

// bit pattern of max(x, +0): non-negative doubles order like unsigned integers (LDS atomicMax)
__device__ __forceinline__ unsigned long long mfx_nonneg_bits(double x) {
  return (unsigned long long)__double_as_longlong(x > 0.0 ? x : 0.0);
}

// wave-wide maximum of NON-NEGATIVE values, rounded down to FP32, without LDS traffic: four DPP butterfly steps inside
// the rows of 16 lanes, then the four row values through scalar registers.  (wave_max's __shfl_xor is six dependent
// ds_bpermute round trips, ~800 of the ~2 600 cycles a register group cost in the FP64 pass while seven waves wait at
// the period's barrier; the result only feeds the threshold, where 6e-8 relative is 0.6 % of the margin.)
template <int CTRL>
__device__ __forceinline__ float mfx_dpp_max_f32(float v) {
  const int o = __builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, false);
  return fmaxf(v, __int_as_float(o));
}
__device__ __forceinline__ double mfx_wave_max_down(double x) {
  float v = (float)x * (1.0f - 1.2e-7f);   // <= x
  v = mfx_dpp_max_f32<0xb1>(v);    // quad_perm [1,0,3,2]
  v = mfx_dpp_max_f32<0x4e>(v);    // quad_perm [2,3,0,1]
  v = mfx_dpp_max_f32<0x141>(v);   // row_half_mirror
  v = mfx_dpp_max_f32<0x140>(v);   // row_mirror
  const int b = __float_as_int(v);
  const float r0 = __int_as_float(__builtin_amdgcn_readlane(b, 0)), r1 = __int_as_float(__builtin_amdgcn_readlane(b, 16)),
              r2 = __int_as_float(__builtin_amdgcn_readlane(b, 32)), r3 = __int_as_float(__builtin_amdgcn_readlane(b, 48));
  return (double)fmaxf(fmaxf(r0, r1), fmaxf(r2, r3));
}
// 1/x for a positive, normal x to ~1e-14 relative: FP32 reciprocal + one Newton step (an IEEE FP64 division is ~10
// quarter-rate instructions; the ranking quantities of the FP64 pass carry a margin of 1e-5)
__device__ __forceinline__ double mfx_rcp_nr(double x) {
  const double r0 = (double)__builtin_amdgcn_rcpf((float)x);
  return fma(r0, fma(-x, r0, 1.0), r0);
}

// value of lane `l` (compile-time constant) in every lane: v_readlane_b32 x 2, no ds_bpermute index arithmetic
__device__ __forceinline__ double mfx_readlane_f64(double v, int l) {
  const long long b = __double_as_longlong(v);
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(b & 0xffffffffll), l);
  const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(b >> 32), l);
  return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

// Neither operand is normalised: the FP32 screening table is pre-scaled on the host so that its values are <= 128,
// the accumulator holds cosine * |d1| * |d2| and the norms sit in the per-atom constants of the pair screen.  Both
// operands are split WITHOUT rescaling the low half:  f = hi + lo + r,  hi = f with its mantissa truncated to 10 bits
// (exact in FP16),  lo = fp16(f - hi),  |r| <= 2^-21 |f|.  With |f| <= 128 the low halves sit around 2^-10 |f|:
// normal FP16 numbers for all but negligible entries (an FP16 subnormal still resolves 6e-8, i.e. ~1e-10 of a column
// norm), so hi.hi, hi.lo and lo.hi can share ONE FP32 accumulator.
__device__ __forceinline__ void mfx_split16(float f, _Float16& hi, _Float16& lo) {
  // f must be ONE rounded FP32 value for both uses below (the compiler may otherwise fold the producing multiply
  // into a mixed-precision FMA for one use and not for the other: the halves then miss f by an FP16 ulp)
  asm("" : "+v"(f));   // not volatile: an opaque value, free to schedule
  const float h = __uint_as_float(__float_as_uint(f) & 0xffffe000u);
  hi = (_Float16)h;
  lo = (_Float16)(f - h);
}

#include "k2s_shared.h"
#include "k2s_tail16_map.h"

// BR: the protocol has G-bracketed rows (screening through the plan's virtual shells, exact stage as mfx_eval_br)
// NB: LDS images of D2 chunks: 3 (one workgroup barrier per chunk) where they fit beside the rest, else 2 (two barriers)
// XC: the voxel class has one fixed extra column x besides the two fascicles (sub-dictionaries [N, N, 1]: CSF).  Leaving
//     x unconstrained turns the problem into a two-atom problem in the orthogonal complement of x: atoms
//     d' = d - u x^ (u = d.x^, x^ = x/|x|), signal y' = y - (y.x^) x^, and  y.x^^2 + S2(d1', d2'; y')  bounds the score of
//     every support made of d1, d2 and x from above.  The projected cross product d1'.d2' = d1.d2 - u1 u2 comes out of
//     the SAME MFMAs: one spare padded measurement row carries -u1 in the A operand and u2 in the B image.  Statistics,
//     pair screen, FP64 criteria and ring then run unchanged on projected quantities (norms |d'|, z' = d'.y'/|d'|, the
//     margin DC amplified by max|d|/|d'| of the two dictionaries); the threshold only rises with pairs whose
//     relaxed solution keeps x's weight non-negative (then it IS a feasible score).  There is no exact stage here: the
//     ring entries that reach the final threshold go to a per-voxel list for fit_k2x.hip's exact stage (list mode),
//     which also owns every support with fewer than two fascicle atoms.
template <int KS, bool BR = false, int NB = 3, bool XC = false>
__global__ __launch_bounds__(512, 2) void mfx_fit_k2s_kernel(FitK2Args a) {
  constexpr int WG = 512, NW = 8;
  constexpr int MP = KS * 16;  // padded measurement count
  extern __shared__ double smem[];
  int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int lr = lane & 31, lh = lane >> 5;
  [[maybe_unused]] const int M = a.P.M;
  const int N = a.T.N, ldn = a.T.ldn;
  const int NP = (N + 31) & ~31;  // atoms padded to a multiple of 32
  const int ntiles = NP >> 5;
  const int vox = a.vox_list ? a.vox_list[a.vox_base + blockIdx.x] : a.vox_base + (int)blockIdx.x;

  // ---- LDS layout, prologue (phases 0 and 1: signal, descriptors, column statistics, margins, starting threshold): k2s_shared.h
  const K2sLds<KS, NB, BR, XC, NW * 64> L(smem, NP);
  K2S_UNPACK(L);
  // A shape with ONE row tile left after full rounds of eight (N = 782: 25 = 3*8 + 1) shares that tile among all waves, each
  // building the B operand of its column tiles straight from the table: a read of all of D2, the same bytes phase 1's
  // statistics pass reads.  So (!XC) that tile goes FIRST and makes D2's statistics on its way: phase 1 is skipped, and its
  // best-single-atom steps follow the pass.  (XC: the projected statistics and the margin's amplification must be known
  // before anything is screened - phase 1 as ever, the shared tile last.)
  const bool fused = !XC && (ntiles > 1) && (ntiles % NW == 1);
  const K2sVoxel VX = k2s_prologue<KS, NB, BR, XC, NW * 64, WG, !XC>(a, L, vox, tid, fused);
  const double y_sq = VX.y_sq, yx = VX.yx, ramp = VX.ramp, dc_eff = VX.dc_eff, mrg = VX.mrg, etol = VX.etol;
  (void)y_sq; (void)yx;
  const float2* __restrict__ tab32 = a.P.tab32s;   // FP32 copy of the table (== a.T.tab32 unless the plan has virtual shells): everything that only RANKS
  auto tab32_at = [&](int ro, int n) -> float2 { return *(const float2*)((const char*)tab32 + ((unsigned)(ro + n) << 3)); };
  // two adjacent atoms (n even) in one 16-byte load: {ylo_n, slope_n, ylo_n+1, slope_n+1}
  auto tab32x2_at = [&](int ro, int n) -> f32x4 { return *(const f32x4*)((const char*)tab32 + ((unsigned)(ro + n) << 3)); };
  auto push = [&](double S, int i, int j) { k2s_push(L, a.scap, S, i, j); };

  MFX_STAMP(2);
#ifdef MFX_STAMPS_RND
  if (a.stamps && tid == 0) a.stamps[(size_t)blockIdx.x * 16] = __builtin_amdgcn_s_memtime();
#endif
  const int nrounds = (ntiles + NW - 1) / NW;
  // the voxel's audited pair (k2s_shared.h): its row tile and column chunk; the shared last row tile is not audited
#ifdef MFX_EXP_NOAUDIT   // timing experiment
  const int aud_key = -1;
#else
  const int aud_key = a.audit ? k2s_audit_key(k2s_audit_hash(vox), (ntiles % NW == 1 && ntiles > 1) ? ntiles - 1 : ntiles, ntiles) : -1;
#endif
  // The body of one round is k2s_round.h, included as plain text.  XC: one copy in the loop it has always been in, the
  // shared tile decided per round at run time (K2S_ROUND_MODE 0).  Otherwise two copies, each without the other's
  // registers: the shared last row tile (1), which goes first - its pass over D2 makes the statistics the full rounds
  // screen with - and the full rounds (2).
  if constexpr (XC) {
    for (int round = 0; round < nrounds; ++round) {
#define K2S_ROUND_MODE 0
#include "k2s_round.h"
#undef K2S_ROUND_MODE
    }
  } else {
    if (fused) {
      for (int round = nrounds - 1; round < nrounds; ++round) {   // (once: the body leaves through `continue`)
#define K2S_ROUND_MODE 1
#include "k2s_round.h"
#undef K2S_ROUND_MODE
      }
    }
    const int nfull = fused ? nrounds - 1 : nrounds;
    for (int round = 0; round < nfull; ++round) {
#define K2S_ROUND_MODE 2
#include "k2s_round.h"
#undef K2S_ROUND_MODE
    }
  }
  k2s_finish<KS, NB, BR, XC, NW * 64, WG>(a, L, VX, vox, wave, lane);
}
