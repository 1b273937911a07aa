// sos_shared.h -- what predict.hip (the forward model of multi-shell protocols) and predict2d.hip (that of 2-D protocols)
// share: the counter-based noise generator of include/mfx_predict.h, the sum-of-squares magnitude of one element, and the
// fixed-order sum over a wave.  Every translation unit gets its own copy (anonymous namespace).
//
// Noise generator: Philox4x32-10 (Salmon et al., SC'11) written out below, keyed by the 64-bit seed, counter =
// (element index lo, hi, coil, MFX_SOS_STREAM).  Four output words -> u1 in (0, 1] and u2 in [0, 1) with 53 bits each
// -> one Box-Muller pair = one coil's in-phase and quadrature noise.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace {

constexpr uint32_t MFX_SOS_STREAM = 0x534f534du;  // fourth counter word: keeps this use of a seed apart from any later one

__host__ __device__ __forceinline__ uint32_t mulhi32(uint32_t a, uint32_t b) {
  return (uint32_t)(((unsigned long long)a * b) >> 32);
}

// Philox4x32-10: counter c[4], key (k0, k1) -> c[4]
__host__ __device__ __forceinline__ void philox4x32_10(uint32_t c[4], uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = mulhi32(0xD2511F53u, c[0]), lo0 = 0xD2511F53u * c[0];
    const uint32_t hi1 = mulhi32(0xCD9E8D57u, c[2]), lo1 = 0xCD9E8D57u * c[2];
    const uint32_t n0 = hi1 ^ c[1] ^ k0, n2 = hi0 ^ c[3] ^ k1;
    c[0] = n0; c[1] = lo1; c[2] = n2; c[3] = lo0;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
}

// sqrt( sum_j (S0 + sg a_j)^2 + (sg b_j)^2 ), summed as the reference does: (Y + in-phase^2) + quadrature^2
__device__ __forceinline__ double sos_value(double S0, double sg, int ncoils, unsigned long long seed, unsigned long long idx) {
  if (sg == 0.0) return sqrt((double)ncoils) * fabs(S0);
  double acc = 0.0;
  for (int j = 0; j < ncoils; ++j) {
    uint32_t c[4] = {(uint32_t)idx, (uint32_t)(idx >> 32), (uint32_t)j, MFX_SOS_STREAM};
    philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
    const double u1 = ((double)(((unsigned long long)(c[0] >> 5) << 26) | (c[1] >> 6)) + 1.0) * 0x1p-53;   // (0, 1]
    const double u2 = (double)(((unsigned long long)(c[2] >> 5) << 26) | (c[3] >> 6)) * 0x1p-53;           // [0, 1)
    const double r = sqrt(-2.0 * log(u1));
    double sn, cs;
    sincospi(2.0 * u2, &sn, &cs);
    const double p = S0 + sg * (r * cs), q = sg * (r * sn);
    acc = (acc + p * p) + q * q;
  }
  return sqrt(acc);
}

__device__ __forceinline__ double wave_sum(double x) {   // fixed order: lane pairs 32, 16, ..., 1 apart; every lane gets the sum
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x = x + __shfl_xor(x, o, 64);
  return x;
}

}  // namespace
