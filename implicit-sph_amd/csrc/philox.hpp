// philox.hpp -- the counter-based generator shared by the random stress (body_force.hpp) and the start vector of the
// eigenvalue estimate (eig_estimate.hpp): a value is a function of (counter, key) alone, whichever thread asks for it.
#pragma once
#include <hip/hip_runtime.h>

namespace isph {

// Philox4x32-10 (Salmon, Moraes, Dror, Shaw: Parallel random numbers: as easy as 1, 2, 3, SC'11)
__device__ __forceinline__ void philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1,
                                              unsigned out[4]) {
  for (int round = 0; round < 10; ++round) {
    const unsigned hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const unsigned hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    c0 = hi1 ^ c1 ^ k0; c1 = lo1; c2 = hi0 ^ c3 ^ k1; c3 = lo0;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// two 32-bit words -> a uniform in (0, 1]: the upper 53 bits, centred in their cell
__device__ __forceinline__ double philox_uniform(unsigned hi, unsigned lo) {
  const unsigned long long w = ((unsigned long long)hi << 32) | lo;
  return ((double)(w >> 11) + 0.5) * 0x1.0p-53;
}

}  // namespace isph
