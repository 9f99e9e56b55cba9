// Counter-based random numbers: bit-compatible with easygaussiansplatting_amd/scene.py (uniform01 / normal).
// Element e of stream s is a pure function of (seed, s, e) -- no generator state -- so data-parallel replicas draw
// identical numbers without communicating.  Shared by egs_density.hip (split offsets) and egs_mcmc.hip (sampling,
// position noise).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace egs {

__device__ __forceinline__ uint64_t splitmix64(uint64_t x) {
  uint64_t z = x + 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
__device__ __forceinline__ double uniform01(uint64_t seed, uint64_t stream, uint64_t e) {
  const uint64_t key = splitmix64(seed * 0x100000001B3ull + stream);
  uint64_t bits = splitmix64(e ^ key);
  bits = splitmix64(bits + key);
  return (double)(bits >> 11) * (1.0 / 9007199254740992.0);
}
__device__ __forceinline__ float unit_normal(uint64_t seed, uint64_t stream, uint64_t e) {
  double u1 = uniform01(seed, 2 * stream + 1000, e);
  const double u2 = uniform01(seed, 2 * stream + 1001, e);
  u1 = u1 > 1e-300 ? u1 : 1e-300;
  return (float)(sqrt(-2.0 * log(u1)) * cos(6.283185307179586476925 * u2));
}

}  // namespace egs
