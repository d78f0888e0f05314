// Counter-based random numbers of the augmentation and dropout kernels (d_aug.hip, d_diffusion.hip, dropout.hip): Philox4x32-10 (Salmon et al., "Parallel random
// numbers: as easy as 1, 2, 3", SC'11), the map of a word to the open unit interval, and Box-Muller in fp32.
//   uniform u = ((x >> 9) + 0.5) * 2^-23: 2^23 values, every one exact in fp32, inside the OPEN interval (0, 1): log(u) is finite
//   normals   r = sqrt(-2 log(u0)), t = 2 pi u1: (r cos t, r sin t), all in fp32
#pragma once
#include "common.h"

namespace {

__device__ __forceinline__ uint4 philox4x32_10(uint4 c, uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, c.x), lo0 = 0xD2511F53u * c.x;
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c.z), lo1 = 0xCD9E8D57u * c.z;
    c = make_uint4(hi1 ^ c.y ^ k0, lo1, hi0 ^ c.w ^ k1, lo0);
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return c;
}

__device__ __forceinline__ float uniform_open(uint32_t x) { return ((float)(x >> 9) + 0.5f) * 1.1920928955078125e-07f; }

__device__ __forceinline__ void box_muller(uint32_t a, uint32_t b, float& n0, float& n1) {
  const float r = sqrtf(-2.0f * logf(uniform_open(a)));
  float sn, cs;
  sincosf(6.283185307179586f * uniform_open(b), &sn, &cs);
  n0 = r * cs;
  n1 = r * sn;
}

constexpr int STREAM_GRID_MAX_BLOCKS = 4096;

inline int stream_grid(long total) {      // sized to the chip as the streaming passes of elementwise.hip are: 256 CUs x 16 blocks at most
  const long b = (total + 255) / 256;
  return (int)(b < 1 ? 1 : b > STREAM_GRID_MAX_BLOCKS ? STREAM_GRID_MAX_BLOCKS : b);
}

}  // namespace
