// Thread-to-element map and grid sizing of the GroupNorm streaming and reduction passes (norm.hip) and of their dropout counterparts
// (dropout.hip): a thread owns one 8-channel octet (one 16-byte vector per pixel) and a strided set of pixels.
#pragma once
#include "common.h"
#include <cstdlib>

namespace {

struct Map {
  int noct, pl, active, chunk;
};
__host__ __device__ inline Map make_map(int C) {
  Map m;
  m.noct = C / 8;
  m.pl = 256 / m.noct;
  if (m.pl < 1) m.pl = 1;
  m.active = m.pl * m.noct;
  m.chunk = m.pl * 16;
  return m;
}

// reductions: 4x more pixels per block than the streaming passes (4x fewer global atomics per channel)
__host__ __device__ inline Map make_map_red(int C, int mult) {
  Map m = make_map(C);
  m.chunk = m.pl * mult;   // mult in {16, 32, 64}: chosen by the host so that small tensors still fill the chip
  return m;
}
inline int red_mult(int B, int HW, int C) {
  const Map m = make_map(C);
  // fewest workgroups a larger chunk must still leave (JG_GN_RED_MINBLK, A/B; see the statistics pass below: the closing global atomics of every
  // workgroup weigh more than an underfilled grid on the CUT generators' maps)
  static const int minblk = getenv("JG_GN_RED_MINBLK") ? atoi(getenv("JG_GN_RED_MINBLK")) : 2048;
  for (int mult = 64; mult > 16; mult >>= 1)
    if ((long)B * ((HW + m.pl * mult - 1) / (m.pl * mult)) >= minblk) return mult;
  return 16;
}

// Deterministic forms (JG_DETERMINISTIC 1, `det`): ONE workgroup per image walks all its pixels (no cross-workgroup atomics), and the
// threads that share a channel octet are combined by an ORDERED sum over their LDS slots instead of ds_add_f32 chains: the result does not
// depend on the order in which waves and workgroups happen to run.  s_part: 256 threads x 16 partial sums behind the [C][2] row.
__device__ __forceinline__ void ordered_octet_sum(float* s_acc, const float (&s1)[8], const float (&s2)[8], const Map& mp, int C, bool active) {
  float* s_part = s_acc + 2 * C;
  const int tid = threadIdx.x;
  if (active) {
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      s_part[tid * 16 + q * 2] = s1[q];
      s_part[tid * 16 + q * 2 + 1] = s2[q];
    }
  }
  __syncthreads();
  for (int i = tid; i < 2 * C; i += 256) {
    const int c = i >> 1, k = i & 1, co = c >> 3, q = c & 7;
    float s = 0.f;
    for (int pl = 0; pl < mp.pl; ++pl) s += s_part[(pl * mp.noct + co) * 16 + q * 2 + k];
    s_acc[i] = s;
  }
}

inline bool bad_shape(int B, int HW, int C) { return B < 1 || HW < 1 || C < 8 || (C % 8) || C > 2048 || B > 65535; }

}  // namespace
