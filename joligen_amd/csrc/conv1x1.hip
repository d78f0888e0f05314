// Streaming 1x1 convolution for the wide, shallow layers of the UNet (skip / shortcut convs at full resolution: 64 -> 128,
// 64 -> 192, 128 -> 64 ... channels on 32 x 256^2 pixels).  These are HBM-bound (a few hundred FLOP per byte at most) and the
// generic LDS-DMA implicit-GEMM kernel reaches only ~2 TB/s on them: one K step per tile leaves its pipeline nothing to overlap.
//
// Here nothing goes through LDS: MFMA computes D^T = W . X^T per 16-pixel tile,
//   A operand = weights (row = output channel), loaded ONCE per wave into registers for the whole kernel;
//   B operand = pixels  (col = pixel): lane (l & 15, l >> 4) loads 16 contiguous bytes of pixel row (l & 15) -- a wave instruction
//               covers 16 full 64-byte segments, no im2col, no barrier;
//   D         = [16 output channels] x [16 pixels]: a lane owns 4 consecutive channels of ONE pixel; the weight rows of two MFMA tiles
//               are interleaved so that a lane's 2 x 4 channels are 8 consecutive ones -> one 16-byte store (and one 16-byte read of
//               the residual) per lane and tile pair.
// A wave keeps the fragments of its next tiles in flight; the plain form walks tiles with a stride of the total wave count, the two forms
// with a fused GroupNorm pass walk contiguous runs (conv1x1_stream_runs_kernel below).
//   y = alpha * conv + bias + res_scale * res     (same epilogue contract as the other convolution kernels)
#include <stdlib.h>

#include "conv_params.h"

namespace {

__device__ __forceinline__ float act_rt(float u, int act) {
  return act == JG_ACT_SILU ? silu_f(u) : act == JG_ACT_RELU ? fmaxf(u, 0.f) : act == JG_ACT_LRELU ? (u > 0.f ? u : 0.2f * u) : u;
}

// The plain form (no fused GroupNorm pass; the SegFormer / CUT legs): a wave walks pixel tiles with a stride of the total wave count.
template <typename T, int PAIRS, int KS>
__global__ __launch_bounds__(256, 2) void conv1x1_stream_kernel(ConvP p, int ntiles) {
  const int lane = threadIdx.x & 63;
  const int a = lane & 15, g = lane >> 4;
  const int n0 = blockIdx.y * (PAIRS * 32);
  const T* __restrict__ x = (const T*)p.x;
  const T* __restrict__ w = (const T*)p.w;
  const T* __restrict__ res = (const T*)p.res;
  T* __restrict__ y = (T*)p.y;

  // weights: tile (pair, half) row a  <->  output channel n0 + pair*32 + (a >> 2)*8 + half*4 + (a & 3)
  uint4 wf[PAIRS][2][KS];
#pragma unroll
  for (int pr = 0; pr < PAIRS; ++pr)
#pragma unroll
    for (int hf = 0; hf < 2; ++hf) {
      const int n = n0 + pr * 32 + (a >> 2) * 8 + hf * 4 + (a & 3);
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) wf[pr][hf][ks] = *reinterpret_cast<const uint4*>(w + (long)n * p.ldw + ks * 32 + g * 8);
    }
  // bias of this lane's 8 channels per pair: n0 + pair*32 + g*8 + 0..7
  float bs[PAIRS][8];
#pragma unroll
  for (int pr = 0; pr < PAIRS; ++pr)
#pragma unroll
    for (int j = 0; j < 8; ++j) bs[pr][j] = p.bias ? p.bias[n0 + pr * 32 + g * 8 + j] : 0.f;

  const int wave = blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = gridDim.x * 4;
  auto load_tile = [&](int t, uint4* xf) {
    const T* px = x + ((long)t * 16 + a) * p.ldx + g * 8;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) xf[ks] = *reinterpret_cast<const uint4*>(px + ks * 32);
  };
  // PF tiles of input fragments in flight per wave (a memory-bound stream needs ~64 KB in flight per CU)
  constexpr int PF = KS <= 2 ? 4 : (KS <= 4 ? 2 : 1);
  uint4 ring[PF][KS];
#pragma unroll
  for (int s = 0; s < PF; ++s)
    if (wave + s * nwaves < ntiles) load_tile(wave + s * nwaves, ring[s]);
  for (int base = wave; base < ntiles; base += PF * nwaves) {
#pragma unroll
    for (int s = 0; s < PF; ++s) {
      const int t = base + s * nwaves;
      if (t >= ntiles) break;
      const long prow = ((long)t * 16 + a);
      uint4 rf[PAIRS];
      if (res) {
#pragma unroll
        for (int pr = 0; pr < PAIRS; ++pr) rf[pr] = *reinterpret_cast<const uint4*>(res + prow * p.ldres + n0 + pr * 32 + g * 8);
      }
      f32x4 acc[PAIRS][2];
#pragma unroll
      for (int pr = 0; pr < PAIRS; ++pr) {
        acc[pr][0] = acc[pr][1] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
          acc[pr][0] = Mfma<T>::run(wf[pr][0][ks], ring[s][ks], acc[pr][0]);
          acc[pr][1] = Mfma<T>::run(wf[pr][1][ks], ring[s][ks], acc[pr][1]);
        }
      }
      const int tn = t + PF * nwaves;       // refill this slot as soon as its fragments have been consumed
      if (tn < ntiles) load_tile(tn, ring[s]);
#pragma unroll
      for (int pr = 0; pr < PAIRS; ++pr) {
        float o[8] = {acc[pr][0][0], acc[pr][0][1], acc[pr][0][2], acc[pr][0][3], acc[pr][1][0], acc[pr][1][1], acc[pr][1][2], acc[pr][1][3]};
        float r8[8];
        if (res) unpack8<T>(rf[pr], r8);
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = p.alpha * o[j] + bs[pr][j] + (res ? p.res_scale * r8[j] : 0.f);
        *reinterpret_cast<uint4*>(y + prow * p.ldy + n0 + pr * 32 + g * 8) = pack8<T>(o);
      }
    }
  }
}

// ---- the two fused forms (the UNet's skip convolutions) -----------------------------------------------------------------------------
// APPLY (!GNB): the launch also writes act(a x + b) of its INPUT (the GroupNorm apply pass of x, ConvP.aab / ay): the block column
// blockIdx.y == 0 transforms every 16-byte fragment it has loaded anyway and stores it; the (a, b) rows of the wave's current image
// sit in a wave-private LDS slot (2 Cin floats).
// GNB: the epilogue adds the GroupNorm-backward apply step of the output tensor (ConvP.bgx ...): per lane and tile pair two more 16-byte
// loads (gx, gdy; + the optional addends) and the per-channel coefficients (a, b, P, Q, R) of the block's PAIRS * 32 output channels from
// a wave-private LDS slot laid out [5][PAIRS * 32].
// Both are streams at their algorithmic byte count, and what they need is loads in flight:
//   - a wave owns a CONTIGUOUS run of tiles (as in conv3x3_c8_stream_kernel), so its coefficient slot is staged once per image the run
//     touches and not once per tile; the rows of the run's next image are requested into registers as soon as the current ones are staged
//     and only written to LDS at the boundary;
//   - every epilogue operand of a tile (gx, gdy, addends, residual: all PAIRS groups) is requested BEFORE the tile's MFMAs and pinned after
//     the ring refill has been issued: vmcnt retires in order and counts stores, so a load requested between two stores waits for the
//     earlier store's write round trip as well (conv_epilogue.h);
//   - KS >= 6, and GNB with 128 output channels per block: the block's weight fragments live in LDS in register-image order (conflict-free
//     ds_read_b128, 32 KB at <2, 8> / <4, 4>) -- as 64 - 128 VGPRs they left no room for the operands in flight (<2, 8, GNB> spilt).  The
//     other way to make room, 32 output channels per block, doubles the re-reads of x: 256 -> 768 @ 64^2 385 us against 219;
//   - ACT: the activation at compile time for the two the UNet schedule uses (SiLU, none); ACT_RT = ConvP.aact / bact at run time.
// The k-step order of the MFMAs and the fp32 epilogue expression are those of the plain kernel, so the outputs are too.
constexpr int ACT_RT = -1;

template <typename T, int PAIRS, int KS, bool GNB, int ACT>
__global__ __launch_bounds__(256, 2) void conv1x1_stream_runs_kernel(ConvP p, int ntiles) {
  constexpr bool WLDS = KS >= 6 || (GNB && PAIRS == 4);
  constexpr int NC = PAIRS * 32, NCOEF = GNB ? 5 * NC : 2 * KS * 32, NFRAG = PAIRS * 2 * KS;
  __shared__ __attribute__((aligned(16))) float s_ab[4 * NCOEF];
  __shared__ uint4 s_w[WLDS ? NFRAG * 64 : 1];
  const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);      // the run's bounds and branches are scalar
  const int a = lane & 15, g = lane >> 4;
  const int n0 = blockIdx.y * NC;
  const T* __restrict__ x = (const T*)p.x;
  const T* __restrict__ w = (const T*)p.w;
  const T* __restrict__ res = (const T*)p.res;
  T* __restrict__ y = (T*)p.y;

  // weight fragment f = (pair * 2 + half) * KS + ks: row a  <->  output channel n0 + pair*32 + (a >> 2)*8 + half*4 + (a & 3)
  auto load_wfrag = [&](int pr, int hf, int ks) {
    const int n = n0 + pr * 32 + (a >> 2) * 8 + hf * 4 + (a & 3);
    return *reinterpret_cast<const uint4*>(w + (long)n * p.ldw + ks * 32 + g * 8);
  };
  uint4 wf[WLDS ? 1 : NFRAG];
  if constexpr (WLDS) {
    for (int f = wv; f < NFRAG; f += 4) s_w[f * 64 + lane] = load_wfrag(f / (2 * KS), (f / KS) & 1, f % KS);
    __syncthreads();
  } else {
#pragma unroll
    for (int f = 0; f < NFRAG; ++f) wf[f] = load_wfrag(f / (2 * KS), (f / KS) & 1, f % KS);
  }
  float bs[PAIRS][8];
#pragma unroll
  for (int pr = 0; pr < PAIRS; ++pr)
#pragma unroll
    for (int j = 0; j < 8; ++j) bs[pr][j] = (!GNB && p.bias) ? p.bias[n0 + pr * 32 + g * 8 + j] : 0.f;      // GNB: an input gradient has no bias

  // this wave's run of tiles [t0, t1): the block columns of one blockIdx.x own the same runs, so the re-reads of x stay close in time
  const int wave = blockIdx.x * 4 + wv, nwaves = gridDim.x * 4;
  const int t0 = (int)((long)wave * ntiles / nwaves), t1 = (int)((long)(wave + 1) * ntiles / nwaves);
  if (t0 >= t1) return;
  auto load_tile = [&](int t, uint4* xf) {
    const T* px = x + ((long)t * 16 + a) * p.ldx + g * 8;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) xf[ks] = *reinterpret_cast<const uint4*>(px + ks * 32);
  };
  const bool do_apply = !GNB && blockIdx.y == 0;
  const bool coefs = GNB || do_apply;
  const bool has1 = GNB && p.badd1, has2 = GNB && p.badd2;
  float* wab = s_ab + wv * NCOEF;       // this wave's coefficient rows

  // coefficient rows of image b -> registers -> the wave's slot (same-wave LDS writes and reads stay in program order)
  // (named registers, not an array: hipcc keeps an array that two lambdas index in a loop in scratch)
  constexpr int NQ = 2 * KS * 32 / 4;       // APPLY: float4 per image; lane l moves l and l + 64
  struct Coef { float a, b, P, Q, R; } k0, k1;
  float4 q0, q1;
  auto coef_load = [&](int b) {
    if constexpr (GNB) {
      const float* ab = p.bab + ((long)b * p.N + n0 + lane) * 2;
      const float* pqr = p.bpqr + ((long)b * p.N + n0 + lane) * 3;
      k0 = Coef{ab[0], ab[1], pqr[0], pqr[1], pqr[2]};
      if (NC > 64) k1 = Coef{ab[128], ab[129], pqr[192], pqr[193], pqr[194]};
    } else {
      const float4* src = reinterpret_cast<const float4*>(p.aab + (long)b * (2 * KS * 32));
      if (lane < NQ) q0 = src[lane];
      if (64 + lane < NQ) q1 = src[64 + lane];
    }
  };
  auto coef_store = [&]() {
    if constexpr (GNB) {
      float* d = wab + lane;
      d[0] = k0.a, d[NC] = k0.b, d[2 * NC] = k0.P, d[3 * NC] = k0.Q, d[4 * NC] = k0.R;
      if (NC > 64) d[64] = k1.a, d[NC + 64] = k1.b, d[2 * NC + 64] = k1.P, d[3 * NC + 64] = k1.Q, d[4 * NC + 64] = k1.R;
    } else {
      if (lane < NQ) reinterpret_cast<float4*>(wab)[lane] = q0;
      if (64 + lane < NQ) reinterpret_cast<float4*>(wab)[64 + lane] = q1;
    }
  };

  const int tiles_per_img = (p.Ho * p.Wo) >> 4;
  int img = t0 / tiles_per_img;
  int tb = (img + 1) * tiles_per_img;       // first tile of the next image
  if (coefs) coef_load(img);
  // PF tiles of input fragments in flight per wave (a memory-bound stream needs ~64 KB in flight per CU)
  constexpr int PF = KS <= 2 ? 4 : (KS <= 4 ? 2 : 1);
  uint4 ring[PF][KS];
#pragma unroll
  for (int s = 0; s < PF; ++s)
    if (t0 + s < t1) load_tile(t0 + s, ring[s]);
  if (coefs) {
    coef_store();
    if (tb < t1) coef_load(img + 1);
  }
  for (int base = t0; base < t1; base += PF) {
#pragma unroll
    for (int s = 0; s < PF; ++s) {
      const int t = base + s;
      if (t >= t1) break;
      const long prow = ((long)t * 16 + a);
      if (coefs && t == tb) {           // wave-uniform: the run enters its next image; the rows were requested one image ago
        coef_store();
        ++img;
        tb += tiles_per_img;
        if (tb < t1) coef_load(img + 1);
      }
      // every epilogue operand of the tile, all PAIRS groups: in flight under the MFMAs
      uint4 rf[PAIRS], egx[PAIRS], egd[PAIRS], ea1[PAIRS], ea2[PAIRS];
      const int cg = n0 + g * 8;
      if constexpr (GNB) {
#pragma unroll
        for (int pr = 0; pr < PAIRS; ++pr) {
          egx[pr] = *reinterpret_cast<const uint4*>((const T*)p.bgx + prow * p.bldgx + cg + pr * 32);
          egd[pr] = *reinterpret_cast<const uint4*>((const T*)p.bgdy + prow * p.bldgdy + cg + pr * 32);
        }
        if (has1) {
#pragma unroll
          for (int pr = 0; pr < PAIRS; ++pr) ea1[pr] = *reinterpret_cast<const uint4*>((const T*)p.badd1 + prow * p.bldadd1 + cg + pr * 32);
        }
        if (has2) {
#pragma unroll
          for (int pr = 0; pr < PAIRS; ++pr) ea2[pr] = *reinterpret_cast<const uint4*>((const T*)p.badd2 + prow * p.bldadd2 + cg + pr * 32);
        }
      } else if (res) {
#pragma unroll
        for (int pr = 0; pr < PAIRS; ++pr) rf[pr] = *reinterpret_cast<const uint4*>(res + prow * p.ldres + cg + pr * 32);
      }
      __builtin_amdgcn_sched_barrier(0);      // (left alone, the scheduler sinks these loads below the MFMAs, next to their use)
      f32x4 acc[PAIRS][2];
#pragma unroll
      for (int pr = 0; pr < PAIRS; ++pr) {
        acc[pr][0] = acc[pr][1] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
          const int f0 = (pr * 2) * KS + ks, f1 = (pr * 2 + 1) * KS + ks;
          acc[pr][0] = Mfma<T>::run(WLDS ? s_w[f0 * 64 + lane] : wf[WLDS ? 0 : f0], ring[s][ks], acc[pr][0]);
          acc[pr][1] = Mfma<T>::run(WLDS ? s_w[f1 * 64 + lane] : wf[WLDS ? 0 : f1], ring[s][ks], acc[pr][1]);
        }
      }
      if (do_apply) {
        T* ay = (T*)p.ay + prow * p.lday + g * 8;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
          float f[8];
          unpack8<T>(ring[s][ks], f);
          const float4* c4 = reinterpret_cast<const float4*>(wab + (ks * 32 + g * 8) * 2);
#pragma unroll
          for (int k4 = 0; k4 < 4; ++k4) {
            const float4 c = c4[k4];      // (a, b) of channels 2 k4, 2 k4 + 1 of the octet
            const float u0 = c.x * f[2 * k4] + c.y, u1 = c.z * f[2 * k4 + 1] + c.w;
            f[2 * k4] = ACT == ACT_RT ? act_rt(u0, p.aact) : act_f<ACT>(u0);
            f[2 * k4 + 1] = ACT == ACT_RT ? act_rt(u1, p.aact) : act_f<ACT>(u1);
          }
          *reinterpret_cast<uint4*>(ay + ks * 32) = pack8<T>(f);
        }
      }
      // refill this slot as soon as its fragments have been consumed.  GNB: UNCONDITIONAL (the run's last PF tiles re-read themselves, out
      // of L1): behind a branch the operands' wait below would be a vmcnt(0), which waits for the refill as well.  APPLY has at most the
      // residual to wait for, and its short runs at 64^2 (4 tiles) would pay for the re-reads: 59 us against 56
      if (GNB) load_tile(t + PF < t1 ? t + PF : t, ring[s]);
      else if (t + PF < t1) load_tile(t + PF, ring[s]);
      __builtin_amdgcn_sched_barrier(0);
      // pin the operands: the wait for them stands here, behind nothing but the refill, and no wait sits between the stores below
      if constexpr (GNB) {
#pragma unroll
        for (int pr = 0; pr < PAIRS; ++pr) {
          asm volatile("" : "+v"(egx[pr].x), "+v"(egx[pr].y), "+v"(egx[pr].z), "+v"(egx[pr].w));
          asm volatile("" : "+v"(egd[pr].x), "+v"(egd[pr].y), "+v"(egd[pr].z), "+v"(egd[pr].w));
        }
        if (has1) {
#pragma unroll
          for (int pr = 0; pr < PAIRS; ++pr) asm volatile("" : "+v"(ea1[pr].x), "+v"(ea1[pr].y), "+v"(ea1[pr].z), "+v"(ea1[pr].w));
        }
        if (has2) {
#pragma unroll
          for (int pr = 0; pr < PAIRS; ++pr) asm volatile("" : "+v"(ea2[pr].x), "+v"(ea2[pr].y), "+v"(ea2[pr].z), "+v"(ea2[pr].w));
        }
      } else if (res) {
#pragma unroll
        for (int pr = 0; pr < PAIRS; ++pr) asm volatile("" : "+v"(rf[pr].x), "+v"(rf[pr].y), "+v"(rf[pr].z), "+v"(rf[pr].w));
      }
#pragma unroll
      for (int pr = 0; pr < PAIRS; ++pr) {
        float o[8] = {acc[pr][0][0], acc[pr][0][1], acc[pr][0][2], acc[pr][0][3], acc[pr][1][0], acc[pr][1][1], acc[pr][1][2], acc[pr][1][3]};
        if constexpr (GNB) {
          const int cl = pr * 32 + g * 8;
          float fx[8], fd[8], ca[8], cb[8], cP[8], cQ[8], cR[8];
          unpack8<T>(egx[pr], fx);
          unpack8<T>(egd[pr], fd);
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            *reinterpret_cast<float4*>(ca + 4 * h) = *reinterpret_cast<const float4*>(wab + cl + 4 * h);
            *reinterpret_cast<float4*>(cb + 4 * h) = *reinterpret_cast<const float4*>(wab + NC + cl + 4 * h);
            *reinterpret_cast<float4*>(cP + 4 * h) = *reinterpret_cast<const float4*>(wab + 2 * NC + cl + 4 * h);
            *reinterpret_cast<float4*>(cQ + 4 * h) = *reinterpret_cast<const float4*>(wab + 3 * NC + cl + 4 * h);
            *reinterpret_cast<float4*>(cR + 4 * h) = *reinterpret_cast<const float4*>(wab + 4 * NC + cl + 4 * h);
          }
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            o[j] = p.alpha * o[j];
            float du = fd[j];
            if (ACT == ACT_RT) {
              if (p.bact != JG_ACT_NONE) du *= act_grad_rt(ca[j] * fx[j] + cb[j], p.bact);
            } else if (ACT != JG_ACT_NONE) {
              du *= act_grad_f<ACT>(ca[j] * fx[j] + cb[j]);
            }
            o[j] += du * cP[j] + fx[j] * cQ[j] + cR[j];
          }
          if (has1) {
            float fa[8];
            unpack8<T>(ea1[pr], fa);
#pragma unroll
            for (int j = 0; j < 8; ++j) o[j] += p.bsc1 * fa[j];
          }
          if (has2) {
            float fa[8];
            unpack8<T>(ea2[pr], fa);
#pragma unroll
            for (int j = 0; j < 8; ++j) o[j] += p.bsc2 * fa[j];
          }
        } else {
          float r8[8];
          if (res) unpack8<T>(rf[pr], r8);
#pragma unroll
          for (int j = 0; j < 8; ++j) o[j] = p.alpha * o[j] + bs[pr][j] + (res ? p.res_scale * r8[j] : 0.f);
        }
        *reinterpret_cast<uint4*>(y + prow * p.ldy + cg + pr * 32) = pack8<T>(o);
        if (GNB) __builtin_amdgcn_sched_barrier(0);      // one channel group at a time: its unpacked operands and coefficient octets die here
      }
    }
  }
}

// ---- the same streaming scheme for the 3x3 stem (and the input gradient of the 3x3 head): Cin = 8 (one 16-byte chunk per tap) ----
// K = 9 taps x 8 channels = 72 -> 3 MFMA k-steps of 4 taps (the last three tap slots are zero); the B operand of lane (pixel a, group g)
// for k-step ks is the 16-byte pixel at tap ks*4 + g, read straight from global memory (zero outside the image).  The generic
// im2col kernel spends 375 us on 32 x 256^2 x (8 -> 64); the layer moves 33 MB in and 268 MB out.
template <typename T, int PAIRS>
__global__ __launch_bounds__(256, 2) void conv3x3_c8_stream_kernel(ConvP p, int ntiles) {
  constexpr int KS = 3;
  const int lane = threadIdx.x & 63;
  const int a = lane & 15, g = lane >> 4;
  const int n0 = blockIdx.y * (PAIRS * 32);
  const T* __restrict__ x = (const T*)p.x;
  const T* __restrict__ w = (const T*)p.w;
  const T* __restrict__ res = (const T*)p.res;
  T* __restrict__ y = (T*)p.y;
  const uint4 zero4 = make_uint4(0u, 0u, 0u, 0u);
  uint4 wf[PAIRS][2][KS];
#pragma unroll
  for (int pr = 0; pr < PAIRS; ++pr)
#pragma unroll
    for (int hf = 0; hf < 2; ++hf) {
      const int n = n0 + pr * 32 + (a >> 2) * 8 + hf * 4 + (a & 3);
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        const int tap = ks * 4 + g;
        wf[pr][hf][ks] = tap < 9 ? *reinterpret_cast<const uint4*>(w + (long)n * p.ldw + tap * 8) : zero4;
      }
    }
  float bs[PAIRS][8];
#pragma unroll
  for (int pr = 0; pr < PAIRS; ++pr)
#pragma unroll
    for (int j = 0; j < 8; ++j) bs[pr][j] = p.bias ? p.bias[n0 + pr * 32 + g * 8 + j] : 0.f;
  const int wave = blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = gridDim.x * 4;
  auto load_tile = [&](int t, uint4* xf) {
    const long pix = (long)t * 16 + a;
    const int px = pix % p.W, py = (pix / p.W) % p.H;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const int tap = ks * 4 + g;
      const int dy = tap / 3 - 1, dx = tap % 3 - 1;
      const bool ok = tap < 9 && (unsigned)(py + dy) < (unsigned)p.H && (unsigned)(px + dx) < (unsigned)p.W;
      xf[ks] = ok ? *reinterpret_cast<const uint4*>(x + (pix + (long)dy * p.W + dx) * 8) : zero4;
    }
  };
  // a wave owns a CONTIGUOUS run of tiles, so the fused GroupNorm statistics (sum, sum of squares per image and channel, from the
  // fp32 values) stay in registers until the image changes: one shuffle reduction + atomic pair per channel and image per wave
  const int per = (ntiles + nwaves - 1) / nwaves;
  const int t0 = wave * per, t1 = min(ntiles, t0 + per);
  const int tiles_per_img = (p.H * p.W) >> 4;
  float s1[PAIRS][8], s2[PAIRS][8];
#pragma unroll
  for (int pr = 0; pr < PAIRS; ++pr)
#pragma unroll
    for (int j = 0; j < 8; ++j) s1[pr][j] = s2[pr][j] = 0.f;
  int cur_b = t0 < t1 ? t0 / tiles_per_img : 0;
  auto flush = [&](int b) {
    float* base = p.stats + ((long)(b * p.nslots + wave % p.nslots) * p.ldstats) * 2;
#pragma unroll
    for (int pr = 0; pr < PAIRS; ++pr)
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        float u = s1[pr][j], v = s2[pr][j];
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) {
          u += __shfl_xor(u, o);
          v += __shfl_xor(v, o);
        }
        if (a == 0) {
          atomicAdd(base + (n0 + pr * 32 + g * 8 + j) * 2, u);
          atomicAdd(base + (n0 + pr * 32 + g * 8 + j) * 2 + 1, v);
        }
        s1[pr][j] = s2[pr][j] = 0.f;
      }
  };
  constexpr int PF = 2;
  uint4 ring[PF][KS];
#pragma unroll
  for (int s = 0; s < PF; ++s)
    if (t0 + s < t1) load_tile(t0 + s, ring[s]);
  for (int base = t0; base < t1; base += PF) {
#pragma unroll
    for (int s = 0; s < PF; ++s) {
      const int t = base + s;
      if (t < t1) {
        const long prow = ((long)t * 16 + a);
        if (p.stats) {
          const int b = t / tiles_per_img;
          if (b != cur_b) {
            flush(cur_b);
            cur_b = b;
          }
        }
        f32x4 acc[PAIRS][2];
#pragma unroll
        for (int pr = 0; pr < PAIRS; ++pr) {
          acc[pr][0] = acc[pr][1] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int ks = 0; ks < KS; ++ks) {
            acc[pr][0] = Mfma<T>::run(wf[pr][0][ks], ring[s][ks], acc[pr][0]);
            acc[pr][1] = Mfma<T>::run(wf[pr][1][ks], ring[s][ks], acc[pr][1]);
          }
        }
        if (t + PF < t1) load_tile(t + PF, ring[s]);
#pragma unroll
        for (int pr = 0; pr < PAIRS; ++pr) {
          float o[8] = {acc[pr][0][0], acc[pr][0][1], acc[pr][0][2], acc[pr][0][3], acc[pr][1][0], acc[pr][1][1], acc[pr][1][2], acc[pr][1][3]};
          float r8[8];
          if (res) unpack8<T>(*reinterpret_cast<const uint4*>(res + prow * p.ldres + n0 + pr * 32 + g * 8), r8);
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            o[j] = p.alpha * o[j] + bs[pr][j] + (res ? p.res_scale * r8[j] : 0.f);
            s1[pr][j] += o[j];
            s2[pr][j] += o[j] * o[j];
          }
          *reinterpret_cast<uint4*>(y + prow * p.ldy + n0 + pr * 32 + g * 8) = pack8<T>(o);
        }
      }
    }
  }
  if (p.stats && t0 < t1) flush(cur_b);
}

template <typename T>
void launch_c8(const ConvP& p, hipStream_t st) {
  const int ntiles = p.M / 16;
  const int ngroups = p.N / 64;
  int bx = (ntiles + 3) / 4;
  const int cap = 256 * 8 / ngroups > 64 ? 256 * 8 / ngroups : 64;
  if (bx > cap) bx = cap;
  jg_note_kernel("conv3x3_c8_stream_kernel");
  hipLaunchKernelGGL((conv3x3_c8_stream_kernel<T, 2>), dim3(bx, ngroups), dim3(256), 0, st, p, ntiles);
}

// (tried: the same LDS-free scheme for the 3x3 / 64 -> 64 layers at full resolution, weights of 32 output channels in registers and the
//  nine shifted pixel reads served by L1 / L2: 714 us against 208 us for the halo-resident kernel -- the 9x operand re-read through the
//  cache hierarchy costs far more than the halo kernel's unoverlapped phases; not kept)

// grid of the streaming 1x1 kernels: blockIdx.y = column group of PAIRS * 32 output channels; blockIdx.x = four waves that share the tiles with
// all other waves of the column.  About 2048 workgroups per launch where the tiles allow (two to four are resident per CU), one tile per wave
// at least: the 64^2 levels of the UNet (8192 tiles, up to 12 column groups) get 680 waves of 12 tiles per column
inline dim3 grid_1x1(int ntiles, int ngroups) {
  int bx = (ntiles + 3) / 4;
  const int cap = 256 * 8 / ngroups > 64 ? 256 * 8 / ngroups : 64;
  if (bx > cap) bx = cap;
  return dim3(bx, ngroups);
}

template <typename T, int PAIRS, int KS>
void launch_1x1_plain(const ConvP& p, hipStream_t st) {
  const int ntiles = p.M / 16;
  jg_note_kernel("conv1x1_stream_kernel");
  hipLaunchKernelGGL((conv1x1_stream_kernel<T, PAIRS, KS>), grid_1x1(ntiles, p.N / (PAIRS * 32)), dim3(256), 0, st, p, ntiles);
}

// the two fused forms: GNB = jg_conv1x1_gn_bwd_apply (ConvP.bgx ...), !GNB = jg_conv1x1_gn_apply (ConvP.aab ...)
template <typename T, int PAIRS, int KS, bool GNB>
void launch_1x1_runs(const ConvP& p, hipStream_t st) {
  const int ntiles = p.M / 16;
  const dim3 grid = grid_1x1(ntiles, p.N / (PAIRS * 32));
  const int act = GNB ? p.bact : p.aact;
  jg_note_kernel(GNB ? "conv1x1_stream_kernel+gn_bwd_apply" : "conv1x1_stream_kernel+gn_apply");
  if (act == JG_ACT_SILU) hipLaunchKernelGGL((conv1x1_stream_runs_kernel<T, PAIRS, KS, GNB, JG_ACT_SILU>), grid, dim3(256), 0, st, p, ntiles);
  else if (act == JG_ACT_NONE) hipLaunchKernelGGL((conv1x1_stream_runs_kernel<T, PAIRS, KS, GNB, JG_ACT_NONE>), grid, dim3(256), 0, st, p, ntiles);
  else hipLaunchKernelGGL((conv1x1_stream_runs_kernel<T, PAIRS, KS, GNB, ACT_RT>), grid, dim3(256), 0, st, p, ntiles);
}

template <typename T, int PAIRS, int KS>
void launch_1x1(const ConvP& p, hipStream_t st) {
  if (p.aab) launch_1x1_runs<T, PAIRS, KS, false>(p, st);
  else if (p.bgx) launch_1x1_runs<T, PAIRS, KS, true>(p, st);
  else launch_1x1_plain<T, PAIRS, KS>(p, st);
}

template <typename T>
bool dispatch_1x1(const ConvP& p, hipStream_t st) {
  const int ks = p.Cin / 32;
  const bool wide = p.N % 128 == 0;
  // round 5: 32-channel inputs (KS 1) and outputs that are a multiple of 32 but not of 64 (PAIRS 1) -- the stage-1 / stage-2 linear layers
  // of the SegFormer generator (32 -> 32 / 128, 128 -> 32, 64 -> 64 / 256, 256 -> 64 on 65 k - 262 k tokens), which the implicit-GEMM
  // kernel streams at 2.0 TB/s (profiles/r05_cut_pmc_hbm_traffic.md)
  if (!p.aab && !p.bgx) {
    if (ks == 1) {
      if (wide) launch_1x1_plain<T, 4, 1>(p, st);
      else if (p.N % 64 == 0) launch_1x1_plain<T, 2, 1>(p, st);
      else launch_1x1_plain<T, 1, 1>(p, st);
      return true;
    }
    if (p.N % 64) {
      switch (ks) {
        case 2: launch_1x1_plain<T, 1, 2>(p, st); return true;
        case 4: launch_1x1_plain<T, 1, 4>(p, st); return true;
        case 8: launch_1x1_plain<T, 1, 8>(p, st); return true;
        default: return false;
      }
    }
  } else if (ks == 1 || p.N % 64) {
    return false;
  }
  switch (ks) {
    case 2: wide ? launch_1x1<T, 4, 2>(p, st) : launch_1x1<T, 2, 2>(p, st); return true;
    case 4:
      // GNB with its weights in LDS fits 128 output channels per block (219 VGPRs): half the re-reads of dO, 128 -> 384 @ 128^2 353 -> 313 us,
      // 128 -> 256 247 -> 214.  With the weights in registers <4, 4> needs 256+ VGPRs (APPLY spills at 256)
      if (wide && p.bgx) launch_1x1_runs<T, 4, 4, true>(p, st);
      else launch_1x1<T, 2, 4>(p, st);
      return true;
    case 6: launch_1x1<T, 2, 6>(p, st); return true;
    case 8: launch_1x1<T, 2, 8>(p, st); return true;
    default: return false;
  }
}

}  // namespace

// true when the shape was handled here (gemm_nt.hip falls through to the generic kernel otherwise)
bool jg_conv1x1_try(int dtype, const ConvP& p, int nbatch, hipStream_t st) {
  if (p.res_up || p.x_up || p.y_pool) return false;   // half-resolution residuals / inputs: LDS-staged kernels only
  const bool off = jg_tune(JG_TUNE_CONV1X1) == 0;
  if (off && !p.aab && !p.bgx) return false;
  if (!p.aab && !p.bgx && nbatch == 1 && p.nh == 1 && p.R == 3 && p.S == 3 && p.pad == 1 && p.stride == 1 && !p.out_f32 && !(p.stats && p.stats_mode) && !p.reflect &&
      p.Cin == 8 && ((p.H * p.W) & 15) == 0 &&
      p.ldx == 8 && p.ldw == 72 && p.N % 64 == 0 && !(p.M & 15) && p.H == p.Ho && p.W == p.Wo && p.ldy % 8 == 0 && (!p.res || p.ldres % 8 == 0) &&
      (long)p.M >= 65536) {
    if (dtype == JG_F16) launch_c8<f16_t>(p, st);
    else if (dtype == JG_BF16) launch_c8<bf16_t>(p, st);
    else return false;
    return true;
  }
  if (nbatch != 1 || p.nh != 1 || p.R != 1 || p.S != 1 || p.pad != 0 || p.stride != 1 || p.out_f32 || p.stats || p.reflect) return false;
  if (p.Cin % 32 || p.Cin > 256 || p.N % 32 || (p.M & 15)) return false;
  if (p.ldx % 8 || p.ldy % 8 || p.ldw % 8 || (p.res && p.ldres % 8)) return false;
  // only where the layer is memory-bound: few hundred FLOP per byte; deep / low-resolution layers stay on the MFMA-tiled GEMM
  if ((long)p.M < 65536) return false;
  // round 6: 256 -> >= 256 channels is GEMM-shaped (128 FLOP per byte): the LDS-tiled kernel is faster there (the point-wise convolutions of the
  // mobile ResNet blocks at 64 x 64: 66 -> ~45 us, mobile_resnet_attn + [projected_d, basic] 347.5 -> 354.2 images/s); the fused GroupNorm forms
  // exist only here and stay
  if (!p.aab && !p.bgx && p.Cin >= 256 && p.N >= 256 && jg_tune(JG_TUNE_CONV1X1) < 2) return false;
  if (dtype == JG_F16) return dispatch_1x1<f16_t>(p, st);
  if (dtype == JG_BF16) return dispatch_1x1<bf16_t>(p, st);
  return false;
}
