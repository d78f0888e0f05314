// Discriminator-input augmentations of the GAN models (dataaug_D_noise and adaptive pseudo augmentation, APA):
//   jg_d_aug      out_d[b,h,w,c] = flag_d[b] ? alt_d[b,h,w,c] : src[b,h,w,c] + sigma * z[b,c,h,w]   for up to 4 targets d in one launch
//   jg_apa_update p <- clamp(p + sign(mean(sign(pred_real)) - target) * num / den, 0, 1)
// Both read their scalars (p, the Philox key) from DEVICE memory: no host value that changes between steps enters a launch.
//
// Random numbers: Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11), counter-based:
//   key     = the two 32-bit words of a device tensor (filled by the host side from torch's generator);
//   counter = (pixel h * W + w,  sample b,  stream id | (group of 4 channels) << 16,  call index)
// so that no two elements, samples, streams or call sites share a counter.  One call yields 4 words = 2 Box-Muller pairs = the normals
// of 4 channels of one pixel; a flag's uniform is word 0 of the counter (0, b, stream id of that target, call index).
// The generator, the uniform map and Box-Muller are in philox.h (shared with d_diffusion.hip).
#include "philox.h"

namespace {

constexpr int D_AUG_MAX = JG_D_AUG_MAX;

struct DAugTargets {
  const void* alt[D_AUG_MAX];
  const float* p[D_AUG_MAX];
  void* out[D_AUG_MAX];
  int32_t* flags[D_AUG_MAX];
  const float* u[D_AUG_MAX];
  uint32_t stream[D_AUG_MAX];
  int n;
};

// flags_d[b] = alt_d given && u_d[b] < p_d (0 for a target without alt); one thread per (target, sample)
__global__ void d_aug_flags_kernel(DAugTargets t, const uint32_t* __restrict__ key, uint32_t call, int B) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= t.n * B) return;
  const int d = i / B, b = i - d * B;
  if (!t.flags[d]) return;
  int f = 0;
  if (t.alt[d]) {
    const float u = t.u[d] ? t.u[d][b] : uniform_open(philox4x32_10(make_uint4(0u, (uint32_t)b, t.stream[d], call), key[0], key[1]).x);
    f = u < *t.p[d] ? 1 : 0;
  }
  t.flags[d][b] = f;
}

// one thread per 16-byte group of 8 channels of one pixel; `G` = Cpad / 8 groups per pixel
template <typename T>
__global__ __launch_bounds__(256) void d_aug_kernel(const T* __restrict__ src, DAugTargets t, float sigma, const float* __restrict__ z,
                                                    const uint32_t* __restrict__ key, uint32_t noise_stream, uint32_t call, int B, long HW,
                                                    int C, int G) {
  const bool noise = sigma != 0.f;
  const bool draw = noise && !z;
  const uint32_t k0 = draw ? key[0] : 0u, k1 = draw ? key[1] : 0u;
  const long total = (long)B * HW * G;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += gridDim.x * 256L) {
    const int g8 = (int)(i % G);
    const long bp = i / G;
    const int b = (int)(bp / HW);
    const long pix = bp - (long)b * HW;
    const int c0 = g8 * 8;
    bool fl[D_AUG_MAX], any_src = false;
#pragma unroll
    for (int d = 0; d < D_AUG_MAX; ++d) {
      fl[d] = d < t.n && t.alt[d] && t.flags[d][b] != 0;
      any_src |= d < t.n && !fl[d];
    }
    // 0xffff for a valid channel, 0 for a padding channel: the padding channels of every output are zero
    uint32_t m[4];
#pragma unroll
    for (int w = 0; w < 4; ++w) m[w] = (c0 + 2 * w < C ? 0xffffu : 0u) | (c0 + 2 * w + 1 < C ? 0xffff0000u : 0u);
    uint4 sv = make_uint4(0u, 0u, 0u, 0u);
    if (any_src) {
      sv = reinterpret_cast<const uint4*>(src)[i];
      if (noise && c0 < C) {
        float f[8], nz[8];
        unpack8<T>(sv, f);
        if (z) {
#pragma unroll
          for (int c = 0; c < 8; ++c) nz[c] = c0 + c < C ? z[((long)b * C + c0 + c) * HW + pix] : 0.f;
        } else {
#pragma unroll
          for (int q = 0; q < 2; ++q) {        // the two groups of 4 channels of this thread
            nz[4 * q] = nz[4 * q + 1] = nz[4 * q + 2] = nz[4 * q + 3] = 0.f;
            if (c0 + 4 * q < C) {
              const uint4 r = philox4x32_10(make_uint4((uint32_t)pix, (uint32_t)b, noise_stream | ((uint32_t)(2 * g8 + q) << 16), call), k0, k1);
              box_muller(r.x, r.y, nz[4 * q], nz[4 * q + 1]);
              if (c0 + 4 * q + 2 < C) box_muller(r.z, r.w, nz[4 * q + 2], nz[4 * q + 3]);
            }
          }
        }
#pragma unroll
        for (int c = 0; c < 8; ++c) f[c] = c0 + c < C ? fmaf(sigma, nz[c], f[c]) : 0.f;      // fp32, rounded once by pack8
        sv = pack8<T>(f);
      }
      sv = make_uint4(sv.x & m[0], sv.y & m[1], sv.z & m[2], sv.w & m[3]);
    }
#pragma unroll
    for (int d = 0; d < D_AUG_MAX; ++d) {
      if (d < t.n) {
        uint4 v = sv;
        if (fl[d]) {
          v = reinterpret_cast<const uint4*>(t.alt[d])[i];
          v = make_uint4(v.x & m[0], v.y & m[1], v.z & m[2], v.w & m[3]);
        }
        reinterpret_cast<uint4*>(t.out[d])[i] = v;
      }
    }
  }
}

// one block: signs counted as integers, then the update of p by thread 0
template <typename T>
__global__ __launch_bounds__(1024) void apa_update_kernel(const T* __restrict__ pred, long n, long stride, float* __restrict__ p,
                                                          float* __restrict__ adjust, float* __restrict__ s_out, float target, float num,
                                                          float den) {
  __shared__ int s_pos[16], s_neg[16];
  int pos = 0, neg = 0;
  for (long i = threadIdx.x; i < n; i += 1024) {
    const float v = to_f32(pred[i * stride]);
    pos += v > 0.f ? 1 : 0;
    neg += v < 0.f ? 1 : 0;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    pos += __shfl_down(pos, o, 64);
    neg += __shfl_down(neg, o, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    s_pos[threadIdx.x >> 6] = pos;
    s_neg[threadIdx.x >> 6] = neg;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    long np = 0, nn = 0;
    for (int w = 0; w < 16; ++w) {
      np += s_pos[w];
      nn += s_neg[w];
    }
    // the reference's order of operations, every step in fp32: s = sum(sign) / n;  adjust = sign(s - target);
    // lambda = (adjust * (B * every)) / (nimg * 1000);  p = p + lambda;  p < 0: p * 0;  p > 1: 1
    const float s = __fdiv_rn((float)(np - nn), (float)n);
    const float d = s - target;
    const float adj = d > 0.f ? 1.f : d < 0.f ? -1.f : 0.f;
    const float lambda = __fdiv_rn(adj * num, den);
    float pn = *p + lambda;
    if (pn < 0.f) pn = pn * 0.f;
    if (pn > 1.f) pn = 1.f;
    *p = pn;
    *adjust = adj;
    *s_out = s;
  }
}

}  // namespace

extern "C" int jg_d_aug(int dtype, const void* src, int nd, const void* const* alt, const float* const* p, void* const* out,
                        int32_t* const* flags, const float* const* u, const uint32_t* stream_ids, float sigma, const float* z,
                        const uint32_t* key, uint32_t noise_stream, uint32_t call, int B, int H, int W, int C, int Cpad, jg_stream_t s) {
  if ((dtype != JG_F16 && dtype != JG_BF16) || !src || !out || nd < 1 || nd > D_AUG_MAX || B < 1 || H < 1 || W < 1 || C < 1 || C > Cpad || Cpad % 8 || !(sigma == sigma))
    return JG_ERR_BAD_ARG;
  if (((uintptr_t)src & 15) || noise_stream > 0xffffu || Cpad / 4 > 0xffff) return JG_ERR_BAD_ARG;
  const bool noise = sigma != 0.f;
  if (noise && !z && !key) return JG_ERR_BAD_ARG;
  DAugTargets t = {};
  t.n = nd;
  bool any_flags = false;
  for (int d = 0; d < nd; ++d) {
    t.out[d] = out[d];
    t.alt[d] = alt ? alt[d] : nullptr;
    t.p[d] = p ? p[d] : nullptr;
    t.flags[d] = flags ? flags[d] : nullptr;
    t.u[d] = u ? u[d] : nullptr;
    t.stream[d] = stream_ids ? stream_ids[d] : 0u;
    if (!t.out[d] || ((uintptr_t)t.out[d] & 15) || t.out[d] == src) return JG_ERR_BAD_ARG;
    if (t.alt[d]) {
      if (!t.p[d] || !t.flags[d] || ((uintptr_t)t.alt[d] & 15) || t.alt[d] == t.out[d]) return JG_ERR_BAD_ARG;
      if (!t.u[d]) {      // drawn flags: a key, and a stream id of their own
        if (!key || t.stream[d] > 0xffffu || (noise && !z && t.stream[d] == noise_stream)) return JG_ERR_BAD_ARG;
        for (int e = 0; e < d; ++e)
          if (t.alt[e] && !t.u[e] && t.stream[e] == t.stream[d]) return JG_ERR_BAD_ARG;
      }
    }
    any_flags |= t.flags[d] != nullptr;
  }
  if (any_flags)
    hipLaunchKernelGGL(d_aug_flags_kernel, dim3((nd * B + 255) / 256), dim3(256), 0, (hipStream_t)s, t, key, call, B);
  const long HW = (long)H * W;
  const int G = Cpad / 8;
  JG_DISPATCH_DTYPE(dtype, hipLaunchKernelGGL((d_aug_kernel<T>), dim3(stream_grid((long)B * HW * G)), dim3(256), 0, (hipStream_t)s,
                                              (const T*)src, t, sigma, z, key, noise_stream, call, B, HW, C, G););
  JG_CHECK_LAUNCH();
  return JG_OK;
}

extern "C" int jg_apa_update(int dtype, const void* pred, int64_t n, int64_t stride, float* p, float* adjust, float* s_out, float target,
                             float num, float den, jg_stream_t s) {
  if (!pred || !p || !adjust || !s_out || n < 1 || stride < 1 || !(den > 0.f) || !(num >= 0.f) || !(target == target)) return JG_ERR_BAD_ARG;
  JG_DISPATCH_DTYPE(dtype, hipLaunchKernelGGL((apa_update_kernel<T>), dim3(1), dim3(1024), 0, (hipStream_t)s, (const T*)pred, (long)n,
                                              (long)stride, p, adjust, s_out, target, num, den););
  JG_CHECK_LAUNCH();
  return JG_OK;
}
