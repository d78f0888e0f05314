// nn.Dropout behind a normalise+activate pass (G_dropout of the CUT ResNet generator, D_dropout of the PatchGAN), inside that pass and its
// two backward passes:
//   jg_gn_apply_drop      y  = m * act(a x + b) / keep
//   jg_gn_bwd_reduce_drop red += (sum du, sum du x) per (image, channel),  du = (dy m / keep) act'(a x + b)
//   jg_gn_bwd_apply_drop  dx = du P + x Q + R                              (ab == NULL: dx = du with a = 1, b = 0)
// m[b, c, pixel] = (u[b, c, pixel] < keep).  The mask is never stored: the three kernels regenerate it from the same counter.
//
// Random numbers (philox.h, as in d_aug.hip): Philox4x32-10 on the two 32-bit words of a device tensor `key` with the counter
//   (pixel h * W + w,  sample b,  stream | (c / 4) << 16,  call)
// whose four words map to the uniforms of the channels 4 (c / 4) .. + 3.  `stream` names the Dropout module, `call` its invocation within the
// step.  A thread owns one 16-byte group of 8 channels of one pixel: two Philox calls per group.
//
// Behind a GroupNorm that runs in front of a nearest 2x upsample (the up-blocks of the efficient diffusion UNet) the mask lives at the HIGH resolution:
//   jg_gn_apply_drop_up2  y[b, i, j, c] = m[b, c, i, j] * act(a x[b, i / 2, j / 2, c] + b) / keep      x [B, H, W, C] -> y [B, 2H, 2W, C]
//   jg_drop_pool2_bwd     g[b, i, j, c] = sum over the 2 x 2 cell of dy * m / keep                     dy [B, 2H, 2W, C] -> g [B, H, W, C]
// with the counter of jg_gn_apply_drop on the materialised upsample (pixel = i * 2W + j).  A thread owns one 16-byte group of one LOW-resolution
// pixel: one load, one activation, four masks and four stores forward; four loads, four masks and one store backward.
#include "gn_map.h"
#include "philox.h"

namespace {

struct DropSrc {
  const float* u;        // injected uniforms fp32 [B, C, H, W], or null: drawn
  uint32_t k0, k1, stream, call;
  float keep, inv;
};

__device__ __forceinline__ DropSrc drop_src(const float* u, const uint32_t* key, uint32_t stream, uint32_t call, float keep) {
  DropSrc d;
  d.u = u;
  d.k0 = u ? 0u : key[0];
  d.k1 = u ? 0u : key[1];
  d.stream = stream;
  d.call = call;
  d.keep = keep;
  d.inv = 1.0f / keep;
  return d;
}

// f[q] = 1 / keep for a kept element, 0 for a dropped one: channels 8 co .. + 7 of pixel `pix` of sample b
__device__ __forceinline__ void drop_factors(const DropSrc& d, int b, long pix, int co, int C, long HW, float (&f)[8]) {
  if (d.u) {
#pragma unroll
    for (int q = 0; q < 8; ++q) f[q] = d.u[((long)b * C + co * 8 + q) * HW + pix] < d.keep ? d.inv : 0.f;
  } else {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const uint4 r = philox4x32_10(make_uint4((uint32_t)pix, (uint32_t)b, d.stream | ((uint32_t)(2 * co + h) << 16), d.call), d.k0, d.k1);
      f[4 * h] = uniform_open(r.x) < d.keep ? d.inv : 0.f;
      f[4 * h + 1] = uniform_open(r.y) < d.keep ? d.inv : 0.f;
      f[4 * h + 2] = uniform_open(r.z) < d.keep ? d.inv : 0.f;
      f[4 * h + 3] = uniform_open(r.w) < d.keep ? d.inv : 0.f;
    }
  }
}

__device__ __forceinline__ void load_ab(const float* __restrict__ ab, int b, int C, int co, float (&a)[8], float (&bb)[8]) {
  if (ab) {
    const float4* p = reinterpret_cast<const float4*>(ab + ((long)b * C + co * 8) * 2);      // 16 floats, 64-byte aligned
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float4 v = p[q];
      a[2 * q] = v.x;
      bb[2 * q] = v.y;
      a[2 * q + 1] = v.z;
      bb[2 * q + 1] = v.w;
    }
  } else {
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      a[q] = 1.f;
      bb[q] = 0.f;
    }
  }
}

// one thread per 16-byte group of 8 channels of one pixel, grid-stride; `G` = C / 8 groups per pixel
template <typename T, int ACT>
__global__ __launch_bounds__(256) void drop_apply_kernel(const T* __restrict__ x, long ldx, const float* __restrict__ ab, T* __restrict__ y, long ldy,
                                                         const float* __restrict__ u, const uint32_t* __restrict__ key, uint32_t stream, uint32_t call,
                                                         float keep, int B, long HW, int C, int G) {
  const DropSrc d = drop_src(u, key, stream, call, keep);
  const long total = (long)B * HW * G;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += gridDim.x * 256L) {
    const int co = (int)(i % G);
    const long bp = i / G;
    const int b = (int)(bp / HW);
    const long pix = bp - (long)b * HW;
    const uint4 v = *reinterpret_cast<const uint4*>(x + bp * ldx + co * 8);
    float a[8], bb[8], f[8], m[8];
    load_ab(ab, b, C, co, a, bb);
    drop_factors(d, b, pix, co, C, HW, m);
    unpack8<T>(v, f);
#pragma unroll
    for (int q = 0; q < 8; ++q) f[q] = m[q] != 0.f ? act_f<ACT>(a[q] * f[q] + bb[q]) * m[q] : 0.f;      // a dropped element is exactly 0
    *reinterpret_cast<uint4*>(y + bp * ldy + co * 8) = pack8<T>(f);
  }
}

// NORM: dx = du P + x Q + R; else (no normalisation in front of the activation) dx = du
template <typename T, int ACT, bool NORM>
__global__ __launch_bounds__(256) void drop_bwd_apply_kernel(const T* __restrict__ x, long ldx, const T* __restrict__ dy, long lddy,
                                                             const float* __restrict__ ab, const float* __restrict__ pqr, T* __restrict__ dx, long lddx,
                                                             const float* __restrict__ u, const uint32_t* __restrict__ key, uint32_t stream,
                                                             uint32_t call, float keep, int B, long HW, int C, int G) {
  const DropSrc d = drop_src(u, key, stream, call, keep);
  const long total = (long)B * HW * G;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += gridDim.x * 256L) {
    const int co = (int)(i % G);
    const long bp = i / G;
    const int b = (int)(bp / HW);
    const long pix = bp - (long)b * HW;
    const uint4 vx = *reinterpret_cast<const uint4*>(x + bp * ldx + co * 8);
    const uint4 vg = *reinterpret_cast<const uint4*>(dy + bp * lddy + co * 8);
    float a[8], bb[8], fx[8], fg[8], m[8];
    load_ab(NORM ? ab : nullptr, b, C, co, a, bb);
    drop_factors(d, b, pix, co, C, HW, m);
    unpack8<T>(vx, fx);
    unpack8<T>(vg, fg);
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      float du = m[q] != 0.f ? fg[q] * m[q] : 0.f;
      if (ACT != JG_ACT_NONE) du *= act_grad_f<ACT>(a[q] * fx[q] + bb[q]);
      if (NORM) {
        const float* c3 = pqr + ((long)b * C + co * 8 + q) * 3;
        du = du * c3[0] + fx[q] * c3[1] + c3[2];
      }
      fg[q] = du;
    }
    *reinterpret_cast<uint4*>(dx + bp * lddx + co * 8) = pack8<T>(fg);
  }
}

// gn_bwd_reduce_kernel of norm.hip with dy * m / keep in place of dy: the same map, the same LDS and global atomics
template <typename T, int ACT>
__global__ __launch_bounds__(256) void drop_bwd_reduce_kernel(const T* __restrict__ x, long ldx, const T* __restrict__ dy, long lddy,
                                                              const float* __restrict__ ab, float* __restrict__ red,
                                                              const float* __restrict__ u, const uint32_t* __restrict__ key, uint32_t stream,
                                                              uint32_t call, float keep, int HW, int C, int mult, int det) {
  extern __shared__ float s_acc[];  // [C][2] (+ [256][16] in the deterministic form, see gn_stats_kernel)
  const DropSrc d = drop_src(u, key, stream, call, keep);
  const Map mp = make_map_red(C, mult);
  const int tid = threadIdx.x, b = blockIdx.y;
  for (int i = tid; i < 2 * C; i += 256) s_acc[i] = 0.f;
  __syncthreads();
  float s1[8], s2[8];
#pragma unroll
  for (int q = 0; q < 8; ++q) s1[q] = s2[q] = 0.f;
  if (tid < mp.active) {
    const int co = tid % mp.noct, pl = tid / mp.noct;
    float a[8], bb[8];
    load_ab(ab, b, C, co, a, bb);
    const int pbeg = det ? 0 : blockIdx.x * mp.chunk;
    const int pend = det ? HW : min(HW, pbeg + mp.chunk);
    const long row0 = (long)b * HW;
    auto accumulate = [&](const uint4& vx, const uint4& vg, int p) {
      float fx[8], fg[8], m[8];
      drop_factors(d, b, p, co, C, HW, m);
      unpack8<T>(vx, fx);
      unpack8<T>(vg, fg);
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        float du = m[q] != 0.f ? fg[q] * m[q] : 0.f;
        if (ACT != JG_ACT_NONE) du *= act_grad_f<ACT>(a[q] * fx[q] + bb[q]);
        s1[q] += du;
        s2[q] += du * fx[q];
      }
    };
    // four pixels per trip, their eight 16-byte loads issued before the first use (see gn_bwd_reduce_kernel)
    int p = pbeg + pl;
    for (; p + 3 * mp.pl < pend; p += 4 * mp.pl) {
      uint4 vx[4], vg[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        vx[k] = *reinterpret_cast<const uint4*>(x + (row0 + p + k * mp.pl) * ldx + co * 8);
        vg[k] = *reinterpret_cast<const uint4*>(dy + (row0 + p + k * mp.pl) * lddy + co * 8);
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) accumulate(vx[k], vg[k], p + k * mp.pl);
    }
    for (; p < pend; p += mp.pl)
      accumulate(*reinterpret_cast<const uint4*>(x + (row0 + p) * ldx + co * 8), *reinterpret_cast<const uint4*>(dy + (row0 + p) * lddy + co * 8), p);
    const bool p2 = (mp.noct & (mp.noct - 1)) == 0 && mp.noct < 64;
    if (!det) {
      if (p2) {
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          for (int o = mp.noct; o < 64; o <<= 1) {
            s1[q] += __shfl_xor(s1[q], o);
            s2[q] += __shfl_xor(s2[q], o);
          }
        }
      }
      if (!p2 || (tid & 63) < mp.noct) {
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          atomicAdd(&s_acc[(co * 8 + q) * 2], s1[q]);
          atomicAdd(&s_acc[(co * 8 + q) * 2 + 1], s2[q]);
        }
      }
    }
  }
  if (det) ordered_octet_sum(s_acc, s1, s2, mp, C, tid < mp.active);
  __syncthreads();
  for (int i = tid; i < 2 * C; i += 256) atomicAdd(&red[(long)b * 2 * C + i], s_acc[i]);
}

// pixel (2 h + dy) * 2W + 2 w + dx of the high-resolution map, for dy, dx in {0, 1}: k = 2 dy + dx
__device__ __forceinline__ long up2_pixel(int h, int w, int W, int k) { return (long)(2 * h + (k >> 1)) * (2 * W) + 2 * w + (k & 1); }

template <typename T, int ACT>
__global__ __launch_bounds__(256) void drop_apply_up2_kernel(const T* __restrict__ x, long ldx, const float* __restrict__ ab, T* __restrict__ y, long ldy,
                                                             const float* __restrict__ u, const uint32_t* __restrict__ key, uint32_t stream,
                                                             uint32_t call, float keep, int B, int H, int W, int C, int G) {
  const DropSrc d = drop_src(u, key, stream, call, keep);
  const long HW = (long)H * W, HW4 = 4 * HW;
  const long total = (long)B * HW * G;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += gridDim.x * 256L) {
    const int co = (int)(i % G);
    const long bp = i / G;
    const int b = (int)(bp / HW);
    const int lp = (int)(bp - (long)b * HW);
    const int h = lp / W, w = lp - h * W;
    const uint4 v = *reinterpret_cast<const uint4*>(x + bp * ldx + co * 8);
    float a[8], bb[8], f[8], r[8], m[8];
    load_ab(ab, b, C, co, a, bb);
    unpack8<T>(v, f);
#pragma unroll
    for (int q = 0; q < 8; ++q) f[q] = act_f<ACT>(a[q] * f[q] + bb[q]);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const long pix = up2_pixel(h, w, W, k);
      drop_factors(d, b, pix, co, C, HW4, m);
#pragma unroll
      for (int q = 0; q < 8; ++q) r[q] = m[q] != 0.f ? f[q] * m[q] : 0.f;      // a dropped element is exactly 0
      *reinterpret_cast<uint4*>(y + ((long)b * HW4 + pix) * ldy + co * 8) = pack8<T>(r);
    }
  }
}

template <typename T>
__global__ __launch_bounds__(256) void drop_pool2_bwd_kernel(const T* __restrict__ dy, long lddy, T* __restrict__ g, long ldg, const float* __restrict__ u,
                                                             const uint32_t* __restrict__ key, uint32_t stream, uint32_t call, float keep, int B, int H,
                                                             int W, int C, int G) {
  const DropSrc d = drop_src(u, key, stream, call, keep);
  const long HW = (long)H * W, HW4 = 4 * HW;
  const long total = (long)B * HW * G;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += gridDim.x * 256L) {
    const int co = (int)(i % G);
    const long bp = i / G;
    const int b = (int)(bp / HW);
    const int lp = (int)(bp - (long)b * HW);
    const int h = lp / W, w = lp - h * W;
    uint4 v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = *reinterpret_cast<const uint4*>(dy + ((long)b * HW4 + up2_pixel(h, w, W, k)) * lddy + co * 8);
    float acc[8], f[8], m[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) acc[q] = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      drop_factors(d, b, up2_pixel(h, w, W, k), co, C, HW4, m);
      unpack8<T>(v[k], f);
#pragma unroll
      for (int q = 0; q < 8; ++q) acc[q] += m[q] != 0.f ? f[q] * m[q] : 0.f;
    }
    *reinterpret_cast<uint4*>(g + bp * ldg + co * 8) = pack8<T>(acc);
  }
}

inline bool bad_drop(float keep, const float* u, const uint32_t* key, uint32_t stream, int C) {
  return !(keep > 0.f && keep <= 1.f) || (!u && !key) || stream > 0xffffu || C / 4 > 0xffff;
}
inline bool bad_ld(const void* p, int64_t ld, int C) { return !p || ((uintptr_t)p & 15) || ld < C || (ld % 8); }
inline bool bad_tab(const float* ab, const float* pqr) { return ((uintptr_t)ab & 15) || ((uintptr_t)pqr & 3); }      // ab is read as float4 rows

}  // namespace

extern "C" int jg_dropout_grid_cap(void) { return STREAM_GRID_MAX_BLOCKS * 256; }

extern "C" int jg_gn_apply_drop(int dtype, const void* x, int64_t ldx, const float* ab, void* y, int64_t ldy, int B, int H, int W, int C, int act,
                                float keep, const float* u, const uint32_t* key, uint32_t stream, uint32_t call, jg_stream_t s) {
  if (H < 1 || W < 1 || (long)H * W > 0x7fffffffL || bad_shape(B, H * W, C) || bad_ld(x, ldx, C) || bad_ld(y, ldy, C) || bad_tab(ab, nullptr) ||
      bad_drop(keep, u, key, stream, C))
    return JG_ERR_BAD_ARG;
  if (act != JG_ACT_NONE && act != JG_ACT_RELU && act != JG_ACT_LRELU && act != JG_ACT_SILU) return JG_ERR_BAD_ARG;
  const long HW = (long)H * W;
  const int G = C / 8;
  JG_DISPATCH_DTYPE(dtype, JG_DISPATCH_ACT(act, hipLaunchKernelGGL((drop_apply_kernel<T, ACT>), dim3(stream_grid((long)B * HW * G)), dim3(256), 0,
                                                            (hipStream_t)s, (const T*)x, (long)ldx, ab, (T*)y, (long)ldy, u, key, stream, call, keep, B,
                                                            HW, C, G);););
  JG_CHECK_LAUNCH();
  return JG_OK;
}

extern "C" int jg_gn_bwd_reduce_drop(int dtype, const void* x, int64_t ldx, const void* dy, int64_t lddy, const float* ab, float* red, int B, int H,
                                     int W, int C, int act, float keep, const float* u, const uint32_t* key, uint32_t stream, uint32_t call,
                                     jg_stream_t s) {
  if (H < 1 || W < 1 || (long)H * W > 0x7fffffffL || bad_shape(B, H * W, C) || bad_ld(x, ldx, C) || bad_ld(dy, lddy, C) || !ab || !red || bad_tab(ab, nullptr) ||
      bad_drop(keep, u, key, stream, C))
    return JG_ERR_BAD_ARG;
  if (act != JG_ACT_NONE && act != JG_ACT_RELU && act != JG_ACT_LRELU && act != JG_ACT_SILU) return JG_ERR_BAD_ARG;
  const int HW = H * W;
  const int mult = red_mult(B, HW, C);
  const Map mp = make_map_red(C, mult);
  const int det = jg_tune(JG_TUNE_DETERMINISTIC) != 0;
  dim3 grid(det ? 1 : (HW + mp.chunk - 1) / mp.chunk, B);
  const size_t shm = (2 * C + (det ? 4096 : 0)) * sizeof(float);
  JG_DISPATCH_DTYPE(dtype, JG_DISPATCH_ACT(act, hipLaunchKernelGGL((drop_bwd_reduce_kernel<T, ACT>), grid, dim3(256), shm, (hipStream_t)s, (const T*)x,
                                                            (long)ldx, (const T*)dy, (long)lddy, ab, red, u, key, stream, call, keep, HW, C, mult,
                                                            det);););
  JG_CHECK_LAUNCH();
  return JG_OK;
}

extern "C" int jg_gn_bwd_apply_drop(int dtype, const void* x, int64_t ldx, const void* dy, int64_t lddy, const float* ab, const float* pqr, void* dx,
                                    int64_t lddx, int B, int H, int W, int C, int act, float keep, const float* u, const uint32_t* key,
                                    uint32_t stream, uint32_t call, jg_stream_t s) {
  if (H < 1 || W < 1 || (long)H * W > 0x7fffffffL || bad_shape(B, H * W, C) || bad_ld(x, ldx, C) || bad_ld(dy, lddy, C) || bad_ld(dx, lddx, C) ||
      (ab != nullptr) != (pqr != nullptr) || bad_tab(ab, pqr) || bad_drop(keep, u, key, stream, C))
    return JG_ERR_BAD_ARG;
  if (act != JG_ACT_NONE && act != JG_ACT_RELU && act != JG_ACT_LRELU && act != JG_ACT_SILU) return JG_ERR_BAD_ARG;
  const long HW = (long)H * W;
  const int G = C / 8;
  const dim3 grid(stream_grid((long)B * HW * G));
  if (ab) {
    JG_DISPATCH_DTYPE(dtype, JG_DISPATCH_ACT(act, hipLaunchKernelGGL((drop_bwd_apply_kernel<T, ACT, true>), grid, dim3(256), 0, (hipStream_t)s,
                                                              (const T*)x, (long)ldx, (const T*)dy, (long)lddy, ab, pqr, (T*)dx, (long)lddx, u, key,
                                                              stream, call, keep, B, HW, C, G);););
  } else {
    JG_DISPATCH_DTYPE(dtype, JG_DISPATCH_ACT(act, hipLaunchKernelGGL((drop_bwd_apply_kernel<T, ACT, false>), grid, dim3(256), 0, (hipStream_t)s,
                                                              (const T*)x, (long)ldx, (const T*)dy, (long)lddy, ab, pqr, (T*)dx, (long)lddx, u, key,
                                                              stream, call, keep, B, HW, C, G);););
  }
  JG_CHECK_LAUNCH();
  return JG_OK;
}

// the low-resolution side is [B, H, W, C], the high-resolution side [B, 2H, 2W, C]: its pixel index 4 H W - 1 has to fit the 32-bit counter word
inline bool bad_up2(int B, int H, int W, int C) { return H < 1 || W < 1 || (long)H * W > 0x7fffffffL / 4 || bad_shape(B, H * W, C); }

extern "C" int jg_gn_apply_drop_up2(int dtype, const void* x, int64_t ldx, const float* ab, void* y, int64_t ldy, int B, int H, int W, int C, int act,
                                    float keep, const float* u, const uint32_t* key, uint32_t stream, uint32_t call, jg_stream_t s) {
  if (bad_up2(B, H, W, C) || bad_ld(x, ldx, C) || bad_ld(y, ldy, C) || bad_tab(ab, nullptr) || bad_drop(keep, u, key, stream, C)) return JG_ERR_BAD_ARG;
  if (act != JG_ACT_NONE && act != JG_ACT_RELU && act != JG_ACT_LRELU && act != JG_ACT_SILU) return JG_ERR_BAD_ARG;
  const int G = C / 8;
  JG_DISPATCH_DTYPE(dtype, JG_DISPATCH_ACT(act, hipLaunchKernelGGL((drop_apply_up2_kernel<T, ACT>), dim3(stream_grid((long)B * H * W * G)), dim3(256), 0,
                                                            (hipStream_t)s, (const T*)x, (long)ldx, ab, (T*)y, (long)ldy, u, key, stream, call, keep, B,
                                                            H, W, C, G);););
  JG_CHECK_LAUNCH();
  return JG_OK;
}

extern "C" int jg_drop_pool2_bwd(int dtype, const void* dy, int64_t lddy, void* g, int64_t ldg, int B, int H, int W, int C, float keep, const float* u,
                                 const uint32_t* key, uint32_t stream, uint32_t call, jg_stream_t s) {
  if (bad_up2(B, H, W, C) || bad_ld(dy, lddy, C) || bad_ld(g, ldg, C) || bad_drop(keep, u, key, stream, C)) return JG_ERR_BAD_ARG;
  const int G = C / 8;
  JG_DISPATCH_DTYPE(dtype, hipLaunchKernelGGL((drop_pool2_bwd_kernel<T>), dim3(stream_grid((long)B * H * W * G)), dim3(256), 0, (hipStream_t)s,
                                              (const T*)dy, (long)lddy, (T*)g, (long)ldg, u, key, stream, call, keep, B, H, W, C, G););
  JG_CHECK_LAUNCH();
  return JG_OK;
}
