// data_online_context_pixels of the GAN models: the generator works on the centre crop, the discriminators see the crop inside its surroundings.
//   jg_context_split  ctx[b,h,w,c] = x[b,c,h,w] (NCHW fp32 -> NHWC 16-bit, as jg_nchw_f32_to_nhwc rounds) and crop = ctx[:, c:-c, c:-c],
//                     both written from ONE read of x
//   jg_context_frame  out[b,h,w,:] = (h, w) inside the window ? inner[b,h-c,w-c,:] : ctx[b,h,w,:]      (the reference's pad + mask * ctx, as a select)
//                     out_noisy    = out + sigma * z over the whole framed image (dataaug_D_noise on fake_B_with_context), optional
// Both follow d_aug.hip: one thread per 16-byte group of 8 channels of one pixel of the FRAMED grid, grid-stride; the padding channels of every
// output are zero; no scalar that changes between steps enters a launch from the host (the Philox key is read from device memory).
// The noise is jg_d_aug's, bit for bit: counter (pixel h * W + w of the framed grid, sample b, noise_stream | (group of 4 channels) << 16, call),
// Box-Muller in fp32, fmaf in fp32, one rounding -- out_noisy equals jg_d_aug(out) with the same (sigma, key, noise_stream, call).
#include "philox.h"

namespace {

// 0xffff for a valid channel, 0 for a padding channel, per 32-bit word of a 16-byte group that starts at channel c0
__device__ __forceinline__ uint4 channel_mask(int c0, int C) {
  uint32_t m[4];
#pragma unroll
  for (int w = 0; w < 4; ++w) m[w] = (c0 + 2 * w < C ? 0xffffu : 0u) | (c0 + 2 * w + 1 < C ? 0xffff0000u : 0u);
  return make_uint4(m[0], m[1], m[2], m[3]);
}

// H, W: the framed size; the window is rows / columns [c, H - c) x [c, W - c)
template <typename T>
__global__ __launch_bounds__(256) void context_split_kernel(const float* __restrict__ x, T* __restrict__ ctx, T* __restrict__ crop, int B, int C, int H,
                                                            int W, int c, int G) {
  const long HW = (long)H * W;
  const long total = (long)B * HW * G;
  const int Hi = H - 2 * c, Wi = W - 2 * c;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += gridDim.x * 256L) {
    const int g8 = (int)(i % G);
    const long bp = i / G;
    const int b = (int)(bp / HW);
    const long pix = bp - (long)b * HW;
    const int h = (int)(pix / W), w = (int)(pix - (long)h * W);
    const int c0 = g8 * 8;
    float f[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) f[k] = c0 + k < C ? x[((long)b * C + c0 + k) * HW + pix] : 0.f;
    const uint4 v = pack8<T>(f);
    reinterpret_cast<uint4*>(ctx)[i] = v;
    if (h >= c && h < H - c && w >= c && w < W - c)
      reinterpret_cast<uint4*>(crop)[(((long)b * Hi + (h - c)) * Wi + (w - c)) * G + g8] = v;
  }
}

template <typename T>
__global__ __launch_bounds__(256) void context_frame_kernel(const T* __restrict__ inner, const T* __restrict__ ctx, T* __restrict__ out,
                                                            T* __restrict__ out_noisy, float sigma, const float* __restrict__ z,
                                                            const uint32_t* __restrict__ key, uint32_t noise_stream, uint32_t call, int B, int H, int W,
                                                            int c, int C, int G) {
  const bool noise = out_noisy && sigma != 0.f;
  const bool draw = noise && !z;
  const uint32_t k0 = draw ? key[0] : 0u, k1 = draw ? key[1] : 0u;
  const long HW = (long)H * W;
  const long total = (long)B * HW * G;
  const int Hi = H - 2 * c, Wi = W - 2 * c;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += gridDim.x * 256L) {
    const int g8 = (int)(i % G);
    const long bp = i / G;
    const int b = (int)(bp / HW);
    const long pix = bp - (long)b * HW;
    const int h = (int)(pix / W), w = (int)(pix - (long)h * W);
    const int c0 = g8 * 8;
    const bool in = h >= c && h < H - c && w >= c && w < W - c;
    uint4 v = in ? reinterpret_cast<const uint4*>(inner)[(((long)b * Hi + (h - c)) * Wi + (w - c)) * G + g8] : reinterpret_cast<const uint4*>(ctx)[i];
    const uint4 m = channel_mask(c0, C);
    v = make_uint4(v.x & m.x, v.y & m.y, v.z & m.z, v.w & m.w);
    reinterpret_cast<uint4*>(out)[i] = v;
    if (!out_noisy) continue;
    if (noise && c0 < C) {
      float f[8], nz[8];
      unpack8<T>(v, f);
      if (z) {
#pragma unroll
        for (int k = 0; k < 8; ++k) nz[k] = c0 + k < C ? z[((long)b * C + c0 + k) * HW + pix] : 0.f;
      } else {
#pragma unroll
        for (int q = 0; q < 2; ++q) {        // the two groups of 4 channels of this thread, as in d_aug_kernel
          nz[4 * q] = nz[4 * q + 1] = nz[4 * q + 2] = nz[4 * q + 3] = 0.f;
          if (c0 + 4 * q < C) {
            const uint4 r = philox4x32_10(make_uint4((uint32_t)pix, (uint32_t)b, noise_stream | ((uint32_t)(2 * g8 + q) << 16), call), k0, k1);
            box_muller(r.x, r.y, nz[4 * q], nz[4 * q + 1]);
            if (c0 + 4 * q + 2 < C) box_muller(r.z, r.w, nz[4 * q + 2], nz[4 * q + 3]);
          }
        }
      }
#pragma unroll
      for (int k = 0; k < 8; ++k) f[k] = c0 + k < C ? fmaf(sigma, nz[k], f[k]) : 0.f;      // fp32, rounded once by pack8
      v = pack8<T>(f);
      v = make_uint4(v.x & m.x, v.y & m.y, v.z & m.z, v.w & m.w);
    }
    reinterpret_cast<uint4*>(out_noisy)[i] = v;
  }
}

inline bool bad_geometry(int B, int C, int H, int W, int c, int Cpad) {
  return B < 1 || C < 1 || C > Cpad || Cpad % 8 || c < 1 || H < 1 || W < 1 || H - 2 * (long)c < 1 || W - 2 * (long)c < 1;
}

}  // namespace

extern "C" int jg_context_split(int dtype, const float* x, void* ctx, void* crop, int B, int C, int H, int W, int c, int Cpad, jg_stream_t s) {
  if (dtype != JG_F16 && dtype != JG_BF16) return JG_ERR_UNSUPPORTED;
  if (!x || !ctx || !crop || ctx == crop || bad_geometry(B, C, H, W, c, Cpad)) return JG_ERR_BAD_ARG;
  if (((uintptr_t)ctx & 15) || ((uintptr_t)crop & 15) || ((uintptr_t)x & 3)) return JG_ERR_BAD_ARG;
  const int G = Cpad / 8;
  JG_DISPATCH_DTYPE(dtype, hipLaunchKernelGGL((context_split_kernel<T>), dim3(stream_grid((long)B * H * W * G)), dim3(256), 0, (hipStream_t)s, x, (T*)ctx,
                                              (T*)crop, B, C, H, W, c, G););
  JG_CHECK_LAUNCH();
  return JG_OK;
}

extern "C" int jg_context_frame(int dtype, const void* inner, const void* ctx, void* out, void* out_noisy, float sigma, const float* z,
                                const uint32_t* key, uint32_t noise_stream, uint32_t call, int B, int H, int W, int c, int C, int Cpad, jg_stream_t s) {
  if (dtype != JG_F16 && dtype != JG_BF16) return JG_ERR_UNSUPPORTED;
  if (!inner || !ctx || !out || bad_geometry(B, C, H, W, c, Cpad) || !(sigma == sigma)) return JG_ERR_BAD_ARG;
  if (((uintptr_t)inner & 15) || ((uintptr_t)ctx & 15) || ((uintptr_t)out & 15) || ((uintptr_t)out_noisy & 15)) return JG_ERR_BAD_ARG;
  if (out == inner || out == ctx || out_noisy == inner || out_noisy == ctx || out_noisy == out) return JG_ERR_BAD_ARG;
  if (noise_stream > 0xffffu || Cpad / 4 > 0xffff) return JG_ERR_BAD_ARG;
  if (sigma != 0.f && (!out_noisy || (!z && !key))) return JG_ERR_BAD_ARG;      // noise needs a destination and a source of z
  const int G = Cpad / 8;
  JG_DISPATCH_DTYPE(dtype, hipLaunchKernelGGL((context_frame_kernel<T>), dim3(stream_grid((long)B * H * W * G)), dim3(256), 0, (hipStream_t)s,
                                              (const T*)inner, (const T*)ctx, (T*)out, (T*)out_noisy, sigma, z, key, noise_stream, call, B, H, W, c, C,
                                              G););
  JG_CHECK_LAUNCH();
  return JG_OK;
}
