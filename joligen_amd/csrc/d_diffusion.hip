// dataaug_D_diffusion: the Diffusion-GAN noising of the projected discriminator's four backbone feature maps
// (models/modules/projected_d/diffusion.py, projector.py:531-556) and the adaptive update of its strength (loss.py:315-331):
//   jg_d_diffusion        out_l[b,h,w,c] = a[t_l[b,c]] * x_l[b,h,w,c] + (noise_std * b[t_l[b,c]]) * z_l[b,c,h,w]   up to 4 levels l, one launch
//   jg_d_diffusion_bwd    dx_l[b,h,w,c]  = a[t_l[b,c]] * dy_l[b,h,w,c]                                            up to 4 levels l, one launch
//   jg_d_diffusion_update p <- clip(p + sign(loss - 0.9) * num / den, 0, 1), then T, n, the tables a / b and t_epl rebuilt from p; one block
// Everything that changes between steps (p, T, n, a, b, t_epl, the Philox key, the loss) is read from DEVICE memory.
//
// Random numbers (philox.h), counters that no two draws share:
//   z : (pixel h * W + w,  sample b,  level l | (group of 4 channels) << 16,  call)      4 words = the normals of 4 channels of one pixel
//   t : (group of 4 channels,  sample b,  8 + l,  call)                                  word j >> 26 = the index into t_epl of channel 4 g + j
//   u : (entry i of t_epl,  0,  16,  call)                                               word 0 -> (0, 1): the update's inverse-CDF draw
#include "philox.h"

namespace {

constexpr int DD_MAX = JG_D_DIFFUSION_MAX;
constexpr int DD_TAB = JG_D_DIFFUSION_TABLE;      // 501 entries: t = 0 .. 500
constexpr int DD_EPL = JG_D_DIFFUSION_EPL;        // 64 entries of t_epl
constexpr uint32_t DD_T_STREAM = 8u, DD_U_STREAM = 16u;

struct DDLevels {
  const void* x[DD_MAX];         // forward: the feature map; backward: dy
  void* out[DD_MAX];             // forward: the noised copy; backward: dx
  int32_t* t_out[DD_MAX];        // forward: the t used, int32 [B, C]
  const int32_t* t_in[DD_MAX];   // forward: injected t or NULL; backward: the saved t
  const float* z[DD_MAX];        // forward: injected noise fp32 [B, C, H, W] or NULL
  long end[DD_MAX];              // prefix sums of B * HW * (C / 8): the 16-byte groups of levels 0 .. l
  int HW[DD_MAX], C[DD_MAX];
  int n;
};

// one thread per 16-byte group of 8 channels of one pixel, all levels in one index space
template <typename T>
__global__ __launch_bounds__(256) void d_diffusion_kernel(DDLevels lv, const float* __restrict__ ta, const float* __restrict__ tb,
                                                          const int32_t* __restrict__ t_epl, float noise_std,
                                                          const uint32_t* __restrict__ key, uint32_t call) {
  const uint32_t k0 = key ? key[0] : 0u, k1 = key ? key[1] : 0u;
  const long total = lv.end[lv.n - 1];
  for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += gridDim.x * 256L) {
    int l = 0;
#pragma unroll
    for (int q = 1; q < DD_MAX; ++q) l += (q < lv.n && i >= lv.end[q - 1]) ? 1 : 0;
    const long j = i - (l ? lv.end[l - 1] : 0L);
    const int C = lv.C[l], G = C >> 3, HW = lv.HW[l];
    const int g8 = (int)(j % G);
    const long bp = j / G;
    const int b = (int)(bp / HW);
    const int pix = (int)(bp - (long)b * HW);
    const int c0 = g8 * 8;
    int t[8];
    if (lv.t_in[l]) {
      const int4* tp = reinterpret_cast<const int4*>(lv.t_in[l] + (long)b * C + c0);      // C % 8 == 0: 32-byte aligned
      const int4 t0 = tp[0], t1 = tp[1];
      t[0] = t0.x, t[1] = t0.y, t[2] = t0.z, t[3] = t0.w, t[4] = t1.x, t[5] = t1.y, t[6] = t1.z, t[7] = t1.w;
    } else {
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const uint4 r = philox4x32_10(make_uint4((uint32_t)(2 * g8 + q), (uint32_t)b, DD_T_STREAM + (uint32_t)l, call), k0, k1);
        t[4 * q] = t_epl[r.x >> 26], t[4 * q + 1] = t_epl[r.y >> 26], t[4 * q + 2] = t_epl[r.z >> 26], t[4 * q + 3] = t_epl[r.w >> 26];
      }
    }
    float a[8], sb[8];
    bool noisy = false;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      t[c] = t[c] < 0 ? 0 : t[c] >= DD_TAB ? DD_TAB - 1 : t[c];      // an injected t cannot index outside the tables
      a[c] = ta[t[c]];
      sb[c] = noise_std * tb[t[c]];
      noisy |= sb[c] != 0.f;
    }
    if (pix == 0) {
      int4* tp = reinterpret_cast<int4*>(lv.t_out[l] + (long)b * C + c0);
      tp[0] = make_int4(t[0], t[1], t[2], t[3]);
      tp[1] = make_int4(t[4], t[5], t[6], t[7]);
    }
    const uint4 xv = reinterpret_cast<const uint4*>(lv.x[l])[j];
    float f[8], nz[8];
    unpack8<T>(xv, f);
    if (noisy) {
      if (lv.z[l]) {
        const float* zp = lv.z[l] + ((long)b * C + c0) * HW + pix;
#pragma unroll
        for (int c = 0; c < 8; ++c) nz[c] = zp[(long)c * HW];
      } else {
#pragma unroll
        for (int q = 0; q < 2; ++q) {
          const uint4 r = philox4x32_10(make_uint4((uint32_t)pix, (uint32_t)b, (uint32_t)l | ((uint32_t)(2 * g8 + q) << 16), call), k0, k1);
          box_muller(r.x, r.y, nz[4 * q], nz[4 * q + 1]);
          box_muller(r.z, r.w, nz[4 * q + 2], nz[4 * q + 3]);
        }
      }
    }
    // fp32, rounded once by pack8.  A channel without noise (b[t] == 0, the whole map at p = 0) is a[t] * x alone: with a[0] == 1 the
    // input passes bit for bit, the sign of a zero included
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      const float ax = a[c] * f[c];
      f[c] = sb[c] != 0.f ? fmaf(sb[c], nz[c], ax) : ax;
    }
    reinterpret_cast<uint4*>(lv.out[l])[j] = pack8<T>(f);
  }
}

template <typename T>
__global__ __launch_bounds__(256) void d_diffusion_bwd_kernel(DDLevels lv, const float* __restrict__ ta) {
  const long total = lv.end[lv.n - 1];
  for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += gridDim.x * 256L) {
    int l = 0;
#pragma unroll
    for (int q = 1; q < DD_MAX; ++q) l += (q < lv.n && i >= lv.end[q - 1]) ? 1 : 0;
    const long j = i - (l ? lv.end[l - 1] : 0L);
    const int C = lv.C[l], G = C >> 3, HW = lv.HW[l];
    const int g8 = (int)(j % G);
    const int b = (int)(j / G / HW);
    const int4* tp = reinterpret_cast<const int4*>(lv.t_in[l] + (long)b * C + g8 * 8);
    const int4 t0 = tp[0], t1 = tp[1];
    const int t[8] = {t0.x, t0.y, t0.z, t0.w, t1.x, t1.y, t1.z, t1.w};
    float f[8];
    unpack8<T>(reinterpret_cast<const uint4*>(lv.x[l])[j], f);
#pragma unroll
    for (int c = 0; c < 8; ++c) f[c] *= ta[t[c] < 0 ? 0 : t[c] >= DD_TAB ? DD_TAB - 1 : t[c]];
    reinterpret_cast<uint4*>(lv.out[l])[j] = pack8<T>(f);
  }
}

// one block of 512 threads: thread 0 moves p and derives T and n; thread i < T forms alpha_i; thread 0 takes the cumulative product in
// fp64; thread i <= 500 writes a[i], b[i]; thread i < 64 writes t_epl[i]
__global__ __launch_bounds__(512) void d_diffusion_update_kernel(float* __restrict__ p, int32_t* __restrict__ Tn, float* __restrict__ ta,
                                                                 float* __restrict__ tb, int32_t* __restrict__ t_epl,
                                                                 const float* __restrict__ loss, float num, float den,
                                                                 const float* __restrict__ u, const uint32_t* __restrict__ key, uint32_t call) {
  __shared__ double cp[DD_TAB];
  __shared__ float alpha[DD_TAB - 1];
  __shared__ int sT, sn;
  const int i = threadIdx.x;
  if (i == 0) {
    // the reference's order, every step in fp32: adjust = sign(loss - 0.9) * (B * every) / (100 * 1000);  p = clip(p + adjust, 0, 1).
    // A loss that is not a number leaves p where it is
    const float d = *loss - 0.9f;
    const float adj = d > 0.f ? 1.f : d < 0.f ? -1.f : 0.f;
    float pn = *p + __fdiv_rn(adj * num, den);
    pn = pn < 0.f ? 0.f : pn > 1.f ? 1.f : pn;
    *p = pn;
    int T = (int)(JG_D_DIFFUSION_T_MIN + rintf(__fmul_rn(pn, (float)(JG_D_DIFFUSION_T_MAX - JG_D_DIFFUSION_T_MIN))));      // round half to even
    T = T < JG_D_DIFFUSION_T_MIN ? JG_D_DIFFUSION_T_MIN : T > JG_D_DIFFUSION_T_MAX ? JG_D_DIFFUSION_T_MAX : T;
    int n = (int)rintf(__fmul_rn(pn, (float)DD_EPL));
    n = n > 48 ? 48 : n;
    Tn[0] = sT = T;
    Tn[1] = sn = n;
  }
  __syncthreads();
  const int T = sT, n = sn;
  if (i < T) {
    // numpy.linspace(1e-4, 1e-2, T) in fp64: i * step + start in two roundings (no contraction), the last entry the end point itself;
    // betas rounded to fp32, alphas = 1 - betas in fp32
    const double step = __ddiv_rn(1e-2 - 1e-4, (double)(T - 1));
    const double beta = i == T - 1 ? 1e-2 : __dadd_rn(__dmul_rn((double)i, step), 1e-4);
    alpha[i] = 1.0f - (float)beta;
  }
  __syncthreads();
  if (i == 0) {
    double c = 1.0;
    cp[0] = c;
    for (int k = 0; k < T; ++k) {
      c = __dmul_rn(c, (double)alpha[k]);
      cp[k + 1] = c;
    }
  }
  __syncthreads();
  if (i < DD_TAB) {
    ta[i] = i <= T ? (float)sqrt(cp[i]) : 0.f;
    tb[i] = i <= T ? (float)sqrt(1.0 - cp[i]) : 0.f;
  }
  if (i < DD_EPL) {
    int v = 0;
    if (i < n) {
      // inverse CDF of prob_t = arange(T) / sum(arange(T)) over the values 1 .. T: value k + 1 for the smallest k >= 1 with
      // k (k + 1) >= u T (T - 1).  u has at most 24 significant bits and T (T - 1) < 2^18: every product below is exact in fp64
      const float uf = u ? u[i] : uniform_open(philox4x32_10(make_uint4((uint32_t)i, 0u, DD_U_STREAM, call), key[0], key[1]).x);
      const double w = (double)uf * (double)(T * (T - 1));
      int k = (int)ceil((sqrt(1.0 + 4.0 * w) - 1.0) * 0.5);
      k = k < 1 ? 1 : k > T - 1 ? T - 1 : k;
      while (k < T - 1 && (double)k * (double)(k + 1) < w) ++k;
      while (k > 1 && (double)(k - 1) * (double)k >= w) --k;
      v = k + 1;
    }
    t_epl[i] = v;
  }
}

}  // namespace

extern "C" int jg_d_diffusion_grid_cap(void) { return STREAM_GRID_MAX_BLOCKS * 256; }

static int dd_levels(DDLevels& lv, int nl, const void* const* x, void* const* out, const int32_t* const* t, const int* H, const int* W,
                     const int* C, int B) {
  if (nl < 1 || nl > DD_MAX || !x || !out || !t || !H || !W || !C || B < 1) return JG_ERR_BAD_ARG;
  lv = {};
  lv.n = nl;
  long end = 0;
  for (int l = 0; l < nl; ++l) {
    if (!x[l] || !out[l] || !t[l] || x[l] == out[l] || ((uintptr_t)x[l] & 15) || ((uintptr_t)out[l] & 15) || ((uintptr_t)t[l] & 15))
      return JG_ERR_BAD_ARG;
    if (H[l] < 1 || W[l] < 1 || C[l] < 8 || C[l] % 8 || C[l] / 4 > 0xffff || (long)H[l] * W[l] > 0x7fffffffL) return JG_ERR_BAD_ARG;
    lv.x[l] = x[l];
    lv.out[l] = out[l];
    lv.HW[l] = H[l] * W[l];
    lv.C[l] = C[l];
    end += (long)B * lv.HW[l] * (C[l] / 8);
    lv.end[l] = end;
  }
  return JG_OK;
}

extern "C" int jg_d_diffusion(int dtype, int nl, const void* const* x, void* const* out, int32_t* const* t_out, const int32_t* const* t_in,
                              const float* const* z, const int* H, const int* W, const int* C, int B, const float* a, const float* b,
                              const int32_t* t_epl, float noise_std, const uint32_t* key, uint32_t call, jg_stream_t s) {
  if ((dtype != JG_F16 && dtype != JG_BF16) || !a || !b || !t_epl || !(noise_std == noise_std)) return JG_ERR_BAD_ARG;
  DDLevels lv;
  const int rc = dd_levels(lv, nl, x, out, t_out, H, W, C, B);
  if (rc != JG_OK) return rc;
  for (int l = 0; l < nl; ++l) {
    lv.t_out[l] = t_out[l];
    lv.t_in[l] = t_in ? t_in[l] : nullptr;
    lv.z[l] = z ? z[l] : nullptr;
    if ((lv.t_in[l] && (((uintptr_t)lv.t_in[l] & 15) || lv.t_in[l] == lv.t_out[l])) || ((!lv.t_in[l] || !lv.z[l]) && !key)) return JG_ERR_BAD_ARG;
  }
  JG_DISPATCH_DTYPE(dtype, hipLaunchKernelGGL((d_diffusion_kernel<T>), dim3(stream_grid(lv.end[nl - 1])), dim3(256), 0, (hipStream_t)s, lv, a,
                                              b, t_epl, noise_std, key, call););
  JG_CHECK_LAUNCH();
  return JG_OK;
}

extern "C" int jg_d_diffusion_bwd(int dtype, int nl, const void* const* dy, void* const* dx, const int32_t* const* t, const int* H,
                                  const int* W, const int* C, int B, const float* a, jg_stream_t s) {
  if ((dtype != JG_F16 && dtype != JG_BF16) || !a) return JG_ERR_BAD_ARG;
  DDLevels lv;
  const int rc = dd_levels(lv, nl, dy, dx, t, H, W, C, B);
  if (rc != JG_OK) return rc;
  for (int l = 0; l < nl; ++l) lv.t_in[l] = t[l];
  JG_DISPATCH_DTYPE(dtype, hipLaunchKernelGGL((d_diffusion_bwd_kernel<T>), dim3(stream_grid(lv.end[nl - 1])), dim3(256), 0, (hipStream_t)s, lv,
                                              a););
  JG_CHECK_LAUNCH();
  return JG_OK;
}

extern "C" int jg_d_diffusion_update(float* p, int32_t* Tn, float* a, float* b, int32_t* t_epl, const float* loss, float num, float den,
                                     const float* u, const uint32_t* key, uint32_t call, jg_stream_t s) {
  if (!p || !Tn || !a || !b || !t_epl || !loss || !(num >= 0.f) || !(den > 0.f) || (!u && !key)) return JG_ERR_BAD_ARG;
  hipLaunchKernelGGL(d_diffusion_update_kernel, dim3(1), dim3(512), 0, (hipStream_t)s, p, Tn, a, b, t_epl, loss, num, den, u, key, call);
  JG_CHECK_LAUNCH();
  return JG_OK;
}
