// Class loss of the semantic-consistency branch (train_semantic_cls; models/base_gan_model.py:686-737, base_model.py:1497-1520):
//   jg_cls_loss   loss = lambda * gate * mean_b l_b,   dlogits[b][j] = lambda * gate * d l_b / d logits[b][j] / B,   argmax[b]
// in ONE launch of ONE workgroup on logits [B, n] (row stride ld >= n; the padding columns are never read).
//   mode 0  cross entropy on int64 labels: l_b = log sum_j exp(x_bj - max_b) + max_b - x_b,label      (fp32, max-subtracted)
//   mode 1  MSE on fp32 targets (n == 1):  l_b = (x_b - t_b)^2
//   mode 2  L1  on fp32 targets (n == 1):  l_b = |x_b - t_b|                                          (gradient sign(d), 0 at d == 0)
// gate: 1 without `prev`; else !(*prev > threshold), read from DEVICE memory (the classifier's loss of the previous iteration: the reference
// compares on the host).  NaN in *prev leaves the gate open, as the reference's `loss_CLS > threshold` does.  With the gate closed the loss is
// 0 and the gradient all zeros, bit for bit (the zeros are written, never 0 * x: a non-finite logit cannot leak through a closed gate).
// A label outside [0, n) is never used as an index: its row contributes NaN to the loss and a zero gradient row.
//
// Order of the sums: wave w (of 16) owns rows w, w + 16, ...; a row is reduced by the 64 lanes (xor butterfly: the same tree for every row)
// and added to the wave's running sum in row order; thread 0 adds the 16 wave sums in wave order.  No atomics, nothing depends on the
// scheduling: the same inputs give the same bits on every launch.
#include "common.h"

namespace {

constexpr int CLS_WAVES = 16;

template <typename T> __device__ __forceinline__ float cls_load(const T* p) { return to_f32(*p); }
template <> __device__ __forceinline__ float cls_load<float>(const float* p) { return *p; }
template <typename T> __device__ __forceinline__ void cls_store(T* p, float v) { *p = from_f32<T>(v); }
template <> __device__ __forceinline__ void cls_store<float>(float* p, float v) { *p = v; }

template <typename T>
__global__ __launch_bounds__(CLS_WAVES * 64) void cls_loss_kernel(const T* __restrict__ logits, long ld, const void* __restrict__ target, int mode, int B, int n,
                                                                  float lambda, const float* __restrict__ prev, float threshold, float* __restrict__ loss,
                                                                  T* __restrict__ dlogits, long ldd, int64_t* __restrict__ argmax, float* state, int state_acc) {
  __shared__ float s_part[CLS_WAVES];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const bool open = prev ? !(*prev > threshold) : true;
  const float gscale = lambda / (float)B;
  float acc = 0.f;
  for (int b = wave; b < B; b += CLS_WAVES) {
    const T* row = logits + (long)b * ld;
    T* drow = dlogits ? dlogits + (long)b * ldd : nullptr;
    float l;
    if (mode == 0) {
      const int64_t lab = static_cast<const int64_t*>(target)[b];
      const bool ok = lab >= 0 && lab < (int64_t)n;
      // row maximum and its lowest index
      float m = -INFINITY;
      int mi = 0x7fffffff;
      for (int j = lane; j < n; j += 64) {
        const float v = cls_load<T>(row + j);
        if (v > m) { m = v; mi = j; }
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const float om = __shfl_xor(m, o);
        const int oi = __shfl_xor(mi, o);
        if (om > m || (om == m && oi < mi)) { m = om; mi = oi; }
      }
      if (mi == 0x7fffffff) mi = 0;      // a row of -inf / NaN only
      float se = 0.f;
      for (int j = lane; j < n; j += 64) se += expf(cls_load<T>(row + j) - m);
      se = wave_sum(se);
      const float xl = ok ? cls_load<T>(row + lab) : 0.f;
      l = ok ? (logf(se) + m) - xl : NAN;
      if (argmax && lane == 0) argmax[b] = mi;
      if (drow) {
        const float inv = 1.f / se;
        for (int j = lane; j < n; j += 64) {
          float g = 0.f;
          if (open && ok) g = gscale * (expf(cls_load<T>(row + j) - m) * inv - (j == (int)lab ? 1.f : 0.f));
          cls_store<T>(drow + j, g);
        }
      }
    } else {
      const float d = cls_load<T>(row) - static_cast<const float*>(target)[b];
      l = mode == 1 ? d * d : fabsf(d);
      if (lane == 0) {
        if (argmax) argmax[b] = 0;
        if (drow) cls_store<T>(drow, open ? gscale * (mode == 1 ? 2.f * d : (d > 0.f ? 1.f : d < 0.f ? -1.f : 0.f)) : 0.f);
      }
    }
    acc += l;
  }
  if (lane == 0) s_part[wave] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    float tot = 0.f;
    const int nw = B < CLS_WAVES ? B : CLS_WAVES;
    for (int w = 0; w < nw; ++w) tot += s_part[w];
    const float out = open ? lambda * (tot / (float)B) : 0.f;
    *loss = out;
    if (state) *state = state_acc ? *state + out : out;
  }
}

}  // namespace

extern "C" int jg_cls_loss(int dtype, int mode, const void* logits, int64_t ld, const void* target, int B, int n, float lambda, const float* prev,
                           float threshold, float* loss, void* dlogits, int64_t ldd, int64_t* argmax, float* state, int state_acc, jg_stream_t s) {
  if (!logits || !target || !loss || B < 1 || n < 1 || ld < n || (dlogits && ldd < n) || mode < 0 || mode > 2 || (mode != 0 && n != 1)) return JG_ERR_BAD_ARG;
  if (dtype != JG_F16 && dtype != JG_BF16 && dtype != JG_CLS_F32) return JG_ERR_BAD_ARG;
  if (dlogits == logits) return JG_ERR_BAD_ARG;
  hipStream_t st = (hipStream_t)s;
#define JG_CLS_LAUNCH(T)                                                                                                                     \
  hipLaunchKernelGGL((cls_loss_kernel<T>), dim3(1), dim3(CLS_WAVES * 64), 0, st, (const T*)logits, (long)ld, target, mode, B, n, lambda, prev, threshold, \
                     loss, (T*)dlogits, (long)ldd, argmax, state, state_acc)
  if (dtype == JG_F16) JG_CLS_LAUNCH(f16_t);
  else if (dtype == JG_BF16) JG_CLS_LAUNCH(bf16_t);
  else JG_CLS_LAUNCH(float);
#undef JG_CLS_LAUNCH
  JG_CHECK_LAUNCH();
  return JG_OK;
}
