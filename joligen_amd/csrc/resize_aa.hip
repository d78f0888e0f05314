// Low-resolution round trip of the palette model's super-resolution task (reference models/palette_model.py:120-130, 546-548):
//   cond_image = Resize((H, W))(Resize((Hlo, Wlo))(gt_image))
// torchvision's Resize on a tensor = F.interpolate(bilinear, antialias=True, align_corners=False): a separable triangle filter, i.e. four
// 1-D passes (W down, H down, W up, H up).  The tap tables of every pass come from the caller (joligen_amd/resize_aa.py reproduces ATen's
// fp32 weights); this file applies all four in ONE launch, the low-resolution image living in LDS only.
//
// A workgroup owns one plane x one band of R output rows:
//   1. the nin input rows the band depends on  -> LDS (one contiguous chunk of the plane: 16-byte loads where W % 4 == 0)
//   2. horizontal reduction  [nin, W]   -> [nin, Wlo]
//   3. vertical reduction    [nin, Wlo] -> [nlo, Wlo]   (the band's low-resolution rows, the extra row(s) of the up pass included)
//   4. horizontal up pass    [nlo, Wlo] -> [nlo, W]     (over the dead image of step 1)
//   5. vertical up pass on the way out: R contiguous output rows, 16-byte stores where W % 4 == 0
// No atomics, a fixed summation order: bit-identical from run to run.  HBM traffic = the plane once out, and nin / R of it in (the input
// rows two neighbouring bands both need): R is the largest band whose images fit LDS, 64 rows at most.
#include "common.h"

namespace {
constexpr int LR_THREADS = 1024;
constexpr int LR_MAX_TAPS = JG_LOWRES_MAX_TAPS;        // down-pass taps per output position (ratio <= 32)
constexpr int LR_UP_TAPS = 3;          // an up pass has support 1: K = 3
constexpr int LR_MAX_BAND = 64;
constexpr int LR_LDS_BIG = 40000;      // floats: 156 KiB of the 160 KiB, one workgroup (16 waves) per CU
constexpr int LR_LDS_SMALL = 16000;    // floats: 62.5 KiB, two workgroups per CU

struct LrTables {      // per pass: first source index [n_out], tap count [n_out], taps [n_out][K]
  const int32_t *dh_min, *dh_size; const float* dh_w;
  const int32_t *dw_min, *dw_size; const float* dw_w;
  const int32_t *uh_min, *uh_size; const float* uh_w;
  const int32_t *uw_min, *uw_size; const float* uw_w;
};

struct LrPlan { int R, nlo_cap, nin_cap, floats; };

// Upper bounds of what a band of R output rows touches (su = Hlo / H <= 1 <= sd = H / Hlo):
//   low rows:   floor(su (r0 + R) - su / 2 + 1.5) - floor(su r0 + su / 2 - 0.5)  <  su R + 3, one more for the fp32 rounding of the tables
//   input rows: floor(sd (l1 + .5) + sd + .5) - floor(sd (l0 + .5) - sd + .5)    <  sd (nlo - 1) + 2 sd + 1 <= sd (nlo - 1) + Kd
// The kernel re-derives the true counts from the tables and leaves the band untouched if they exceed these (they cannot for the
// tables of this shape), so that no table content can make it index outside its LDS images.
bool lr_plan(int H, int W, int Hlo, int Wlo, int Kd, LrPlan* p) {
  for (int R = H < LR_MAX_BAND ? H : LR_MAX_BAND; R >= 1; R /= 2) {
    long nlo = (long)R * Hlo / H + 4;
    if (nlo > Hlo) nlo = Hlo;
    long nin = ((nlo - 1) * H + Hlo - 1) / Hlo + Kd;
    if (nin > H) nin = H;
    const long floats = nin * W + nin * Wlo + nlo * Wlo + (long)Wlo * Kd;
    if (floats <= LR_LDS_BIG) {
      p->R = R, p->nlo_cap = (int)nlo, p->nin_cap = (int)nin, p->floats = (int)floats;
      return true;
    }
  }
  return false;
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }

template <int LDSF>
__global__ __launch_bounds__(LR_THREADS) void lowres_roundtrip_kernel(const float* __restrict__ x, float* __restrict__ y, LrTables t, int H, int W, int Hlo,
                                                                      int Wlo, int Kd, int R, int nbands, int nlo_cap, int nin_cap, int vec) {
  __shared__ __attribute__((aligned(16))) float sm[LDSF];
  const int tid = threadIdx.x;
  const long plane = blockIdx.x / nbands;
  const int r0 = (int)(blockIdx.x % nbands) * R, r1 = r0 + R < H ? r0 + R : H;
  // the band's low-resolution rows [lo_first, lo_end) and input rows [in_first, in_end), from the (monotone) tables
  const int lo_first = clampi(t.uh_min[r0], 0, Hlo - 1);
  const int lo_end = clampi(t.uh_min[r1 - 1] + t.uh_size[r1 - 1], lo_first + 1, Hlo);
  const int in_first = clampi(t.dh_min[lo_first], 0, H - 1);
  const int in_end = clampi(t.dh_min[lo_end - 1] + t.dh_size[lo_end - 1], in_first + 1, H);
  const int nlo = lo_end - lo_first, nin = in_end - in_first;
  if (nlo > nlo_cap || nin > nin_cap) return;      // uniform over the workgroup
  float* sA = sm;                          // [nin][W] input rows; later [nlo][W] the horizontally up-sampled low rows
  float* sB = sA + (long)nin_cap * W;      // [nin][Wlo]
  float* sC = sB + (long)nin_cap * Wlo;    // [nlo][Wlo] the low-resolution band
  float* sW = sC + (long)nlo_cap * Wlo;    // [Wlo][Kd] taps of the horizontal reduction
  const float* xp = x + (plane * H + in_first) * W;
  float* yp = y + (plane * H + r0) * W;

  // 1. input rows -> LDS
  for (int i = tid; i < Wlo * Kd; i += LR_THREADS) sW[i] = t.dw_w[i];
  if (vec) {
    const float4* src = reinterpret_cast<const float4*>(xp);
    float4* dst = reinterpret_cast<float4*>(sA);
    const int n4 = nin * (W / 4);
    for (int i = tid; i < n4; i += LR_THREADS) dst[i] = src[i];
  } else {
    for (int i = tid; i < nin * W; i += LR_THREADS) sA[i] = xp[i];
  }
  __syncthreads();
  // 2. horizontal reduction
  for (int o = tid; o < nin * Wlo; o += LR_THREADS) {
    const int r = o / Wlo, j = o - r * Wlo;
    const int lo = clampi(t.dw_min[j], 0, W - 1);
    const int n = clampi(t.dw_size[j], 0, Kd);
    const float* row = sA + r * W;
    const float* w = sW + j * Kd;
    float acc = 0.f;
    for (int k = 0; k < n; ++k) acc += w[k] * row[lo + k < W ? lo + k : W - 1];
    sB[o] = acc;
  }
  __syncthreads();
  // 3. vertical reduction
  for (int o = tid; o < nlo * Wlo; o += LR_THREADS) {
    const int l = o / Wlo, j = o - l * Wlo;
    const int lo = t.dh_min[lo_first + l];
    const int n = clampi(t.dh_size[lo_first + l], 0, Kd);
    const float* w = t.dh_w + (long)(lo_first + l) * Kd;
    float acc = 0.f;
    for (int k = 0; k < n; ++k) acc += w[k] * sB[(clampi(lo + k, in_first, in_end - 1) - in_first) * Wlo + j];
    sC[o] = acc;
  }
  __syncthreads();
  // 4. horizontal up pass (sA is dead since the barrier after step 2)
  for (int o = tid; o < nlo * W; o += LR_THREADS) {
    const int l = o / W, j = o - l * W;
    const int lo = t.uw_min[j];
    const int n = clampi(t.uw_size[j], 0, LR_UP_TAPS);
    const float* w = t.uw_w + j * LR_UP_TAPS;
    const float* row = sC + l * Wlo;
    float acc = 0.f;
    for (int k = 0; k < n; ++k) acc += w[k] * row[clampi(lo + k, 0, Wlo - 1)];
    sA[o] = acc;
  }
  __syncthreads();
  // 5. vertical up pass -> the band's output rows
  if (vec) {
    const int W4 = W / 4;
    const float4* src = reinterpret_cast<const float4*>(sA);
    float4* dst = reinterpret_cast<float4*>(yp);
    for (int o = tid; o < (r1 - r0) * W4; o += LR_THREADS) {
      const int i = o / W4, j = o - i * W4;
      const int lo = t.uh_min[r0 + i];
      const int n = clampi(t.uh_size[r0 + i], 0, LR_UP_TAPS);
      const float* w = t.uh_w + (r0 + i) * LR_UP_TAPS;
      float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
      for (int k = 0; k < n; ++k) {
        const float4 v = src[(clampi(lo + k, lo_first, lo_end - 1) - lo_first) * W4 + j];
        const float wk = w[k];
        acc.x += wk * v.x, acc.y += wk * v.y, acc.z += wk * v.z, acc.w += wk * v.w;
      }
      dst[o] = acc;
    }
  } else {
    for (int o = tid; o < (r1 - r0) * W; o += LR_THREADS) {
      const int i = o / W, j = o - i * W;
      const int lo = t.uh_min[r0 + i];
      const int n = clampi(t.uh_size[r0 + i], 0, LR_UP_TAPS);
      const float* w = t.uh_w + (r0 + i) * LR_UP_TAPS;
      float acc = 0.f;
      for (int k = 0; k < n; ++k) acc += w[k] * sA[(clampi(lo + k, lo_first, lo_end - 1) - lo_first) * W + j];
      yp[o] = acc;
    }
  }
}

int lr_check_shape(int H, int W, int Hlo, int Wlo, int Kd, LrPlan* p) {
  if (H < 1 || W < 1 || Hlo < 1 || Wlo < 1 || Hlo > H || Wlo > W || Kd < LR_UP_TAPS) return JG_ERR_BAD_ARG;
  if (Kd < 2 * ((H + Hlo - 1) / Hlo) + 1 || Kd < 2 * ((W + Wlo - 1) / Wlo) + 1) return JG_ERR_BAD_ARG;      // shorter than the filter's support
  if (Kd > LR_MAX_TAPS) return JG_ERR_UNSUPPORTED;
  return lr_plan(H, W, Hlo, Wlo, Kd, p) ? JG_OK : JG_ERR_UNSUPPORTED;
}
}  // namespace

extern "C" int jg_lowres_roundtrip_band(int H, int W, int Hlo, int Wlo, int Kdown) {
  LrPlan p;
  const int rc = lr_check_shape(H, W, Hlo, Wlo, Kdown, &p);
  return rc == JG_OK ? p.R : rc;
}

extern "C" int jg_lowres_roundtrip_f32(const float* x, float* y, const int32_t* dh_min, const int32_t* dh_size, const float* dh_w, const int32_t* dw_min,
                                       const int32_t* dw_size, const float* dw_w, const int32_t* uh_min, const int32_t* uh_size, const float* uh_w,
                                       const int32_t* uw_min, const int32_t* uw_size, const float* uw_w, int planes, int H, int W, int Hlo, int Wlo,
                                       int Kdown, jg_stream_t s) {
  if (!x || !y || x == y || !dh_min || !dh_size || !dh_w || !dw_min || !dw_size || !dw_w || !uh_min || !uh_size || !uh_w || !uw_min || !uw_size || !uw_w ||
      planes < 1)
    return JG_ERR_BAD_ARG;
  LrPlan p;
  const int rc = lr_check_shape(H, W, Hlo, Wlo, Kdown, &p);
  if (rc != JG_OK) return rc;
  const int nbands = (H + p.R - 1) / p.R;
  if ((long)planes * nbands > 0x7fffffffL) return JG_ERR_UNSUPPORTED;
  const LrTables t = {dh_min, dh_size, dh_w, dw_min, dw_size, dw_w, uh_min, uh_size, uh_w, uw_min, uw_size, uw_w};
  const int vec = (W % 4 == 0 && ((uintptr_t)x % 16 == 0) && ((uintptr_t)y % 16 == 0)) ? 1 : 0;
  const dim3 grid((unsigned)((long)planes * nbands));
  if (p.floats <= LR_LDS_SMALL)
    hipLaunchKernelGGL((lowres_roundtrip_kernel<LR_LDS_SMALL>), grid, dim3(LR_THREADS), 0, (hipStream_t)s, x, y, t, H, W, Hlo, Wlo, Kdown, p.R, nbands,
                       p.nlo_cap, p.nin_cap, vec);
  else
    hipLaunchKernelGGL((lowres_roundtrip_kernel<LR_LDS_BIG>), grid, dim3(LR_THREADS), 0, (hipStream_t)s, x, y, t, H, W, Hlo, Wlo, Kdown, p.R, nbands,
                       p.nlo_cap, p.nin_cap, vec);
  JG_CHECK_LAUNCH();
  return JG_OK;
}
