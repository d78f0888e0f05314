// Kernel-side parameter block and split-K policy shared by the weight-gradient kernels (gemm_tn.hip, wgrad_halo.hip, wgrad_sw.hip, wgrad_kxk.hip).
#pragma once
#include "common.h"

struct WgP {
  const char* dy; const char* x; char* dw; float* dbias;
  int Mpix, Cout, Ktot;  // reduction length, rows, cols (= R*S*Cin)
  int H, W, Cin, R, S, pad, stride, Ho, Wo;
  int Cin_out, Cout_out;
  long lddy, ldx, lddw;
  int nh, splitk;
  long sdyb, sdyh, sxb, sxh, sdwb, sdwh;
  float alpha;
  int out_mode;
  int B;
  float dbias_scale;
  int x_up;      // 1: x is [B, H/2, W/2, Cin], read through the nearest-upsample index map (halo kernel only); 2: the same in sub-pixel form
  int reflect;   // 1: the x halo mirrors the interior at the image border (ReflectionPad2d(1) + pad-0 3x3 conv)
};

// Split-K choice of the halo-resident 3x3 kernels (wgrad_halo.hip, wgrad_sw.hip): `slots` workgroups run at a time (1 or 2 per CU by
// LDS), so the launch runs in rounds; every block walks `per` tiles and pays a fixed prologue + atomic epilogue worth about `ovh` tiles.
inline void jg_wgrad_pick_split(int npairs, int ntiles, int ovh, int slots, int* per_out, int* splitk_out) {
  long best = -1;
  int bper = ntiles, bsk = 1;
  if (jg_tune(JG_TUNE_DETERMINISTIC) != 0) {     // no split over the tiles: one workgroup, one thread per element of dw -- a reproducible sum
    *per_out = ntiles; *splitk_out = 1;
    return;
  }
  const int skmax = ntiles < 2048 / npairs + 1 ? ntiles : 2048 / npairs + 1;
  for (int sk = 1; sk <= skmax; ++sk) {
    const int per = (ntiles + sk - 1) / sk;
    const int ske = (ntiles + per - 1) / per;
    const long blocks = (long)npairs * ske;
    const long rounds = (blocks + slots - 1) / slots;
    const long cost = (long)(per + ovh) * rounds;
    if (best < 0 || cost < best) { best = cost; bper = per; bsk = ske; }
  }
  *per_out = bper; *splitk_out = bsk;
}

// wgrad_halo.hip: returns true when the shape was handled by the halo-resident 3x3 kernel.
// dry_run: only answer whether the kernel WOULD take the problem (the grouped entry validates every descriptor before it launches anything)
bool jg_wgrad_halo_try(int dtype, const WgP& p, int nbatch, hipStream_t st, bool dry_run = false);
// wgrad_kxk.hip: returns true when the shape was handled by the halo-resident large-kernel (7x7) weight-gradient kernel.
bool jg_wgrad_kxk_try(int dtype, const WgP& p, int nbatch, hipStream_t st, bool dry_run = false);
// wgrad_sw.hip: sliding-window form of the 16-row x 64-co tile (v_mfma_f32_32x32x16, one pixel row per K step); the caller has validated the shape.
void jg_wgrad_sw_launch(int dtype, const WgP& p, hipStream_t st);
