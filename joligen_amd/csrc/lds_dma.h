// LDS-DMA staging, transposing fragment reads, pixel-column swizzles and the XCD-aware tile order: the device helpers shared by the
// halo-resident and LDS-DMA kernels (conv_halo, conv_p64, gemm_nt, gemm_tn, wgrad_halo, wgrad_sw, wgrad_kxk).  Each hardware contract
// below is stated here ONCE; a new kernel includes this header, it does not copy from a neighbour.
//
// Everything is __forceinline__ and has internal linkage; the zero page is one 16-byte object per translation unit that includes this
// header (the s16x4_t / lds_v4 typedefs live in common.h, for the files that want the transposing read without a zero page).
#pragma once
#include "common.h"

namespace {

// Out-of-image / out-of-range lanes of an LDS-DMA round cannot be predicated off (the instruction writes wave_base + lane * 16 for every
// lane, and the LDS slot must become zero): they fetch this page instead.  It must therefore always be a valid, readable address.
__device__ uint4 jg_zero_page = {0u, 0u, 0u, 0u};

// LDS-DMA (global_load_lds_dwordx4: 16 bytes per lane, global -> LDS at M0 + lane * 16, no VGPR round trip) issued from inline asm:
// hipcc does not model it, so it neither drains it with a vmcnt(0) before the next ds_read (what it does for
// __builtin_amdgcn_global_load_lds) nor counts it -- which is what lets a ring keep several stages in flight across one raw s_barrier
// per K step, and why every wait on these loads is an explicit wait_vmcnt<N>() with a count kept BY HAND (N = the loads the wave issued
// after the ones it waits for).  M0 (the LDS destination base) is compiler-reserved: saved, written and restored inside the one statement
// (cdna_hip_programming.md 5.7).  lds_dst is the wave-uniform LDS byte address of lane 0's slot.
__device__ __forceinline__ void glds16(const void* gsrc, unsigned lds_dst) {
  unsigned keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
               : "=&s"(keep) : "v"(gsrc), "s"(lds_dst) : "memory");
}
// at most N of this wave's vector-memory loads (glds16 included) still in flight; they return in order
template <int N> __device__ __forceinline__ void wait_vmcnt() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// One 16x16x32 MFMA operand fragment out of a PIXEL-major LDS image: two transposing reads (ds_read_b64_tr_b16: lane i of a 16-lane
// group addresses 4 channels of pixel k0 + i / 4 and receives channel c0 + i of pixels k0 .. k0 + 3) at byte offsets off0 / off1 of
// smb give the 8 k-values of a lane.  The reads stay compiler-visible builtins: their s_waitcnt lgkmcnt is the compiler's.
// (smb is taken by reference on purpose: with a by-value pointer hipcc schedules the reads of the wgrad MFMA loops in another order)
__device__ __forceinline__ uint4 tr_frag(const char* const& smb, int off0, int off1) {
  const uint2 u0 = __builtin_bit_cast(uint2, __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4)(smb + off0)));
  const uint2 u1 = __builtin_bit_cast(uint2, __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4)(smb + off1)));
  return make_uint4(u0.x, u0.y, u1.x, u1.y);
}

// Swizzles of the 32-byte block index of a pixel row, by pixel COLUMN c (so that vertical tap shifts are plain address offsets).  A
// 32-lane service group of the transposing read touches the 8 pixels {h .. h+3, h+8 .. h+11} x 32 B; each function is injective on
// the bank positions of every such set, for every h, i.e. conflict-free for every horizontal tap shift.  LDS-DMA writes lane-linearly,
// so the writer applies the same XOR to the SOURCE chunk index (cdna_hip_programming.md 5.4 rule 21).
// 2-bit swizzle of a 128-byte pixel row (4 blocks of 32 B): the row is half a bank row, the parity of the column picks the half and
// bits {1, 3} of the column tell the four pixels of one parity apart
__device__ __forceinline__ int f4(int c) { return ((c >> 1) & 1) | (((c >> 3) & 1) << 1); }
// 3-bit swizzle of a 256-byte pixel row (8 blocks of 32 B): every pixel starts a bank row, bits {0, 1, 3} number the 8 pixels
__device__ __forceinline__ int f8(int c) { return (c & 3) | (((c >> 3) & 1) << 2); }
// 1-bit swizzle of a 64-byte pixel row (2 blocks of 32 B): the 8 pixels {h..h+3, h+8..h+11} of a service group are four bank quarters
// (pixel % 4) x the two blocks, told apart by bit 3 of the column
__device__ __forceinline__ int f2(int c) { return (c >> 3) & 1; }
// block swizzle of a dy pixel row of BCO channels
template <int BCO> __device__ __forceinline__ int fdy(int c) { return BCO == 32 ? f2(c) : BCO == 64 ? f4(c) : f8(c); }

// XCD-aware tile order: workgroup b runs on XCD b % 8, so with the plain order neighbouring tile ids -- which read the SAME operand
// rows -- sit in eight different L2s and the operand crosses HBM once per L2 (gemm_nt.hip, PMC: 1.49 x the algorithmic bytes on the
// 128 x 128 tile; gemm_tn.hip: 232 MB read per launch for 100 MB of operands).  Each XCD instead owns a contiguous run of ids: the
// first nwg % 8 XCDs take nwg / 8 + 1 ids, the others nwg / 8 -- a bijection of the launch order `lin` onto [0, nwg) for every nwg.
// (I: int or unsigned, as the caller holds `lin` -- the same value either way, but lin >> 3 is s_ashr for one and s_lshr for the other)
template <typename I> __device__ __forceinline__ int xcd_remap(I lin, int nwg) {
  const int q = nwg >> 3, r8 = nwg & 7, xcd = lin & 7, idx = lin >> 3;
  return (xcd < r8 ? xcd * (q + 1) : r8 * (q + 1) + (xcd - r8) * q) + idx;
}
// the common case: a 1-D grid
__device__ __forceinline__ int xcd_block_id() { return xcd_remap<unsigned>(blockIdx.x, gridDim.x); }

}  // namespace
