// Shared pieces of the tr16 split-K transpose-A weight-grad kernels
// (csrc/wgrad2.hip, csrc/ggnn_wgrad.hip): the padded subtile image that
// ds_read_b64_tr_b16 reads, the register-staged global loads with their
// uniform K-tail test, and the natural-layout LDS write.
//
// One block stages 64 K-rows x 128 columns of each operand per slice, as the
// rows lie in memory, with 256 threads.
#pragma once

#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>

#define WAVE 64
#define WBM 128  // out rows (M) per block
#define WBC 128  // out cols (C) per block
#define WBK 64   // K rows per tile

using bf16 = __hip_bfloat16;
using bf16x8 = __attribute__((ext_vector_type(8))) __bf16;
using f32x4 = __attribute__((ext_vector_type(4))) float;
using uint4v = __attribute__((ext_vector_type(4))) unsigned int;
using bf16x4v = __attribute__((ext_vector_type(4))) __bf16;
typedef __attribute__((address_space(3))) bf16x4v lds_bf16x4;

// Subtiled image for ds_read_b64_tr_b16 hardware-transpose reads (guide
// T10; mapping verified by tools/tr_probe): [4 k][16 col] row-major
// subtiles, padded 128->144 B so the 16 staging b128 writes (subtile
// stride * 2 lanes/subtile) spread over the 64-dword bank modulus.
// One tr read delivers 4 k-column elements per lane (lane l&15 = column)
// — 2 reads per 8-deep MFMA fragment instead of 8 scalar ds_read_u16.
#define W2_SUBB 144
#define W2_SUB(kb, cb) (((kb)*8 + (cb)) * W2_SUBB)
#define W2_TILEB (16 * 8 * W2_SUBB)  // 64 k x 128 col = 18432 B

// each thread loads 4 x 16 B of one operand tile (64 K-rows x 128 cols):
// pass p: k = (t>>4) + 16p, col8 = (t&15)*8
__device__ __forceinline__ void w2_load(const bf16* __restrict__ src, long ld,
                                        int k0, int col0, int tid,
                                        uint4v regs[4], int k_lim) {
  const int kr = tid >> 4;
  const int c8 = (tid & 15) * 8;
  // a per-element bound check makes hipcc branch around each load and
  // drain vmcnt per element (guide §5 trap (c)); hoist to one uniform test
  if (k0 + 64 <= k_lim) {
#pragma unroll
    for (int p = 0; p < 4; ++p)
      regs[p] = *reinterpret_cast<const uint4v*>(
          src + (long)(k0 + kr + 16 * p) * ld + col0 + c8);
  } else {
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const int k = k0 + kr + 16 * p;
      regs[p] = {};
      if (k < k_lim)
        regs[p] = *reinterpret_cast<const uint4v*>(src + (long)k * ld + col0 + c8);
    }
  }
}

// subtiled write: thread covers (k = tid>>4 + 16p, cols (tid&15)*8..+7)
// -> one 16-B write into half ((tid&15)&1) of subtile (k>>2, (tid&15)>>1)
__device__ __forceinline__ void w2_write_nat(char* lds, const uint4v regs[4], int tid) {
  const int kr = tid >> 4;
  const int cb = (tid & 15) >> 1;
  const int halfb = ((tid & 15) & 1) * 16;
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const int k = kr + 16 * p;
    *reinterpret_cast<uint4v*>(lds + W2_SUB(k >> 2, cb) + (k & 3) * 32 + halfb) = regs[p];
  }
}

// One 32-deep K step of a 64 x 64 wave tile: 16 tr16 fragment reads from the
// two staged images, then 16 MFMAs. ks = 0/1 selects the half of the slice;
// wm/wc are the wave's 64-row / 64-column quadrant of the block tile.
__device__ __forceinline__ void w2_mfma_step(const char* a_lds, const char* b_lds, int ks,
                                             int lane, int wm, int wc, f32x4 acc[4][4]) {
  const int kb0 = ks * 8 + (lane >> 4) * 2;  // first 4-k subtile row
  const int slot = (lane & 15) * 8;          // this lane's 8-B column slot
  bf16x8 a_frag[4], b_frag[4];
#pragma unroll
  for (int f = 0; f < 4; ++f) {
    const int cba = wm * 4 + f;
    const int cbb = wc * 4 + f;
    bf16x4v* af = reinterpret_cast<bf16x4v*>(&a_frag[f]);
    bf16x4v* bf = reinterpret_cast<bf16x4v*>(&b_frag[f]);
    af[0] = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(
        (lds_bf16x4*)(a_lds + W2_SUB(kb0, cba) + slot));
    af[1] = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(
        (lds_bf16x4*)(a_lds + W2_SUB(kb0 + 1, cba) + slot));
    bf[0] = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(
        (lds_bf16x4*)(b_lds + W2_SUB(kb0, cbb) + slot));
    bf[1] = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(
        (lds_bf16x4*)(b_lds + W2_SUB(kb0 + 1, cbb) + slot));
  }
  __builtin_amdgcn_s_setprio(1);
#pragma unroll
  for (int fm = 0; fm < 4; ++fm)
#pragma unroll
    for (int fc = 0; fc < 4; ++fc)
      acc[fm][fc] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
          a_frag[fm], b_frag[fc], acc[fm][fc], 0, 0, 0);
  __builtin_amdgcn_s_setprio(0);
}
