// All six GGNN parameter gradients at H = 128 in one split-K launch.
//
// With K = S*N rows of saved activations and gradients,
//   gW_ih (3H, H) = [r | z | gi_n]^T M        gb_ih = colsum [r | z | gi_n]
//   gW_hh (3H, H) = [r | z | gh_n]^T HH       gb_hh = colsum [r | z | gh_n]
//   gW_e  (H, H)  = Gwh^T HH                  gb_e  = colsum Gwh
// where r, z, gi_n, gh_n are the four H-wide column blocks of Ggicat (K, 4H).
// That is seven live 128 x 128 x K products. The packed (4H, 2H) form that
// csrc/wgrad.hip computes has an eighth and a ninth, gi_n^T HH and gh_n^T M,
// which belong to structurally zero blocks of Wcat: they are never formed.
//
// Grid: one block per (K chunk, tile), 1-D. The seven tiles of a chunk sit
// at block indices that differ by multiples of 8, so under round-robin
// dispatch they share an XCD and the repeated reads of a chunk (r and z
// twice, M three times, HH four times) can hit that L2. Placement serves
// speed only: every block is self-contained.
//
// Inner loop: wgrad2's tr16 form (csrc/wgrad_tr16.h): operands staged as
// they lie in memory into padded [4 k][16 col] subtiles, double-buffered,
// next slice's global loads issued before this slice's MFMAs. Loading two
// or three slices ahead in further register sets measured slower
// (profiles/ggnn_wgrad.md) and is not kept.
//
// Bias gradients: each A column block has one owner tile (r, z, gi_n with
// the M tiles, gh_n and Gwh with their HH tiles). The owner sums the block's
// columns from the registers it stages anyway, 8 columns per thread, and
// folds the 16 row-groups through LDS after the K loop: one atomic per
// column per chunk. r/z feed b_ih and b_hh from that one value.
//
// Every output is accumulated with fp32 atomics and never plain-stored, so
// the six destinations may be live .grad views at any 4-byte alignment.

#include <hip/hip_runtime.h>

#include "wgrad_tr16.h"

#define GW_H 128
#define GW_TILES 7
#define GW_XCD 8
#define GW_LDS (4 * W2_TILEB)  // 2 operands x 2 buffers = 73728 B
#define GW_EPI_LD 132          // fp32 row stride of the epilogue image

struct GgnnWgradArgs {
  const bf16* ggicat;  // (K, 4H)
  const bf16* gwh;     // (K, H)
  const bf16* m;       // (K, H)
  const bf16* hh;      // (K, H): the first S slabs of HH
  float* w_ih;         // (3H, H)
  float* w_hh;         // (3H, H)
  float* w_e;          // (H, H)
  float* b_ih;         // (3H)
  float* b_hh;         // (3H)
  float* b_e;          // (H)
  int K;
  int kchunk;
  int zsplit;
  int b_hh_rz;  // 1: add the r/z column sums to b_hh[0, 2H) as well
};

__device__ __forceinline__ void gw_colsum(const uint4v regs[4], float cs[8]) {
#pragma unroll
  for (int p = 0; p < 4; ++p)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      cs[2 * j] += __uint_as_float(regs[p][j] << 16);
      cs[2 * j + 1] += __uint_as_float(regs[p][j] & 0xffff0000u);
    }
}

// LDS_EPI: pass the accumulator tile through LDS so that one atomic
// wave-instruction covers 256 contiguous bytes of one output row; otherwise
// add straight from the MFMA layout (four 64-B row segments).
template <bool LDS_EPI>
__global__ __launch_bounds__(256, 2) void ggnn_wgrad_kernel(GgnnWgradArgs p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
#define A_LDS(i) (smem + (i) * (2 * W2_TILEB))
#define B_LDS(i) (smem + W2_TILEB + (i) * (2 * W2_TILEB))

  // block -> (chunk, tile): chunk = 8 cg + x, block = (7 cg + tile) 8 + x
  const int x = blockIdx.x % GW_XCD;
  const int g = blockIdx.x / GW_XCD;
  const int tile = g % GW_TILES;
  const int chunk = (g / GW_TILES) * GW_XCD + x;
  if (chunk >= p.zsplit) return;

  // tile -> operands and destinations (all block-uniform)
  //   0 r x M    1 z x M    2 gi_n x M    3 r x HH    4 z x HH
  //   5 gh_n x HH    6 Gwh x HH
  const bool we = tile == 6;
  const int ablk = tile < 3 ? tile : (tile == 5 ? 3 : tile - 3);
  const bf16* A = we ? p.gwh : p.ggicat;
  const long lda = we ? GW_H : 4 * GW_H;
  const int acol = we ? 0 : ablk * GW_H;
  const bf16* B = tile < 3 ? p.m : p.hh;
  float* out = we ? p.w_e
                  : (tile < 3 ? p.w_ih + tile * GW_H * GW_H
                              : p.w_hh + (tile - 3) * GW_H * GW_H);
  float* cs1 = nullptr;
  float* cs2 = nullptr;
  if (tile < 3) cs1 = p.b_ih + tile * GW_H;
  if (tile < 2 && p.b_hh_rz) cs2 = p.b_hh + tile * GW_H;
  if (tile == 5) cs1 = p.b_hh + 2 * GW_H;
  if (we) cs1 = p.b_e;
  const bool owner = cs1 != nullptr;

  const int k_begin = chunk * p.kchunk;
  const int k_end = min(p.K, k_begin + p.kchunk);
  const int tid = threadIdx.x;
  const int lane = tid & (WAVE - 1);
  const int wid = tid >> 6;
  const int wm = wid >> 1;
  const int wc = wid & 1;

  f32x4 acc[4][4] = {};
  float cs[8] = {};

  uint4v a_regs[4], b_regs[4];
  w2_load(A, lda, k_begin, acol, tid, a_regs, k_end);
  w2_load(B, GW_H, k_begin, 0, tid, b_regs, k_end);
  w2_write_nat(A_LDS(0), a_regs, tid);
  w2_write_nat(B_LDS(0), b_regs, tid);
  if (owner) gw_colsum(a_regs, cs);
  __syncthreads();

  int cur = 0;
  for (int k0 = k_begin; k0 < k_end; k0 += WBK) {
    const bool has_next = (k0 + WBK) < k_end;
    if (has_next) {  // T14: issue next slice's loads before this slice's MFMAs
      w2_load(A, lda, k0 + WBK, acol, tid, a_regs, k_end);
      w2_load(B, GW_H, k0 + WBK, 0, tid, b_regs, k_end);
    }
    // rolled, as in wgrad2 (instruction fetch)
#pragma unroll 1
    for (int ks = 0; ks < 2; ++ks)
      w2_mfma_step(A_LDS(cur), B_LDS(cur), ks, lane, wm, wc, acc);
    __syncthreads();
    if (has_next) {
      w2_write_nat(A_LDS(cur ^ 1), a_regs, tid);
      w2_write_nat(B_LDS(cur ^ 1), b_regs, tid);
      if (owner) gw_colsum(a_regs, cs);
    }
    __syncthreads();
    cur ^= 1;
  }
#undef A_LDS
#undef B_LDS

  // the K loop is done and every wave is past its last LDS read: smem is free
  float* fs = reinterpret_cast<float*>(smem);
  if (owner) {
    // fs[kr][col]: thread (kr = tid>>4) holds columns (tid&15)*8 .. +7
    float* row = fs + (tid >> 4) * GW_H + (tid & 15) * 8;
    *reinterpret_cast<f32x4*>(row) = f32x4{cs[0], cs[1], cs[2], cs[3]};
    *reinterpret_cast<f32x4*>(row + 4) = f32x4{cs[4], cs[5], cs[6], cs[7]};
    __syncthreads();
    if (tid < GW_H) {
      float s = 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) s += fs[r * GW_H + tid];
      atomicAdd(cs1 + tid, s);
      if (cs2 != nullptr) atomicAdd(cs2 + tid, s);
    }
    if (LDS_EPI) __syncthreads();
  }

  // accumulator layout: D col = lane&15 (B column), row = (lane>>4)*4 + i
  if (LDS_EPI) {
#pragma unroll
    for (int fm = 0; fm < 4; ++fm) {
      const int m_base = wm * 64 + fm * 16 + (lane >> 4) * 4;
#pragma unroll
      for (int fc = 0; fc < 4; ++fc) {
        const int c = wc * 64 + fc * 16 + (lane & 15);
#pragma unroll
        for (int i = 0; i < 4; ++i) fs[(m_base + i) * GW_EPI_LD + c] = acc[fm][fc][i];
      }
    }
    __syncthreads();
    // wave w adds rows [32w, 32w+32), half a row (256 B) per instruction
#pragma unroll 8
    for (int r = 0; r < 32; ++r) {
      const int m = wid * 32 + r;
      atomicAdd(out + m * GW_H + lane, fs[m * GW_EPI_LD + lane]);
      atomicAdd(out + m * GW_H + 64 + lane, fs[m * GW_EPI_LD + 64 + lane]);
    }
  } else {
#pragma unroll
    for (int fm = 0; fm < 4; ++fm) {
      const int m_base = wm * 64 + fm * 16 + (lane >> 4) * 4;
#pragma unroll
      for (int fc = 0; fc < 4; ++fc) {
        const int c = wc * 64 + fc * 16 + (lane & 15);
#pragma unroll
        for (int i = 0; i < 4; ++i)
          atomicAdd(out + (m_base + i) * GW_H + c, acc[fm][fc][i]);
      }
    }
  }
}

// Chunk rule. The output is fixed, so the atomics cost zsplit x 448 KiB at
// the chip-wide float-atomic rate whatever the schedule, and they are added
// when the blocks end, which is at the same time for all of them. A chunk
// gives seven blocks of which a CU holds two (LDS). About GW_ZTARGET chunks
// measured best at the training shape (K = 57 835; tools/ggnn_wgrad_probe.py,
// profiles/ggnn_wgrad.md); below GW_KCHUNK_MIN rows a chunk's atomics
// outweigh its loads.
#define GW_ZTARGET 56
#define GW_KCHUNK_MIN 768
#define GW_LDS_EPI_DEFAULT 1

// K rows per chunk for a K-row problem; kchunk > 0 overrides the rule
int ggnn_wgrad_kchunk(int K, int kchunk) {
  if (kchunk <= 0) kchunk = max((K + GW_ZTARGET - 1) / GW_ZTARGET, GW_KCHUNK_MIN);
  return ((kchunk + WBK - 1) / WBK) * WBK;
}

// kchunk <= 0 and lds_epi < 0 take the defaults; they are launcher
// parameters so that the probe can sweep them in one build
void launch_ggnn_wgrad(const bf16* ggicat, const bf16* gwh, const bf16* m, const bf16* hh,
                       float* w_ih, float* w_hh, float* w_e, float* b_ih, float* b_hh,
                       float* b_e, int K, int b_hh_rz, int kchunk, int lds_epi,
                       hipStream_t stream) {
  if (K <= 0) return;
  // dynamic LDS above 64 KiB: raise the kernels' limit once per process
  static const bool raised = [] {
    return hipFuncSetAttribute(reinterpret_cast<const void*>(&ggnn_wgrad_kernel<true>),
                               hipFuncAttributeMaxDynamicSharedMemorySize,
                               GW_LDS) == hipSuccess &&
           hipFuncSetAttribute(reinterpret_cast<const void*>(&ggnn_wgrad_kernel<false>),
                               hipFuncAttributeMaxDynamicSharedMemorySize,
                               GW_LDS) == hipSuccess;
  }();
  (void)raised;
  GgnnWgradArgs p;
  p.ggicat = ggicat;
  p.gwh = gwh;
  p.m = m;
  p.hh = hh;
  p.w_ih = w_ih;
  p.w_hh = w_hh;
  p.w_e = w_e;
  p.b_ih = b_ih;
  p.b_hh = b_hh;
  p.b_e = b_e;
  p.K = K;
  p.kchunk = ggnn_wgrad_kchunk(K, kchunk);
  p.zsplit = (K + p.kchunk - 1) / p.kchunk;
  p.b_hh_rz = b_hh_rz;
  const int groups = (p.zsplit + GW_XCD - 1) / GW_XCD;
  const dim3 grid(groups * GW_TILES * GW_XCD);
  if (lds_epi < 0) lds_epi = GW_LDS_EPI_DEFAULT;
  if (lds_epi)
    hipLaunchKernelGGL(ggnn_wgrad_kernel<true>, grid, dim3(256), GW_LDS, stream, p);
  else
    hipLaunchKernelGGL(ggnn_wgrad_kernel<false>, grid, dim3(256), GW_LDS, stream, p);
}
