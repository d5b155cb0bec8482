// Transformer-shape bf16 GEMM: out(N, COL) = A(N, K) @ W(COL, K)^T [+ bias]
// [+ addend], MI355X (gfx950).
//
// hipBLASLt runs the encoder projections at 173-420 TF on these shapes
// (rocprof, profiles/): this kernel applies the guide's minimum 2-phase
// glds pipeline (cdna_hip_programming.md §5.5 T3 recipe): 128x128 tile,
// BK=64, double-buffered LDS filled by global_load_lds (16-B pieces),
// XOR-swizzle applied on the SOURCE address + the read side (rule 21),
// one vmcnt(0)+barrier per K-tile, s_setprio around the MFMA cluster.
//
// Geometry contract (wrapper-enforced, else fall back to rocBLAS):
// N % 128 == 0, K % 64 == 0, COL % 128 == 0.

#include <hip/hip_runtime.h>

#include "mfma_tile.h"

#define BM2 128
#define BN2 TILE_BN

// BMT2 = 128 normally; 64 when the 128-row grid would underfill the chip
// (e.g. the CodeT5 decoder's N=4096 projections: 32x6 = 192 blocks on 512
// resident-block slots)
template <int BMT2>
__global__ __launch_bounds__(256) void gemm2_kernel(
    const bf16* __restrict__ A, const bf16* __restrict__ W,
    const float* __restrict__ bias, const bf16* __restrict__ addend,
    bf16* __restrict__ out, int N, int K, int COL) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  // double-buffered A and B tiles: tile_lds_bytes(BMT2)
  const int r0 = blockIdx.x * BMT2;
  const int c0 = blockIdx.y * BN2;
  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x >> 6;
  const int wm = wid >> 1;  // 2x2 waves, 64x64 tile each
  const int wn = wid & 1;

  constexpr int MF = BMT2 / 32;  // a-fragments per row-wave
  f32x4 acc[MF][4] = {};

  tile_glds_gemm<BMT2>(acc, smem, A + (long)r0 * K, W + (long)c0 * K, K, lane,
                       wid);

  // epilogue: the D fragment layout (col = lane&15, row = (lane>>4)*4+i)
  // would need 64 x 2-B scalar stores per lane (store-issue bound, T21
  // diagnostic); bounce the tile through the now-free LDS and store
  // 16-B-per-lane row-major instead (8 dwordx4 stores per thread).
  __syncthreads();
  char* tile = smem;  // [BMT2][128] bf16
#pragma unroll
  for (int fm = 0; fm < MF; ++fm) {
    const int row = wm * (BMT2 / 2) + fm * 16 + (lane >> 4) * 4;
#pragma unroll
    for (int fn = 0; fn < 4; ++fn) {
      const int col = wn * 64 + fn * 16 + (lane & 15);
      const float b = bias ? bias[c0 + col] : 0.f;
#pragma unroll
      for (int i = 0; i < 4; ++i)
        *reinterpret_cast<__bf16*>(tile + (row + i) * 256 + col * 2) =
            (__bf16)(acc[fm][fn][i] + b);
    }
  }
  __syncthreads();
  {
    const int trow = threadIdx.x >> 4;          // 16 rows per pass
    const int tcol = (threadIdx.x & 15) * 8;    // 8 bf16 = 16 B per store
#pragma unroll
    for (int p = 0; p < BMT2 / 16; ++p) {
      const int row = trow + p * 16;
      uint4 v = *reinterpret_cast<const uint4*>(tile + row * 256 + tcol * 2);
      if (addend) {
        __bf16 vals[8];
        *reinterpret_cast<uint4*>(vals) = v;
        const bf16* add = addend + (long)(r0 + row) * COL + c0 + tcol;
#pragma unroll
        for (int j = 0; j < 8; ++j)
          vals[j] = (__bf16)((float)vals[j] + __bfloat162float(add[j]));
        v = *reinterpret_cast<const uint4*>(vals);
      }
      *reinterpret_cast<uint4*>(out + (long)(r0 + row) * COL + c0 + tcol) = v;
    }
  }
}

void launch_gemm2(const bf16* A, const bf16* W, const float* bias,
                  const bf16* addend, bf16* out, int N, int K, int COL,
                  hipStream_t stream) {
  const long blocks128 = (long)(N / BM2) * (COL / BN2);
  // tests/test_gpu_gemm_tiles.py: test_gemm2_64row_tile takes the 64-row
  // tile, test_gemm2_128row_tile (1024 x 8192 = 512 blocks) the 128-row tile
  if (N % 128 == 0 && blocks128 < 512) {
    const dim3 grid(N / 64, COL / BN2);
    hipLaunchKernelGGL(gemm2_kernel<64>, grid, dim3(256),
                       tile_lds_bytes(64), stream, A, W, bias, addend, out, N, K, COL);
  } else {
    const dim3 grid(N / BM2, COL / BN2);
    hipLaunchKernelGGL(gemm2_kernel<128>, grid, dim3(256),
                       tile_lds_bytes(BM2), stream, A, W, bias, addend, out, N, K, COL);
  }
}
