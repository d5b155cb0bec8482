// MFMA bf16 GEMM with bias + split-A, tuned for the flow-GNN's node-state
// GEMMs on MI355X (gfx950): out(N, COL) = [A1|A2](N, K) @ W(COL, K)^T + bias.
//
// Shapes in this framework: N ~ 11-12k nodes, K in {128, 256}, COL in
// {128, 512}. hipBLASLt's heuristic picks an 84-91us kernel for these
// shapes (rocprof, profiles/); this kernel is ~10x faster by being sized
// for them: 64x128 tile, BK=64, v_mfma_f32_16x16x32_bf16, XOR-swizzled LDS
// (cdna_hip_programming.md T2: byte ^= (row&7)<<4 spreads the 16-lane
// ds_read_b128 fragment groups across bank slots).
//
// The split-A form reads K-columns [0,K1) from A1 and [K1,K) from A2 so the
// fused-GRU GEMM can consume [messages | hidden] without materializing the
// concatenation.

#include <hip/hip_runtime.h>

#include "mfma_tile.h"

// tile geometry (register-staged pipeline of mfma_tile.h)
#define BM 64
#define BN TILE_BN

// out(N, COL) = concat_K(A1, A2)(N, K) @ W(COL, K)^T + bias
// grid = (ceil(N/BMT), COL/BN), block = 256 (4 waves, 2x2)
// BMT = 64 normally; 32 when the 64-row grid would underfill 256 CUs —
// these GNN GEMMs are HBM-latency-bound at ~0.7 waves/SIMD (PMC: WAIT_ANY
// 73% of wave cycles), so doubling the block count is the lever
// CT (column tail): COL is not a multiple of BN (the GGNN W_e GEMMs at
// H = 64 or 192) — W rows and output columns past COL are masked. The
// 128-aligned instantiations compile without the checks.
template <int BMT, bool CT = false>
__global__ __launch_bounds__(256) void gemm_bias_kernel(
    const bf16* __restrict__ A1, const bf16* __restrict__ A2,
    const bf16* __restrict__ W, const bf16* __restrict__ bias,
    const bf16* __restrict__ addend, long astride,
    const bf16* __restrict__ addend2, long astride2,
    bf16* __restrict__ out, int N, int K,
    int K1, int COL) {
  extern __shared__ __attribute__((aligned(16))) char smem[];

  const int r0 = blockIdx.x * BMT;
  const int c0 = blockIdx.y * BN;
  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x >> 6;   // 4 waves: (wm, wn) = (wid>>1, wid&1)
  const int wm = wid >> 1;            // 2 row-waves of BMT/2 rows
  const int wn = wid & 1;             // 2 col-waves of 64 cols

  constexpr int MFRAG = BMT / 32;     // fragments per row-wave
  f32x4 acc[MFRAG][4] = {};
  tile_regstaged_gemm<BMT, CT>(acc, smem, A1, A2, K1, W, N, K, COL, r0, c0);

  // epilogue: D mapping col = lane&15, row = (lane>>4)*4 + i
#pragma unroll
  for (int m = 0; m < MFRAG; ++m) {
    const int row_base = r0 + wm * (BMT / 2) + m * 16 + (lane >> 4) * 4;
#pragma unroll
    for (int n = 0; n < 4; ++n) {
      const int col = c0 + wn * 64 + n * 16 + (lane & 15);
      if constexpr (CT) {
        if (col >= COL) continue;
      }
      const float b = bias ? __bfloat162float(bias[col]) : 0.0f;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int row = row_base + i;
        if (row < N) {
          float v = acc[m][n][i] + b;
          if (addend) v += __bfloat162float(addend[(long)row * astride + col]);
          if (addend2) v += __bfloat162float(addend2[(long)row * astride2 + col]);
          out[(long)row * COL + col] = __float2bfloat16(v);
        }
      }
    }
  }
}

void launch_gemm_bias2(const bf16* A1, const bf16* A2, const bf16* W,
                       const bf16* bias, const bf16* addend, long astride,
                       const bf16* addend2, long astride2, bf16* out, int N,
                       int K, int K1, int COL, hipStream_t stream) {
  // tests/test_gpu_ggnn.py: test_fused_fwd_teacher_forced[small-64-2] and
  // [small-192-2] take the column tail, every H = 128 case the aligned side
  if (COL % BN != 0) {  // column-tail variant, 32-row tile only
    const dim3 grid((N + 31) / 32, (COL + BN - 1) / BN);
    const size_t lds = tile_lds_bytes(32);
    hipLaunchKernelGGL((gemm_bias_kernel<32, true>), grid, dim3(256), lds,
                       stream, A1, A2, W, bias, addend, astride, addend2,
                       astride2, out, N, K, K1, COL);
    return;
  }
  const long blocks64 = (long)((N + BM - 1) / BM) * (COL / BN);
  // tests/test_gpu_ggnn.py: test_fused_fwd_teacher_forced[small-128-3] takes
  // the 32-row tile, test_gemm_bias_64row_tile the 64-row tile
  if (blocks64 < 384) {
    const dim3 grid((N + 31) / 32, COL / BN);
    const size_t lds = tile_lds_bytes(32);
    hipLaunchKernelGGL(gemm_bias_kernel<32>, grid, dim3(256), lds, stream, A1,
                       A2, W, bias, addend, astride, addend2, astride2, out, N,
                       K, K1, COL);
  } else {
    const dim3 grid((N + BM - 1) / BM, COL / BN);
    const size_t lds = tile_lds_bytes(BM);
    hipLaunchKernelGGL(gemm_bias_kernel<BM>, grid, dim3(256), lds, stream, A1,
                       A2, W, bias, addend, astride, addend2, astride2, out, N,
                       K, K1, COL);
  }
}

void launch_gemm_bias(const bf16* A1, const bf16* A2, const bf16* W,
                      const bf16* bias, const bf16* addend, bf16* out, int N,
                      int K, int K1, int COL, hipStream_t stream) {
  launch_gemm_bias2(A1, A2, W, bias, addend, COL, nullptr, 0, out, N, K, K1,
                    COL, stream);
}

// ---------------------------------------------------------------------------
// Fused gate GEMM + GRU cell: out of the Wcat GEMM's accumulators, compute
// r/z/n and the blended h' directly (VERDICT round-1 item 4: "fuse
// gru_gates into the Wcat GEMM epilogue"). Uses a gate-INTERLEAVED weight
// layout Wcat_perm[row j*4+g] = Wcat[row g*H+j] so one 128-col block owns
// all four gate pre-activations for 32 j-columns; the accumulator tile is
// bounced through LDS in fp32 (more precise than the old bf16 gicat
// round-trip) and the gate math runs as the epilogue. Emits h_new plus the
// R/Z/Nn/HN activations the backward consumes (gru_gates2_bwd unchanged).
// ---------------------------------------------------------------------------

__device__ __forceinline__ float sigf_(float x) { return 1.f / (1.f + __expf(-x)); }

#define GRU_TS 132  // floats per row of the fp32 gate tile

// the gate tile reuses the pipeline's buffers once the K loop is done
constexpr size_t gru_lds_bytes(int bmt) {
  const size_t pipe = tile_lds_bytes(bmt), gate = bmt * GRU_TS * sizeof(float);
  return pipe > gate ? pipe : gate;
}

template <int BMT>
__global__ __launch_bounds__(256) void gemm_gru_kernel(
    const bf16* __restrict__ A1, const bf16* __restrict__ A2,
    const bf16* __restrict__ Wperm, const bf16* __restrict__ bperm,
    const bf16* __restrict__ h_in, bf16* __restrict__ h_new,
    bf16* __restrict__ R, bf16* __restrict__ Z, bf16* __restrict__ Nn,
    bf16* __restrict__ HN, int N, int K, int K1, int H) {
  extern __shared__ __attribute__((aligned(16))) char smem[];

  const int r0 = blockIdx.x * BMT;
  const int c0 = blockIdx.y * BN;  // column block of the PERMUTED 4H space
  const int tid = threadIdx.x;
  const int lane = tid & (WAVE - 1);
  const int wid = tid >> 6;
  const int wm = wid >> 1;
  const int wn = wid & 1;

  constexpr int MFRAG = BMT / 32;
  f32x4 acc[MFRAG][4] = {};
  tile_regstaged_gemm<BMT, false>(acc, smem, A1, A2, K1, Wperm, N, K, 4 * H,
                                  r0, c0);

  // bounce fp32 gate pre-activations (+bias) through LDS, row stride GRU_TS
  float* tile = reinterpret_cast<float*>(smem);
#pragma unroll
  for (int m = 0; m < MFRAG; ++m) {
    const int row = wm * (BMT / 2) + m * 16 + (lane >> 4) * 4;
#pragma unroll
    for (int n = 0; n < 4; ++n) {
      const int col = wn * 64 + n * 16 + (lane & 15);
      const float b = __bfloat162float(bperm[c0 + col]);
#pragma unroll
      for (int i = 0; i < 4; ++i)
        tile[(row + i) * GRU_TS + col] = acc[m][n][i] + b;
    }
  }
  __syncthreads();

  // gate epilogue: item = (row, j-within-block); 4 adjacent tile floats are
  // the r/z/n_i/n_h pre-activations of one (row, j)
  const int j0 = c0 >> 2;  // global j base for this column block (32 j's)
  for (int it = tid; it < BMT * 32; it += 256) {
    const int row = it >> 5;
    const int jj = it & 31;
    const int gr = r0 + row;
    if (gr >= N) continue;
    const f32x4 gse = *reinterpret_cast<const f32x4*>(tile + row * GRU_TS + jj * 4);
    const float r = sigf_(gse[0]);
    const float z = sigf_(gse[1]);
    const float n = tanhf(gse[2] + r * gse[3]);
    const long o = (long)gr * H + j0 + jj;
    const float hv = __bfloat162float(h_in[o]);
    h_new[o] = __float2bfloat16((1.f - z) * n + z * hv);
    R[o] = __float2bfloat16(r);
    Z[o] = __float2bfloat16(z);
    Nn[o] = __float2bfloat16(n);
    HN[o] = __float2bfloat16(gse[3]);
  }
}

void launch_gemm_gru(const bf16* A1, const bf16* A2, const bf16* Wperm,
                     const bf16* bperm, const bf16* h_in, bf16* h_new, bf16* R,
                     bf16* Z, bf16* Nn, bf16* HN, int N, int K, int K1, int H,
                     hipStream_t stream) {
  const int COL = 4 * H;
  const long blocks64 = (long)((N + BM - 1) / BM) * (COL / BN);
  // tests/test_gpu_ggnn.py: test_fused_fwd_teacher_forced[small-128-3] takes
  // the 32-row tile, [n24577-128-1] and [n6081-128-2] the 64-row tile
  if (blocks64 < 384) {
    const dim3 grid((N + 31) / 32, COL / BN);
    const size_t lds = gru_lds_bytes(32);
    hipLaunchKernelGGL(gemm_gru_kernel<32>, grid, dim3(256), lds, stream, A1,
                       A2, Wperm, bperm, h_in, h_new, R, Z, Nn, HN, N, K, K1, H);
  } else {
    const dim3 grid((N + BM - 1) / BM, COL / BN);
    const size_t lds = gru_lds_bytes(BM);
    hipLaunchKernelGGL(gemm_gru_kernel<BM>, grid, dim3(256), lds, stream, A1,
                       A2, Wperm, bperm, h_in, h_new, R, Z, Nn, HN, N, K, K1, H);
  }
}
