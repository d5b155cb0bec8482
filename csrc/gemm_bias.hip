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

// Edges prefetched per row by the gathering variants (mfma_tile.h): 4 on
// the 32-row tile; 2 on the 64-row tile, where 3 or 4 take gemm_gru from 114
// to 153 / 194 VGPRs and below the 3 blocks per CU its LDS allows (measured
// on the training shape: 19.5 us with 2, 27.6 with 3, 25.5 with 4).
constexpr int gather_gpf(int bmt) { return bmt == 32 ? 4 : 2; }

// epilogue of gemm_bias_kernel and gates_gemm_kernel: bias, two strided
// addends, bf16 store. D mapping col = lane&15, row = (lane>>4)*4 + i
template <int BMT, bool CT>
__device__ __forceinline__ void gemm_bias_epilogue(
    const f32x4 (&acc)[BMT / 32][4], const bf16* __restrict__ bias,
    const bf16* __restrict__ addend, long astride,
    const bf16* __restrict__ addend2, long astride2, bf16* __restrict__ out,
    int N, int COL, int r0, int c0, int lane, int wm, int wn) {
#pragma unroll
  for (int m = 0; m < BMT / 32; ++m) {
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

// out(N, COL) = concat_K(A1, A2)(N, K) @ W(COL, K)^T + bias
// grid = (ceil(N/BMT), COL/BN), block = 256 (4 waves, 2x2)
// BMT = 64 normally; 32 when the 64-row grid would underfill 256 CUs —
// these GNN GEMMs are HBM-latency-bound at ~0.7 waves/SIMD (PMC: WAIT_ANY
// 73% of wave cycles), so doubling the block count is the lever
// CT (column tail): COL is not a multiple of BN (the GGNN W_e GEMMs at
// H = 64 or 192) — W rows and output columns past COL are masked. The
// 128-aligned instantiations compile without the checks.
// GPF > 0: A1 is summed over a CSR graph's in-edges while it is staged
// (mfma_tile.h TileGather; the GGNN backward's grad_h GEMM reads
// spmm(grad_A[:, :H]) this way). Column block 0 stores the staged sums.
template <int BMT, bool CT = false, int GPF = 0>
__global__ __launch_bounds__(256) void gemm_bias_kernel(
    const bf16* __restrict__ A1, const bf16* __restrict__ A2,
    const bf16* __restrict__ W, const bf16* __restrict__ bias,
    const bf16* __restrict__ addend, long astride,
    const bf16* __restrict__ addend2, long astride2,
    bf16* __restrict__ out, int N, int K,
    int K1, int COL, TileGather g) {
  extern __shared__ __attribute__((aligned(16))) char smem[];

  const int r0 = blockIdx.x * BMT;
  const int c0 = blockIdx.y * BN;
  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x >> 6;   // 4 waves: (wm, wn) = (wid>>1, wid&1)
  const int wm = wid >> 1;            // 2 row-waves of BMT/2 rows
  const int wn = wid & 1;             // 2 col-waves of 64 cols

  constexpr int MFRAG = BMT / 32;     // fragments per row-wave
  f32x4 acc[MFRAG][4] = {};
  if (blockIdx.y != 0) g.out = nullptr;
  tile_regstaged_gemm<BMT, CT, GPF>(acc, smem, A1, A2, K1, W, N, K, COL, r0,
                                       c0, g);
  gemm_bias_epilogue<BMT, CT>(acc, bias, addend, astride, addend2, astride2,
                              out, N, COL, r0, c0, lane, wm, wn);
}

// g_indptr != nullptr: A1 (row stride g_lda) is gathered over the CSR graph
// while it is staged, and the (N, K1) sums are also stored to g_out
void launch_gemm_bias2(const bf16* A1, const bf16* A2, const bf16* W,
                       const bf16* bias, const bf16* addend, long astride,
                       const bf16* addend2, long astride2, bf16* out, int N,
                       int K, int K1, int COL, hipStream_t stream,
                       const int* g_indptr, const int* g_indices, long g_lda,
                       bf16* g_out) {
  const bool g = g_indptr != nullptr;
  const TileGather tg = {g_indptr, g_indices, g_lda, g_out};
  // tests/test_gpu_ggnn.py: test_fused_fwd_teacher_forced[small-64-2] and
  // [small-192-2] take the column tail, every H = 128 case the aligned side
  if (COL % BN != 0) {  // column-tail variant, 32-row tile only
    const dim3 grid((N + 31) / 32, (COL + BN - 1) / BN);
    const size_t lds = tile_lds_bytes(32);
    if (g)
      hipLaunchKernelGGL((gemm_bias_kernel<32, true, gather_gpf(32)>), grid, dim3(256),
                         lds, stream, A1, A2, W, bias, addend, astride, addend2,
                         astride2, out, N, K, K1, COL, tg);
    else
      hipLaunchKernelGGL((gemm_bias_kernel<32, true>), grid, dim3(256), lds,
                         stream, A1, A2, W, bias, addend, astride, addend2,
                         astride2, out, N, K, K1, COL, tg);
    return;
  }
  const long blocks64 = (long)((N + BM - 1) / BM) * (COL / BN);
  // tests/test_gpu_ggnn.py: test_fused_fwd_teacher_forced[small-128-3] takes
  // the 32-row tile, test_gemm_bias_64row_tile the 64-row tile
  if (blocks64 < 384) {
    const dim3 grid((N + 31) / 32, COL / BN);
    const size_t lds = tile_lds_bytes(32);
    if (g)
      hipLaunchKernelGGL((gemm_bias_kernel<32, false, gather_gpf(32)>), grid, dim3(256),
                         lds, stream, A1, A2, W, bias, addend, astride, addend2,
                         astride2, out, N, K, K1, COL, tg);
    else
      hipLaunchKernelGGL(gemm_bias_kernel<32>, grid, dim3(256), lds, stream,
                         A1, A2, W, bias, addend, astride, addend2, astride2,
                         out, N, K, K1, COL, tg);
  } else {
    const dim3 grid((N + BM - 1) / BM, COL / BN);
    const size_t lds = tile_lds_bytes(BM);
    if (g)
      hipLaunchKernelGGL((gemm_bias_kernel<BM, false, gather_gpf(BM)>), grid, dim3(256),
                         lds, stream, A1, A2, W, bias, addend, astride, addend2,
                         astride2, out, N, K, K1, COL, tg);
    else
      hipLaunchKernelGGL(gemm_bias_kernel<BM>, grid, dim3(256), lds, stream,
                         A1, A2, W, bias, addend, astride, addend2, astride2,
                         out, N, K, K1, COL, tg);
  }
}

void launch_gemm_bias(const bf16* A1, const bf16* A2, const bf16* W,
                      const bf16* bias, const bf16* addend, bf16* out, int N,
                      int K, int K1, int COL, hipStream_t stream) {
  launch_gemm_bias2(A1, A2, W, bias, addend, COL, nullptr, 0, out, N, K, K1,
                    COL, stream, nullptr, nullptr, 0, nullptr);
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

// GPF > 0: A1 is wh = W_e h + b, and the message half of the A operand is
// its segment sum over the in-edges, formed while it is staged (mfma_tile.h
// TileGather). Column block 0 of each row tile stores the staged sums to
// M[s]; the other 4H/128 - 1 column blocks repeat the gather (about 2.2
// rows per row on the training graphs, L2-resident) and store nothing.
template <int BMT, int GPF = 0>
__global__ __launch_bounds__(256) void gemm_gru_kernel(
    const bf16* __restrict__ A1, const bf16* __restrict__ A2,
    const bf16* __restrict__ Wperm, const bf16* __restrict__ bperm,
    const bf16* __restrict__ h_in, bf16* __restrict__ h_new,
    bf16* __restrict__ R, bf16* __restrict__ Z, bf16* __restrict__ Nn,
    bf16* __restrict__ HN, int N, int K, int K1, int H, TileGather g) {
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
  if (blockIdx.y != 0) g.out = nullptr;
  tile_regstaged_gemm<BMT, false, GPF>(acc, smem, A1, A2, K1, Wperm, N, K,
                                          4 * H, r0, c0, g);

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
                     hipStream_t stream, const int* g_indptr,
                     const int* g_indices, bf16* g_out) {
  const int COL = 4 * H;
  const bool g = g_indptr != nullptr;
  const TileGather tg = {g_indptr, g_indices, (long)K1, g_out};
  const long blocks64 = (long)((N + BM - 1) / BM) * (COL / BN);
  // tests/test_gpu_ggnn.py: test_fused_fwd_teacher_forced[small-128-3] takes
  // the 32-row tile, [n24577-128-1] and [n6081-128-2] the 64-row tile
  if (blocks64 < 384) {
    const dim3 grid((N + 31) / 32, COL / BN);
    const size_t lds = gru_lds_bytes(32);
    if (g)
      hipLaunchKernelGGL((gemm_gru_kernel<32, gather_gpf(32)>), grid, dim3(256), lds,
                         stream, A1, A2, Wperm, bperm, h_in, h_new, R, Z, Nn,
                         HN, N, K, K1, H, tg);
    else
      hipLaunchKernelGGL(gemm_gru_kernel<32>, grid, dim3(256), lds, stream, A1,
                         A2, Wperm, bperm, h_in, h_new, R, Z, Nn, HN, N, K, K1,
                         H, tg);
  } else {
    const dim3 grid((N + BM - 1) / BM, COL / BN);
    const size_t lds = gru_lds_bytes(BM);
    if (g)
      hipLaunchKernelGGL((gemm_gru_kernel<BM, gather_gpf(BM)>), grid, dim3(256), lds,
                         stream, A1, A2, Wperm, bperm, h_in, h_new, R, Z, Nn,
                         HN, N, K, K1, H, tg);
    else
      hipLaunchKernelGGL(gemm_gru_kernel<BM>, grid, dim3(256), lds, stream, A1,
                         A2, Wperm, bperm, h_in, h_new, R, Z, Nn, HN, N, K, K1,
                         H, tg);
  }
}

// ---------------------------------------------------------------------------
// Gate backward + grad_A GEMM in one launch (GGNN backward, per step):
//   ggic = gru_gates2_bwd(grad_h, h_in, R, Z, Nn, HN)        (N, 4H)
//   grad_A = ggic @ WcatT^T                                   (N, 2H)
// Structure of node_head.hip: a prologue computes the block's whole
// (BMT, 4H) ggic tile from the six (N, H) inputs and writes it ONCE to LDS in
// the swizzled A-operand layout (NSL = 4H/64 k-slices of BMT x 128 B); the K
// loop then streams only the WcatT slices (register-staged, double-buffered
// in LDS, GG_PF slices ahead in registers: one MFMA k-step hides a small
// part of a slice's load latency, and LDS, not registers, bounds the blocks
// per CU here) and runs the shared k-step in K order 0..4H, so the accumulators see the
// sequence gemm_bias_kernel sees reading a stored ggic. The gate arithmetic
// is gru_gate2_bwd_elem, the function gru_gates2_bwd_kernel compiles.
//
// grid = (ceil(N/BMT), 2H/128): every column block repeats the prologue, and
// column block 0 also stores ggic and grad_hd for the batched weight-grad.
// Chosen over one block looping over the column tiles with the A tile
// resident: the parent GEMM is latency-bound with 2 x 360 blocks on 256 CUs
// at the training shape, the loop form would halve the block count to 1.4
// per CU and run two K = 4H passes back to back in each, while the repeated
// prologue costs one more L2-resident read of the six inputs (1.5 KiB per
// row). The loop form was not measured.
//
// LDS (static): BMT * 4H * 2 B for the tile + two 128-row W slices (32 KiB):
// 64 KiB at BMT = 32, H = 128; 128 KiB at BMT = 64, H = 192.
// ---------------------------------------------------------------------------

#include "gru_gate_bwd.h"

#define GG_WBUF (TILE_BN * TILE_ROWB)  // one W slice: 128 rows = 16 KiB
#define GG_PF 3                        // W slices in flight in registers

template <int BMT, int NSL>
__global__ __launch_bounds__(256) void gates_gemm_kernel(
    const bf16* __restrict__ grad_h, const bf16* __restrict__ h_in,
    const bf16* __restrict__ R, const bf16* __restrict__ Z,
    const bf16* __restrict__ Nn, const bf16* __restrict__ HN,
    const bf16* __restrict__ WcatT, bf16* __restrict__ ggic_out,
    bf16* __restrict__ grad_hd, bf16* __restrict__ grad_A, int N) {
  constexpr int H = NSL * 16;        // 4H = NSL * 64
  constexpr int K = 4 * H;
  constexpr int COL = 2 * H;
  constexpr int HC = H / 8;          // 16-B chunks per (N, H) row
  constexpr int SPG = NSL / 4;       // k-slices per gate
  __shared__ __attribute__((aligned(16))) char smem[BMT * NSL * TILE_ROWB + 2 * GG_WBUF];
  char* act = smem;
  char* wbuf = smem + BMT * NSL * TILE_ROWB;

  const int r0 = blockIdx.x * BMT;
  const int c0 = blockIdx.y * BN;
  const int tid = threadIdx.x;
  const int lane = tid & (WAVE - 1);
  const int wid = tid >> 6;
  const int wm = wid >> 1;
  const int wn = wid & 1;
  const bool save = blockIdx.y == 0;

  // W slices t = 0 .. GG_PF-1 are requested up front; register set t % GG_PF
  // holds slice t until it is stored to LDS, then takes slice t + GG_PF
  uint4v wr[GG_PF][4];
#pragma unroll
  for (int t = 0; t < GG_PF; ++t)
    tile_w_load<4>(WcatT, K, c0, t * TILE_BK, COL, tid, wr[t]);

  // prologue: item = (row, 16-B chunk c of the H columns); its four gate
  // chunks land in k-slices g * SPG + c / 8 at chunk c % 8
  constexpr int NIT = BMT * HC / 256;
  static_assert(BMT * HC % 256 == 0, "whole items per thread");
#pragma unroll
  for (int q = 0; q < NIT; ++q) {
    const int it = tid + q * 256;
    const int row = it / HC;
    const int c = it % HC;
    const int gr = r0 + row;
    tile_pack8 o[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) o[g].v = uint4v{0u, 0u, 0u, 0u};
    if (gr < N) {
      const long off = (long)gr * H + c * 8;
      tile_pack8 go, hv, r, z, n, hn, hd;
      go.v = *reinterpret_cast<const uint4v*>(grad_h + off);
      hv.v = *reinterpret_cast<const uint4v*>(h_in + off);
      r.v = *reinterpret_cast<const uint4v*>(R + off);
      z.v = *reinterpret_cast<const uint4v*>(Z + off);
      n.v = *reinterpret_cast<const uint4v*>(Nn + off);
      hn.v = *reinterpret_cast<const uint4v*>(HN + off);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const GruGate2Grad d = gru_gate2_bwd_elem(
            __bfloat162float(go.e[j]), __bfloat162float(hv.e[j]),
            __bfloat162float(r.e[j]), __bfloat162float(z.e[j]),
            __bfloat162float(n.e[j]), __bfloat162float(hn.e[j]));
        o[0].e[j] = __float2bfloat16(d.dpr);
        o[1].e[j] = __float2bfloat16(d.dpz);
        o[2].e[j] = __float2bfloat16(d.dpn);
        o[3].e[j] = __float2bfloat16(d.dpnr);
        hd.e[j] = __float2bfloat16(d.ghd);
      }
      if (save) {
#pragma unroll
        for (int g = 0; g < 4; ++g)
          *reinterpret_cast<uint4v*>(ggic_out + (long)gr * K + g * H + c * 8) = o[g].v;
        *reinterpret_cast<uint4v*>(grad_hd + off) = hd.v;
      }
    }
#pragma unroll
    for (int g = 0; g < 4; ++g)
      *reinterpret_cast<uint4v*>(act + (g * SPG + (c >> 3)) * BMT * TILE_ROWB +
                                 tile_swz(row, (c & 7) * 16)) = o[g].v;
  }
  tile_regs_store<4>(wbuf, tid, wr[0]);
  if (GG_PF < NSL) tile_w_load<4>(WcatT, K, c0, GG_PF * TILE_BK, COL, tid, wr[0]);
  __syncthreads();

  constexpr int MFRAG = BMT / 32;
  f32x4 acc[MFRAG][4] = {};
#pragma unroll
  for (int s = 0; s < NSL; ++s) {
    const int cur = s & 1;
    tile_kstep<false>(acc, act + s * BMT * TILE_ROWB, wm * (BMT / 2),
                      wbuf + cur * GG_WBUF, wn * 64, lane);
    if (s + 1 < NSL)
      tile_regs_store<4>(wbuf + (cur ^ 1) * GG_WBUF, tid, wr[(s + 1) % GG_PF]);
    if (s + 1 + GG_PF < NSL)
      tile_w_load<4>(WcatT, K, c0, (s + 1 + GG_PF) * TILE_BK, COL, tid,
                     wr[(s + 1) % GG_PF]);
    __syncthreads();
  }
  gemm_bias_epilogue<BMT, false>(acc, nullptr, nullptr, 0, nullptr, 0, grad_A,
                                 N, COL, r0, c0, lane, wm, wn);
}

template <int BMT, int NSL>
static void gates_gemm_launch(const bf16* grad_h, const bf16* h_in,
                              const bf16* R, const bf16* Z, const bf16* Nn,
                              const bf16* HN, const bf16* WcatT, bf16* ggic,
                              bf16* grad_hd, bf16* grad_A, int N,
                              hipStream_t stream) {
  const dim3 grid((N + BMT - 1) / BMT, NSL * 32 / BN);
  hipLaunchKernelGGL((gates_gemm_kernel<BMT, NSL>), grid, dim3(256), 0, stream,
                     grad_h, h_in, R, Z, Nn, HN, WcatT, ggic, grad_hd, grad_A,
                     N);
}

// Returns false, launching nothing, where no instantiation covers H (the
// tile is compiled for H = 64, 128, 192; from H = 256 on, the 64-row tile
// plus the W buffers reaches the 160 KiB of LDS): the caller then runs
// gru_gates2_bwd + gemm_bias. Row tile by launch_gemm_bias2's rule.
bool launch_gates_gemm(const bf16* grad_h, const bf16* h_in, const bf16* R,
                       const bf16* Z, const bf16* Nn, const bf16* HN,
                       const bf16* WcatT, bf16* ggic, bf16* grad_hd,
                       bf16* grad_A, int N, int H, hipStream_t stream) {
  if (H != 64 && H != 128 && H != 192) return false;
  if (N <= 0) return true;
  const long blocks64 = (long)((N + BM - 1) / BM) * (2 * H / BN);
  const bool small = blocks64 < 384;
#define GG_CASE(h)                                                            \
  if (H == h) {                                                               \
    if (small)                                                                \
      gates_gemm_launch<32, h / 16>(grad_h, h_in, R, Z, Nn, HN, WcatT, ggic,  \
                                    grad_hd, grad_A, N, stream);              \
    else                                                                      \
      gates_gemm_launch<BM, h / 16>(grad_h, h_in, R, Z, Nn, HN, WcatT, ggic,  \
                                    grad_hd, grad_A, N, stream);              \
  }
  GG_CASE(64)
  GG_CASE(128)
  GG_CASE(192)
#undef GG_CASE
  return true;
}
