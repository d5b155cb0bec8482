// Fused node-level head for the flow-GNN on MI355X (gfx950): the 3-layer
// MLP over every node, one launch per direction.
//
//   fwd: logits[n] = w3 . relu(W2 relu(W1 [h[n]|fe[n]] + b1) + b2) + b3
//   bwd: dH2 = (dlogits x w3) * (H2 > 0)
//        dH1 = (dH2 W2) * (H1 > 0)
//        [dh|dfe] = dH1 W1           (+ dW3 += H2^T dlogits, db3 += sum)
//
// Geometry is fixed: h, fe are (N,128), every hidden width is 256. Tile
// conventions follow gemm_bias.hip: 256-thread blocks, BK = 64 slices,
// v_mfma_f32_16x16x32_bf16, XOR-swizzled LDS rows (tile_swz),
// register-staged double-buffered weight slices; the swizzle, the k-step and
// the weight-slice staging come from mfma_tile.h. A block owns BMT rows x
// all 256 columns (4 column-waves of 64 columns), so a layer's bias+ReLU'd
// output tile can be written back to LDS as the next layer's A operand; the (N,256)
// concatenation and the inter-layer activations never round-trip through
// HBM on the forward's critical path. The two layers' eight weight slices
// are streamed as ONE pipeline: the last slice of a layer prefetches the
// first slice of the next.
//
// LDS: activation tile BMT x 256 bf16 (4 k-slices of BMT x 128 B) plus two
// 256 x 128 B weight-slice buffers = 96 KiB (BMT=64) / 80 KiB (BMT=32),
// one static array.

#include <hip/hip_runtime.h>

#include "mfma_tile.h"

#define NH_D 256                  // hidden width (= 2 x 128 inputs)
#define NH_DH 128                 // width of each input half
#define NH_BK TILE_BK
#define NH_ROWB TILE_ROWB         // bytes per LDS row (64 bf16)
#define NH_WBUF (NH_D * NH_ROWB)  // one weight slice: 256 rows = 32 KiB
#define NH_NSL (NH_D / NH_BK)     // k-slices per layer

union nh_pack8 {
  uint4v v;
  bf16 e[8];
};

// weight-slice staging (mfma_tile.h register staging, 8 row groups): the
// 256 rows of W[:, kk:kk+64], W in (out, in) layout with NH_D columns
__device__ __forceinline__ void nh_w_load(const bf16* __restrict__ W, int kk,
                                          int tid, uint4v r[8]) {
  tile_w_load<8>(W, NH_D, 0, kk, NH_D, tid, r);
}

// acc(BMT x 64 per wave) = act(BMT x 256) @ W(256 x 256)^T, W in
// (out, in) layout. Precondition: W's slice 0 sits in wbuf[cur] and the
// act tile is visible (barrier passed). On return every wave is past the
// last barrier, wbuf[cur] holds Wnext's slice 0 (when Wnext != nullptr)
// and the act tile may be overwritten.
template <int BMT>
__device__ __forceinline__ void nh_layer_gemm(
    f32x4 (&acc)[BMT / 16][4], const char* act, char* wbuf, int& cur,
    const bf16* __restrict__ W, const bf16* __restrict__ Wnext, int tid,
    int lane, int wn) {
  constexpr int MF = BMT / 16;
#pragma unroll
  for (int m = 0; m < MF; ++m)
#pragma unroll
    for (int n = 0; n < 4; ++n) acc[m][n] = f32x4{0.f, 0.f, 0.f, 0.f};
  uint4v wr[8];
#pragma unroll
  for (int s = 0; s < NH_NSL; ++s) {
    const bf16* Wp = (s + 1 < NH_NSL) ? W : Wnext;
    const int kn = (s + 1 < NH_NSL) ? (s + 1) * NH_BK : 0;
    if (Wp) nh_w_load(Wp, kn, tid, wr);
    const char* a_s = act + s * BMT * NH_ROWB;
    const char* b_s = wbuf + cur * NH_WBUF;
    tile_kstep<false>(acc, a_s, 0, b_s, wn * 64, lane);
    if (Wp) tile_regs_store<8>(wbuf + (cur ^ 1) * NH_WBUF, tid, wr);
    __syncthreads();
    cur ^= 1;
  }
}

// accumulators -> bf16 act tile in the swizzled A-operand layout.
// D mapping: col = lane&15, row = (lane>>4)*4 + i; this wave's 64 columns
// are exactly k-slice `wn` of the next layer's A operand.
template <int BMT>
__device__ __forceinline__ void nh_acc_to_act(const f32x4 (&acc)[BMT / 16][4],
                                              char* act, int lane, int wn) {
  char* a_s = act + wn * BMT * NH_ROWB;
#pragma unroll
  for (int m = 0; m < BMT / 16; ++m)
#pragma unroll
    for (int n = 0; n < 4; ++n) {
      const int byte = (n * 16 + (lane & 15)) * 2;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int row = m * 16 + (lane >> 4) * 4 + i;
        *reinterpret_cast<bf16*>(a_s + tile_swz(row, byte)) =
            __float2bfloat16(acc[m][n][i]);
      }
    }
}

// act tile -> global, 16 B per thread per step, rows >= N skipped.
// out2 == nullptr: one (N,256) tensor; else columns [0,128) go to out1
// and [128,256) to out2, both (N,128).
template <int BMT>
__device__ __forceinline__ void nh_act_to_global(const char* act,
                                                 bf16* __restrict__ out1,
                                                 bf16* __restrict__ out2,
                                                 int r0, int N, int tid) {
  for (int it = tid; it < BMT * 32; it += 256) {
    const int row = it >> 5;
    const int c = it & 31;
    const int gr = r0 + row;
    if (gr >= N) continue;
    const uint4v v = *reinterpret_cast<const uint4v*>(
        act + (c >> 3) * BMT * NH_ROWB + tile_swz(row, (c & 7) * 16));
    bf16* dst;
    if (out2 == nullptr)
      dst = out1 + (long)gr * NH_D + c * 8;
    else
      dst = (c < 16) ? out1 + (long)gr * NH_DH + c * 8
                     : out2 + (long)gr * NH_DH + (c - 16) * 8;
    *reinterpret_cast<uint4v*>(dst) = v;
  }
}

template <int BMT>
__global__ __launch_bounds__(256) void node_head_fwd_kernel(
    const bf16* __restrict__ h, const bf16* __restrict__ fe,
    const bf16* __restrict__ W1, const bf16* __restrict__ W2,
    const float* __restrict__ b1, const float* __restrict__ b2,
    const float* __restrict__ w3, const float* __restrict__ b3,
    float* __restrict__ logits, bf16* __restrict__ X, bf16* __restrict__ H1,
    bf16* __restrict__ H2, int N, int save) {
  __shared__ __attribute__((aligned(16))) char smem[BMT * NH_D * 2 + 2 * NH_WBUF];
  char* act = smem;
  char* wbuf = smem + BMT * NH_D * 2;
  constexpr int MF = BMT / 16;

  const int r0 = blockIdx.x * BMT;
  const int tid = threadIdx.x;
  const int lane = tid & (WAVE - 1);
  const int wn = tid >> 6;  // 4 column-waves of 64 columns, all BMT rows

  // prologue: W1 slice 0 and the whole [h|fe] tile (split-A: columns
  // < 128 from h, the rest from fe); rows >= N are zero-filled
  uint4v wr[8];
  nh_w_load(W1, 0, tid, wr);
  for (int it = tid; it < BMT * 32; it += 256) {
    const int row = it >> 5;
    const int c = it & 31;
    const int gr = r0 + row;
    uint4v v = {};
    if (gr < N) {
      const bf16* src = (c < 16) ? h + (long)gr * NH_DH + c * 8
                                 : fe + (long)gr * NH_DH + (c - 16) * 8;
      v = *reinterpret_cast<const uint4v*>(src);
      // the dW1 wgrad wants a contiguous (N,256) B operand
      if (save) *reinterpret_cast<uint4v*>(X + (long)gr * NH_D + c * 8) = v;
    }
    *reinterpret_cast<uint4v*>(act + (c >> 3) * BMT * NH_ROWB +
                               tile_swz(row, (c & 7) * 16)) = v;
  }
  tile_regs_store<8>(wbuf, tid, wr);
  __syncthreads();

  int cur = 0;
  f32x4 acc[MF][4];

  // layer 1
  nh_layer_gemm<BMT>(acc, act, wbuf, cur, W1, W2, tid, lane, wn);
#pragma unroll
  for (int n = 0; n < 4; ++n) {
    const float b = b1[wn * 64 + n * 16 + (lane & 15)];
#pragma unroll
    for (int m = 0; m < MF; ++m)
#pragma unroll
      for (int i = 0; i < 4; ++i) acc[m][n][i] = fmaxf(acc[m][n][i] + b, 0.f);
  }
  nh_acc_to_act<BMT>(acc, act, lane, wn);
  __syncthreads();
  if (save) nh_act_to_global<BMT>(act, H1, nullptr, r0, N, tid);

  // layer 2
  nh_layer_gemm<BMT>(acc, act, wbuf, cur, W2, nullptr, tid, lane, wn);

  // layer 3 straight from the fp32 accumulators: per-lane partial over
  // this lane's 4 columns, then the 16 column lanes, then the 4 waves
  float* red = reinterpret_cast<float*>(wbuf);  // weight buffers are idle now
  float bb[4], ww[4];
#pragma unroll
  for (int n = 0; n < 4; ++n) {
    const int col = wn * 64 + n * 16 + (lane & 15);
    bb[n] = b2[col];
    ww[n] = w3[col];
  }
#pragma unroll
  for (int m = 0; m < MF; ++m)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float p = 0.f;
#pragma unroll
      for (int n = 0; n < 4; ++n) {
        const float v = fmaxf(acc[m][n][i] + bb[n], 0.f);
        acc[m][n][i] = v;
        p += v * ww[n];
      }
      p += __shfl_xor(p, 1);
      p += __shfl_xor(p, 2);
      p += __shfl_xor(p, 4);
      p += __shfl_xor(p, 8);
      if ((lane & 15) == 0) red[wn * BMT + m * 16 + (lane >> 4) * 4 + i] = p;
    }
  if (save) nh_acc_to_act<BMT>(acc, act, lane, wn);
  __syncthreads();
  if (tid < BMT && r0 + tid < N)
    logits[r0 + tid] = ((red[tid] + red[BMT + tid]) +
                        (red[2 * BMT + tid] + red[3 * BMT + tid])) + b3[0];
  if (save) nh_act_to_global<BMT>(act, H2, nullptr, r0, N, tid);
}

// W2T, W1T: the (in, out)-major transposes, i.e. W2T[j][k] = W2[k][j], so
// the forward's B-operand path serves the dgrad products unchanged.
template <int BMT>
__global__ __launch_bounds__(256) void node_head_bwd_kernel(
    const float* __restrict__ dlogits, const bf16* __restrict__ H1,
    const bf16* __restrict__ H2, const bf16* __restrict__ W2T,
    const bf16* __restrict__ W1T, const float* __restrict__ w3,
    bf16* __restrict__ dH1, bf16* __restrict__ dH2, bf16* __restrict__ dh,
    bf16* __restrict__ dfe, float* __restrict__ dW3, float* __restrict__ db3,
    int N) {
  __shared__ __attribute__((aligned(16))) char smem[BMT * NH_D * 2 + 2 * NH_WBUF];
  char* act = smem;
  char* wbuf = smem + BMT * NH_D * 2;
  constexpr int MF = BMT / 16;

  const int r0 = blockIdx.x * BMT;
  const int tid = threadIdx.x;
  const int lane = tid & (WAVE - 1);
  const int wn = tid >> 6;

  uint4v wr[8];
  nh_w_load(W2T, 0, tid, wr);

  // prologue: dH2 tile = (dlogits x w3) * (H2 > 0) -> LDS (A operand of
  // the first dgrad) and global (the dW2 / db2 operand); the same pass
  // accumulates this block's dW3 partials, 8 columns per thread
  {
    const int c = tid & 31;   // 16-B column chunk
    const int rg = tid >> 5;  // row group: rows rg + 8p
    float w3v[8], dw[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      w3v[j] = w3[c * 8 + j];
      dw[j] = 0.f;
    }
#pragma unroll
    for (int p = 0; p < BMT / 8; ++p) {
      const int row = rg + p * 8;
      const int gr = r0 + row;
      nh_pack8 o;
      o.v = uint4v{0u, 0u, 0u, 0u};
      if (gr < N) {
        const float dl = dlogits[gr];
        nh_pack8 hv;
        hv.v = *reinterpret_cast<const uint4v*>(H2 + (long)gr * NH_D + c * 8);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float hf = __bfloat162float(hv.e[j]);
          o.e[j] = __float2bfloat16(hf > 0.f ? dl * w3v[j] : 0.f);
          dw[j] += dl * hf;
        }
        *reinterpret_cast<uint4v*>(dH2 + (long)gr * NH_D + c * 8) = o.v;
      }
      *reinterpret_cast<uint4v*>(act + (c >> 3) * BMT * NH_ROWB +
                                 tile_swz(row, (c & 7) * 16)) = o.v;
    }
    // weight buffer 1 is idle until the first slice's prefetch lands in it
    float* scr = reinterpret_cast<float*>(wbuf + NH_WBUF);
#pragma unroll
    for (int j = 0; j < 8; ++j) scr[rg * NH_D + c * 8 + j] = dw[j];
    tile_regs_store<8>(wbuf, tid, wr);
    __syncthreads();
    float s = 0.f;
#pragma unroll
    for (int g = 0; g < 8; ++g) s += scr[g * NH_D + tid];
    // accumulate: dW3 / db3 may be live .grad views holding an earlier
    // micro-batch's contribution
    atomicAdd(dW3 + tid, s);
    if (tid < WAVE) {
      float v = (tid < BMT && r0 + tid < N) ? dlogits[r0 + tid] : 0.f;
#pragma unroll
      for (int off = WAVE / 2; off > 0; off >>= 1) v += __shfl_xor(v, off);
      if (tid == 0) atomicAdd(db3, v);
    }
    __syncthreads();  // scr reads finish before slice 1 overwrites it
  }

  int cur = 0;
  f32x4 acc[MF][4];

  // dH1 = (dH2 @ W2) * (H1 > 0). The H1 values behind this lane's
  // accumulator elements are loaded up front, unconditionally (row index
  // clamped: rows >= N have a zero dH2 row, so their accumulators are zero
  // whatever the mask says), so the loads fly under the GEMM instead of
  // serialising behind per-element branches in the epilogue.
  float h1v[MF][4][4];
#pragma unroll
  for (int m = 0; m < MF; ++m)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int gr = min(r0 + m * 16 + (lane >> 4) * 4 + i, N - 1);
#pragma unroll
      for (int n = 0; n < 4; ++n)
        h1v[m][n][i] = __bfloat162float(
            H1[(long)gr * NH_D + wn * 64 + n * 16 + (lane & 15)]);
    }
  nh_layer_gemm<BMT>(acc, act, wbuf, cur, W2T, W1T, tid, lane, wn);
#pragma unroll
  for (int m = 0; m < MF; ++m)
#pragma unroll
    for (int n = 0; n < 4; ++n)
#pragma unroll
      for (int i = 0; i < 4; ++i)
        acc[m][n][i] = h1v[m][n][i] > 0.f ? acc[m][n][i] : 0.f;
  nh_acc_to_act<BMT>(acc, act, lane, wn);
  __syncthreads();
  nh_act_to_global<BMT>(act, dH1, nullptr, r0, N, tid);

  // [dh | dfe] = dH1 @ W1, written as the split directly
  nh_layer_gemm<BMT>(acc, act, wbuf, cur, W1T, nullptr, tid, lane, wn);
  nh_acc_to_act<BMT>(acc, act, lane, wn);
  __syncthreads();
  nh_act_to_global<BMT>(act, dh, dfe, r0, N, tid);
}

// 64-row tiles normally; 32-row tiles while the 64-row grid would leave
// some of the 256 CUs without a block (N < 16384, which covers the
// ~12k-node training batches). tile = 32 / 64 forces a geometry (tests,
// tools/bench_node_head.py); 0 = this rule.
int node_head_tile_rows(int N, int tile) {
  if (tile == 32 || tile == 64) return tile;
  return ((N + 63) / 64 < 256) ? 32 : 64;
}

void launch_node_head_fwd(const bf16* h, const bf16* fe, const bf16* W1,
                          const bf16* W2, const float* b1, const float* b2,
                          const float* w3, const float* b3, float* logits,
                          bf16* X, bf16* H1, bf16* H2, int N, int save,
                          int tile, hipStream_t stream) {
  if (N <= 0) return;
  if (node_head_tile_rows(N, tile) == 32)
    hipLaunchKernelGGL(node_head_fwd_kernel<32>, dim3((N + 31) / 32), dim3(256),
                       0, stream, h, fe, W1, W2, b1, b2, w3, b3, logits, X, H1,
                       H2, N, save);
  else
    hipLaunchKernelGGL(node_head_fwd_kernel<64>, dim3((N + 63) / 64), dim3(256),
                       0, stream, h, fe, W1, W2, b1, b2, w3, b3, logits, X, H1,
                       H2, N, save);
}

void launch_node_head_bwd(const float* dlogits, const bf16* H1, const bf16* H2,
                          const bf16* W2T, const bf16* W1T, const float* w3,
                          bf16* dH1, bf16* dH2, bf16* dh, bf16* dfe, float* dW3,
                          float* db3, int N, int tile, hipStream_t stream) {
  if (N <= 0) return;
  if (node_head_tile_rows(N, tile) == 32)
    hipLaunchKernelGGL(node_head_bwd_kernel<32>, dim3((N + 31) / 32), dim3(256),
                       0, stream, dlogits, H1, H2, W2T, W1T, w3, dH1, dH2, dh,
                       dfe, dW3, db3, N);
  else
    hipLaunchKernelGGL(node_head_bwd_kernel<64>, dim3((N + 63) / 64), dim3(256),
                       0, stream, dlogits, H1, H2, W2T, W1T, w3, dH1, dH2, dh,
                       dfe, dW3, db3, N);
}
