// Graph-level flow-GNN head for MI355X (gfx950, CDNA4). Native HIP.
//
//   concat([ggnn_out, feat_embed]) -> gate linear -> segment-softmax
//   attention pool -> [256->256 relu] x2 -> 256->1 logit
//
// at batch ~256 graphs / ~11.5k nodes. Weights are read as fp32 master
// values and every accumulation is fp32: the MLP products run on the exact
// f32-input MFMA (v_mfma_f32_16x16x4_f32, a k-ordered fmaf chain), never a
// bf16 shortcut, so results equal the scalar kernels these replace up to
// fp32 summation order and every reduction order is fixed (run-to-run
// reproducible; only the dwg/dbg float atomics of the pool backward
// commute freely, as before).
//
// MFMA 16x16x4 f32 lane maps (lane l, c = l & 15, q = l >> 4):
//   A[i = c][k = q]   B[k = q][j = c]   C/D[row = 4q + reg][col = c]
// A k-step may use ANY four k values as long as A and B agree per lane, so
// a lane that holds four consecutive k (one 16-B load) feeds four k-steps:
// step s of group g uses k = 16g + 4q + s.
//
// Kernels (VGPR / LDS bytes per block from hipcc
// -Rpass-analysis=kernel-resource-usage on gfx950; scratch is 0 in all):
//   mlp3_fwd_kernel      512 thr  158 VGPR  33792 B  16 rows x 256 cols per
//                        block, 8 waves x 32 cols
//   mlp3_bwd_kernel      512 thr  199 VGPR  33280 B  same tiling, B operand
//                        read along W's 2nd index
//   mlp3_wgrad_kernel    256 thr   80 VGPR   6144 B  one 16x32 dW tile per
//                        block, K = B split over 4 waves (+8 AGPR)
//   gate_pool_fwd_kernel 256 thr   67 VGPR  34056 B  one 64-node chunk
//   gate_pool_combine_kernel 256 thr 25 VGPR    0 B  one graph
//   gate_pool_bwd_kernel 256 thr  154 VGPR   8224 B  one 64-node chunk
//
// MLP weight staging: every wave owns its own 32 output columns, so a weight
// element is used by exactly one wave of a block — there is nothing for LDS
// to share. The B fragments go global -> VGPR as whole 128-column halves of
// a layer (64 VGPRs), two halves in flight, the next layer's halves issued
// while the current ones feed the MFMAs: no wave waits on a chain of
// dependent loads, and no LDS bank question arises for B. The A operand
// (the 16-row activation tile, shared by all 8 waves) lives in LDS with
// rows padded by 4 floats so the ds_read_b128 fragment reads of 16 rows
// land on 16 different 16-B slots.
//
// Pool partitioning (scheme 1 of the two the design allows): blocks take
// FIXED 64-node chunks [64c, 64c+64) of the batch's node array, so no graph
// size can set the kernel's duration. Rows are read once with 16-B loads
// (gate dot taken from the registers on the way into LDS), the segment
// softmax of every graph piece inside the chunk is one wave's segmented
// shuffle scan, and the weighted sums run from LDS. A graph that lies
// inside one chunk is finished there. A graph cut by a chunk boundary
// leaves one online-softmax partial (max, sum, weighted vector) per chunk;
// gate_pool_combine_kernel (one block per graph, a no-op for whole graphs)
// merges the partials, rescales that graph's alpha and zero-fills the rows
// of empty graphs. The forward also keeps the un-rounded fp32 pooled row:
// the backward's per-graph scalar sum_v alpha_v <go, x_v> equals
// <go, pooled_fp32>, which makes the backward one chunk-parallel pass that
// reads every node row exactly once, whatever the graph sizes.

#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>

#include <cstdint>

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
// parameters and their .grad buffers may be views into a flat fp32 buffer at
// any element offset: vector accesses to them promise 4-byte alignment only
typedef f32x4 __attribute__((aligned(4))) f32x4u;
typedef f32x2 __attribute__((aligned(4))) f32x2u;

constexpr int HD = 256;        // head width (128 + 128 concat)
constexpr int LDA = HD + 4;    // padded LDS row of the A tile (floats)
constexpr int TR = 16;         // rows per MLP block (one MFMA M tile)

__device__ __forceinline__ float bf_lo(uint32_t u) { return __uint_as_float(u << 16); }
__device__ __forceinline__ float bf_hi(uint32_t u) { return __uint_as_float(u & 0xffff0000u); }
__device__ __forceinline__ uint32_t f2bf(float v) {
  const __hip_bfloat16 b = __float2bfloat16(v);
  return (uint32_t)(*reinterpret_cast<const unsigned short*>(&b));
}
__device__ __forceinline__ uint32_t pack_bf2(float a, float b) {
  return f2bf(a) | (f2bf(b) << 16);
}
// 8 bf16 (one 16-B load) -> 8 floats
__device__ __forceinline__ void unpack8(const uint4& u, float (&f)[8]) {
  f[0] = bf_lo(u.x); f[1] = bf_hi(u.x); f[2] = bf_lo(u.y); f[3] = bf_hi(u.y);
  f[4] = bf_lo(u.z); f[5] = bf_hi(u.z); f[6] = bf_lo(u.w); f[7] = bf_hi(u.w);
}

#define MFMA_F32(a, b, c) __builtin_amdgcn_mfma_f32_16x16x4f32((a), (b), (c), 0, 0, 0)

// ---------------------------------------------------------------------------
// MLP forward: B fragment of x @ W^T is W[(out) n][(in) k], contiguous in k.
// ---------------------------------------------------------------------------

// one 128-wide K half of a layer for this wave's two 16-column tiles
__device__ __forceinline__ void load_w_fwd(const float* __restrict__ W, int half,
                                           int ncol0, int c, int q,
                                           f32x4 (&w)[2][8]) {
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int g = 0; g < 8; ++g)
      w[t][g] = *reinterpret_cast<const f32x4u*>(
          W + (size_t)(ncol0 + t * 16 + c) * HD + half * 128 + g * 16 + 4 * q);
}

__device__ __forceinline__ void mma_fwd(const float* __restrict__ as, int half, int c,
                                        int q, const f32x4 (&w)[2][8],
                                        f32x4 (&acc)[2]) {
#pragma unroll
  for (int g = 0; g < 8; ++g) {
    const f32x4 a =
        *reinterpret_cast<const f32x4*>(as + c * LDA + half * 128 + g * 16 + 4 * q);
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      acc[0] = MFMA_F32(a[s], w[0][g][s], acc[0]);
      acc[1] = MFMA_F32(a[s], w[1][g][s], acc[1]);
    }
  }
}

__global__ __launch_bounds__(512) void mlp3_fwd_kernel(
    const __hip_bfloat16* __restrict__ x, const float* __restrict__ W1,
    const float* __restrict__ b1, const float* __restrict__ W2,
    const float* __restrict__ b2, const float* __restrict__ W3,
    const float* __restrict__ b3, float* __restrict__ h1, float* __restrict__ h2,
    float* __restrict__ logits, int B) {
  __shared__ __attribute__((aligned(16))) float sm[2 * TR * LDA + 8 * TR];
  float* xs = sm;
  float* hs = sm + TR * LDA;
  float* red = hs + TR * LDA;
  const int tid = threadIdx.x, wid = tid >> 6, lane = tid & 63;
  const int c = lane & 15, q = lane >> 4;
  const int r0 = blockIdx.x * TR;
  const int ncol0 = wid * 32;

  f32x4 wa[2][8], wb[2][8];
  load_w_fwd(W1, 0, ncol0, c, q, wa);
  load_w_fwd(W1, 1, ncol0, c, q, wb);
  {  // x tile -> fp32 LDS; rows past B become zeros (clamped address)
    const int row = tid >> 5, seg = tid & 31;
    const int gr = r0 + row;
    const uint4 u = *reinterpret_cast<const uint4*>(
        x + (size_t)(gr < B ? gr : B - 1) * HD + seg * 8);
    float f[8];
    unpack8(u, f);
    const float keep = gr < B ? 1.f : 0.f;
    f32x4 lo = {f[0] * keep, f[1] * keep, f[2] * keep, f[3] * keep};
    f32x4 hi = {f[4] * keep, f[5] * keep, f[6] * keep, f[7] * keep};
    *reinterpret_cast<f32x4*>(xs + row * LDA + seg * 8) = lo;
    *reinterpret_cast<f32x4*>(xs + row * LDA + seg * 8 + 4) = hi;
  }
  __syncthreads();
  f32x4 acc[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
  mma_fwd(xs, 0, c, q, wa, acc);
  load_w_fwd(W2, 0, ncol0, c, q, wa);
  mma_fwd(xs, 1, c, q, wb, acc);
  load_w_fwd(W2, 1, ncol0, c, q, wb);
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const int col = ncol0 + t * 16 + c;
    const float bias = b1[col];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = 4 * q + r;
      const float v = fmaxf(acc[t][r] + bias, 0.f);
      hs[row * LDA + col] = v;
      if (r0 + row < B) h1[(size_t)(r0 + row) * HD + col] = v;
    }
    acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  __syncthreads();
  mma_fwd(hs, 0, c, q, wa, acc);
  mma_fwd(hs, 1, c, q, wb, acc);
  // layer-2 epilogue with the 256->1 GEMV folded in
  float part[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const int col = ncol0 + t * 16 + c;
    const float bias = b2[col], w3 = W3[col];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = 4 * q + r;
      const float v = fmaxf(acc[t][r] + bias, 0.f);
      if (r0 + row < B) h2[(size_t)(r0 + row) * HD + col] = v;
      part[r] += w3 * v;
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
#pragma unroll
    for (int off = 1; off < 16; off <<= 1) part[r] += __shfl_xor(part[r], off);
    if (c == 0) red[wid * TR + 4 * q + r] = part[r];
  }
  __syncthreads();
  if (tid < TR && r0 + tid < B) {
    float z = b3[0];
#pragma unroll
    for (int w = 0; w < 8; ++w) z += red[w * TR + tid];
    logits[r0 + tid] = z;
  }
}

// ---------------------------------------------------------------------------
// MLP backward: dh @ W, B fragment is W[(out) k][(in) n], read along n. A lane
// loads a float2 so 16 lanes cover one full 128-B line of a W row; the wave's
// two column tiles are the even and odd columns of its 32-column slice, which
// also makes every epilogue access a contiguous pair.
// ---------------------------------------------------------------------------

__device__ __forceinline__ void load_w_bwd(const float* __restrict__ W, int half,
                                           int ncol0, int c, int q,
                                           f32x2 (&w)[8][4]) {
#pragma unroll
  for (int g = 0; g < 8; ++g)
#pragma unroll
    for (int s = 0; s < 4; ++s)
      w[g][s] = *reinterpret_cast<const f32x2u*>(
          W + (size_t)(half * 128 + g * 16 + 4 * q + s) * HD + ncol0 + 2 * c);
}

__device__ __forceinline__ void mma_bwd(const float* __restrict__ as, int half, int c,
                                        int q, const f32x2 (&w)[8][4],
                                        f32x4 (&acc)[2]) {
#pragma unroll
  for (int g = 0; g < 8; ++g) {
    const f32x4 a =
        *reinterpret_cast<const f32x4*>(as + c * LDA + half * 128 + g * 16 + 4 * q);
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      acc[0] = MFMA_F32(a[s], w[g][s][0], acc[0]);
      acc[1] = MFMA_F32(a[s], w[g][s][1], acc[1]);
    }
  }
}

__global__ __launch_bounds__(512) void mlp3_bwd_kernel(
    const float* __restrict__ dlogits, const float* __restrict__ h1,
    const float* __restrict__ h2, const float* __restrict__ W1,
    const float* __restrict__ W2, const float* __restrict__ W3,
    float* __restrict__ dh1, float* __restrict__ dh2,
    __hip_bfloat16* __restrict__ dx, int B) {
  __shared__ __attribute__((aligned(16))) float sm[2 * TR * LDA];
  float* as = sm;
  float* bs = sm + TR * LDA;
  const int tid = threadIdx.x, wid = tid >> 6, lane = tid & 63;
  const int c = lane & 15, q = lane >> 4;
  const int r0 = blockIdx.x * TR;
  const int ncol0 = wid * 32;
  const int col0 = ncol0 + 2 * c;  // this lane's column pair

  f32x2 wa[8][4], wb[8][4];
  load_w_bwd(W2, 0, ncol0, c, q, wa);
  load_w_bwd(W2, 1, ncol0, c, q, wb);
  // relu mask of layer 1 for this lane's outputs, fetched ahead of its use
  f32x2 h1v[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int gr = r0 + 4 * q + r;
    h1v[r] = *reinterpret_cast<const f32x2*>(h1 + (size_t)(gr < B ? gr : B - 1) * HD + col0);
  }
  {  // dh2 = (dlogits x w3) * [h2 > 0]: elementwise, written out and staged
    const int row = tid >> 5, seg = tid & 31;
    const int gr = r0 + row;
    const bool ok = gr < B;
    const size_t off = (size_t)(ok ? gr : B - 1) * HD + seg * 8;
    const f32x4 ha = *reinterpret_cast<const f32x4*>(h2 + off);
    const f32x4 hb = *reinterpret_cast<const f32x4*>(h2 + off + 4);
    const f32x4 w3a = *reinterpret_cast<const f32x4u*>(W3 + seg * 8);
    const f32x4 w3b = *reinterpret_cast<const f32x4u*>(W3 + seg * 8 + 4);
    const float dl = ok ? dlogits[gr] : 0.f;
    f32x4 ga, gb;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      ga[j] = (ok && ha[j] > 0.f) ? dl * w3a[j] : 0.f;
      gb[j] = (ok && hb[j] > 0.f) ? dl * w3b[j] : 0.f;
    }
    *reinterpret_cast<f32x4*>(as + row * LDA + seg * 8) = ga;
    *reinterpret_cast<f32x4*>(as + row * LDA + seg * 8 + 4) = gb;
    if (ok) {
      *reinterpret_cast<f32x4*>(dh2 + off) = ga;
      *reinterpret_cast<f32x4*>(dh2 + off + 4) = gb;
    }
  }
  __syncthreads();
  f32x4 acc[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
  mma_bwd(as, 0, c, q, wa, acc);
  load_w_bwd(W1, 0, ncol0, c, q, wa);
  mma_bwd(as, 1, c, q, wb, acc);
  load_w_bwd(W1, 1, ncol0, c, q, wb);
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = 4 * q + r;
    f32x2 g1;
    g1[0] = h1v[r][0] > 0.f ? acc[0][r] : 0.f;
    g1[1] = h1v[r][1] > 0.f ? acc[1][r] : 0.f;
    *reinterpret_cast<f32x2*>(bs + row * LDA + col0) = g1;
    if (r0 + row < B)
      *reinterpret_cast<f32x2*>(dh1 + (size_t)(r0 + row) * HD + col0) = g1;
  }
  acc[0] = f32x4{0.f, 0.f, 0.f, 0.f};
  acc[1] = f32x4{0.f, 0.f, 0.f, 0.f};
  __syncthreads();
  mma_bwd(bs, 0, c, q, wa, acc);
  mma_bwd(bs, 1, c, q, wb, acc);
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = 4 * q + r;
    if (r0 + row < B)
      *reinterpret_cast<uint32_t*>(dx + (size_t)(r0 + row) * HD + col0) =
          pack_bf2(acc[0][r], acc[1][r]);
  }
}

// ---------------------------------------------------------------------------
// MLP weight grads: dW1 = dh1^T x, dW2 = dh2^T h1 as 16(i) x 32(j) f32-MFMA
// tiles over K = B, one tile per block. The block's 4 waves split K in
// 32-row chunks (wave w takes chunks w, w+4, ...), so at B <= 256 every load
// of the launch is issued up front; the four partial tiles meet in LDS in a
// fixed order and ONE lane per element adds the sum into dW. The outputs may
// be live flat .grad views holding an earlier micro-batch, so this is
// always `+=` (a plain read-modify-write: each element has one owner, no
// atomics, deterministic). There is no LDS bound on B. The tail blocks fold
// db1/db2 (column sums), dW3 = dlogits^T h2 and db3 = sum(dlogits).
// ---------------------------------------------------------------------------

constexpr int WG_CH = 32;          // rows per K chunk (8 MFMA k-steps)
constexpr int WG_TILES = 2 * 16 * 8;  // 2 matrices x (256/16) x (256/32)
constexpr int WG_TAIL = 3 * 16;    // 3 column-sum sources x 16 blocks of 16 cols

struct WgChunk {
  float a[8];
  f32x2 b[8];
};

template <bool X_BF16>
__device__ __forceinline__ void wg_load(const float* __restrict__ dh,
                                        const void* __restrict__ src, int rbase,
                                        int B, int i0, int j0, int c, int q,
                                        WgChunk& ch) {
#pragma unroll
  for (int g = 0; g < 8; ++g) {
    const int r = rbase + 4 * g + q;
    const bool ok = r < B;
    const size_t ro = (size_t)(ok ? r : B - 1) * HD;
    const float av = dh[ro + i0 + c];
    f32x2 bv;
    if (X_BF16) {
      const uint32_t u = *reinterpret_cast<const uint32_t*>(
          reinterpret_cast<const __hip_bfloat16*>(src) + ro + j0 + 2 * c);
      bv[0] = bf_lo(u);
      bv[1] = bf_hi(u);
    } else {
      bv = *reinterpret_cast<const f32x2*>(reinterpret_cast<const float*>(src) + ro +
                                           j0 + 2 * c);
    }
    ch.a[g] = ok ? av : 0.f;
    ch.b[g][0] = ok ? bv[0] : 0.f;
    ch.b[g][1] = ok ? bv[1] : 0.f;
  }
}

__device__ __forceinline__ void wg_mma(const WgChunk& ch, f32x4 (&acc)[2]) {
#pragma unroll
  for (int g = 0; g < 8; ++g) {
    acc[0] = MFMA_F32(ch.a[g], ch.b[g][0], acc[0]);
    acc[1] = MFMA_F32(ch.a[g], ch.b[g][1], acc[1]);
  }
}

template <bool X_BF16>
__device__ __forceinline__ void wg_tile(const float* __restrict__ dh,
                                        const void* __restrict__ src, int B, int i0,
                                        int j0, int wid, int c, int q,
                                        f32x4 (&acc)[2]) {
  const int stride = 4 * WG_CH;
  int r = wid * WG_CH;
  if (r >= B) return;
  WgChunk cur, nxt;
  wg_load<X_BF16>(dh, src, r, B, i0, j0, c, q, cur);
  while (true) {
    const int rn = r + stride;
    const bool more = rn < B;
    if (more) wg_load<X_BF16>(dh, src, rn, B, i0, j0, c, q, nxt);
    wg_mma(cur, acc);
    if (!more) break;
    cur = nxt;
    r = rn;
  }
}

__global__ __launch_bounds__(256) void mlp3_wgrad_kernel(
    const __hip_bfloat16* __restrict__ x, const float* __restrict__ h1,
    const float* __restrict__ h2, const float* __restrict__ dh1,
    const float* __restrict__ dh2, const float* __restrict__ dlogits,
    float* __restrict__ dW1, float* __restrict__ dW2, float* __restrict__ dW3,
    float* __restrict__ db1, float* __restrict__ db2, float* __restrict__ db3,
    int B) {
  __shared__ __attribute__((aligned(16))) float red[3 * 64 * 8];
  const int tid = threadIdx.x, wid = tid >> 6, lane = tid & 63;
  if (blockIdx.x < WG_TILES) {
    const int c = lane & 15, q = lane >> 4;
    const int which = blockIdx.x >> 7, rem = blockIdx.x & 127;
    const int i0 = (rem >> 3) * 16, j0 = (rem & 7) * 32;
    float* dW = which == 0 ? dW1 : dW2;
    // the owner lanes fetch the running dW values before the K loop
    f32x2 old[4];
    if (wid == 0) {
#pragma unroll
      for (int r = 0; r < 4; ++r)
        old[r] = *reinterpret_cast<const f32x2u*>(dW + (size_t)(i0 + 4 * q + r) * HD +
                                                 j0 + 2 * c);
    }
    f32x4 acc[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
    if (which == 0)
      wg_tile<true>(dh1, x, B, i0, j0, wid, c, q, acc);
    else
      wg_tile<false>(dh2, h1, B, i0, j0, wid, c, q, acc);
    if (wid > 0) {
      float* dst = red + ((wid - 1) * 64 + lane) * 8;
      *reinterpret_cast<f32x4*>(dst) = acc[0];
      *reinterpret_cast<f32x4*>(dst + 4) = acc[1];
    }
    __syncthreads();
    if (wid == 0) {
#pragma unroll
      for (int w = 0; w < 3; ++w) {
        const float* s = red + (w * 64 + lane) * 8;
        acc[0] += *reinterpret_cast<const f32x4*>(s);
        acc[1] += *reinterpret_cast<const f32x4*>(s + 4);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        f32x2 o = old[r];
        o[0] += acc[0][r];
        o[1] += acc[1][r];
        *reinterpret_cast<f32x2u*>(dW + (size_t)(i0 + 4 * q + r) * HD + j0 + 2 * c) = o;
      }
    }
    return;
  }
  // tail: 16 columns x 16 row groups per block, 8 independent loads per
  // thread and round (B = 256 is two rounds)
  const int tb = blockIdx.x - WG_TILES;
  const int srcid = tb >> 4;  // 0: dW3, 1: db1, 2: db2
  const int col = (tb & 15) * 16 + (tid & 15);
  const int rg = tid >> 4;
  const float* src = srcid == 0 ? h2 : (srcid == 1 ? dh1 : dh2);
  float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int r = rg; r < B; r += 128) {
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int rr = r + 16 * u;
      const int rc = min(rr, B - 1);
      const float v = src[(size_t)rc * HD + col];
      const float m = srcid == 0 ? dlogits[rc] : 1.f;
      s[u] += rr < B ? m * v : 0.f;
    }
  }
  red[rg * 16 + (tid & 15)] =
      ((s[0] + s[1]) + (s[2] + s[3])) + ((s[4] + s[5]) + (s[6] + s[7]));
  __syncthreads();
  if (tid < 16) {
    float t = 0.f;
#pragma unroll
    for (int g = 0; g < 16; ++g) t += red[g * 16 + tid];
    float* dst = srcid == 0 ? dW3 : (srcid == 1 ? db1 : db2);
    dst[col] += t;  // accumulate: out may be a live .grad
  }
  if (tb == 0 && wid == 1) {  // db3 = sum(dlogits), one wave, fixed order
    float t = 0.f;
    for (int rr = lane; rr < B; rr += 64) t += dlogits[rr];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) t += __shfl_xor(t, off);
    if (lane == 0) db3[0] += t;
  }
}

// ---------------------------------------------------------------------------
// Gate + attention pool, node-chunk parallel (see the file header).
// ---------------------------------------------------------------------------

constexpr int GP_CH = 64;  // nodes per block: one wave's width for the scans

// largest g in [0, B) with offs[g] <= v (v < offs[B]); skips empty graphs.
// 16-ary: the 15 pivot loads of a round are independent, so B = 256 costs
// two memory round trips where a binary search chains nine.
__device__ __forceinline__ int find_graph(const int* __restrict__ offs, int B, int v) {
  int lo = 0, hi = B;  // offs[lo] <= v < offs[hi]
  while (hi - lo > 1) {
    const int step = (hi - lo + 15) >> 4;
    int cnt = 0;
#pragma unroll
    for (int j = 1; j < 16; ++j) cnt += offs[min(lo + step * j, hi)] <= v ? 1 : 0;
    lo += step * cnt;  // sorted offsets: the pivots <= v are a prefix
    hi = min(lo + step, hi);
  }
  return lo;
}

// workspace per chunk: two partial slots. Slot 1 is the piece of a graph that
// runs on past the chunk's end, slot 0 the piece of a graph that began before
// the chunk and ends inside it. ws_vec[(2c+slot)*256 + d], ws_ms[(2c+slot)*2].
__global__ __launch_bounds__(256) void gate_pool_fwd_kernel(
    const __hip_bfloat16* __restrict__ x1, const __hip_bfloat16* __restrict__ x2,
    const float* __restrict__ wg, const float* __restrict__ bg,
    const int* __restrict__ offs, __hip_bfloat16* __restrict__ out,
    float* __restrict__ pooled32, float* __restrict__ alpha, int* __restrict__ gid_out,
    float* __restrict__ ws_vec, float* __restrict__ ws_ms, int N, int B) {
  __shared__ uint4 xs4[GP_CH * 32];  // 64 rows x 512 B (bf16 concat rows)
  __shared__ float gl[GP_CH], wv[GP_CH], pM[GP_CH], pS[GP_CH];
  __shared__ int code[GP_CH];
  __shared__ unsigned long long hmask;
  const int tid = threadIdx.x, lane = tid & 63;
  const int rg = tid >> 5, seg = tid & 31;
  const int c0 = blockIdx.x * GP_CH;
  const int nv = min(GP_CH, N - c0);

  // every row of the chunk in flight at once: 8 x 16-B loads per thread
  uint4 xv[8];
#pragma unroll
  for (int p = 0; p < 8; ++p) {
    const int gr = min(c0 + p * 8 + rg, N - 1);
    const __hip_bfloat16* src = seg < 16 ? x1 + (size_t)gr * 128 + seg * 8
                                         : x2 + (size_t)gr * 128 + (seg - 16) * 8;
    xv[p] = *reinterpret_cast<const uint4*>(src);
  }
  const f32x4 wga = *reinterpret_cast<const f32x4u*>(wg + seg * 8);
  const f32x4 wgb = *reinterpret_cast<const f32x4u*>(wg + seg * 8 + 4);
  // wave 0 locates each node's graph while the rows are on their way
  int g = -1, glo = 0, ghi = 0;
  if (tid < GP_CH && tid < nv) {
    g = find_graph(offs, B, c0 + tid);
    glo = offs[g];
    ghi = offs[g + 1];
  }
  const float bias = bg[0];
#pragma unroll
  for (int p = 0; p < 8; ++p) {
    const int row = p * 8 + rg;
    xs4[row * 32 + seg] = xv[p];
    float f[8];
    unpack8(xv[p], f);
    float dot = ((wga[0] * f[0] + wga[1] * f[1]) + (wga[2] * f[2] + wga[3] * f[3])) +
                ((wgb[0] * f[4] + wgb[1] * f[5]) + (wgb[2] * f[6] + wgb[3] * f[7]));
#pragma unroll
    for (int off = 16; off > 0; off >>= 1) dot += __shfl_xor(dot, off);
    if (seg == 0) gl[row] = dot + bias;
  }
  __syncthreads();
  if (tid < GP_CH) {  // wave 0: segmented softmax over the chunk's pieces
    const bool valid = lane < nv;
    const float l = valid ? gl[lane] : -3.0e38f;
    const int gprev = __shfl_up(g, 1);
    const bool head = valid && (lane == 0 || gprev != g);
    const unsigned long long mask = __ballot(head);
    float m = l;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const float y = __shfl_up(m, d);
      const int gy = __shfl_up(g, d);
      if (lane >= d && gy == g) m = fmaxf(m, y);
    }
    const int last = valid ? (min(ghi, c0 + nv) - c0 - 1) : lane;
    const float M = __shfl(m, last);
    const float pe = valid ? expf(l - M) : 0.f;
    float s = pe;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const float y = __shfl_up(s, d);
      const int gy = __shfl_up(g, d);
      if (lane >= d && gy == g) s += y;
    }
    const float S = __shfl(s, last);
    if (valid) {
      const bool whole = glo >= c0 && ghi <= c0 + GP_CH;
      const float w = whole ? pe / S : pe;
      wv[lane] = w;
      alpha[c0 + lane] = w;
      gid_out[c0 + lane] = g;
      code[lane] = whole ? g : (ghi > c0 + GP_CH ? -2 : -1);
      pM[lane] = M;
      pS[lane] = S;
    }
    if (lane == 0) hmask = mask;
  }
  __syncthreads();
  // weighted sums from LDS: thread d owns column d of every piece
  const unsigned short* xs16 = reinterpret_cast<const unsigned short*>(xs4);
  unsigned long long mask = hmask;
  while (mask) {
    const int s = __ffsll((long long)mask) - 1;
    mask &= mask - 1;
    const int e = mask ? __ffsll((long long)mask) - 1 : nv;
    float acc = 0.f;
#pragma unroll 4
    for (int v = s; v < e; ++v)
      acc += wv[v] * __uint_as_float((uint32_t)xs16[v * HD + tid] << 16);
    const int cd = code[s];
    if (cd >= 0) {
      out[(size_t)cd * HD + tid] = __float2bfloat16(acc);
      pooled32[(size_t)cd * HD + tid] = acc;
    } else {
      const size_t slot = (size_t)blockIdx.x * 2 + (-1 - cd);
      ws_vec[slot * HD + tid] = acc;
      if (tid == 0) {
        ws_ms[slot * 2] = pM[s];
        ws_ms[slot * 2 + 1] = pS[s];
      }
    }
  }
}

// one block per graph: merges the per-chunk partials of a graph that a chunk
// boundary cut, rescales its alpha to the global max/sum, and zero-fills the
// rows of empty graphs. Graphs that lie inside one chunk return at once.
__global__ __launch_bounds__(256) void gate_pool_combine_kernel(
    const int* __restrict__ offs, const float* __restrict__ ws_vec,
    const float* __restrict__ ws_ms, __hip_bfloat16* __restrict__ out,
    float* __restrict__ pooled32, float* __restrict__ alpha) {
  const int g = blockIdx.x, tid = threadIdx.x;
  const int lo = offs[g], hi = offs[g + 1];
  if (hi <= lo) {
    out[(size_t)g * HD + tid] = __float2bfloat16(0.f);
    pooled32[(size_t)g * HD + tid] = 0.f;
    return;
  }
  const int cf = lo / GP_CH, cl = (hi - 1) / GP_CH;
  if (cf == cl) return;
  float M = -3.0e38f;
  for (int c = cf; c <= cl; ++c) {
    const int slot = 2 * c + (hi > (c + 1) * GP_CH ? 1 : 0);
    M = fmaxf(M, ws_ms[slot * 2]);
  }
  float S = 0.f, acc = 0.f;
  for (int c = cf; c <= cl; ++c) {
    const int slot = 2 * c + (hi > (c + 1) * GP_CH ? 1 : 0);
    const float f = expf(ws_ms[slot * 2] - M);
    S += ws_ms[slot * 2 + 1] * f;
    acc += ws_vec[(size_t)slot * HD + tid] * f;
  }
  const float inv = 1.0f / S;
  out[(size_t)g * HD + tid] = __float2bfloat16(acc * inv);
  pooled32[(size_t)g * HD + tid] = acc * inv;
  for (int v = lo + tid; v < hi; v += 256) {
    const int c = v / GP_CH;
    const int slot = 2 * c + (hi > (c + 1) * GP_CH ? 1 : 0);
    alpha[v] *= expf(ws_ms[slot * 2] - M) * inv;
  }
}

// backward, one pass, one 64-node chunk per block. For node v of graph g:
//   s_v = <go_g, x_v>, dot_g = <go_g, pooled_fp32_g> (= sum_u alpha_u s_u),
//   dgate_v = alpha_v (s_v - dot_g), gx_v = alpha_v go_g + dgate_v wg,
//   dwg += dgate_v x_v, dbg += dgate_v.
// A thread holds 8 columns of 8 rows in registers; nothing goes through
// global memory inside the block and the rows never touch LDS at all. The
// node -> graph map is the one the forward already worked out (gid).
__global__ __launch_bounds__(256) void gate_pool_bwd_kernel(
    const __hip_bfloat16* __restrict__ go, const __hip_bfloat16* __restrict__ x1,
    const __hip_bfloat16* __restrict__ x2, const float* __restrict__ wg,
    const float* __restrict__ alpha, const float* __restrict__ pooled32,
    const int* __restrict__ gid, __hip_bfloat16* __restrict__ gx1,
    __hip_bfloat16* __restrict__ gx2, float* __restrict__ dwg,
    float* __restrict__ dbg, int N) {
  __shared__ __attribute__((aligned(16))) float redw[8 * HD];
  __shared__ float redb[8];
  const int tid = threadIdx.x;
  const int rg = tid >> 5, seg = tid & 31;
  const int c0 = blockIdx.x * GP_CH;

  uint4 xv[8];
#pragma unroll
  for (int p = 0; p < 8; ++p) {
    const int gr = min(c0 + p * 8 + rg, N - 1);
    const __hip_bfloat16* src = seg < 16 ? x1 + (size_t)gr * 128 + seg * 8
                                         : x2 + (size_t)gr * 128 + (seg - 16) * 8;
    xv[p] = *reinterpret_cast<const uint4*>(src);
  }
  const f32x4 wga = *reinterpret_cast<const f32x4u*>(wg + seg * 8);
  const f32x4 wgb = *reinterpret_cast<const f32x4u*>(wg + seg * 8 + 4);
  float ldw[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  float lb = 0.f;
#pragma unroll
  for (int p = 0; p < 8; ++p) {
    const int row = p * 8 + rg;
    const int v = c0 + row;
    const bool valid = v < N;
    const int g = gid[min(v, N - 1)];  // per-node graph id saved by the forward
    const float a = valid ? alpha[v] : 0.f;
    const uint4 gu = *reinterpret_cast<const uint4*>(go + (size_t)g * HD + seg * 8);
    const f32x4 pa = *reinterpret_cast<const f32x4*>(pooled32 + (size_t)g * HD + seg * 8);
    const f32x4 pb =
        *reinterpret_cast<const f32x4*>(pooled32 + (size_t)g * HD + seg * 8 + 4);
    float gf[8], xf[8];
    unpack8(gu, gf);
    unpack8(xv[p], xf);
    float sv = ((gf[0] * xf[0] + gf[1] * xf[1]) + (gf[2] * xf[2] + gf[3] * xf[3])) +
               ((gf[4] * xf[4] + gf[5] * xf[5]) + (gf[6] * xf[6] + gf[7] * xf[7]));
    float dt = ((gf[0] * pa[0] + gf[1] * pa[1]) + (gf[2] * pa[2] + gf[3] * pa[3])) +
               ((gf[4] * pb[0] + gf[5] * pb[1]) + (gf[6] * pb[2] + gf[7] * pb[3]));
#pragma unroll
    for (int off = 16; off > 0; off >>= 1) {
      sv += __shfl_xor(sv, off);
      dt += __shfl_xor(dt, off);
    }
    const float dgate = valid ? a * (sv - dt) : 0.f;
    const float wgf[8] = {wga[0], wga[1], wga[2], wga[3], wgb[0], wgb[1], wgb[2], wgb[3]};
    float o[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      o[j] = a * gf[j] + dgate * wgf[j];
      ldw[j] += dgate * xf[j];
    }
    if (seg == 0) lb += dgate;
    if (valid) {
      uint4 ou;
      ou.x = pack_bf2(o[0], o[1]);
      ou.y = pack_bf2(o[2], o[3]);
      ou.z = pack_bf2(o[4], o[5]);
      ou.w = pack_bf2(o[6], o[7]);
      __hip_bfloat16* dst = seg < 16 ? gx1 + (size_t)v * 128 + seg * 8
                                     : gx2 + (size_t)v * 128 + (seg - 16) * 8;
      *reinterpret_cast<uint4*>(dst) = ou;
    }
  }
  *reinterpret_cast<f32x4*>(redw + rg * HD + seg * 8) = f32x4{ldw[0], ldw[1], ldw[2], ldw[3]};
  *reinterpret_cast<f32x4*>(redw + rg * HD + seg * 8 + 4) =
      f32x4{ldw[4], ldw[5], ldw[6], ldw[7]};
  if (seg == 0) redb[rg] = lb;
  __syncthreads();
  float t = 0.f;
#pragma unroll
  for (int r = 0; r < 8; ++r) t += redw[r * HD + tid];
  if (t != 0.f) atomicAdd(&dwg[tid], t);
  if (tid == 0) {
    float tb = 0.f;
#pragma unroll
    for (int r = 0; r < 8; ++r) tb += redb[r];
    if (tb != 0.f) atomicAdd(dbg, tb);
  }
}

}  // namespace

// ---------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------

int gate_pool_num_chunks(int N) { return (N + GP_CH - 1) / GP_CH; }

void launch_gate_pool_fwd(const __hip_bfloat16* x1, const __hip_bfloat16* x2,
                          const float* wg, const float* bg, const int* node_offsets,
                          __hip_bfloat16* out, float* pooled32, float* alpha,
                          int* gid, float* ws_vec, float* ws_ms, int N, int B,
                          hipStream_t stream) {
  if (B <= 0) return;
  const int nch = gate_pool_num_chunks(N);
  if (nch > 0)
    hipLaunchKernelGGL(gate_pool_fwd_kernel, dim3(nch), dim3(256), 0, stream, x1, x2,
                       wg, bg, node_offsets, out, pooled32, alpha, gid, ws_vec, ws_ms, N, B);
  hipLaunchKernelGGL(gate_pool_combine_kernel, dim3(B), dim3(256), 0, stream,
                     node_offsets, ws_vec, ws_ms, out, pooled32, alpha);
}

void launch_gate_pool_bwd(const __hip_bfloat16* grad_out, const __hip_bfloat16* x1,
                          const __hip_bfloat16* x2, const float* wg,
                          const float* alpha, const float* pooled32,
                          const int* gid, __hip_bfloat16* gx1,
                          __hip_bfloat16* gx2, float* dwg, float* dbg, int N, int B,
                          hipStream_t stream) {
  const int nch = gate_pool_num_chunks(N);
  if (B <= 0 || nch <= 0) return;
  hipLaunchKernelGGL(gate_pool_bwd_kernel, dim3(nch), dim3(256), 0, stream, grad_out,
                     x1, x2, wg, alpha, pooled32, gid, gx1, gx2, dwg, dbg, N);
}

void launch_mlp3_fwd(const __hip_bfloat16* x, const float* W1, const float* b1,
                     const float* W2, const float* b2, const float* W3,
                     const float* b3, float* h1, float* h2, float* logits, int B,
                     hipStream_t stream) {
  if (B <= 0) return;
  hipLaunchKernelGGL(mlp3_fwd_kernel, dim3((B + TR - 1) / TR), dim3(512), 0, stream, x,
                     W1, b1, W2, b2, W3, b3, h1, h2, logits, B);
}

void launch_mlp3_bwd(const float* dlogits, const float* h1, const float* h2,
                     const float* W1, const float* W2, const float* W3, float* dh1,
                     float* dh2, __hip_bfloat16* dx, int B, hipStream_t stream) {
  if (B <= 0) return;
  hipLaunchKernelGGL(mlp3_bwd_kernel, dim3((B + TR - 1) / TR), dim3(512), 0, stream,
                     dlogits, h1, h2, W1, W2, W3, dh1, dh2, dx, B);
}

void launch_mlp3_wgrad(const __hip_bfloat16* x, const float* h1, const float* h2,
                       const float* dh1, const float* dh2, const float* dlogits,
                       float* dW1, float* dW2, float* dW3, float* db1, float* db2,
                       float* db3, int B, hipStream_t stream) {
  if (B <= 0) return;
  hipLaunchKernelGGL(mlp3_wgrad_kernel, dim3(WG_TILES + WG_TAIL), dim3(256), 0, stream,
                     x, h1, h2, dh1, dh2, dlogits, dW1, dW2, dW3, db1, db2, db3, B);
}
