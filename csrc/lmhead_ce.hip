// K21: fused LM-head GEMM + cross-entropy over vocab 32100 (CodeT5),
// MI355X (gfx950).
//
// Reference call site: CodeT5 models.py, the seq2seq loss — the T5
// teacher-forcing step computes logits (b*512, 32100) and CE over them;
// torch materializes the fp32 logits (526 MB at b=8) plus fp32 dlogits in
// the backward. Here the forward computes online logsumexp per row while
// streaming vocab tiles through the gemm2 MFMA pipeline (gemm_bf16.hip) —
// logits are NEVER materialized; the backward recomputes each tile and
// emits scaled bf16 dlogits = (softmax - onehot) * gscale directly (the
// only V-sized tensor, half the reference's smallest materialization),
// which then feeds two library GEMMs for dh and the tied-embedding dW.
//
// Geometry contract (wrapper-enforced): M % 128 == 0, K % 64 == 0,
// Vp % 128 == 0 (W padded with zero rows to Vp; cols >= V are masked).

#include <hip/hip_runtime.h>

#include "mfma_tile.h"

#define CE_BM 128
#define CE_BN TILE_BN
#define CE_BK TILE_BK
#define CE_CTILES 8       // vocab c-tiles (of 128) per workgroup chunk

// one 128x64 bf16 tile -> LDS via global_load_lds, 4 1-KiB pieces per wave.
// This file keeps its own copy of the glds stage and main loop of
// mfma_tile.h (tile_glds_stage<4>, tile_glds_gemm<128>): routed through the
// shared loop the forward ran 2.8 % slower (0.7 % through the shared stage
// and k-step under its own loop) with the same instruction counts, and the
// cause was not found. It shares the aliases, tile_swz and the LDS layout.
__device__ __forceinline__ void ce_stage(const bf16* __restrict__ src_base,
                                         long row_stride_elems, int kk,
                                         char* lds, int wid, int lane) {
#pragma unroll
  for (int c4 = 0; c4 < 4; ++c4) {
    const int c = wid * 4 + c4;
    const int row = 8 * c + (lane >> 3);
    const int kbyte = (lane & 7) * 16;
    const int src_byte = tile_swz_byte(row, kbyte);
    const bf16* gsrc = src_base + row * row_stride_elems + kk + src_byte / 2;
    __builtin_amdgcn_global_load_lds(
        reinterpret_cast<const unsigned int*>(gsrc),
        reinterpret_cast<unsigned int*>(lds + c * 1024 + (lane & 63) * 16), 16, 0, 0);
  }
}

// LDS: the two (A | B) buffer pairs of mfma_tile.h, then the fp32 logits
// tile [CE_BM][CE_TS], then the forward's per-row reduction scratch
#define CE_ABUF(i) (smem + (i) * tile_pair_bytes(CE_BM))
#define CE_BBUF(i) (smem + CE_BM * TILE_ROWB + (i) * tile_pair_bytes(CE_BM))
#define CE_TILE (smem + tile_lds_bytes(CE_BM))
#define CE_TS 132
#define CE_RED_FLOATS 1024
constexpr size_t ce_lds_bytes() {
  return tile_lds_bytes(CE_BM) + (CE_TS * CE_BM + CE_RED_FLOATS) * sizeof(float);
}

// compute the 128x128 logits tile (r0, c0) into acc and spill fp32 to
// CE_TILE (row stride CE_TS floats). Shared by fwd and bwd kernels.
__device__ __forceinline__ void ce_tile_gemm(
    const bf16* __restrict__ A, const bf16* __restrict__ W, char* smem,
    long r0, long c0, int K, float scale, int lane, int wid) {
  const int wm = wid >> 1;
  const int wn = wid & 1;
  f32x4 acc[4][4] = {};
  const int nt = K / CE_BK;
  int cur = 0;
  ce_stage(A + r0 * K, K, 0, CE_ABUF(0), wid, lane);
  ce_stage(W + c0 * K, K, 0, CE_BBUF(0), wid, lane);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  for (int t = 0; t < nt; ++t) {
    if (t + 1 < nt) {
      ce_stage(A + r0 * K, K, (t + 1) * CE_BK, CE_ABUF(cur ^ 1), wid, lane);
      ce_stage(W + c0 * K, K, (t + 1) * CE_BK, CE_BBUF(cur ^ 1), wid, lane);
    }
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      const int kbyte = ks * 64 + (lane >> 4) * 16;
      bf16x8 a_frag[4], b_frag[4];
#pragma unroll
      for (int f = 0; f < 4; ++f) {
        const int brow = wn * 64 + f * 16 + (lane & 15);
        b_frag[f] = *reinterpret_cast<const bf16x8*>(CE_BBUF(cur) + tile_swz(brow, kbyte));
      }
#pragma unroll
      for (int f = 0; f < 4; ++f) {
        const int arow = wm * 64 + f * 16 + (lane & 15);
        a_frag[f] = *reinterpret_cast<const bf16x8*>(CE_ABUF(cur) + tile_swz(arow, kbyte));
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int fm = 0; fm < 4; ++fm)
#pragma unroll
        for (int fn = 0; fn < 4; ++fn)
          acc[fm][fn] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              a_frag[fm], b_frag[fn], acc[fm][fn], 0, 0, 0);
      __builtin_amdgcn_s_setprio(0);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    cur ^= 1;
  }
  // spill scaled fp32 logits tile to LDS (row stride CE_TS floats spreads
  // the per-row scans across banks)
  float* tile = reinterpret_cast<float*>(CE_TILE);
#pragma unroll
  for (int fm = 0; fm < 4; ++fm) {
    const int row = wm * 64 + fm * 16 + (lane >> 4) * 4;
#pragma unroll
    for (int fn = 0; fn < 4; ++fn) {
      const int col = wn * 64 + fn * 16 + (lane & 15);
#pragma unroll
      for (int i = 0; i < 4; ++i)
        tile[(row + i) * CE_TS + col] = acc[fm][fn][i] * scale;
    }
  }
  __syncthreads();
}

// -------- forward: online logsumexp over this WG's vocab chunk ------------
// grid (M/128, nChunks); partial outputs (M, nChunks) fp32: running max,
// running sum(exp), target logit (0 when the target is outside the chunk).
__global__ __launch_bounds__(256) void lmhead_ce_fwd_kernel(
    const bf16* __restrict__ A, const bf16* __restrict__ W,
    const int* __restrict__ targets, float scale, int K, int V, int Vp,
    int n_chunks, float* __restrict__ pmax, float* __restrict__ psum,
    float* __restrict__ ptgt) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const long r0 = (long)blockIdx.x * CE_BM;
  const int chunk = blockIdx.y;
  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x >> 6;
  const int row = threadIdx.x >> 1;   // softmax pass: 2 threads per row
  const int half = threadIdx.x & 1;

  float run_m = -3.4e38f, run_s = 0.f, run_t = 0.f;
  const int tgt = targets[r0 + row];  // -1 = ignored row

  const int ct_lo = chunk * CE_CTILES;
  const int ct_hi = min(ct_lo + CE_CTILES, Vp / CE_BN);
  // reduction scratch sits after the fp32 tile: [128][2 halves][m,s,t]
  float* red = reinterpret_cast<float*>(CE_TILE) + CE_TS * CE_BM;

  for (int ct = ct_lo; ct < ct_hi; ++ct) {
    const long c0 = (long)ct * CE_BN;
    ce_tile_gemm(A, W, smem, r0, c0, K, scale, lane, wid);
    const float* tile = reinterpret_cast<const float*>(CE_TILE);
    float m = -3.4e38f, s = 0.f, tl = 0.f;
    const int cbase = half * 64;
    const int cend = min(64, (int)(V - c0) - cbase);
#pragma unroll 4
    for (int j = 0; j < cend; ++j) {
      const float v = tile[row * CE_TS + cbase + j];
      m = fmaxf(m, v);
    }
    for (int j = 0; j < cend; ++j) {
      const float v = tile[row * CE_TS + cbase + j];
      s += __expf(v - m);
      if ((long)cbase + j + c0 == tgt) tl = v;
    }
    // merge the two halves of the row
    red[row * 6 + half * 3] = m;
    red[row * 6 + half * 3 + 1] = s;
    red[row * 6 + half * 3 + 2] = tl;
    __syncthreads();
    if (half == 0) {  // half-0 thread carries the row's running state
      const float m0 = red[row * 6], s0 = red[row * 6 + 1];
      const float m1 = red[row * 6 + 3], s1 = red[row * 6 + 4];
      const float mt = fmaxf(m0, m1);
      const float st = (s0 > 0.f ? s0 * __expf(m0 - mt) : 0.f) +
                       (s1 > 0.f ? s1 * __expf(m1 - mt) : 0.f);
      run_t += red[row * 6 + 2] + red[row * 6 + 5];
      if (mt > -3.0e38f) {
        const float mn = fmaxf(run_m, mt);
        run_s = (run_s > 0.f ? run_s * __expf(run_m - mn) : 0.f) +
                (st > 0.f ? st * __expf(mt - mn) : 0.f);
        run_m = mn;
      }
    }
    __syncthreads();  // tile + red LDS are rewritten next iteration
  }
  if (half == 0) {
    const long o = (r0 + row) * n_chunks + chunk;
    pmax[o] = run_m;
    psum[o] = run_s;
    ptgt[o] = run_t;
  }
}

// -------- combine partials: lse + per-row loss ----------------------------
__global__ void lmhead_ce_reduce_kernel(
    const float* __restrict__ pmax, const float* __restrict__ psum,
    const float* __restrict__ ptgt, const int* __restrict__ targets,
    int n_chunks, long M, float* __restrict__ lse, float* __restrict__ loss) {
  const long r = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= M) return;
  float m = -3.4e38f;
  for (int c = 0; c < n_chunks; ++c) m = fmaxf(m, pmax[r * n_chunks + c]);
  float s = 0.f, t = 0.f;
  for (int c = 0; c < n_chunks; ++c) {
    const float pm = pmax[r * n_chunks + c], ps = psum[r * n_chunks + c];
    if (ps > 0.f) s += ps * __expf(pm - m);
    t += ptgt[r * n_chunks + c];
  }
  const float l = m + __logf(s);
  lse[r] = l;
  loss[r] = (targets[r] >= 0) ? (l - t) : 0.f;
}

// -------- backward: recompute tile, emit scaled bf16 dlogits --------------
// grid (M/128, Vp/128); dlogits (M, Vp) bf16 = (softmax - onehot) * gscale.
__global__ __launch_bounds__(256) void lmhead_ce_bwd_kernel(
    const bf16* __restrict__ A, const bf16* __restrict__ W,
    const int* __restrict__ targets, const float* __restrict__ lse,
    const float* __restrict__ gscale, float scale, int K, int V, int Vp,
    bf16* __restrict__ dlogits) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const long r0 = (long)blockIdx.x * CE_BM;
  const long c0 = (long)blockIdx.y * CE_BN;
  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x >> 6;
  ce_tile_gemm(A, W, smem, r0, c0, K, scale, lane, wid);
  // transform the fp32 LDS tile in place, then store row-major bf16
  float* tile = reinterpret_cast<float*>(CE_TILE);
  const int row = threadIdx.x >> 1;
  const int half = threadIdx.x & 1;
  const float l = lse[r0 + row];
  const float g = gscale[r0 + row];
  const int tgt = targets[r0 + row];
  const int cbase = half * 64;
#pragma unroll 4
  for (int j = 0; j < 64; ++j) {
    const long col = c0 + cbase + j;
    const float v = tile[row * CE_TS + cbase + j];
    float d = 0.f;
    if (col < V) {
      d = (__expf(v - l) - (col == tgt ? 1.f : 0.f)) * g;
    }
    tile[row * CE_TS + cbase + j] = d;
  }
  __syncthreads();
  // 16-B stores: thread covers 8 bf16; 256 threads x 8 = 2048 of 16384
  const int trow = threadIdx.x >> 4;
  const int tcol = (threadIdx.x & 15) * 8;
  for (int p = 0; p < 8; ++p) {
    const int r = trow + p * 16;
    __bf16 vals[8];
#pragma unroll
    for (int j = 0; j < 8; ++j)
      vals[j] = (__bf16)tile[r * CE_TS + tcol + j];
    *reinterpret_cast<uint4*>(dlogits + (r0 + r) * Vp + c0 + tcol) =
        *reinterpret_cast<const uint4*>(vals);
  }
}

// -------- launchers -------------------------------------------------------

void launch_lmhead_ce_fwd(const bf16* A, const bf16* W, const int* targets,
                          float scale, long M, int K, int V, int Vp,
                          float* pmax, float* psum, float* ptgt, float* lse,
                          float* loss, int n_chunks, hipStream_t stream) {
  const dim3 grid(M / CE_BM, n_chunks);
  const size_t shmem = ce_lds_bytes();
  hipLaunchKernelGGL(lmhead_ce_fwd_kernel, grid, dim3(256), shmem, stream, A, W,
                     targets, scale, K, V, Vp, n_chunks, pmax, psum, ptgt);
  const int tpb = 256;
  hipLaunchKernelGGL(lmhead_ce_reduce_kernel, dim3((M + tpb - 1) / tpb),
                     dim3(tpb), 0, stream, pmax, psum, ptgt, targets, n_chunks,
                     M, lse, loss);
}

void launch_lmhead_ce_bwd(const bf16* A, const bf16* W, const int* targets,
                          const float* lse, const float* gscale, float scale,
                          long M, int K, int V, int Vp, bf16* dlogits,
                          hipStream_t stream) {
  const dim3 grid(M / CE_BM, Vp / CE_BN);
  const size_t shmem = ce_lds_bytes();
  hipLaunchKernelGGL(lmhead_ce_bwd_kernel, grid, dim3(256), shmem, stream, A, W,
                     targets, lse, gscale, scale, K, V, Vp, dlogits);
}
