// Fused LM-head GEMM + top-k + logsumexp for generation, and the beam-search
// selection step that consumes it. MI355X (gfx950).
//
// The inference counterpart of lmhead_ce.hip: one decoding step needs, per
// row of the (R, Kd) hidden state, the logsumexp over the vocabulary and the
// k best columns of scale * h @ W^T. lmhead_topk_kernel streams 128-column
// vocabulary tiles through the glds MFMA pipeline of mfma_tile.h, keeps an
// online (max, sum-exp) and a sorted k-list per scanning thread and never
// materialises logits; lmhead_topk_combine_kernel merges the partial lists of
// a row. beam_select_kernel then picks the K best continuations of a source
// among its K rows' candidates. Nothing here uses atomics: equal inputs give
// bit-equal outputs.
//
// Order contract of every list in this file: value descending; among
// bit-equal values the smaller column (beam_select: the smaller parent beam,
// then the smaller candidate rank) comes first.
//
// Geometry contract (binding-enforced): Kd % 64 == 0, Wp has at least
// ceil(V / 128) * 128 rows, 1 <= k <= 16, k <= V. M is arbitrary: A rows past
// M - 1 are loaded from row M - 1 (in bounds) and produce no output.

#include <hip/hip_runtime.h>

#include "mfma_tile.h"

#define LT_BM 128
#define LT_TS 132                 // fp32 tile row stride, as lmhead_ce.hip
#define LT_TILE (smem + tile_lds_bytes(LT_BM))
#define LT_KMAX 16
#define LT_NONE (-3.4e38f)        // empty list slot / empty running max

// LDS: the two (A | B) buffer pairs of mfma_tile.h, then the fp32 logits
// tile. The k-lists live in VGPRs and the two halves of a row are merged by
// the combine kernel, so the forward's reduction scratch is not needed.
constexpr size_t lt_lds_bytes() {
  return tile_lds_bytes(LT_BM) + LT_TS * LT_BM * sizeof(float);
}

// Chunk width. lmhead_ce_fwd uses 8 column tiles per workgroup because its M
// is thousands of rows; decoding has M = batch * beams (320, 32, 6): at
// M = 320 and V = 32100 that is 3 x 32 = 96 workgroups on 256 CUs, and the
// kernel's LDS allows one workgroup per CU. The launcher therefore picks the
// smallest chunk (in tiles) whose grid still fits one wave of workgroups over
// LT_CUS CUs, capped at the CE value: 3 tiles (252 workgroups) at M = 320,
// 1 tile (251) below 129 rows, 8 from M = 1024 on. Narrower chunks cost
// (2 + 2k) floats of partials per row and chunk half, which is small against
// the vocabulary matrix each row tile streams.
#define LT_CUS 256
#define LT_CTILES_MAX 8

int lmhead_topk_chunk_tiles(long M, int n_tiles) {
  const long row_tiles = (M + LT_BM - 1) / LT_BM;
  long ct = (row_tiles * n_tiles + LT_CUS - 1) / LT_CUS;
  if (ct < 1) ct = 1;
  if (ct > LT_CTILES_MAX) ct = LT_CTILES_MAX;
  return (int)ct;
}

// A-side glds stage: tile_glds_stage<4> with the source row clamped to
// M - 1, which is why this file carries its own copy of the ~20-line main
// loop of tile_glds_gemm<128>; the W side, the k-step and the LDS layout are
// the shared ones.
__device__ __forceinline__ void lt_stage_a(const bf16* __restrict__ A, long M,
                                           long r0, int K, int kk, char* lds,
                                           int wid, int lane) {
#pragma unroll
  for (int c4 = 0; c4 < 4; ++c4) {
    const int c = wid * 4 + c4;
    const int row = 8 * c + (lane >> 3);
    const int kbyte = (lane & 7) * 16;
    const int src_byte = tile_swz_byte(row, kbyte);
    long gr = r0 + row;
    gr = gr < M ? gr : M - 1;
    const bf16* gsrc = A + gr * K + kk + src_byte / 2;
    __builtin_amdgcn_global_load_lds(
        reinterpret_cast<const unsigned int*>(gsrc),
        reinterpret_cast<unsigned int*>(lds + c * 1024 + (lane & 63) * 16), 16, 0, 0);
  }
}

// the 128x128 logits tile (r0, c0), scaled, as fp32 in LT_TILE
__device__ __forceinline__ void lt_tile_gemm(
    const bf16* __restrict__ A, const bf16* __restrict__ W, char* smem, long M,
    long r0, long c0, int K, float scale, int lane, int wid) {
  const int wm = wid >> 1;
  const int wn = wid & 1;
  f32x4 acc[4][4] = {};
  const int nt = K / TILE_BK;
  const bf16* Wrows = W + c0 * K;
  int cur = 0;
  lt_stage_a(A, M, r0, K, 0, tile_abuf<LT_BM>(smem, 0), wid, lane);
  tile_glds_stage<4>(Wrows, K, 0, tile_bbuf<LT_BM>(smem, 0), wid, lane);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  for (int t = 0; t < nt; ++t) {
    if (t + 1 < nt) {
      lt_stage_a(A, M, r0, K, (t + 1) * TILE_BK, tile_abuf<LT_BM>(smem, cur ^ 1), wid, lane);
      tile_glds_stage<4>(Wrows, K, (t + 1) * TILE_BK, tile_bbuf<LT_BM>(smem, cur ^ 1), wid,
                         lane);
    }
    tile_kstep<true>(acc, tile_abuf<LT_BM>(smem, cur), wm * 64, tile_bbuf<LT_BM>(smem, cur),
                     wn * 64, lane);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    cur ^= 1;
  }
  float* tile = reinterpret_cast<float*>(LT_TILE);
#pragma unroll
  for (int fm = 0; fm < 4; ++fm) {
    const int row = wm * 64 + fm * 16 + (lane >> 4) * 4;
#pragma unroll
    for (int fn = 0; fn < 4; ++fn) {
      const int col = wn * 64 + fn * 16 + (lane & 15);
#pragma unroll
      for (int i = 0; i < 4; ++i)
        tile[(row + i) * LT_TS + col] = acc[fm][fn][i] * scale;
    }
  }
  __syncthreads();
}

// Sorted insertion into a register-resident list, fully unrolled so that
// every index is static. The caller has already checked v > val[KC - 1]. The
// strict compare keeps an earlier (smaller) column ahead of an equal value.
template <int KC>
__device__ __forceinline__ void lt_insert(float (&val)[KC], int (&idx)[KC],
                                          float v, int col) {
#pragma unroll
  for (int c = KC - 1; c > 0; --c) {
    if (v > val[c - 1]) {  // v lands above slot c: slot c - 1 moves down
      val[c] = val[c - 1];
      idx[c] = idx[c - 1];
    } else if (v > val[c]) {
      val[c] = v;
      idx[c] = col;
    }
  }
  if (v > val[0]) {
    val[0] = v;
    idx[0] = col;
  }
}

// grid (ceil(M / 128), n_chunks). Two threads scan each tile row, 64 columns
// each; thread (row, half) of chunk c owns partial slot p = 2c + half of
// P = 2 n_chunks: running max, running sum(exp), and its k best (value,
// column) pairs in list order. Columns >= V are never scanned. Almost every
// scanned logit fails the one compare against the list's last slot; the
// insertion is the rare path.
template <int KC>
__global__ __launch_bounds__(256) void lmhead_topk_kernel(
    const bf16* __restrict__ A, const bf16* __restrict__ W, float scale, long M,
    int K, int V, int n_tiles, int ctiles, int P, int k,
    float* __restrict__ pmax, float* __restrict__ psum,
    float* __restrict__ pval, int* __restrict__ pidx) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const long r0 = (long)blockIdx.x * LT_BM;
  const int chunk = blockIdx.y;
  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x >> 6;
  const int row = threadIdx.x >> 1;
  const int half = threadIdx.x & 1;

  float run_m = LT_NONE, run_s = 0.f;
  float val[KC];
  int idx[KC];
#pragma unroll
  for (int c = 0; c < KC; ++c) {
    val[c] = LT_NONE;
    idx[c] = -1;
  }

  const int ct_lo = chunk * ctiles;
  const int ct_hi = min(ct_lo + ctiles, n_tiles);
  for (int ct = ct_lo; ct < ct_hi; ++ct) {
    const long c0 = (long)ct * TILE_BN;
    lt_tile_gemm(A, W, smem, M, r0, c0, K, scale, lane, wid);
    const float* trow =
        reinterpret_cast<const float*>(LT_TILE) + row * LT_TS + half * 64;
    const int col0 = (int)c0 + half * 64;
    const int cend = min(64, V - col0);
    if (cend > 0) {
      float m = LT_NONE;
      for (int j = 0; j < cend; ++j) {
        const float v = trow[j];
        m = fmaxf(m, v);
        if (v > val[KC - 1]) lt_insert<KC>(val, idx, v, col0 + j);
      }
      const float mn = fmaxf(run_m, m);
      float s = run_s > 0.f ? run_s * __expf(run_m - mn) : 0.f;
#pragma unroll 4
      for (int j = 0; j < cend; ++j) s += __expf(trow[j] - mn);
      run_m = mn;
      run_s = s;
    }
    __syncthreads();  // the tile is rewritten by the next iteration
  }
  if (r0 + row < M) {
    const long o = (r0 + row) * P + chunk * 2 + half;
    pmax[o] = run_m;
    psum[o] = run_s;
#pragma unroll
    for (int c = 0; c < KC; ++c) {
      if (c < k) {
        pval[o * k + c] = val[c];
        pidx[o * k + c] = idx[c];
      }
    }
  }
}

// a precedes b in list order
__device__ __forceinline__ bool lt_before(float av, int ai, float bv, int bi) {
  return av > bv || (av == bv && ai < bi);
}

// -------- combine: one wave per row merges its P partial slots ------------
// lse as in lmhead_ce_reduce_kernel. Top-k: k rounds, each taking the first
// candidate in list order that comes strictly after the previous round's
// winner (columns are distinct, so the order is total); empty slots carry
// column -1 and are skipped. The candidates of a row (P k pairs, 13 KB at
// M = 320, k = 10) stay in cache across the rounds.
__global__ __launch_bounds__(256) void lmhead_topk_combine_kernel(
    const float* __restrict__ pmax, const float* __restrict__ psum,
    const float* __restrict__ pval, const int* __restrict__ pidx, int P, int k,
    long M, float* __restrict__ lse, float* __restrict__ val,
    int* __restrict__ idx) {
  const int lane = threadIdx.x & (WAVE - 1);
  const long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= M) return;  // whole waves leave; no barrier below
  float m = LT_NONE;
  for (int p = lane; p < P; p += WAVE) m = fmaxf(m, pmax[r * P + p]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
  float s = 0.f;
  for (int p = lane; p < P; p += WAVE) {
    const float ps = psum[r * P + p];
    if (ps > 0.f) s += ps * __expf(pmax[r * P + p] - m);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
  if (lane == 0) lse[r] = m + __logf(s);

  const int n = P * k;
  const float* cv = pval + r * n;
  const int* ci = pidx + r * n;
  float last_v = __builtin_inff();
  int last_i = -1;
  for (int c = 0; c < k; ++c) {
    float bv = -__builtin_inff();
    int bi = 0x7fffffff;
    for (int e = lane; e < n; e += WAVE) {
      const int i = ci[e];
      if (i < 0) continue;
      const float v = cv[e];
      if (lt_before(last_v, last_i, v, i) && lt_before(v, i, bv, bi)) {
        bv = v;
        bi = i;
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(bv, o);
      const int oi = __shfl_xor(bi, o);
      if (lt_before(ov, oi, bv, bi)) {
        bv = ov;
        bi = oi;
      }
    }
    if (lane == 0) {
      val[r * k + c] = bv;
      idx[r * k + c] = bi;
    }
    last_v = bv;
    last_i = bi;
  }
}

// -------- beam selection: one wave per source -----------------------------
// Row r = b K + p (parent beam p) offers candidate (p, c), c < K:
//   live      total = beam_scores[r] + (val[r, c] - lse[r]), token idx[r, c]
//   finished  c = 0 only: total = beam_scores[r], token fill_token.
// The K best in (total descending, p ascending, c ascending) become the
// source's new beams. K <= 16: a lane holds candidates e = lane + 64 i, i < 4,
// e = p K + c, which makes "e ascending" the tie order.
__global__ __launch_bounds__(64) void beam_select_kernel(
    const float* __restrict__ val, const int* __restrict__ idx,
    const float* __restrict__ lse, const float* __restrict__ beam_scores,
    const bool* __restrict__ done, int K, long fill_token, long eos,
    float* __restrict__ out_scores, long* __restrict__ parent,
    long* __restrict__ tok, bool* __restrict__ done_new) {
  const int lane = threadIdx.x;
  const long b = blockIdx.x;
  const int n = K * K;
  float tot[4];
  bool ok[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int e = lane + WAVE * i;
    ok[i] = false;
    tot[i] = 0.f;
    if (e < n) {
      const int p = e / K, c = e - p * K;
      const long r = b * K + p;
      const bool fin = done[r];
      const float bs = beam_scores[r];
      ok[i] = !fin || c == 0;
      tot[i] = fin ? bs : bs + (val[r * K + c] - lse[r]);
    }
  }
  for (int j = 0; j < K; ++j) {
    float bt = -__builtin_inff();
    int be = 0x7fffffff;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int e = lane + WAVE * i;
      if (ok[i] && lt_before(tot[i], e, bt, be)) {
        bt = tot[i];
        be = e;
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ot = __shfl_xor(bt, o);
      const int oe = __shfl_xor(be, o);
      if (lt_before(ot, oe, bt, be)) {
        bt = ot;
        be = oe;
      }
    }
    // K rows offer at least one candidate each, so be is a real candidate
    // unless totals are NaN; the clamp keeps even that case in bounds
    if (be >= n) be = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (be == lane + WAVE * i) ok[i] = false;
    if (lane == 0) {
      const int p = be / K, c = be - p * K;
      const long r = b * K + p;
      const bool fin = done[r];
      const long t = fin ? fill_token : (long)idx[r * K + c];
      const long o = b * K + j;
      out_scores[o] = bt;
      parent[o] = r;
      tok[o] = t;
      done_new[o] = fin || t == eos;
    }
  }
}

// -------- launchers -------------------------------------------------------

size_t lmhead_topk_lds_bytes() { return lt_lds_bytes(); }

template <int KC>
static void launch_lt(const bf16* A, const bf16* W, float scale, long M, int K,
                      int V, int n_tiles, int ctiles, int n_chunks, int k,
                      float* pmax, float* psum, float* pval, int* pidx,
                      hipStream_t stream) {
  const dim3 grid((M + LT_BM - 1) / LT_BM, n_chunks);
  hipLaunchKernelGGL(lmhead_topk_kernel<KC>, grid, dim3(256), lt_lds_bytes(),
                     stream, A, W, scale, M, K, V, n_tiles, ctiles,
                     2 * n_chunks, k, pmax, psum, pval, pidx);
}

// partials: pmax, psum (M, 2 n_chunks); pval, pidx (M, 2 n_chunks, k).
// The list length is a template parameter (static register indices); 10 is
// the beam width of the CodeT5 evaluation configs.
void launch_lmhead_topk(const bf16* A, const bf16* W, float scale, long M,
                        int K, int V, int ctiles, int n_chunks, int k,
                        float* pmax, float* psum, float* pval, int* pidx,
                        float* lse, float* val, int* idx, hipStream_t stream) {
  const int n_tiles = (V + TILE_BN - 1) / TILE_BN;
#define LT_ARGS A, W, scale, M, K, V, n_tiles, ctiles, n_chunks, k, pmax, psum, pval, pidx, stream
  if (k == 1) launch_lt<1>(LT_ARGS);
  else if (k <= 4) launch_lt<4>(LT_ARGS);
  else if (k <= 10) launch_lt<10>(LT_ARGS);
  else launch_lt<LT_KMAX>(LT_ARGS);
#undef LT_ARGS
  hipLaunchKernelGGL(lmhead_topk_combine_kernel, dim3((M + 3) / 4), dim3(256),
                     0, stream, pmax, psum, pval, pidx, 2 * n_chunks, k, M, lse,
                     val, idx);
}

void launch_beam_select(const float* val, const int* idx, const float* lse,
                        const float* beam_scores, const bool* done, long B,
                        int K, long fill_token, long eos, float* out_scores,
                        long* parent, long* tok, bool* done_new,
                        hipStream_t stream) {
  hipLaunchKernelGGL(beam_select_kernel, dim3(B), dim3(64), 0, stream, val, idx,
                     lse, beam_scores, done, K, fill_token, eos, out_scores,
                     parent, tok, done_new);
}
