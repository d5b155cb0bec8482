// Shared bf16 MFMA tile core for the GEMM-shaped kernels on MI355X (gfx950):
// gemm_bias.hip, gemm_bf16.hip, lmhead_ce.hip, lmhead_topk.hip, node_head.hip.
//
// Common geometry: 256-thread blocks, BK = 64 K-slices held in LDS as
// 128-byte rows (64 bf16) under the XOR swizzle of tile_swz
// (cdna_hip_programming.md T2), v_mfma_f32_16x16x32_bf16, 4 B-fragments
// (64 columns) per wave. Two software pipelines feed the same k-step:
//
//   register-staged (T14)   next slice: global -> VGPRs before this slice's
//                           MFMAs, VGPRs -> LDS after them, one barrier.
//                           gemm_bias_kernel, gemm_gru_kernel; node_head
//                           takes the B-side staging and the k-step.
//   glds two-phase          next slice: global_load_lds straight into the
//                           other LDS buffer (swizzle on the source
//                           address), vmcnt(0) + barrier per slice.
//                           gemm2_kernel. lmhead_ce.hip keeps a copy of
//                           this loop (see there) on the shared layout.
//
// Both pipelines double-buffer an (A: BMT rows | B: 128 rows) pair, so one
// LDS-size helper serves the kernels' buffer addressing and the launchers.

#pragma once

#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>

#define WAVE 64

using bf16 = __hip_bfloat16;
using bf16x8 = __attribute__((ext_vector_type(8))) __bf16;  // 4 VGPRs
using f32x4 = __attribute__((ext_vector_type(4))) float;
using uint4v = __attribute__((ext_vector_type(4))) unsigned int;

#define TILE_BN 128    // B rows (output columns) per block tile
#define TILE_BK 64     // K elements per slice
#define TILE_ROWB 128  // bytes per LDS row (TILE_BK bf16)

// 128-byte-row XOR swizzle: spreads the 16-lane ds_read_b128 fragment
// groups across bank slots. tile_swz_byte is the in-row part alone.
__device__ __forceinline__ int tile_swz_byte(int row, int byte) {
  return byte ^ ((row & 7) << 4);
}
__device__ __forceinline__ int tile_swz(int row, int byte) {
  return row * TILE_ROWB + tile_swz_byte(row, byte);
}

// ---- LDS layout: buffer i = [A: bmt rows][B: TILE_BN rows], i in {0, 1} ----

constexpr int tile_pair_bytes(int bmt) { return (bmt + TILE_BN) * TILE_ROWB; }
constexpr int tile_lds_bytes(int bmt) { return 2 * tile_pair_bytes(bmt); }

template <int BMT>
__device__ __forceinline__ char* tile_abuf(char* base, int i) {
  return base + i * tile_pair_bytes(BMT);
}
template <int BMT>
__device__ __forceinline__ char* tile_bbuf(char* base, int i) {
  return base + BMT * TILE_ROWB + i * tile_pair_bytes(BMT);
}

// ---- k-step: one 64-wide K slice = two 32-wide MFMA sub-steps ----
// acc[m][n] += A(rows arow0 + 16m ..) x B(rows brow0 + 16n ..)^T from swizzled
// LDS; fragment k-range: lane>>4 picks one of 4 groups of 8 elements.
// GLDS = false (register-staged family): A fragments load first and the
//   compiler places the LDS waits between the MFMAs.
// GLDS = true (glds family): B fragments load first and an explicit
//   s_waitcnt lgkmcnt(0) precedes the MFMA cluster.
// The two forms are kept apart because each family was tuned with its own.
template <bool GLDS, int MF>
__device__ __forceinline__ void tile_kstep(f32x4 (&acc)[MF][4],
                                           const char* a_lds, int arow0,
                                           const char* b_lds, int brow0,
                                           int lane) {
  static_assert(MF == 1 || MF == 2 || MF == 4, "A fragments per wave");
#pragma unroll
  for (int ks = 0; ks < TILE_BK / 32; ++ks) {
    const int kbyte = ks * 64 + (lane >> 4) * 16;
    bf16x8 a_frag[MF], b_frag[4];
    if constexpr (GLDS) {
#pragma unroll
      for (int n = 0; n < 4; ++n)
        b_frag[n] = *reinterpret_cast<const bf16x8*>(
            b_lds + tile_swz(brow0 + n * 16 + (lane & 15), kbyte));
    }
#pragma unroll
    for (int m = 0; m < MF; ++m)
      a_frag[m] = *reinterpret_cast<const bf16x8*>(
          a_lds + tile_swz(arow0 + m * 16 + (lane & 15), kbyte));
    if constexpr (!GLDS) {
#pragma unroll
      for (int n = 0; n < 4; ++n)
        b_frag[n] = *reinterpret_cast<const bf16x8*>(
            b_lds + tile_swz(brow0 + n * 16 + (lane & 15), kbyte));
    }
    if constexpr (GLDS) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int m = 0; m < MF; ++m)
#pragma unroll
      for (int n = 0; n < 4; ++n)
        acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            a_frag[m], b_frag[n], acc[m][n], 0, 0, 0);
    __builtin_amdgcn_s_setprio(0);
  }
}

// ---- register staging: thread (tid>>3, tid&7) moves the 16-B chunk (tid&7)
// of rows (tid>>3) + 32p, p < NP, of one K slice ----

// W rows row0 + .. of W[:, kk:kk+64], row stride ldw elements. CT: rows at
// or past row_end read as zero (column tail of the output).
template <int NP, bool CT = false>
__device__ __forceinline__ void tile_w_load(const bf16* __restrict__ W,
                                            long ldw, int row0, int kk,
                                            int row_end, int tid,
                                            uint4v r[NP]) {
  const int srow = tid >> 3;
  const int soff = (tid & 7) * 16;
#pragma unroll
  for (int p = 0; p < NP; ++p) {
    const int rr = row0 + srow + p * 32;
    if constexpr (CT) {
      r[p] = {};
      if (rr >= row_end) continue;
    }
    r[p] = *reinterpret_cast<const uint4v*>(W + (long)rr * ldw + kk + soff / 2);
  }
}

template <int NP>
__device__ __forceinline__ void tile_regs_store(char* lds, int tid,
                                                const uint4v r[NP]) {
  const int srow = tid >> 3;
  const int soff = (tid & 7) * 16;
#pragma unroll
  for (int p = 0; p < NP; ++p)
    *reinterpret_cast<uint4v*>(lds + tile_swz(srow + p * 32, soff)) = r[p];
}

// ---- gathered A chunk: one 16-B chunk of a CSR segment sum ----
// The A1 half of a register-staged GEMM can be a segment sum over a CSR
// graph instead of a stored matrix: A1'[v] = sum_{e in [indptr[v],
// indptr[v+1])} A1[indices[e]]. The sum starts at 0.f, adds in edge order in
// fp32 and rounds to bf16 once, which is spmm_sum_kernel's arithmetic, so
// the staged chunk holds the bits that kernel would have written
// (flowgnn_kernels.hip).
struct TileGather {
  const int* indptr;   // (N + 1)
  const int* indices;  // source row per edge
  long lda;            // row stride of the gathered matrix, elements
  bf16* out;           // (N, K1) copy of the staged sums, or nullptr
};

union tile_pack8 {
  uint4v v;
  bf16 e[8];
};

// The gather is split like every other staged load of the pipeline: the
// rows of a segment's first GPF edges (their indices are fetched once,
// before the K loop) are requested with the slice's other global loads,
// ahead of the current slice's MFMAs, and summed here, after them. Edges
// past those (on the synthetic training graphs 18% / 35% of the nodes have
// more than 2 in- / out-edges, 0.1% / 0.7% more than 4) are walked here,
// their latency exposed, two in flight per trip; the second index of an
// odd tail is clamped (a repeated, in-bounds load) and its add skipped.
// src points at this chunk's column of row 0.
template <int GPF>
__device__ __forceinline__ uint4v tile_gather_finish(const uint4v raw[GPF],
                                                     const bf16* __restrict__ src,
                                                     long lda,
                                                     const int* __restrict__ indices,
                                                     int e0, int e1) {
  float a[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  tile_pack8 v0, v1;
#pragma unroll
  for (int q = 0; q < GPF; ++q) {
    if (e0 + q < e1) {
      v0.v = raw[q];
#pragma unroll
      for (int j = 0; j < 8; ++j) a[j] += __bfloat162float(v0.e[j]);
    }
  }
  for (int e = e0 + GPF; e < e1; e += 2) {
    const bool two = e + 1 < e1;
    const int i0 = indices[e];
    const int i1 = indices[two ? e + 1 : e];
    v0.v = *reinterpret_cast<const uint4v*>(src + (long)i0 * lda);
    v1.v = *reinterpret_cast<const uint4v*>(src + (long)i1 * lda);
#pragma unroll
    for (int j = 0; j < 8; ++j) a[j] += __bfloat162float(v0.e[j]);
    if (two) {
#pragma unroll
      for (int j = 0; j < 8; ++j) a[j] += __bfloat162float(v1.e[j]);
    }
  }
  tile_pack8 o;
#pragma unroll
  for (int j = 0; j < 8; ++j) o.e[j] = __float2bfloat16(a[j]);
  return o.v;
}

// ---- register-staged main loop (T14 double buffering), 2x2 waves ----
// acc(BMT x 128 block tile at (r0, c0)) = [A1|A2](N, K) @ W(COL, K)^T, K
// columns [0, K1) from A1 and [K1, K) from A2; rows >= N read as zero.
// The next slice's global loads issue before this slice's MFMAs (these
// N x 128-ish GEMMs are HBM-latency-bound at ~1.4 blocks/CU;
// single-buffered staging serialized load latency with the MFMA phase).
// On return every wave is past the last barrier: smem may be reused.
// GPF > 0 (GATHER): the A1 half is the segment sum (tile_gather_finish,
// GPF edges prefetched per row) over A1's rows (row stride g.lda), which
// index the whole matrix, not the block's rows; A2 and the K order of the
// slices are unchanged,
// so the accumulators see the sequence they would see reading the stored
// sum. With g.out set, the staged chunks of rows < N are also stored there.
template <int BMT, bool CT, int GPF = 0>
__device__ __forceinline__ void tile_regstaged_gemm(
    f32x4 (&acc)[BMT / 32][4], char* smem, const bf16* __restrict__ A1,
    const bf16* __restrict__ A2, int K1, const bf16* __restrict__ W, int N,
    int K, int COL, int r0, int c0, const TileGather g = {}) {
  constexpr int NAR = BMT / 32;  // A rows per thread
  constexpr bool GATHER = GPF > 0;
  constexpr int NPF = GATHER ? GPF : 1;
  const int tid = threadIdx.x;
  const int lane = tid & (WAVE - 1);
  const int wm = tid >> 7;       // 2 row-waves of BMT/2 rows
  const int wn = (tid >> 6) & 1;  // 2 col-waves of 64 cols
  const int srow = tid >> 3;
  const int soff = (tid & 7) * 16;
  // GATHER: this thread's rows' edge ranges and first GPF source rows
  int ge0[NAR], ge1[NAR], gi[NAR][NPF];
  if constexpr (GATHER) {
#pragma unroll
    for (int p = 0; p < NAR; ++p) {
      const int gr = r0 + srow + p * 32;
      ge0[p] = ge1[p] = 0;
      if (gr < N) {
        ge0[p] = g.indptr[gr];
        ge1[p] = g.indptr[gr + 1];
      }
    }
#pragma unroll
    for (int p = 0; p < NAR; ++p)
#pragma unroll
      for (int q = 0; q < NPF; ++q) {
        gi[p][q] = 0;
        if (ge0[p] + q < ge1[p]) gi[p][q] = g.indices[ge0[p] + q];
      }
  }
  // araw: the raw chunks of a gathered slice's first edges (GATHER only)
  auto load_regs = [&](int kk, uint4v ar[NAR], uint4v araw[NAR][NPF],
                       uint4v br[4]) {
    const int gk = kk + soff / 2;  // element index in K
#pragma unroll
    for (int p = 0; p < NAR; ++p) {
      const int gr = r0 + srow + p * 32;
      ar[p] = {};
      if constexpr (GATHER) {
        if (kk < K1) {  // rows >= N have an empty edge range
#pragma unroll
          for (int q = 0; q < NPF; ++q) {
            araw[p][q] = {};
            if (ge0[p] + q < ge1[p])
              araw[p][q] = *reinterpret_cast<const uint4v*>(
                  A1 + (long)gi[p][q] * g.lda + gk);
          }
          continue;
        }
      }
      if (gr < N) {
        const bf16* src = (gk < K1) ? (A1 + (long)gr * K1 + gk)
                                    : (A2 + (long)gr * (K - K1) + (gk - K1));
        ar[p] = *reinterpret_cast<const uint4v*>(src);
      }
    }
    tile_w_load<4, CT>(W, K, c0, kk, COL, tid, br);
  };
  auto write_regs = [&](int i, int kk, uint4v ar[NAR],
                        const uint4v araw[NAR][NPF], const uint4v br[4]) {
    if constexpr (GATHER) {
      if (kk < K1) {
        const int gk = kk + soff / 2;
#pragma unroll
        for (int p = 0; p < NAR; ++p) {
          const int gr = r0 + srow + p * 32;
          ar[p] = tile_gather_finish<NPF>(araw[p], A1 + gk, g.lda, g.indices, ge0[p],
                                     ge1[p]);
          if (g.out && gr < N)
            *reinterpret_cast<uint4v*>(g.out + (long)gr * K1 + gk) = ar[p];
        }
      }
    }
    tile_regs_store<NAR>(tile_abuf<BMT>(smem, i), tid, ar);
    tile_regs_store<4>(tile_bbuf<BMT>(smem, i), tid, br);
  };
  uint4v areg[NAR], areg2[NAR][NPF], breg[4];
  load_regs(0, areg, areg2, breg);
  write_regs(0, 0, areg, areg2, breg);
  __syncthreads();
  int cur = 0;
  for (int kk = 0; kk < K; kk += TILE_BK) {
    const bool has_next = (kk + TILE_BK) < K;
    if (has_next) load_regs(kk + TILE_BK, areg, areg2, breg);
    tile_kstep<false>(acc, tile_abuf<BMT>(smem, cur), wm * (BMT / 2),
                      tile_bbuf<BMT>(smem, cur), wn * 64, lane);
    if (has_next) write_regs(cur ^ 1, kk + TILE_BK, areg, areg2, breg);
    __syncthreads();
    cur ^= 1;
  }
}

// ---- glds staging: NP 1-KiB pieces per wave (4 waves: NP = rows / 32) ----
// Lane l of piece c covers (row = 8c + l/8, kbyte = (l%8)*16); the LDS side
// is linear, so the source byte offset carries the XOR swizzle.
template <int NP>
__device__ __forceinline__ void tile_glds_stage(const bf16* __restrict__ src_base,
                                                long row_stride_elems, int kk,
                                                char* lds, int wid, int lane) {
#pragma unroll
  for (int c4 = 0; c4 < NP; ++c4) {
    const int c = wid * NP + c4;
    const int row = 8 * c + (lane >> 3);
    const int kbyte = (lane & 7) * 16;
    const int src_byte = tile_swz_byte(row, kbyte);
    const bf16* gsrc = src_base + row * row_stride_elems + kk + src_byte / 2;
    __builtin_amdgcn_global_load_lds(
        reinterpret_cast<const unsigned int*>(gsrc),
        reinterpret_cast<unsigned int*>(lds + c * 1024 + (lane & 63) * 16), 16, 0, 0);
  }
}

// ---- glds two-phase main loop, 2x2 waves ----
// acc(BMT x 128) = Arows(BMT, K) @ Wrows(128, K)^T; Arows / Wrows point at
// the block's first row, all rows in bounds, K % 64 == 0. buf is the base of
// the two buffer pairs (tile_lds_bytes(BMT)); a kernel may keep more LDS
// behind them, as lmhead_ce.hip does with its fp32 tile. One vmcnt(0) + barrier per slice; on return every wave is
// past the last barrier.
template <int BMT>
__device__ __forceinline__ void tile_glds_gemm(f32x4 (&acc)[BMT / 32][4],
                                               char* buf,
                                               const bf16* __restrict__ Arows,
                                               const bf16* __restrict__ Wrows,
                                               int K, int lane, int wid) {
  const int wm = wid >> 1;
  const int wn = wid & 1;
  const int nt = K / TILE_BK;
  int cur = 0;
  tile_glds_stage<BMT / 32>(Arows, K, 0, tile_abuf<BMT>(buf, 0), wid, lane);
  tile_glds_stage<4>(Wrows, K, 0, tile_bbuf<BMT>(buf, 0), wid, lane);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  for (int t = 0; t < nt; ++t) {
    if (t + 1 < nt) {
      tile_glds_stage<BMT / 32>(Arows, K, (t + 1) * TILE_BK,
                                tile_abuf<BMT>(buf, cur ^ 1), wid, lane);
      tile_glds_stage<4>(Wrows, K, (t + 1) * TILE_BK,
                         tile_bbuf<BMT>(buf, cur ^ 1), wid, lane);
    }
    tile_kstep<true>(acc, tile_abuf<BMT>(buf, cur), wm * (BMT / 2),
                     tile_bbuf<BMT>(buf, cur), wn * 64, lane);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    cur ^= 1;
  }
}
