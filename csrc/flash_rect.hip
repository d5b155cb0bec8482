// General flash attention for MI355X (gfx950), head_dim = 64: any query
// length Lq >= 1 and any key length Lk >= 1.
//
// csrc/flash_attn.hip serves Lq == Lk on the 64 grid with a heavily tuned
// kernel trio; this file serves every other shape (decoder cross-attention,
// self-attention at lengths off the grid) so that no training attention call
// has to materialise a (B, H, Lq, Lk) score tensor. Same family contract:
//   Q, O (B, Lq, H*64); K, V (B, Lk, H*64), row-strided views with a
//   contiguous last dim (the halves of a fused (B, Lk, 2D) K|V buffer work);
//   keys >= min(valid[b], Lk) are masked, padded QUERY rows are computed like
//   any other row; a row with no unmasked key gives O = 0, lse = 0;
//   causal and the fp32 key-major (H, Lk, Lq) bias only at Lq == Lk;
//   stateless dropout on element ((b*H + h) * Lq + q) * Lk + key, the tuned
//   kernels' generator and, at Lq == Lk, their index.
//
// Tiling is the tuned file's 4-wave form without its profiling, 8-wave and
// XCD-remap instantiations: one block = 4 waves = 128 query rows of one
// (b, h), 64-key tiles double-buffered in LDS (K natural [key][d] with XOR
// swizzle, V as [4 key][16 d] subtiles for ds_read_b64_tr_b16),
// v_mfma_f32_16x16x32_bf16, swapped-operand QK^T so the softmax statistics
// stay inside a 16-lane column group. What differs is the edge handling:
//   * key rows >= vl are zero-filled in LDS and masked by key index, so a
//     partial last tile needs no separate path;
//   * query rows >= Lq are neither loaded nor stored; a wave whose 32 rows
//     all lie past Lq only helps staging and takes the barriers;
//   * bias reads are guarded per element (key < vl, q < Lq): a bias row is
//     Lq floats, no multiple of 16.
// Rows are H*64 bf16 = a multiple of 128 B, so the 16-B loads are aligned at
// any length.
//
// Backward is the FA2 two-pass split (launch_flash_dterm of flash_attn.hip
// with L = Lq, then a dq kernel over query tiles and a dkv kernel over
// ceil(Lk / 64) key tiles): every dQ, dK, dV element is owned by one block
// and stored exactly once, so outputs may come from an uninitialised
// allocation and results are bit-reproducible. dBias: fp32 atomicAdd.

#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>

#define WAVE 64
#define TK 64    // keys per KV tile
#define TQW 32   // query rows per wave
#define NWAVE 4  // waves per block -> 128 q rows per block

using bf16 = __hip_bfloat16;
using bf16x8 = __attribute__((ext_vector_type(8))) __bf16;
using bf16x4v = __attribute__((ext_vector_type(4))) __bf16;
using f32x4 = __attribute__((ext_vector_type(4))) float;
using uint4v = __attribute__((ext_vector_type(4))) unsigned int;
typedef __attribute__((address_space(3))) bf16x4v lds_bf16x4;

namespace {

// the family's stateless dropout generator (flash_attn.hip fa_hash4/fa_keep)
__device__ __forceinline__ unsigned fr_hash4(unsigned long long quad_idx,
                                             unsigned long long seed) {
  unsigned h = (unsigned)quad_idx * 2654435761u + (unsigned)(quad_idx >> 32) * 40503u +
               (unsigned)seed + (unsigned)(seed >> 32) * 97u;
  h ^= h >> 16;
  h *= 0x7feb352du;
  h ^= h >> 15;
  h *= 0x846ca68bu;
  h ^= h >> 16;
  return h;
}

__device__ __forceinline__ bool fr_keep(unsigned long long idx,
                                        unsigned long long seed, unsigned p8) {
  const unsigned h = fr_hash4(idx >> 2, seed);
  return ((h >> (8 * ((unsigned)idx & 3))) & 0xFF) >= p8;
}

// LDS addressing: 128-B rows, XOR swizzle vs 16-lane b128 fragment groups
__device__ __forceinline__ int fr_swz(int row, int byte) {
  return row * 128 + (byte ^ ((row & 7) << 4));
}

// swizzle of the transposed ([d][key]) K image of the dq kernel: XOR on
// d >> 3 spreads its scalar staging writes (d & 7 constant per instruction)
// over all banks
__device__ __forceinline__ int fr_swzT(int row, int byte) {
  return row * 128 + (byte ^ (((row >> 3) & 7) << 4));
}

// V image of the forward: [4 key][16 d] row-major bf16 subtiles padded
// 128 -> 144 B for ds_read_b64_tr_b16 (the layout of flash_attn.hip)
#define FR_VSUB(kb, db) (((kb) * 4 + (db)) * 144)
#define FR_VBYTES ((TK / 4) * 4 * 144)

// one 16-B chunk per thread and pass of a 64-key K and V tile; rows >= vl
// come back as zeros
__device__ __forceinline__ void fr_load_kv(
    const bf16* __restrict__ K, const bf16* __restrict__ V, long row0, long ldkv,
    int h, int kv0, int vl, int srow, int soff, uint4v kreg[2], uint4v vreg[2]) {
#pragma unroll
  for (int rr = 0; rr < 2; ++rr) {
    const int key = kv0 + srow + rr * 32;
    kreg[rr] = {};
    vreg[rr] = {};
    if (key < vl) {
      const long off = (row0 + key) * ldkv + (long)h * 64 + soff / 2;
      kreg[rr] = *reinterpret_cast<const uint4v*>(K + off);
      vreg[rr] = *reinterpret_cast<const uint4v*>(V + off);
    }
  }
}

// Q-side fragment (B-operand layout: lane holds row qw + fq*16 + (lane&15),
// 8 d at ks*32 + (lane>>4)*8); rows >= Lq are zeros
__device__ __forceinline__ void fr_load_rows(
    const bf16* __restrict__ X, long row0, long ld, int h, int qw, int Lq,
    int lane, bf16x8 frag[2][2]) {
#pragma unroll
  for (int fq = 0; fq < 2; ++fq)
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      const int qrow = qw + fq * 16 + (lane & 15);
      const int d = ks * 32 + (lane >> 4) * 8;
      if (qrow < Lq)
        frag[fq][ks] = *reinterpret_cast<const bf16x8*>(
            X + (row0 + qrow) * ld + (long)h * 64 + d);
      else
        frag[fq][ks] = bf16x8{};
    }
}

}  // namespace

// ---------------------------------------------------------------------------
// Forward
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(NWAVE * 64) void flash_rect_fwd_kernel(
    const bf16* __restrict__ Q, const bf16* __restrict__ K,
    const bf16* __restrict__ V, const int* __restrict__ valid,
    const float* __restrict__ bias, bf16* __restrict__ O,
    float* __restrict__ lse, int H, int Lq, int Lk, float scale, int causal,
    unsigned p8, unsigned long long seed, long ldq, long ldkv) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  // two buffers of: K [TK][64] bf16 swizzled (8 KiB) | V tr16 subtiles (9 KiB)
#define K_BUF(i) (smem + (i) * (TK * 128 + FR_VBYTES))
#define V_BUF(i) (smem + TK * 128 + (i) * (TK * 128 + FR_VBYTES))

  const int bh = blockIdx.y;
  const int b = bh / H;
  const int h = bh % H;
  const int q0 = blockIdx.x * (NWAVE * TQW);
  const int tid = threadIdx.x;
  const int lane = tid & (WAVE - 1);
  const int wid = tid >> 6;
  const int qw = q0 + wid * TQW;  // this wave's first q row
  const bool live = qw < Lq;      // wave-uniform
  const long HD = (long)H * 64;
  const int vl = valid ? min(max(valid[b], 0), Lk) : Lk;

  bf16x8 q_frag[2][2];
  fr_load_rows(Q, (long)b * Lq, ldq, h, qw, Lq, lane, q_frag);

  float m_st[2] = {-3.4e38f, -3.4e38f};
  float l_st[2] = {0.f, 0.f};
  f32x4 o_acc[2][4] = {};  // [fq][fd]: O rows (l>>4)*4+i of fq block, col fd*16+(l&15)

  const int kv_end = causal ? min(vl, q0 + NWAVE * TQW) : vl;
  const int srow = tid >> 3;        // staging row 0..31 (+32 in the 2nd pass)
  const int soff = (tid & 7) * 16;  // byte offset (8 bf16)
  auto write_tile = [&](char* kb, char* vb, const uint4v kreg[2], const uint4v vreg[2]) {
#pragma unroll
    for (int rr = 0; rr < 2; ++rr) {
      const int key = srow + rr * 32;
      const int d0 = soff / 2;
      *reinterpret_cast<uint4v*>(kb + fr_swz(key, soff)) = kreg[rr];
      *reinterpret_cast<uint4v*>(vb + FR_VSUB(key >> 2, d0 >> 4) + (key & 3) * 32 +
                                 (d0 & 15) * 2) = vreg[rr];
    }
  };
  uint4v kreg[2], vreg[2];
  int cur = 0;
  const int qcol[2] = {qw + (lane & 15), qw + 16 + (lane & 15)};
  if (kv_end > 0) {
    fr_load_kv(K, V, (long)b * Lk, ldkv, h, 0, vl, srow, soff, kreg, vreg);
    write_tile(K_BUF(0), V_BUF(0), kreg, vreg);
  }
  __syncthreads();
  for (int kv0 = 0; kv0 < kv_end; kv0 += TK) {
    const bool has_next = (kv0 + TK) < kv_end;
    if (has_next) {
      fr_load_kv(K, V, (long)b * Lk, ldkv, h, kv0 + TK, vl, srow, soff, kreg, vreg);
      write_tile(K_BUF(cur ^ 1), V_BUF(cur ^ 1), kreg, vreg);
    }
    if (live) {
      const char* k_lds_c = K_BUF(cur);
      const char* v_lds_c = V_BUF(cur);

      // ---- S^T = K @ Q^T : D[key][qrow] ----
      f32x4 s_acc[4][2] = {};  // [fkey][fq]
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        bf16x8 k_frag[4];
#pragma unroll
        for (int fk = 0; fk < 4; ++fk) {
          const int key = fk * 16 + (lane & 15);
          const int kbyte = ks * 64 + (lane >> 4) * 16;
          k_frag[fk] = *reinterpret_cast<const bf16x8*>(k_lds_c + fr_swz(key, kbyte));
        }
#pragma unroll
        for (int fk = 0; fk < 4; ++fk)
#pragma unroll
          for (int fq = 0; fq < 2; ++fq)
            s_acc[fk][fq] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                k_frag[fk], q_frag[fq][ks], s_acc[fk][fq], 0, 0, 0);
      }

      // ---- masking + bias + tile row-max (over keys, per qrow column) ----
      float tile_max[2] = {-3.4e38f, -3.4e38f};
#pragma unroll
      for (int fk = 0; fk < 4; ++fk)
#pragma unroll
        for (int fq = 0; fq < 2; ++fq)
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const int key = kv0 + fk * 16 + (lane >> 4) * 4 + i;
            const bool masked =
                key >= vl || (causal && key > qcol[fq]) || qcol[fq] >= Lq;
            float s = s_acc[fk][fq][i] * scale;
            // bias (H, key, qcol) with Lq == Lk: read in-range elements only
            if (bias && !masked) s += bias[((long)h * Lk + key) * Lq + qcol[fq]];
            s = masked ? -3.4e38f : s;
            s_acc[fk][fq][i] = s;
            tile_max[fq] = fmaxf(tile_max[fq], s);
          }
#pragma unroll
      for (int fq = 0; fq < 2; ++fq) {
        tile_max[fq] = fmaxf(tile_max[fq], __shfl_xor(tile_max[fq], 16));
        tile_max[fq] = fmaxf(tile_max[fq], __shfl_xor(tile_max[fq], 32));
      }

      // ---- online softmax update ----
      float alpha[2], sum_p[2] = {0.f, 0.f};
#pragma unroll
      for (int fq = 0; fq < 2; ++fq) {
        const float m_new = fmaxf(m_st[fq], tile_max[fq]);
        alpha[fq] = (m_st[fq] > -3.0e38f) ? __expf(m_st[fq] - m_new) : 0.f;
        m_st[fq] = m_new;
#pragma unroll
        for (int fk = 0; fk < 4; ++fk)
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const float e = (s_acc[fk][fq][i] > -3.0e38f && m_new > -3.0e38f)
                                ? __expf(s_acc[fk][fq][i] - m_new)
                                : 0.f;
            s_acc[fk][fq][i] = e;
            sum_p[fq] += e;
          }
        sum_p[fq] += __shfl_xor(sum_p[fq], 16);
        sum_p[fq] += __shfl_xor(sum_p[fq], 32);
        l_st[fq] = l_st[fq] * alpha[fq] + sum_p[fq];
      }

      // ---- dropout on P (post-softmax-numerator; scaled at epilogue) ----
      if (p8 > 0) {
        const float dscale = 256.0f / (256.0f - p8);
#pragma unroll
        for (int fk = 0; fk < 4; ++fk)
#pragma unroll
          for (int fq = 0; fq < 2; ++fq)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              const int key = kv0 + fk * 16 + (lane >> 4) * 4 + i;
              const unsigned long long idx =
                  ((unsigned long long)bh * Lq + qcol[fq]) * Lk + key;
              s_acc[fk][fq][i] = fr_keep(idx, seed, p8) ? s_acc[fk][fq][i] * dscale : 0.f;
            }
      }

      // ---- rescale O by alpha (per O-row qrow = (l>>4)*4 + i) ----
#pragma unroll
      for (int fq = 0; fq < 2; ++fq)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float a = __shfl(alpha[fq], (lane >> 4) * 4 + i);
#pragma unroll
          for (int fd = 0; fd < 4; ++fd) o_acc[fq][fd][i] *= a;
        }

      // ---- P^T (D-layout) -> P A-fragments via lane exchange, then PV ----
      // A-frag for PV k-step kp (keys kp*32..kp*32+31): lane needs
      // P[qrow = l&15 + fq*16][key = kp*32 + (l>>4)*8 + j], j = 0..7.
      // source: value (key, qrow) lives at lane ((key%16)>>2)<<4 | (qrow%16),
      // frag fkey = key/16, reg i = key%4.
#pragma unroll
      for (int kp = 0; kp < 2; ++kp) {
        bf16x8 pa[2];  // [fq]
        const int hi_half = (lane >> 5) & 1;  // lane groups 2,3 take fkey kp*2+1
#pragma unroll
        for (int fq = 0; fq < 2; ++fq) {
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            const int key = kp * 32 + (lane >> 4) * 8 + j;
            const int src = (((key & 15) >> 2) << 4) | (lane & 15);
            const float v0 = __shfl(s_acc[kp * 2][fq][j & 3], src);
            const float v1 = __shfl(s_acc[kp * 2 + 1][fq][j & 3], src);
            pa[fq][j] = (__bf16)(hi_half ? v1 : v0);
          }
        }
        bf16x8 v_frag[4];
        const int kb0 = kp * 8 + (lane >> 4) * 2;
        const int vslot = (lane & 15) * 8;
#pragma unroll
        for (int fd = 0; fd < 4; ++fd) {
          bf16x4v* vf = reinterpret_cast<bf16x4v*>(&v_frag[fd]);
          vf[0] = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(
              (lds_bf16x4*)(v_lds_c + FR_VSUB(kb0, fd) + vslot));
          vf[1] = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(
              (lds_bf16x4*)(v_lds_c + FR_VSUB(kb0 + 1, fd) + vslot));
        }
#pragma unroll
        for (int fq = 0; fq < 2; ++fq)
#pragma unroll
          for (int fd = 0; fd < 4; ++fd)
            o_acc[fq][fd] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                pa[fq], v_frag[fd], o_acc[fq][fd], 0, 0, 0);
      }
    }
    __syncthreads();
    cur ^= 1;
  }
#undef K_BUF
#undef V_BUF
  if (!live) return;  // past the last barrier

  // ---- epilogue: O /= l via a wave-local LDS bounce (16-B row stores); all
  // waves passed the loop's final barrier, so the K/V buffers are free
  char* obuf = smem + wid * 4096;  // [32 rows][64 d] bf16, swizzled
#pragma unroll
  for (int fq = 0; fq < 2; ++fq) {
    const float inv_l = (l_st[fq] > 0.f) ? 1.0f / l_st[fq] : 0.f;
    if ((lane >> 4) == 0) {
      const int qrow = qw + fq * 16 + (lane & 15);
      if (qrow < Lq)
        lse[(long)bh * Lq + qrow] = (l_st[fq] > 0.f) ? m_st[fq] + __logf(l_st[fq]) : 0.f;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int row_loc = fq * 16 + (lane >> 4) * 4 + i;
      const float il = __shfl(inv_l, (lane >> 4) * 4 + i);
#pragma unroll
      for (int fd = 0; fd < 4; ++fd) {
        const int d = fd * 16 + (lane & 15);
        *reinterpret_cast<bf16*>(obuf + fr_swz(row_loc, d * 2)) =
            __float2bfloat16(o_acc[fq][fd][i] * il);
      }
    }
    // wave-local buffer: only lgkm ordering needed (same wave reads)
#pragma unroll
    for (int pp = 0; pp < 2; ++pp) {
      const int row_loc = fq * 16 + pp * 8 + (lane >> 3);
      const int qrow = qw + row_loc;
      if (qrow < Lq) {
        const uint4v vvv =
            *reinterpret_cast<const uint4v*>(obuf + fr_swz(row_loc, (lane & 7) * 16));
        *reinterpret_cast<uint4v*>(O + ((long)b * Lq + qrow) * HD + (long)h * 64 +
                                   (lane & 7) * 8) = vvv;
      }
    }
  }
}

// ---------------------------------------------------------------------------
// Backward
// ---------------------------------------------------------------------------

// recompute P^T for NFK 16-key fragments starting at key_off of the staged
// tile: p[fk][fq][i] in D-layout (key = kv0 + key_off + fk*16 + (lane>>4)*4
// + i, qrow-col = qw + fq*16 + (lane&15)). Shared by the dq and dkv kernels.
template <int NFK>
__device__ __forceinline__ void fr_recompute_pT(
    const char* k_lds, const bf16x8 q_frag[2][2], const float* __restrict__ bias,
    const float lse_w[2], int lane, int h, int Lq, int Lk, int qw, int kv0,
    int key_off, int vl, float scale, int causal, float p[NFK][2][4]) {
  f32x4 s_acc[NFK][2] = {};
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) {
    bf16x8 k_frag[NFK];
#pragma unroll
    for (int fk = 0; fk < NFK; ++fk) {
      const int key = key_off + fk * 16 + (lane & 15);
      const int kbyte = ks * 64 + (lane >> 4) * 16;
      k_frag[fk] = *reinterpret_cast<const bf16x8*>(k_lds + fr_swz(key, kbyte));
    }
#pragma unroll
    for (int fk = 0; fk < NFK; ++fk)
#pragma unroll
      for (int fq = 0; fq < 2; ++fq)
        s_acc[fk][fq] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            k_frag[fk], q_frag[fq][ks], s_acc[fk][fq], 0, 0, 0);
  }
#pragma unroll
  for (int fk = 0; fk < NFK; ++fk)
#pragma unroll
    for (int fq = 0; fq < 2; ++fq) {
      const int qcol = qw + fq * 16 + (lane & 15);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int key = kv0 + key_off + fk * 16 + (lane >> 4) * 4 + i;
        const bool masked = key >= vl || (causal && key > qcol) || qcol >= Lq;
        float s = s_acc[fk][fq][i] * scale;
        if (bias && !masked) s += bias[((long)h * Lk + key) * Lq + qcol];
        p[fk][fq][i] = masked ? 0.f : __expf(s - lse_w[fq]);
      }
    }
}

__global__ __launch_bounds__(256) void flash_rect_dq_kernel(
    const bf16* __restrict__ Q, const bf16* __restrict__ K,
    const bf16* __restrict__ V, const bf16* __restrict__ dO,
    const int* __restrict__ valid, const float* __restrict__ bias,
    const float* __restrict__ lse, const float* __restrict__ Dterm,
    bf16* __restrict__ dQ, float* __restrict__ dBias, int H, int Lq, int Lk,
    float scale, int causal, unsigned p8, unsigned long long seed, long ldq,
    long ldkv) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  // two buffers of: K [key][d] | K^T [d][key] | V [key][d], 8 KiB each
#define DQ_K(i) (smem + (i) * 3 * TK * 128)
#define DQ_KT(i) (smem + TK * 128 + (i) * 3 * TK * 128)
#define DQ_V(i) (smem + 2 * TK * 128 + (i) * 3 * TK * 128)

  const int bh = blockIdx.y;
  const int b = bh / H;
  const int h = bh % H;
  const int q0 = blockIdx.x * (NWAVE * TQW);
  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x >> 6;
  const int qw = q0 + wid * TQW;
  const bool live = qw < Lq;  // wave-uniform
  const long HD = (long)H * 64;
  const int vl = valid ? min(max(valid[b], 0), Lk) : Lk;
  const float dscale = (p8 > 0) ? 256.0f / (256.0f - p8) : 1.0f;

  bf16x8 q_frag[2][2], do_frag[2][2];
  fr_load_rows(Q, (long)b * Lq, ldq, h, qw, Lq, lane, q_frag);
  fr_load_rows(dO, (long)b * Lq, HD, h, qw, Lq, lane, do_frag);
  float lse_w[2], dterm_w[2];
#pragma unroll
  for (int fq = 0; fq < 2; ++fq) {
    const int qrow = qw + fq * 16 + (lane & 15);
    lse_w[fq] = (qrow < Lq) ? lse[(long)bh * Lq + qrow] : 0.f;
    dterm_w[fq] = (qrow < Lq) ? Dterm[(long)bh * Lq + qrow] : 0.f;
  }

  f32x4 dq_acc[2][4] = {};  // [fq][fd]: rows (l>>4)*4+i, col fd*16+(l&15)

  const int kv_end = causal ? min(vl, q0 + NWAVE * TQW) : vl;
  const int srow = threadIdx.x >> 3;
  const int soff = (threadIdx.x & 7) * 16;
  auto dq_write = [&](char* kb, char* ktb, char* vb, const uint4v kreg[2],
                      const uint4v vreg[2]) {
#pragma unroll
    for (int rr = 0; rr < 2; ++rr) {
      *reinterpret_cast<uint4v*>(kb + fr_swz(srow + rr * 32, soff)) = kreg[rr];
      *reinterpret_cast<uint4v*>(vb + fr_swz(srow + rr * 32, soff)) = vreg[rr];
      bf16 kk[8];
      *reinterpret_cast<uint4v*>(kk) = kreg[rr];
      const int d0 = soff / 2;
#pragma unroll
      for (int j = 0; j < 8; ++j)
        *reinterpret_cast<bf16*>(ktb + fr_swzT(d0 + j, (srow + rr * 32) * 2)) = kk[j];
    }
  };
  uint4v kreg[2], vreg[2];
  int cur = 0;
  if (kv_end > 0) {
    fr_load_kv(K, V, (long)b * Lk, ldkv, h, 0, vl, srow, soff, kreg, vreg);
    dq_write(DQ_K(0), DQ_KT(0), DQ_V(0), kreg, vreg);
  }
  __syncthreads();
  for (int kv0 = 0; kv0 < kv_end; kv0 += TK) {
    const bool has_next = (kv0 + TK) < kv_end;
    if (has_next)
      fr_load_kv(K, V, (long)b * Lk, ldkv, h, kv0 + TK, vl, srow, soff, kreg, vreg);
    if (live) {
      const char* k_lds_c = DQ_K(cur);
      const char* kt_lds_c = DQ_KT(cur);
      const char* v_lds_c = DQ_V(cur);

      float p[4][2][4];
      fr_recompute_pT<4>(k_lds_c, q_frag, bias, lse_w, lane, h, Lq, Lk, qw, kv0, 0, vl,
                         scale, causal, p);

      // dPd^T = V dO^T (same structure as S^T), then ds
      f32x4 dp_acc[4][2] = {};
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        bf16x8 v_frag[4];
#pragma unroll
        for (int fk = 0; fk < 4; ++fk) {
          const int key = fk * 16 + (lane & 15);
          const int kbyte = ks * 64 + (lane >> 4) * 16;
          v_frag[fk] = *reinterpret_cast<const bf16x8*>(v_lds_c + fr_swz(key, kbyte));
        }
#pragma unroll
        for (int fk = 0; fk < 4; ++fk)
#pragma unroll
          for (int fq = 0; fq < 2; ++fq)
            dp_acc[fk][fq] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                v_frag[fk], do_frag[fq][ks], dp_acc[fk][fq], 0, 0, 0);
      }

      float ds[4][2][4];  // post-bias dS (pre-scale)
#pragma unroll
      for (int fk = 0; fk < 4; ++fk)
#pragma unroll
        for (int fq = 0; fq < 2; ++fq)
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const int key = kv0 + fk * 16 + (lane >> 4) * 4 + i;
            const int qcol = qw + fq * 16 + (lane & 15);
            float dp = dp_acc[fk][fq][i];
            if (p8 > 0) {
              const unsigned long long idx =
                  ((unsigned long long)bh * Lq + qcol) * Lk + key;
              dp = fr_keep(idx, seed, p8) ? dp * dscale : 0.f;
            }
            ds[fk][fq][i] = p[fk][fq][i] * (dp - dterm_w[fq]);
            // p == 0 wherever key >= vl or qcol >= Lq: the index is in range
            if (dBias && ds[fk][fq][i] != 0.f)
              atomicAdd(dBias + ((long)h * Lk + key) * Lq + qcol, ds[fk][fq][i]);
          }

      // dQ += scale * ds @ K : A = ds (q, key) via lane exchange, B = K^T
#pragma unroll
      for (int kp = 0; kp < 2; ++kp) {
        bf16x8 dsa[2];
        const int hi_half = (lane >> 5) & 1;
#pragma unroll
        for (int fq = 0; fq < 2; ++fq)
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            const int key = kp * 32 + (lane >> 4) * 8 + j;
            const int src = (((key & 15) >> 2) << 4) | (lane & 15);
            const float v0 = __shfl(ds[kp * 2][fq][j & 3], src);
            const float v1 = __shfl(ds[kp * 2 + 1][fq][j & 3], src);
            dsa[fq][j] = (__bf16)(scale * (hi_half ? v1 : v0));
          }
        bf16x8 kt_frag[4];
#pragma unroll
        for (int fd = 0; fd < 4; ++fd) {
          const int d = fd * 16 + (lane & 15);
          const int keybyte = kp * 64 + (lane >> 4) * 16;
          kt_frag[fd] = *reinterpret_cast<const bf16x8*>(kt_lds_c + fr_swzT(d, keybyte));
        }
#pragma unroll
        for (int fq = 0; fq < 2; ++fq)
#pragma unroll
          for (int fd = 0; fd < 4; ++fd)
            dq_acc[fq][fd] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                dsa[fq], kt_frag[fd], dq_acc[fq][fd], 0, 0, 0);
      }
    }
    if (has_next) dq_write(DQ_K(cur ^ 1), DQ_KT(cur ^ 1), DQ_V(cur ^ 1), kreg, vreg);
    __syncthreads();
    cur ^= 1;
  }
#undef DQ_K
#undef DQ_KT
#undef DQ_V
  if (!live) return;

  // write dQ (B, Lq, H*64), rows < Lq only
#pragma unroll
  for (int fq = 0; fq < 2; ++fq)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int qrow = qw + fq * 16 + (lane >> 4) * 4 + i;
      if (qrow >= Lq) continue;
#pragma unroll
      for (int fd = 0; fd < 4; ++fd) {
        const int d = fd * 16 + (lane & 15);
        dQ[((long)b * Lq + qrow) * HD + (long)h * 64 + d] =
            __float2bfloat16(dq_acc[fq][fd][i]);
      }
    }
}

__global__ __launch_bounds__(256) void flash_rect_dkv_kernel(
    const bf16* __restrict__ Q, const bf16* __restrict__ K,
    const bf16* __restrict__ V, const bf16* __restrict__ dO,
    const int* __restrict__ valid, const float* __restrict__ bias,
    const float* __restrict__ lse, const float* __restrict__ Dterm,
    bf16* __restrict__ dK, bf16* __restrict__ dV, int H, int Lq, int Lk,
    float scale, int causal, unsigned p8, unsigned long long seed, long ldq,
    long ldkv, long ldout) {
  // Wave grid 2 (32-key halves) x 2 (q-strip interleave), as the tuned dkv.
  // LDS map: K nat 8K | V nat 8K | per-wave pd 2304 B, ds 2304 B (72-B rows);
  // the pd/ds region is reused as the [d][key] fp32 pair-reduce image.
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* k_lds = smem;
  char* v_lds = smem + TK * 128;
  char* wave_base = smem + 2 * TK * 128;

  const int bh = blockIdx.y;
  const int b = bh / H;
  const int h = bh % H;
  const int kv0 = blockIdx.x * TK;
  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x >> 6;
  const int wk = wid >> 1;  // key half: keys wk*32 .. wk*32+31
  const int wq = wid & 1;   // q interleave
  const int key_off = wk * 32;
  const long HD = (long)H * 64;
  const int vl = valid ? min(max(valid[b], 0), Lk) : Lk;
  const float dscale = (p8 > 0) ? 256.0f / (256.0f - p8) : 1.0f;
  char* pd_lds = wave_base + wid * 2304;
  char* ds_lds = wave_base + 9216 + wid * 2304;

  {  // stage the K and V tiles (natural layout, swizzled), rows >= vl zero
    uint4v kreg[2], vreg[2];
    const int srow = threadIdx.x >> 3;
    const int soff = (threadIdx.x & 7) * 16;
    fr_load_kv(K, V, (long)b * Lk, ldkv, h, kv0, vl, srow, soff, kreg, vreg);
#pragma unroll
    for (int rr = 0; rr < 2; ++rr) {
      *reinterpret_cast<uint4v*>(k_lds + fr_swz(srow + rr * 32, soff)) = kreg[rr];
      *reinterpret_cast<uint4v*>(v_lds + fr_swz(srow + rr * 32, soff)) = vreg[rr];
    }
  }
  __syncthreads();

  f32x4 dv_acc[2][4] = {};  // [fkey][fd] over this wave's 32-key half
  f32x4 dk_acc[2][4] = {};

  if (kv0 < vl) {
    const int q_begin = causal ? kv0 : 0;  // a multiple of 32; < Lq with causal
    const int nstrips = (Lq - q_begin + TQW - 1) / TQW;
    for (int strip = wq; strip < nstrips; strip += 2) {
      const int qw = q_begin + strip * TQW;
      bf16x8 q_frag[2][2], do_frag[2][2];
      fr_load_rows(Q, (long)b * Lq, ldq, h, qw, Lq, lane, q_frag);
      fr_load_rows(dO, (long)b * Lq, HD, h, qw, Lq, lane, do_frag);
      float lse_w[2], dterm_w[2];
#pragma unroll
      for (int fq = 0; fq < 2; ++fq) {
        const int qrow = qw + fq * 16 + (lane & 15);
        lse_w[fq] = (qrow < Lq) ? lse[(long)bh * Lq + qrow] : 0.f;
        dterm_w[fq] = (qrow < Lq) ? Dterm[(long)bh * Lq + qrow] : 0.f;
      }

      float p[2][2][4];
      fr_recompute_pT<2>(k_lds, q_frag, bias, lse_w, lane, h, Lq, Lk, qw, kv0, key_off,
                         vl, scale, causal, p);

      f32x4 dp_acc[2][2] = {};
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        bf16x8 v_frag[2];
#pragma unroll
        for (int fk = 0; fk < 2; ++fk) {
          const int key = key_off + fk * 16 + (lane & 15);
          const int kbyte = ks * 64 + (lane >> 4) * 16;
          v_frag[fk] = *reinterpret_cast<const bf16x8*>(v_lds + fr_swz(key, kbyte));
        }
#pragma unroll
        for (int fk = 0; fk < 2; ++fk)
#pragma unroll
          for (int fq = 0; fq < 2; ++fq)
            dp_acc[fk][fq] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                v_frag[fk], do_frag[fq][ks], dp_acc[fk][fq], 0, 0, 0);
      }

      // pd (dropout-masked P) and ds = scale * P (dP - D) -> LDS bounce
#pragma unroll
      for (int fk = 0; fk < 2; ++fk)
#pragma unroll
        for (int fq = 0; fq < 2; ++fq)
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const int key_loc = fk * 16 + (lane >> 4) * 4 + i;
            const int key = kv0 + key_off + key_loc;
            const int qcol = qw + fq * 16 + (lane & 15);
            const int q_loc = fq * 16 + (lane & 15);
            float pd = p[fk][fq][i];
            float dp = dp_acc[fk][fq][i];
            if (p8 > 0) {
              const unsigned long long idx =
                  ((unsigned long long)bh * Lq + qcol) * Lk + key;
              const bool keep = fr_keep(idx, seed, p8);
              pd = keep ? pd * dscale : 0.f;
              dp = keep ? dp * dscale : 0.f;
            }
            const float dsv = scale * p[fk][fq][i] * (dp - dterm_w[fq]);
            *reinterpret_cast<bf16*>(pd_lds + key_loc * 72 + q_loc * 2) =
                __float2bfloat16(pd);
            *reinterpret_cast<bf16*>(ds_lds + key_loc * 72 + q_loc * 2) =
                __float2bfloat16(dsv);
          }

      // dV += pd(key, q) @ dO(q, d);  dK += ds(key, q) @ Q(q, d)
      bf16x8 pa[2], dsa[2];
#pragma unroll
      for (int fk = 0; fk < 2; ++fk) {
        const int key_loc = fk * 16 + (lane & 15);
        const int qbyte = (lane >> 4) * 16;
        pa[fk] = *reinterpret_cast<const bf16x8*>(pd_lds + key_loc * 72 + qbyte);
        dsa[fk] = *reinterpret_cast<const bf16x8*>(ds_lds + key_loc * 72 + qbyte);
      }
      // dO/Q B-fragments (lane holds d = fd*16 + (lane&15), 8 q rows) read
      // straight from global in transposed order: the 16-B fragment loads
      // above warmed exactly these L1 lines
      bf16x8 dob[4], qb[4];
#pragma unroll
      for (int fd = 0; fd < 4; ++fd) {
        const int d = fd * 16 + (lane & 15);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int qrow = qw + (lane >> 4) * 8 + j;
          if (qrow < Lq) {
            const long row = (long)b * Lq + qrow;
            dob[fd][j] = *reinterpret_cast<const __bf16*>(dO + row * HD + (long)h * 64 + d);
            qb[fd][j] = *reinterpret_cast<const __bf16*>(Q + row * ldq + (long)h * 64 + d);
          } else {
            dob[fd][j] = (__bf16)0.0f;
            qb[fd][j] = (__bf16)0.0f;
          }
        }
      }
#pragma unroll
      for (int fk = 0; fk < 2; ++fk)
#pragma unroll
        for (int fd = 0; fd < 4; ++fd) {
          dv_acc[fk][fd] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              pa[fk], dob[fd], dv_acc[fk][fd], 0, 0, 0);
          dk_acc[fk][fd] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              dsa[fk], qb[fd], dk_acc[fk][fd], 0, 0, 0);
        }
    }
  }

  // pair-wise reduce: the two waves of a key half (wq 0/1) hold the only
  // partials for those 32 keys. wq = 1 writes its accumulators to a [d][key]
  // fp32 image with 272-B padded rows, wq = 0 adds (always wq0 + wq1) and
  // stores every key < Lk of the tile: exact zeros for keys >= vl.
  char* img = wave_base;  // 64 * 272 B = 17 KiB <= the 18 KiB pd/ds region
#define FR_PAIR_REDUCE(ACC, OUT)                                              \
  __syncthreads();                                                            \
  if (wq == 1) {                                                              \
    _Pragma("unroll") for (int fk = 0; fk < 2; ++fk)                          \
        _Pragma("unroll") for (int fd = 0; fd < 4; ++fd) {                    \
      const int d = fd * 16 + (lane & 15);                                    \
      const int key_loc = key_off + fk * 16 + (lane >> 4) * 4;                \
      *reinterpret_cast<f32x4*>(img + d * 272 + key_loc * 4) = ACC[fk][fd];   \
    }                                                                         \
  }                                                                           \
  __syncthreads();                                                            \
  if (wq == 0) {                                                              \
    _Pragma("unroll") for (int fk = 0; fk < 2; ++fk)                          \
        _Pragma("unroll") for (int fd = 0; fd < 4; ++fd) {                    \
      const int d = fd * 16 + (lane & 15);                                    \
      const int key_loc = key_off + fk * 16 + (lane >> 4) * 4;                \
      const f32x4 other =                                                     \
          *reinterpret_cast<const f32x4*>(img + d * 272 + key_loc * 4);       \
      _Pragma("unroll") for (int i = 0; i < 4; ++i) {                         \
        const int key = kv0 + key_loc + i;                                    \
        if (key < Lk)                                                         \
          OUT[((long)b * Lk + key) * ldout + (long)h * 64 + d] =              \
              __float2bfloat16(ACC[fk][fd][i] + other[i]);                    \
      }                                                                       \
    }                                                                         \
  }
  FR_PAIR_REDUCE(dv_acc, dV)
  FR_PAIR_REDUCE(dk_acc, dK)
#undef FR_PAIR_REDUCE
}

// ---------------------------------------------------------------------------
// Launchers. Grids: x = tiles, y = b*H + h (B*H <= 65535, checked by the
// bindings). LDS stays under the 64 KiB default limit.
// ---------------------------------------------------------------------------
void launch_flash_rect_fwd(const bf16* Q, const bf16* K, const bf16* V,
                           const int* valid, const float* bias, bf16* O, float* lse,
                           int B, int H, int Lq, int Lk, float scale, int causal,
                           unsigned p8, unsigned long long seed, long ldq,
                           long ldkv, hipStream_t stream) {
  const dim3 grid((Lq + NWAVE * TQW - 1) / (NWAVE * TQW), B * H);
  const size_t lds = 2 * (TK * 128 + FR_VBYTES);  // 34816 B
  hipLaunchKernelGGL(flash_rect_fwd_kernel, grid, dim3(NWAVE * 64), lds, stream, Q, K,
                     V, valid, bias, O, lse, H, Lq, Lk, scale, causal, p8, seed, ldq,
                     ldkv);
}

void launch_flash_rect_dq(const bf16* Q, const bf16* K, const bf16* V, const bf16* dO,
                          const int* valid, const float* bias, const float* lse,
                          const float* Dterm, bf16* dQ, float* dBias, int B, int H,
                          int Lq, int Lk, float scale, int causal, unsigned p8,
                          unsigned long long seed, long ldq, long ldkv,
                          hipStream_t stream) {
  const dim3 grid((Lq + NWAVE * TQW - 1) / (NWAVE * TQW), B * H);
  const size_t lds = 2 * 3 * TK * 128;  // 49152 B
  hipLaunchKernelGGL(flash_rect_dq_kernel, grid, dim3(256), lds, stream, Q, K, V, dO,
                     valid, bias, lse, Dterm, dQ, dBias, H, Lq, Lk, scale, causal, p8,
                     seed, ldq, ldkv);
}

void launch_flash_rect_dkv(const bf16* Q, const bf16* K, const bf16* V, const bf16* dO,
                           const int* valid, const float* bias, const float* lse,
                           const float* Dterm, bf16* dK, bf16* dV, int B, int H,
                           int Lq, int Lk, float scale, int causal, unsigned p8,
                           unsigned long long seed, long ldq, long ldkv, long ldout,
                           hipStream_t stream) {
  const dim3 grid((Lk + TK - 1) / TK, B * H);
  const size_t lds = 2 * TK * 128 + 18432;  // 34816 B
  hipLaunchKernelGGL(flash_rect_dkv_kernel, grid, dim3(256), lds, stream, Q, K, V, dO,
                     valid, bias, lse, Dterm, dK, dV, H, Lq, Lk, scale, causal, p8,
                     seed, ldq, ldkv, ldout);
}
