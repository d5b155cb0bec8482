// Flash attention for MI355X (gfx950), head_dim = 64.
//
// Replaces the materialized-P attention path (QK^T bmm + softmax + P@V bmm
// + the layout transposes around them — together ~10 ms of the 27 ms
// LineVul step, rocprof in profiles/) with one fused kernel per direction.
//
// Shapes: Q/K/V/O are (B, L, H*64) — the projections' natural output — so
// no transpose/contiguous copies exist anywhere in the attention path.
// Supports: suffix-padding valid lengths per batch row, causal masking
// (T5 decoder), additive position bias (T5 relative attention, fp32,
// stored TRANSPOSED key-major (H, Lk, Lq) so the 16 q-column lanes of an
// unrolled load share one 64-B line — models/t5.py _flash_bias_T),
// fused stateless dropout (mask regenerated in backward),
// softmax scale, and the log-sum-exp save for the backward pass.
//
// Tiling (cdna_hip_programming.md §B attention ladder, adapted to d=64):
// one block = 4 waves = 128 query rows of one (b, h); KV tiles of 64 keys
// staged in LDS (K natural [key][d] with XOR swizzle; V transposed to
// [d][key] at staging so the PV B-fragments are contiguous reads).
// v_mfma_f32_16x16x32_bf16 throughout; swapped-operand QK^T
// (S^T = mfma(K, Q)) keeps the softmax row statistics lane-local to a
// 16-lane column group (two shfl_xor hops per reduction).

#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>

#define WAVE 64
#define TK 64    // keys per KV tile
#define TQW 32   // query rows per wave
#define NWAVE 4  // waves per block -> 128 q rows per block

using bf16 = __hip_bfloat16;
using bf16x8 = __attribute__((ext_vector_type(8))) __bf16;
using f32x4 = __attribute__((ext_vector_type(4))) float;
using uint4v = __attribute__((ext_vector_type(4))) unsigned int;

__device__ __forceinline__ unsigned fa_hash4(unsigned long long quad_idx,
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

__device__ __forceinline__ bool fa_keep(unsigned long long idx,
                                        unsigned long long seed, unsigned p8) {
  const unsigned h = fa_hash4(idx >> 2, seed);
  return ((h >> (8 * ((unsigned)idx & 3))) & 0xFF) >= p8;
}

// LDS addressing: 128-B rows, XOR swizzle vs 16-lane b128 fragment groups
__device__ __forceinline__ int fa_swz(int row, int byte) {
  return row * 128 + (byte ^ ((row & 7) << 4));
}

// Swizzle for the TRANSPOSED ([d][key]) images. Their scalar staging
// writes have d = (lane&7)*8 + j, i.e. d&7 is constant per instruction —
// with the fa_swz map all 64 lanes land in a 4-dword window (16-way
// conflict). XOR on d>>3 instead: the staging writes then spread over all
// 32 banks, and the b128 fragment reads (d = fd*16 + (lane&15)) stay at
// their previous ~2-way worst case.
__device__ __forceinline__ int fa_swzT(int row, int byte) {
  return row * 128 + (byte ^ (((row >> 3) & 7) << 4));
}

// fwd V image: [4 key][16 d] row-major bf16 subtiles padded 128->144 B for
// ds_read_b64_tr_b16 hardware-transpose reads (same verified layout as
// csrc/wgrad2.hip / tools/tr_probe): staging V is then a 16-B vector write
// per 8 elements (the old transposed image needed 8 scalar 2-B writes —
// the fwd loop-head's dominant cost per the FSEG profile), and each PV
// B-fragment is 2 tr reads.
#define FWD_VSUB(kb, db) (((kb) * 4 + (db)) * 144)
#define FWD_VBYTES ((TK / 4) * 4 * 144)
using fwd_bf16x4v = __attribute__((ext_vector_type(4))) __bf16;
typedef __attribute__((address_space(3))) fwd_bf16x4v fwd_lds_bf16x4;

// fwd segment accumulator (env DFA_FWD_PROF=1 selects the instrumented
// instantiation)
__device__ unsigned long long dfa_fwd_prof[8];

// NW = waves per block (8 preferred for L >= 256: K/V staging, barriers
// and tile loads amortize over 2x the query rows; 4-wave fallback keeps
// short-sequence grids filled)
template <int PROF, int NW>
__global__ __launch_bounds__(NW * 64, 12 / NW) void flash_fwd_kernel(
    const bf16* __restrict__ Q, const bf16* __restrict__ K,
    const bf16* __restrict__ V, const int* __restrict__ valid,
    const float* __restrict__ bias, bf16* __restrict__ O,
    float* __restrict__ lse, int B, int H, int L, float scale, int causal,
    unsigned p8, unsigned long long seed, long ldq, long ldkv) {
  // ldq/ldkv: row strides (elements) of the Q and K/V inputs — H*64 for
  // contiguous tensors, 3*H*64 when they are slices of a fused QKV buffer
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* k_lds = smem;                // [TK][64] bf16 swizzled = 8 KiB
  char* v_lds = smem + TK * 128;     // [TK/4][4 key x 16 d] tr16 subtiles

  // XCD-affine remap: with the natural (x=tile, y=b*H+h) order the B
  // blocks that re-read one bias slice bias[h, tile rows, :] scatter
  // across XCDs and the ~B-fold (H, L, L) fp32 bias re-read misses L2.
  // Deriving (b, h, tile) from the linear dispatch id as id = b*S + slice
  // (S = gridDim.x*H) makes same-slice blocks id-congruent mod S; since
  // workgroups round-robin across the 8 XCDs, S % 8 == 0 pins each slice's
  // B blocks to ONE XCD whose L2 then serves the repeats.
  const int lid = blockIdx.y * gridDim.x + blockIdx.x;
  const int S = gridDim.x * H;
  const int b = lid / S;
  const int h = (lid % S) / gridDim.x;
  const int q0 = ((lid % S) % gridDim.x) * (NW * TQW);
  const int bh = b * H + h;
  const int tid = threadIdx.x;
  const int lane = tid & (WAVE - 1);
  const int wid = tid >> 6;
  const int qw = q0 + wid * TQW;      // this wave's first q row
  const long HD = (long)H * 64;
  const int vl = valid ? valid[b] : L;

  // ---- load Q fragments (B-operand layout: lane holds Q[qrow][8 d]) ----
  // frag index [fq][ks]: qrow = qw + fq*16 + (lane&15), d = ks*32 + (lane>>4)*8
  bf16x8 q_frag[2][2];
  const bool q_full = (qw + TQW) <= L;  // uniform: avoids per-load branches
#pragma unroll
  for (int fq = 0; fq < 2; ++fq) {
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      const int qrow = qw + fq * 16 + (lane & 15);
      const int d = ks * 32 + (lane >> 4) * 8;
      if (q_full)
        q_frag[fq][ks] = *reinterpret_cast<const bf16x8*>(
            Q + ((long)b * L + qrow) * ldq + (long)h * 64 + d);
      else if (qrow < L)
        q_frag[fq][ks] = *reinterpret_cast<const bf16x8*>(
            Q + ((long)b * L + qrow) * ldq + (long)h * 64 + d);
      else
        q_frag[fq][ks] = bf16x8{};
    }
  }

  unsigned long long fsegt[8] = {};
  unsigned long long fseg_last = PROF ? __builtin_readcyclecounter() : 0;
#define FSEG(i)                                                  \
  if (PROF) {                                                    \
    unsigned long long now = __builtin_readcyclecounter();       \
    fsegt[i] += now - fseg_last;                                 \
    fseg_last = now;                                             \
  }
  // softmax state per (fq, its lane-column qrow)
  float m_st[2] = {-3.4e38f, -3.4e38f};
  float l_st[2] = {0.f, 0.f};
  f32x4 o_acc[2][4] = {};  // [fq][fd]: O rows (l>>4)*4+i of fq block, col fd*16+(l&15)

  // T14 double-buffered K/V staging: next tile's global loads issue before
  // this tile's MFMAs; one barrier per tile (write targets the buffer the
  // NEXT iteration reads — no same-buffer hazard)
  const int kv_end = causal ? min(vl, q0 + NW * TQW) : vl;
  constexpr int SROWS = NW * 8;        // staging rows per pass
  constexpr int NPASS = TK / SROWS;
  const int srow = tid >> 3;           // staging: 0..SROWS-1
  const int soff = (tid & 7) * 16;     // byte offset (8 bf16)
  auto load_tile = [&](int kv0, uint4v kreg[NPASS], uint4v vreg[NPASS]) {
    const bool kv_full = (kv0 + TK) <= vl;  // uniform fast path
#pragma unroll
    for (int rr = 0; rr < NPASS; ++rr) {
      const int key = kv0 + srow + rr * SROWS;
      kreg[rr] = {};
      vreg[rr] = {};
      if (kv_full) {
        kreg[rr] = *reinterpret_cast<const uint4v*>(
            K + ((long)b * L + key) * ldkv + (long)h * 64 + soff / 2);
        vreg[rr] = *reinterpret_cast<const uint4v*>(
            V + ((long)b * L + key) * ldkv + (long)h * 64 + soff / 2);
      } else if (key < vl) {
        kreg[rr] = *reinterpret_cast<const uint4v*>(
            K + ((long)b * L + key) * ldkv + (long)h * 64 + soff / 2);
        vreg[rr] = *reinterpret_cast<const uint4v*>(
            V + ((long)b * L + key) * ldkv + (long)h * 64 + soff / 2);
      }
    }
  };
  auto write_tile = [&](char* kb, char* vb, const uint4v kreg[NPASS],
                        const uint4v vreg[NPASS]) {
#pragma unroll
    for (int rr = 0; rr < NPASS; ++rr) {
      *reinterpret_cast<uint4v*>(kb + fa_swz(srow + rr * SROWS, soff)) = kreg[rr];
      const int key = srow + rr * SROWS;
      const int d0 = soff / 2;
      *reinterpret_cast<uint4v*>(vb + FWD_VSUB(key >> 2, d0 >> 4) +
                                 (key & 3) * 32 + (d0 & 15) * 2) = vreg[rr];
    }
  };
#define K_BUF(i) (k_lds + (i) * (TK * 128 + FWD_VBYTES))
#define V_BUF(i) (v_lds + (i) * (TK * 128 + FWD_VBYTES))
  uint4v kreg[NPASS], vreg[NPASS];
  int cur = 0;
  // this lane's two query columns. With L % 128 == 64 the last query block
  // has waves that lie wholly past L (qw and L are multiples of TQW); their
  // scores are masked below, but bias[.. + qcol] would be read up to 63
  // columns past the (H, L, L) allocation. Clamp the wave's column window to
  // [L - TQW, L - 1] instead: qshift is wave-uniform, so it folds into the
  // scalar base pointer and the key loop gains neither an instruction nor a
  // VGPR (a per-lane min(qcol, L - 1) cost two, and 0.25 % of a T5 step).
  const int qcol[2] = {qw + (lane & 15), qw + 16 + (lane & 15)};
  const int qshift = (qw < L) ? 0 : qw + TQW - L;
  const float* bias_h = bias ? bias + (long)h * L * L - qshift : nullptr;
  if (kv_end > 0) {
    load_tile(0, kreg, vreg);
    write_tile(K_BUF(0), V_BUF(0), kreg, vreg);
  }
  __syncthreads();
  for (int kv0 = 0; kv0 < kv_end; kv0 += TK) {
    const bool has_next = (kv0 + TK) < kv_end;
    FSEG(0)  // loop head
    if (has_next) load_tile(kv0 + TK, kreg, vreg);
    char* k_lds_c = K_BUF(cur);
    char* v_lds_c = V_BUF(cur);
    FSEG(1)  // next-tile load issue
    if (has_next) write_tile(K_BUF(cur ^ 1), V_BUF(cur ^ 1), kreg, vreg);

    // ---- S^T = K @ Q^T : D[key][qrow] ----
    f32x4 s_acc[4][2] = {};  // [fkey][fq]
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      bf16x8 k_frag[4];
#pragma unroll
      for (int fk = 0; fk < 4; ++fk) {
        const int key = fk * 16 + (lane & 15);
        const int kbyte = ks * 64 + (lane >> 4) * 16;
        k_frag[fk] = *reinterpret_cast<const bf16x8*>(k_lds_c + fa_swz(key, kbyte));
      }
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int fk = 0; fk < 4; ++fk)
#pragma unroll
        for (int fq = 0; fq < 2; ++fq)
          s_acc[fk][fq] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              k_frag[fk], q_frag[fq][ks], s_acc[fk][fq], 0, 0, 0);
      __builtin_amdgcn_s_setprio(0);
    }
    FSEG(2)  // QK^T MFMAs (+k_frag reads)

    // ---- masking + bias + tile row-max (over keys, per qrow column) ----
    // scores -> probabilities transform IN s_acc: a separate p[4][2][4]
    // copy cost 32 VGPRs (232 total = 2 waves/SIMD; the kernel is
    // latency-bound at that occupancy, PMC WAIT_ANY 35%)
    float tile_max[2] = {-3.4e38f, -3.4e38f};
#pragma unroll
    for (int fk = 0; fk < 4; ++fk)
#pragma unroll
      for (int fq = 0; fq < 2; ++fq)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int key = kv0 + fk * 16 + (lane >> 4) * 4 + i;
          float s = s_acc[fk][fq][i] * scale;
          // bias is stored TRANSPOSED (H, key, qcol): the 16 qcol lanes of
        // one unrolled load hit one 64-B line (row-major (H, q, key) made
        // every lane fetch its own line: measured ~half the biased
        // kernel's time, tools/flash_bias_probe.py)
        if (bias) s += bias_h[(long)key * L + qcol[fq]];
          const bool masked = key >= vl || (causal && key > qcol[fq]) || qcol[fq] >= L;
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
    FSEG(3)  // mask + max + exp + sums (softmax VALU/shfl)

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
                ((unsigned long long)(bh)*L + qcol[fq]) * L + key;
            s_acc[fk][fq][i] = fa_keep(idx, seed, p8) ? s_acc[fk][fq][i] * dscale : 0.f;
          }
    }

    // ---- rescale O by alpha (per O-row qrow = (l>>4)*4 + i) ----
#pragma unroll
    for (int fq = 0; fq < 2; ++fq)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int qrow16 = (lane >> 4) * 4 + i;
        const float a = __shfl(alpha[fq], qrow16);
#pragma unroll
        for (int fd = 0; fd < 4; ++fd) o_acc[fq][fd][i] *= a;
      }
    FSEG(4)  // dropout + O rescale

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
          // register indices must be compile-time (rule 20); the source
          // fragment differs only between lane halves -> shuffle both
          // candidate registers and select
          const float v0 = __shfl(s_acc[kp * 2][fq][j & 3], src);
          const float v1 = __shfl(s_acc[kp * 2 + 1][fq][j & 3], src);
          pa[fq][j] = (__bf16)(hi_half ? v1 : v0);
        }
      }
      FSEG(5)  // P exchange (shfl)
      bf16x8 v_frag[4];
      const int kb0 = kp * 8 + (lane >> 4) * 2;
      const int vslot = (lane & 15) * 8;
#pragma unroll
      for (int fd = 0; fd < 4; ++fd) {
        fwd_bf16x4v* vf = reinterpret_cast<fwd_bf16x4v*>(&v_frag[fd]);
        vf[0] = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(
            (fwd_lds_bf16x4*)(v_lds_c + FWD_VSUB(kb0, fd) + vslot));
        vf[1] = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(
            (fwd_lds_bf16x4*)(v_lds_c + FWD_VSUB(kb0 + 1, fd) + vslot));
      }
#pragma unroll
      for (int fq = 0; fq < 2; ++fq)
#pragma unroll
        for (int fd = 0; fd < 4; ++fd)
          o_acc[fq][fd] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              pa[fq], v_frag[fd], o_acc[fq][fd], 0, 0, 0);
    }
    FSEG(6)  // v_frag reads + PV MFMAs
    __syncthreads();
    cur ^= 1;
  }
#undef K_BUF
#undef V_BUF

  // ---- epilogue: O /= l via a wave-local LDS bounce (the direct form is
  // 32 scalar 2-B stores per lane — 24% of the kernel, FSEG profile);
  // all waves passed the loop's final barrier, so the K/V buffers are free
  char* obuf = smem + wid * 4096;  // [32 rows][64 d] bf16, fa_swz'd
#pragma unroll
  for (int fq = 0; fq < 2; ++fq) {
    const float inv_l = (l_st[fq] > 0.f) ? 1.0f / l_st[fq] : 0.f;
    if ((lane >> 4) == 0 && lse) {
      const int qrow = qw + fq * 16 + (lane & 15);
      if (qrow < L)
        lse[((long)bh) * L + qrow] =
            (l_st[fq] > 0.f) ? m_st[fq] + __logf(l_st[fq]) : 0.f;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int row_loc = fq * 16 + (lane >> 4) * 4 + i;
      const float il = __shfl(inv_l, (lane >> 4) * 4 + i);
#pragma unroll
      for (int fd = 0; fd < 4; ++fd) {
        const int d = fd * 16 + (lane & 15);
        *reinterpret_cast<bf16*>(obuf + fa_swz(row_loc & 31, d * 2)) =
            __float2bfloat16(o_acc[fq][fd][i] * il);
      }
    }
    // wave-local buffer: only lgkm ordering needed (same wave reads)
#pragma unroll
    for (int pp = 0; pp < 2; ++pp) {
      const int row_loc = fq * 16 + pp * 8 + (lane >> 3);
      const int qrow = qw + row_loc;
      if (qrow < L) {
        const uint4v vvv = *reinterpret_cast<const uint4v*>(
            obuf + fa_swz(row_loc & 31, (lane & 7) * 16));
        *reinterpret_cast<uint4v*>(
            O + ((long)b * L + qrow) * HD + (long)h * 64 + (lane & 7) * 8) = vvv;
      }
    }
  }
  FSEG(7)  // epilogue
  if (PROF && lane == 0) {
#pragma unroll
    for (int i = 0; i < 8; ++i) atomicAdd(&dfa_fwd_prof[i], fsegt[i]);
  }
#undef FSEG
}

// ---------------------------------------------------------------------------
// Backward. Standard FA2 two-pass split so every output is owned by exactly
// one block (no global atomics on dQ/dK/dV):
//   * Dterm kernel: D[b,h,q] = sum_d dO * O  (needed by both passes; equals
//     rowsum(Pd o dPd), which the dropout mask cancels out of)
//   * dq kernel:  grid (q-tile, bh), loops KV tiles, accumulates dQ in regs
//   * dkv kernel: grid (kv-tile, bh), loops Q strips, accumulates dK/dV in
//     regs, cross-wave reduce through LDS
// T5's additive position bias gets its gradient via fp32 atomicAdd from the
// dq pass (B adds per element).
// ---------------------------------------------------------------------------

__global__ void flash_dterm_kernel(const bf16* __restrict__ dO,
                                   const bf16* __restrict__ O,
                                   float* __restrict__ Dterm, int B, int H,
                                   int L) {
  // 8 lanes per 64-element (b, q, h) row via 16-B loads -> 8 rows per wave
  // (the 1-row-per-wave form was ~17 instructions per 256 B of traffic and
  // ran 5x off the copy roofline)
  const int lane = threadIdx.x & (WAVE - 1);
  const int sub = lane >> 3;  // row slot within the wave
  const int sl = lane & 7;    // lane within the row
  const long R = (long)B * L * H;
  const long row =
      ((long)blockIdx.x * (blockDim.x / WAVE) + threadIdx.x / WAVE) * 8 + sub;
  if (row >= R) return;  // row = ((b*L + q)*H + h)
  const long base = row * 64 + sl * 8;
  const bf16x8 a = *reinterpret_cast<const bf16x8*>(dO + base);
  const bf16x8 o = *reinterpret_cast<const bf16x8*>(O + base);
  float acc = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) acc += (float)a[j] * (float)o[j];
  acc += __shfl_down(acc, 4);
  acc += __shfl_down(acc, 2);
  acc += __shfl_down(acc, 1);
  if (sl == 0) {
    const long bq = row / H;
    const int h = (int)(row % H);
    const long b = bq / L;
    const long q = bq % L;
    Dterm[((b * H + h) * L) + q] = acc;
  }
}

// recompute P^T for one (wave q-strip, kv tile): returns scores in p[4][2][4]
// D-layout (key = fk*16 + (lane>>4)*4 + i, qrow-col = fq*16 + (lane&15)).
// Shared by the dq and dkv kernels.
__device__ __forceinline__ void recompute_pT(
    const char* k_lds, const bf16x8 q_frag[2][2], const float* __restrict__ bias,
    const float lse_w[2], int lane, int h, int L, int qw, int kv0,
    int vl, float scale, int causal, float p[4][2][4]) {
  // a wave wholly past L (partial last q block, masked below) reads the
  // bias through a column window clamped to [L - TQW, L - 1]: see the forward
  const int qshift = (qw < L) ? 0 : qw + TQW - L;
  f32x4 s_acc[4][2] = {};
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) {
    bf16x8 k_frag[4];
#pragma unroll
    for (int fk = 0; fk < 4; ++fk) {
      const int key = fk * 16 + (lane & 15);
      const int kbyte = ks * 64 + (lane >> 4) * 16;
      k_frag[fk] = *reinterpret_cast<const bf16x8*>(k_lds + fa_swz(key, kbyte));
    }
#pragma unroll
    for (int fk = 0; fk < 4; ++fk)
#pragma unroll
      for (int fq = 0; fq < 2; ++fq)
        s_acc[fk][fq] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            k_frag[fk], q_frag[fq][ks], s_acc[fk][fq], 0, 0, 0);
  }
#pragma unroll
  for (int fk = 0; fk < 4; ++fk)
#pragma unroll
    for (int fq = 0; fq < 2; ++fq) {
      const int qcol = qw + fq * 16 + (lane & 15);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int key = kv0 + fk * 16 + (lane >> 4) * 4 + i;
        float s = s_acc[fk][fq][i] * scale;
        if (bias) s += bias[((long)h * L + key) * L + qcol - qshift];  // (H, key, qcol) layout
        const bool masked = key >= vl || (causal && key > qcol) || qcol >= L;
        p[fk][fq][i] = masked ? 0.f : __expf(s - lse_w[fq]);
      }
    }
}

__global__ __launch_bounds__(256) void flash_dq_kernel(
    const bf16* __restrict__ Q, const bf16* __restrict__ K,
    const bf16* __restrict__ V, const bf16* __restrict__ dO,
    const int* __restrict__ valid, const float* __restrict__ bias,
    const float* __restrict__ lse, const float* __restrict__ Dterm,
    bf16* __restrict__ dQ, float* __restrict__ dBias, int B, int H, int L,
    float scale, int causal, unsigned p8, unsigned long long seed, long ldq,
    long ldkv, long ldout) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* k_lds = smem;                 // [key][d] swizzled, 8 KiB
  char* kt_lds = smem + TK * 128;     // [d][key] swizzled, 8 KiB
  char* v_lds = smem + 2 * TK * 128;  // [key][d] swizzled, 8 KiB

  const int lid = blockIdx.y * gridDim.x + blockIdx.x;  // XCD-affine (see fwd)
  const int S = gridDim.x * H;
  const int b = lid / S;
  const int h = (lid % S) / gridDim.x;
  const int q0 = ((lid % S) % gridDim.x) * (NWAVE * TQW);
  const int bh = b * H + h;
  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x >> 6;
  const int qw = q0 + wid * TQW;
  const long HD = (long)H * 64;
  const int vl = valid ? valid[b] : L;
  const float dscale = (p8 > 0) ? 256.0f / (256.0f - p8) : 1.0f;

  bf16x8 q_frag[2][2], do_frag[2][2];
  const bool q_full = (qw + TQW) <= L;
#pragma unroll
  for (int fq = 0; fq < 2; ++fq)
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      const int qrow = qw + fq * 16 + (lane & 15);
      const int d = ks * 32 + (lane >> 4) * 8;
      const long baseq = ((long)b * L + qrow) * ldq + (long)h * 64 + d;
      const long baseo = ((long)b * L + qrow) * HD + (long)h * 64 + d;
      if (q_full) {
        q_frag[fq][ks] = *reinterpret_cast<const bf16x8*>(Q + baseq);
        do_frag[fq][ks] = *reinterpret_cast<const bf16x8*>(dO + baseo);
      } else if (qrow < L) {
        q_frag[fq][ks] = *reinterpret_cast<const bf16x8*>(Q + baseq);
        do_frag[fq][ks] = *reinterpret_cast<const bf16x8*>(dO + baseo);
      } else {
        q_frag[fq][ks] = bf16x8{};
        do_frag[fq][ks] = bf16x8{};
      }
    }
  float lse_w[2], dterm_w[2];
#pragma unroll
  for (int fq = 0; fq < 2; ++fq) {
    const int qrow = qw + fq * 16 + (lane & 15);
    lse_w[fq] = (qrow < L) ? lse[(long)bh * L + qrow] : 0.f;
    dterm_w[fq] = (qrow < L) ? Dterm[(long)bh * L + qrow] : 0.f;
  }

  f32x4 dq_acc[2][4] = {};  // [fq][fd]: rows (l>>4)*4+i, col fd*16+(l&15)

  // T14 double-buffered staging of K (nat + transposed) and V (nat)
  const int kv_end = causal ? min(vl, q0 + NWAVE * TQW) : vl;
  const int srow = threadIdx.x >> 3;
  const int soff = (threadIdx.x & 7) * 16;
  auto dq_load = [&](int kv0, uint4v kreg[2], uint4v vreg[2]) {
    const bool kv_full = (kv0 + TK) <= vl;
#pragma unroll
    for (int rr = 0; rr < 2; ++rr) {
      const int key = kv0 + srow + rr * 32;
      kreg[rr] = {};
      vreg[rr] = {};
      if (kv_full) {
        kreg[rr] = *reinterpret_cast<const uint4v*>(
            K + ((long)b * L + key) * ldkv + (long)h * 64 + soff / 2);
        vreg[rr] = *reinterpret_cast<const uint4v*>(
            V + ((long)b * L + key) * ldkv + (long)h * 64 + soff / 2);
      } else if (key < vl) {
        kreg[rr] = *reinterpret_cast<const uint4v*>(
            K + ((long)b * L + key) * ldkv + (long)h * 64 + soff / 2);
        vreg[rr] = *reinterpret_cast<const uint4v*>(
            V + ((long)b * L + key) * ldkv + (long)h * 64 + soff / 2);
      }
    }
  };
  auto dq_write = [&](char* kb, char* ktb, char* vb, const uint4v kreg[2],
                      const uint4v vreg[2]) {
#pragma unroll
    for (int rr = 0; rr < 2; ++rr) {
      *reinterpret_cast<uint4v*>(kb + fa_swz(srow + rr * 32, soff)) = kreg[rr];
      *reinterpret_cast<uint4v*>(vb + fa_swz(srow + rr * 32, soff)) = vreg[rr];
      bf16 kk[8];
      *reinterpret_cast<uint4v*>(kk) = kreg[rr];
      const int d0 = soff / 2;
#pragma unroll
      for (int j = 0; j < 8; ++j)
        *reinterpret_cast<bf16*>(ktb + fa_swzT(d0 + j, (srow + rr * 32) * 2)) =
            kk[j];
    }
  };
#define DQ_BUF(base, i) ((base) + (i)*3 * TK * 128)
  uint4v kreg[2], vreg[2];
  int cur = 0;
  if (kv_end > 0) {
    dq_load(0, kreg, vreg);
    dq_write(DQ_BUF(k_lds, 0), DQ_BUF(kt_lds, 0), DQ_BUF(v_lds, 0), kreg, vreg);
  }
  __syncthreads();
  for (int kv0 = 0; kv0 < kv_end; kv0 += TK) {
    const bool has_next = (kv0 + TK) < kv_end;
    if (has_next) dq_load(kv0 + TK, kreg, vreg);
    char* k_lds_c = DQ_BUF(k_lds, cur);
    char* kt_lds_c = DQ_BUF(kt_lds, cur);
    char* v_lds_c = DQ_BUF(v_lds, cur);

    float p[4][2][4];
    recompute_pT(k_lds_c, q_frag, bias, lse_w, lane, h, L, qw, kv0, vl, scale,
                 causal, p);

    // dPd^T = V dO^T (same structure as S^T), then ds
    f32x4 dp_acc[4][2] = {};
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      bf16x8 v_frag[4];
#pragma unroll
      for (int fk = 0; fk < 4; ++fk) {
        const int key = fk * 16 + (lane & 15);
        const int kbyte = ks * 64 + (lane >> 4) * 16;
        v_frag[fk] = *reinterpret_cast<const bf16x8*>(v_lds_c + fa_swz(key, kbyte));
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
                ((unsigned long long)(bh)*L + qcol) * L + key;
            dp = fa_keep(idx, seed, p8) ? dp * dscale : 0.f;
          }
          ds[fk][fq][i] = p[fk][fq][i] * (dp - dterm_w[fq]);
          if (dBias && ds[fk][fq][i] != 0.f)
            atomicAdd(dBias + ((long)h * L + key) * L + qcol, ds[fk][fq][i]);
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
        kt_frag[fd] = *reinterpret_cast<const bf16x8*>(kt_lds_c + fa_swzT(d, keybyte));
      }
#pragma unroll
      for (int fq = 0; fq < 2; ++fq)
#pragma unroll
        for (int fd = 0; fd < 4; ++fd)
          dq_acc[fq][fd] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              dsa[fq], kt_frag[fd], dq_acc[fq][fd], 0, 0, 0);
    }
    if (has_next)
      dq_write(DQ_BUF(k_lds, cur ^ 1), DQ_BUF(kt_lds, cur ^ 1),
               DQ_BUF(v_lds, cur ^ 1), kreg, vreg);
    __syncthreads();
    cur ^= 1;
  }
#undef DQ_BUF

  // write dQ (B, L, H*64)
#pragma unroll
  for (int fq = 0; fq < 2; ++fq)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int qrow = qw + fq * 16 + (lane >> 4) * 4 + i;
      if (qrow >= L) continue;
#pragma unroll
      for (int fd = 0; fd < 4; ++fd) {
        const int d = fd * 16 + (lane & 15);
        dQ[((long)b * L + qrow) * ldout + (long)h * 64 + d] =
            __float2bfloat16(dq_acc[fq][fd][i]);
      }
    }
}

// recompute P^T for a 32-key half-tile: p[2][2][4], keys key_off + fk*16 + ...
__device__ __forceinline__ void recompute_pT32(
    const char* k_lds, const bf16x8 q_frag[2][2], const float* __restrict__ bias,
    const float lse_w[2], int lane, int h, int L, int qw, int kv0, int key_off,
    int vl, float scale, int causal, float p[2][2][4]) {
  f32x4 s_acc[2][2] = {};
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) {
    bf16x8 k_frag[2];
#pragma unroll
    for (int fk = 0; fk < 2; ++fk) {
      const int key = key_off + fk * 16 + (lane & 15);
      const int kbyte = ks * 64 + (lane >> 4) * 16;
      k_frag[fk] = *reinterpret_cast<const bf16x8*>(k_lds + fa_swz(key, kbyte));
    }
#pragma unroll
    for (int fk = 0; fk < 2; ++fk)
#pragma unroll
      for (int fq = 0; fq < 2; ++fq)
        s_acc[fk][fq] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            k_frag[fk], q_frag[fq][ks], s_acc[fk][fq], 0, 0, 0);
  }
#pragma unroll
  for (int fk = 0; fk < 2; ++fk)
#pragma unroll
    for (int fq = 0; fq < 2; ++fq) {
      const int qcol = qw + fq * 16 + (lane & 15);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int key = kv0 + key_off + fk * 16 + (lane >> 4) * 4 + i;
        float sc = s_acc[fk][fq][i] * scale;
        if (bias) sc += bias[((long)h * L + key) * L + qcol];  // (H, key, qcol) layout
        const bool masked = key >= vl || (causal && key > qcol) || qcol >= L;
        p[fk][fq][i] = masked ? 0.f : __expf(sc - lse_w[fq]);
      }
    }
}

// dO^T/Q^T bounce image (variant 2): per-wave [d 64][q 32] bf16 rows padded
// to 72 B so the 16-B B-fragment reads spread across the 64-dword bank
// modulus instead of 4-way conflicting at a 64-B stride.
#define DKV_T_STRIDE 72
#define DKV_T_BYTES (64 * DKV_T_STRIDE)

// variant 6: [4 q][16 d] subtiles (144-B padded) for ds_read_b64_tr_b16
// B-fragment reads (see csrc/wgrad2.hip / tools/tr_probe): staging is 16-B
// vector writes straight from the q/dO fragments, reads are 2 tr reads per
// fragment — replaces the 64 scalar L1 transposed loads per strip
#define DKV_SUB(kb, cb) (((kb)*4 + (cb)) * 144)
using bf16x4v = __attribute__((ext_vector_type(4))) __bf16;
typedef __attribute__((address_space(3))) bf16x4v lds_bf16x4;

// variant-9 instrumentation accumulator (cycles per kernel segment)
__device__ unsigned long long dfa_dkv_prof[8];

template <int VAR>
__global__ __launch_bounds__(256) void flash_dkv_kernel(
    const bf16* __restrict__ Q, const bf16* __restrict__ K,
    const bf16* __restrict__ V, const bf16* __restrict__ dO,
    const int* __restrict__ valid, const float* __restrict__ bias,
    const float* __restrict__ lse, const float* __restrict__ Dterm,
    bf16* __restrict__ dK, bf16* __restrict__ dV, int B, int H, int L,
    float scale, int causal, unsigned p8, unsigned long long seed, long ldq,
    long ldkv, long ldout) {
  // Wave grid 2 (key halves) x 2 (q interleave): halves the per-wave
  // accumulator footprint (the 64-key variant needed 128 fp32 accumulators
  // on top of ~176 VGPRs -> 1 wave/SIMD on the unified register file).
  // LDS map: K nat 8K | V nat 8K | per-wave pd 2K, ds 2K (reused as the
  // fp32 reduction buffer afterwards) | VAR 2 only: per-wave doT/qT images.
  // Variants (within-probe A/B, see profiles/flash_dkv_pmc.md):
  //   0 = direct L1 scalar dob/qb loads
  //   2 = 0 with the transposed fragments bounced through LDS (vector reads)
  //   3 = 0 + s_setprio(1) on the younger wave half through the MFMA loop
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* k_lds = smem;
  char* v_lds = smem + TK * 128;
  char* wave_base = smem + 2 * TK * 128;

  const int lid = blockIdx.y * gridDim.x + blockIdx.x;  // XCD-affine (see fwd)
  const int S = gridDim.x * H;
  const int b = lid / S;
  const int h = (lid % S) / gridDim.x;
  const int kv0 = ((lid % S) % gridDim.x) * TK;
  const int bh = b * H + h;
  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x >> 6;
  const int wk = wid >> 1;   // key half: keys wk*32 .. wk*32+31
  const int wq = wid & 1;    // q interleave
  const int key_off = wk * 32;
  const long HD = (long)H * 64;
  const int vl = valid ? valid[b] : L;
  const float dscale = (p8 > 0) ? 256.0f / (256.0f - p8) : 1.0f;
  // pd/ds rows padded to 72 B: at 64 B the scalar writes put all four
  // (lane>>4) key groups (4 rows * 16 dwords = 0 mod 32) on the same 8
  // banks; 72 B (18 dwords) staggers the groups by 8 banks each
  char* pd_lds = wave_base + wid * 2304;
  char* ds_lds = wave_base + 9216 + wid * 2304;
  char* dot_lds = wave_base + 18432 + wid * 2 * DKV_T_BYTES;
  char* qt_lds = dot_lds + DKV_T_BYTES;
  if (VAR == 3 && __builtin_amdgcn_readfirstlane(threadIdx.x) >= 128)
    __builtin_amdgcn_s_setprio(1);

  {  // stage K and V tiles (natural layout, swizzled)
    const int row = threadIdx.x >> 3;
    const int off = (threadIdx.x & 7) * 16;
    const bool kv_full = (kv0 + TK) <= vl;
#pragma unroll
    for (int rr = 0; rr < TK; rr += 32) {
      const int key = kv0 + row + rr;
      uint4v kv = {}, vv = {};
      if (kv_full) {
        kv = *reinterpret_cast<const uint4v*>(
            K + ((long)b * L + key) * ldkv + (long)h * 64 + off / 2);
        vv = *reinterpret_cast<const uint4v*>(
            V + ((long)b * L + key) * ldkv + (long)h * 64 + off / 2);
      } else if (key < vl && kv0 < vl) {
        kv = *reinterpret_cast<const uint4v*>(
            K + ((long)b * L + key) * ldkv + (long)h * 64 + off / 2);
        vv = *reinterpret_cast<const uint4v*>(
            V + ((long)b * L + key) * ldkv + (long)h * 64 + off / 2);
      }
      *reinterpret_cast<uint4v*>(k_lds + fa_swz(row + rr, off)) = kv;
      *reinterpret_cast<uint4v*>(v_lds + fa_swz(row + rr, off)) = vv;
    }
  }
  __syncthreads();

  f32x4 dv_acc[2][4] = {};  // [fkey][fd] over this wave's 32-key half
  f32x4 dk_acc[2][4] = {};

  // VAR 9: per-segment cycle instrumentation (s_memtime; guide §5.4 —
  // ~+11% overhead, relative shares are what matters)
  unsigned long long segt[8] = {};
  unsigned long long seg_last = (VAR == 9) ? __builtin_readcyclecounter() : 0;
#define SEG_MARK(i)                                          \
  if (VAR == 9) {                                            \
    unsigned long long now = __builtin_readcyclecounter();   \
    segt[i] += now - seg_last;                               \
    seg_last = now;                                          \
  }

  if (kv0 < vl) {
    const int q_begin = causal ? kv0 : 0;  // kv0 is a multiple of 32
    const int nstrips = (L - q_begin + TQW - 1) / TQW;
    bf16x8 q_frag[2][2], do_frag[2][2];
    for (int strip = wq; strip < nstrips; strip += 2) {
      const int qw = q_begin + strip * TQW;
      const bool q_full = (qw + TQW) <= L;
      SEG_MARK(7)  // loop overhead / previous-iteration tail
#pragma unroll
      for (int fq = 0; fq < 2; ++fq)
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
          const int qrow = qw + fq * 16 + (lane & 15);
          const int d = ks * 32 + (lane >> 4) * 8;
          const long baseq = ((long)b * L + qrow) * ldq + (long)h * 64 + d;
          const long baseo = ((long)b * L + qrow) * HD + (long)h * 64 + d;
          if (q_full) {
            q_frag[fq][ks] = *reinterpret_cast<const bf16x8*>(Q + baseq);
            do_frag[fq][ks] = *reinterpret_cast<const bf16x8*>(dO + baseo);
          } else if (qrow < L) {
            q_frag[fq][ks] = *reinterpret_cast<const bf16x8*>(Q + baseq);
            do_frag[fq][ks] = *reinterpret_cast<const bf16x8*>(dO + baseo);
          } else {
            q_frag[fq][ks] = bf16x8{};
            do_frag[fq][ks] = bf16x8{};
          }
        }
      if (VAR == 2 || VAR == 5) {
        // stage this wave's dO^T and Q^T slices ([d][q] padded rows)
#pragma unroll
        for (int fq = 0; fq < 2; ++fq)
#pragma unroll
          for (int ks = 0; ks < 2; ++ks)
#pragma unroll
            for (int j = 0; j < 8; ++j) {
              const int d = ks * 32 + (lane >> 4) * 8 + j;
              const int q_loc = fq * 16 + (lane & 15);
              *reinterpret_cast<bf16*>(dot_lds + d * DKV_T_STRIDE + q_loc * 2) =
                  (bf16)do_frag[fq][ks][j];
              *reinterpret_cast<bf16*>(qt_lds + d * DKV_T_STRIDE + q_loc * 2) =
                  (bf16)q_frag[fq][ks][j];
            }
      }
      if (VAR == 6) {
        // subtiled staging: one 16-B vector write per (fq, ks) fragment
#pragma unroll
        for (int fq = 0; fq < 2; ++fq)
#pragma unroll
          for (int ks = 0; ks < 2; ++ks) {
            const int q_loc = fq * 16 + (lane & 15);
            const int d = ks * 32 + (lane >> 4) * 8;
            const int off = DKV_SUB(q_loc >> 2, d >> 4) + (q_loc & 3) * 32 +
                            ((d >> 3) & 1) * 16;
            *reinterpret_cast<bf16x8*>(dot_lds + off) = do_frag[fq][ks];
            *reinterpret_cast<bf16x8*>(qt_lds + off) = q_frag[fq][ks];
          }
      }

      float lse_w[2], dterm_w[2];
#pragma unroll
      for (int fq = 0; fq < 2; ++fq) {
        const int qrow = qw + fq * 16 + (lane & 15);
        lse_w[fq] = (qrow < L) ? lse[(long)bh * L + qrow] : 0.f;
        dterm_w[fq] = (qrow < L) ? Dterm[(long)bh * L + qrow] : 0.f;
      }
      SEG_MARK(0)  // q/dO fragment + lse/dterm loads

      float p[2][2][4];
      recompute_pT32(k_lds, q_frag, bias, lse_w, lane, h, L, qw, kv0, key_off,
                     vl, scale, causal, p);
      SEG_MARK(1)  // P recompute (QK^T MFMAs + exp)

      f32x4 dp_acc[2][2] = {};
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        bf16x8 v_frag[2];
#pragma unroll
        for (int fk = 0; fk < 2; ++fk) {
          const int key = key_off + fk * 16 + (lane & 15);
          const int kbyte = ks * 64 + (lane >> 4) * 16;
          v_frag[fk] = *reinterpret_cast<const bf16x8*>(v_lds + fa_swz(key, kbyte));
        }
#pragma unroll
        for (int fk = 0; fk < 2; ++fk)
#pragma unroll
          for (int fq = 0; fq < 2; ++fq)
            dp_acc[fk][fq] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                v_frag[fk], do_frag[fq][ks], dp_acc[fk][fq], 0, 0, 0);
      }
      SEG_MARK(2)  // dP = dO V^T MFMAs

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
                  ((unsigned long long)(bh)*L + qcol) * L + key;
              const bool keep = fa_keep(idx, seed, p8);
              pd = keep ? pd * dscale : 0.f;
              dp = keep ? dp * dscale : 0.f;
            }
            const float dsv = scale * p[fk][fq][i] * (dp - dterm_w[fq]);
            *reinterpret_cast<bf16*>(pd_lds + key_loc * 72 + q_loc * 2) =
                __float2bfloat16(pd);
            *reinterpret_cast<bf16*>(ds_lds + key_loc * 72 + q_loc * 2) =
                __float2bfloat16(dsv);
          }
      SEG_MARK(3)  // pd/ds compute + LDS bounce writes

      // dV += pd(key, q) @ dO(q, d);  dK += ds(key, q) @ Q(q, d)
      bf16x8 pa[2], dsa[2];
#pragma unroll
      for (int fk = 0; fk < 2; ++fk) {
        const int key_loc = fk * 16 + (lane & 15);
        const int qbyte = (lane >> 4) * 16;
        pa[fk] = *reinterpret_cast<const bf16x8*>(pd_lds + key_loc * 72 + qbyte);
        dsa[fk] = *reinterpret_cast<const bf16x8*>(ds_lds + key_loc * 72 + qbyte);
      }
      // dO/Q B-fragments read straight from global in transposed order:
      // the 16-B q_frag/do_frag loads above warmed exactly these L1 lines,
      // and dropping the [d][q] LDS bounce removes ~2/3 of the kernel's
      // LDS-issue cost (PMC: WAIT_INST_ANY 55%, LDS_IDX 39% of cycles)
      bf16x8 dob[4], qb[4];
      if (VAR == 6) {
        const int kb0 = (lane >> 4) * 2;
        const int slot = (lane & 15) * 8;
#pragma unroll
        for (int fd = 0; fd < 4; ++fd) {
          bf16x4v* dv4 = reinterpret_cast<bf16x4v*>(&dob[fd]);
          bf16x4v* qv4 = reinterpret_cast<bf16x4v*>(&qb[fd]);
          dv4[0] = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(
              (lds_bf16x4*)(dot_lds + DKV_SUB(kb0, fd) + slot));
          dv4[1] = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(
              (lds_bf16x4*)(dot_lds + DKV_SUB(kb0 + 1, fd) + slot));
          qv4[0] = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(
              (lds_bf16x4*)(qt_lds + DKV_SUB(kb0, fd) + slot));
          qv4[1] = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(
              (lds_bf16x4*)(qt_lds + DKV_SUB(kb0 + 1, fd) + slot));
        }
      } else if (VAR == 2 || VAR == 5) {
        // vector B-fragment reads from the padded [d][q] bounce images
        // (per-wave buffers: the compiler orders same-wave LDS write->read)
#pragma unroll
        for (int fd = 0; fd < 4; ++fd) {
          const int off = (fd * 16 + (lane & 15)) * DKV_T_STRIDE + (lane >> 4) * 16;
          dob[fd] = *reinterpret_cast<const bf16x8*>(dot_lds + off);
          qb[fd] = *reinterpret_cast<const bf16x8*>(qt_lds + off);
        }
      } else if (q_full) {
#pragma unroll
        for (int fd = 0; fd < 4; ++fd) {
          const int d = fd * 16 + (lane & 15);
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            const long row = (long)b * L + qw + (lane >> 4) * 8 + j;
            dob[fd][j] = *reinterpret_cast<const __bf16*>(
                dO + row * HD + (long)h * 64 + d);
            qb[fd][j] = *reinterpret_cast<const __bf16*>(
                Q + row * ldq + (long)h * 64 + d);
          }
        }
      } else {
#pragma unroll
        for (int fd = 0; fd < 4; ++fd) {
          const int d = fd * 16 + (lane & 15);
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            const int qrow = qw + (lane >> 4) * 8 + j;
            if (qrow < L) {
              const long row = (long)b * L + qrow;
              dob[fd][j] = *reinterpret_cast<const __bf16*>(
                  dO + row * HD + (long)h * 64 + d);
              qb[fd][j] = *reinterpret_cast<const __bf16*>(
                  Q + row * ldq + (long)h * 64 + d);
            } else {
              dob[fd][j] = (__bf16)0.0f;
              qb[fd][j] = (__bf16)0.0f;
            }
          }
        }
      }
      SEG_MARK(4)  // pa/dsa LDS reads + transposed dob/qb loads
#pragma unroll
      for (int fk = 0; fk < 2; ++fk)
#pragma unroll
        for (int fd = 0; fd < 4; ++fd) {
          dv_acc[fk][fd] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              pa[fk], dob[fd], dv_acc[fk][fd], 0, 0, 0);
          dk_acc[fk][fd] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              dsa[fk], qb[fd], dk_acc[fk][fd], 0, 0, 0);
        }
      SEG_MARK(5)  // dV/dK MFMAs
    }
  }

  if (VAR == 4 || VAR == 5 || VAR == 6) {
    // pair-wise reduce: the two waves of a key half (wq 0/1) hold the only
    // partials for those 32 keys. wq=1 vector-writes its accs to a [d][key]
    // f32 image with 272-B padded rows ((4d + key) mod 64 distinct within
    // every b128 access -> conflict-free), wq=0 adds and stores to global.
    // Replaces the atomic+zero-fill epilogue that was 45% of the kernel
    // (s_memtime segment breakdown, profiles/flash_dkv_pmc.md).
    char* img = wave_base;  // 64 * 272 B = 17 KiB (reuses the pd/ds region)
#define FA_PAIR_REDUCE(ACC, OUT)                                              \
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
        if (key < L)                                                          \
          OUT[((long)b * L + key) * ldout + (long)h * 64 + d] =               \
              __float2bfloat16(ACC[fk][fd][i] + other[i]);                    \
      }                                                                       \
    }                                                                         \
  }
    FA_PAIR_REDUCE(dv_acc, dV)
    FA_PAIR_REDUCE(dk_acc, dK)
#undef FA_PAIR_REDUCE
    return;
  }

  // cross-wave reduce through LDS (2 waves per key half), then plain store
  float* red = reinterpret_cast<float*>(wave_base);  // 64x64 fp32 = 16 KiB
#define FA_REDUCE_STORE(ACC, OUT)                                             \
  __syncthreads();                                                            \
  for (int i = threadIdx.x; i < TK * 64; i += blockDim.x) red[i] = 0.f;       \
  __syncthreads();                                                            \
  _Pragma("unroll") for (int fk = 0; fk < 2; ++fk)                            \
      _Pragma("unroll") for (int fd = 0; fd < 4; ++fd)                        \
      _Pragma("unroll") for (int i = 0; i < 4; ++i) {                         \
    const int key_loc = key_off + fk * 16 + (lane >> 4) * 4 + i;              \
    const int d = fd * 16 + (lane & 15);                                      \
    atomicAdd(red + key_loc * 64 + d, ACC[fk][fd][i]);                        \
  }                                                                           \
  __syncthreads();                                                            \
  for (int i = threadIdx.x; i < TK * 64; i += blockDim.x) {                   \
    const int key = kv0 + i / 64;                                             \
    const int d = i % 64;                                                     \
    if (key < L)                                                              \
      OUT[((long)b * L + key) * ldout + (long)h * 64 + d] =                   \
          __float2bfloat16(red[i]);                                           \
  }
  FA_REDUCE_STORE(dv_acc, dV)
  FA_REDUCE_STORE(dk_acc, dK)
#undef FA_REDUCE_STORE
  SEG_MARK(6)  // cross-wave reduce + store epilogue
  if (VAR == 9 && lane == 0) {
#pragma unroll
    for (int i = 0; i < 8; ++i) atomicAdd(&dfa_dkv_prof[i], segt[i]);
  }
#undef SEG_MARK
}

// ---------------------------------------------------------------------------
// Attention received: R[b, h, j] = sum_i P[b, h, i, j], the column sums of
// the pre-dropout probabilities (line-level localization scores a key token
// by the total attention it receives). P is rebuilt from K, Q, bias and the
// forward's lse exactly as the dK/dV pass rebuilds it, so no (L, L) buffer,
// V or dO is touched. Masking is the family's: keys >= valid[b] (and, with
// causal, keys > i) get P = 0. Padded QUERY rows i >= valid[b] are summed as
// well — the materialised path and the reference mask keys only, and the
// forward writes a real lse for those rows.
//
// One block owns a 64-key tile of one (b, h) and loops over 32-row query
// strips on dkv's 2 (32-key halves) x 2 (strip interleave) wave grid. Each
// lane keeps 8 fp32 column partials; the epilogue folds the 16 query lanes
// with shfl_xor, the two interleaved waves through LDS in a fixed order, and
// stores every one of the tile's 64 floats from exactly one lane: no atomics,
// so results are bit-reproducible, and R may come from an uninitialised
// allocation (tiles and keys past valid[b] store exact 0).
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void flash_received_kernel(
    const bf16* __restrict__ Q, const bf16* __restrict__ K,
    const int* __restrict__ valid, const float* __restrict__ bias,
    const float* __restrict__ lse, float* __restrict__ R, int B, int H, int L,
    float scale, int causal, long ldq, long ldkv) {
  // LDS map: K nat 8K (swizzled) | 64 fp32 wave-pair reduction slots
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* k_lds = smem;
  float* red = reinterpret_cast<float*>(smem + TK * 128);

  const int lid = blockIdx.y * gridDim.x + blockIdx.x;  // XCD-affine (see fwd)
  const int S = gridDim.x * H;
  const int b = lid / S;
  const int h = (lid % S) / gridDim.x;
  const int kv0 = ((lid % S) % gridDim.x) * TK;
  const int bh = b * H + h;
  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x >> 6;
  const int wk = wid >> 1;   // key half: keys wk*32 .. wk*32+31
  const int wq = wid & 1;    // q interleave
  const int key_off = wk * 32;
  const int vl = valid ? valid[b] : L;

  {  // stage the K tile (natural layout, swizzled); keys >= vl zero-filled
    const int row = threadIdx.x >> 3;
    const int off = (threadIdx.x & 7) * 16;
#pragma unroll
    for (int rr = 0; rr < TK; rr += 32) {
      const int key = kv0 + row + rr;
      uint4v kv = {};
      if (key < vl)
        kv = *reinterpret_cast<const uint4v*>(
            K + ((long)b * L + key) * ldkv + (long)h * 64 + off / 2);
      *reinterpret_cast<uint4v*>(k_lds + fa_swz(row + rr, off)) = kv;
    }
  }
  __syncthreads();

  // [fk][i]: key = key_off + fk*16 + (lane>>4)*4 + i, partial over this
  // lane's query columns
  float acc[2][4] = {};
  if (kv0 < vl) {
    const int q_begin = causal ? kv0 : 0;  // kv0 is a multiple of 32
    const int nstrips = (L - q_begin + TQW - 1) / TQW;
    for (int strip = wq; strip < nstrips; strip += 2) {
      const int qw = q_begin + strip * TQW;
      bf16x8 q_frag[2][2];
      float lse_w[2];
#pragma unroll
      for (int fq = 0; fq < 2; ++fq) {
        const int qrow = qw + fq * 16 + (lane & 15);
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
          const int d = ks * 32 + (lane >> 4) * 8;
          if (qrow < L)
            q_frag[fq][ks] = *reinterpret_cast<const bf16x8*>(
                Q + ((long)b * L + qrow) * ldq + (long)h * 64 + d);
          else
            q_frag[fq][ks] = bf16x8{};
        }
        lse_w[fq] = (qrow < L) ? lse[(long)bh * L + qrow] : 0.f;
      }
      float p[2][2][4];
      recompute_pT32(k_lds, q_frag, bias, lse_w, lane, h, L, qw, kv0, key_off,
                     vl, scale, causal, p);
#pragma unroll
      for (int fk = 0; fk < 2; ++fk)
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[fk][i] += p[fk][0][i] + p[fk][1][i];
    }
  }

  // fold the 16 query lanes (lane & 15) of each key group
#pragma unroll
  for (int fk = 0; fk < 2; ++fk)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float a = acc[fk][i];
      a += __shfl_xor(a, 1);
      a += __shfl_xor(a, 2);
      a += __shfl_xor(a, 4);
      a += __shfl_xor(a, 8);
      acc[fk][i] = a;
    }
  // wave pair (wq 0/1) of a key half: wq=1 parks its sums, wq=0 adds them
  // (always wq0 + wq1) and stores its half's 32 floats, 4 per lane
  const bool owner = (lane & 15) == 0;
  if (wq == 1 && owner) {
#pragma unroll
    for (int fk = 0; fk < 2; ++fk)
      *reinterpret_cast<f32x4*>(red + key_off + fk * 16 + (lane >> 4) * 4) =
          f32x4{acc[fk][0], acc[fk][1], acc[fk][2], acc[fk][3]};
  }
  __syncthreads();
  if (wq == 0 && owner) {
#pragma unroll
    for (int fk = 0; fk < 2; ++fk) {
      const int key_loc = key_off + fk * 16 + (lane >> 4) * 4;  // kv0 + 63 < L
      const f32x4 other = *reinterpret_cast<const f32x4*>(red + key_loc);
      *reinterpret_cast<f32x4*>(R + (long)bh * L + kv0 + key_loc) =
          f32x4{acc[fk][0] + other[0], acc[fk][1] + other[1],
                acc[fk][2] + other[2], acc[fk][3] + other[3]};
    }
  }
}

void launch_flash_received(const bf16* Q, const bf16* K, const int* valid,
                           const float* bias, const float* lse, float* R,
                           int B, int H, int L, float scale, int causal,
                           long ldq, long ldkv, hipStream_t stream) {
  // L % 64 == 0 (checked by the binding): every tile is whole, so neither
  // the bias reads nor the R stores need a key < L guard
  const dim3 grid(L / TK, B * H);
  const size_t lds = TK * 128 + TK * sizeof(float);
  hipLaunchKernelGGL(flash_received_kernel, grid, dim3(256), lds, stream, Q, K,
                     valid, bias, lse, R, B, H, L, scale, causal, ldq, ldkv);
}

void fwd_prof_fetch(unsigned long long* out) {
  (void)hipMemcpyFromSymbol(out, HIP_SYMBOL(dfa_fwd_prof),
                            8 * sizeof(unsigned long long));
  unsigned long long z[8] = {};
  (void)hipMemcpyToSymbol(HIP_SYMBOL(dfa_fwd_prof), z, sizeof(z));
}

void launch_flash_fwd(const bf16* Q, const bf16* K, const bf16* V,
                      const int* valid, const float* bias, bf16* O, float* lse,
                      int B, int H, int L, float scale, int causal,
                      unsigned p8, unsigned long long seed, long ldq,
                      long ldkv, hipStream_t stream) {
  const size_t lds = 2 * (TK * 128 + FWD_VBYTES);  // double-buffered K+V
  const char* e = getenv("DFA_FWD_PROF");
  // 8-wave variant measured SLOWER on B16 L512 H12 (72.5 vs 66.5 us —
  // fewer blocks lose more to tail/latency than staging amortization
  // gains); keep the template but select it never for now
  const long blocks8 = (long)((L + 8 * TQW - 1) / (8 * TQW)) * B * H;
  if (false && L % (8 * TQW) == 0 && blocks8 >= 192) {
    const dim3 grid(L / (8 * TQW), B * H);
    if (e && e[0] == '1')
      hipLaunchKernelGGL((flash_fwd_kernel<1, 8>), grid, dim3(512), lds, stream,
                         Q, K, V, valid, bias, O, lse, B, H, L, scale, causal,
                         p8, seed, ldq, ldkv);
    else
      hipLaunchKernelGGL((flash_fwd_kernel<0, 8>), grid, dim3(512), lds, stream,
                         Q, K, V, valid, bias, O, lse, B, H, L, scale, causal,
                         p8, seed, ldq, ldkv);
    return;
  }
  const dim3 grid((L + NWAVE * TQW - 1) / (NWAVE * TQW), B * H);
  if (e && e[0] == '1')
    hipLaunchKernelGGL((flash_fwd_kernel<1, 4>), grid, dim3(256), lds, stream,
                       Q, K, V, valid, bias, O, lse, B, H, L, scale, causal,
                       p8, seed, ldq, ldkv);
  else
    hipLaunchKernelGGL((flash_fwd_kernel<0, 4>), grid, dim3(256), lds, stream,
                       Q, K, V, valid, bias, O, lse, B, H, L, scale, causal,
                       p8, seed, ldq, ldkv);
}

void launch_flash_dterm(const bf16* dO, const bf16* O, float* Dterm, int B,
                        int H, int L, hipStream_t stream) {
  const long rows = (long)B * L * H;
  const int rows_per_block = 32;  // 4 waves x 8 rows
  hipLaunchKernelGGL(flash_dterm_kernel,
                     dim3((rows + rows_per_block - 1) / rows_per_block),
                     dim3(256), 0, stream, dO, O, Dterm, B, H, L);
}

void launch_flash_dq(const bf16* Q, const bf16* K, const bf16* V,
                     const bf16* dO, const int* valid, const float* bias,
                     const float* lse, const float* Dterm, bf16* dQ,
                     float* dBias, int B, int H, int L, float scale,
                     int causal, unsigned p8, unsigned long long seed,
                     long ldq, long ldkv, long ldout, hipStream_t stream) {
  const dim3 grid((L + NWAVE * TQW - 1) / (NWAVE * TQW), B * H);
  const size_t lds = 2 * 3 * TK * 128;  // double-buffered K/K^T/V tiles
  hipLaunchKernelGGL(flash_dq_kernel, grid, dim3(256), lds, stream, Q, K, V,
                     dO, valid, bias, lse, Dterm, dQ, dBias, B, H, L, scale,
                     causal, p8, seed, ldq, ldkv, ldout);
}

void launch_flash_dkv(const bf16* Q, const bf16* K, const bf16* V,
                      const bf16* dO, const int* valid, const float* bias,
                      const float* lse, const float* Dterm, bf16* dK,
                      bf16* dV, int B, int H, int L, float scale, int causal,
                      unsigned p8, unsigned long long seed, long ldq,
                      long ldkv, long ldout, hipStream_t stream) {
  const dim3 grid((L + TK - 1) / TK, B * H);
  size_t lds = 2 * TK * 128 + 18432;  // K,V + pd/ds bounces (72-B rows)
  const char* e = getenv("DFA_DKV_VARIANT");  // re-read: lets one probe
  const int var = e ? atoi(e) : 4;            // process A/B the variants
  if (var == 2) {
    lds += 4 * 2 * DKV_T_BYTES;
    hipLaunchKernelGGL(flash_dkv_kernel<2>, grid, dim3(256), lds, stream, Q, K,
                       V, dO, valid, bias, lse, Dterm, dK, dV, B, H, L, scale,
                       causal, p8, seed, ldq, ldkv, ldout);
  } else if (var == 4) {
    // K,V + max(pd/ds region, 64x272 pair image)
    lds = 2 * TK * 128 + 18432;
    hipLaunchKernelGGL(flash_dkv_kernel<4>, grid, dim3(256), lds, stream, Q, K,
                       V, dO, valid, bias, lse, Dterm, dK, dV, B, H, L, scale,
                       causal, p8, seed, ldq, ldkv, ldout);
  } else if (var == 3) {
    hipLaunchKernelGGL(flash_dkv_kernel<3>, grid, dim3(256), lds, stream, Q, K,
                       V, dO, valid, bias, lse, Dterm, dK, dV, B, H, L, scale,
                       causal, p8, seed, ldq, ldkv, ldout);
  } else if (var == 5) {
    lds += 4 * 2 * DKV_T_BYTES;  // bounce staging + pair-reduce epilogue
    hipLaunchKernelGGL(flash_dkv_kernel<5>, grid, dim3(256), lds, stream, Q, K,
                       V, dO, valid, bias, lse, Dterm, dK, dV, B, H, L, scale,
                       causal, p8, seed, ldq, ldkv, ldout);
  } else if (var == 6) {
    lds += 4 * 2 * DKV_T_BYTES;  // subtiled tr_b16 bounce + pair-reduce
    hipLaunchKernelGGL(flash_dkv_kernel<6>, grid, dim3(256), lds, stream, Q, K,
                       V, dO, valid, bias, lse, Dterm, dK, dV, B, H, L, scale,
                       causal, p8, seed, ldq, ldkv, ldout);
  } else if (var == 9) {
    hipLaunchKernelGGL(flash_dkv_kernel<9>, grid, dim3(256), lds, stream, Q, K,
                       V, dO, valid, bias, lse, Dterm, dK, dV, B, H, L, scale,
                       causal, p8, seed, ldq, ldkv, ldout);
  } else {
    hipLaunchKernelGGL(flash_dkv_kernel<0>, grid, dim3(256), lds, stream, Q, K,
                       V, dO, valid, bias, lse, Dterm, dK, dV, B, H, L, scale,
                       causal, p8, seed, ldq, ldkv, ldout);
  }
}

void dkv_prof_fetch(unsigned long long* out) {
  // read + zero the variant-9 per-segment cycle accumulators
  (void)hipMemcpyFromSymbol(out, HIP_SYMBOL(dfa_dkv_prof),
                            8 * sizeof(unsigned long long));
  unsigned long long z[8] = {};
  (void)hipMemcpyToSymbol(HIP_SYMBOL(dfa_dkv_prof), z, sizeof(z));
}
