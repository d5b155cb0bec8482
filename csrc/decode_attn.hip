// Decode-time attention for T5 generation: ONE query row per sequence,
// head_dim 64, bf16 in/out, fp32 scores / softmax / accumulation.
//
//   decode_self_kernel   one wave per (row r, head h). Stores the new token's
//                        K/V into cache[r, pos], attends over keys 0..pos
//                        where key j < pos lives at cache[anc[r, j], j] (the
//                        beam-search indirection table) and key pos is taken
//                        from registers, adds the relative-position bias
//                        bias_dist[h, pos - j].
//   decode_cross_kernel  one 256-thread workgroup per (source b, head h)
//                        serving every beam row r = b * beams + i of that
//                        source: K and V tiles are staged in LDS once per
//                        group of <= 16 beam rows and reused by all of them.
//
// Why the in-place self cache is race-free: slot (r, pos) is written only by
// row r's workgroups at step pos (one per head, disjoint 128-B pieces); other
// rows read it only in LATER launches (a row reads keys j < pos from the
// cache and key pos from its own registers, never from the store it just
// issued); no slot is ever rewritten. So no launch both writes and reads one
// address, whatever anc holds.
//
// Both are memory/latency bound at one query row, so the dot products are
// plain fp32 VALU FMAs: probabilities stay fp32 into PV (a bf16 MFMA would
// round P to 8 bits, which the error bound of tests/test_gpu_decode_attn.py
// does not allow), there is exactly ONE __expf per probability (two-pass
// softmax, scores parked in LDS) and one rounding to bf16 at the output.
// No atomics, no global scratch: outputs are deterministic.
//
// Every global K/V/Q access is a 16-B load by 8 adjacent lanes = one whole
// 128-B head row per lane group.

#include <hip/hip_bf16.h>
#include <hip/hip_runtime.h>

namespace {

typedef __hip_bfloat16 bf16_t;

constexpr int HD = 64;          // head dim
constexpr float NEG = -3.0e38f; // "no key yet": finite, so NEG - NEG = 0, never NaN

__device__ __forceinline__ void unpack8(const uint4& u, float* f) {
  f[0] = __uint_as_float(u.x << 16);
  f[1] = __uint_as_float(u.x & 0xffff0000u);
  f[2] = __uint_as_float(u.y << 16);
  f[3] = __uint_as_float(u.y & 0xffff0000u);
  f[4] = __uint_as_float(u.z << 16);
  f[5] = __uint_as_float(u.z & 0xffff0000u);
  f[6] = __uint_as_float(u.w << 16);
  f[7] = __uint_as_float(u.w & 0xffff0000u);
}

__device__ __forceinline__ unsigned pack2(float a, float b) {
  bf16_t lo = __float2bfloat16(a), hi = __float2bfloat16(b);
  return (unsigned)(*reinterpret_cast<unsigned short*>(&lo)) |
         ((unsigned)(*reinterpret_cast<unsigned short*>(&hi)) << 16);
}

__device__ __forceinline__ uint4 ld16(const bf16_t* p) {
  return *reinterpret_cast<const uint4*>(p);
}

__device__ __forceinline__ float dot8(const float* a, const float* b) {
  float s = a[0] * b[0];
#pragma unroll
  for (int i = 1; i < 8; ++i) s = fmaf(a[i], b[i], s);
  return s;
}

// sum over the 8 lanes of a lane group (every lane gets the total)
__device__ __forceinline__ float group_sum(float v) {
  v += __shfl_xor(v, 1);
  v += __shfl_xor(v, 2);
  v += __shfl_xor(v, 4);
  return v;
}

// ---------------------------------------------------------------------------
// self attention: grid (R, H), 64 threads. Lane group g = lane >> 3 owns keys
// g, g + 8, ...; lane c = lane & 7 holds dims 8c .. 8c + 7 of every row.
// Dynamic LDS: (pos + 1) fp32 scores.
// ---------------------------------------------------------------------------
constexpr int SELF_UNROLL = 4;  // independent 16-B loads in flight per lane

__global__ __launch_bounds__(64) void decode_self_kernel(
    const bf16_t* __restrict__ q, const bf16_t* __restrict__ k_new,
    const bf16_t* __restrict__ v_new, bf16_t* __restrict__ k_cache,
    bf16_t* __restrict__ v_cache, const int* __restrict__ anc,
    const float* __restrict__ bias_dist, bf16_t* __restrict__ out, int Tmax, int pos, int H,
    float scale, long ldq, long ldk, long ldv) {
  extern __shared__ float sc[];
  const int lane = threadIdx.x, g = lane >> 3, c = lane & 7;
  const long r = blockIdx.x;
  const int h = blockIdx.y;
  const long D = (long)H * HD;
  const int col = h * HD + c * 8;

  const uint4 qraw = ld16(q + r * ldq + col);
  const uint4 kraw = ld16(k_new + r * ldk + col);
  const uint4 vraw = ld16(v_new + r * ldv + col);
  if (g == 0) {
    const long slot = (r * Tmax + pos) * D + col;
    *reinterpret_cast<uint4*>(k_cache + slot) = kraw;
    *reinterpret_cast<uint4*>(v_cache + slot) = vraw;
  }
  float qf[8], tmp[8];
  unpack8(qraw, qf);
  unpack8(kraw, tmp);
  const float* brow = bias_dist ? bias_dist + (long)h * Tmax : nullptr;
  float s_new = scale * group_sum(dot8(qf, tmp));
  if (brow) s_new += brow[0];

  // pass 1: scores of the cached keys. Lanes past the end recompute key
  // pos - 1 (in bounds) and discard it, so the shuffles never diverge.
  const int* arow = anc ? anc + r * Tmax : nullptr;
  const int Rm1 = (int)gridDim.x - 1;  // a corrupt table entry must not leave the cache
  float mx = s_new;
  for (int j0 = 0; j0 < pos; j0 += 8 * SELF_UNROLL) {
    uint4 kr[SELF_UNROLL];
#pragma unroll
    for (int u = 0; u < SELF_UNROLL; ++u) {
      const int j = min(j0 + u * 8 + g, pos - 1);
      const long pr = arow ? (long)min(max(arow[j], 0), Rm1) : r;
      kr[u] = ld16(k_cache + (pr * Tmax + j) * D + col);
    }
#pragma unroll
    for (int u = 0; u < SELF_UNROLL; ++u) {
      const int j = j0 + u * 8 + g;
      unpack8(kr[u], tmp);
      float s = scale * group_sum(dot8(qf, tmp));
      if (j < pos) {
        if (brow) s += brow[pos - j];
        mx = fmaxf(mx, s);
        if (c == 0) sc[j] = s;
      }
    }
  }
  mx = fmaxf(mx, __shfl_xor(mx, 8));
  mx = fmaxf(mx, __shfl_xor(mx, 16));
  mx = fmaxf(mx, __shfl_xor(mx, 32));
  __syncthreads();

  // pass 2: p = exp(s - max), PV. The new token goes to group 0.
  float acc[8], l = 0.f;
#pragma unroll
  for (int i = 0; i < 8; ++i) acc[i] = 0.f;
  if (g == 0) {
    const float p = __expf(s_new - mx);
    unpack8(vraw, tmp);
    l = p;
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[i] = p * tmp[i];
  }
  for (int j0 = 0; j0 < pos; j0 += 8 * SELF_UNROLL) {
    uint4 vr[SELF_UNROLL];
    float p[SELF_UNROLL];
#pragma unroll
    for (int u = 0; u < SELF_UNROLL; ++u) {
      const int j = j0 + u * 8 + g;
      const int jc = min(j, pos - 1);
      const long pr = arow ? (long)min(max(arow[jc], 0), Rm1) : r;
      vr[u] = ld16(v_cache + (pr * Tmax + jc) * D + col);
      p[u] = j < pos ? __expf(sc[jc] - mx) : 0.f;
    }
#pragma unroll
    for (int u = 0; u < SELF_UNROLL; ++u) {
      if (j0 + u * 8 + g < pos) {  // a discarded row may hold anything, NaN included
        unpack8(vr[u], tmp);
        l += p[u];
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[i] = fmaf(p[u], tmp[i], acc[i]);
      }
    }
  }
#pragma unroll
  for (int off = 8; off < 64; off <<= 1) {
    l += __shfl_xor(l, off);
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[i] += __shfl_xor(acc[i], off);
  }
  if (g == 0) {
    const float il = 1.f / l;  // l >= exp(0) of the max key: never 0
    uint4 o;
    o.x = pack2(acc[0] * il, acc[1] * il);
    o.y = pack2(acc[2] * il, acc[3] * il);
    o.z = pack2(acc[4] * il, acc[5] * il);
    o.w = pack2(acc[6] * il, acc[7] * il);
    *reinterpret_cast<uint4*>(out + r * D + col) = o;
  }
}

// ---------------------------------------------------------------------------
// cross attention: grid (B, H), 256 threads = 4 waves. Beam rows are served in
// groups of CG = 16; wave w owns rows w, w + 4, w + 8, w + 12 of the group.
// Per group: pass 1 stages each 64-key K tile and writes the scores, the
// softmax turns them into probabilities in place, pass 2 stages each V tile
// and accumulates PV; the next tile's global loads fly during each compute. Keys >= valid[b] are never loaded (tile rows past the
// live length are zero-filled, their probabilities are 0).
// Dynamic LDS, floats: q[CG][64] | tile[64][TLD] bf16 | sc[CG][Lpad]
// ---------------------------------------------------------------------------
constexpr int CG = 16;
constexpr int CT = 64;   // keys per tile
constexpr int TLD = 72;  // bf16 per staged row: 144 B, so key-per-lane 16-B reads spread over banks

// A 64-key tile is staged in two halves: load_tile issues the global loads
// into registers (8 lanes x 16 B = one whole 128-B row; 256 threads = 32 rows
// per pass), store_tile writes them to LDS. The loads of tile t + 1 are issued
// before tile t is computed on, so their latency hides behind the FMAs.
struct TileRegs {
  uint4 v[CT / 32];
};

__device__ __forceinline__ void load_tile(const bf16_t* __restrict__ src, long ld, int j0,
                                          int live, int tid, TileRegs& regs) {
#pragma unroll
  for (int pass = 0; pass < CT / 32; ++pass) {
    const int row = pass * 32 + (tid >> 3), c = tid & 7;
    regs.v[pass] = make_uint4(0u, 0u, 0u, 0u);
    if (j0 + row < live) regs.v[pass] = ld16(src + (long)(j0 + row) * ld + c * 8);
  }
}

__device__ __forceinline__ void store_tile(const TileRegs& regs, bf16_t* tile, int tid) {
#pragma unroll
  for (int pass = 0; pass < CT / 32; ++pass) {
    const int row = pass * 32 + (tid >> 3), c = tid & 7;
    *reinterpret_cast<uint4*>(tile + row * TLD + c * 8) = regs.v[pass];
  }
}

__global__ __launch_bounds__(256) void decode_cross_kernel(
    const bf16_t* __restrict__ q, const bf16_t* __restrict__ k, const bf16_t* __restrict__ v,
    const int* __restrict__ valid, bf16_t* __restrict__ out, int Lk, int beams, int H,
    float scale, long ldq, long ldk, long ldv, long bsk, long bsv) {
  extern __shared__ float smem[];
  float* qs = smem;                                           // [CG][64]
  bf16_t* tile = reinterpret_cast<bf16_t*>(smem + CG * HD);   // [CT][TLD]
  float* sc = smem + CG * HD + CT * TLD / 2;                  // [CG][Lpad]

  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int b = blockIdx.x, h = blockIdx.y;
  const long D = (long)H * HD;
  int live = Lk;
  if (valid) live = max(0, min(valid[b], Lk));
  const int ntile = (live + CT - 1) / CT;
  const int Lpad = ntile * CT;  // <= the launch's padded Lk
  const bf16_t* kb = k + (long)b * bsk + h * HD;
  const bf16_t* vb = v + (long)b * bsv + h * HD;

  for (int i0 = 0; i0 < beams; i0 += CG) {
    const int nb = min(CG, beams - i0);
    const long r0 = (long)b * beams + i0;
    if (live == 0) {  // no key to attend to: exact zeros
      for (int e = tid; e < nb * HD; e += 256)
        out[(r0 + (e >> 6)) * D + h * HD + (e & 63)] = __float2bfloat16(0.f);
      continue;
    }
    __syncthreads();  // the previous group is done with qs / sc / tile
    for (int e = tid; e < nb * 8; e += 256) {
      float f[8];
      unpack8(ld16(q + (r0 + (e >> 3)) * ldq + h * HD + (e & 7) * 8), f);
#pragma unroll
      for (int i = 0; i < 8; ++i) qs[(e >> 3) * HD + (e & 7) * 8 + i] = f[i];
    }

    // pass 1: thread = key `lane` of the tile x this wave's rows
    TileRegs regs;
    load_tile(kb, ldk, 0, live, tid, regs);
    for (int t = 0; t < ntile; ++t) {
      __syncthreads();
      store_tile(regs, tile, tid);
      if (t + 1 < ntile) load_tile(kb, ldk, (t + 1) * CT, live, tid, regs);
      __syncthreads();
      float s[CG / 4];
#pragma unroll
      for (int i = 0; i < CG / 4; ++i) s[i] = 0.f;
#pragma unroll
      for (int ch = 0; ch < 8; ++ch) {
        float kf[8];
        unpack8(*reinterpret_cast<const uint4*>(tile + lane * TLD + ch * 8), kf);
#pragma unroll
        for (int i = 0; i < CG / 4; ++i) {
          const int row = i * 4 + w;
          if (row < nb) {
            const float4 qa = *reinterpret_cast<const float4*>(qs + row * HD + ch * 8);
            const float4 qb = *reinterpret_cast<const float4*>(qs + row * HD + ch * 8 + 4);
            float a = s[i];
            a = fmaf(qa.x, kf[0], a);
            a = fmaf(qa.y, kf[1], a);
            a = fmaf(qa.z, kf[2], a);
            a = fmaf(qa.w, kf[3], a);
            a = fmaf(qb.x, kf[4], a);
            a = fmaf(qb.y, kf[5], a);
            a = fmaf(qb.z, kf[6], a);
            a = fmaf(qb.w, kf[7], a);
            s[i] = a;
          }
        }
      }
#pragma unroll
      for (int i = 0; i < CG / 4; ++i) {
        const int row = i * 4 + w;
        if (row < nb) sc[row * Lpad + t * CT + lane] = scale * s[i];
      }
    }
    __syncthreads();
    load_tile(vb, ldv, 0, live, tid, regs);  // in flight during the softmax

    // softmax in place: each wave its own rows; padded keys get p = 0
    float il[CG / 4];
#pragma unroll
    for (int i = 0; i < CG / 4; ++i) {
      const int row = i * 4 + w;
      il[i] = 0.f;
      if (row < nb) {
        float* srow = sc + row * Lpad;
        float mx = NEG;
        for (int j = lane; j < live; j += 64) mx = fmaxf(mx, srow[j]);
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) mx = fmaxf(mx, __shfl_xor(mx, off));
        float l = 0.f;
        for (int j = lane; j < Lpad; j += 64) {
          const float p = j < live ? __expf(srow[j] - mx) : 0.f;
          srow[j] = p;
          l += p;
        }
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) l += __shfl_xor(l, off);
        il[i] = 1.f / l;
      }
    }

    // pass 2: thread = output dim `lane` x this wave's rows
    float acc[CG / 4];
#pragma unroll
    for (int i = 0; i < CG / 4; ++i) acc[i] = 0.f;
    for (int t = 0; t < ntile; ++t) {
      __syncthreads();  // also orders the softmax's LDS writes (same wave) before the reads
      store_tile(regs, tile, tid);
      if (t + 1 < ntile) load_tile(vb, ldv, (t + 1) * CT, live, tid, regs);
      __syncthreads();
      for (int j = 0; j < CT; j += 4) {
        float vf[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const unsigned short raw =
              *reinterpret_cast<const unsigned short*>(tile + (j + u) * TLD + lane);
          vf[u] = __uint_as_float((unsigned)raw << 16);
        }
#pragma unroll
        for (int i = 0; i < CG / 4; ++i) {
          const int row = i * 4 + w;
          if (row < nb) {
            const float4 p = *reinterpret_cast<const float4*>(sc + row * Lpad + t * CT + j);
            float a = acc[i];
            a = fmaf(p.x, vf[0], a);
            a = fmaf(p.y, vf[1], a);
            a = fmaf(p.z, vf[2], a);
            a = fmaf(p.w, vf[3], a);
            acc[i] = a;
          }
        }
      }
    }
#pragma unroll
    for (int i = 0; i < CG / 4; ++i) {
      const int row = i * 4 + w;
      if (row < nb) out[(r0 + row) * D + h * HD + lane] = __float2bfloat16(acc[i] * il[i]);
    }
  }
}

}  // namespace

void launch_decode_self(const __hip_bfloat16* q, const __hip_bfloat16* k_new,
                        const __hip_bfloat16* v_new, __hip_bfloat16* k_cache,
                        __hip_bfloat16* v_cache, const int* anc, const float* bias_dist,
                        __hip_bfloat16* out, long R, int Tmax, int pos, int H, float scale,
                        long ldq, long ldk, long ldv, hipStream_t stream) {
  const size_t lds = (size_t)(pos + 1) * sizeof(float);
  hipLaunchKernelGGL(decode_self_kernel, dim3((unsigned)R, (unsigned)H), dim3(64), lds, stream,
                     q, k_new, v_new, k_cache, v_cache, anc, bias_dist, out, Tmax, pos, H, scale,
                     ldq, ldk, ldv);
}

// LDS bytes of a cross launch at key length Lk (the binding checks it against the limit)
size_t decode_cross_lds_bytes(int Lk) {
  const int Lpad = (Lk + CT - 1) / CT * CT;
  return sizeof(float) * ((size_t)CG * HD + CT * TLD / 2 + (size_t)CG * Lpad);
}

void launch_decode_cross(const __hip_bfloat16* q, const __hip_bfloat16* k,
                         const __hip_bfloat16* v, const int* valid, __hip_bfloat16* out, int B,
                         int Lk, int beams, int H, float scale, long ldq, long ldk, long ldv,
                         long bsk, long bsv, hipStream_t stream) {
  hipLaunchKernelGGL(decode_cross_kernel, dim3((unsigned)B, (unsigned)H), dim3(256),
                     decode_cross_lds_bytes(Lk), stream, q, k, v, valid, out, Lk, beams, H, scale,
                     ldq, ldk, ldv, bsk, bsv);
}
