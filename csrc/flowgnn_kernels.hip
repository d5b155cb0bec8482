// Flow-GNN kernels for MI355X (gfx950, CDNA4). Native HIP — no CUDA compat.
//
// Covers the DGL-delegated ops of the reference's flow-GNN (SURVEY.md §2.6
// K1-K10): fused 4-way embedding gather, block-diagonal CSR segment-sum
// (message aggregation + its CSC transpose backward), fused GRU gates,
// gated-attention segment softmax pooling, per-graph label max.
//
// Regime: the whole model is tiny (N ~= 12k nodes, D = 128 at batch 256), so
// every kernel here is memory/latency-bound, never MFMA-bound; the design
// rules that matter are coalescing (vectorized 2-element lanes: 64-lane wave
// covers a 128-wide row), one wave per CSR row (avg degree ~2.5, max ~500),
// and few kernels per step (fused gates) — the GEMMs go to rocBLAS via
// torch.matmul, which is the right tool for plain 128x384 GEMMs.

#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>

#include <algorithm>
using std::min;

#include "gru_gate_bwd.h"

#define WAVE 64

// ---------------------------------------------------------------------------
// dtype helpers
// ---------------------------------------------------------------------------

template <typename T> __device__ __forceinline__ float to_f(T v);
template <> __device__ __forceinline__ float to_f<float>(float v) { return v; }
template <> __device__ __forceinline__ float to_f<__hip_bfloat16>(__hip_bfloat16 v) {
  return __bfloat162float(v);
}

template <typename T> __device__ __forceinline__ T from_f(float v);
template <> __device__ __forceinline__ float from_f<float>(float v) { return v; }
template <> __device__ __forceinline__ __hip_bfloat16 from_f<__hip_bfloat16>(float v) {
  return __float2bfloat16(v);
}

__device__ __forceinline__ float sigmoidf_(float x) { return 1.0f / (1.0f + __expf(-x)); }

// ---------------------------------------------------------------------------
// K1: fused 4-way embedding gather-concat.
// tables (4, V, 32) T; idx (N, 4) int64 -> out (N, 128) T.
// One wave per node; lane l writes out[n][2l..2l+1]; feature f = l/16.
// ---------------------------------------------------------------------------

template <typename T, typename TO>
__global__ void embed4_fwd_kernel(const T* __restrict__ tables,
                                  const long* __restrict__ idx,
                                  TO* __restrict__ out, int N, int V) {
  // TO may differ from T: under bf16 autocast the gather emits bf16
  // directly from the fp32 master tables (removes the .to(bf16) cast
  // kernels + their backward casts on both consumers of the embedding)
  const int wid = (blockIdx.x * blockDim.x + threadIdx.x) / WAVE;
  const int lane = threadIdx.x & (WAVE - 1);
  if (wid >= N) return;
  const int c = lane * 2;          // column in [0,128)
  const int f = c >> 5;            // feature index
  const int off = c & 31;          // offset within the 32-wide embedding
  const long row = idx[(long)wid * 4 + f];
  const T* src = tables + ((long)f * V + row) * 32 + off;
  TO* dst = out + (long)wid * 128 + c;
  dst[0] = from_f<TO>(to_f(src[0]));
  dst[1] = from_f<TO>(to_f(src[1]));
}

template <typename T>
__global__ void embed4_bwd_kernel(const T* __restrict__ grad_out,
                                  const long* __restrict__ idx,
                                  float* __restrict__ grad_tables, long total,
                                  int V) {
  // Grid-stride over N*128 elements; fp32 scatter-add. Vocabulary rows 0
  // ("not a definition", ~60% of nodes) and 1 (UNKNOWN) are accumulated in
  // LDS per block and flushed once — global atomic contention on those two
  // rows otherwise serializes the whole kernel (rocprof: 95 us -> ~10 us).
  __shared__ float hot[2 * 128];
  for (int i = threadIdx.x; i < 2 * 128; i += blockDim.x) hot[i] = 0.f;
  __syncthreads();
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (long)gridDim.x * blockDim.x) {
    const long n = i >> 7;
    const int c = (int)(i & 127);
    const int f = c >> 5;
    const int off = c & 31;
    const long row = idx[n * 4 + f];
    const float g = to_f(grad_out[i]);
    if (row < 2) {
      atomicAdd(hot + (int)row * 128 + c, g);
    } else {
      atomicAdd(grad_tables + ((long)f * V + row) * 32 + off, g);
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 2 * 128; i += blockDim.x) {
    const float v = hot[i];
    if (v != 0.f) {
      const int row = i >> 7;
      const int c = i & 127;
      const int f = c >> 5;
      const int off = c & 31;
      atomicAdd(grad_tables + ((long)f * V + row) * 32 + off, v);
    }
  }
}

// ---------------------------------------------------------------------------
// K2: CSR segment-sum  m[v] = sum_{e in [indptr[v], indptr[v+1])} x[indices[e]].
// One wave per destination row; lane covers 2 columns, strided by 128 for
// D > 128. fp32 accumulation. Used for forward (in-CSR) and backward (CSC).
// ---------------------------------------------------------------------------

template <typename T>
__global__ void spmm_sum_kernel(const int* __restrict__ indptr,
                                const int* __restrict__ indices,
                                const T* __restrict__ x, T* __restrict__ out,
                                int N, int D, long x_stride) {
  const int v = (blockIdx.x * blockDim.x + threadIdx.x) / WAVE;
  const int lane = threadIdx.x & (WAVE - 1);
  if (v >= N) return;
  const int e0 = indptr[v], e1 = indptr[v + 1];
  for (int c = lane * 2; c < D; c += WAVE * 2) {
    float a0 = 0.f, a1 = 0.f;
    for (int e = e0; e < e1; ++e) {
      const T* row = x + (long)indices[e] * x_stride + c;
      a0 += to_f(row[0]);
      a1 += to_f(row[1]);
    }
    T* dst = out + (long)v * D + c;
    dst[0] = from_f<T>(a0);
    dst[1] = from_f<T>(a1);
  }
}

// ---------------------------------------------------------------------------
// K3: fused GRU gates (torch.nn.GRUCell semantics).
// gi, gh (N, 3H); h (N, H) -> h_new, r, z, n (N, H). Elementwise, fp32 math.
// ---------------------------------------------------------------------------

template <typename T>
__global__ void gru_gates_fwd_kernel(const T* __restrict__ gi,
                                     const T* __restrict__ gh,
                                     const T* __restrict__ h,
                                     T* __restrict__ h_new, T* __restrict__ r_o,
                                     T* __restrict__ z_o, T* __restrict__ n_o,
                                     long NH, int H) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < NH;
       i += (long)gridDim.x * blockDim.x) {
    const long row = i / H;
    const int c = (int)(i - row * H);
    const long b = row * 3 * H + c;
    const float ir = to_f(gi[b]), iz = to_f(gi[b + H]), in_ = to_f(gi[b + 2 * H]);
    const float hr = to_f(gh[b]), hz = to_f(gh[b + H]), hn = to_f(gh[b + 2 * H]);
    const float r = sigmoidf_(ir + hr);
    const float z = sigmoidf_(iz + hz);
    const float n = tanhf(in_ + r * hn);
    const float hv = to_f(h[i]);
    h_new[i] = from_f<T>((1.f - z) * n + z * hv);
    r_o[i] = from_f<T>(r);
    z_o[i] = from_f<T>(z);
    n_o[i] = from_f<T>(n);
  }
}

template <typename T>
__global__ void gru_gates_bwd_kernel(const T* __restrict__ grad_h_new,
                                     const T* __restrict__ gh,
                                     const T* __restrict__ h,
                                     const T* __restrict__ r_i,
                                     const T* __restrict__ z_i,
                                     const T* __restrict__ n_i,
                                     T* __restrict__ grad_gi,
                                     T* __restrict__ grad_gh,
                                     T* __restrict__ grad_h, long NH, int H) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < NH;
       i += (long)gridDim.x * blockDim.x) {
    const long row = i / H;
    const int c = (int)(i - row * H);
    const long b = row * 3 * H + c;
    const float go = to_f(grad_h_new[i]);
    const float r = to_f(r_i[i]), z = to_f(z_i[i]), n = to_f(n_i[i]);
    const float hv = to_f(h[i]);
    const float hn = to_f(gh[b + 2 * H]);
    const float dn = go * (1.f - z);
    const float dz = go * (hv - n);
    const float dpn = dn * (1.f - n * n);
    const float dr = dpn * hn;
    const float dpr = dr * r * (1.f - r);
    const float dpz = dz * z * (1.f - z);
    grad_gi[b] = from_f<T>(dpr);
    grad_gi[b + H] = from_f<T>(dpz);
    grad_gi[b + 2 * H] = from_f<T>(dpn);
    grad_gh[b] = from_f<T>(dpr);
    grad_gh[b + H] = from_f<T>(dpz);
    grad_gh[b + 2 * H] = from_f<T>(dpn * r);
    grad_h[i] = from_f<T>(go * z);
  }
}

// ---------------------------------------------------------------------------
// K3b: fused GRU gates over the block-GEMM output ("gicat" layout).
// gicat (N, 4H) columns: [rsum | zsum | i_n | h_n] where rsum = i_r + h_r
// etc. come straight from one MFMA GEMM of [m|h] against the block weight
// matrix Wcat (see bindings ggnn_fused_fwd). Saves r/z/n/h_n for backward.
// ---------------------------------------------------------------------------

template <typename T>
__global__ void gru_gates2_fwd_kernel(const T* __restrict__ gicat,
                                      const T* __restrict__ h,
                                      T* __restrict__ h_new, T* __restrict__ r_o,
                                      T* __restrict__ z_o, T* __restrict__ n_o,
                                      T* __restrict__ hn_o, long NH, int H) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < NH;
       i += (long)gridDim.x * blockDim.x) {
    const long row = i / H;
    const int c = (int)(i - row * H);
    const long b = row * 4 * H + c;
    const float rs = to_f(gicat[b]);
    const float zs = to_f(gicat[b + H]);
    const float in_ = to_f(gicat[b + 2 * H]);
    const float hn = to_f(gicat[b + 3 * H]);
    const float r = sigmoidf_(rs);
    const float z = sigmoidf_(zs);
    const float n = tanhf(in_ + r * hn);
    const float hv = to_f(h[i]);
    h_new[i] = from_f<T>((1.f - z) * n + z * hv);
    r_o[i] = from_f<T>(r);
    z_o[i] = from_f<T>(z);
    n_o[i] = from_f<T>(n);
    hn_o[i] = from_f<T>(hn);
  }
}

// grad_gicat columns: [dpr | dpz | dpn | dpn*r]; grad_h_direct = go * z.
template <typename T>
__global__ void gru_gates2_bwd_kernel(const T* __restrict__ grad_h_new,
                                      const T* __restrict__ h,
                                      const T* __restrict__ r_i,
                                      const T* __restrict__ z_i,
                                      const T* __restrict__ n_i,
                                      const T* __restrict__ hn_i,
                                      T* __restrict__ grad_gicat,
                                      T* __restrict__ grad_h, long NH, int H) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < NH;
       i += (long)gridDim.x * blockDim.x) {
    const long row = i / H;
    const int c = (int)(i - row * H);
    const long b = row * 4 * H + c;
    const float go = to_f(grad_h_new[i]);
    const float r = to_f(r_i[i]), z = to_f(z_i[i]), n = to_f(n_i[i]);
    const float hn = to_f(hn_i[i]);
    const float hv = to_f(h[i]);
    const GruGate2Grad d = gru_gate2_bwd_elem(go, hv, r, z, n, hn);
    grad_gicat[b] = from_f<T>(d.dpr);
    grad_gicat[b + H] = from_f<T>(d.dpz);
    grad_gicat[b + 2 * H] = from_f<T>(d.dpn);
    grad_gicat[b + 3 * H] = from_f<T>(d.dpnr);
    grad_h[i] = from_f<T>(d.ghd);
  }
}

// ---------------------------------------------------------------------------
// Column sum (bias gradients): out[c] += sum_rows x[r][c], fp32 accumulate.
// Blocks tile (row-chunk, col-chunk); one atomicAdd per (block, column).
// ---------------------------------------------------------------------------

template <typename T>
__global__ void colsum_kernel(const T* __restrict__ x, float* __restrict__ out,
                              int N, int C, int rows_per_block) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  const int r0 = blockIdx.y * rows_per_block;
  const int r1 = min(r0 + rows_per_block, N);
  // 4 independent accumulators: the serial dependent-add chain otherwise
  // pays full memory latency per row (rocprof: 84 us -> ~4 us).
  float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
  int r = r0;
  for (; r + 4 <= r1; r += 4) {
    a0 += to_f(x[(long)r * C + c]);
    a1 += to_f(x[(long)(r + 1) * C + c]);
    a2 += to_f(x[(long)(r + 2) * C + c]);
    a3 += to_f(x[(long)(r + 3) * C + c]);
  }
  for (; r < r1; ++r) a0 += to_f(x[(long)r * C + c]);
  atomicAdd(out + c, (a0 + a1) + (a2 + a3));
}
//   fwd: alpha = softmax(gate[seg]); out[g] = sum_v alpha_v * x_v
//   bwd: grad_x = alpha * grad_out[g];  grad_gate = alpha*(s - <alpha,s>),
//        s_v = <grad_out[g], x_v>.
// Block-level reductions through one LDS scratch array.
// ---------------------------------------------------------------------------

__device__ float block_reduce(float v, float* scratch, int op /*0=max,1=sum*/) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int w = threadIdx.x / WAVE;
  // wave reduce
  for (int off = WAVE / 2; off > 0; off >>= 1) {
    const float o = __shfl_down(v, off);
    v = op == 0 ? fmaxf(v, o) : v + o;
  }
  if (lane == 0) scratch[w] = v;
  __syncthreads();
  const int nw = blockDim.x / WAVE;
  float out = scratch[0];
  if (threadIdx.x == 0) {
    for (int i = 1; i < nw; ++i) out = op == 0 ? fmaxf(out, scratch[i]) : out + scratch[i];
    scratch[0] = out;
  }
  __syncthreads();
  out = scratch[0];
  __syncthreads();
  return out;
}

template <typename T>
__global__ void attn_pool_fwd_kernel(const T* __restrict__ x,
                                     const T* __restrict__ gate,
                                     const int* __restrict__ node_offsets,
                                     T* __restrict__ out,
                                     float* __restrict__ alpha, int D) {
  __shared__ float scratch[8];
  const int g = blockIdx.x;
  const int lo = node_offsets[g], hi = node_offsets[g + 1];
  const int n = hi - lo;
  if (n <= 0) return;
  // phase A: segment max of gate
  float m = -3.4e38f;
  for (int v = threadIdx.x; v < n; v += blockDim.x) m = fmaxf(m, to_f(gate[lo + v]));
  m = block_reduce(m, scratch, 0);
  // phase B: exp/sum -> alpha
  float s = 0.f;
  for (int v = threadIdx.x; v < n; v += blockDim.x) {
    const float e = __expf(to_f(gate[lo + v]) - m);
    alpha[lo + v] = e;
    s += e;
  }
  s = block_reduce(s, scratch, 1);
  const float inv = 1.0f / s;
  for (int v = threadIdx.x; v < n; v += blockDim.x) alpha[lo + v] *= inv;
  __syncthreads();
  // phase C: weighted segment sum, one output column per thread (strided).
  // 8 independent accumulators: a 500-node graph is otherwise a serial
  // dependent-add chain at full memory latency (the kernel's whole cost).
  for (int d = threadIdx.x; d < D; d += blockDim.x) {
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f, a4 = 0.f, a5 = 0.f, a6 = 0.f, a7 = 0.f;
    int v = 0;
    for (; v + 8 <= n; v += 8) {
      const long base = (long)(lo + v) * D + d;
      a0 += alpha[lo + v] * to_f(x[base]);
      a1 += alpha[lo + v + 1] * to_f(x[base + D]);
      a2 += alpha[lo + v + 2] * to_f(x[base + 2 * D]);
      a3 += alpha[lo + v + 3] * to_f(x[base + 3 * D]);
      a4 += alpha[lo + v + 4] * to_f(x[base + 4 * D]);
      a5 += alpha[lo + v + 5] * to_f(x[base + 5 * D]);
      a6 += alpha[lo + v + 6] * to_f(x[base + 6 * D]);
      a7 += alpha[lo + v + 7] * to_f(x[base + 7 * D]);
    }
    for (; v < n; ++v) a0 += alpha[lo + v] * to_f(x[(long)(lo + v) * D + d]);
    out[(long)g * D + d] = from_f<T>(((a0 + a1) + (a2 + a3)) + ((a4 + a5) + (a6 + a7)));
  }
}

template <typename T>
__global__ void attn_pool_bwd_kernel(const T* __restrict__ grad_out,
                                     const T* __restrict__ x,
                                     const float* __restrict__ alpha,
                                     const int* __restrict__ node_offsets,
                                     T* __restrict__ grad_x,
                                     T* __restrict__ grad_gate,
                                     float* __restrict__ s_ws, int D) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* go = reinterpret_cast<float*>(smem);          // D floats
  float* scratch = go + D;                             // 8 floats
  const int g = blockIdx.x;
  const int lo = node_offsets[g], hi = node_offsets[g + 1];
  const int n = hi - lo;
  if (n <= 0) return;
  for (int d = threadIdx.x; d < D; d += blockDim.x)
    go[d] = to_f(grad_out[(long)g * D + d]);
  __syncthreads();
  // pass 1: s_v = <go, x_v> (one wave per node pair, 2-node ILP so the
  // dot-product latency chains of a 500-node graph overlap)
  const int wid = threadIdx.x / WAVE;
  const int lane = threadIdx.x & (WAVE - 1);
  const int nw = blockDim.x / WAVE;
  float local_dot = 0.f;
  for (int v = wid * 2; v < n; v += nw * 2) {
    float sv0 = 0.f, sv1 = 0.f;
    const bool has1 = (v + 1) < n;
    for (int d = lane; d < D; d += WAVE) {
      sv0 += go[d] * to_f(x[(long)(lo + v) * D + d]);
      if (has1) sv1 += go[d] * to_f(x[(long)(lo + v + 1) * D + d]);
    }
    for (int off = WAVE / 2; off > 0; off >>= 1) {
      sv0 += __shfl_down(sv0, off);
      sv1 += __shfl_down(sv1, off);
    }
    if (lane == 0) {
      s_ws[lo + v] = sv0;
      local_dot += alpha[lo + v] * sv0;
      if (has1) {
        s_ws[lo + v + 1] = sv1;
        local_dot += alpha[lo + v + 1] * sv1;
      }
    }
  }
  __syncthreads();
  const float dot = block_reduce(lane == 0 ? local_dot : 0.f, scratch, 1);
  // pass 2: outputs
  for (int v = wid; v < n; v += nw) {
    const float a = alpha[lo + v];
    for (int d = lane; d < D; d += WAVE)
      grad_x[(long)(lo + v) * D + d] = from_f<T>(a * go[d]);
    if (lane == 0) grad_gate[lo + v] = from_f<T>(a * (s_ws[lo + v] - dot));
  }
}

// ---------------------------------------------------------------------------
// K7: per-graph max of node values (graph label reduction).
// ---------------------------------------------------------------------------

__global__ void segment_max_kernel(const float* __restrict__ values,
                                   const int* __restrict__ node_offsets,
                                   float* __restrict__ out) {
  __shared__ float scratch[8];
  const int g = blockIdx.x;
  const int lo = node_offsets[g], hi = node_offsets[g + 1];
  float m = -3.4e38f;
  for (int v = lo + threadIdx.x; v < hi; v += blockDim.x) m = fmaxf(m, values[v]);
  m = block_reduce(m, scratch, 0);
  if (threadIdx.x == 0) out[g] = (hi > lo) ? m : 0.f;
}

// ---------------------------------------------------------------------------
// Launchers (called from bindings.cpp)
// ---------------------------------------------------------------------------

template <typename T, typename TO>
void launch_embed4_fwd2(const T* tables, const long* idx, TO* out, int N, int V,
                        hipStream_t stream) {
  const int waves_per_block = 4;
  const int block = WAVE * waves_per_block;
  const int grid = (N + waves_per_block - 1) / waves_per_block;
  if (grid > 0)
    hipLaunchKernelGGL((embed4_fwd_kernel<T, TO>), dim3(grid), dim3(block), 0,
                       stream, tables, idx, out, N, V);
}
template void launch_embed4_fwd2<float, __hip_bfloat16>(
    const float*, const long*, __hip_bfloat16*, int, int, hipStream_t);

template <typename T>
void launch_embed4_fwd(const T* tables, const long* idx, T* out, int N, int V,
                       hipStream_t stream) {
  launch_embed4_fwd2<T, T>(tables, idx, out, N, V, stream);
}

template <typename T>
void launch_embed4_bwd(const T* grad_out, const long* idx, float* grad_tables,
                       long total, int V, hipStream_t stream) {
  const int block = 256;
  // few blocks => few per-block LDS flushes of the hot rows
  const int grid = (int)min((total + block - 1) / block, (long)512);
  if (grid > 0)
    hipLaunchKernelGGL(embed4_bwd_kernel<T>, dim3(grid), dim3(block), 0, stream,
                       grad_out, idx, grad_tables, total, V);
}

template <typename T>
void launch_spmm_sum_strided(const int* indptr, const int* indices, const T* x,
                             T* out, int N, int D, long x_stride,
                             hipStream_t stream) {
  const int waves_per_block = 4;
  const int block = WAVE * waves_per_block;
  const int grid = (N + waves_per_block - 1) / waves_per_block;
  if (grid > 0)
    hipLaunchKernelGGL(spmm_sum_kernel<T>, dim3(grid), dim3(block), 0, stream,
                       indptr, indices, x, out, N, D, x_stride);
}

template <typename T>
void launch_spmm_sum(const int* indptr, const int* indices, const T* x, T* out,
                     int N, int D, hipStream_t stream) {
  launch_spmm_sum_strided<T>(indptr, indices, x, out, N, D, (long)D, stream);
}

template <typename T>
void launch_gru_gates_fwd(const T* gi, const T* gh, const T* h, T* h_new, T* r,
                          T* z, T* n, long NH, int H, hipStream_t stream) {
  const int block = 256;
  const int grid = (int)min((NH + block - 1) / block, (long)2048);
  if (grid > 0)
    hipLaunchKernelGGL(gru_gates_fwd_kernel<T>, dim3(grid), dim3(block), 0,
                       stream, gi, gh, h, h_new, r, z, n, NH, H);
}

template <typename T>
void launch_gru_gates_bwd(const T* grad_h_new, const T* gh, const T* h,
                          const T* r, const T* z, const T* n, T* grad_gi,
                          T* grad_gh, T* grad_h, long NH, int H,
                          hipStream_t stream) {
  const int block = 256;
  const int grid = (int)min((NH + block - 1) / block, (long)2048);
  if (grid > 0)
    hipLaunchKernelGGL(gru_gates_bwd_kernel<T>, dim3(grid), dim3(block), 0,
                       stream, grad_h_new, gh, h, r, z, n, grad_gi, grad_gh,
                       grad_h, NH, H);
}

template <typename T>
void launch_attn_pool_fwd(const T* x, const T* gate, const int* node_offsets,
                          T* out, float* alpha, int B, int D,
                          hipStream_t stream) {
  if (B > 0)
    hipLaunchKernelGGL(attn_pool_fwd_kernel<T>, dim3(B), dim3(256), 0, stream,
                       x, gate, node_offsets, out, alpha, D);
}

template <typename T>
void launch_attn_pool_bwd(const T* grad_out, const T* x, const float* alpha,
                          const int* node_offsets, T* grad_x, T* grad_gate,
                          float* s_ws, int B, int D, hipStream_t stream) {
  const size_t lds = (D + 8) * sizeof(float);
  if (B > 0)
    hipLaunchKernelGGL(attn_pool_bwd_kernel<T>, dim3(B), dim3(512), lds, stream,
                       grad_out, x, alpha, node_offsets, grad_x, grad_gate,
                       s_ws, D);
}

template <typename T>
void launch_gru_gates2_fwd(const T* gicat, const T* h, T* h_new, T* r, T* z,
                           T* n, T* hn, long NH, int H, hipStream_t stream) {
  const int block = 256;
  const int grid = (int)min((NH + block - 1) / block, (long)2048);
  if (grid > 0)
    hipLaunchKernelGGL(gru_gates2_fwd_kernel<T>, dim3(grid), dim3(block), 0,
                       stream, gicat, h, h_new, r, z, n, hn, NH, H);
}

template <typename T>
void launch_gru_gates2_bwd(const T* grad_h_new, const T* h, const T* r,
                           const T* z, const T* n, const T* hn, T* grad_gicat,
                           T* grad_h, long NH, int H, hipStream_t stream) {
  const int block = 256;
  const int grid = (int)min((NH + block - 1) / block, (long)2048);
  if (grid > 0)
    hipLaunchKernelGGL(gru_gates2_bwd_kernel<T>, dim3(grid), dim3(block), 0,
                       stream, grad_h_new, h, r, z, n, hn, grad_gicat, grad_h,
                       NH, H);
}

template <typename T>
void launch_colsum(const T* x, float* out, int N, int C, hipStream_t stream) {
  // narrow C (the GNN's 128-column grads): a 256-thread block would idle
  // half its lanes; shrink the block and the row chunk together
  const int block = (C < 256) ? ((C < 64) ? 64 : C) : 256;
  const int colb = (C + block - 1) / block;
  const int rows_per_block = (C < 256) ? 32 : 64;
  const int rowb = (N + rows_per_block - 1) / rows_per_block;
  if (N > 0 && C > 0)
    hipLaunchKernelGGL(colsum_kernel<T>, dim3(colb, rowb), dim3(block), 0,
                       stream, x, out, N, C, rows_per_block);
}

void launch_segment_max(const float* values, const int* node_offsets,
                        float* out, int B, hipStream_t stream) {
  if (B > 0)
    hipLaunchKernelGGL(segment_max_kernel, dim3(B), dim3(256), 0, stream,
                       values, node_offsets, out);
}

// explicit instantiations
#define INSTANTIATE(T)                                                        \
  template void launch_embed4_fwd<T>(const T*, const long*, T*, int, int,     \
                                     hipStream_t);                            \
  template void launch_embed4_bwd<T>(const T*, const long*, float*, long,     \
                                     int, hipStream_t);                       \
  template void launch_spmm_sum_strided<T>(const int*, const int*, const T*,  \
                                            T*, int, int, long, hipStream_t);  \
  template void launch_spmm_sum<T>(const int*, const int*, const T*, T*, int, \
                                   int, hipStream_t);                         \
  template void launch_gru_gates_fwd<T>(const T*, const T*, const T*, T*, T*, \
                                        T*, T*, long, int, hipStream_t);      \
  template void launch_gru_gates_bwd<T>(const T*, const T*, const T*,         \
                                        const T*, const T*, const T*, T*, T*, \
                                        T*, long, int, hipStream_t);          \
  template void launch_attn_pool_fwd<T>(const T*, const T*, const int*, T*,   \
                                        float*, int, int, hipStream_t);       \
  template void launch_attn_pool_bwd<T>(const T*, const T*, const float*,     \
                                        const int*, T*, T*, float*, int, int, \
                                        hipStream_t);                         \
  template void launch_gru_gates2_fwd<T>(const T*, const T*, T*, T*, T*, T*,  \
                                         T*, long, int, hipStream_t);         \
  template void launch_gru_gates2_bwd<T>(const T*, const T*, const T*,        \
                                         const T*, const T*, const T*, T*,    \
                                         T*, long, int, hipStream_t);         \
  template void launch_colsum<T>(const T*, float*, int, int, hipStream_t);

INSTANTIATE(float)
INSTANTIATE(__hip_bfloat16)

// Pack all derived GGNN weight buffers in ONE launch: bf16 casts of the
// step linear (W_e, b_e), the block gate matrix Wcat(4H,2H) =
// [[Wih_r|Whh_r],[Wih_z|Whh_z],[Wih_n|0],[0|Whh_n]] (+ its transpose) and
// the merged bias b_cat. Replaces the per-step chain of ~12 torch
// cast/narrow/cat/transpose nodes the fused-GGNN path needed (hipGraph
// replay overhead is per-node; see VERDICT round-1 item 4).
__global__ void pack_gru_weights_kernel(
    const float* __restrict__ W_e, const float* __restrict__ b_e,
    const float* __restrict__ W_ih, const float* __restrict__ W_hh,
    const float* __restrict__ b_ih, const float* __restrict__ b_hh, int H,
    __hip_bfloat16* __restrict__ w_e16, __hip_bfloat16* __restrict__ b_e16,
    __hip_bfloat16* __restrict__ Wcat, __hip_bfloat16* __restrict__ WcatT,
    __hip_bfloat16* __restrict__ b_cat, __hip_bfloat16* __restrict__ W_eT,
    __hip_bfloat16* __restrict__ Wcat_perm, __hip_bfloat16* __restrict__ b_perm) {
  const long HH_ = (long)H * H;
  const long WCAT = 8L * HH_;  // (4H, 2H)
  // index space: HH_ covers w_e16+W_eT, WCAT covers Wcat+WcatT (each index
  // writes the element AND its transpose twin), 4H b_cat, H b_e16
  const long total = HH_ + WCAT + 5L * H;
  const long stride = (long)gridDim.x * blockDim.x;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += stride) {
    long o = i;
    if (o < HH_) {  // w_e16 + W_eT
      const float v = W_e[o];
      w_e16[o] = __float2bfloat16(v);
      const long r = o / H, c = o % H;
      W_eT[c * H + r] = __float2bfloat16(v);
      continue;
    }
    o -= HH_;
    if (o < WCAT) {  // Wcat + WcatT, value by block
      const long r = o / (2 * H), c = o % (2 * H);
      const int gate = (int)(r / H);           // 0=r,1=z,2=n_i,3=n_h
      const long rr = r % H;
      float v = 0.f;
      if (c < H) {                              // W_ih side
        if (gate < 3) v = W_ih[(gate * H + rr) * (long)H + c];
      } else {                                  // W_hh side
        const long cc = c - H;
        if (gate < 2) v = W_hh[(gate * H + rr) * (long)H + cc];
        else if (gate == 3) v = W_hh[(2 * H + rr) * (long)H + cc];
      }
      const __hip_bfloat16 b = __float2bfloat16(v);
      Wcat[o] = b;
      WcatT[c * (4L * H) + r] = b;
      // gate-interleaved layout for the fused GEMM+GRU kernel: row j*4+g
      Wcat_perm[(rr * 4 + gate) * (2L * H) + c] = b;
      continue;
    }
    o -= WCAT;
    if (o < 4 * H) {  // b_cat
      float v;
      if (o < 2 * H) v = b_ih[o] + b_hh[o];
      else if (o < 3 * H) v = b_ih[o];
      else v = b_hh[o - H];
      const __hip_bfloat16 bb = __float2bfloat16(v);
      b_cat[o] = bb;
      b_perm[(o % H) * 4 + (o / H)] = bb;
      continue;
    }
    o -= 4L * H;
    if (o < H) b_e16[o] = __float2bfloat16(b_e[o]);
  }
}

void launch_pack_gru_weights(const float* W_e, const float* b_e,
                             const float* W_ih, const float* W_hh,
                             const float* b_ih, const float* b_hh, int H,
                             __hip_bfloat16* w_e16, __hip_bfloat16* b_e16,
                             __hip_bfloat16* Wcat, __hip_bfloat16* WcatT,
                             __hip_bfloat16* b_cat, __hip_bfloat16* W_eT,
                             __hip_bfloat16* Wcat_perm, __hip_bfloat16* b_perm,
                             hipStream_t stream) {
  const long total = (long)H * H + 8L * H * H + 5L * H;
  const int block = 256;
  const int grid = (int)min((total + block - 1) / block, (long)1024);
  hipLaunchKernelGGL(pack_gru_weights_kernel, dim3(grid), dim3(block), 0,
                     stream, W_e, b_e, W_ih, W_hh, b_ih, b_hh, H, w_e16, b_e16,
                     Wcat, WcatT, b_cat, W_eT, Wcat_perm, b_perm);
}

// The graph-level head (gate + attention pool, 3-layer MLP) lives in
// csrc/graph_head.hip.

// Fused BCE-with-logits (mean over weighted graphs) + backward seed. The
// torch chain (binary_cross_entropy_with_logits fwd + mean + backward's
// sigmoid/sub/scale, ~6 nodes at batch-256 launch-floor sizes) becomes
// one tiny kernel per direction. Supports pos_weight and the capture
// padding weight mask (loss = sum w*bce / sum w).
__global__ void bce_logits_fwd_kernel(
    const float* __restrict__ logits, const float* __restrict__ labels,
    const float* __restrict__ weight, const float* __restrict__ pos_weight,
    float* __restrict__ out2 /* {loss_num, w_sum} */, int B) {
  __shared__ float red[2][8];
  float acc = 0.f, wacc = 0.f;
  const float pw = pos_weight ? pos_weight[0] : 1.0f;
  for (int i = threadIdx.x; i < B; i += blockDim.x) {
    const float z = logits[i];
    const float y = labels[i];
    const float w = weight ? weight[i] : 1.0f;
    // log(1+exp(-|z|)) form is exact and overflow-safe
    const float sp_pos = log1pf(__expf(-fabsf(z))) + fmaxf(-z, 0.f);  // -log sig(z)
    const float sp_neg = log1pf(__expf(-fabsf(z))) + fmaxf(z, 0.f);   // -log(1-sig(z))
    acc += w * (pw * y * sp_pos + (1.f - y) * sp_neg);
    wacc += w;
  }
  const int lane = threadIdx.x & (WAVE - 1);
  const int wv = threadIdx.x / WAVE;
  for (int off = WAVE / 2; off > 0; off >>= 1) {
    acc += __shfl_down(acc, off);
    wacc += __shfl_down(wacc, off);
  }
  if (lane == 0) {
    red[0][wv] = acc;
    red[1][wv] = wacc;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float a = 0.f, w = 0.f;
    for (int i = 0; i < (int)(blockDim.x / WAVE); ++i) {
      a += red[0][i];
      w += red[1][i];
    }
    out2[0] = a / fmaxf(w, 1.0f);  // the mean loss itself
    out2[1] = w;
  }
}

__global__ void bce_logits_bwd_kernel(
    const float* __restrict__ logits, const float* __restrict__ labels,
    const float* __restrict__ weight, const float* __restrict__ pos_weight,
    const float* __restrict__ grad /* upstream scalar */,
    const float* __restrict__ out2 /* {_, w_sum} */,
    float* __restrict__ dlogits, int B) {
  const float pw = pos_weight ? pos_weight[0] : 1.0f;
  const float g = grad[0] / fmaxf(out2[1], 1.0f);
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < B;
       i += gridDim.x * blockDim.x) {
    const float z = logits[i];
    const float y = labels[i];
    const float w = weight ? weight[i] : 1.0f;
    const float sig = 1.0f / (1.0f + __expf(-z));
    // d/dz [pw*y*softplus(-z) + (1-y)*softplus(z)]
    const float d = pw * y * (sig - 1.0f) + (1.0f - y) * sig;
    dlogits[i] = w * g * d;
  }
}

void launch_bce_logits_fwd(const float* logits, const float* labels,
                           const float* weight, const float* pos_weight,
                           float* out2, int B, hipStream_t stream) {
  hipLaunchKernelGGL(bce_logits_fwd_kernel, dim3(1), dim3(256), 0, stream,
                     logits, labels, weight, pos_weight, out2, B);
}

void launch_bce_logits_bwd(const float* logits, const float* labels,
                           const float* weight, const float* pos_weight,
                           const float* grad, const float* out2,
                           float* dlogits, int B, hipStream_t stream) {
  const int grid = (B + 255) / 256;
  hipLaunchKernelGGL(bce_logits_bwd_kernel, dim3(grid), dim3(256), 0, stream,
                     logits, labels, weight, pos_weight, grad, out2, dlogits, B);
}
