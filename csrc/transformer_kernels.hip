// Transformer kernels for MI355X (gfx950): fused LayerNorm, bias+GELU and
// masked row-softmax, forward + backward, bf16/fp32 IO with fp32 math.
//
// These cover the fused elementwise/normalization work of the LineVul
// RoBERTa encoder and the CodeT5 stack; the plain
// GEMMs (QKV/FFN projections) go to rocBLAS/hipBLASLt, the weight-grad
// GEMMs to csrc/wgrad.hip when hipBLASLt's picks are pathological.
//
// Geometry notes: hidden D = 768 (12 elems/lane on a 64-wide wave) or 3072;
// softmax rows are seq-length 512 (8/lane). One wave per row everywhere,
// 4 rows per 256-thread block; fp32 statistics.

#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>

#include <algorithm>
using std::max;
using std::min;

#define WAVE 64

template <typename T> __device__ __forceinline__ float tf(T v);
template <> __device__ __forceinline__ float tf<float>(float v) { return v; }
template <> __device__ __forceinline__ float tf<__hip_bfloat16>(__hip_bfloat16 v) {
  return __bfloat162float(v);
}
template <typename T> __device__ __forceinline__ T ff(float v);
template <> __device__ __forceinline__ float ff<float>(float v) { return v; }
template <> __device__ __forceinline__ __hip_bfloat16 ff<__hip_bfloat16>(float v) {
  return __float2bfloat16(v);
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int off = WAVE / 2; off > 0; off >>= 1) v += __shfl_down(v, off);
  return __shfl(v, 0);
}

// 4-element vector IO for the row kernels (scalar 2-B element loads waste
// 8x load-issue bandwidth on a bandwidth-bound kernel)
struct f4 {
  float v[4];
};
template <typename T> __device__ __forceinline__ f4 load4(const T* p);
template <> __device__ __forceinline__ f4 load4<float>(const float* p) {
  const float4 a = *reinterpret_cast<const float4*>(p);
  return {a.x, a.y, a.z, a.w};
}
template <> __device__ __forceinline__ f4 load4<__hip_bfloat16>(const __hip_bfloat16* p) {
  __hip_bfloat16 b[4];
  *reinterpret_cast<unsigned long long*>(b) = *reinterpret_cast<const unsigned long long*>(p);
  return {__bfloat162float(b[0]), __bfloat162float(b[1]), __bfloat162float(b[2]),
          __bfloat162float(b[3])};
}
template <typename T> __device__ __forceinline__ void store4(T* p, const f4& a);
template <> __device__ __forceinline__ void store4<float>(float* p, const f4& a) {
  *reinterpret_cast<float4*>(p) = {a.v[0], a.v[1], a.v[2], a.v[3]};
}
template <> __device__ __forceinline__ void store4<__hip_bfloat16>(__hip_bfloat16* p,
                                                                   const f4& a) {
  __hip_bfloat16 b[4] = {__float2bfloat16(a.v[0]), __float2bfloat16(a.v[1]),
                         __float2bfloat16(a.v[2]), __float2bfloat16(a.v[3])};
  *reinterpret_cast<unsigned long long*>(p) = *reinterpret_cast<const unsigned long long*>(b);
}

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int off = WAVE / 2; off > 0; off >>= 1) v = fmaxf(v, __shfl_down(v, off));
  return __shfl(v, 0);
}

// ---------------------------------------------------------------------------
// LayerNorm: y = (x - mean) * rstd * gamma + beta  (per row of D)
// ---------------------------------------------------------------------------

// vector iterations of a row the forward kernels keep in registers between
// their passes (mean, centred variance, output): D <= 4 * 256 = 1024
#define LN_CACHE_IT 4

template <typename T>
__global__ void layernorm_fwd_kernel(const T* __restrict__ x,
                                     const float* __restrict__ gamma,
                                     const float* __restrict__ beta,
                                     T* __restrict__ y, float* __restrict__ mean,
                                     float* __restrict__ rstd, long N, int D,
                                     float eps) {
  const long row = (long)(blockIdx.x * (blockDim.x / WAVE)) + threadIdx.x / WAVE;
  const int lane = threadIdx.x & (WAVE - 1);
  if (row >= N) return;
  const T* xr = x + row * D;
  const bool vec = (D % (WAVE * 4) == 0);
  // Mean from sums shifted by the row's first element (a constant row gives
  // mu == x0 exactly), then a second pass centred on mu for the variance:
  // the one-pass s2/D - mu*mu cancels catastrophically once |mean| >> std
  // and can go negative.
  const float x0 = tf(xr[0]);
  T* yr = y + row * D;
  if (vec && D <= LN_CACHE_IT * WAVE * 4) {
    // the row stays in registers across the three passes: one read of x
    f4 c[LN_CACHE_IT];
    float s = 0.f;
#pragma unroll
    for (int it = 0; it < LN_CACHE_IT; ++it) {
      const int d = (it * WAVE + lane) * 4;
      if (d < D) {
        c[it] = load4(xr + d);
#pragma unroll
        for (int u = 0; u < 4; ++u) s += c[it].v[u] - x0;
      }
    }
    const float mu = x0 + wave_sum(s) / D;
    float s2 = 0.f;
#pragma unroll
    for (int it = 0; it < LN_CACHE_IT; ++it) {
      if ((it * WAVE + lane) * 4 < D) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          c[it].v[u] -= mu;
          s2 += c[it].v[u] * c[it].v[u];
        }
      }
    }
    const float rs = rsqrtf(wave_sum(s2) / D + eps);
    if (lane == 0) {
      mean[row] = mu;
      rstd[row] = rs;
    }
#pragma unroll
    for (int it = 0; it < LN_CACHE_IT; ++it) {
      const int d = (it * WAVE + lane) * 4;
      if (d < D) {
        const f4 g = load4(gamma + d);
        const f4 bb = load4(beta + d);
        f4 o;
#pragma unroll
        for (int u = 0; u < 4; ++u) o.v[u] = c[it].v[u] * rs * g.v[u] + bb.v[u];
        store4(yr + d, o);
      }
    }
    return;
  }
  // wider or unaligned rows: the second and third pass re-read the row
  // (L1/L2-resident)
  float s = 0.f;
  if (vec) {
    for (int d = lane * 4; d < D; d += WAVE * 4) {
      const f4 a = load4(xr + d);
#pragma unroll
      for (int u = 0; u < 4; ++u) s += a.v[u] - x0;
    }
  } else {
    for (int d = lane; d < D; d += WAVE) s += tf(xr[d]) - x0;
  }
  const float mu = x0 + wave_sum(s) / D;
  float s2 = 0.f;
  if (vec) {
    for (int d = lane * 4; d < D; d += WAVE * 4) {
      const f4 a = load4(xr + d);
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const float c = a.v[u] - mu;
        s2 += c * c;
      }
    }
  } else {
    for (int d = lane; d < D; d += WAVE) {
      const float c = tf(xr[d]) - mu;
      s2 += c * c;
    }
  }
  const float var = wave_sum(s2) / D;  // a sum of squares: never negative
  const float rs = rsqrtf(var + eps);
  if (lane == 0) {
    mean[row] = mu;
    rstd[row] = rs;
  }
  if (vec) {
    for (int d = lane * 4; d < D; d += WAVE * 4) {
      const f4 a = load4(xr + d);
      const f4 g = load4(gamma + d);
      const f4 bb = load4(beta + d);
      f4 o;
#pragma unroll
      for (int u = 0; u < 4; ++u) o.v[u] = (a.v[u] - mu) * rs * g.v[u] + bb.v[u];
      store4(yr + d, o);
    }
  } else {
    for (int d = lane; d < D; d += WAVE)
      yr[d] = ff<T>((tf(xr[d]) - mu) * rs * gamma[d] + beta[d]);
  }
}

// dx = rstd * (dyg - mean_d(dyg) - xhat * mean_d(dyg * xhat)), dyg = dy*gamma
template <typename T>
__global__ void layernorm_bwd_kernel(const T* __restrict__ dy,
                                     const T* __restrict__ x,
                                     const float* __restrict__ gamma,
                                     const float* __restrict__ mean,
                                     const float* __restrict__ rstd,
                                     T* __restrict__ dx, long N, int D) {
  const long row = (long)(blockIdx.x * (blockDim.x / WAVE)) + threadIdx.x / WAVE;
  const int lane = threadIdx.x & (WAVE - 1);
  if (row >= N) return;
  const T* dyr = dy + row * D;
  const T* xr = x + row * D;
  const float mu = mean[row], rs = rstd[row];
  const bool vec = (D % (WAVE * 4) == 0);
  float c1 = 0.f, c2 = 0.f;
  if (vec) {
    for (int d = lane * 4; d < D; d += WAVE * 4) {
      const f4 a = load4(xr + d);
      const f4 dyv = load4(dyr + d);
      const f4 g4 = load4(gamma + d);
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const float g = dyv.v[u] * g4.v[u];
        c1 += g;
        c2 += g * (a.v[u] - mu) * rs;
      }
    }
  } else {
    for (int d = lane; d < D; d += WAVE) {
      const float xh = (tf(xr[d]) - mu) * rs;
      const float g = tf(dyr[d]) * gamma[d];
      c1 += g;
      c2 += g * xh;
    }
  }
  c1 = wave_sum(c1) / D;
  c2 = wave_sum(c2) / D;
  T* dxr = dx + row * D;
  if (vec) {
    for (int d = lane * 4; d < D; d += WAVE * 4) {
      const f4 a = load4(xr + d);
      const f4 dyv = load4(dyr + d);
      const f4 g4 = load4(gamma + d);
      f4 o;
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const float xh = (a.v[u] - mu) * rs;
        o.v[u] = rs * (dyv.v[u] * g4.v[u] - c1 - xh * c2);
      }
      store4(dxr + d, o);
    }
  } else {
    for (int d = lane; d < D; d += WAVE) {
      const float xh = (tf(xr[d]) - mu) * rs;
      const float g = tf(dyr[d]) * gamma[d];
      dxr[d] = ff<T>(rs * (g - c1 - xh * c2));
    }
  }
}

// per-column reductions: dgamma[d] = sum_rows dy*xhat, dbeta[d] = sum_rows dy
template <typename T>
__global__ void layernorm_wgrad_kernel(const T* __restrict__ dy,
                                       const T* __restrict__ x,
                                       const float* __restrict__ mean,
                                       const float* __restrict__ rstd,
                                       float* __restrict__ dgamma,
                                       float* __restrict__ dbeta, long N, int D,
                                       int rows_per_block) {
  const int d = blockIdx.x * blockDim.x + threadIdx.x;
  if (d >= D) return;
  const long r0 = (long)blockIdx.y * rows_per_block;
  const long r1 = min((long)(r0 + rows_per_block), N);
  // 4 independent accumulator pairs: the single-pair form serializes on
  // the fma chain (dependent-latency bound, 5x the streaming roofline)
  float dg[4] = {}, db[4] = {};
  long r = r0;
  for (; r + 4 <= r1; r += 4) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const float g = tf(dy[(r + u) * D + d]);
      dg[u] += g * (tf(x[(r + u) * D + d]) - mean[r + u]) * rstd[r + u];
      db[u] += g;
    }
  }
  for (; r < r1; ++r) {
    const float g = tf(dy[r * D + d]);
    dg[0] += g * (tf(x[r * D + d]) - mean[r]) * rstd[r];
    db[0] += g;
  }
  atomicAdd(dgamma + d, dg[0] + dg[1] + dg[2] + dg[3]);
  atomicAdd(dbeta + d, db[0] + db[1] + db[2] + db[3]);
}


// ---------------------------------------------------------------------------
// RMSNorm (T5LayerNorm): y = x * rsqrt(mean(x^2) + eps) * gamma.
// T5 computes the variance in fp32 and casts the normalized value to the
// weight dtype before multiplying; here: fp32 math, IO dtype T.
// ---------------------------------------------------------------------------

template <typename T>
__global__ void rmsnorm_fwd_kernel(const T* __restrict__ x,
                                   const float* __restrict__ gamma,
                                   T* __restrict__ y, float* __restrict__ rstd,
                                   long N, int D, float eps) {
  const long row = (long)(blockIdx.x * (blockDim.x / WAVE)) + threadIdx.x / WAVE;
  const int lane = threadIdx.x & (WAVE - 1);
  if (row >= N) return;
  const T* xr = x + row * D;
  const bool vec = (D % (WAVE * 4) == 0);
  float s2 = 0.f;
  if (vec) {
    for (int d = lane * 4; d < D; d += WAVE * 4) {
      const f4 a = load4(xr + d);
#pragma unroll
      for (int u = 0; u < 4; ++u) s2 += a.v[u] * a.v[u];
    }
  } else {
    for (int d = lane; d < D; d += WAVE) {
      const float v = tf(xr[d]);
      s2 += v * v;
    }
  }
  s2 = wave_sum(s2);
  const float rs = rsqrtf(s2 / D + eps);
  if (lane == 0) rstd[row] = rs;
  T* yr = y + row * D;
  if (vec) {
    for (int d = lane * 4; d < D; d += WAVE * 4) {
      const f4 a = load4(xr + d);
      const f4 g = load4(gamma + d);
      f4 o;
#pragma unroll
      for (int u = 0; u < 4; ++u) o.v[u] = a.v[u] * rs * g.v[u];
      store4(yr + d, o);
    }
  } else {
    for (int d = lane; d < D; d += WAVE) yr[d] = ff<T>(tf(xr[d]) * rs * gamma[d]);
  }
}

// dx = rs * (dyg - xhat * mean_d(dyg * xhat)); xhat = x * rs; dyg = dy*gamma
template <typename T>
__global__ void rmsnorm_bwd_kernel(const T* __restrict__ dy,
                                   const T* __restrict__ x,
                                   const float* __restrict__ gamma,
                                   const float* __restrict__ rstd,
                                   T* __restrict__ dx, long N, int D) {
  const long row = (long)(blockIdx.x * (blockDim.x / WAVE)) + threadIdx.x / WAVE;
  const int lane = threadIdx.x & (WAVE - 1);
  if (row >= N) return;
  const T* dyr = dy + row * D;
  const T* xr = x + row * D;
  const float rs = rstd[row];
  const bool vec = (D % (WAVE * 4) == 0);
  float c2 = 0.f;
  if (vec) {
    for (int d = lane * 4; d < D; d += WAVE * 4) {
      const f4 a = load4(xr + d);
      const f4 dyv = load4(dyr + d);
      const f4 g4 = load4(gamma + d);
#pragma unroll
      for (int u = 0; u < 4; ++u) c2 += dyv.v[u] * g4.v[u] * a.v[u] * rs;
    }
  } else {
    for (int d = lane; d < D; d += WAVE) {
      const float xh = tf(xr[d]) * rs;
      c2 += tf(dyr[d]) * gamma[d] * xh;
    }
  }
  c2 = wave_sum(c2) / D;
  T* dxr = dx + row * D;
  if (vec) {
    for (int d = lane * 4; d < D; d += WAVE * 4) {
      const f4 a = load4(xr + d);
      const f4 dyv = load4(dyr + d);
      const f4 g4 = load4(gamma + d);
      f4 o;
#pragma unroll
      for (int u = 0; u < 4; ++u)
        o.v[u] = rs * (dyv.v[u] * g4.v[u] - a.v[u] * rs * c2);
      store4(dxr + d, o);
    }
  } else {
    for (int d = lane; d < D; d += WAVE) {
      const float xh = tf(xr[d]) * rs;
      dxr[d] = ff<T>(rs * (tf(dyr[d]) * gamma[d] - xh * c2));
    }
  }
}

template <typename T>
__global__ void rmsnorm_wgrad_kernel(const T* __restrict__ dy,
                                     const T* __restrict__ x,
                                     const float* __restrict__ rstd,
                                     float* __restrict__ dgamma, long N, int D,
                                     int rows_per_block) {
  const int d = blockIdx.x * blockDim.x + threadIdx.x;
  if (d >= D) return;
  const long r0 = (long)blockIdx.y * rows_per_block;
  const long r1 = min((long)(r0 + rows_per_block), N);
  float dg[4] = {};  // 4 chains: see layernorm_wgrad_kernel
  long r = r0;
  for (; r + 4 <= r1; r += 4) {
#pragma unroll
    for (int u = 0; u < 4; ++u)
      dg[u] += tf(dy[(r + u) * D + d]) * tf(x[(r + u) * D + d]) * rstd[r + u];
  }
  for (; r < r1; ++r) dg[0] += tf(dy[r * D + d]) * tf(x[r * D + d]) * rstd[r];
  atomicAdd(dgamma + d, dg[0] + dg[1] + dg[2] + dg[3]);
}

// ---------------------------------------------------------------------------
// bias + GELU (erf form, matching torch F.gelu / HF "gelu")
// ---------------------------------------------------------------------------

// Abramowitz-Stegun 7.1.26 erf (max abs error 1.5e-7 — far below bf16):
// ~10 VALU + the ONE exp(-z^2) that the GELU derivative's pdf term needs
// anyway; libdevice erff was ~2x the whole kernel's VALU budget
// (bias_gelu_bwd measured 50.8 us vs ~24 roofline).
__device__ __forceinline__ float erf_as_f(float z, float expmz2) {
  const float az = fabsf(z);
  const float t = 1.0f / (1.0f + 0.3275911f * az);
  float poly = 1.061405429f;
  poly = poly * t - 1.453152027f;
  poly = poly * t + 1.421413741f;
  poly = poly * t - 0.284496736f;
  poly = poly * t + 0.254829592f;
  const float e = 1.0f - poly * t * expmz2;
  return z < 0.f ? -e : e;
}
__device__ __forceinline__ float gelu_f(float v) {
  const float z = v * 0.70710678118654752f;
  const float s = __expf(-0.5f * v * v);  // == exp(-z^2)
  return 0.5f * v * (1.0f + erf_as_f(z, s));
}
__device__ __forceinline__ float gelu_grad_f(float v) {
  const float z = v * 0.70710678118654752f;
  const float s = __expf(-0.5f * v * v);
  const float cdf = 0.5f * (1.0f + erf_as_f(z, s));
  const float pdf = 0.3989422804014327f * s;
  return cdf + v * pdf;
}

// 16-B vectors per lane (8 bf16 / 4 fp32); D % VEC == 0 (host-checked)
template <typename T>
__global__ void bias_gelu_fwd_kernel(const T* __restrict__ x,
                                     const float* __restrict__ bias,
                                     T* __restrict__ y, long total, int D) {
  // 4 independent 16-B vectors in flight per iteration (latency), bias
  // column tracked incrementally (one modulo at entry; a per-vector 64-bit
  // modulo costs ~20 VALU ops), bias row staged in LDS (per-element global
  // bias loads were 64 scalar vmem ops per iteration on a streaming kernel)
  constexpr int VEC = 16 / sizeof(T);
  extern __shared__ float bias_lds[];
  for (int i = threadIdx.x; i < D; i += blockDim.x) bias_lds[i] = bias[i];
  __syncthreads();
  const long nvec = total / VEC;
  const long stride = (long)gridDim.x * blockDim.x;
  const int step = (int)((stride * VEC) % D);
  long iv = (long)blockIdx.x * blockDim.x + threadIdx.x;
  int d0 = (int)((iv * VEC) % D);
  for (; iv < nvec; iv += stride * 4) {
    T vx[4][VEC], vy[4][VEC];
    int ds[4];
    int d = d0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const long i = iv + r * stride;
      ds[r] = d;
      d += step;
      if (d >= D) d -= D;
      if (i < nvec)
        *reinterpret_cast<ulonglong2*>(vx[r]) =
            *reinterpret_cast<const ulonglong2*>(x + i * VEC);
    }
    d0 = d;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const long i = iv + r * stride;
      if (i >= nvec) continue;
      float b[VEC];
#pragma unroll
      for (int u = 0; u < VEC; u += 4)
        *reinterpret_cast<float4*>(b + u) =
            *reinterpret_cast<const float4*>(bias_lds + ds[r] + u);
#pragma unroll
      for (int u = 0; u < VEC; ++u)
        vy[r][u] = ff<T>(gelu_f(tf(vx[r][u]) + b[u]));
      *reinterpret_cast<ulonglong2*>(y + i * VEC) =
          *reinterpret_cast<ulonglong2*>(vy[r]);
    }
  }
}

template <typename T>
__global__ void bias_gelu_bwd_kernel(const T* __restrict__ dy,
                                     const T* __restrict__ x,
                                     const float* __restrict__ bias,
                                     T* __restrict__ dx, long total, int D) {
  constexpr int VEC = 16 / sizeof(T);
  extern __shared__ float bias_lds[];
  for (int i = threadIdx.x; i < D; i += blockDim.x) bias_lds[i] = bias[i];
  __syncthreads();
  const long nvec = total / VEC;
  const long stride = (long)gridDim.x * blockDim.x;
  const int step = (int)((stride * VEC) % D);
  long iv = (long)blockIdx.x * blockDim.x + threadIdx.x;
  int d0 = (int)((iv * VEC) % D);
  for (; iv < nvec; iv += stride * 4) {
    T vdy[4][VEC], vx[4][VEC], vdx[4][VEC];
    int ds[4];
    int d = d0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const long i = iv + r * stride;
      ds[r] = d;
      d += step;
      if (d >= D) d -= D;
      if (i < nvec) {
        *reinterpret_cast<ulonglong2*>(vdy[r]) =
            *reinterpret_cast<const ulonglong2*>(dy + i * VEC);
        *reinterpret_cast<ulonglong2*>(vx[r]) =
            *reinterpret_cast<const ulonglong2*>(x + i * VEC);
      }
    }
    d0 = d;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const long i = iv + r * stride;
      if (i >= nvec) continue;
      float b[VEC];
#pragma unroll
      for (int u = 0; u < VEC; u += 4)
        *reinterpret_cast<float4*>(b + u) =
            *reinterpret_cast<const float4*>(bias_lds + ds[r] + u);
#pragma unroll
      for (int u = 0; u < VEC; ++u)
        vdx[r][u] = ff<T>(tf(vdy[r][u]) * gelu_grad_f(tf(vx[r][u]) + b[u]));
      *reinterpret_cast<ulonglong2*>(dx + i * VEC) =
          *reinterpret_cast<ulonglong2*>(vdx[r]);
    }
  }
}

// ---------------------------------------------------------------------------
// Masked scaled row-softmax over attention scores.
// S (R, L) where R = B*H*L rows; key positions >= valid[b] get -inf.
// P = softmax(S * scale + mask). One wave per row.
// ---------------------------------------------------------------------------

// Stateless dropout RNG (regenerated identically in backward — no mask
// storage). One 32-bit hash yields keep-bytes for FOUR consecutive
// elements (per-element 64-bit hashing measurably slowed the softmax).
__device__ __forceinline__ unsigned hash4(unsigned long long quad_idx,
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

// keep element `idx` with probability 1-p (p8 = p * 256, byte compare)
__device__ __forceinline__ bool keep_mask(unsigned long long idx,
                                          unsigned long long seed,
                                          unsigned p8) {
  const unsigned h = hash4(idx >> 2, seed);
  const unsigned byte = (h >> (8 * ((unsigned)idx & 3))) & 0xFF;
  return byte >= p8;
}

// 8 bf16 / 8 fp32-pair loads per lane (one row of L<=512 in registers).
template <typename T>
__global__ void softmax_mask_fwd_kernel(const T* __restrict__ S,
                                        const int* __restrict__ valid,
                                        T* __restrict__ P, T* __restrict__ Pd,
                                        long R, int L, int rows_per_batch,
                                        float scale, float dropout_p,
                                        unsigned long long seed, int causal,
                                        int Lq) {
  const long row = (long)(blockIdx.x * (blockDim.x / WAVE)) + threadIdx.x / WAVE;
  const int lane = threadIdx.x & (WAVE - 1);
  if (row >= R) return;
  // clamp: a valid[b] outside [0, L] would read past the row
  int vl = valid ? max(0, min(valid[row / rows_per_batch], L)) : L;
  if (causal) vl = min(vl, (int)(row % Lq) + 1);
  const T* sr = S + row * L;
  constexpr int VEC = 16 / sizeof(T);  // one 16-B vector store per lane
  const int niter = (L + WAVE * VEC - 1) / (WAVE * VEC);
  float v[4][VEC];  // supports L <= 4*WAVE*VEC (host-checked)
  float m = -3.4e38f;
  for (int it = 0; it < niter; ++it) {
    const int j0 = (it * WAVE + lane) * VEC;
#pragma unroll
    for (int u = 0; u < VEC; ++u) {
      const int j = j0 + u;
      v[it][u] = (j < vl) ? tf(sr[j]) * scale : -3.4e38f;
      m = fmaxf(m, v[it][u]);
    }
  }
  m = wave_max(m);
  float sum = 0.f;
  for (int it = 0; it < niter; ++it)
#pragma unroll
    for (int u = 0; u < VEC; ++u) {
      v[it][u] = (v[it][u] > -3.0e38f) ? __expf(v[it][u] - m) : 0.f;
      sum += v[it][u];
    }
  sum = wave_sum(sum);
  const float inv = (sum > 0.f) ? 1.0f / sum : 0.f;
  const unsigned p8 = (unsigned)(dropout_p * 256.0f);
  // match the byte-quantized keep threshold: P(keep) = (256-p8)/256
  const float dscale = (p8 > 0) ? 256.0f / (256.0f - p8) : 1.0f;
  for (int it = 0; it < niter; ++it) {
    const int j0 = (it * WAVE + lane) * VEC;
    T pv[VEC], pdv[VEC];
#pragma unroll
    for (int u = 0; u < VEC; ++u) {
      const float p = v[it][u] * inv;
      pv[u] = ff<T>(p);
      if (Pd) {
        const bool keep = (p8 == 0) || keep_mask(row * L + j0 + u, seed, p8);
        pdv[u] = ff<T>(keep ? p * dscale : 0.f);
      }
    }
    if (j0 < L) {
      *reinterpret_cast<ulonglong2*>(P + row * L + j0) = *reinterpret_cast<ulonglong2*>(pv);
      if (Pd)
        *reinterpret_cast<ulonglong2*>(Pd + row * L + j0) = *reinterpret_cast<ulonglong2*>(pdv);
    }
  }
}

// dS = scale * P * (dP - sum_j(dP * P)); dP = dPd * mask / (1-p) regenerated
template <typename T>
__global__ void softmax_mask_bwd_kernel(const T* __restrict__ dPd,
                                        const T* __restrict__ P,
                                        T* __restrict__ dS, long R, int L,
                                        float scale, float dropout_p,
                                        unsigned long long seed) {
  const long row = (long)(blockIdx.x * (blockDim.x / WAVE)) + threadIdx.x / WAVE;
  const int lane = threadIdx.x & (WAVE - 1);
  if (row >= R) return;
  const T* dpr = dPd + row * L;
  const T* pr = P + row * L;
  constexpr int VEC = 16 / sizeof(T);
  const int niter = (L + WAVE * VEC - 1) / (WAVE * VEC);
  const unsigned p8 = (unsigned)(dropout_p * 256.0f);
  // match the byte-quantized keep threshold: P(keep) = (256-p8)/256
  const float dscale = (p8 > 0) ? 256.0f / (256.0f - p8) : 1.0f;
  float dp[4][VEC], p[4][VEC];
  float dot = 0.f;
  for (int it = 0; it < niter; ++it) {
    const int j0 = (it * WAVE + lane) * VEC;
    if (j0 < L) {
#pragma unroll
      for (int u = 0; u < VEC; ++u) {
        const int j = j0 + u;
        const bool keep = (p8 == 0) || keep_mask(row * L + j, seed, p8);
        dp[it][u] = keep ? tf(dpr[j]) * dscale : 0.f;
        p[it][u] = tf(pr[j]);
        dot += dp[it][u] * p[it][u];
      }
    }
  }
  dot = wave_sum(dot);
  for (int it = 0; it < niter; ++it) {
    const int j0 = (it * WAVE + lane) * VEC;
    if (j0 < L) {
      T out[VEC];
#pragma unroll
      for (int u = 0; u < VEC; ++u)
        out[u] = ff<T>(scale * p[it][u] * (dp[it][u] - dot));
      *reinterpret_cast<ulonglong2*>(dS + row * L + j0) = *reinterpret_cast<ulonglong2*>(out);
    }
  }
}

// ---------------------------------------------------------------------------
// Launchers
// ---------------------------------------------------------------------------

#define ROWS_PER_BLOCK 4

template <typename T>
void launch_layernorm_fwd(const T* x, const float* gamma, const float* beta,
                          T* y, float* mean, float* rstd, long N, int D,
                          float eps, hipStream_t stream) {
  const int grid = (int)((N + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK);
  if (grid)
    hipLaunchKernelGGL(layernorm_fwd_kernel<T>, dim3(grid),
                       dim3(WAVE * ROWS_PER_BLOCK), 0, stream, x, gamma, beta, y,
                       mean, rstd, N, D, eps);
}

template <typename T>
void launch_layernorm_bwd(const T* dy, const T* x, const float* gamma,
                          const float* mean, const float* rstd, T* dx, long N,
                          int D, hipStream_t stream) {
  const int grid = (int)((N + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK);
  if (grid)
    hipLaunchKernelGGL(layernorm_bwd_kernel<T>, dim3(grid),
                       dim3(WAVE * ROWS_PER_BLOCK), 0, stream, dy, x, gamma,
                       mean, rstd, dx, N, D);
}

template <typename T>
void launch_layernorm_wgrad(const T* dy, const T* x, const float* mean,
                            const float* rstd, float* dgamma, float* dbeta,
                            long N, int D, hipStream_t stream) {
  const int block = 256;
  const int colb = (D + block - 1) / block;
  const int rows_per_block = 64;
  const int rowb = (int)((N + rows_per_block - 1) / rows_per_block);
  if (colb && rowb)
    hipLaunchKernelGGL(layernorm_wgrad_kernel<T>, dim3(colb, rowb), dim3(block),
                       0, stream, dy, x, mean, rstd, dgamma, dbeta, N, D,
                       rows_per_block);
}

template <typename T>
void launch_bias_gelu_fwd(const T* x, const float* bias, T* y, long total,
                          int D, hipStream_t stream) {
  const int block = 256;
  const long nvec = total / (16 / sizeof(T));
  const int grid = (int)min((nvec + block - 1) / block, (long)4096);
  if (grid)
    hipLaunchKernelGGL(bias_gelu_fwd_kernel<T>, dim3(grid), dim3(block),
                       D * sizeof(float), stream, x, bias, y, total, D);
}

template <typename T>
void launch_bias_gelu_bwd(const T* dy, const T* x, const float* bias, T* dx,
                          long total, int D, hipStream_t stream) {
  const int block = 256;
  const long nvec = total / (16 / sizeof(T));
  const int grid = (int)min((nvec + block - 1) / block, (long)4096);
  if (grid)
    hipLaunchKernelGGL(bias_gelu_bwd_kernel<T>, dim3(grid), dim3(block),
                       D * sizeof(float), stream, dy, x, bias, dx, total, D);
}

template <typename T>
void launch_softmax_mask_fwd(const T* S, const int* valid, T* P, T* Pd, long R,
                             int L, int rows_per_batch, float scale,
                             float dropout_p, unsigned long long seed,
                             int causal, int Lq, hipStream_t stream) {
  const int grid = (int)((R + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK);
  if (grid)
    hipLaunchKernelGGL(softmax_mask_fwd_kernel<T>, dim3(grid),
                       dim3(WAVE * ROWS_PER_BLOCK), 0, stream, S, valid, P, Pd,
                       R, L, rows_per_batch, scale, dropout_p, seed, causal, Lq);
}

template <typename T>
void launch_softmax_mask_bwd(const T* dPd, const T* P, T* dS, long R, int L,
                             float scale, float dropout_p,
                             unsigned long long seed, hipStream_t stream) {
  const int grid = (int)((R + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK);
  if (grid)
    hipLaunchKernelGGL(softmax_mask_bwd_kernel<T>, dim3(grid),
                       dim3(WAVE * ROWS_PER_BLOCK), 0, stream, dPd, P, dS, R, L,
                       scale, dropout_p, seed);
}

template <typename T>
void launch_rmsnorm_fwd(const T* x, const float* gamma, T* y, float* rstd,
                        long N, int D, float eps, hipStream_t stream) {
  const int grid = (int)((N + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK);
  if (grid)
    hipLaunchKernelGGL(rmsnorm_fwd_kernel<T>, dim3(grid),
                       dim3(WAVE * ROWS_PER_BLOCK), 0, stream, x, gamma, y,
                       rstd, N, D, eps);
}

template <typename T>
void launch_rmsnorm_bwd(const T* dy, const T* x, const float* gamma,
                        const float* rstd, T* dx, long N, int D,
                        hipStream_t stream) {
  const int grid = (int)((N + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK);
  if (grid)
    hipLaunchKernelGGL(rmsnorm_bwd_kernel<T>, dim3(grid),
                       dim3(WAVE * ROWS_PER_BLOCK), 0, stream, dy, x, gamma,
                       rstd, dx, N, D);
}

template <typename T>
void launch_rmsnorm_wgrad(const T* dy, const T* x, const float* rstd,
                          float* dgamma, long N, int D, hipStream_t stream) {
  const int block = 256;
  const int colb = (D + block - 1) / block;
  const int rows_per_block = 64;
  const int rowb = (int)((N + rows_per_block - 1) / rows_per_block);
  if (colb && rowb)
    hipLaunchKernelGGL(rmsnorm_wgrad_kernel<T>, dim3(colb, rowb), dim3(block),
                       0, stream, dy, x, rstd, dgamma, N, D, rows_per_block);
}

#define INSTANTIATE_TK(T)                                                    \
  template void launch_layernorm_fwd<T>(const T*, const float*, const float*, \
                                        T*, float*, float*, long, int, float, \
                                        hipStream_t);                         \
  template void launch_layernorm_bwd<T>(const T*, const T*, const float*,     \
                                        const float*, const float*, T*, long, \
                                        int, hipStream_t);                    \
  template void launch_layernorm_wgrad<T>(const T*, const T*, const float*,   \
                                          const float*, float*, float*, long, \
                                          int, hipStream_t);                  \
  template void launch_bias_gelu_fwd<T>(const T*, const float*, T*, long,     \
                                        int, hipStream_t);                    \
  template void launch_bias_gelu_bwd<T>(const T*, const T*, const float*, T*, \
                                        long, int, hipStream_t);              \
  template void launch_softmax_mask_fwd<T>(const T*, const int*, T*, T*,     \
                                           long, int, int, float, float,      \
                                           unsigned long long, int, int,      \
                                           hipStream_t);                      \
  template void launch_rmsnorm_fwd<T>(const T*, const float*, T*, float*,     \
                                      long, int, float, hipStream_t);         \
  template void launch_rmsnorm_bwd<T>(const T*, const T*, const float*,       \
                                      const float*, T*, long, int,            \
                                      hipStream_t);                           \
  template void launch_rmsnorm_wgrad<T>(const T*, const T*, const float*,     \
                                        float*, long, int, hipStream_t);      \
  template void launch_softmax_mask_bwd<T>(const T*, const T*, T*, long, int, \
                                           float, float, unsigned long long,  \
                                           hipStream_t);

INSTANTIATE_TK(float)
INSTANTIATE_TK(__hip_bfloat16)

// ---------------------------------------------------------------------------
// Embedding backward: dW[idx[n]] += dY[n] (fp32 accum), padding_idx skipped.
// Replaces torch's sort + segment-reduce + scatter stack (~0.5 ms/step on
// the LineVul step for 3 embeddings).
// ---------------------------------------------------------------------------

template <typename T>
__global__ void embed_scatter_kernel(const T* __restrict__ dY,
                                     const long* __restrict__ idx,
                                     float* __restrict__ dW, long N, int D,
                                     long padding_idx) {
  const long row = (long)(blockIdx.x * (blockDim.x / WAVE)) + threadIdx.x / WAVE;
  const int lane = threadIdx.x & (WAVE - 1);
  if (row >= N) return;
  const long i = idx[row];
  if (i == padding_idx) return;
  const T* src = dY + row * D;
  float* dst = dW + i * D;
  if (D % (WAVE * 4) == 0) {
    for (int d = lane * 4; d < D; d += WAVE * 4) {
      const f4 a = load4(src + d);
#pragma unroll
      for (int u = 0; u < 4; ++u) atomicAdd(dst + d + u, a.v[u]);
    }
  } else {
    for (int d = lane; d < D; d += WAVE) atomicAdd(dst + d, tf(src[d]));
  }
}

template <typename T>
void launch_embed_scatter(const T* dY, const long* idx, float* dW, long N,
                          int D, long padding_idx, hipStream_t stream) {
  const int grid = (int)((N + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK);
  if (grid)
    hipLaunchKernelGGL(embed_scatter_kernel<T>, dim3(grid),
                       dim3(WAVE * ROWS_PER_BLOCK), 0, stream, dY, idx, dW, N,
                       D, padding_idx);
}

template void launch_embed_scatter<float>(const float*, const long*, float*,
                                          long, int, long, hipStream_t);
template void launch_embed_scatter<__hip_bfloat16>(const __hip_bfloat16*,
                                                   const long*, float*, long,
                                                   int, long, hipStream_t);

// ---------------------------------------------------------------------------
// Fused y = LayerNorm(dropout(h) + residual): the transformer residual
// pattern (RobertaSelfOutput/RobertaOutput) as ONE kernel per direction.
// Stateless dropout (hash4 mask, regenerated in backward) — nothing but
// (h, res) and the seed is stored; z = dropout(h)+res is recomputed.
// Requires D % 256 == 0 (vector path only; the op wrapper falls back).
// ---------------------------------------------------------------------------

template <typename T>
__global__ void ln_res_dropout_fwd_kernel(
    const T* __restrict__ h, const T* __restrict__ res,
    const float* __restrict__ gamma, const float* __restrict__ beta,
    T* __restrict__ y, float* __restrict__ mean, float* __restrict__ rstd,
    long N, int D, float eps, unsigned p8, unsigned long long seed,
    float dscale) {
  const long row = (long)(blockIdx.x * (blockDim.x / WAVE)) + threadIdx.x / WAVE;
  const int lane = threadIdx.x & (WAVE - 1);
  if (row >= N) return;
  const T* hr = h + row * D;
  const T* rr = res + row * D;
  // shifted mean + centred variance pass: see layernorm_fwd_kernel
  const bool keep0 = (p8 == 0) || keep_mask(row * D, seed, p8);
  const float z0 = (keep0 ? tf(hr[0]) * dscale : 0.f) + tf(rr[0]);
  T* yr = y + row * D;
  if (D <= LN_CACHE_IT * WAVE * 4) {
    // z = dropout(h) + res is formed once (one hash, one read of h and res)
    // and stays in registers across the three passes
    f4 c[LN_CACHE_IT];
    float s = 0.f;
#pragma unroll
    for (int it = 0; it < LN_CACHE_IT; ++it) {
      const int d = (it * WAVE + lane) * 4;
      if (d < D) {
        const f4 a = load4(hr + d);
        const f4 b = load4(rr + d);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const bool keep = (p8 == 0) || keep_mask(row * D + d + u, seed, p8);
          c[it].v[u] = (keep ? a.v[u] * dscale : 0.f) + b.v[u];
          s += c[it].v[u] - z0;
        }
      }
    }
    const float mu = z0 + wave_sum(s) / D;
    float s2 = 0.f;
#pragma unroll
    for (int it = 0; it < LN_CACHE_IT; ++it) {
      if ((it * WAVE + lane) * 4 < D) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          c[it].v[u] -= mu;
          s2 += c[it].v[u] * c[it].v[u];
        }
      }
    }
    const float rs = rsqrtf(wave_sum(s2) / D + eps);
    if (lane == 0) {
      mean[row] = mu;
      rstd[row] = rs;
    }
#pragma unroll
    for (int it = 0; it < LN_CACHE_IT; ++it) {
      const int d = (it * WAVE + lane) * 4;
      if (d < D) {
        const f4 g = load4(gamma + d);
        const f4 bb = load4(beta + d);
        f4 o;
#pragma unroll
        for (int u = 0; u < 4; ++u) o.v[u] = c[it].v[u] * rs * g.v[u] + bb.v[u];
        store4(yr + d, o);
      }
    }
    return;
  }
  float s = 0.f;
  for (int d = lane * 4; d < D; d += WAVE * 4) {
    const f4 a = load4(hr + d);
    const f4 b = load4(rr + d);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const bool keep = (p8 == 0) || keep_mask(row * D + d + u, seed, p8);
      const float z = (keep ? a.v[u] * dscale : 0.f) + b.v[u];
      s += z - z0;
    }
  }
  const float mu = z0 + wave_sum(s) / D;
  float s2 = 0.f;
  for (int d = lane * 4; d < D; d += WAVE * 4) {
    const f4 a = load4(hr + d);
    const f4 b = load4(rr + d);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const bool keep = (p8 == 0) || keep_mask(row * D + d + u, seed, p8);
      const float c = (keep ? a.v[u] * dscale : 0.f) + b.v[u] - mu;
      s2 += c * c;
    }
  }
  const float rs = rsqrtf(wave_sum(s2) / D + eps);
  if (lane == 0) {
    mean[row] = mu;
    rstd[row] = rs;
  }
  for (int d = lane * 4; d < D; d += WAVE * 4) {
    const f4 a = load4(hr + d);
    const f4 b = load4(rr + d);
    const f4 g = load4(gamma + d);
    const f4 bb = load4(beta + d);
    f4 o;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const bool keep = (p8 == 0) || keep_mask(row * D + d + u, seed, p8);
      const float z = (keep ? a.v[u] * dscale : 0.f) + b.v[u];
      o.v[u] = (z - mu) * rs * g.v[u] + bb.v[u];
    }
    store4(yr + d, o);
  }
}

template <typename T>
__global__ void ln_res_dropout_bwd_kernel(
    const T* __restrict__ dy, const T* __restrict__ h,
    const T* __restrict__ res, const float* __restrict__ gamma,
    const float* __restrict__ mean, const float* __restrict__ rstd,
    T* __restrict__ dz, T* __restrict__ dh, T* __restrict__ zout, long N,
    int D, unsigned p8, unsigned long long seed, float dscale) {
  // zout: reconstructed z = dropout(h)+res, written once here so the
  // column-reduction wgrad can run the plain (hash-free) LN wgrad kernel
  const long row = (long)(blockIdx.x * (blockDim.x / WAVE)) + threadIdx.x / WAVE;
  const int lane = threadIdx.x & (WAVE - 1);
  if (row >= N) return;
  const T* dyr = dy + row * D;
  const T* hr = h + row * D;
  const T* rr = res + row * D;
  const float mu = mean[row], rs = rstd[row];
  float c1 = 0.f, c2 = 0.f;
  for (int d = lane * 4; d < D; d += WAVE * 4) {
    const f4 a = load4(hr + d);
    const f4 b = load4(rr + d);
    const f4 dyv = load4(dyr + d);
    const f4 g4 = load4(gamma + d);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const bool keep = (p8 == 0) || keep_mask(row * D + d + u, seed, p8);
      const float z = (keep ? a.v[u] * dscale : 0.f) + b.v[u];
      const float g = dyv.v[u] * g4.v[u];
      c1 += g;
      c2 += g * (z - mu) * rs;
    }
  }
  c1 = wave_sum(c1) / D;
  c2 = wave_sum(c2) / D;
  T* dzr = dz + row * D;
  T* dhr = dh + row * D;
  T* zr = zout + row * D;
  for (int d = lane * 4; d < D; d += WAVE * 4) {
    const f4 a = load4(hr + d);
    const f4 b = load4(rr + d);
    const f4 dyv = load4(dyr + d);
    const f4 g4 = load4(gamma + d);
    f4 oz, oh, ozv;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const bool keep = (p8 == 0) || keep_mask(row * D + d + u, seed, p8);
      const float z = (keep ? a.v[u] * dscale : 0.f) + b.v[u];
      const float xh = (z - mu) * rs;
      const float dzv = rs * (dyv.v[u] * g4.v[u] - c1 - xh * c2);
      oz.v[u] = dzv;
      oh.v[u] = keep ? dzv * dscale : 0.f;
      ozv.v[u] = z;
    }
    store4(dzr + d, oz);
    store4(dhr + d, oh);
    store4(zr + d, ozv);
  }
}

template <typename T>
__global__ void ln_res_dropout_wgrad_kernel(
    const T* __restrict__ dy, const T* __restrict__ h,
    const T* __restrict__ res, const float* __restrict__ mean,
    const float* __restrict__ rstd, float* __restrict__ dgamma,
    float* __restrict__ dbeta, long N, int D, int rows_per_block, unsigned p8,
    unsigned long long seed, float dscale) {
  const int d = blockIdx.x * blockDim.x + threadIdx.x;
  if (d >= D) return;
  const long r0 = (long)blockIdx.y * rows_per_block;
  const long r1 = min((long)(r0 + rows_per_block), N);
  float dg[4] = {}, db[4] = {};
  long r = r0;
  for (; r + 4 <= r1; r += 4) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const long rr_ = r + u;
      const float g = tf(dy[rr_ * D + d]);
      const bool keep = (p8 == 0) || keep_mask(rr_ * D + d, seed, p8);
      const float z = (keep ? tf(h[rr_ * D + d]) * dscale : 0.f) + tf(res[rr_ * D + d]);
      dg[u] += g * (z - mean[rr_]) * rstd[rr_];
      db[u] += g;
    }
  }
  for (; r < r1; ++r) {
    const float g = tf(dy[r * D + d]);
    const bool keep = (p8 == 0) || keep_mask(r * D + d, seed, p8);
    const float z = (keep ? tf(h[r * D + d]) * dscale : 0.f) + tf(res[r * D + d]);
    dg[0] += g * (z - mean[r]) * rstd[r];
    db[0] += g;
  }
  atomicAdd(dgamma + d, dg[0] + dg[1] + dg[2] + dg[3]);
  atomicAdd(dbeta + d, db[0] + db[1] + db[2] + db[3]);
}

template <typename T>
void launch_ln_res_dropout_fwd(const T* h, const T* res, const float* gamma,
                               const float* beta, T* y, float* mean,
                               float* rstd, long N, int D, float eps,
                               float dropout_p, unsigned long long seed,
                               hipStream_t stream) {
  const unsigned p8 = (unsigned)(dropout_p * 256.0f);
  const float dscale = (p8 > 0) ? 256.0f / (256.0f - p8) : 1.0f;
  const int grid = (int)((N + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK);
  if (grid)
    hipLaunchKernelGGL(ln_res_dropout_fwd_kernel<T>, dim3(grid),
                       dim3(WAVE * ROWS_PER_BLOCK), 0, stream, h, res, gamma,
                       beta, y, mean, rstd, N, D, eps, p8, seed, dscale);
}

template <typename T>
void launch_ln_res_dropout_bwd(const T* dy, const T* h, const T* res,
                               const float* gamma, const float* mean,
                               const float* rstd, T* dz, T* dh, T* zout,
                               long N, int D, float dropout_p,
                               unsigned long long seed, hipStream_t stream) {
  const unsigned p8 = (unsigned)(dropout_p * 256.0f);
  const float dscale = (p8 > 0) ? 256.0f / (256.0f - p8) : 1.0f;
  const int grid = (int)((N + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK);
  if (grid)
    hipLaunchKernelGGL(ln_res_dropout_bwd_kernel<T>, dim3(grid),
                       dim3(WAVE * ROWS_PER_BLOCK), 0, stream, dy, h, res,
                       gamma, mean, rstd, dz, dh, zout, N, D, p8, seed,
                       dscale);
}

template <typename T>
void launch_ln_res_dropout_wgrad(const T* dy, const T* h, const T* res,
                                 const float* mean, const float* rstd,
                                 float* dgamma, float* dbeta, long N, int D,
                                 float dropout_p, unsigned long long seed,
                                 hipStream_t stream) {
  const unsigned p8 = (unsigned)(dropout_p * 256.0f);
  const float dscale = (p8 > 0) ? 256.0f / (256.0f - p8) : 1.0f;
  const int block = 256;
  const int colb = (D + block - 1) / block;
  const int rows_per_block = 64;
  const int rowb = (int)((N + rows_per_block - 1) / rows_per_block);
  if (colb && rowb)
    hipLaunchKernelGGL(ln_res_dropout_wgrad_kernel<T>, dim3(colb, rowb),
                       dim3(block), 0, stream, dy, h, res, mean, rstd, dgamma,
                       dbeta, N, D, rows_per_block, p8, seed, dscale);
}

#define INST_LNRD(T)                                                          \
  template void launch_ln_res_dropout_fwd<T>(const T*, const T*, const float*,\
                                             const float*, T*, float*, float*,\
                                             long, int, float, float,         \
                                             unsigned long long, hipStream_t);\
  template void launch_ln_res_dropout_bwd<T>(const T*, const T*, const T*,    \
                                             const float*, const float*,      \
                                             const float*, T*, T*, T*, long,  \
                                             int, float, unsigned long long,  \
                                             hipStream_t);                    \
  template void launch_ln_res_dropout_wgrad<T>(                               \
      const T*, const T*, const T*, const float*, const float*, float*,       \
      float*, long, int, float, unsigned long long, hipStream_t);
INST_LNRD(float)
INST_LNRD(__hip_bfloat16)
#undef INST_LNRD

// ---------------------------------------------------------------------------
// Fused out = res + dropout(h): the pre-norm residual pattern (T5 layers).
// Stateless dropout; backward needs only one kernel (dh = mask * dy, and
// d(res) = dy is a pass-through the op returns directly).
// ---------------------------------------------------------------------------

template <typename T>
__global__ void dropout_add_fwd_kernel(const T* __restrict__ h,
                                       const T* __restrict__ res,
                                       T* __restrict__ out, long total,
                                       unsigned p8, unsigned long long seed,
                                       float dscale) {
  constexpr int VEC = 16 / sizeof(T);
  const long nvec = total / VEC;
  const long stride = (long)gridDim.x * blockDim.x;
  for (long iv = (long)blockIdx.x * blockDim.x + threadIdx.x; iv < nvec;
       iv += stride) {
    T vh[VEC], vr[VEC], vo[VEC];
    *reinterpret_cast<ulonglong2*>(vh) =
        *reinterpret_cast<const ulonglong2*>(h + iv * VEC);
    *reinterpret_cast<ulonglong2*>(vr) =
        *reinterpret_cast<const ulonglong2*>(res + iv * VEC);
#pragma unroll
    for (int u = 0; u < VEC; ++u) {
      const bool keep = (p8 == 0) || keep_mask(iv * VEC + u, seed, p8);
      vo[u] = ff<T>(tf(vr[u]) + (keep ? tf(vh[u]) * dscale : 0.f));
    }
    *reinterpret_cast<ulonglong2*>(out + iv * VEC) =
        *reinterpret_cast<const ulonglong2*>(vo);
  }
}

template <typename T>
__global__ void dropout_add_bwd_kernel(const T* __restrict__ dy,
                                       T* __restrict__ dh, long total,
                                       unsigned p8, unsigned long long seed,
                                       float dscale) {
  constexpr int VEC = 16 / sizeof(T);
  const long nvec = total / VEC;
  const long stride = (long)gridDim.x * blockDim.x;
  for (long iv = (long)blockIdx.x * blockDim.x + threadIdx.x; iv < nvec;
       iv += stride) {
    T v[VEC], o[VEC];
    *reinterpret_cast<ulonglong2*>(v) =
        *reinterpret_cast<const ulonglong2*>(dy + iv * VEC);
#pragma unroll
    for (int u = 0; u < VEC; ++u) {
      const bool keep = (p8 == 0) || keep_mask(iv * VEC + u, seed, p8);
      o[u] = ff<T>(keep ? tf(v[u]) * dscale : 0.f);
    }
    *reinterpret_cast<ulonglong2*>(dh + iv * VEC) =
        *reinterpret_cast<const ulonglong2*>(o);
  }
}

template <typename T>
void launch_dropout_add_fwd(const T* h, const T* res, T* out, long total,
                            float p, unsigned long long seed,
                            hipStream_t stream) {
  const unsigned p8 = (unsigned)(p * 256.0f);
  const float dscale = (p8 > 0) ? 256.0f / (256.0f - p8) : 1.0f;
  const int block = 256;
  const long nvec = total / (16 / sizeof(T));
  const int grid = (int)min((nvec + block - 1) / block, (long)4096);
  if (grid)
    hipLaunchKernelGGL(dropout_add_fwd_kernel<T>, dim3(grid), dim3(block), 0,
                       stream, h, res, out, total, p8, seed, dscale);
}

template <typename T>
void launch_dropout_add_bwd(const T* dy, T* dh, long total, float p,
                            unsigned long long seed, hipStream_t stream) {
  const unsigned p8 = (unsigned)(p * 256.0f);
  const float dscale = (p8 > 0) ? 256.0f / (256.0f - p8) : 1.0f;
  const int block = 256;
  const long nvec = total / (16 / sizeof(T));
  const int grid = (int)min((nvec + block - 1) / block, (long)4096);
  if (grid)
    hipLaunchKernelGGL(dropout_add_bwd_kernel<T>, dim3(grid), dim3(block), 0,
                       stream, dy, dh, total, p8, seed, dscale);
}

#define INST_DA(T)                                                            \
  template void launch_dropout_add_fwd<T>(const T*, const T*, T*, long, float,\
                                          unsigned long long, hipStream_t);   \
  template void launch_dropout_add_bwd<T>(const T*, T*, long, float,          \
                                          unsigned long long, hipStream_t);
INST_DA(float)
INST_DA(__hip_bfloat16)
#undef INST_DA

// Fused ReLU + dropout (T5 FFN: wo(dropout(relu(wi x))) — torch ran relu,
// a bernoulli mask, a mul and a masked_scale backward as 4 separate
// passes over the (N, 3072) activation). Stateless: the keep mask is
// regenerated from the seed in backward; only the pre-ReLU input is saved.
template <typename T>
__global__ void relu_dropout_fwd_kernel(const T* __restrict__ x,
                                        T* __restrict__ out, long total,
                                        unsigned p8, unsigned long long seed,
                                        float dscale) {
  constexpr int VEC = 16 / sizeof(T);
  const long nvec = total / VEC;
  const long stride = (long)gridDim.x * blockDim.x;
  for (long iv = (long)blockIdx.x * blockDim.x + threadIdx.x; iv < nvec;
       iv += stride) {
    T vx[VEC], vo[VEC];
    *reinterpret_cast<ulonglong2*>(vx) =
        *reinterpret_cast<const ulonglong2*>(x + iv * VEC);
#pragma unroll
    for (int u = 0; u < VEC; ++u) {
      const bool keep = (p8 == 0) || keep_mask(iv * VEC + u, seed, p8);
      const float r = fmaxf(tf(vx[u]), 0.f);
      vo[u] = ff<T>(keep ? r * dscale : 0.f);
    }
    *reinterpret_cast<ulonglong2*>(out + iv * VEC) =
        *reinterpret_cast<const ulonglong2*>(vo);
  }
}

template <typename T>
__global__ void relu_dropout_bwd_kernel(const T* __restrict__ dy,
                                        const T* __restrict__ x,
                                        T* __restrict__ dx, long total,
                                        unsigned p8, unsigned long long seed,
                                        float dscale) {
  constexpr int VEC = 16 / sizeof(T);
  const long nvec = total / VEC;
  const long stride = (long)gridDim.x * blockDim.x;
  for (long iv = (long)blockIdx.x * blockDim.x + threadIdx.x; iv < nvec;
       iv += stride) {
    T vd[VEC], vx[VEC], vo[VEC];
    *reinterpret_cast<ulonglong2*>(vd) =
        *reinterpret_cast<const ulonglong2*>(dy + iv * VEC);
    *reinterpret_cast<ulonglong2*>(vx) =
        *reinterpret_cast<const ulonglong2*>(x + iv * VEC);
#pragma unroll
    for (int u = 0; u < VEC; ++u) {
      const bool keep = (p8 == 0) || keep_mask(iv * VEC + u, seed, p8);
      const bool pos = tf(vx[u]) > 0.f;
      vo[u] = ff<T>((keep && pos) ? tf(vd[u]) * dscale : 0.f);
    }
    *reinterpret_cast<ulonglong2*>(dx + iv * VEC) =
        *reinterpret_cast<const ulonglong2*>(vo);
  }
}

template <typename T>
void launch_relu_dropout_fwd(const T* x, T* out, long total, float dropout_p,
                             unsigned long long seed, hipStream_t stream) {
  constexpr int VEC = 16 / sizeof(T);
  const unsigned p8 = (unsigned)(dropout_p * 256.0f);
  const float dscale = (p8 > 0) ? 256.0f / (256.0f - p8) : 1.0f;
  const int block = 256;
  const int grid = (int)min((total / VEC + block - 1) / block, (long)4096);
  if (grid)
    hipLaunchKernelGGL(relu_dropout_fwd_kernel<T>, dim3(grid), dim3(block), 0,
                       stream, x, out, total, p8, seed, dscale);
}

template <typename T>
void launch_relu_dropout_bwd(const T* dy, const T* x, T* dx, long total,
                             float dropout_p, unsigned long long seed,
                             hipStream_t stream) {
  constexpr int VEC = 16 / sizeof(T);
  const unsigned p8 = (unsigned)(dropout_p * 256.0f);
  const float dscale = (p8 > 0) ? 256.0f / (256.0f - p8) : 1.0f;
  const int block = 256;
  const int grid = (int)min((total / VEC + block - 1) / block, (long)4096);
  if (grid)
    hipLaunchKernelGGL(relu_dropout_bwd_kernel<T>, dim3(grid), dim3(block), 0,
                       stream, dy, x, dx, total, p8, seed, dscale);
}

template void launch_relu_dropout_fwd<__hip_bfloat16>(
    const __hip_bfloat16*, __hip_bfloat16*, long, float, unsigned long long,
    hipStream_t);
template void launch_relu_dropout_bwd<__hip_bfloat16>(
    const __hip_bfloat16*, const __hip_bfloat16*, __hip_bfloat16*, long, float,
    unsigned long long, hipStream_t);
template void launch_relu_dropout_fwd<float>(
    const float*, float*, long, float, unsigned long long, hipStream_t);
template void launch_relu_dropout_bwd<float>(
    const float*, const float*, float*, long, float, unsigned long long,
    hipStream_t);

// T5 relative-position-bias weight grad: dW[bucket, h] = sum over (q,k)
// with buckets[q,k]==bucket of dBias[h, q, k]. The onehot-matmul form hit
// hipBLASLt's tall-skinny pathology (MT16x32, 381 us for a 100-MFLOP
// reduction); this is a bucket scatter-reduce with per-wave LDS partials.
__global__ void relbias_wgrad_kernel(const float* __restrict__ dbias,
                                     const int* __restrict__ buckets,
                                     float* __restrict__ dw, long QK, int H,
                                     int NB) {
  extern __shared__ float part[];  // [waves][NB * H]
  const int lane = threadIdx.x & (WAVE - 1);
  const int wv = threadIdx.x / WAVE;
  const int nwv = blockDim.x / WAVE;
  float* mine = part + wv * NB * H;
  for (int i = threadIdx.x; i < nwv * NB * H; i += blockDim.x) part[i] = 0.f;
  __syncthreads();
  // lane covers h = lane % 16 (masked), qk strided by 4 per wave
  const int h = lane & 15;
  const int qsub = lane >> 4;
  if (h < H) {
    for (long qk = (long)blockIdx.x * (nwv * 4) + wv * 4 + qsub; qk < QK;
         qk += (long)gridDim.x * nwv * 4) {
      const int b = buckets[qk];
      // a bucket outside [0, NB) would write past this wave's partials
      if ((unsigned)b < (unsigned)NB) atomicAdd(mine + b * H + h, dbias[(long)h * QK + qk]);
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < NB * H; i += blockDim.x) {
    float s = 0.f;
    for (int w = 0; w < nwv; ++w) s += part[w * NB * H + i];
    if (s != 0.f) atomicAdd(dw + i, s);
  }
}

void launch_relbias_wgrad(const float* dbias, const int* buckets, float* dw,
                          long QK, int H, int NB, hipStream_t stream) {
  const int block = 256;
  const int grid = 256;
  const size_t lds = (size_t)(block / WAVE) * NB * H * sizeof(float);
  hipLaunchKernelGGL(relbias_wgrad_kernel, dim3(grid), dim3(block), lds,
                     stream, dbias, buckets, dw, QK, H, NB);
}
