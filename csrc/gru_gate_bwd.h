// Backward of one GRU gate element in the "gicat" layout, shared by
// gru_gates2_bwd_kernel (flowgnn_kernels.hip) and the gate prologue of
// gates_gemm_kernel (gemm_bias.hip) so that both compile one expression.
//
// go = grad of h', hv = h entering the step, r/z/n/hn the saved activations.
// grad_gicat columns: [dpr | dpz | dpn | dpn*r]; ghd = go * z is the direct
// z-path grad of h.

#pragma once

#include <hip/hip_runtime.h>

struct GruGate2Grad {
  float dpr, dpz, dpn, dpnr, ghd;
};

__device__ __forceinline__ GruGate2Grad gru_gate2_bwd_elem(float go, float hv,
                                                           float r, float z,
                                                           float n, float hn) {
  const float dn = go * (1.f - z);
  const float dz = go * (hv - n);
  const float dpn = dn * (1.f - n * n);
  const float dr = dpn * hn;
  const float dpr = dr * r * (1.f - r);
  const float dpz = dz * z * (1.f - z);
  return {dpr, dpz, dpn, dpn * r, go * z};
}
