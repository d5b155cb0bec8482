// Python bindings for the MI355X flow-GNN kernels (deepdfa_amd._C).

#include <torch/extension.h>

#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <c10/hip/HIPStream.h>
#include <c10/util/accumulate.h>

#include <climits>

// the launchers are defined (at global scope) in flowgnn_kernels.hip
template <typename T>
void launch_embed4_fwd(const T*, const long*, T*, int, int, hipStream_t);
template <typename T, typename TO>
void launch_embed4_fwd2(const T*, const long*, TO*, int, int, hipStream_t);
template <typename T>
void launch_embed4_bwd(const T*, const long*, float*, long, int, hipStream_t);
template <typename T>
void launch_spmm_sum(const int*, const int*, const T*, T*, int, int, hipStream_t);
template <typename T>
void launch_gru_gates_fwd(const T*, const T*, const T*, T*, T*, T*, T*, long, int, hipStream_t);
template <typename T>
void launch_gru_gates_bwd(const T*, const T*, const T*, const T*, const T*, const T*, T*, T*, T*,
                          long, int, hipStream_t);
template <typename T>
void launch_attn_pool_fwd(const T*, const T*, const int*, T*, float*, int, int, hipStream_t);
template <typename T>
void launch_attn_pool_bwd(const T*, const T*, const float*, const int*, T*, T*, float*, int, int,
                          hipStream_t);
void launch_segment_max(const float*, const int*, float*, int, hipStream_t);
template <typename T>
void launch_gru_gates2_fwd(const T*, const T*, T*, T*, T*, T*, T*, long, int, hipStream_t);
template <typename T>
void launch_gru_gates2_bwd(const T*, const T*, const T*, const T*, const T*, const T*, T*, T*,
                           long, int, hipStream_t);
template <typename T>
void launch_colsum(const T*, float*, int, int, hipStream_t);
template <typename T>
void launch_spmm_sum_strided(const int*, const int*, const T*, T*, int, int, long,
                             hipStream_t);
void launch_gemm_bias2(const __hip_bfloat16*, const __hip_bfloat16*, const __hip_bfloat16*,
                       const __hip_bfloat16*, const __hip_bfloat16*, long,
                       const __hip_bfloat16*, long, __hip_bfloat16*, int, int, int, int,
                       hipStream_t, const int* = nullptr, const int* = nullptr, long = 0,
                       __hip_bfloat16* = nullptr);
bool launch_gates_gemm(const __hip_bfloat16*, const __hip_bfloat16*, const __hip_bfloat16*,
                       const __hip_bfloat16*, const __hip_bfloat16*, const __hip_bfloat16*,
                       const __hip_bfloat16*, __hip_bfloat16*, __hip_bfloat16*,
                       __hip_bfloat16*, int, int, hipStream_t);
void launch_gemm_bias(const __hip_bfloat16*, const __hip_bfloat16*, const __hip_bfloat16*,
                      const __hip_bfloat16*, const __hip_bfloat16*, __hip_bfloat16*, int, int,
                      int, int, hipStream_t);
void launch_wgrad(const __hip_bfloat16*, const __hip_bfloat16*, const __hip_bfloat16*, float*,
                  float*, int, int, int, int, hipStream_t, float* = nullptr,
                  float* = nullptr, float* = nullptr, float* = nullptr);
template <typename T>
void launch_layernorm_fwd(const T*, const float*, const float*, T*, float*, float*, long, int,
                          float, hipStream_t);
template <typename T>
void launch_layernorm_bwd(const T*, const T*, const float*, const float*, const float*, T*, long,
                          int, hipStream_t);
template <typename T>
void launch_layernorm_wgrad(const T*, const T*, const float*, const float*, float*, float*, long,
                            int, hipStream_t);
template <typename T>
void launch_bias_gelu_fwd(const T*, const float*, T*, long, int, hipStream_t);
template <typename T>
void launch_bias_gelu_bwd(const T*, const T*, const float*, T*, long, int, hipStream_t);
template <typename T>
void launch_softmax_mask_fwd(const T*, const int*, T*, T*, long, int, int, float, float,
                             unsigned long long, int, int, hipStream_t);
template <typename T>
void launch_rmsnorm_fwd(const T*, const float*, T*, float*, long, int, float, hipStream_t);
template <typename T>
void launch_rmsnorm_bwd(const T*, const T*, const float*, const float*, T*, long, int,
                        hipStream_t);
template <typename T>
void launch_rmsnorm_wgrad(const T*, const T*, const float*, float*, long, int, hipStream_t);
void launch_flash_fwd(const __hip_bfloat16*, const __hip_bfloat16*, const __hip_bfloat16*,
                      const int*, const float*, __hip_bfloat16*, float*, int, int, int, float,
                      int, unsigned, unsigned long long, long, long, hipStream_t);
void launch_flash_dterm(const __hip_bfloat16*, const __hip_bfloat16*, float*, int, int, int,
                        hipStream_t);
void launch_flash_dq(const __hip_bfloat16*, const __hip_bfloat16*, const __hip_bfloat16*,
                     const __hip_bfloat16*, const int*, const float*, const float*, const float*,
                     __hip_bfloat16*, float*, int, int, int, float, int, unsigned,
                     unsigned long long, long, long, long, hipStream_t);
// all six GGNN parameter grads at H = 128 in one launch (csrc/ggnn_wgrad.hip)
void launch_ggnn_wgrad(const __hip_bfloat16*, const __hip_bfloat16*, const __hip_bfloat16*,
                       const __hip_bfloat16*, float*, float*, float*, float*, float*, float*,
                       int, int, int, int, hipStream_t);
int ggnn_wgrad_kchunk(int, int);
void launch_wgrad2(const __hip_bfloat16*, const __hip_bfloat16*, float*, float*,
                   int, int, int, int, hipStream_t);
void launch_adamw_fused(float*, const float*, float*, float*, long, float, float, float, float,
                        float, const float*, const float*, int, void*, hipStream_t);
void launch_gemm2(const __hip_bfloat16*, const __hip_bfloat16*, const float*,
                  const __hip_bfloat16*, __hip_bfloat16*, int, int, int, hipStream_t);
void launch_flash_dkv(const __hip_bfloat16*, const __hip_bfloat16*, const __hip_bfloat16*,
                      const __hip_bfloat16*, const int*, const float*, const float*, const float*,
                      __hip_bfloat16*, __hip_bfloat16*, int, int, int, float, int, unsigned,
                      unsigned long long, long, long, long, hipStream_t);
template <typename T>
void launch_softmax_mask_bwd(const T*, const T*, T*, long, int, float, float,
                             unsigned long long, hipStream_t);
void launch_flash_received(const __hip_bfloat16*, const __hip_bfloat16*, const int*, const float*,
                           const float*, float*, int, int, int, float, int, long, long,
                           hipStream_t);
// general (Lq, Lk) flash attention (csrc/flash_rect.hip)
void launch_flash_rect_fwd(const __hip_bfloat16*, const __hip_bfloat16*, const __hip_bfloat16*,
                           const int*, const float*, __hip_bfloat16*, float*, int, int, int, int,
                           float, int, unsigned, unsigned long long, long, long, hipStream_t);
void launch_flash_rect_dq(const __hip_bfloat16*, const __hip_bfloat16*, const __hip_bfloat16*,
                          const __hip_bfloat16*, const int*, const float*, const float*,
                          const float*, __hip_bfloat16*, float*, int, int, int, int, float, int,
                          unsigned, unsigned long long, long, long, hipStream_t);
void launch_flash_rect_dkv(const __hip_bfloat16*, const __hip_bfloat16*, const __hip_bfloat16*,
                           const __hip_bfloat16*, const int*, const float*, const float*,
                           const float*, __hip_bfloat16*, __hip_bfloat16*, int, int, int, int,
                           float, int, unsigned, unsigned long long, long, long, long,
                           hipStream_t);
void launch_decode_self(const __hip_bfloat16*, const __hip_bfloat16*, const __hip_bfloat16*,
                        __hip_bfloat16*, __hip_bfloat16*, const int*, const float*,
                        __hip_bfloat16*, long, int, int, int, float, long, long, long,
                        hipStream_t);
size_t decode_cross_lds_bytes(int);
void launch_decode_cross(const __hip_bfloat16*, const __hip_bfloat16*, const __hip_bfloat16*,
                         const int*, __hip_bfloat16*, int, int, int, int, float, long, long, long,
                         long, long, hipStream_t);
void dkv_prof_fetch(unsigned long long*);
void fwd_prof_fetch(unsigned long long*);
template <typename T>
void launch_dropout_add_fwd(const T*, const T*, T*, long, float, unsigned long long,
                            hipStream_t);
template <typename T>
void launch_dropout_add_bwd(const T*, T*, long, float, unsigned long long, hipStream_t);
template <typename T>
void launch_ln_res_dropout_fwd(const T*, const T*, const float*, const float*, T*, float*,
                               float*, long, int, float, float, unsigned long long, hipStream_t);
template <typename T>
void launch_ln_res_dropout_bwd(const T*, const T*, const T*, const float*, const float*,
                               const float*, T*, T*, T*, long, int, float,
                               unsigned long long, hipStream_t);
template <typename T>
void launch_ln_res_dropout_wgrad(const T*, const T*, const T*, const float*, const float*,
                                 float*, float*, long, int, float, unsigned long long,
                                 hipStream_t);
template <typename T>
void launch_embed_scatter(const T*, const long*, float*, long, int, long, hipStream_t);
void launch_relbias_wgrad(const float*, const int*, float*, long, int, int,
                          hipStream_t);
template <typename T>
void launch_relu_dropout_fwd(const T*, T*, long, float, unsigned long long, hipStream_t);
template <typename T>
void launch_relu_dropout_bwd(const T*, const T*, T*, long, float, unsigned long long,
                             hipStream_t);

#define CHECK_GPU(t) \
  TORCH_CHECK((t).is_cuda() && (t).is_contiguous(), #t " must be contiguous GPU tensor")

static hipStream_t cur_stream() {
  return c10::hip::getCurrentHIPStream().stream();
}

template <typename F>
void dispatch_float_bf16(const at::Tensor& t, const char* name, F&& f) {
  if (t.scalar_type() == at::kFloat) {
    f(float{});
  } else if (t.scalar_type() == at::kBFloat16) {
    f(__hip_bfloat16{});
  } else {
    TORCH_CHECK(false, name, ": unsupported dtype ", t.scalar_type());
  }
}

// fp32 gradient accumulator of an op: `out` when given — a live flat .grad
// view (parallel/optim.py) the kernel ADDS into — else fresh zeros.
static at::Tensor acc_or_zeros(const c10::optional<at::Tensor>& out, at::IntArrayRef shape,
                               const at::TensorOptions& like, const char* name) {
  if (!out.has_value()) return at::zeros(shape, like.dtype(at::kFloat));
  TORCH_CHECK(out->is_cuda() && out->scalar_type() == at::kFloat && out->is_contiguous() &&
                  out->numel() == c10::multiply_integers(shape),
              name, ": accumulator must be a contiguous fp32 GPU tensor of ",
              c10::multiply_integers(shape), " elements");
  return *out;
}

template <typename T>
const T* ptr(const at::Tensor& t) {
  return reinterpret_cast<const T*>(t.data_ptr());
}
template <typename T>
T* mptr(at::Tensor& t) {
  return reinterpret_cast<T*>(t.data_ptr());
}

at::Tensor embed4_fwd(at::Tensor tables, at::Tensor idx, bool out_bf16 = false) {
  CHECK_GPU(tables);
  CHECK_GPU(idx);
  TORCH_CHECK(tables.dim() == 3 && tables.size(0) == 4 && tables.size(2) == 32,
              "tables must be (4, V, 32)");
  TORCH_CHECK(idx.dim() == 2 && idx.size(1) == 4 && idx.scalar_type() == at::kLong);
  const int N = idx.size(0);
  const int V = tables.size(1);
  if (out_bf16 && tables.scalar_type() == at::kFloat) {
    // autocast path: gather fp32 master rows, emit bf16 directly
    auto out = at::empty({N, 128}, tables.options().dtype(at::kBFloat16));
    launch_embed4_fwd2<float, __hip_bfloat16>(
        tables.data_ptr<float>(), idx.data_ptr<long>(),
        reinterpret_cast<__hip_bfloat16*>(out.data_ptr()), N, V, cur_stream());
    return out;
  }
  auto out = at::empty({N, 128}, tables.options());
  dispatch_float_bf16(tables, "embed4_fwd", [&](auto tag) {
    using T = decltype(tag);
    launch_embed4_fwd<T>(ptr<T>(tables), idx.data_ptr<long>(), mptr<T>(out), N, V, cur_stream());
  });
  return out;
}

at::Tensor embed4_bwd(at::Tensor grad_out, at::Tensor idx, long V, long Demb,
                      c10::optional<at::Tensor> out_opt) {
  CHECK_GPU(grad_out);
  CHECK_GPU(idx);
  TORCH_CHECK(Demb == 32, "Demb must be 32");
  const bool acc = out_opt.has_value();  // the flat .grad region of the 4 tables
  auto grad = acc_or_zeros(out_opt, {4, V, Demb}, grad_out.options(), "embed4_bwd");
  const long total = grad_out.numel();
  dispatch_float_bf16(grad_out, "embed4_bwd", [&](auto tag) {
    using T = decltype(tag);
    launch_embed4_bwd<T>(ptr<T>(grad_out), idx.data_ptr<long>(), grad.data_ptr<float>(), total,
                         (int)V, cur_stream());
  });
  return acc ? grad : grad.to(grad_out.scalar_type());
}

at::Tensor spmm_sum(at::Tensor indptr, at::Tensor indices, at::Tensor x) {
  CHECK_GPU(indptr);
  CHECK_GPU(indices);
  CHECK_GPU(x);
  TORCH_CHECK(indptr.scalar_type() == at::kInt && indices.scalar_type() == at::kInt);
  const int N = indptr.size(0) - 1;
  const int D = x.size(1);
  TORCH_CHECK(D % 2 == 0, "D must be even");
  TORCH_CHECK(x.size(0) == N, "x rows must match indptr");
  auto out = at::empty_like(x);
  dispatch_float_bf16(x, "spmm_sum", [&](auto tag) {
    using T = decltype(tag);
    launch_spmm_sum<T>(indptr.data_ptr<int>(), indices.data_ptr<int>(), ptr<T>(x), mptr<T>(out),
                       N, D, cur_stream());
  });
  return out;
}

std::vector<at::Tensor> gru_gates_fwd(at::Tensor gi, at::Tensor gh, at::Tensor h) {
  CHECK_GPU(gi);
  CHECK_GPU(gh);
  CHECK_GPU(h);
  const long N = h.size(0);
  const int H = h.size(1);
  TORCH_CHECK(gi.size(1) == 3 * H && gh.size(1) == 3 * H);
  TORCH_CHECK(gi.scalar_type() == h.scalar_type() && gh.scalar_type() == h.scalar_type(),
              "gi/gh/h dtypes must match");
  auto h_new = at::empty_like(h);
  auto r = at::empty_like(h);
  auto z = at::empty_like(h);
  auto n = at::empty_like(h);
  dispatch_float_bf16(h, "gru_gates_fwd", [&](auto tag) {
    using T = decltype(tag);
    launch_gru_gates_fwd<T>(ptr<T>(gi), ptr<T>(gh), ptr<T>(h), mptr<T>(h_new), mptr<T>(r),
                            mptr<T>(z), mptr<T>(n), N * H, H, cur_stream());
  });
  return {h_new, r, z, n};
}

std::vector<at::Tensor> gru_gates_bwd(at::Tensor grad_h_new, at::Tensor gh, at::Tensor h,
                                      at::Tensor r, at::Tensor z, at::Tensor n) {
  CHECK_GPU(grad_h_new);
  const long N = h.size(0);
  const int H = h.size(1);
  auto grad_gi = at::empty({N, 3 * H}, h.options());
  auto grad_gh = at::empty({N, 3 * H}, h.options());
  auto grad_h = at::empty_like(h);
  dispatch_float_bf16(h, "gru_gates_bwd", [&](auto tag) {
    using T = decltype(tag);
    launch_gru_gates_bwd<T>(ptr<T>(grad_h_new), ptr<T>(gh), ptr<T>(h), ptr<T>(r), ptr<T>(z),
                            ptr<T>(n), mptr<T>(grad_gi), mptr<T>(grad_gh), mptr<T>(grad_h), N * H,
                            H, cur_stream());
  });
  return {grad_gi, grad_gh, grad_h};
}

std::vector<at::Tensor> attn_pool_fwd(at::Tensor x, at::Tensor gate, at::Tensor node_offsets) {
  CHECK_GPU(x);
  CHECK_GPU(gate);
  CHECK_GPU(node_offsets);
  TORCH_CHECK(node_offsets.scalar_type() == at::kInt);
  TORCH_CHECK(gate.scalar_type() == x.scalar_type(), "gate/x dtypes must match");
  const int B = node_offsets.size(0) - 1;
  const int D = x.size(1);
  auto out = at::empty({B, D}, x.options());
  auto alpha = at::empty({x.size(0)}, x.options().dtype(at::kFloat));
  dispatch_float_bf16(x, "attn_pool_fwd", [&](auto tag) {
    using T = decltype(tag);
    launch_attn_pool_fwd<T>(ptr<T>(x), ptr<T>(gate), node_offsets.data_ptr<int>(), mptr<T>(out),
                            alpha.data_ptr<float>(), B, D, cur_stream());
  });
  return {out, alpha};
}

std::vector<at::Tensor> attn_pool_bwd(at::Tensor grad_out, at::Tensor x, at::Tensor alpha,
                                      at::Tensor node_offsets) {
  CHECK_GPU(grad_out);
  CHECK_GPU(x);
  CHECK_GPU(alpha);
  const int B = node_offsets.size(0) - 1;
  const int D = x.size(1);
  auto grad_x = at::empty_like(x);
  auto grad_gate = at::empty({x.size(0)}, x.options());
  auto s_ws = at::empty({x.size(0)}, x.options().dtype(at::kFloat));
  dispatch_float_bf16(x, "attn_pool_bwd", [&](auto tag) {
    using T = decltype(tag);
    launch_attn_pool_bwd<T>(ptr<T>(grad_out), ptr<T>(x), alpha.data_ptr<float>(),
                            node_offsets.data_ptr<int>(), mptr<T>(grad_x), mptr<T>(grad_gate),
                            s_ws.data_ptr<float>(), B, D, cur_stream());
  });
  return {grad_x, grad_gate};
}

at::Tensor segment_max(at::Tensor values, at::Tensor node_offsets) {
  CHECK_GPU(values);
  CHECK_GPU(node_offsets);
  TORCH_CHECK(values.scalar_type() == at::kFloat, "segment_max expects fp32");
  const int B = node_offsets.size(0) - 1;
  auto out = at::empty({B}, values.options());
  launch_segment_max(values.data_ptr<float>(), node_offsets.data_ptr<int>(),
                     out.data_ptr<float>(), B, cur_stream());
  return out;
}

// ---------------------------------------------------------------------------
// Fused GGNN: the whole n_steps message-passing loop driven from C++.
// Replaces {linear, spmm, GRUCell} x n_steps of the reference's DGL
// GatedGraphConv (ggnn.py:57-60,95) with per step:
//   wh    = gemm_bias(h, W_e^T) + b_e                      [MFMA]
//   m     = csr_segment_sum(wh)                            [spmm kernel]
//   gicat = gemm_bias([m|h], Wcat^T) + b_cat               [MFMA, split-A]
//   h     = fused_gru_gates(gicat, h)                      [elementwise]
// Wcat is the (4H, 2H) block weight matrix [W_ir|W_hr; W_iz|W_hz; W_in|0;
// 0|W_hn] so one GEMM produces all gate pre-activations.
// ---------------------------------------------------------------------------

using bf16_t = __hip_bfloat16;

at::Tensor gemm_bias(at::Tensor A, at::Tensor W, c10::optional<at::Tensor> bias,
                     c10::optional<at::Tensor> addend) {
  CHECK_GPU(A);
  CHECK_GPU(W);
  TORCH_CHECK(A.scalar_type() == at::kBFloat16 && W.scalar_type() == at::kBFloat16);
  const int N = A.size(0), K = A.size(1), COL = W.size(0);
  TORCH_CHECK(W.size(1) == K && K % 64 == 0 && COL % 128 == 0);
  auto out = at::empty({N, COL}, A.options());
  const bf16_t* b = nullptr;
  if (bias.has_value()) b = reinterpret_cast<const bf16_t*>(bias->data_ptr());
  const bf16_t* add = nullptr;
  if (addend.has_value()) {
    TORCH_CHECK(addend->is_contiguous() && addend->sizes() == out.sizes());
    add = reinterpret_cast<const bf16_t*>(addend->data_ptr());
  }
  launch_gemm_bias(ptr<bf16_t>(A), nullptr, ptr<bf16_t>(W), b, add, mptr<bf16_t>(out), N, K, K,
                   COL, cur_stream());
  return out;
}

// out(M, C) = A(K, M)^T @ B(K, C), fp32 output (wgrad shape class).
// 128-aligned shapes take the pipelined wgrad2 kernel; others the generic
// split-K kernel.
// `out` (optional): ACCUMULATE the weight grad into an existing pre-zeroed
// fp32 buffer — the flat optimizer's .grad view — via atomic epilogues.
// Skips the per-call zeros() fill and autograd's AccumulateGrad add
// (~145 fills + ~270 adds = ~2.7 ms/step on the CodeT5 step).
at::Tensor wgrad(at::Tensor A, at::Tensor B, c10::optional<at::Tensor> out_opt) {
  CHECK_GPU(A);
  CHECK_GPU(B);
  const int K = A.size(0), M = A.size(1), C = B.size(1);
  TORCH_CHECK(B.size(0) == K && M % 64 == 0 && C % 8 == 0);
  const bool acc = out_opt.has_value();
  // always zero-init: whether the launcher plain-stores (one K chunk) or
  // atomically accumulates (split K) is ITS decision — duplicating the
  // chunking math here to pick empty-vs-zeros risked an uninitialized
  // accumulator if the two ever diverged (they did differ by K-floor)
  auto out = acc_or_zeros(out_opt, {M, C}, A.options(), "wgrad");
  if (M % 128 == 0 && C % 128 == 0) {  // wgrad2 zero-fills K tails
    launch_wgrad2(ptr<bf16_t>(A), ptr<bf16_t>(B), out.data_ptr<float>(), nullptr,
                  K, M, C, acc ? 1 : 0, cur_stream());
    return out;
  }
  launch_wgrad(ptr<bf16_t>(A), ptr<bf16_t>(B), nullptr, out.data_ptr<float>(), nullptr,
               K, M, C, C, cur_stream());
  return out;
}

void launch_pack_gru_weights(const float*, const float*, const float*, const float*,
                             const float*, const float*, int, __hip_bfloat16*,
                             __hip_bfloat16*, __hip_bfloat16*, __hip_bfloat16*,
                             __hip_bfloat16*, __hip_bfloat16*, __hip_bfloat16*,
                             __hip_bfloat16*, hipStream_t);
void launch_gemm_gru(const __hip_bfloat16*, const __hip_bfloat16*, const __hip_bfloat16*,
                     const __hip_bfloat16*, const __hip_bfloat16*, __hip_bfloat16*,
                     __hip_bfloat16*, __hip_bfloat16*, __hip_bfloat16*, __hip_bfloat16*,
                     int, int, int, int, hipStream_t, const int* = nullptr,
                     const int* = nullptr, __hip_bfloat16* = nullptr);

// one-launch refresh of every derived GGNN weight buffer (bf16 casts,
// Wcat/WcatT block matrix, merged bias) — see ops/flowgnn.py cache
void pack_gru_weights(at::Tensor W_e, at::Tensor b_e, at::Tensor W_ih, at::Tensor W_hh,
                      at::Tensor b_ih, at::Tensor b_hh, at::Tensor w_e16, at::Tensor b_e16,
                      at::Tensor Wcat, at::Tensor WcatT, at::Tensor b_cat, at::Tensor W_eT,
                      at::Tensor Wcat_perm, at::Tensor b_perm) {
  CHECK_GPU(W_e);
  const int H = W_e.size(0);
  TORCH_CHECK(W_e.scalar_type() == at::kFloat && W_ih.scalar_type() == at::kFloat,
              "pack_gru_weights reads fp32 master weights");
  TORCH_CHECK(Wcat.size(0) == 4 * H && Wcat.size(1) == 2 * H);
  launch_pack_gru_weights(W_e.data_ptr<float>(), b_e.data_ptr<float>(),
                          W_ih.data_ptr<float>(), W_hh.data_ptr<float>(),
                          b_ih.data_ptr<float>(), b_hh.data_ptr<float>(), H,
                          mptr<bf16_t>(w_e16), mptr<bf16_t>(b_e16), mptr<bf16_t>(Wcat),
                          mptr<bf16_t>(WcatT), mptr<bf16_t>(b_cat), mptr<bf16_t>(W_eT),
                          mptr<bf16_t>(Wcat_perm), mptr<bf16_t>(b_perm),
                          cur_stream());
}

std::vector<at::Tensor> ggnn_fused_fwd(at::Tensor indptr, at::Tensor indices, at::Tensor x,
                                       at::Tensor W_e, at::Tensor b_e, at::Tensor Wcat_perm,
                                       at::Tensor b_perm, long n_steps, bool fuse) {
  CHECK_GPU(x);
  TORCH_CHECK(x.scalar_type() == at::kBFloat16, "fused GGNN path is bf16");
  const long N = x.size(0);
  const long H = x.size(1);
  TORCH_CHECK(H % 64 == 0 && (4 * H) % 128 == 0, "H must suit the MFMA tile");
  TORCH_CHECK(Wcat_perm.size(0) == 4 * H && Wcat_perm.size(1) == 2 * H &&
              b_perm.numel() == 4 * H,
              "Wcat_perm/b_perm must be prebuilt (ops/flowgnn.py cache)");
  auto stream = cur_stream();
  const long S = n_steps;
  auto opts = x.options();
  // HH[s] = hidden state entering step s; HH[S] = final output.
  auto HH = at::empty({S + 1, N, H}, opts);
  HH.select(0, 0).copy_(x);
  auto M = at::empty({S, N, H}, opts);
  auto R = at::empty({S, N, H}, opts);
  auto Z = at::empty({S, N, H}, opts);
  auto Nn = at::empty({S, N, H}, opts);
  auto HN = at::empty({S, N, H}, opts);
  auto wh = at::empty({N, H}, opts);
  const long NH = N * H;
  for (long s = 0; s < S; ++s) {
    const bf16_t* h = ptr<bf16_t>(HH) + s * NH;
    launch_gemm_bias(h, nullptr, ptr<bf16_t>(W_e), ptr<bf16_t>(b_e), nullptr, mptr<bf16_t>(wh),
                     N, H, H, H, stream);
    bf16_t* m = mptr<bf16_t>(M) + s * NH;
    // fuse: M[s] = spmm_sum(wh) is formed in gemm_gru's A staging (and
    // stored from there); otherwise by its own launch
    if (!fuse)
      launch_spmm_sum<bf16_t>(indptr.data_ptr<int>(), indices.data_ptr<int>(), ptr<bf16_t>(wh),
                              m, N, H, stream);
    // fused gate GEMM + GRU cell (gate-interleaved Wcat layout): replaces
    // the gicat GEMM + separate gru_gates2_fwd, with fp32 pre-activations
    launch_gemm_gru(fuse ? ptr<bf16_t>(wh) : m, h, ptr<bf16_t>(Wcat_perm), ptr<bf16_t>(b_perm),
                    h, mptr<bf16_t>(HH) + (s + 1) * NH, mptr<bf16_t>(R) + s * NH,
                    mptr<bf16_t>(Z) + s * NH, mptr<bf16_t>(Nn) + s * NH,
                    mptr<bf16_t>(HN) + s * NH, N, 2 * H, H, H, stream,
                    fuse ? indptr.data_ptr<int>() : nullptr,
                    fuse ? indices.data_ptr<int>() : nullptr, fuse ? m : nullptr);
  }
  auto h_final = HH.select(0, S);
  return {h_final, HH, M, R, Z, Nn, HN};
}

// The six GGNN parameter grads of K = S*N saved rows at H = 128, one launch.
// gru_outs = [gW_ih, gW_hh, gb_ih, gb_hh] and out_we/out_be are live flat
// .grad views the kernel adds into; without them fresh zero-filled tensors
// are returned. Returns {gW_ih, gW_hh, gb_ih, gb_hh, gW_e, gb_e}.
static std::vector<at::Tensor> ggnn_wgrad_run(const at::Tensor& Ggicat, const at::Tensor& M,
                                              const at::Tensor& HH, const at::Tensor& Gwh,
                                              long K, long H,
                                              const c10::optional<at::Tensor>& out_we,
                                              const c10::optional<at::Tensor>& out_be,
                                              const c10::optional<std::vector<at::Tensor>>& gru_outs,
                                              long kchunk = 0, long lds_epi = -1,
                                              bool two_launches = false) {
  TORCH_CHECK(H == 128, "ggnn_wgrad is written for H = 128");
  TORCH_CHECK(out_be.has_value() == out_we.has_value(),
              "ggnn_wgrad: out_we and out_be go together");
  auto opts = Ggicat.options();
  const bool gru_direct = gru_outs.has_value();
  if (gru_direct)
    TORCH_CHECK(gru_outs->size() == 4, "gru_outs = [gW_ih, gW_hh, gb_ih, gb_hh]");
  auto pick = [&](int i) {
    return gru_direct ? c10::optional<at::Tensor>((*gru_outs)[i]) : c10::nullopt;
  };
  auto gW_ih = acc_or_zeros(pick(0), {3 * H, H}, opts, "ggnn_wgrad gW_ih");
  auto gW_hh = acc_or_zeros(pick(1), {3 * H, H}, opts, "ggnn_wgrad gW_hh");
  auto gb_ih = acc_or_zeros(pick(2), {3 * H}, opts, "ggnn_wgrad gb_ih");
  auto gb_hh = acc_or_zeros(pick(3), {3 * H}, opts, "ggnn_wgrad gb_hh");
  auto gW_e = acc_or_zeros(out_we, {H, H}, opts, "ggnn_wgrad out_we");
  auto gb_e = acc_or_zeros(out_be, {H}, opts, "ggnn_wgrad out_be");
  if (two_launches) {  // the old pair on the same six buffers (probe A/B only)
    launch_wgrad(ptr<bf16_t>(Ggicat), ptr<bf16_t>(M), ptr<bf16_t>(HH), nullptr, nullptr, K,
                 4 * H, 2 * H, H, cur_stream(), gW_ih.data_ptr<float>(),
                 gW_hh.data_ptr<float>(), gb_ih.data_ptr<float>(), gb_hh.data_ptr<float>());
    launch_wgrad2(ptr<bf16_t>(Gwh), ptr<bf16_t>(HH), gW_e.data_ptr<float>(),
                  gb_e.data_ptr<float>(), K, H, H, 1, cur_stream());
    return {gW_ih, gW_hh, gb_ih, gb_hh, gW_e, gb_e};
  }
  // live views: the r/z column sums are added to both biases by the kernel.
  // Fresh tensors: added to gb_ih only and copied, so that the two returned
  // halves are the same bits (atomic order would otherwise differ).
  launch_ggnn_wgrad(ptr<bf16_t>(Ggicat), ptr<bf16_t>(Gwh), ptr<bf16_t>(M), ptr<bf16_t>(HH),
                    gW_ih.data_ptr<float>(), gW_hh.data_ptr<float>(), gW_e.data_ptr<float>(),
                    gb_ih.data_ptr<float>(), gb_hh.data_ptr<float>(), gb_e.data_ptr<float>(),
                    (int)K, gru_direct ? 1 : 0, (int)kchunk, (int)lds_epi, cur_stream());
  if (!gru_direct) gb_hh.narrow(0, 0, 2 * H).copy_(gb_ih.narrow(0, 0, 2 * H));
  return {gW_ih, gW_hh, gb_ih, gb_hh, gW_e, gb_e};
}

// raw binding of the kernel alone, for tests and tools/ggnn_wgrad_probe.py.
// HH may carry more slabs than S (the loop's HH has S + 1); only the first
// S*N rows of any operand are read. kchunk = 0 / lds_epi = -1 (K rows per
// chunk, LDS-staged epilogue): the launcher's defaults.
// two_launches runs the wgrad_kernel + wgrad2_kernel pair it replaced on the
// same buffers, for a same-build timing A/B.
std::vector<at::Tensor> ggnn_wgrad(at::Tensor Ggicat, at::Tensor M, at::Tensor HH,
                                   at::Tensor Gwh, long S,
                                   c10::optional<at::Tensor> out_we,
                                   c10::optional<at::Tensor> out_be,
                                   c10::optional<std::vector<at::Tensor>> gru_outs,
                                   long kchunk, long lds_epi, bool two_launches) {
  CHECK_GPU(Ggicat);
  CHECK_GPU(M);
  CHECK_GPU(HH);
  CHECK_GPU(Gwh);
  for (const at::Tensor* t : {&Ggicat, &M, &HH, &Gwh})
    TORCH_CHECK(t->scalar_type() == at::kBFloat16 && t->dim() == 3, "ggnn_wgrad: (S, N, cols) bf16");
  const long N = M.size(1);
  const long H = M.size(2);
  TORCH_CHECK(S >= 0 && Ggicat.size(0) >= S && M.size(0) >= S && HH.size(0) >= S &&
                  Gwh.size(0) >= S,
              "ggnn_wgrad: fewer than S slabs");
  TORCH_CHECK(Ggicat.size(1) == N && HH.size(1) == N && Gwh.size(1) == N &&
                  Ggicat.size(2) == 4 * H && HH.size(2) == H && Gwh.size(2) == H,
              "ggnn_wgrad: operand shapes disagree");
  TORCH_CHECK(S * N < (1L << 31), "ggnn_wgrad: S*N must fit an int");
  return ggnn_wgrad_run(Ggicat, M, HH, Gwh, S * N, H, out_we, out_be, gru_outs, kchunk,
                        lds_epi, two_launches);
}

std::vector<at::Tensor> ggnn_fused_bwd(at::Tensor grad_out, at::Tensor t_indptr,
                                       at::Tensor t_indices, at::Tensor x, at::Tensor W_eT,
                                       at::Tensor WcatT, at::Tensor HH,
                                       at::Tensor M, at::Tensor R, at::Tensor Z, at::Tensor Nn,
                                       at::Tensor HN, long n_steps,
                                       c10::optional<at::Tensor> out_we,
                                       c10::optional<at::Tensor> out_be,
                                       c10::optional<std::vector<at::Tensor>> gru_outs,
                                       bool fuse, bool fused_wgrad) {
  const long N = x.size(0);
  const long H = x.size(1);
  const long S = n_steps;
  const long NH = N * H;
  auto stream = cur_stream();
  TORCH_CHECK(WcatT.size(0) == 2 * H && WcatT.size(1) == 4 * H && W_eT.size(0) == H,
              "WcatT/W_eT must be prebuilt (ops/flowgnn.py cache)");
  auto opts = x.options();
  // per-step gate/message grads, kept for ONE batched K = S*N weight-grad
  // GEMM at the end (hipBLASLt's transpose-A kernels are the pathology the
  // custom split-K wgrad kernel replaces; see csrc/wgrad.hip header)
  auto Ggicat = at::empty({S, N, 4 * H}, opts);
  auto Gwh = at::empty({S, N, H}, opts);
  // grad_out is only read: step S-1 takes it as its incoming grad, and every
  // step writes the grad of its h_in into the loop's own buffer
  auto go = grad_out.contiguous();
  auto grad_h = S > 0 ? at::empty({N, H}, opts) : go.clone();
  auto grad_hd = at::empty({N, H}, opts);
  auto grad_A = at::empty({N, 2 * H}, opts);
  for (long s = S - 1; s >= 0; --s) {
    const bf16_t* h_in = ptr<bf16_t>(HH) + s * NH;
    const bf16_t* g_in = (s == S - 1) ? ptr<bf16_t>(go) : ptr<bf16_t>(grad_h);
    auto ggic = Ggicat.select(0, s);
    auto gwh = Gwh.select(0, s);
    // grad_A = ggic @ Wcat : (N, 2H); left half = grad_m, right = gh-path.
    // fuse: the gate backward is the GEMM's prologue (one launch) where the
    // tile fits; otherwise gru_gates2_bwd writes ggic and the GEMM reads it
    if (!fuse ||
        !launch_gates_gemm(g_in, h_in, ptr<bf16_t>(R) + s * NH, ptr<bf16_t>(Z) + s * NH,
                           ptr<bf16_t>(Nn) + s * NH, ptr<bf16_t>(HN) + s * NH,
                           ptr<bf16_t>(WcatT), mptr<bf16_t>(ggic), mptr<bf16_t>(grad_hd),
                           mptr<bf16_t>(grad_A), N, H, stream)) {
      launch_gru_gates2_bwd<bf16_t>(g_in, h_in, ptr<bf16_t>(R) + s * NH,
                                    ptr<bf16_t>(Z) + s * NH, ptr<bf16_t>(Nn) + s * NH,
                                    ptr<bf16_t>(HN) + s * NH, mptr<bf16_t>(ggic),
                                    mptr<bf16_t>(grad_hd), NH, H, stream);
      launch_gemm_bias(ptr<bf16_t>(ggic), nullptr, ptr<bf16_t>(WcatT), nullptr, nullptr,
                       mptr<bf16_t>(grad_A), N, 4 * H, 4 * H, 2 * H, stream);
    }
    // grad wrt h_in = (grad_wh @ W_e) + direct z-path + gh-path, the two
    // additions fused into the GEMM epilogue as strided addends. grad_wh =
    // Gwh[s] is the CSC segment sum of grad_m, read STRIDED out of grad_A's
    // left half (no contiguous copy). fuse: summed in the GEMM's A staging
    // (and stored from there); otherwise by its own launch
    if (fuse) {
      launch_gemm_bias2(ptr<bf16_t>(grad_A), nullptr, ptr<bf16_t>(W_eT), nullptr,
                        ptr<bf16_t>(grad_hd), H, ptr<bf16_t>(grad_A) + H, 2 * H,
                        mptr<bf16_t>(grad_h), N, H, H, H, stream,
                        t_indptr.data_ptr<int>(), t_indices.data_ptr<int>(), 2 * H,
                        mptr<bf16_t>(gwh));
    } else {
      launch_spmm_sum_strided<bf16_t>(t_indptr.data_ptr<int>(), t_indices.data_ptr<int>(),
                                      ptr<bf16_t>(grad_A), mptr<bf16_t>(gwh), N, H,
                                      2 * H, stream);
      launch_gemm_bias2(ptr<bf16_t>(gwh), nullptr, ptr<bf16_t>(W_eT), nullptr,
                        ptr<bf16_t>(grad_hd), H, ptr<bf16_t>(grad_A) + H, 2 * H,
                        mptr<bf16_t>(grad_h), N, H, H, H, stream);
    }
  }
  // batched weight/bias grads over all steps (K = S*N). At H = 128 one
  // launch forms the seven live 128 x 128 tiles and the five bias sums;
  // fused_wgrad = false (and every other H) keeps the two launches below.
  if (fused_wgrad && H == 128) {
    auto g = ggnn_wgrad_run(Ggicat, M, HH, Gwh, S * N, H, out_we, out_be, gru_outs);
    if (gru_outs.has_value()) {  // grads already accumulated in the flat views
      auto none = at::empty({0}, opts.dtype(at::kFloat));
      return {grad_h, g[4], g[5], none, none, none, none};
    }
    return {grad_h, g[4], g[5], g[0], g[1], g[2], g[3]};
  }
  auto A_g = Ggicat.view({S * N, 4 * H});
  const bool gru_direct = gru_outs.has_value();
  at::Tensor gWcat, cs4;
  if (gru_direct) {  // scatter epilogue straight into the 4 flat .grad views
    TORCH_CHECK(gru_outs->size() == 4, "gru_outs = [gW_ih, gW_hh, gb_ih, gb_hh]");
    for (auto& t : *gru_outs)
      TORCH_CHECK(t.is_cuda() && t.scalar_type() == at::kFloat && t.is_contiguous());
    TORCH_CHECK((*gru_outs)[0].numel() == 3 * H * H &&
                (*gru_outs)[1].numel() == 3 * H * H &&
                (*gru_outs)[2].numel() == 3 * H && (*gru_outs)[3].numel() == 3 * H);
  } else {
    gWcat = at::zeros({4 * H, 2 * H}, opts.dtype(at::kFloat));
    cs4 = at::zeros({4 * H}, opts.dtype(at::kFloat));
  }
  // The two-launch path: H = 64, 192, ... and the fused_wgrad = false A/B.
  // Bias grads (column sums of the gate/message grads) ride along in the
  // wgrad kernels' A-tile staging. The gate wgrad is the packed (4H, 2H)
  // SPLIT-B product with the GRU scatter epilogue, which only the generic
  // bounds-checked split-K kernel has (it also computes the two dead
  // tiles); the W_e grad (plain A^T B) takes the tr16-subtiled wgrad2 where
  // H is a multiple of 128 (K tails zero-filled in staging).
  if (gru_direct)
    launch_wgrad(ptr<bf16_t>(A_g), ptr<bf16_t>(M), ptr<bf16_t>(HH), nullptr, nullptr,
                 S * N, 4 * H, 2 * H, H, stream, (*gru_outs)[0].data_ptr<float>(),
                 (*gru_outs)[1].data_ptr<float>(), (*gru_outs)[2].data_ptr<float>(),
                 (*gru_outs)[3].data_ptr<float>());
  else
    launch_wgrad(ptr<bf16_t>(A_g), ptr<bf16_t>(M), ptr<bf16_t>(HH), gWcat.data_ptr<float>(),
                 cs4.data_ptr<float>(), S * N, 4 * H, 2 * H, H, stream);
  auto A_w = Gwh.view({S * N, H});
  const bool acc_we = out_we.has_value();  // W_e/b_e grads into the flat .grad views
  TORCH_CHECK(out_be.has_value() == acc_we, "ggnn_fused_bwd: out_we and out_be go together");
  auto gW_e = acc_or_zeros(out_we, {H, H}, opts, "ggnn_fused_bwd out_we");
  auto cs_e = acc_or_zeros(out_be, {H}, opts, "ggnn_fused_bwd out_be");
  if (H % 128 == 0)
    launch_wgrad2(ptr<bf16_t>(A_w), ptr<bf16_t>(HH), gW_e.data_ptr<float>(),
                  cs_e.data_ptr<float>(), S * N, H, H, acc_we ? 1 : 0, stream);
  else  // wgrad2 needs 128-aligned M and C; the generic kernel is bounds-checked
    launch_wgrad(ptr<bf16_t>(A_w), ptr<bf16_t>(HH), nullptr, gW_e.data_ptr<float>(),
                 cs_e.data_ptr<float>(), S * N, H, H, H, stream);
  if (gru_direct) {  // grads already accumulated in the flat views
    auto none = at::empty({0}, opts.dtype(at::kFloat));
    return {grad_h, gW_e, cs_e, none, none, none, none};
  }
  // scatter gWcat blocks back to the GRUCell weight layout (views are fine
  // as autograd outputs; no contiguous copy)
  auto gW_ih = gWcat.narrow(0, 0, 3 * H).narrow(1, 0, H);
  auto gW_hh = at::cat({gWcat.narrow(0, 0, 2 * H).narrow(1, H, H),
                        gWcat.narrow(0, 3 * H, H).narrow(1, H, H)});
  auto gb_ih = cs4.narrow(0, 0, 3 * H).contiguous();
  auto gb_hh = at::cat({cs4.narrow(0, 0, 2 * H), cs4.narrow(0, 3 * H, H)});
  return {grad_h, gW_e, cs_e, gW_ih, gW_hh, gb_ih, gb_hh};
}

std::vector<at::Tensor> gru_gates2_fwd(at::Tensor gicat, at::Tensor h) {
  CHECK_GPU(gicat);
  CHECK_GPU(h);
  const long N = h.size(0);
  const int H = h.size(1);
  auto h_new = at::empty_like(h);
  auto r = at::empty_like(h);
  auto z = at::empty_like(h);
  auto n = at::empty_like(h);
  auto hn = at::empty_like(h);
  dispatch_float_bf16(h, "gru_gates2_fwd", [&](auto tag) {
    using T = decltype(tag);
    launch_gru_gates2_fwd<T>(ptr<T>(gicat), ptr<T>(h), mptr<T>(h_new), mptr<T>(r), mptr<T>(z),
                             mptr<T>(n), mptr<T>(hn), N * H, H, cur_stream());
  });
  return {h_new, r, z, n, hn};
}

// stand-alone entry to the gate backward the fused loop launches per step
// (unit tests); returns {grad_gicat (N, 4H), grad_h_direct (N, H)}
std::vector<at::Tensor> gru_gates2_bwd(at::Tensor grad_h_new, at::Tensor h, at::Tensor r,
                                       at::Tensor z, at::Tensor n, at::Tensor hn) {
  CHECK_GPU(grad_h_new);
  CHECK_GPU(h);
  const long N = h.size(0);
  const int H = h.size(1);
  for (const at::Tensor* t : {&grad_h_new, &r, &z, &n, &hn})
    TORCH_CHECK(t->is_cuda() && t->is_contiguous() && t->sizes() == h.sizes() &&
                    t->scalar_type() == h.scalar_type(),
                "gru_gates2_bwd: operands must match h");
  auto grad_gicat = at::empty({N, 4 * H}, h.options());
  auto grad_h = at::empty_like(h);
  dispatch_float_bf16(h, "gru_gates2_bwd", [&](auto tag) {
    using T = decltype(tag);
    launch_gru_gates2_bwd<T>(ptr<T>(grad_h_new), ptr<T>(h), ptr<T>(r), ptr<T>(z), ptr<T>(n),
                             ptr<T>(hn), mptr<T>(grad_gicat), mptr<T>(grad_h), N * H, H,
                             cur_stream());
  });
  return {grad_gicat, grad_h};
}

at::Tensor colsum(at::Tensor x, c10::optional<at::Tensor> out_opt) {
  CHECK_GPU(x);
  TORCH_CHECK(x.dim() == 2, "colsum: x must be (N, C)");
  TORCH_CHECK(x.size(0) <= INT_MAX && x.size(1) <= INT_MAX, "colsum: extent exceeds int");
  auto out = acc_or_zeros(out_opt, {x.size(1)}, x.options(), "colsum");
  dispatch_float_bf16(x, "colsum", [&](auto tag) {
    using T = decltype(tag);
    launch_colsum<T>(ptr<T>(x), out.data_ptr<float>(), x.size(0), x.size(1), cur_stream());
  });
  return out;
}


// ---------------------------------------------------------------------------
// Transformer kernels (csrc/transformer_kernels.hip)
// ---------------------------------------------------------------------------

// Argument checks shared by every binding of this family. The kernels index
// raw pointers, so each tensor argument is held to: contiguous, on the lead
// tensor's device, the expected dtype and the expected shape.
static constexpr size_t kLdsLimit = 64 * 1024;  // dynamic LDS without opt-in

static void tk_lead(const char* op, const at::Tensor& x, bool rows = true) {
  TORCH_CHECK(x.is_cuda() && x.is_contiguous(), op, ": lead tensor must be a contiguous GPU tensor");
  TORCH_CHECK(x.scalar_type() == at::kFloat || x.scalar_type() == at::kBFloat16, op,
              ": unsupported dtype ", x.scalar_type());
  // the row kernels divide by the last dimension; the flat elementwise ones
  // (rows = false) take any shape, an empty one included
  TORCH_CHECK(!rows || (x.dim() >= 1 && x.size(-1) > 0), op,
              ": needs a non-empty last dimension");
}

static void tk_arg(const char* op, const char* name, const at::Tensor& t, const at::Tensor& lead,
                   at::ScalarType dt, at::IntArrayRef shape) {
  TORCH_CHECK(t.is_cuda() && t.device() == lead.device(), op, ": ", name,
              " must be on the lead tensor's GPU");
  TORCH_CHECK(t.scalar_type() == dt, op, ": ", name, " must have dtype ", dt, ", got ",
              t.scalar_type());
  TORCH_CHECK(t.is_contiguous(), op, ": ", name, " must be contiguous");
  TORCH_CHECK(t.sizes() == shape, op, ": ", name, " must have shape ", shape, ", got ",
              t.sizes());
}

std::vector<at::Tensor> layernorm_fwd(at::Tensor x, at::Tensor gamma, at::Tensor beta,
                                      double eps) {
  tk_lead("layernorm_fwd", x);
  const int D = x.size(-1);
  const long N = x.numel() / D;
  tk_arg("layernorm_fwd", "gamma", gamma, x, at::kFloat, {D});
  tk_arg("layernorm_fwd", "beta", beta, x, at::kFloat, {D});
  auto y = at::empty_like(x);
  auto mean = at::empty({N}, x.options().dtype(at::kFloat));
  auto rstd = at::empty({N}, x.options().dtype(at::kFloat));
  dispatch_float_bf16(x, "layernorm_fwd", [&](auto tag) {
    using T = decltype(tag);
    launch_layernorm_fwd<T>(ptr<T>(x), gamma.data_ptr<float>(), beta.data_ptr<float>(),
                            mptr<T>(y), mean.data_ptr<float>(), rstd.data_ptr<float>(), N, D,
                            (float)eps, cur_stream());
  });
  return {y, mean, rstd};
}

at::Tensor layernorm_bwd(at::Tensor dy, at::Tensor x, at::Tensor gamma, at::Tensor mean,
                         at::Tensor rstd) {
  tk_lead("layernorm_bwd", x);
  const int D = x.size(-1);
  const long N = x.numel() / D;
  tk_arg("layernorm_bwd", "dy", dy, x, x.scalar_type(), x.sizes());
  tk_arg("layernorm_bwd", "gamma", gamma, x, at::kFloat, {D});
  tk_arg("layernorm_bwd", "mean", mean, x, at::kFloat, {N});
  tk_arg("layernorm_bwd", "rstd", rstd, x, at::kFloat, {N});
  auto dx = at::empty_like(x);
  dispatch_float_bf16(x, "layernorm_bwd", [&](auto tag) {
    using T = decltype(tag);
    launch_layernorm_bwd<T>(ptr<T>(dy), ptr<T>(x), gamma.data_ptr<float>(),
                            mean.data_ptr<float>(), rstd.data_ptr<float>(), mptr<T>(dx), N, D,
                            cur_stream());
  });
  return dx;
}

std::vector<at::Tensor> layernorm_wgrad(at::Tensor dy, at::Tensor x, at::Tensor mean,
                                        at::Tensor rstd) {
  tk_lead("layernorm_wgrad", x);
  const int D = x.size(-1);
  const long N = x.numel() / D;
  tk_arg("layernorm_wgrad", "dy", dy, x, x.scalar_type(), x.sizes());
  tk_arg("layernorm_wgrad", "mean", mean, x, at::kFloat, {N});
  tk_arg("layernorm_wgrad", "rstd", rstd, x, at::kFloat, {N});
  auto dgamma = at::zeros({D}, x.options().dtype(at::kFloat));
  auto dbeta = at::zeros({D}, x.options().dtype(at::kFloat));
  dispatch_float_bf16(x, "layernorm_wgrad", [&](auto tag) {
    using T = decltype(tag);
    launch_layernorm_wgrad<T>(ptr<T>(dy), ptr<T>(x), mean.data_ptr<float>(),
                              rstd.data_ptr<float>(), dgamma.data_ptr<float>(),
                              dbeta.data_ptr<float>(), N, D, cur_stream());
  });
  return {dgamma, dbeta};
}

// D: a multiple of the 16-B vector, and the fp32 bias row must fit in LDS
static int check_bias_gelu_geom(const char* op, const at::Tensor& x, const at::Tensor& bias) {
  tk_lead(op, x);
  const int D = x.size(-1);
  TORCH_CHECK(D % (x.scalar_type() == at::kFloat ? 4 : 8) == 0, op,
              ": D must be a multiple of the 16-B vector width");
  TORCH_CHECK((size_t)D * sizeof(float) <= kLdsLimit, op, ": D = ", D,
              " exceeds the LDS-staged bias row (", kLdsLimit / sizeof(float), ")");
  tk_arg(op, "bias", bias, x, at::kFloat, {D});
  return D;
}

at::Tensor bias_gelu_fwd(at::Tensor x, at::Tensor bias) {
  const int D = check_bias_gelu_geom("bias_gelu_fwd", x, bias);
  auto y = at::empty_like(x);
  dispatch_float_bf16(x, "bias_gelu_fwd", [&](auto tag) {
    using T = decltype(tag);
    launch_bias_gelu_fwd<T>(ptr<T>(x), bias.data_ptr<float>(), mptr<T>(y), x.numel(), D,
                            cur_stream());
  });
  return y;
}

at::Tensor bias_gelu_bwd(at::Tensor dy, at::Tensor x, at::Tensor bias) {
  const int D = check_bias_gelu_geom("bias_gelu_bwd", x, bias);
  tk_arg("bias_gelu_bwd", "dy", dy, x, x.scalar_type(), x.sizes());
  auto dx = at::empty_like(x);
  dispatch_float_bf16(x, "bias_gelu_bwd", [&](auto tag) {
    using T = decltype(tag);
    launch_bias_gelu_bwd<T>(ptr<T>(dy), ptr<T>(x), bias.data_ptr<float>(), mptr<T>(dx),
                            x.numel(), D, cur_stream());
  });
  return dx;
}

static void check_softmax_geom(const at::Tensor& t, int L) {
  const int vec = t.scalar_type() == at::kBFloat16 ? 8 : 4;
  TORCH_CHECK(L % vec == 0 && L <= 64 * vec * 4, "unsupported softmax row length ", L);
}

// returns {P (pre-dropout, saved for bwd), Pd (post-dropout, feeds P@V)};
// Pd aliases P when dropout_p == 0
std::vector<at::Tensor> softmax_mask_fwd(at::Tensor S, c10::optional<at::Tensor> valid,
                                         double scale, double dropout_p, int64_t seed,
                                         bool causal) {
  tk_lead("softmax_mask_fwd", S);
  TORCH_CHECK(S.dim() >= 2, "softmax_mask_fwd: S must be (..., Lq, L)");
  const int L = S.size(-1);
  const long R = S.numel() / L;
  check_softmax_geom(S, L);
  auto P = at::empty_like(S);
  const bool drop = dropout_p > 0.0;
  // p == 0: Pd shares storage with P via an explicit alias so autograd can
  // keep the two outputs' differentiability separate
  auto Pd = drop ? at::empty_like(S) : at::alias(P);
  const int* vptr = nullptr;
  int rows_per_batch = 1;
  if (valid.has_value()) {
    const long nb = valid->numel();
    TORCH_CHECK(valid->dim() == 1 && nb > 0 && R % nb == 0,
                "softmax_mask_fwd: valid must be 1-D and its length must divide the ", R,
                " rows");
    tk_arg("softmax_mask_fwd", "valid", *valid, S, at::kInt, {nb});
    vptr = valid->data_ptr<int>();
    rows_per_batch = (int)(R / nb);
  }
  dispatch_float_bf16(S, "softmax_mask_fwd", [&](auto tag) {
    using T = decltype(tag);
    launch_softmax_mask_fwd<T>(ptr<T>(S), vptr, mptr<T>(P), drop ? mptr<T>(Pd) : nullptr, R, L,
                               rows_per_batch, (float)scale, (float)dropout_p,
                               (unsigned long long)seed, causal ? 1 : 0, (int)S.size(-2),
                               cur_stream());
  });
  return {P, Pd};
}

at::Tensor softmax_mask_bwd(at::Tensor dPd, at::Tensor P, double scale, double dropout_p,
                            int64_t seed) {
  tk_lead("softmax_mask_bwd", P);
  tk_arg("softmax_mask_bwd", "dPd", dPd, P, P.scalar_type(), P.sizes());
  const int L = P.size(-1);
  const long R = P.numel() / L;
  check_softmax_geom(P, L);
  auto dS = at::empty_like(P);
  dispatch_float_bf16(P, "softmax_mask_bwd", [&](auto tag) {
    using T = decltype(tag);
    launch_softmax_mask_bwd<T>(ptr<T>(dPd), ptr<T>(P), mptr<T>(dS), R, L, (float)scale,
                               (float)dropout_p, (unsigned long long)seed, cur_stream());
  });
  return dS;
}


std::vector<at::Tensor> rmsnorm_fwd(at::Tensor x, at::Tensor gamma, double eps) {
  tk_lead("rmsnorm_fwd", x);
  const int D = x.size(-1);
  const long N = x.numel() / D;
  tk_arg("rmsnorm_fwd", "gamma", gamma, x, at::kFloat, {D});
  auto y = at::empty_like(x);
  auto rstd = at::empty({N}, x.options().dtype(at::kFloat));
  dispatch_float_bf16(x, "rmsnorm_fwd", [&](auto tag) {
    using T = decltype(tag);
    launch_rmsnorm_fwd<T>(ptr<T>(x), gamma.data_ptr<float>(), mptr<T>(y),
                          rstd.data_ptr<float>(), N, D, (float)eps, cur_stream());
  });
  return {y, rstd};
}

at::Tensor rmsnorm_bwd(at::Tensor dy, at::Tensor x, at::Tensor gamma, at::Tensor rstd) {
  tk_lead("rmsnorm_bwd", x);
  const int D = x.size(-1);
  const long N = x.numel() / D;
  tk_arg("rmsnorm_bwd", "dy", dy, x, x.scalar_type(), x.sizes());
  tk_arg("rmsnorm_bwd", "gamma", gamma, x, at::kFloat, {D});
  tk_arg("rmsnorm_bwd", "rstd", rstd, x, at::kFloat, {N});
  auto dx = at::empty_like(x);
  dispatch_float_bf16(x, "rmsnorm_bwd", [&](auto tag) {
    using T = decltype(tag);
    launch_rmsnorm_bwd<T>(ptr<T>(dy), ptr<T>(x), gamma.data_ptr<float>(),
                          rstd.data_ptr<float>(), mptr<T>(dx), N, D, cur_stream());
  });
  return dx;
}

at::Tensor rmsnorm_wgrad(at::Tensor dy, at::Tensor x, at::Tensor rstd,
                         c10::optional<at::Tensor> out_opt) {
  tk_lead("rmsnorm_wgrad", x);
  const int D = x.size(-1);
  const long N = x.numel() / D;
  tk_arg("rmsnorm_wgrad", "dy", dy, x, x.scalar_type(), x.sizes());
  tk_arg("rmsnorm_wgrad", "rstd", rstd, x, at::kFloat, {N});
  auto dgamma = acc_or_zeros(out_opt, {D}, x.options(), "rmsnorm_wgrad");
  dispatch_float_bf16(x, "rmsnorm_wgrad", [&](auto tag) {
    using T = decltype(tag);
    launch_rmsnorm_wgrad<T>(ptr<T>(dy), ptr<T>(x), rstd.data_ptr<float>(),
                            dgamma.data_ptr<float>(), N, D, cur_stream());
  });
  return dgamma;
}


// ---------------------------------------------------------------------------
// Flash attention (csrc/flash_attn.hip): head_dim 64, (B, L, H*64) layout
// ---------------------------------------------------------------------------

static const int* opt_valid_ptr(const c10::optional<at::Tensor>& valid) {
  if (!valid.has_value()) return nullptr;
  TORCH_CHECK(valid->scalar_type() == at::kInt && valid->is_contiguous());
  return valid->data_ptr<int>();
}

// Q/K/V may be row-strided views (slices of a fused QKV projection):
// last dim contiguous, batch stride == L * row stride
static long fa_ld(const at::Tensor& t, int L) {
  TORCH_CHECK(t.is_cuda() && t.dim() == 3 && t.stride(2) == 1 &&
                  t.stride(0) == (long)L * t.stride(1) && t.stride(1) >= t.size(2),
              "flash tensor must be a (B, L, D) row-strided view");
  return t.stride(1);
}

std::vector<at::Tensor> flash_attn_fwd(at::Tensor Q, at::Tensor K, at::Tensor V, int64_t H,
                                       c10::optional<at::Tensor> valid,
                                       c10::optional<at::Tensor> bias, double scale, bool causal,
                                       double dropout_p, int64_t seed) {
  TORCH_CHECK(Q.scalar_type() == at::kBFloat16, "flash attention is bf16");
  const int B = Q.size(0), L = Q.size(1);
  const long ldq = fa_ld(Q, L);
  const long ldkv = fa_ld(K, L);
  TORCH_CHECK(fa_ld(V, L) == ldkv, "K and V must share a row stride");
  TORCH_CHECK(Q.size(2) == H * 64, "head_dim must be 64");
  TORCH_CHECK(L % 64 == 0, "L must be a multiple of 64");
  auto O = at::empty({B, L, H * 64}, Q.options());
  auto lse = at::empty({B, H, L}, Q.options().dtype(at::kFloat));
  const float* bptr = nullptr;
  if (bias.has_value()) {
    TORCH_CHECK(bias->scalar_type() == at::kFloat && bias->is_contiguous());
    TORCH_CHECK(bias->numel() == H * (long)L * L, "bias must be (H, L, L)");
    bptr = bias->data_ptr<float>();
  }
  launch_flash_fwd(ptr<bf16_t>(Q), ptr<bf16_t>(K), ptr<bf16_t>(V), opt_valid_ptr(valid), bptr,
                   mptr<bf16_t>(O), lse.data_ptr<float>(), B, H, L, (float)scale, causal ? 1 : 0,
                   (unsigned)(dropout_p * 256.0), (unsigned long long)seed, ldq, ldkv,
                   cur_stream());
  return {O, lse};
}

// Attention received R[b, h, j] = sum_i P[b, h, i, j] from the forward's lse
// (flash_received_kernel): fp32 (B, H, L), every element written
at::Tensor flash_attn_received(at::Tensor Q, at::Tensor K, at::Tensor lse, int64_t H,
                               c10::optional<at::Tensor> valid,
                               c10::optional<at::Tensor> bias, double scale, bool causal) {
  TORCH_CHECK(Q.scalar_type() == at::kBFloat16 && K.scalar_type() == at::kBFloat16,
              "flash attention is bf16");
  const int B = Q.size(0), L = Q.size(1);
  const long ldq = fa_ld(Q, L);
  const long ldkv = fa_ld(K, L);
  TORCH_CHECK(K.device() == Q.device() && K.size(0) == B && K.size(1) == L &&
                  K.size(2) == Q.size(2),
              "Q and K must have the same shape and device");
  TORCH_CHECK(Q.size(2) == H * 64, "head_dim must be 64");
  TORCH_CHECK(L % 64 == 0, "L must be a multiple of 64");
  TORCH_CHECK(lse.scalar_type() == at::kFloat && lse.is_contiguous() &&
                  lse.device() == Q.device() && lse.dim() == 3 && lse.size(0) == B &&
                  lse.size(1) == H && lse.size(2) == L,
              "lse must be a contiguous fp32 (B, H, L) tensor on Q's device");
  if (valid.has_value())
    TORCH_CHECK(valid->device() == Q.device() && valid->numel() == B,
                "valid must hold B lengths on Q's device");
  const float* bptr = nullptr;
  if (bias.has_value()) {
    TORCH_CHECK(bias->scalar_type() == at::kFloat && bias->is_contiguous() &&
                bias->device() == Q.device());
    TORCH_CHECK(bias->numel() == H * (long)L * L, "bias must be (H, L, L)");
    bptr = bias->data_ptr<float>();
  }
  auto R = at::empty({B, H, L}, Q.options().dtype(at::kFloat));
  if (R.numel() == 0) return R;
  launch_flash_received(ptr<bf16_t>(Q), ptr<bf16_t>(K), opt_valid_ptr(valid), bptr,
                        lse.data_ptr<float>(), R.data_ptr<float>(), B, H, L, (float)scale,
                        causal ? 1 : 0, ldq, ldkv, cur_stream());
  return R;
}

// ---------------------------------------------------------------------------
// Decode attention (csrc/decode_attn.hip): one query row per sequence
// ---------------------------------------------------------------------------

// (R, H*64) bf16 row-strided view (a slice of a fused projection): last dim
// contiguous, rows 16-B aligned. Returns the row stride.
static long da_rows(const char* name, const at::Tensor& t, long R, int64_t H,
                    const at::Tensor& like) {
  TORCH_CHECK(t.is_cuda() && t.device() == like.device() && t.scalar_type() == at::kBFloat16,
              name, " must be a bf16 tensor on q's device");
  TORCH_CHECK(t.dim() == 2 && t.size(0) == R && t.size(1) == H * 64, name,
              " must be (R, H*64) with head_dim 64");
  TORCH_CHECK(t.stride(1) == 1 && (R == 1 || t.stride(0) >= t.size(1)) && t.stride(0) % 8 == 0 &&
                  reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0,
              name, " must be a row-strided view with 16-B aligned rows");
  return t.stride(0);
}

// Stores k_new / v_new into cache[r, pos] and returns the attention output of
// the new token over keys 0..pos, (R, H*64) bf16, every element written.
at::Tensor decode_self_attn(at::Tensor q, at::Tensor k_new, at::Tensor v_new, at::Tensor k_cache,
                            at::Tensor v_cache, c10::optional<at::Tensor> anc,
                            c10::optional<at::Tensor> bias_dist, int64_t pos, int64_t H,
                            double scale) {
  TORCH_CHECK(H >= 1 && H <= 65535, "decode_self_attn: bad head count");
  TORCH_CHECK(q.dim() == 2, "decode_self_attn: q must be (R, H*64)");
  const long R = q.size(0);
  const long ldq = da_rows("decode_self_attn: q", q, R, H, q);
  const long ldk = da_rows("decode_self_attn: k_new", k_new, R, H, q);
  const long ldv = da_rows("decode_self_attn: v_new", v_new, R, H, q);
  for (const at::Tensor* c : {&k_cache, &v_cache})
    TORCH_CHECK(c->is_cuda() && c->device() == q.device() && c->scalar_type() == at::kBFloat16 &&
                    c->is_contiguous() && c->dim() == 3 && c->size(0) == R &&
                    c->size(2) == H * 64 && c->size(1) == k_cache.size(1),
                "decode_self_attn: caches must be contiguous bf16 (R, Tmax, H*64) on q's device");
  const long Tmax = k_cache.size(1);
  TORCH_CHECK(pos >= 0 && pos < Tmax, "decode_self_attn: pos must be in [0, Tmax)");
  TORCH_CHECK(Tmax <= 8192, "decode_self_attn: Tmax above 8192");
  const int* aptr = nullptr;
  if (anc.has_value()) {
    TORCH_CHECK(anc->is_cuda() && anc->device() == q.device() && anc->scalar_type() == at::kInt &&
                    anc->is_contiguous() && anc->dim() == 2 && anc->size(0) == R &&
                    anc->size(1) == Tmax,
                "decode_self_attn: anc must be a contiguous int32 (R, Tmax) tensor on q's device");
    aptr = anc->data_ptr<int>();
  }
  const float* bptr = nullptr;
  if (bias_dist.has_value()) {
    TORCH_CHECK(bias_dist->is_cuda() && bias_dist->device() == q.device() &&
                    bias_dist->scalar_type() == at::kFloat && bias_dist->is_contiguous() &&
                    bias_dist->dim() == 2 && bias_dist->size(0) == H &&
                    bias_dist->size(1) == Tmax,
                "decode_self_attn: bias_dist must be a contiguous fp32 (H, Tmax) tensor");
    bptr = bias_dist->data_ptr<float>();
  }
  auto out = at::empty({R, H * 64}, q.options());
  if (R == 0) return out;
  launch_decode_self(ptr<bf16_t>(q), ptr<bf16_t>(k_new), ptr<bf16_t>(v_new),
                     mptr<bf16_t>(k_cache), mptr<bf16_t>(v_cache), aptr, bptr, mptr<bf16_t>(out),
                     R, (int)Tmax, (int)pos, (int)H, (float)scale, ldq, ldk, ldv, cur_stream());
  return out;
}

// (B, Lk, H*64) bf16 view of a fused K/V buffer: last dim contiguous, 16-B
// aligned rows, any batch stride
static void da_kv(const char* name, const at::Tensor& t, int64_t H, const at::Tensor& like) {
  TORCH_CHECK(t.is_cuda() && t.device() == like.device() && t.scalar_type() == at::kBFloat16,
              name, " must be a bf16 tensor on q's device");
  TORCH_CHECK(t.dim() == 3 && t.size(2) == H * 64, name, " must be (B, Lk, H*64)");
  TORCH_CHECK(t.stride(2) == 1 && t.stride(1) >= t.size(2) && t.stride(1) % 8 == 0 &&
                  t.stride(0) % 8 == 0 && t.stride(0) >= 0 &&
                  reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0,
              name, " must be a row-strided view with 16-B aligned rows");
}

// Row r = b * beams + i attends over source b's keys < valid[b]; (R, H*64)
// bf16, every element written (exact zeros where valid[b] == 0).
at::Tensor decode_cross_attn(at::Tensor q, at::Tensor k, at::Tensor v,
                             c10::optional<at::Tensor> valid, int64_t beams, int64_t H,
                             double scale) {
  TORCH_CHECK(H >= 1 && H <= 65535, "decode_cross_attn: bad head count");
  TORCH_CHECK(q.dim() == 2, "decode_cross_attn: q must be (R, H*64)");
  const long R = q.size(0);
  const long ldq = da_rows("decode_cross_attn: q", q, R, H, q);
  da_kv("decode_cross_attn: k", k, H, q);
  da_kv("decode_cross_attn: v", v, H, q);
  const long B = k.size(0), Lk = k.size(1);
  TORCH_CHECK(v.size(0) == B && v.size(1) == Lk, "decode_cross_attn: k and v shapes differ");
  TORCH_CHECK(beams >= 1 && R == B * beams, "decode_cross_attn: R must be B * beams");
  TORCH_CHECK(Lk >= 1 && decode_cross_lds_bytes((int)std::min<long>(Lk, 1 << 20)) <= 65536,
              "decode_cross_attn: Lk must be in [1, 768]");
  const int* vptr = nullptr;
  if (valid.has_value()) {
    TORCH_CHECK(valid->is_cuda() && valid->device() == q.device() &&
                    valid->scalar_type() == at::kInt && valid->is_contiguous() &&
                    valid->numel() == B,
                "decode_cross_attn: valid must hold B int32 lengths on q's device");
    vptr = valid->data_ptr<int>();
  }
  auto out = at::empty({R, H * 64}, q.options());
  if (R == 0) return out;
  launch_decode_cross(ptr<bf16_t>(q), ptr<bf16_t>(k), ptr<bf16_t>(v), vptr, mptr<bf16_t>(out),
                      (int)B, (int)Lk, (int)beams, (int)H, (float)scale, ldq, k.stride(1),
                      v.stride(1), k.stride(0), v.stride(0), cur_stream());
  return out;
}

std::vector<at::Tensor> flash_attn_bwd(at::Tensor dO, at::Tensor Q, at::Tensor K, at::Tensor V,
                                       at::Tensor O, at::Tensor lse, int64_t H,
                                       c10::optional<at::Tensor> valid,
                                       c10::optional<at::Tensor> bias, double scale, bool causal,
                                       double dropout_p, int64_t seed, bool need_dbias,
                                       bool fused_grads,
                                       c10::optional<at::Tensor> dbias_accum = c10::nullopt,
                                       bool kv_fused = false) {
  CHECK_GPU(dO);
  const int B = Q.size(0), L = Q.size(1);
  const long ldq = fa_ld(Q, L);
  const long ldkv = fa_ld(K, L);
  TORCH_CHECK(fa_ld(V, L) == ldkv, "K and V must share a row stride");
  auto stream = cur_stream();
  auto Dterm = at::empty({B, H, L}, Q.options().dtype(at::kFloat));
  launch_flash_dterm(ptr<bf16_t>(dO), ptr<bf16_t>(O), Dterm.data_ptr<float>(), B, H, L, stream);
  // fused_grads: one (B, L, 3*H*64) buffer whose [q|k|v] slices the
  // kernels write directly (ld 3*H*64) — lets the attention op consume a
  // fused QKV projection with zero slice-backward scatter work
  const long HD64 = (long)H * 64;
  at::Tensor dQKV, dKV, dQ, dK, dV;
  long ld_dq = HD64, ld_dkv = HD64;
  if (fused_grads) {
    TORCH_CHECK(ldq == 3 * HD64 && ldkv == 3 * HD64,
                "fused_grads expects q/k/v slices of one (B, L, 3D) buffer");
    dQKV = at::empty({B, L, 3 * HD64}, Q.options());
    ld_dq = ld_dkv = 3 * HD64;
    dQ = dQKV.narrow(2, 0, HD64);
    dK = dQKV.narrow(2, HD64, HD64);
    dV = dQKV.narrow(2, 2 * HD64, HD64);
  } else if (kv_fused) {
    // cross-attention: dense dQ, dK/dV written as the [k|v] slices of one
    // (B, L, 2D) buffer matching a fused K/V projection of the encoder
    TORCH_CHECK(ldkv == 2 * HD64,
                "kv_fused expects k/v slices of one (B, L, 2D) buffer");
    dQ = at::empty({B, L, HD64}, Q.options());
    dKV = at::empty({B, L, 2 * HD64}, Q.options());
    ld_dkv = 2 * HD64;
    dK = dKV.narrow(2, 0, HD64);
    dV = dKV.narrow(2, HD64, HD64);
  } else {
    dQ = at::empty({B, L, HD64}, Q.options());
    dK = at::empty({B, L, HD64}, Q.options());
    dV = at::empty({B, L, HD64}, Q.options());
  }
  const float* bptr = nullptr;
  if (bias.has_value()) bptr = bias->data_ptr<float>();
  at::Tensor dBias;
  float* dbias_ptr = nullptr;
  if (dbias_accum.has_value()) {
    // shared accumulation buffer (T5: 24 layers share one position bias;
    // the dq kernel's atomics land in ONE tensor instead of 24 separate
    // dBias allocations + the autograd fan-in adds)
    TORCH_CHECK(dbias_accum->scalar_type() == at::kFloat &&
                dbias_accum->numel() == (long)H * L * L);
    dbias_ptr = dbias_accum->data_ptr<float>();
  } else if (need_dbias) {
    TORCH_CHECK(bias.has_value());
    dBias = at::zeros({H, L, L}, Q.options().dtype(at::kFloat));
    dbias_ptr = dBias.data_ptr<float>();
  }
  launch_flash_dq(ptr<bf16_t>(Q), ptr<bf16_t>(K), ptr<bf16_t>(V), ptr<bf16_t>(dO),
                  opt_valid_ptr(valid), bptr, lse.data_ptr<float>(), Dterm.data_ptr<float>(),
                  mptr<bf16_t>(dQ), dbias_ptr, B, H, L, (float)scale, causal ? 1 : 0,
                  (unsigned)(dropout_p * 256.0), (unsigned long long)seed, ldq, ldkv, ld_dq,
                  stream);
  launch_flash_dkv(ptr<bf16_t>(Q), ptr<bf16_t>(K), ptr<bf16_t>(V), ptr<bf16_t>(dO),
                   opt_valid_ptr(valid), bptr, lse.data_ptr<float>(), Dterm.data_ptr<float>(),
                   mptr<bf16_t>(dK), mptr<bf16_t>(dV), B, H, L, (float)scale,
                   causal ? 1 : 0, (unsigned)(dropout_p * 256.0), (unsigned long long)seed,
                   ldq, ldkv, ld_dkv, stream);
  if (fused_grads) {
    if (need_dbias && !dbias_accum.has_value()) return {dQKV, dBias};
    return {dQKV};
  }
  if (kv_fused) {
    if (need_dbias && !dbias_accum.has_value()) return {dQ, dKV, dBias};
    return {dQ, dKV};
  }
  if (need_dbias && !dbias_accum.has_value()) return {dQ, dK, dV, dBias};
  return {dQ, dK, dV};
}

// ---------------------------------------------------------------------------
// General flash attention (csrc/flash_rect.hip): any Lq >= 1, Lk >= 1
// ---------------------------------------------------------------------------

struct FlashRectArgs {
  int B, Lq, Lk;
  long ldq, ldkv;
  const int* valid;
  const float* bias;
};

// Shape, dtype and layout checks shared by flash_rect_fwd / flash_rect_bwd.
// Argument-shape errors come before the device checks.
static FlashRectArgs flash_rect_check(const char* fn, const at::Tensor& Q, const at::Tensor& K,
                                      const at::Tensor& V, int64_t H,
                                      const c10::optional<at::Tensor>& valid,
                                      const c10::optional<at::Tensor>& bias, bool causal,
                                      double dropout_p) {
  TORCH_CHECK(Q.scalar_type() == at::kBFloat16 && K.scalar_type() == at::kBFloat16 &&
                  V.scalar_type() == at::kBFloat16,
              fn, ": Q, K and V must be bf16");
  TORCH_CHECK(Q.dim() == 3 && K.dim() == 3 && V.dim() == 3, fn,
              ": Q must be (B, Lq, H*64), K and V (B, Lk, H*64)");
  TORCH_CHECK(H >= 1 && Q.size(2) == H * 64 && K.size(2) == H * 64, fn,
              ": head_dim must be 64");
  TORCH_CHECK(K.sizes() == V.sizes() && K.stride(1) == V.stride(1), fn,
              ": K and V must have the same shape and row stride");
  FlashRectArgs a;
  TORCH_CHECK(K.size(0) == Q.size(0), fn, ": Q and K differ in batch size");
  TORCH_CHECK(Q.size(1) >= 1 && K.size(1) >= 1 && Q.size(1) < (1 << 30) && K.size(1) < (1 << 30),
              fn, ": Lq and Lk must be >= 1");
  a.B = Q.size(0);
  a.Lq = Q.size(1);
  a.Lk = K.size(1);
  TORCH_CHECK((long)a.B * H <= 65535, fn, ": B*H must not exceed 65535");
  TORCH_CHECK(!causal || a.Lq == a.Lk, fn, ": causal needs Lq == Lk");
  TORCH_CHECK(!bias.has_value() || a.Lq == a.Lk, fn, ": bias needs Lq == Lk");
  TORCH_CHECK(dropout_p >= 0.0 && dropout_p < 1.0, fn, ": dropout_p must be in [0, 1)");
  a.bias = nullptr;
  if (bias.has_value()) {
    TORCH_CHECK(bias->scalar_type() == at::kFloat && bias->is_contiguous(), fn,
                ": bias must be contiguous fp32");
    TORCH_CHECK(bias->numel() == H * (long)a.Lk * a.Lq, fn,
                ": bias must be key-major (H, Lk, Lq)");
  }
  a.valid = nullptr;
  if (valid.has_value())
    TORCH_CHECK(valid->scalar_type() == at::kInt && valid->is_contiguous() &&
                    valid->numel() == a.B,
                fn, ": valid must be a contiguous int32 tensor of B lengths");
  for (const at::Tensor* t : {&Q, &K, &V})
    TORCH_CHECK(t->stride(2) == 1 && t->stride(1) >= t->size(2) && t->stride(1) % 8 == 0 &&
                    (t->size(0) == 1 || t->stride(0) == t->size(1) * t->stride(1)),
                fn, ": flash tensor must be a (B, L, D) row-strided view");
  TORCH_CHECK(Q.is_cuda() && K.device() == Q.device() && V.device() == Q.device(), fn,
              ": Q, K and V must be on one GPU");
  for (const at::Tensor* t : {&Q, &K, &V})
    TORCH_CHECK(reinterpret_cast<uintptr_t>(t->data_ptr()) % 16 == 0, fn,
                ": flash tensor rows must be 16-B aligned");
  if (bias.has_value()) {
    TORCH_CHECK(bias->device() == Q.device(), fn, ": bias must be on Q's device");
    a.bias = bias->data_ptr<float>();
  }
  if (valid.has_value()) {
    TORCH_CHECK(valid->device() == Q.device(), fn, ": valid must be on Q's device");
    a.valid = valid->data_ptr<int>();
  }
  a.ldq = Q.stride(1);
  a.ldkv = K.stride(1);
  return a;
}

// [O (B, Lq, H*64) bf16, lse (B, H, Lq) fp32], every element written
std::vector<at::Tensor> flash_rect_fwd(at::Tensor Q, at::Tensor K, at::Tensor V, int64_t H,
                                       c10::optional<at::Tensor> valid,
                                       c10::optional<at::Tensor> bias, double scale, bool causal,
                                       double dropout_p, int64_t seed) {
  const FlashRectArgs a =
      flash_rect_check("flash_rect_fwd", Q, K, V, H, valid, bias, causal, dropout_p);
  auto O = at::empty({a.B, a.Lq, H * 64}, Q.options());
  auto lse = at::empty({a.B, H, a.Lq}, Q.options().dtype(at::kFloat));
  if (a.B == 0) return {O, lse};
  launch_flash_rect_fwd(ptr<bf16_t>(Q), ptr<bf16_t>(K), ptr<bf16_t>(V), a.valid, a.bias,
                        mptr<bf16_t>(O), lse.data_ptr<float>(), a.B, (int)H, a.Lq, a.Lk,
                        (float)scale, causal ? 1 : 0, (unsigned)(dropout_p * 256.0),
                        (unsigned long long)seed, a.ldq, a.ldkv, cur_stream());
  return {O, lse};
}

// [dQ, dK, dV, (dBias)], or with kv_fused [dQ, dKV (B, Lk, 2*H*64)]; every
// element written, dK/dV rows of keys >= valid[b] exact zeros. dBias (fp32
// atomics) goes into dbias_accum when given, else into a fresh (H, L, L).
std::vector<at::Tensor> flash_rect_bwd(at::Tensor dO, at::Tensor Q, at::Tensor K, at::Tensor V,
                                       at::Tensor O, at::Tensor lse, int64_t H,
                                       c10::optional<at::Tensor> valid,
                                       c10::optional<at::Tensor> bias, double scale, bool causal,
                                       double dropout_p, int64_t seed, bool need_dbias,
                                       c10::optional<at::Tensor> dbias_accum = c10::nullopt,
                                       bool kv_fused = false) {
  const FlashRectArgs a =
      flash_rect_check("flash_rect_bwd", Q, K, V, H, valid, bias, causal, dropout_p);
  const long HD64 = (long)H * 64;
  for (const at::Tensor* t : {&dO, &O})
    TORCH_CHECK(t->scalar_type() == at::kBFloat16 && t->is_contiguous() &&
                    t->device() == Q.device() && t->dim() == 3 && t->size(0) == a.B &&
                    t->size(1) == a.Lq && t->size(2) == HD64,
                "flash_rect_bwd: dO and O must be contiguous bf16 (B, Lq, H*64) on Q's device");
  TORCH_CHECK(lse.scalar_type() == at::kFloat && lse.is_contiguous() &&
                  lse.device() == Q.device() && lse.dim() == 3 && lse.size(0) == a.B &&
                  lse.size(1) == H && lse.size(2) == a.Lq,
              "flash_rect_bwd: lse must be a contiguous fp32 (B, H, Lq) tensor on Q's device");
  TORCH_CHECK(!kv_fused || a.ldkv == 2 * HD64,
              "flash_rect_bwd: kv_fused expects k/v slices of one (B, Lk, 2D) buffer");
  float* dbias_ptr = nullptr;
  at::Tensor dBias;
  if (dbias_accum.has_value()) {
    TORCH_CHECK(bias.has_value(), "flash_rect_bwd: dbias_accum without a bias");
    TORCH_CHECK(dbias_accum->scalar_type() == at::kFloat && dbias_accum->is_contiguous() &&
                    dbias_accum->device() == Q.device() &&
                    dbias_accum->numel() == H * (long)a.Lk * a.Lq,
                "flash_rect_bwd: dbias_accum must be a contiguous fp32 (H, Lk, Lq) tensor");
    dbias_ptr = dbias_accum->data_ptr<float>();
  } else if (need_dbias) {
    TORCH_CHECK(bias.has_value(), "flash_rect_bwd: need_dbias without a bias");
    dBias = at::zeros({H, (long)a.Lk, (long)a.Lq}, Q.options().dtype(at::kFloat));
    dbias_ptr = dBias.data_ptr<float>();
  }
  auto stream = cur_stream();
  at::Tensor dKV, dK, dV;
  auto dQ = at::empty({a.B, a.Lq, HD64}, Q.options());
  long ld_dkv = HD64;
  if (kv_fused) {
    dKV = at::empty({a.B, a.Lk, 2 * HD64}, Q.options());
    ld_dkv = 2 * HD64;
    dK = dKV.narrow(2, 0, HD64);
    dV = dKV.narrow(2, HD64, HD64);
  } else {
    dK = at::empty({a.B, a.Lk, HD64}, Q.options());
    dV = at::empty({a.B, a.Lk, HD64}, Q.options());
  }
  if (a.B > 0) {
    auto Dterm = at::empty({a.B, H, a.Lq}, Q.options().dtype(at::kFloat));
    launch_flash_dterm(ptr<bf16_t>(dO), ptr<bf16_t>(O), Dterm.data_ptr<float>(), a.B, (int)H,
                       a.Lq, stream);
    const unsigned p8 = (unsigned)(dropout_p * 256.0);
    launch_flash_rect_dq(ptr<bf16_t>(Q), ptr<bf16_t>(K), ptr<bf16_t>(V), ptr<bf16_t>(dO), a.valid,
                         a.bias, lse.data_ptr<float>(), Dterm.data_ptr<float>(),
                         mptr<bf16_t>(dQ), dbias_ptr, a.B, (int)H, a.Lq, a.Lk, (float)scale,
                         causal ? 1 : 0, p8, (unsigned long long)seed, a.ldq, a.ldkv, stream);
    launch_flash_rect_dkv(ptr<bf16_t>(Q), ptr<bf16_t>(K), ptr<bf16_t>(V), ptr<bf16_t>(dO),
                          a.valid, a.bias, lse.data_ptr<float>(), Dterm.data_ptr<float>(),
                          mptr<bf16_t>(dK), mptr<bf16_t>(dV), a.B, (int)H, a.Lq, a.Lk,
                          (float)scale, causal ? 1 : 0, p8, (unsigned long long)seed, a.ldq,
                          a.ldkv, ld_dkv, stream);
  }
  const bool ret_dbias = need_dbias && !dbias_accum.has_value();
  if (kv_fused) {
    if (ret_dbias) return {dQ, dKV, dBias};
    return {dQ, dKV};
  }
  if (ret_dbias) return {dQ, dK, dV, dBias};
  return {dQ, dK, dV};
}



// out(N, COL) = A(N, K) @ W(COL, K)^T [+ bias] [+ addend] — transformer
// shapes (csrc/gemm_bf16.hip). Geometry: N%128, K%64, COL%128 == 0.
at::Tensor gemm2(at::Tensor A, at::Tensor W, c10::optional<at::Tensor> bias,
                 c10::optional<at::Tensor> addend) {
  CHECK_GPU(A);
  CHECK_GPU(W);
  TORCH_CHECK(A.scalar_type() == at::kBFloat16 && W.scalar_type() == at::kBFloat16);
  const int N = A.size(0), K = A.size(1), COL = W.size(0);
  TORCH_CHECK(W.size(1) == K && N % 128 == 0 && K % 64 == 0 && COL % 128 == 0,
              "gemm2 geometry violated: ", N, "x", K, "x", COL);
  auto out = at::empty({N, COL}, A.options());
  const float* b = nullptr;
  if (bias.has_value()) {
    TORCH_CHECK(bias->scalar_type() == at::kFloat && bias->is_contiguous());
    b = bias->data_ptr<float>();
  }
  const bf16_t* add = nullptr;
  if (addend.has_value()) add = reinterpret_cast<const bf16_t*>(addend->data_ptr());
  launch_gemm2(ptr<bf16_t>(A), ptr<bf16_t>(W), b, add, mptr<bf16_t>(out), N, K, COL,
               cur_stream());
  return out;
}


void launch_lmhead_ce_fwd(const __hip_bfloat16*, const __hip_bfloat16*, const int*,
                          float, long, int, int, int, float*, float*, float*,
                          float*, float*, int, hipStream_t);
void launch_lmhead_ce_bwd(const __hip_bfloat16*, const __hip_bfloat16*, const int*,
                          const float*, const float*, float, long, int, int, int,
                          __hip_bfloat16*, hipStream_t);

// the operands both lmhead_ce kernels read: h (M,K) bf16, Wp (Vp,K) bf16,
// targets (M,) int32; the kernels index all three without bounds checks
static void check_lmhead_ce(const at::Tensor& h, const at::Tensor& Wp,
                            const at::Tensor& targets, int64_t V) {
  CHECK_GPU(h);
  CHECK_GPU(Wp);
  CHECK_GPU(targets);
  TORCH_CHECK(h.scalar_type() == at::kBFloat16 && Wp.scalar_type() == at::kBFloat16);
  TORCH_CHECK(targets.scalar_type() == at::kInt && targets.is_contiguous());
  TORCH_CHECK(h.dim() == 2 && Wp.dim() == 2);
  const long M = h.size(0), K = h.size(1), Vp = Wp.size(0);
  TORCH_CHECK(Wp.size(1) == K && M % 128 == 0 && K % 64 == 0 && Vp % 128 == 0,
              "lmhead_ce geometry violated: ", M, "x", K, " vocab ", Vp);
  TORCH_CHECK(V > 0 && V <= Vp, "lmhead_ce: V = ", V, " outside (0, Vp = ", Vp, "]");
  TORCH_CHECK(targets.numel() == M);
}

// K21 forward: per-row (loss, lse) of CE(softmax(scale * h @ Wp^T), target)
// without materializing logits. h (M,K) bf16, Wp (Vp,K) bf16 zero-padded
// past V, targets (M,) int32 with -1 = ignore. csrc/lmhead_ce.hip.
std::vector<at::Tensor> lmhead_ce_fwd(at::Tensor h, at::Tensor Wp, at::Tensor targets,
                                      double scale, int64_t V) {
  check_lmhead_ce(h, Wp, targets, V);
  const long M = h.size(0);
  const int K = h.size(1), Vp = Wp.size(0);
  const int n_chunks = (Vp / 128 + 7) / 8;
  auto fopt = h.options().dtype(at::kFloat);
  auto pmax = at::empty({M, n_chunks}, fopt);
  auto psum = at::empty({M, n_chunks}, fopt);
  auto ptgt = at::empty({M, n_chunks}, fopt);
  auto lse = at::empty({M}, fopt);
  auto loss = at::empty({M}, fopt);
  launch_lmhead_ce_fwd(ptr<bf16_t>(h), ptr<bf16_t>(Wp), targets.data_ptr<int>(),
                       (float)scale, M, K, (int)V, Vp, pmax.data_ptr<float>(),
                       psum.data_ptr<float>(), ptgt.data_ptr<float>(),
                       lse.data_ptr<float>(), loss.data_ptr<float>(), n_chunks,
                       cur_stream());
  return {loss, lse};
}

// K21 backward: dlogits (M, Vp) bf16 = (softmax - onehot(target)) * gscale,
// recomputed tile-by-tile (cols >= V zeroed).
at::Tensor lmhead_ce_bwd(at::Tensor h, at::Tensor Wp, at::Tensor targets,
                         at::Tensor lse, at::Tensor gscale, double scale, int64_t V) {
  check_lmhead_ce(h, Wp, targets, V);
  CHECK_GPU(lse);
  CHECK_GPU(gscale);
  const long M = h.size(0);
  const int K = h.size(1), Vp = Wp.size(0);
  TORCH_CHECK(lse.scalar_type() == at::kFloat && gscale.scalar_type() == at::kFloat);
  TORCH_CHECK(lse.numel() == M && gscale.numel() == M);
  auto dlogits = at::empty({M, (long)Vp}, h.options());
  launch_lmhead_ce_bwd(ptr<bf16_t>(h), ptr<bf16_t>(Wp), targets.data_ptr<int>(),
                       lse.data_ptr<float>(), gscale.data_ptr<float>(),
                       (float)scale, M, K, (int)V, Vp,
                       mptr<bf16_t>(dlogits), cur_stream());
  return dlogits;
}

int lmhead_topk_chunk_tiles(long, int);
void launch_lmhead_topk(const __hip_bfloat16*, const __hip_bfloat16*, float, long, int,
                        int, int, int, int, float*, float*, float*, int*, float*,
                        float*, int*, hipStream_t);
void launch_beam_select(const float*, const int*, const float*, const float*, const bool*,
                        long, int, long, long, float*, long*, long*, bool*, hipStream_t);

// Generation LM head: (val, idx, lse) = the k largest of scale * h @ Wp[:V]^T
// per row (value descending, smaller column first among equal values), their
// columns, and the row's logsumexp over the V columns; logits are never
// materialised. h (M, Kd) bf16 with any M >= 0, Wp (Vp, Kd) bf16 padded to a
// multiple of 128 rows (rows >= V are masked). chunk_tiles = 0 lets the
// launcher choose the vocabulary chunk; tests pin it. csrc/lmhead_topk.hip.
std::vector<at::Tensor> lmhead_topk(at::Tensor h, at::Tensor Wp, int64_t V, double scale,
                                    int64_t k, int64_t chunk_tiles) {
  CHECK_GPU(h);
  CHECK_GPU(Wp);
  TORCH_CHECK(h.scalar_type() == at::kBFloat16 && Wp.scalar_type() == at::kBFloat16,
              "lmhead_topk: h and Wp must be bf16");
  TORCH_CHECK(h.dim() == 2 && Wp.dim() == 2, "lmhead_topk: h and Wp must be 2-D");
  const long M = h.size(0), K = h.size(1), Vp = Wp.size(0);
  TORCH_CHECK(Wp.size(1) == K && K > 0 && K % 64 == 0 && Vp % 128 == 0,
              "lmhead_topk geometry violated: ", M, "x", K, " vocab ", Vp, "x", Wp.size(1));
  TORCH_CHECK(V > 0 && V <= Vp && V < (1L << 31),
              "lmhead_topk: V = ", V, " outside (0, Vp = ", Vp, "]");
  TORCH_CHECK(k >= 1 && k <= 16 && k <= V, "lmhead_topk: k = ", k,
              " outside [1, min(16, V)]");
  TORCH_CHECK(chunk_tiles >= 0 && chunk_tiles <= 64,
              "lmhead_topk: chunk_tiles = ", chunk_tiles, " outside [0, 64]");
  auto fopt = h.options().dtype(at::kFloat);
  auto iopt = h.options().dtype(at::kInt);
  auto lse = at::empty({M}, fopt);
  auto val = at::empty({M, k}, fopt);
  auto idx = at::empty({M, k}, iopt);
  if (M == 0) return {val, idx, lse};
  const int n_tiles = (int)((V + 127) / 128);
  const int ct = chunk_tiles > 0 ? (int)chunk_tiles : lmhead_topk_chunk_tiles(M, n_tiles);
  const int n_chunks = (n_tiles + ct - 1) / ct;
  const long P = 2L * n_chunks;
  auto pmax = at::empty({M, P}, fopt);
  auto psum = at::empty({M, P}, fopt);
  auto pval = at::empty({M, P, k}, fopt);
  auto pidx = at::empty({M, P, k}, iopt);
  launch_lmhead_topk(ptr<bf16_t>(h), ptr<bf16_t>(Wp), (float)scale, M, (int)K, (int)V, ct,
                     n_chunks, (int)k, pmax.data_ptr<float>(), psum.data_ptr<float>(),
                     pval.data_ptr<float>(), pidx.data_ptr<int>(), lse.data_ptr<float>(),
                     val.data_ptr<float>(), idx.data_ptr<int>(), cur_stream());
  return {val, idx, lse};
}

// One beam-search selection step over the candidates of lmhead_topk: val, idx
// (B*K, K), lse (B*K,), beam_scores (B, K) fp32, done (B*K,) bool. Returns
// (scores (B, K) fp32, parent (B*K,) int64 flat rows, tok (B*K,) int64,
// done (B*K,) bool). A finished row offers the single candidate fill_token at
// its own score. csrc/lmhead_topk.hip.
std::vector<at::Tensor> beam_select(at::Tensor val, at::Tensor idx, at::Tensor lse,
                                    at::Tensor beam_scores, at::Tensor done,
                                    int64_t fill_token, int64_t eos) {
  CHECK_GPU(val);
  CHECK_GPU(idx);
  CHECK_GPU(lse);
  CHECK_GPU(beam_scores);
  CHECK_GPU(done);
  TORCH_CHECK(val.scalar_type() == at::kFloat && lse.scalar_type() == at::kFloat &&
                  beam_scores.scalar_type() == at::kFloat,
              "beam_select: val, lse and beam_scores must be fp32");
  TORCH_CHECK(idx.scalar_type() == at::kInt, "beam_select: idx must be int32");
  TORCH_CHECK(done.scalar_type() == at::kBool, "beam_select: done must be bool");
  TORCH_CHECK(val.dim() == 2 && beam_scores.dim() == 2, "beam_select: val (B*K, K), beam_scores (B, K)");
  const long B = beam_scores.size(0), K = beam_scores.size(1);
  TORCH_CHECK(K >= 1 && K <= 16, "beam_select: K = ", K, " outside [1, 16]");
  TORCH_CHECK(val.size(0) == B * K && val.size(1) == K && idx.sizes() == val.sizes() &&
                  lse.numel() == B * K && lse.dim() == 1 && done.numel() == B * K &&
                  done.dim() == 1,
              "beam_select: shapes disagree with beam_scores (", B, ", ", K, ")");
  auto scores = at::empty({B, K}, beam_scores.options());
  auto lopt = val.options().dtype(at::kLong);
  auto parent = at::empty({B * K}, lopt);
  auto tok = at::empty({B * K}, lopt);
  auto done_new = at::empty({B * K}, done.options());
  if (B == 0) return {scores, parent, tok, done_new};
  launch_beam_select(val.data_ptr<float>(), idx.data_ptr<int>(), lse.data_ptr<float>(),
                     beam_scores.data_ptr<float>(), done.data_ptr<bool>(), B, (int)K,
                     (long)fill_token, (long)eos, scores.data_ptr<float>(),
                     parent.data_ptr<long>(), tok.data_ptr<long>(), done_new.data_ptr<bool>(),
                     cur_stream());
  return {scores, parent, tok, done_new};
}

void launch_bce_logits_fwd(const float*, const float*, const float*, const float*,
                           float*, int, hipStream_t);
void launch_bce_logits_bwd(const float*, const float*, const float*, const float*,
                           const float*, const float*, float*, int, hipStream_t);

// graph-level head (csrc/graph_head.hip)
int gate_pool_num_chunks(int N);
void launch_gate_pool_fwd(const __hip_bfloat16*, const __hip_bfloat16*, const float*,
                          const float*, const int*, __hip_bfloat16*, float*, float*,
                          int*, float*, float*, int, int, hipStream_t);
void launch_gate_pool_bwd(const __hip_bfloat16*, const __hip_bfloat16*, const __hip_bfloat16*,
                          const float*, const float*, const float*, const int*,
                          __hip_bfloat16*, __hip_bfloat16*, float*, float*, int, int,
                          hipStream_t);
void launch_mlp3_fwd(const __hip_bfloat16*, const float*, const float*, const float*,
                     const float*, const float*, const float*, float*, float*, float*,
                     int, hipStream_t);
void launch_mlp3_bwd(const float*, const float*, const float*, const float*, const float*,
                     const float*, float*, float*, __hip_bfloat16*, int, hipStream_t);
void launch_mlp3_wgrad(const __hip_bfloat16*, const float*, const float*, const float*,
                       const float*, const float*, float*, float*, float*, float*,
                       float*, float*, int, hipStream_t);

// fused concat + gate linear + segment-softmax attention pool (flow-GNN head).
// Returns {pooled bf16 (B,256), alpha fp32 (N), pooled fp32 (B,256), node ->
// graph id int32 (N)}; the last two are for the backward, which takes its
// per-graph dot from the fp32 row. A graph with no nodes gets a zero row.
std::vector<at::Tensor> gate_pool_fwd(at::Tensor x1, at::Tensor x2, at::Tensor wg,
                                      at::Tensor bg, at::Tensor node_offsets) {
  CHECK_GPU(x1);
  CHECK_GPU(x2);
  TORCH_CHECK(x1.scalar_type() == at::kBFloat16 && x2.scalar_type() == at::kBFloat16);
  TORCH_CHECK(x1.is_contiguous() && x2.is_contiguous());
  TORCH_CHECK(wg.scalar_type() == at::kFloat && bg.scalar_type() == at::kFloat);
  TORCH_CHECK(node_offsets.is_cuda() && node_offsets.scalar_type() == at::kInt &&
              node_offsets.is_contiguous() && node_offsets.numel() >= 1);
  const int N = x1.size(0), D1 = x1.size(1), D = D1 + (int)x2.size(1);
  const int B = node_offsets.numel() - 1;
  TORCH_CHECK(x2.size(0) == N && wg.numel() == D);
  TORCH_CHECK(D == 256 && D1 == 128, "fused gate_pool is built for the "
              "128+128 concat geometry (vectorized lane mapping)");
  auto fopt = x1.options().dtype(at::kFloat);
  auto out = at::empty({B, D}, x1.options());
  auto pooled32 = at::empty({B, D}, fopt);
  auto alpha = at::empty({N}, fopt);
  auto gid = at::empty({N}, x1.options().dtype(at::kInt));
  const int nch = gate_pool_num_chunks(N);
  auto ws_vec = at::empty({std::max(nch, 1) * 2, D}, fopt);
  auto ws_ms = at::empty({std::max(nch, 1) * 2, 2}, fopt);
  launch_gate_pool_fwd(ptr<bf16_t>(x1), ptr<bf16_t>(x2), wg.data_ptr<float>(),
                       bg.data_ptr<float>(), node_offsets.data_ptr<int>(),
                       mptr<bf16_t>(out), pooled32.data_ptr<float>(),
                       alpha.data_ptr<float>(), gid.data_ptr<int>(),
                       ws_vec.data_ptr<float>(), ws_ms.data_ptr<float>(), N, B,
                       cur_stream());
  return {out, alpha, pooled32, gid};
}

std::vector<at::Tensor> gate_pool_bwd(at::Tensor grad_out, at::Tensor x1, at::Tensor x2,
                                      at::Tensor wg, at::Tensor alpha,
                                      at::Tensor node_offsets, at::Tensor pooled32,
                                      at::Tensor gid,
                                      c10::optional<at::Tensor> out_wg,
                                      c10::optional<at::Tensor> out_bg) {
  CHECK_GPU(grad_out);
  const int N = x1.size(0), D1 = x1.size(1), D = D1 + (int)x2.size(1);
  const int B = node_offsets.numel() - 1;
  TORCH_CHECK(D == 256 && D1 == 128, "fused gate_pool is built for the "
              "128+128 concat geometry (vectorized lane mapping)");
  TORCH_CHECK(grad_out.scalar_type() == at::kBFloat16 && grad_out.is_contiguous() &&
              grad_out.size(0) == B && grad_out.size(1) == D);
  TORCH_CHECK(pooled32.is_cuda() && pooled32.scalar_type() == at::kFloat &&
              pooled32.is_contiguous() && pooled32.numel() == (long)B * D);
  TORCH_CHECK(gid.is_cuda() && gid.scalar_type() == at::kInt && gid.is_contiguous() &&
              gid.numel() == N);
  TORCH_CHECK(alpha.scalar_type() == at::kFloat && alpha.numel() == N &&
              wg.scalar_type() == at::kFloat && wg.numel() == D);
  auto gx1 = at::empty_like(x1);
  auto gx2 = at::empty_like(x2);
  TORCH_CHECK(out_wg.has_value() == out_bg.has_value(),
              "gate_pool_bwd: out_wg and out_bg go together");
  auto dwg = acc_or_zeros(out_wg, {D}, x1.options(), "gate_pool_bwd out_wg");
  auto dbg = acc_or_zeros(out_bg, {1}, x1.options(), "gate_pool_bwd out_bg");
  launch_gate_pool_bwd(ptr<bf16_t>(grad_out), ptr<bf16_t>(x1), ptr<bf16_t>(x2),
                       wg.data_ptr<float>(), alpha.data_ptr<float>(),
                       pooled32.data_ptr<float>(), gid.data_ptr<int>(),
                       mptr<bf16_t>(gx1), mptr<bf16_t>(gx2), dwg.data_ptr<float>(),
                       dbg.data_ptr<float>(), N, B, cur_stream());
  return {gx1, gx2, dwg, dbg};
}

// fused 3-layer MLP head forward: logits + relu activations (fp32 saves).
// W1/W2 are the master weights in their native (out, in) layout.
std::vector<at::Tensor> mlp3_fwd(at::Tensor x, at::Tensor W1, at::Tensor b1,
                                 at::Tensor W2, at::Tensor b2, at::Tensor W3,
                                 at::Tensor b3) {
  CHECK_GPU(x);
  TORCH_CHECK(x.scalar_type() == at::kBFloat16 && x.is_contiguous());
  const int B = x.size(0), D = x.size(1);
  TORCH_CHECK(D == 256 && W1.numel() == (long)D * D && W2.numel() == (long)D * D &&
              W3.numel() == D && b1.numel() == D && b2.numel() == D && b3.numel() == 1);
  for (const at::Tensor* t : {&W1, &b1, &W2, &b2, &W3, &b3})
    TORCH_CHECK(t->is_cuda() && t->scalar_type() == at::kFloat && t->is_contiguous());
  auto fopt = x.options().dtype(at::kFloat);
  auto h1 = at::empty({B, D}, fopt);
  auto h2 = at::empty({B, D}, fopt);
  auto logits = at::empty({B}, fopt);
  launch_mlp3_fwd(ptr<bf16_t>(x), W1.data_ptr<float>(), b1.data_ptr<float>(),
                  W2.data_ptr<float>(), b2.data_ptr<float>(), W3.data_ptr<float>(),
                  b3.data_ptr<float>(), h1.data_ptr<float>(), h2.data_ptr<float>(),
                  logits.data_ptr<float>(), B, cur_stream());
  return {logits, h1, h2};
}

std::vector<at::Tensor> mlp3_bwd(at::Tensor dlogits, at::Tensor x, at::Tensor h1,
                                 at::Tensor h2, at::Tensor W1, at::Tensor W2,
                                 at::Tensor W3,
                                 c10::optional<std::vector<at::Tensor>> outs) {
  CHECK_GPU(dlogits);
  const int B = x.size(0), D = x.size(1);
  TORCH_CHECK(D == 256 && x.scalar_type() == at::kBFloat16 && x.is_contiguous() &&
              dlogits.scalar_type() == at::kFloat && dlogits.numel() == B &&
              h1.numel() == (long)B * D && h2.numel() == (long)B * D);
  for (const at::Tensor* t : {&W1, &W2, &W3})
    TORCH_CHECK(t->is_cuda() && t->scalar_type() == at::kFloat && t->is_contiguous());
  auto fopt = x.options().dtype(at::kFloat);
  auto dh1 = at::empty({B, D}, fopt);
  auto dh2 = at::empty({B, D}, fopt);
  auto dx = at::empty_like(x);
  launch_mlp3_bwd(dlogits.data_ptr<float>(), h1.data_ptr<float>(), h2.data_ptr<float>(),
                  W1.data_ptr<float>(), W2.data_ptr<float>(), W3.data_ptr<float>(),
                  dh1.data_ptr<float>(), dh2.data_ptr<float>(), mptr<bf16_t>(dx), B,
                  cur_stream());
  // the wgrad kernel accumulates (+=): into the flat .grad views when given
  // (outs = [dW1, db1, dW2, db2, dW3, db3]), else into fresh zeros
  TORCH_CHECK(!outs.has_value() || outs->size() == 6, "mlp3_bwd: outs takes 6 tensors");
  auto acc = [&](int i, at::IntArrayRef shape) {
    c10::optional<at::Tensor> out;
    if (outs.has_value()) out = (*outs)[i];
    return acc_or_zeros(out, shape, fopt, "mlp3_bwd outs");
  };
  auto dW1 = acc(0, {D, D}), dW2 = acc(2, {D, D}), dW3 = acc(4, {1, D});
  auto db1 = acc(1, {D}), db2 = acc(3, {D}), db3 = acc(5, {1});
  launch_mlp3_wgrad(ptr<bf16_t>(x), h1.data_ptr<float>(), h2.data_ptr<float>(),
                    dh1.data_ptr<float>(), dh2.data_ptr<float>(),
                    dlogits.data_ptr<float>(), dW1.data_ptr<float>(),
                    dW2.data_ptr<float>(), dW3.data_ptr<float>(), db1.data_ptr<float>(),
                    db2.data_ptr<float>(), db3.data_ptr<float>(), B, cur_stream());
  if (outs.has_value()) return {dx};
  return {dx, dW1, dW2, dW3, db1, db2, db3};
}

// ---------------------------------------------------------------------------
// Fused node-level head (csrc/node_head.hip): D1 = D2 = 128, D = 256 only.
// ---------------------------------------------------------------------------
void launch_node_head_fwd(const __hip_bfloat16*, const __hip_bfloat16*, const __hip_bfloat16*,
                          const __hip_bfloat16*, const float*, const float*, const float*,
                          const float*, float*, __hip_bfloat16*, __hip_bfloat16*,
                          __hip_bfloat16*, int, int, int, hipStream_t);
void launch_node_head_bwd(const float*, const __hip_bfloat16*, const __hip_bfloat16*,
                          const __hip_bfloat16*, const __hip_bfloat16*, const float*,
                          __hip_bfloat16*, __hip_bfloat16*, __hip_bfloat16*, __hip_bfloat16*,
                          float*, float*, int, int, hipStream_t);
int node_head_tile_rows(int, int);

static void check_node_head_w(const at::Tensor& W, const char* name) {
  TORCH_CHECK(W.is_cuda() && W.is_contiguous() && W.scalar_type() == at::kBFloat16 &&
              W.dim() == 2 && W.size(0) == 256 && W.size(1) == 256,
              name, " must be a contiguous (256,256) bf16 GPU tensor");
}
static void check_node_head_v(const at::Tensor& v, long n, const char* name) {
  TORCH_CHECK(v.is_cuda() && v.is_contiguous() && v.scalar_type() == at::kFloat &&
              v.numel() == n, name, " must be a contiguous fp32 GPU tensor of ", n,
              " elements");
}

// returns {logits} or, with save, {logits, X = [h|fe], H1, H2}
std::vector<at::Tensor> node_head_fwd(at::Tensor h, at::Tensor fe, at::Tensor W1,
                                      at::Tensor W2, at::Tensor b1, at::Tensor b2,
                                      at::Tensor w3, at::Tensor b3, bool save,
                                      int64_t tile_rows) {
  CHECK_GPU(h);
  CHECK_GPU(fe);
  TORCH_CHECK(h.scalar_type() == at::kBFloat16 && fe.scalar_type() == at::kBFloat16,
              "node_head_fwd: h and fe must be bf16");
  TORCH_CHECK(h.dim() == 2 && fe.dim() == 2 && h.size(1) == 128 && fe.size(1) == 128 &&
              h.size(0) == fe.size(0),
              "node_head_fwd supports only D1 = D2 = 128 (D = 256)");
  check_node_head_w(W1, "W1");
  check_node_head_w(W2, "W2");
  check_node_head_v(b1, 256, "b1");
  check_node_head_v(b2, 256, "b2");
  check_node_head_v(w3, 256, "w3");
  check_node_head_v(b3, 1, "b3");
  const int N = h.size(0);
  auto logits = at::empty({N}, h.options().dtype(at::kFloat));
  at::Tensor X, H1, H2;
  if (save) {
    X = at::empty({N, 256}, h.options());
    H1 = at::empty({N, 256}, h.options());
    H2 = at::empty({N, 256}, h.options());
  }
  launch_node_head_fwd(ptr<bf16_t>(h), ptr<bf16_t>(fe), ptr<bf16_t>(W1), ptr<bf16_t>(W2),
                       b1.data_ptr<float>(), b2.data_ptr<float>(), w3.data_ptr<float>(),
                       b3.data_ptr<float>(), logits.data_ptr<float>(),
                       save ? mptr<bf16_t>(X) : nullptr, save ? mptr<bf16_t>(H1) : nullptr,
                       save ? mptr<bf16_t>(H2) : nullptr, N, save ? 1 : 0, (int)tile_rows,
                       cur_stream());
  if (save) return {logits, X, H1, H2};
  return {logits};
}

// returns {dh, dfe, dH1, dH2, dW3, db3}; dW3/db3 ACCUMULATE into out_w3 /
// out_b3 (live fp32 .grad views) when given, else into fresh zeros
std::vector<at::Tensor> node_head_bwd(at::Tensor dlogits, at::Tensor H1, at::Tensor H2,
                                      at::Tensor W1T, at::Tensor W2T, at::Tensor w3,
                                      c10::optional<at::Tensor> out_w3,
                                      c10::optional<at::Tensor> out_b3,
                                      int64_t tile_rows) {
  CHECK_GPU(dlogits);
  CHECK_GPU(H1);
  CHECK_GPU(H2);
  const int N = H1.size(0);
  TORCH_CHECK(H1.scalar_type() == at::kBFloat16 && H2.scalar_type() == at::kBFloat16 &&
              H1.dim() == 2 && H1.size(1) == 256 && H2.dim() == 2 && H2.size(1) == 256 &&
              H2.size(0) == N, "node_head_bwd: H1, H2 must be (N,256) bf16");
  check_node_head_v(dlogits, N, "dlogits");
  check_node_head_w(W1T, "W1T");
  check_node_head_w(W2T, "W2T");
  check_node_head_v(w3, 256, "w3");
  auto fopt = H1.options().dtype(at::kFloat);
  auto dW3 = acc_or_zeros(out_w3, {1, 256}, fopt, "node_head_bwd out_w3");
  auto db3 = acc_or_zeros(out_b3, {1}, fopt, "node_head_bwd out_b3");
  auto dH1 = at::empty_like(H1);
  auto dH2 = at::empty_like(H2);
  auto dh = at::empty({N, 128}, H1.options());
  auto dfe = at::empty({N, 128}, H1.options());
  launch_node_head_bwd(dlogits.data_ptr<float>(), ptr<bf16_t>(H1), ptr<bf16_t>(H2),
                       ptr<bf16_t>(W2T), ptr<bf16_t>(W1T), w3.data_ptr<float>(),
                       mptr<bf16_t>(dH1), mptr<bf16_t>(dH2), mptr<bf16_t>(dh),
                       mptr<bf16_t>(dfe), dW3.data_ptr<float>(), db3.data_ptr<float>(), N,
                       (int)tile_rows, cur_stream());
  return {dh, dfe, dH1, dH2, dW3, db3};
}

void adamw_fused(at::Tensor p, at::Tensor g, at::Tensor m, at::Tensor v, double lr,
                 double beta1, double beta2, double eps, double weight_decay, at::Tensor step,
                 c10::optional<at::Tensor> gclip, bool l2_mode,
                 c10::optional<at::Tensor> p16) {
  CHECK_GPU(p);
  TORCH_CHECK(p.scalar_type() == at::kFloat && g.scalar_type() == at::kFloat);
  TORCH_CHECK(p.numel() == g.numel() && p.numel() == m.numel() && p.numel() == v.numel());
  TORCH_CHECK(step.is_cuda() && step.scalar_type() == at::kFloat && step.numel() == 1,
              "step must be a device float[1] step counter (pre-incremented)");
  const float* gc = nullptr;
  if (gclip.has_value()) {
    TORCH_CHECK(gclip->is_cuda() && gclip->scalar_type() == at::kFloat);
    gc = gclip->data_ptr<float>();
  }
  void* s16 = nullptr;
  if (p16.has_value()) {
    TORCH_CHECK(p16->is_cuda() && p16->scalar_type() == at::kBFloat16 &&
                p16->numel() == p.numel() && p16->is_contiguous(),
                "p16 must be a contiguous bf16 shadow of p");
    s16 = p16->data_ptr();
  }
  launch_adamw_fused(p.data_ptr<float>(), g.data_ptr<float>(), m.data_ptr<float>(),
                     v.data_ptr<float>(), p.numel(), (float)lr, (float)beta1, (float)beta2,
                     (float)eps, (float)weight_decay, step.data_ptr<float>(), gc,
                     l2_mode ? 1 : 0, s16, cur_stream());
}

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.doc() = "deepdfa_amd MI355X (gfx950) kernels";
  m.def("embed4_fwd", &embed4_fwd, pybind11::arg("tables"), pybind11::arg("idx"), pybind11::arg("out_bf16") = false);
  m.def("embed4_bwd", &embed4_bwd, pybind11::arg("grad_out"), pybind11::arg("idx"),
        pybind11::arg("V"), pybind11::arg("Demb"),
        pybind11::arg("out") = pybind11::none());
  m.def("spmm_sum", &spmm_sum);
  m.def("gru_gates_fwd", &gru_gates_fwd);
  m.def("gru_gates_bwd", &gru_gates_bwd);
  m.def("attn_pool_fwd", &attn_pool_fwd);
  m.def("attn_pool_bwd", &attn_pool_bwd);
  m.def("segment_max", &segment_max);
  m.def("gemm_bias", &gemm_bias);
  m.def("wgrad", &wgrad, pybind11::arg("A"), pybind11::arg("B"),
        pybind11::arg("out") = pybind11::none());
  m.def("gru_gates2_fwd", &gru_gates2_fwd);
  m.def("gru_gates2_bwd", &gru_gates2_bwd);
  m.def("colsum", &colsum, pybind11::arg("x"), pybind11::arg("out") = pybind11::none());
  m.def("ggnn_fused_fwd", &ggnn_fused_fwd, pybind11::arg("indptr"), pybind11::arg("indices"),
        pybind11::arg("x"), pybind11::arg("W_e"), pybind11::arg("b_e"),
        pybind11::arg("Wcat_perm"), pybind11::arg("b_perm"), pybind11::arg("n_steps"),
        pybind11::arg("fuse") = true);
  m.def("pack_gru_weights", &pack_gru_weights);
  m.def("bce_logits_fwd", [](at::Tensor logits, at::Tensor labels,
                             c10::optional<at::Tensor> weight,
                             c10::optional<at::Tensor> pos_weight) {
    CHECK_GPU(logits);
    auto out2 = at::empty({2}, logits.options());
    launch_bce_logits_fwd(
        logits.data_ptr<float>(), labels.data_ptr<float>(),
        weight.has_value() ? weight->data_ptr<float>() : nullptr,
        pos_weight.has_value() ? pos_weight->data_ptr<float>() : nullptr,
        out2.data_ptr<float>(), logits.numel(), cur_stream());
    return out2;
  });
  m.def("bce_logits_bwd", [](at::Tensor logits, at::Tensor labels,
                             c10::optional<at::Tensor> weight,
                             c10::optional<at::Tensor> pos_weight,
                             at::Tensor grad, at::Tensor out2) {
    auto dlogits = at::empty_like(logits);
    launch_bce_logits_bwd(
        logits.data_ptr<float>(), labels.data_ptr<float>(),
        weight.has_value() ? weight->data_ptr<float>() : nullptr,
        pos_weight.has_value() ? pos_weight->data_ptr<float>() : nullptr,
        grad.data_ptr<float>(), out2.data_ptr<float>(),
        dlogits.data_ptr<float>(), logits.numel(), cur_stream());
    return dlogits;
  });
  m.def("gate_pool_fwd", &gate_pool_fwd);
  m.def("gate_pool_bwd", &gate_pool_bwd, pybind11::arg("grad_out"), pybind11::arg("x1"),
        pybind11::arg("x2"), pybind11::arg("wg"), pybind11::arg("alpha"),
        pybind11::arg("node_offsets"), pybind11::arg("pooled32"), pybind11::arg("gid"),
        pybind11::arg("out_wg") = pybind11::none(),
        pybind11::arg("out_bg") = pybind11::none());
  m.def("mlp3_fwd", &mlp3_fwd);
  m.def("mlp3_bwd", &mlp3_bwd, pybind11::arg("dlogits"), pybind11::arg("x"),
        pybind11::arg("h1"), pybind11::arg("h2"), pybind11::arg("W1"),
        pybind11::arg("W2"), pybind11::arg("W3"),
        pybind11::arg("outs") = pybind11::none());
  m.def("layernorm_fwd", &layernorm_fwd);
  m.def("layernorm_bwd", &layernorm_bwd);
  m.def("layernorm_wgrad", &layernorm_wgrad);
  m.def("bias_gelu_fwd", &bias_gelu_fwd);
  m.def("bias_gelu_bwd", &bias_gelu_bwd);
  m.def("softmax_mask_fwd", &softmax_mask_fwd);
  m.def("rmsnorm_fwd", &rmsnorm_fwd);
  m.def("rmsnorm_bwd", &rmsnorm_bwd);
  m.def("rmsnorm_wgrad", &rmsnorm_wgrad, pybind11::arg("dy"), pybind11::arg("x"),
        pybind11::arg("rstd"), pybind11::arg("out") = pybind11::none());
  m.def("flash_attn_fwd", &flash_attn_fwd);
  m.def("flash_attn_received", &flash_attn_received);
  m.def("decode_self_attn", &decode_self_attn);
  m.def("decode_cross_attn", &decode_cross_attn);
  m.def("flash_attn_bwd", &flash_attn_bwd, pybind11::arg("dO"), pybind11::arg("Q"),
        pybind11::arg("K"), pybind11::arg("V"), pybind11::arg("O"), pybind11::arg("lse"),
        pybind11::arg("H"), pybind11::arg("valid"), pybind11::arg("bias"),
        pybind11::arg("scale"), pybind11::arg("causal"), pybind11::arg("dropout_p"),
        pybind11::arg("seed"), pybind11::arg("need_dbias"), pybind11::arg("fused_grads"),
        pybind11::arg("dbias_accum") = pybind11::none(),
        pybind11::arg("kv_fused") = false);
  m.def("flash_rect_fwd", &flash_rect_fwd);
  m.def("flash_rect_bwd", &flash_rect_bwd, pybind11::arg("dO"), pybind11::arg("Q"),
        pybind11::arg("K"), pybind11::arg("V"), pybind11::arg("O"), pybind11::arg("lse"),
        pybind11::arg("H"), pybind11::arg("valid"), pybind11::arg("bias"),
        pybind11::arg("scale"), pybind11::arg("causal"), pybind11::arg("dropout_p"),
        pybind11::arg("seed"), pybind11::arg("need_dbias"),
        pybind11::arg("dbias_accum") = pybind11::none(), pybind11::arg("kv_fused") = false);
  m.def("lmhead_ce_fwd", &lmhead_ce_fwd);
  m.def("lmhead_ce_bwd", &lmhead_ce_bwd);
  m.def("lmhead_topk", &lmhead_topk);
  m.def("beam_select", &beam_select);
  m.def("relbias_wgrad", [](at::Tensor dbias, at::Tensor buckets, int64_t nb) {
    tk_lead("relbias_wgrad", dbias);
    TORCH_CHECK(dbias.scalar_type() == at::kFloat, "relbias_wgrad: dbias must be fp32");
    TORCH_CHECK(dbias.dim() >= 2 && dbias.size(0) > 0, "relbias_wgrad: dbias must be (H, ...)");
    const int H = dbias.size(0);
    const long QK = dbias.numel() / H;
    // the kernel maps one head per lane of a 16-lane group
    TORCH_CHECK(H <= 16, "relbias_wgrad: at most 16 heads, got ", H);
    TORCH_CHECK(nb > 0 && (size_t)4 * nb * H * sizeof(float) <= kLdsLimit,
                "relbias_wgrad: num_buckets * H exceeds the per-wave LDS partials");
    TORCH_CHECK(buckets.numel() == QK, "relbias_wgrad: buckets must have ", QK, " entries");
    tk_arg("relbias_wgrad", "buckets", buckets, dbias, at::kInt, buckets.sizes());
    auto dw = at::zeros({nb, (long)H}, dbias.options());
    launch_relbias_wgrad(dbias.data_ptr<float>(), buckets.data_ptr<int>(),
                         dw.data_ptr<float>(), QK, H, (int)nb, cur_stream());
    return dw;
  });
  m.def("relu_dropout_fwd", [](at::Tensor x, double p, int64_t seed) {
    tk_lead("relu_dropout_fwd", x, false);
    TORCH_CHECK(x.numel() % (x.scalar_type() == at::kFloat ? 4 : 8) == 0,
                "relu_dropout: numel must be a multiple of the 16-B vector");
    auto out = at::empty_like(x);
    dispatch_float_bf16(x, "relu_dropout_fwd", [&](auto tag) {
      using T = decltype(tag);
      launch_relu_dropout_fwd<T>(ptr<T>(x), mptr<T>(out), x.numel(), (float)p,
                                 (unsigned long long)seed, cur_stream());
    });
    return out;
  });
  m.def("relu_dropout_bwd", [](at::Tensor dy, at::Tensor x, double p, int64_t seed) {
    tk_lead("relu_dropout_bwd", dy, false);
    TORCH_CHECK(dy.numel() % (dy.scalar_type() == at::kFloat ? 4 : 8) == 0,
                "relu_dropout: numel must be a multiple of the 16-B vector");
    tk_arg("relu_dropout_bwd", "x", x, dy, dy.scalar_type(), dy.sizes());
    auto dx = at::empty_like(dy);
    dispatch_float_bf16(dy, "relu_dropout_bwd", [&](auto tag) {
      using T = decltype(tag);
      launch_relu_dropout_bwd<T>(ptr<T>(dy), ptr<T>(x), mptr<T>(dx), dy.numel(),
                                 (float)p, (unsigned long long)seed, cur_stream());
    });
    return dx;
  });
  m.def("dropout_add_fwd", [](at::Tensor h, at::Tensor res, double p, int64_t seed) {
    tk_lead("dropout_add_fwd", h, false);
    tk_arg("dropout_add_fwd", "res", res, h, h.scalar_type(), h.sizes());
    TORCH_CHECK(h.numel() % (h.scalar_type() == at::kFloat ? 4 : 8) == 0,
                "dropout_add: numel must be a multiple of the 16-B vector");
    auto out = at::empty_like(h);
    dispatch_float_bf16(h, "dropout_add_fwd", [&](auto tag) {
      using T = decltype(tag);
      launch_dropout_add_fwd<T>(ptr<T>(h), ptr<T>(res), mptr<T>(out), h.numel(), (float)p,
                                (unsigned long long)seed, cur_stream());
    });
    return out;
  });
  m.def("dropout_add_bwd", [](at::Tensor dy, double p, int64_t seed) {
    tk_lead("dropout_add_bwd", dy, false);
    TORCH_CHECK(dy.numel() % (dy.scalar_type() == at::kFloat ? 4 : 8) == 0,
                "dropout_add: numel must be a multiple of the 16-B vector");
    auto dh = at::empty_like(dy);
    dispatch_float_bf16(dy, "dropout_add_bwd", [&](auto tag) {
      using T = decltype(tag);
      launch_dropout_add_bwd<T>(ptr<T>(dy), mptr<T>(dh), dy.numel(), (float)p,
                                (unsigned long long)seed, cur_stream());
    });
    return dh;
  });
  m.def("ln_res_dropout_fwd", [](at::Tensor h, at::Tensor res, at::Tensor gamma,
                                 at::Tensor beta, double eps, double p, int64_t seed) {
    tk_lead("ln_res_dropout_fwd", h);
    const int D = h.size(-1);
    TORCH_CHECK(D % 256 == 0, "ln_res_dropout: D must be a multiple of 256");
    const long N = h.numel() / D;
    tk_arg("ln_res_dropout_fwd", "res", res, h, h.scalar_type(), h.sizes());
    tk_arg("ln_res_dropout_fwd", "gamma", gamma, h, at::kFloat, {D});
    tk_arg("ln_res_dropout_fwd", "beta", beta, h, at::kFloat, {D});
    auto y = at::empty_like(h);
    auto mean = at::empty({N}, h.options().dtype(at::kFloat));
    auto rstd = at::empty({N}, h.options().dtype(at::kFloat));
    dispatch_float_bf16(h, "ln_res_dropout_fwd", [&](auto tag) {
      using T = decltype(tag);
      launch_ln_res_dropout_fwd<T>(ptr<T>(h), ptr<T>(res), gamma.data_ptr<float>(),
                                   beta.data_ptr<float>(), mptr<T>(y),
                                   mean.data_ptr<float>(), rstd.data_ptr<float>(), N, D,
                                   (float)eps, (float)p, (unsigned long long)seed,
                                   cur_stream());
    });
    return std::vector<at::Tensor>{y, mean, rstd};
  });
  m.def("ln_res_dropout_bwd", [](at::Tensor dy, at::Tensor h, at::Tensor res,
                                 at::Tensor gamma, at::Tensor mean, at::Tensor rstd,
                                 double p, int64_t seed) {
    tk_lead("ln_res_dropout_bwd", dy);
    const int D = dy.size(-1);
    TORCH_CHECK(D % 256 == 0, "ln_res_dropout: D must be a multiple of 256");
    const long N = dy.numel() / D;
    tk_arg("ln_res_dropout_bwd", "h", h, dy, dy.scalar_type(), dy.sizes());
    tk_arg("ln_res_dropout_bwd", "res", res, dy, dy.scalar_type(), dy.sizes());
    tk_arg("ln_res_dropout_bwd", "gamma", gamma, dy, at::kFloat, {D});
    tk_arg("ln_res_dropout_bwd", "mean", mean, dy, at::kFloat, {N});
    tk_arg("ln_res_dropout_bwd", "rstd", rstd, dy, at::kFloat, {N});
    auto dz = at::empty_like(dy);
    auto dh = at::empty_like(dy);
    auto z = at::empty_like(dy);
    dispatch_float_bf16(dy, "ln_res_dropout_bwd", [&](auto tag) {
      using T = decltype(tag);
      launch_ln_res_dropout_bwd<T>(ptr<T>(dy), ptr<T>(h), ptr<T>(res),
                                   gamma.data_ptr<float>(), mean.data_ptr<float>(),
                                   rstd.data_ptr<float>(), mptr<T>(dz), mptr<T>(dh),
                                   mptr<T>(z), N, D, (float)p, (unsigned long long)seed,
                                   cur_stream());
    });
    return std::vector<at::Tensor>{dz, dh, z};
  });
  m.def("ln_res_dropout_wgrad", [](at::Tensor dy, at::Tensor h, at::Tensor res,
                                   at::Tensor mean, at::Tensor rstd, double p,
                                   int64_t seed) {
    tk_lead("ln_res_dropout_wgrad", dy);
    const int D = dy.size(-1);
    const long N = dy.numel() / D;
    tk_arg("ln_res_dropout_wgrad", "h", h, dy, dy.scalar_type(), dy.sizes());
    tk_arg("ln_res_dropout_wgrad", "res", res, dy, dy.scalar_type(), dy.sizes());
    tk_arg("ln_res_dropout_wgrad", "mean", mean, dy, at::kFloat, {N});
    tk_arg("ln_res_dropout_wgrad", "rstd", rstd, dy, at::kFloat, {N});
    auto dgamma = at::zeros({(long)D}, dy.options().dtype(at::kFloat));
    auto dbeta = at::zeros({(long)D}, dy.options().dtype(at::kFloat));
    dispatch_float_bf16(dy, "ln_res_dropout_wgrad", [&](auto tag) {
      using T = decltype(tag);
      launch_ln_res_dropout_wgrad<T>(ptr<T>(dy), ptr<T>(h), ptr<T>(res),
                                     mean.data_ptr<float>(), rstd.data_ptr<float>(),
                                     dgamma.data_ptr<float>(), dbeta.data_ptr<float>(), N,
                                     D, (float)p, (unsigned long long)seed, cur_stream());
    });
    return std::vector<at::Tensor>{dgamma, dbeta};
  });
  m.def("embed_scatter", [](at::Tensor dY, at::Tensor idx, long num_rows, long padding_idx,
                            c10::optional<at::Tensor> out_opt) {
    tk_lead("embed_scatter", dY);
    const int D = dY.size(-1);
    const long N = dY.numel() / D;
    TORCH_CHECK(idx.numel() == N, "embed_scatter: idx must have one entry per row of dY");
    tk_arg("embed_scatter", "idx", idx, dY, at::kLong, idx.sizes());
    auto dW = acc_or_zeros(out_opt, {num_rows, (long)D}, dY.options(), "embed_scatter");
    dispatch_float_bf16(dY, "embed_scatter", [&](auto tag) {
      using T = decltype(tag);
      launch_embed_scatter<T>(ptr<T>(dY), idx.data_ptr<long>(),
                              dW.data_ptr<float>(), N, D, padding_idx,
                              cur_stream());
    });
    return dW;
  }, pybind11::arg("dY"), pybind11::arg("idx"), pybind11::arg("num_rows"),
     pybind11::arg("padding_idx"), pybind11::arg("out") = pybind11::none());
  m.def("fwd_prof", []() {
    auto t = torch::zeros({8}, torch::dtype(torch::kLong));
    fwd_prof_fetch(reinterpret_cast<unsigned long long*>(t.data_ptr<long>()));
    return t;
  });
  m.def("dkv_prof", []() {
    // variant-9 instrumentation readout: per-segment cycle totals
    auto t = torch::zeros({8}, torch::dtype(torch::kLong));
    dkv_prof_fetch(reinterpret_cast<unsigned long long*>(t.data_ptr<long>()));
    return t;
  });
  m.def("gemm2", &gemm2);
  m.def("adamw_fused", &adamw_fused, pybind11::arg("p"), pybind11::arg("g"),
        pybind11::arg("m"), pybind11::arg("v"), pybind11::arg("lr"),
        pybind11::arg("beta1"), pybind11::arg("beta2"), pybind11::arg("eps"),
        pybind11::arg("weight_decay"), pybind11::arg("step"),
        pybind11::arg("gclip") = pybind11::none(),
        pybind11::arg("l2_mode") = false,
        pybind11::arg("p16") = pybind11::none());
  m.def("softmax_mask_bwd", &softmax_mask_bwd);
  m.def("node_head_fwd", &node_head_fwd, pybind11::arg("h"), pybind11::arg("fe"),
        pybind11::arg("W1"), pybind11::arg("W2"), pybind11::arg("b1"), pybind11::arg("b2"),
        pybind11::arg("w3"), pybind11::arg("b3"), pybind11::arg("save") = true,
        pybind11::arg("tile_rows") = 0);
  m.def("node_head_bwd", &node_head_bwd, pybind11::arg("dlogits"), pybind11::arg("H1"),
        pybind11::arg("H2"), pybind11::arg("W1T"), pybind11::arg("W2T"), pybind11::arg("w3"),
        pybind11::arg("out_w3") = pybind11::none(), pybind11::arg("out_b3") = pybind11::none(),
        pybind11::arg("tile_rows") = 0);
  m.def("node_head_tile_rows", [](int64_t N, int64_t tile) {
    return node_head_tile_rows((int)N, (int)tile);
  }, pybind11::arg("N"), pybind11::arg("tile_rows") = 0);
  m.def("ggnn_fused_bwd", &ggnn_fused_bwd, pybind11::arg("grad_out"),
        pybind11::arg("t_indptr"), pybind11::arg("t_indices"), pybind11::arg("x"),
        pybind11::arg("W_eT"), pybind11::arg("WcatT"), pybind11::arg("HH"),
        pybind11::arg("M"), pybind11::arg("R"), pybind11::arg("Z"), pybind11::arg("Nn"),
        pybind11::arg("HN"), pybind11::arg("n_steps"),
        pybind11::arg("out_we") = pybind11::none(),
        pybind11::arg("out_be") = pybind11::none(),
        pybind11::arg("gru_outs") = pybind11::none(), pybind11::arg("fuse") = true,
        pybind11::arg("fused_wgrad") = true);
  m.def("ggnn_wgrad", &ggnn_wgrad, pybind11::arg("Ggicat"), pybind11::arg("M"),
        pybind11::arg("HH"), pybind11::arg("Gwh"), pybind11::arg("S"),
        pybind11::arg("out_we") = pybind11::none(), pybind11::arg("out_be") = pybind11::none(),
        pybind11::arg("gru_outs") = pybind11::none(), pybind11::arg("kchunk") = 0,
        pybind11::arg("lds_epi") = -1, pybind11::arg("two_launches") = false);
  // K rows per chunk the launcher uses for a K-row problem (kchunk = 0: its rule)
  m.def("ggnn_wgrad_kchunk", [](int64_t K, int64_t kchunk) {
    return ggnn_wgrad_kchunk((int)K, (int)kchunk);
  }, pybind11::arg("K"), pybind11::arg("kchunk") = 0);
}
