"""Autograd ops for the transformer stacks.

GPU: hand-written HIP kernels (csrc/transformer_kernels.hip), bf16/fp32 IO
with fp32 statistics and fp32 LN/bias parameters (mixed-precision master
weights). CPU: plain torch (also the numerics oracle).
"""

from __future__ import annotations

from typing import Optional

import torch

from ._ext import load_ext
from ._weights import (  # noqa: F401  (the first five are re-exported)
    CAPTURE_REFRESH, _bias_f32, _shadow_w16, _weights_epoch, bump_weights_epoch,
    derived, direct_grads, packed_grad, packed_shadow)


class _LayerNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, eps):
        ext = load_ext(required=True)
        wf = weight.float().contiguous()
        bf = bias.float().contiguous()
        x = x.contiguous()
        y, mean, rstd = ext.layernorm_fwd(x, wf, bf, eps)
        ctx.save_for_backward(x, wf, mean, rstd)
        return y

    @staticmethod
    def backward(ctx, dy):
        ext = load_ext(required=True)
        x, wf, mean, rstd = ctx.saved_tensors
        dy = dy.contiguous()
        dx = ext.layernorm_bwd(dy, x, wf, mean, rstd)
        dgamma, dbeta = ext.layernorm_wgrad(dy, x, mean, rstd)
        return dx, dgamma, dbeta, None


def layer_norm(x, weight, bias, eps: float = 1e-5):
    if x.is_cuda:
        return _LayerNorm.apply(x, weight, bias, eps)
    return torch.nn.functional.layer_norm(
        x.float(), (x.shape[-1],), weight.float(), bias.float(), eps
    ).to(x.dtype)


class _BiasGelu(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, bias):
        ext = load_ext(required=True)
        bf = bias.float().contiguous()
        x = x.contiguous()
        ctx.save_for_backward(x, bf)
        return ext.bias_gelu_fwd(x, bf)

    @staticmethod
    def backward(ctx, dy):
        ext = load_ext(required=True)
        x, bf = ctx.saved_tensors
        dy = dy.contiguous()
        dx = ext.bias_gelu_bwd(dy, x, bf)
        dbias = ext.colsum(dx.view(-1, dx.shape[-1]))
        return dx, dbias


def bias_gelu(x, bias):
    if x.is_cuda:
        return _BiasGelu.apply(x, bias)
    return torch.nn.functional.gelu(x.float() + bias.float()).to(x.dtype)


_seed_state = {"base": None, "ctr": 0}


def _next_seed() -> int:
    if _seed_state["base"] is None:
        _seed_state["base"] = torch.initial_seed() & 0x7FFFFFFF
    _seed_state["ctr"] += 1
    return (_seed_state["base"] * 2654435761 + _seed_state["ctr"]) & 0x7FFFFFFFFFFFFFFF


class _MaskedSoftmaxDropout(torch.autograd.Function):
    """(P, Pd) = softmax(S * scale) with key positions >= valid[b] masked,
    plus fused attention dropout (mask regenerated from the seed in
    backward; no mask storage). Pd is the differentiable output feeding
    P @ V; P is the pre-dropout probabilities (analysis output, marked
    non-differentiable)."""

    @staticmethod
    def forward(ctx, S, valid, scale, dropout_p, causal=False):
        ext = load_ext(required=True)
        seed = _next_seed() if dropout_p > 0 else 0
        P, Pd = ext.softmax_mask_fwd(S.contiguous(), valid, scale, dropout_p, seed, causal)
        ctx.save_for_backward(P)
        ctx.scale = scale
        ctx.dropout_p = dropout_p
        ctx.seed = seed
        ctx.mark_non_differentiable(P)
        return P, Pd

    @staticmethod
    def backward(ctx, _dP_unused, dPd):
        ext = load_ext(required=True)
        (P,) = ctx.saved_tensors
        dS = ext.softmax_mask_bwd(dPd.contiguous(), P, ctx.scale, ctx.dropout_p, ctx.seed)
        return dS, None, None, None, None


def masked_softmax_dropout(
    S: torch.Tensor,
    valid: Optional[torch.Tensor],
    scale: float,
    dropout_p: float = 0.0,
    causal: bool = False,
):
    """Returns (P pre-dropout, Pd post-dropout)."""
    if S.is_cuda:
        return _MaskedSoftmaxDropout.apply(S, valid, scale, dropout_p, causal)
    s = S.float() * scale
    L = S.shape[-1]
    if valid is not None:
        mask = torch.arange(L).view(1, 1, 1, L) >= valid.view(-1, 1, 1, 1)
        s = s.masked_fill(mask, float("-inf"))
    if causal:
        Lq = S.shape[-2]
        cmask = torch.arange(L).view(1, L) > torch.arange(Lq).view(Lq, 1)
        s = s.masked_fill(cmask.view(1, 1, Lq, L), float("-inf"))
    p = torch.softmax(s, dim=-1)
    p = torch.nan_to_num(p, nan=0.0).to(S.dtype)
    pd = torch.nn.functional.dropout(p, dropout_p) if dropout_p > 0 else p
    return p, pd


class _LinearBf16(torch.autograd.Function):
    """Linear layer on the custom transformer-shape GEMMs: forward and
    input-grad via gemm2 (2-phase glds MFMA), weight grad via the split-K
    wgrad kernel (fp32 output — the master-weight grad dtype directly),
    bias grad via colsum."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        ext = load_ext(required=True)
        x2d = x.reshape(-1, x.shape[-1]).contiguous()
        # fat shapes route to the library GEMMs and never read wt16 (backward
        # uses w16 directly), so the transpose copy is skipped for them
        fat = weight.shape[0] > 1024 or weight.shape[1] > 1024
        bf = torch.bfloat16
        w16 = _shadow_w16(weight)
        if w16 is not None:
            # optimizer-maintained bf16 shadow (parallel/optim.py): no cast
            # kernel — the adamw kernel wrote this view at the last step.
            # Only the transposed copy (square shapes) needs per-step refresh.
            b32 = _bias_f32(bias)
            wt16 = None if fat else derived(
                weight, "_dfa_wt_cache", (weight,),
                lambda: torch.empty(weight.shape[::-1], dtype=bf, device=weight.device),
                lambda wt: wt.copy_(w16.t()))
        else:
            # no flat optimizer: cache the bf16 / transposed weight and the
            # fp32 bias per parameter VERSION — the cast and transpose copies
            # otherwise dominate the elementwise kernel count (~3 x 72
            # linears/step)
            def alloc():
                dev = weight.device
                return (
                    torch.empty(weight.shape, dtype=bf, device=dev),
                    None if fat else torch.empty(weight.shape[::-1], dtype=bf, device=dev),
                    None if bias is None else torch.empty(
                        bias.shape, dtype=torch.float32, device=dev),
                )

            def fill(bufs):
                w16, wt16, b32 = bufs
                w16.copy_(weight.detach())
                if wt16 is not None:
                    wt16.copy_(w16.t())
                if b32 is not None:
                    b32.copy_(bias.detach())

            w16, wt16, b32 = derived(weight, "_dfa_cast_cache", (weight, bias),
                                     alloc, fill, extra=(bias is not None,))
        # shape dispatch (measured, profiles/optimization_r2.md): our gemm2
        # beats hipBLASLt on the square 768-ish shapes; the library wins the
        # fat no-bias ones (K or COL >= ~2k)
        if b32 is None and fat:
            out = torch.matmul(x2d, w16.t())
        else:
            out = ext.gemm2(x2d, w16, b32, None)
        ctx.save_for_backward(x2d, w16, wt16)
        ctx.has_bias = bias is not None
        ctx.x_shape = x.shape
        ctx.wp, ctx.bp = weight, bias
        return out.view(*x.shape[:-1], w16.shape[0])

    @staticmethod
    def backward(ctx, dy):
        ext = load_ext(required=True)
        x2d, w16, wt16 = ctx.saved_tensors
        dy2d = dy.reshape(-1, dy.shape[-1]).contiguous()
        if w16.shape[0] > 1024 or w16.shape[1] > 1024:
            dx = torch.matmul(dy2d, w16)  # dY @ W, library wins fat shapes
        else:
            dx = ext.gemm2(dy2d, wt16, None, None)
        # direct accumulation (parallel/optim.py): under the flat optimizer
        # the kernels atomically add into the pre-zeroed flat .grad views and
        # autograd sees None — no zeros() fill, no AccumulateGrad add
        dw = db = None
        wp, bp = ctx.wp, ctx.bp
        if ctx.needs_input_grad[1]:
            if direct_grads(wp):
                ext.wgrad(dy2d, x2d, out=wp.grad)
            else:
                dw = ext.wgrad(dy2d, x2d)  # (COL, K) fp32
        if ctx.has_bias and ctx.needs_input_grad[2]:
            if direct_grads(bp):
                ext.colsum(dy2d, out=bp.grad)
            else:
                db = ext.colsum(dy2d)
        return dx.view(ctx.x_shape), dw, db


def linear_usable(x, weight) -> bool:
    n = x.numel() // x.shape[-1]
    K, COL = weight.shape[1], weight.shape[0]
    return (
        x.is_cuda
        and x.dtype == torch.bfloat16
        and n % 128 == 0
        and K % 64 == 0
        and COL % 128 == 0
    )


def fused_linear(x, weight, bias=None):
    """F.linear with custom MFMA kernels where the geometry allows."""
    if linear_usable(x, weight):
        return _LinearBf16.apply(x, weight, bias)
    return torch.nn.functional.linear(x, weight, bias)


class _FlashAttention(torch.autograd.Function):
    """Fused attention, head_dim 64, (B, L, H*64) layout (csrc/flash_attn.hip):
    masked softmax + dropout + PV in one kernel, FA2-style two-pass backward.
    `bias` is the T5 additive position bias, fp32, TRANSPOSED key-major
    (H, Lk, Lq) — see models/t5.py _flash_bias_T."""

    @staticmethod
    def forward(ctx, q, k, v, H, valid, bias, scale, causal, dropout_p,
                bias_accum=None):
        ext = load_ext(required=True)
        seed = _next_seed() if dropout_p > 0 else 0
        # q/k/v may be row-strided slices of a fused QKV buffer — the
        # kernels take a row stride, so no contiguous() copies here
        O, lse = ext.flash_attn_fwd(q, k, v, H, valid, bias,
                                    scale, causal, dropout_p, seed)
        ctx.save_for_backward(q, k, v, O, lse)
        ctx.meta = (H, valid, bias, scale, causal, dropout_p, seed, bias_accum)
        ctx.need_dbias = bias is not None and ctx.needs_input_grad[5]
        return O

    @staticmethod
    def backward(ctx, dO):
        ext = load_ext(required=True)
        q, k, v, O, lse = ctx.saved_tensors
        H, valid, bias, scale, causal, dropout_p, seed, bias_accum = ctx.meta
        outs = ext.flash_attn_bwd(
            dO.contiguous(), q, k, v, O, lse,
            H, valid, bias, scale, causal, dropout_p, seed, ctx.need_dbias, False,
            bias_accum,
        )
        dbias = outs[3] if (ctx.need_dbias and bias_accum is None) else None
        return (outs[0], outs[1], outs[2], None, None, dbias, None, None, None,
                None)


def flash_attention(q, k, v, num_heads, valid=None, bias=None, scale=1.0,
                    causal=False, dropout_p=0.0, bias_accum=None):
    return _FlashAttention.apply(q, k, v, num_heads, valid, bias, scale, causal,
                                 dropout_p, bias_accum)


def flash_usable(x, L, Lk=None) -> bool:
    return (
        x.is_cuda
        and x.dtype == torch.bfloat16
        and L % 64 == 0
        and (Lk is None or Lk == L)
    )


class _RMSNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, eps):
        ext = load_ext(required=True)
        wf = weight.float().contiguous()
        x = x.contiguous()
        y, rstd = ext.rmsnorm_fwd(x, wf, eps)
        ctx.save_for_backward(x, wf, rstd)
        ctx.wp = weight
        return y

    @staticmethod
    def backward(ctx, dy):
        ext = load_ext(required=True)
        x, wf, rstd = ctx.saved_tensors
        dy = dy.contiguous()
        dx = ext.rmsnorm_bwd(dy, x, wf, rstd)
        wp = ctx.wp
        if direct_grads(wp) and ctx.needs_input_grad[1]:
            # direct accumulation into the flat .grad view (parallel/optim.py)
            ext.rmsnorm_wgrad(dy, x, rstd, out=wp.grad)
            return dx, None, None
        dgamma = ext.rmsnorm_wgrad(dy, x, rstd)
        return dx, dgamma, None


def rms_norm(x, weight, eps: float = 1e-6):
    """T5LayerNorm: no mean subtraction, no bias."""
    if x.is_cuda:
        return _RMSNorm.apply(x, weight, eps)
    v = x.float()
    y = v * torch.rsqrt(v.pow(2).mean(-1, keepdim=True) + eps)
    return (y * weight.float()).to(x.dtype)


def masked_softmax(S: torch.Tensor, valid: Optional[torch.Tensor], scale: float):
    # index 1 (the post-dropout output) is the differentiable one; with
    # dropout 0 it aliases the probabilities
    return masked_softmax_dropout(S, valid, scale, 0.0)[1]


class _EmbeddingLookup(torch.autograd.Function):
    """nn.Embedding fwd (torch gather) with a custom scatter-add backward
    (csrc/transformer_kernels.hip embed_scatter): replaces torch's
    radix-sort + segment-reduce + scatter stack in the grad path."""

    @staticmethod
    def forward(ctx, indices, weight, padding_idx):
        ctx.save_for_backward(indices)
        ctx.num_rows = weight.shape[0]
        ctx.w_dtype = weight.dtype
        ctx.padding_idx = padding_idx if padding_idx is not None else -1
        ctx.wp = weight
        return torch.nn.functional.embedding(indices, weight, padding_idx)

    @staticmethod
    def backward(ctx, dy):
        ext = load_ext(required=True)
        (indices,) = ctx.saved_tensors
        wp = ctx.wp
        if direct_grads(wp) and ctx.w_dtype == torch.float32:
            # scatter straight into the flat fp32 .grad view (pre-zeroed):
            # skips a (V, D) zeros + full-table AccumulateGrad add
            ext.embed_scatter(dy.contiguous(), indices.reshape(-1).contiguous(),
                              ctx.num_rows, ctx.padding_idx, out=wp.grad)
            return None, None, None
        dw = ext.embed_scatter(dy.contiguous(), indices.reshape(-1).contiguous(),
                               ctx.num_rows, ctx.padding_idx)
        return None, dw.to(ctx.w_dtype), None


def embedding_lookup(indices, weight, padding_idx=None):
    if indices.is_cuda:
        return _EmbeddingLookup.apply(indices, weight, padding_idx)
    return torch.nn.functional.embedding(indices, weight, padding_idx)


class _LayerNormResDropout(torch.autograd.Function):
    """y = LayerNorm(dropout(h) + residual) in one kernel per direction
    (csrc/transformer_kernels.hip ln_res_dropout_*): the transformer
    residual pattern with stateless dropout (mask regenerated from the
    seed in backward — only (h, res, seed) are kept)."""

    @staticmethod
    def forward(ctx, h, res, weight, bias, dropout_p, eps):
        ext = load_ext(required=True)
        wf = weight.float().contiguous()
        bf = bias.float().contiguous()
        h = h.contiguous()
        res = res.contiguous()
        seed = _next_seed() if dropout_p > 0 else 0
        y, mean, rstd = ext.ln_res_dropout_fwd(h, res, wf, bf, eps, dropout_p, seed)
        ctx.save_for_backward(h, res, wf, mean, rstd)
        ctx.meta = (dropout_p, seed)
        return y

    @staticmethod
    def backward(ctx, dy):
        ext = load_ext(required=True)
        h, res, wf, mean, rstd = ctx.saved_tensors
        p, seed = ctx.meta
        dy = dy.contiguous()
        # bwd also reconstructs z = dropout(h)+res once, so the column
        # reduction runs the plain (hash-free) LN wgrad kernel
        dz, dh, z = ext.ln_res_dropout_bwd(dy, h, res, wf, mean, rstd, p, seed)
        dgamma, dbeta = ext.layernorm_wgrad(dy, z, mean, rstd)
        return dh, dz, dgamma, dbeta, None, None


def layer_norm_res_dropout(h, res, weight, bias, dropout_p=0.0, eps=1e-5):
    """Fused LayerNorm(dropout(h) + res); falls back to composition on CPU
    or when D is not a multiple of 256."""
    if h.is_cuda and h.shape[-1] % 256 == 0:
        return _LayerNormResDropout.apply(h, res, weight, bias, dropout_p, eps)
    z = torch.nn.functional.dropout(h, dropout_p) if dropout_p > 0 else h
    z = z + res
    return layer_norm(z, weight, bias, eps) if z.is_cuda else (
        torch.nn.functional.layer_norm(
            z.float(), (z.shape[-1],), weight.float(), bias.float(), eps
        ).to(z.dtype)
    )


def _packed_cast(slot, ws, bs=()):
    """(w16, b32): the bf16 row-stack of the (D, K) weights `ws` and the fp32
    stack of the biases `bs` (None without biases), for parameters the flat
    optimizer does not hold back-to-back. Cached on ws[0] under `slot`;
    refreshed by one slice copy per parameter."""
    D, dev = ws[0].shape[0], ws[0].device

    def alloc():
        return (
            torch.empty(len(ws) * D, ws[0].shape[1], dtype=torch.bfloat16, device=dev),
            torch.empty(len(bs) * D, dtype=torch.float32, device=dev) if bs else None,
        )

    def fill(bufs):
        for buf, ps in zip(bufs, (ws, bs)):
            for i, p in enumerate(ps):
                buf[i * D:(i + 1) * D].copy_(p.detach())

    return derived(ws[0], slot, (*ws, *bs), alloc, fill, extra=(len(bs),))


class _QKVLinear(torch.autograd.Function):
    """Fused QKV projection: one (N, 3D) gemm2 / wgrad per layer instead of
    three 768-column calls (a 64x6-block grid underfills 256 CUs; the
    64x18 fused grid balances, and one K=8192 wgrad replaces three)."""

    @staticmethod
    def forward(ctx, x, wq, wk, wv, bq, bk, bv):
        ext = load_ext(required=True)
        x2d = x.reshape(-1, x.shape[-1]).contiguous()
        has_bias = bq is not None
        D = wq.shape[0]
        # q/k/v defined back-to-back sit ADJACENT in the flat optimizer's
        # bf16 shadow: the packed (3D, K) weight is a zero-copy view of the
        # shadow buffer — no per-step packing or cast kernels
        flat = packed_shadow((wq, wk, wv))
        if flat is not None:
            w16 = flat.view(3 * D, wq.shape[1])
            # the biases are fp32 masters already: one cat into the cached
            # buffer packs them
            b32 = derived(
                wq, "_dfa_qkv_bias_cache", (bq, bk, bv),
                lambda: torch.empty(3 * D, dtype=torch.float32, device=wq.device),
                lambda b: torch.cat([bq.detach(), bk.detach(), bv.detach()], out=b),
            ) if has_bias else None
        else:
            w16, b32 = _packed_cast("_dfa_qkv_cache", (wq, wk, wv),
                                    (bq, bk, bv) if has_bias else ())
        out = ext.gemm2(x2d, w16, b32, None)
        ctx.save_for_backward(x2d, w16)
        ctx.has_bias = has_bias
        ctx.x_shape = x.shape
        ctx.wparams = (wq, wk, wv)
        return out.view(*x.shape[:-1], w16.shape[0])

    @staticmethod
    def backward(ctx, dy):
        ext = load_ext(required=True)
        x2d, w16 = ctx.saved_tensors
        dy2d = dy.reshape(-1, dy.shape[-1]).contiguous()
        dx = torch.matmul(dy2d, w16)  # (N, 3D) @ (3D, D): fat K, library wins
        D = w16.shape[0] // 3
        wq, wk, wv = ctx.wparams
        # q/k/v grads adjacent in the flat grad buffer (T5, bias-free):
        # ONE wgrad accumulates the packed (3D, K) grad straight into the
        # flat .grad region — no zeros, no slicing, no AccumulateGrad adds
        g3 = None if ctx.has_bias else packed_grad((wq, wk, wv))
        if g3 is not None:
            ext.wgrad(dy2d, x2d, out=g3.view(3 * D, -1))
            return (dx.view(ctx.x_shape), None, None, None, None, None, None)
        dw = ext.wgrad(dy2d, x2d)  # (3D, K) fp32
        if ctx.has_bias:
            db = ext.colsum(dy2d)
            return (dx.view(ctx.x_shape), dw[:D], dw[D:2 * D], dw[2 * D:],
                    db[:D], db[D:2 * D], db[2 * D:])
        return (dx.view(ctx.x_shape), dw[:D], dw[D:2 * D], dw[2 * D:],
                None, None, None)


def fused_qkv(x, wq, wk, wv, bq=None, bk=None, bv=None):
    """Returns the fused (B, L, 3D) projection, or None if the geometry
    doesn't fit the custom GEMMs (caller falls back to per-projection)."""
    if linear_usable(x, wq) and wq.shape[0] % 128 == 0:
        return _QKVLinear.apply(x, wq, wk, wv, bq, bk, bv)
    return None


class _KVLinear(torch.autograd.Function):
    """Fused bias-free K/V projection for cross-attention (both read the
    SAME encoder states): one (N, 2D) gemm2/wgrad per layer instead of two
    768-column calls. With the flat optimizer the packed (2D, K) weight is a
    zero-copy view (k/v adjacent), and the packed grad accumulates directly
    into the flat .grad region (one wgrad, no AccumulateGrad adds)."""

    @staticmethod
    def forward(ctx, x, wk, wv):
        ext = load_ext(required=True)
        x2d = x.reshape(-1, x.shape[-1]).contiguous()
        flat = packed_shadow((wk, wv))
        if flat is not None:
            w16 = flat.view(2 * wk.shape[0], wk.shape[1])
        else:
            w16, _ = _packed_cast("_dfa_kv_cache", (wk, wv))
        out = ext.gemm2(x2d, w16, None, None)
        ctx.save_for_backward(x2d, w16)
        ctx.x_shape = x.shape
        ctx.wparams = (wk, wv)
        return out.view(*x.shape[:-1], w16.shape[0])

    @staticmethod
    def backward(ctx, dy):
        ext = load_ext(required=True)
        x2d, w16 = ctx.saved_tensors
        dy2d = dy.reshape(-1, dy.shape[-1]).contiguous()
        dx = torch.matmul(dy2d, w16)  # (N, 2D) @ (2D, D): fat K, library wins
        D = w16.shape[0] // 2
        wk, wv = ctx.wparams
        g2 = packed_grad((wk, wv))
        if g2 is not None:
            ext.wgrad(dy2d, x2d, out=g2.view(2 * D, -1))
            return dx.view(ctx.x_shape), None, None
        dw = ext.wgrad(dy2d, x2d)
        return dx.view(ctx.x_shape), dw[:D], dw[D:]


def fused_kv(x, wk, wv):
    """Fused (B, L, 2D) cross-attention K/V projection, or None when the
    geometry doesn't fit the custom GEMMs."""
    if linear_usable(x, wk) and wk.shape[0] % 128 == 0:
        return _KVLinear.apply(x, wk, wv)
    return None


class _FlashAttentionKV(torch.autograd.Function):
    """Flash attention with a dense Q and the FUSED (B, L, 2D) K/V
    projection (cross-attention): k/v are strided slices forward, backward
    writes dk/dv into one (B, L, 2D) buffer (flash_attn_bwd kv_fused)."""

    @staticmethod
    def forward(ctx, q, kv, H, valid, scale, dropout_p):
        ext = load_ext(required=True)
        D = kv.shape[-1] // 2
        k, v = kv[..., :D], kv[..., D:]
        seed = _next_seed() if dropout_p > 0 else 0
        O, lse = ext.flash_attn_fwd(q, k, v, H, valid, None, scale, False,
                                    dropout_p, seed)
        ctx.save_for_backward(q, kv, O, lse)
        ctx.meta = (H, valid, scale, dropout_p, seed)
        return O

    @staticmethod
    def backward(ctx, dO):
        ext = load_ext(required=True)
        q, kv, O, lse = ctx.saved_tensors
        H, valid, scale, dropout_p, seed = ctx.meta
        D = kv.shape[-1] // 2
        k, v = kv[..., :D], kv[..., D:]
        dq, dkv = ext.flash_attn_bwd(
            dO.contiguous(), q, k, v, O, lse, H, valid, None, scale, False,
            dropout_p, seed, False, False, None, kv_fused=True,
        )
        return dq, dkv, None, None, None, None


def flash_attention_kv(q, kv, num_heads, valid=None, scale=1.0, dropout_p=0.0):
    return _FlashAttentionKV.apply(q, kv, num_heads, valid, scale, dropout_p)


def flash_rect_usable(x, d) -> bool:
    """True where the general flash kernels (csrc/flash_rect.hip) serve `x`:
    CUDA, bf16, head_dim 64; any query and key length."""
    return x.is_cuda and x.dtype == torch.bfloat16 and d == 64


def _attention_rect_torch(q, k, v, H, valid, bias, scale, causal, dropout_p):
    """The flash_rect contract as a torch composition (CPU / oracle path):
    q (B, Lq, H*d), k, v (B, Lk, H*d), bias key-major (H, Lk, Lq). Keys >=
    min(valid[b], Lk) and, with causal, keys > q are masked; a row with no
    unmasked key gives 0. Computed in fp32 (fp64 for fp64 inputs)."""
    B, Lq, D = q.shape
    Lk = k.shape[1]
    d = D // H
    if (causal or bias is not None) and Lq != Lk:
        raise ValueError("causal and bias need Lq == Lk")
    if k.shape != v.shape or k.shape[0] != B or k.shape[2] != D:
        raise ValueError("k and v must both be (B, Lk, H*d)")
    ct = torch.float64 if q.dtype == torch.float64 else torch.float32
    qh = q.to(ct).view(B, Lq, H, d).transpose(1, 2)
    kh = k.to(ct).view(B, Lk, H, d).transpose(1, 2)
    vh = v.to(ct).view(B, Lk, H, d).transpose(1, 2)
    s = torch.matmul(qh, kh.transpose(-1, -2)) * scale
    if bias is not None:
        s = s + bias.to(ct).transpose(-1, -2).unsqueeze(0)
    key = torch.arange(Lk, device=q.device).view(1, 1, 1, Lk)
    dead = torch.zeros(B, 1, Lq, Lk, dtype=torch.bool, device=q.device)
    if valid is not None:
        dead = dead | (key >= valid.view(B, 1, 1, 1))
    if causal:
        dead = dead | (key > torch.arange(Lq, device=q.device).view(1, 1, Lq, 1))
    s = s.masked_fill(dead, float("-inf"))
    row_dead = dead.all(-1, keepdim=True)
    p = torch.softmax(s.masked_fill(row_dead, 0.0), dim=-1).masked_fill(row_dead, 0.0)
    if dropout_p > 0:
        p = torch.nn.functional.dropout(p, dropout_p, training=True)
    out = torch.matmul(p, vh)
    return out.transpose(1, 2).reshape(B, Lq, D).to(q.dtype)


class _FlashAttentionRect(torch.autograd.Function):
    """General fused attention, head_dim 64 (csrc/flash_rect.hip): Q
    (B, Lq, H*64), K/V (B, Lk, H*64) at any Lq, Lk >= 1; causal and the
    key-major (H, Lk, Lq) bias at Lq == Lk."""

    @staticmethod
    def forward(ctx, q, k, v, H, valid, bias, scale, causal, dropout_p,
                bias_accum=None):
        ext = load_ext(required=True)
        seed = _next_seed() if dropout_p > 0 else 0
        O, lse = ext.flash_rect_fwd(q, k, v, H, valid, bias, scale, causal,
                                    dropout_p, seed)
        ctx.save_for_backward(q, k, v, O, lse)
        ctx.meta = (H, valid, bias, scale, causal, dropout_p, seed, bias_accum)
        ctx.need_dbias = bias is not None and ctx.needs_input_grad[5]
        return O

    @staticmethod
    def backward(ctx, dO):
        ext = load_ext(required=True)
        q, k, v, O, lse = ctx.saved_tensors
        H, valid, bias, scale, causal, dropout_p, seed, bias_accum = ctx.meta
        outs = ext.flash_rect_bwd(
            dO.contiguous(), q, k, v, O, lse, H, valid, bias, scale, causal,
            dropout_p, seed, ctx.need_dbias, bias_accum,
        )
        dbias = outs[3] if (ctx.need_dbias and bias_accum is None) else None
        return (outs[0], outs[1], outs[2], None, None, dbias, None, None, None,
                None)


def flash_attention_rect(q, k, v, num_heads, valid=None, bias=None, scale=1.0,
                         causal=False, dropout_p=0.0, bias_accum=None):
    """Attention of q (B, Lq, H*d) over k, v (B, Lk, H*d) -> (B, Lq, H*d), any
    Lq and Lk. Keys >= min(valid[b], Lk) are masked (padded query rows are
    computed like any other); a row with no unmasked key gives 0. `causal` and
    `bias` (fp32, key-major (H, Lk, Lq), models/t5.py _flash_bias_T) need
    Lq == Lk. `bias_accum`: the shared (H, L, L) buffer dBias is added into
    instead of being returned as bias.grad.

    On the GPU (bf16, d = 64) this is csrc/flash_rect.hip; elsewhere the same
    contract in plain torch, where `bias_accum` is unused and the bias gets
    its gradient from autograd."""
    if q.is_cuda:
        return _FlashAttentionRect.apply(q, k, v, num_heads, valid, bias, scale,
                                         causal, dropout_p, bias_accum)
    return _attention_rect_torch(q, k, v, num_heads, valid, bias, scale, causal,
                                 dropout_p)


class _FlashAttentionRectKV(torch.autograd.Function):
    """flash_attention_rect with the fused (B, Lk, 2D) K|V projection: k/v
    are strided halves forward, backward writes dk|dv into one (B, Lk, 2D)
    buffer (flash_rect_bwd kv_fused)."""

    @staticmethod
    def forward(ctx, q, kv, H, valid, scale, dropout_p):
        ext = load_ext(required=True)
        D = kv.shape[-1] // 2
        seed = _next_seed() if dropout_p > 0 else 0
        O, lse = ext.flash_rect_fwd(q, kv[..., :D], kv[..., D:], H, valid, None,
                                    scale, False, dropout_p, seed)
        ctx.save_for_backward(q, kv, O, lse)
        ctx.meta = (H, valid, scale, dropout_p, seed)
        return O

    @staticmethod
    def backward(ctx, dO):
        ext = load_ext(required=True)
        q, kv, O, lse = ctx.saved_tensors
        H, valid, scale, dropout_p, seed = ctx.meta
        D = kv.shape[-1] // 2
        dq, dkv = ext.flash_rect_bwd(
            dO.contiguous(), q, kv[..., :D], kv[..., D:], O, lse, H, valid, None,
            scale, False, dropout_p, seed, False, None, kv_fused=True,
        )
        return dq, dkv, None, None, None, None


def flash_attention_rect_kv(q, kv, num_heads, valid=None, scale=1.0, dropout_p=0.0):
    """Cross-attention of q (B, Lq, D) over the two halves k | v of one
    (B, Lk, 2D) buffer (ops.fused_kv); see flash_attention_rect."""
    if q.is_cuda:
        if not kv.is_contiguous():
            raise ValueError("kv must be a contiguous (B, Lk, 2D) buffer")
        return _FlashAttentionRectKV.apply(q, kv, num_heads, valid, scale, dropout_p)
    D = kv.shape[-1] // 2
    return _attention_rect_torch(q, kv[..., :D], kv[..., D:], num_heads, valid, None,
                                 scale, False, dropout_p)


class _DropoutAdd(torch.autograd.Function):
    """out = res + dropout(h) in one kernel (T5 pre-norm residuals);
    d(res) = dy passes through with no kernel."""

    @staticmethod
    def forward(ctx, h, res, p):
        ext = load_ext(required=True)
        seed = _next_seed() if p > 0 else 0
        ctx.meta = (p, seed)
        return ext.dropout_add_fwd(h.contiguous(), res.contiguous(), p, seed)

    @staticmethod
    def backward(ctx, dy):
        p, seed = ctx.meta
        if p == 0:
            return dy, dy, None
        ext = load_ext(required=True)
        dy = dy.contiguous()
        return ext.dropout_add_bwd(dy, p, seed), dy, None


def dropout_add(h, res, p=0.0, training=True):
    """res + dropout(h); fused on GPU, torch composition elsewhere."""
    if not training:
        p = 0.0
    if h.is_cuda and h.numel() % (4 if h.dtype == torch.float32 else 8) == 0:
        return _DropoutAdd.apply(h, res, p)
    z = torch.nn.functional.dropout(h, p) if p > 0 else h
    return res + z


class _FlashAttentionQKV(torch.autograd.Function):
    """Flash attention taking the FUSED (B, L, 3D) QKV projection as one
    input: forward slices q/k/v as strided views (the kernels take row
    strides), backward writes dq/dk/dv into ONE (B, L, 3D) buffer — no
    slice-backward zero+scatter work in autograd."""

    @staticmethod
    def forward(ctx, qkv, H, valid, bias, scale, causal, dropout_p,
                bias_accum=None):
        ext = load_ext(required=True)
        D = qkv.shape[-1] // 3
        q, k, v = qkv[..., :D], qkv[..., D:2 * D], qkv[..., 2 * D:]
        seed = _next_seed() if dropout_p > 0 else 0
        O, lse = ext.flash_attn_fwd(q, k, v, H, valid, bias, scale, causal,
                                    dropout_p, seed)
        ctx.save_for_backward(qkv, O, lse)
        ctx.meta = (H, valid, bias, scale, causal, dropout_p, seed, bias_accum)
        ctx.need_dbias = bias is not None and ctx.needs_input_grad[3]
        return O

    @staticmethod
    def backward(ctx, dO):
        ext = load_ext(required=True)
        qkv, O, lse = ctx.saved_tensors
        H, valid, bias, scale, causal, dropout_p, seed, bias_accum = ctx.meta
        D = qkv.shape[-1] // 3
        q, k, v = qkv[..., :D], qkv[..., D:2 * D], qkv[..., 2 * D:]
        outs = ext.flash_attn_bwd(
            dO.contiguous(), q, k, v, O, lse,
            H, valid, bias, scale, causal, dropout_p, seed, ctx.need_dbias, True,
            bias_accum,
        )
        # bias_accum set: the dq kernel atomics landed in the SHARED buffer
        # (T5's 24 layers share one position bias) — no per-layer dBias
        dbias = outs[1] if (ctx.need_dbias and bias_accum is None) else None
        return outs[0], None, None, dbias, None, None, None, None


def flash_attention_qkv(qkv, num_heads, valid=None, bias=None, scale=1.0,
                        causal=False, dropout_p=0.0, bias_accum=None):
    return _FlashAttentionQKV.apply(qkv, num_heads, valid, bias, scale, causal,
                                    dropout_p, bias_accum)


def attention_received(q, k, num_heads, lse, valid=None, bias=None, scale=1.0,
                       causal=False):
    """R[b, h, j] = sum_i P[b, h, i, j], fp32 (B, H, L): the total attention
    each key token receives, with P = softmax_j(scale * q_i.k_j + bias[h, j, i])
    pre-dropout. Keys >= valid[b] (and, with `causal`, keys > i) are masked;
    padded query rows i >= valid[b] are summed like every other row, as the
    materialised path and the reference do. `bias` is fp32 key-major
    (H, Lk, Lq). Inference output: no gradient flows through it.

    On the GPU with bf16 head_dim-64 inputs and L % 64 == 0 this is
    flash_received_kernel, which rebuilds P from q, k and the forward's
    `lse`. Anything else computes the same quantity materialised in fp32;
    `lse` is then ignored and may be None."""
    B, L, D = q.shape
    H = num_heads
    with torch.no_grad():
        if (D == H * 64 and k.dtype == q.dtype and k.is_cuda
                and flash_usable(q, L, k.shape[1])):
            if lse is None:
                raise ValueError("attention_received needs the forward's lse on the kernel path")
            ext = load_ext(required=True)
            return ext.flash_attn_received(q, k, lse, H, valid, bias, scale, causal)
        d = D // H
        qh = q.float().view(B, L, H, d).transpose(1, 2)
        kh = k.float().view(B, k.shape[1], H, d).transpose(1, 2)
        s = torch.matmul(qh, kh.transpose(-1, -2)) * scale
        Lk = s.shape[-1]
        if bias is not None:
            s = s + bias.float().view(H, Lk, L).transpose(-1, -2)
        ar = torch.arange(Lk, device=s.device)
        if valid is not None:
            s = s.masked_fill(ar.view(1, 1, 1, Lk) >= valid.view(-1, 1, 1, 1), float("-inf"))
        if causal:
            qi = torch.arange(L, device=s.device)
            s = s.masked_fill((ar.view(1, Lk) > qi.view(L, 1)).view(1, 1, L, Lk), float("-inf"))
        p = torch.nan_to_num(torch.softmax(s, dim=-1), nan=0.0)
        return p.sum(dim=-2)


def _no_grad_inputs(name, *tensors):
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors):
        raise ValueError(
            f"{name} is an inference output: call it under torch.no_grad() "
            "or on inputs that do not require grad"
        )


def flash_attention_received(q, k, v, num_heads, valid=None, bias=None, scale=1.0,
                             causal=False):
    """(O, R): the flash forward's output (bit-identical to flash_attention at
    dropout_p = 0 — it is the same kernel launch) and the attention each key
    receives, computed from that forward's lse. Inference only: returns
    tensors without grad and raises ValueError on inputs that would need one."""
    _no_grad_inputs("flash_attention_received", q, k, v, bias)
    ext = load_ext(required=True)
    with torch.no_grad():
        O, lse = ext.flash_attn_fwd(q, k, v, num_heads, valid, bias, scale, causal, 0.0, 0)
        R = ext.flash_attn_received(q, k, lse, num_heads, valid, bias, scale, causal)
    return O, R


def flash_attention_received_qkv(qkv, num_heads, valid=None, bias=None, scale=1.0,
                                 causal=False):
    """flash_attention_received on the fused (B, L, 3D) projection: q/k/v are
    strided views, no copies."""
    _no_grad_inputs("flash_attention_received_qkv", qkv, bias)
    D = qkv.shape[-1] // 3
    with torch.no_grad():
        q, k, v = qkv[..., :D], qkv[..., D:2 * D], qkv[..., 2 * D:]
        return flash_attention_received(q, k, v, num_heads, valid, bias, scale, causal)


DECODE_CROSS_MAX_LK = 768  # the cross kernel parks 16 x Lk fp32 scores in 64 KB of LDS


def decode_attention_usable(x, d_kv, Lk=None) -> bool:
    """True where the decode attention kernels (csrc/decode_attn.hip) serve
    `x`: CUDA, bf16, head_dim 64 (and a source length the cross kernel holds)."""
    return (
        x.is_cuda
        and x.dtype == torch.bfloat16
        and d_kv == 64
        and (Lk is None or 1 <= Lk <= DECODE_CROSS_MAX_LK)
    )


def _decode_compute_dtype(q):
    return torch.float64 if q.dtype == torch.float64 else torch.float32


def decode_self_attention(q, k_new, v_new, k_cache, v_cache, anc, bias_dist, pos,
                          num_heads, scale=1.0):
    """One decoding step of causal self-attention with an in-place KV cache.

    q, k_new, v_new (R, H*d) are the new token's projections (row-strided
    views are fine). The call stores k_new / v_new into cache[r, pos] of the
    (R, Tmax, H*d) caches and returns the (R, H*d) attention output over keys
    0..pos. Key j < pos of row r is read from cache[anc[r, j], j]: `anc`
    (int32 (R, Tmax), or None for identity) is the beam-search indirection
    table, so reordering beams never moves K/V. Key pos is the new token
    itself. `bias_dist` (fp32 (H, Tmax), or None) adds bias_dist[h, pos - j]
    to the score of key j. Inference only: ValueError with grad enabled on an
    input that requires grad.

    On the GPU this is decode_self_kernel (bf16, d = 64); elsewhere the same
    contract in plain torch, computed in fp32 (fp64 for fp64 inputs)."""
    _no_grad_inputs("decode_self_attention", q, k_new, v_new, k_cache, v_cache, bias_dist)
    H = num_heads
    with torch.no_grad():
        if q.is_cuda:
            ext = load_ext(required=True)
            return ext.decode_self_attn(q, k_new, v_new, k_cache, v_cache, anc, bias_dist,
                                        int(pos), H, float(scale))
        R, D = q.shape
        d = D // H
        Tmax = k_cache.shape[1]
        if not 0 <= pos < Tmax:
            raise ValueError("pos must be in [0, Tmax)")
        k_cache[:, pos] = k_new
        v_cache[:, pos] = v_new
        T = pos + 1
        ct = _decode_compute_dtype(q)
        if anc is None:
            kh, vh = k_cache[:, :T], v_cache[:, :T]
        else:
            rows = anc[:, :T].long().clone()
            rows[:, pos] = torch.arange(R, device=q.device)  # the new token: own row
            cols = torch.arange(T, device=q.device).unsqueeze(0)
            kh, vh = k_cache[rows, cols], v_cache[rows, cols]
        s = torch.einsum("rhd,rthd->rht", q.to(ct).view(R, H, d),
                         kh.to(ct).view(R, T, H, d)) * scale
        if bias_dist is not None:
            s = s + bias_dist[:, pos - torch.arange(T, device=q.device)].to(ct)
        p = torch.softmax(s, dim=-1)
        out = torch.einsum("rht,rthd->rhd", p, vh.to(ct).view(R, T, H, d))
        return out.reshape(R, D).to(q.dtype)


def decode_cross_attention(q, k, v, valid, beams, num_heads, scale=1.0):
    """One decoding step of cross-attention over K/V stored once per SOURCE.

    q (R, H*d) with R = B * beams; k, v (B, Lk, H*d), e.g. the two halves of a
    fused_kv buffer. Row r attends over source r // beams (the
    repeat_interleave order of generate). Keys >= valid[b] get probability
    exactly 0; a source with valid[b] == 0 returns exact zeros (the eager
    softmax over an all-masked row gives NaN instead). Inference only.

    On the GPU this is decode_cross_kernel (bf16, d = 64, Lk <= 768);
    elsewhere plain torch in fp32 (fp64 for fp64 inputs)."""
    _no_grad_inputs("decode_cross_attention", q, k, v)
    H = num_heads
    with torch.no_grad():
        if q.is_cuda:
            ext = load_ext(required=True)
            return ext.decode_cross_attn(q, k, v, valid, int(beams), H, float(scale))
        R, D = q.shape
        B, Lk, _ = k.shape
        if beams < 1 or R != B * beams:
            raise ValueError("q must hold B * beams rows")
        d = D // H
        ct = _decode_compute_dtype(q)
        s = torch.einsum("bihd,bkhd->bhik", q.to(ct).view(B, beams, H, d),
                         k.to(ct).view(B, Lk, H, d)) * scale
        if valid is not None:
            dead = torch.arange(Lk, device=q.device).view(1, 1, 1, Lk) >= valid.view(-1, 1, 1, 1)
            s = s.masked_fill(dead, float("-inf"))
        p = torch.nan_to_num(torch.softmax(s, dim=-1), nan=0.0)
        out = torch.einsum("bhik,bkhd->bihd", p, v.to(ct).view(B, Lk, H, d))
        return out.reshape(R, D).to(q.dtype)


def _vocab_padded(weight):
    """The (Vp, K) bf16 copy of the vocabulary matrix, zero rows from V to
    Vp = V rounded up to 128, that the lmhead_ce and lmhead_topk kernels
    stream: one `derived` cache per weight, shared by training and decoding."""
    V, K = weight.shape
    Vp = (V + 127) // 128 * 128

    def fill(Wp):  # padded bf16 vocab weight: rows >= V stay zero
        # from the optimizer's bf16 shadow when present: a bf16->bf16
        # copy is 2/3 the traffic of the fp32 cast at V=32100
        src = _shadow_w16(weight)
        Wp[:V].copy_(src if src is not None else weight.detach())

    return derived(
        weight, "_dfa_vocab_cache", (weight,),
        lambda: torch.zeros(Vp, K, dtype=torch.bfloat16, device=weight.device),
        fill)


class _LMHeadCE(torch.autograd.Function):
    """K21: fused LM-head GEMM + cross-entropy over the 32100-token vocab
    (csrc/lmhead_ce.hip). Forward streams vocab tiles with online
    logsumexp — logits are never materialized (the reference call site,
    CodeT5/models.py:140-149, materializes b*512*32100 fp32 twice).
    Backward recomputes tiles into scaled bf16 dlogits, then dh/dW are two
    library GEMMs. Semantics == F.cross_entropy(logits.float(), targets,
    ignore_index=-100) with logits = scale * h @ W^T (mean over valid)."""

    @staticmethod
    def forward(ctx, h, weight, targets, scale):
        ext = load_ext(required=True)
        K = h.shape[-1]
        h2d = h.reshape(-1, K).to(torch.bfloat16).contiguous()
        V = weight.shape[0]
        Wp = _vocab_padded(weight)
        tgt = targets.reshape(-1).to(torch.int32)
        tgt = torch.where(tgt == -100, tgt.new_full((), -1), tgt).contiguous()
        loss_rows, lse = ext.lmhead_ce_fwd(h2d, Wp, tgt, float(scale), V)
        n_valid = (tgt >= 0).sum().to(torch.float32).clamp(min=1.0)
        loss = loss_rows.sum() / n_valid
        ctx.save_for_backward(h2d, Wp, tgt, lse, n_valid)
        ctx.scale = float(scale)
        ctx.V = V
        ctx.h_shape = h.shape
        ctx.h_dtype = h.dtype
        ctx.w_dtype = weight.dtype
        return loss

    @staticmethod
    def backward(ctx, grad):
        ext = load_ext(required=True)
        h2d, Wp, tgt, lse, n_valid = ctx.saved_tensors
        # fold the chain scale into gscale once: it multiplies both dh and dW
        g = grad.float() * ctx.scale / n_valid
        gscale = torch.where(tgt >= 0, g, torch.zeros_like(g)).contiguous()
        dlogits = ext.lmhead_ce_bwd(h2d, Wp, tgt, lse, gscale, ctx.scale, ctx.V)
        dh = torch.matmul(dlogits, Wp)            # (M, K) bf16
        dw = torch.matmul(dlogits.t(), h2d)       # (Vp, K) bf16
        return (
            dh.view(ctx.h_shape).to(ctx.h_dtype),
            dw[: ctx.V].to(ctx.w_dtype),
            None,
            None,
        )


def lmhead_ce_usable(h, weight) -> bool:
    if not (h.is_cuda and load_ext() is not None):
        return False
    M = h.numel() // h.shape[-1]
    return M % 128 == 0 and h.shape[-1] % 64 == 0


def lmhead_cross_entropy(h, weight, targets, scale: float = 1.0):
    """Mean CE over rows where target != -100, logits = scale * h @ W^T."""
    if lmhead_ce_usable(h, weight):
        return _LMHeadCE.apply(h, weight, targets, scale)
    logits = torch.nn.functional.linear(h.reshape(-1, h.shape[-1]) * scale, weight)
    return torch.nn.functional.cross_entropy(
        logits.float(), targets.reshape(-1), ignore_index=-100
    )


LMHEAD_TOPK_MAX_K = 16  # the kernel's candidate lists live in registers


def _check_topk_k(k, V):
    if not 1 <= k <= LMHEAD_TOPK_MAX_K:
        raise ValueError(f"lmhead_topk: k = {k} outside [1, {LMHEAD_TOPK_MAX_K}]")
    if k > V:
        raise ValueError(f"lmhead_topk: k = {k} exceeds the vocabulary size {V}")


def lmhead_topk_usable(h, weight, k) -> bool:
    """True where lmhead_topk_kernel (csrc/lmhead_topk.hip) serves the call:
    GPU, the extension built, hidden size a multiple of 64, 1 <= k <= 16 and
    k <= V. The row count is free."""
    return (
        h.is_cuda
        and weight.is_cuda
        and load_ext() is not None
        and h.shape[-1] % 64 == 0
        and 1 <= k <= min(LMHEAD_TOPK_MAX_K, weight.shape[0])
    )


def lmhead_topk(h, weight, k, scale: float = 1.0, chunk_tiles: Optional[int] = None):
    """(val, idx, lse) of the LM head for one decoding step, logits =
    scale * h @ weight^T never materialised: val (M, k) fp32 the k largest
    logits of each row (as logits, not log-probabilities), idx (M, k) int32
    their columns, lse (M,) fp32 the row's logsumexp. Order within a row:
    value descending, and among bit-equal values the smaller column first.
    1 <= k <= 16 and k <= V, else ValueError. Inference only.

    On the GPU (lmhead_topk_usable) h is read in bf16 against the cached
    padded bf16 vocabulary matrix of lmhead_cross_entropy and ranking happens
    on the fp32 accumulators; `chunk_tiles` pins the kernel's vocabulary chunk
    (in 128-column tiles) instead of the launcher's choice. Elsewhere the same
    contract in plain torch, in fp32 (fp64 for fp64 inputs)."""
    _no_grad_inputs("lmhead_topk", h, weight)
    V = weight.shape[0]
    _check_topk_k(k, V)
    with torch.no_grad():
        h2d = h.reshape(-1, h.shape[-1])
        if lmhead_topk_usable(h2d, weight, k):
            ext = load_ext(required=True)
            val, idx, lse = ext.lmhead_topk(h2d.to(torch.bfloat16).contiguous(),
                                            _vocab_padded(weight), V, float(scale), int(k),
                                            int(chunk_tiles or 0))
            return val, idx, lse
        if h.is_cuda:
            raise RuntimeError("lmhead_topk: no kernel serves this call on the GPU "
                               f"(hidden size {h.shape[-1]}, k = {k})")
        ct = _decode_compute_dtype(h2d)
        logits = (h2d.to(ct) @ weight.detach().to(ct).t()) * scale
        lse = torch.logsumexp(logits, dim=-1)
        # a stable descending sort keeps equal values in column order
        val, idx = torch.sort(logits, dim=-1, descending=True, stable=True)
        return val[:, :k].contiguous(), idx[:, :k].to(torch.int32).contiguous(), lse


def beam_select(val, idx, lse, beam_scores, done, fill_token, eos):
    """One beam-search selection step over the candidates of lmhead_topk.

    val, idx (B*K, K), lse (B*K,), beam_scores (B, K), done (B*K,) bool; row
    r = b * K + p is beam p of source b. A live row offers K candidates
    beam_scores[r] + (val[r, c] - lse[r]) with token idx[r, c]; a finished row
    offers exactly one, `fill_token` at beam_scores[r] unchanged. Each source
    keeps its best K by total descending, then parent beam ascending, then
    candidate rank ascending. Returns (scores (B, K), parent (B*K,) int64 flat
    row indices, tok (B*K,) int64, done (B*K,) bool = done[parent] |
    (tok == eos)). K = 1 is greedy decoding. Inference only.

    On the GPU this is beam_select_kernel (fp32, K <= 16); elsewhere plain
    torch with the same arithmetic and order."""
    _no_grad_inputs("beam_select", val, lse, beam_scores)
    B, K = beam_scores.shape
    if val.shape != (B * K, K) or idx.shape != val.shape or lse.shape != (B * K,) \
            or done.shape != (B * K,):
        raise ValueError("beam_select: val, idx (B*K, K), lse, done (B*K,), beam_scores (B, K)")
    with torch.no_grad():
        if val.is_cuda:
            ext = load_ext(required=True)
            scores, parent, tok, done_new = ext.beam_select(
                val.float().contiguous(), idx.to(torch.int32).contiguous(),
                lse.float().contiguous(), beam_scores.float().contiguous(),
                done.contiguous(), int(fill_token), int(eos))
            return scores, parent, tok, done_new
        dev = val.device
        fin = done.view(B * K, 1)
        total = beam_scores.reshape(B * K, 1) + (val - lse.view(-1, 1))
        total = torch.where(fin, beam_scores.reshape(B * K, 1).expand_as(total), total)
        offered = ~fin | (torch.arange(K, device=dev).view(1, K) == 0)
        # candidates a finished row does not offer sort last: (offered, total)
        # is the key, flat position p * K + c the stable tie order
        key = total.masked_fill(~offered, float("-inf")).view(B, K * K)
        order = torch.sort(key, dim=-1, descending=True, stable=True).indices
        off_sorted = offered.view(B, K * K).gather(1, order)
        # among equal keys of -inf, offered candidates must precede the rest
        order = order.gather(1, torch.sort((~off_sorted).to(torch.int8), dim=-1,
                                           stable=True).indices)[:, :K]
        scores = total.view(B, K * K).gather(1, order)
        parent = (torch.arange(B, device=dev).view(B, 1) * K + order // K).view(-1)
        tok = idx.view(B, K * K).gather(1, order).view(-1).long()
        tok = torch.where(done[parent], torch.full_like(tok, fill_token), tok)
        return scores, parent, tok, done[parent] | (tok == eos)


class _ReluDropout(torch.autograd.Function):
    """Fused ReLU + dropout (T5 FFN inner activation): stateless mask from
    the seed, only the pre-ReLU input saved."""

    @staticmethod
    def forward(ctx, x, p, training):
        ext = load_ext(required=True)
        seed = _next_seed() if (training and p > 0) else 0
        pp = p if training else 0.0
        xc = x.contiguous()
        out = ext.relu_dropout_fwd(xc, pp, seed)
        ctx.save_for_backward(xc)
        ctx.p = pp
        ctx.seed = seed
        return out

    @staticmethod
    def backward(ctx, dy):
        ext = load_ext(required=True)
        (x,) = ctx.saved_tensors
        dx = ext.relu_dropout_bwd(dy.contiguous(), x, ctx.p, ctx.seed)
        return dx, None, None


def relu_dropout(x, p=0.0, training=True):
    """dropout(relu(x)); fused on GPU when numel fills whole 16-B vectors,
    torch composition elsewhere (as dropout_add)."""
    if x.is_cuda and x.numel() % (4 if x.dtype == torch.float32 else 8) == 0:
        return _ReluDropout.apply(x, p, training)
    h = torch.relu(x)
    return torch.nn.functional.dropout(h, p) if (training and p > 0) else h
