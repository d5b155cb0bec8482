"""Autograd ops for the flow-GNN (K1-K10 of SURVEY.md §2.6).

Each op is a torch.autograd.Function that dispatches to the hand-written
HIP/CDNA4 kernel on GPU (required — no eager fallback on GPU) and to the
fp32 torch reference on CPU. On GPU under bf16 the whole GGNN loop
(ggnn_fused) and both heads (gate_pool + mlp3, node_head) run on the
hand-written MFMA kernels, as do the gathers and segment ops; only the
op-by-op fp32 route (gru_cell, the numerics path) sends its GRU projections
through torch.matmul. Derived-weight caches and direct gradient
accumulation follow ops/_weights.py.
"""

from __future__ import annotations

from typing import Optional

import torch

from . import reference as ref
from ._ext import ext_for, load_ext
from ._weights import _bias_f32, _shadow_w16, derived, direct_grads, packed_shadow


class _Embed4(torch.autograd.Function):
    """K1: fused 4-way embedding gather-concat. tables (4, V, Demb); idx (N, 4)."""

    @staticmethod
    def forward(ctx, tables: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
        ctx.save_for_backward(idx)
        ctx.tables_shape = tables.shape
        ext = ext_for(tables)
        if ext is not None:
            # under autocast emit bf16 straight out of the gather: both
            # consumers (GGNN input, fused head) want bf16, so this removes
            # two cast kernels + their backward casts per step
            out_bf16 = tables.dtype == torch.float32 and torch.is_autocast_enabled()
            return ext.embed4_fwd(tables, idx, out_bf16)
        return ref.embed4_fwd(list(tables), idx)

    @staticmethod
    def backward(ctx, grad_out: torch.Tensor):
        (idx,) = ctx.saved_tensors
        F, V, Demb = ctx.tables_shape
        ext = ext_for(grad_out)
        if ext is not None:
            grad_tables = ext.embed4_bwd(grad_out.contiguous(), idx, V, Demb)
        else:
            grad_tables = torch.stack(
                ref.embed4_bwd(grad_out.float(), idx, V, Demb)
            ).to(grad_out.dtype)
        return grad_tables, None


def embed4(tables: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
    return _Embed4.apply(tables, idx)


class _Embed4Direct(torch.autograd.Function):
    """K1 under the flat optimizer: the (4, V, 32) table stack is a
    ZERO-COPY bf16 view of the optimizer's shadow buffer (the 4 tables are
    adjacent), and the backward scatter-adds straight into the flat fp32
    .grad region — no per-step stack copy, no (4, V, 32) zeros, no unbind
    adds, no dtype casts. `w0` is only the autograd hook that makes the
    output differentiable; its grad is returned as None."""

    @staticmethod
    def forward(ctx, w0, tables16, idx, wrefs):
        ctx.save_for_backward(idx)
        ctx.wrefs = wrefs
        ctx.V = tables16.shape[1]
        ext = ext_for(tables16)
        return ext.embed4_fwd(tables16, idx, False)

    @staticmethod
    def backward(ctx, grad_out):
        (idx,) = ctx.saved_tensors
        ws = ctx.wrefs
        w0 = ws[0]
        n4 = sum(w.numel() for w in ws)
        g4 = w0._dfa_gbase[w0._dfa_goff : w0._dfa_goff + n4]
        ext = ext_for(grad_out)
        ext.embed4_bwd(grad_out.contiguous(), idx, ctx.V, 32, out=g4)
        return None, None, None, None


def embed4_direct_view(ws):
    """Returns the zero-copy (4, V, 32) bf16 stack view of the 4 table
    weights' optimizer shadow, or None when unavailable (no flat optimizer,
    non-adjacent tables, or CPU). Syncs each table's shadow first so a
    torch-level write (checkpoint load) is reflected (_shadow_w16)."""
    n = ws[0].numel()
    if any(w.numel() != n or w.shape[-1] != 32 for w in ws) or not direct_grads(*ws):
        return None
    flat = packed_shadow(ws)
    return None if flat is None else flat.view(4, ws[0].shape[0], 32)


def embed4_direct(ws, idx):
    tables16 = embed4_direct_view(ws)
    if tables16 is None:
        return None
    return _Embed4Direct.apply(ws[0], tables16, idx, ws)


class _SpmmSum(torch.autograd.Function):
    """K2 aggregation: m[v] = sum_{u->v} x[u] over the block-diagonal CSR.
    Backward gathers through the transpose (CSC)."""

    @staticmethod
    def forward(
        ctx,
        x: torch.Tensor,
        indptr: torch.Tensor,
        indices: torch.Tensor,
        t_indptr: torch.Tensor,
        t_indices: torch.Tensor,
    ) -> torch.Tensor:
        ctx.save_for_backward(t_indptr, t_indices)
        ext = ext_for(x)
        if ext is not None:
            return ext.spmm_sum(indptr, indices, x.contiguous())
        return ref.spmm_sum(indptr, indices, x)

    @staticmethod
    def backward(ctx, grad_out: torch.Tensor):
        t_indptr, t_indices = ctx.saved_tensors
        ext = ext_for(grad_out)
        if ext is not None:
            gx = ext.spmm_sum(t_indptr, t_indices, grad_out.contiguous())
        else:
            gx = ref.spmm_sum(t_indptr, t_indices, grad_out)
        return gx, None, None, None, None


def spmm_sum(x, graph) -> torch.Tensor:
    return _SpmmSum.apply(x, graph.indptr, graph.indices, graph.t_indptr, graph.t_indices)


class _GruGates(torch.autograd.Function):
    """K3 fused GRU gate elementwise (the GEMMs producing gi/gh are matmuls)."""

    @staticmethod
    def forward(ctx, gi: torch.Tensor, gh: torch.Tensor, h: torch.Tensor) -> torch.Tensor:
        ext = ext_for(gi)
        if ext is not None:
            h_new, r, z, n = ext.gru_gates_fwd(gi.contiguous(), gh.contiguous(), h.contiguous())
        else:
            h_new, r, z, n = ref.gru_gates_fwd(gi, gh, h)
        ctx.save_for_backward(gh, h, r, z, n)
        return h_new

    @staticmethod
    def backward(ctx, grad_h_new: torch.Tensor):
        gh, h, r, z, n = ctx.saved_tensors
        ext = ext_for(grad_h_new)
        if ext is not None:
            grad_gi, grad_gh, grad_h = ext.gru_gates_bwd(
                grad_h_new.contiguous(), gh, h, r, z, n
            )
        else:
            grad_gi, grad_gh, grad_h = ref.gru_gates_bwd(grad_h_new, gh, h, r, z, n)
        return grad_gi, grad_gh, grad_h


def gru_cell(
    a: torch.Tensor,
    h: torch.Tensor,
    w_ih: torch.Tensor,
    w_hh: torch.Tensor,
    b_ih: Optional[torch.Tensor],
    b_hh: Optional[torch.Tensor],
) -> torch.Tensor:
    """torch.nn.GRUCell-compatible: a is the input (aggregated message)."""
    gi = a @ w_ih.t()
    gh = h @ w_hh.t()
    if b_ih is not None:
        gi = gi + b_ih.to(gi.dtype)
    if b_hh is not None:
        gh = gh + b_hh.to(gh.dtype)
    # under bf16 autocast the matmuls emit bf16 while h may still be fp32
    return _GruGates.apply(gi, gh, h.to(gi.dtype))


def _ggnn_pack_cache(linear: torch.nn.Linear, gru: torch.nn.GRUCell):
    """Derived-weight buffers for the fused GGNN path: bf16 casts of the
    step linear, the block gate matrix Wcat(4H,2H) + transpose, merged
    bias, W_e transpose — all refreshed by ONE pack kernel
    (csrc/flowgnn_kernels.hip pack_gru_weights) under the same
    version/epoch/capture invalidation protocol as the transformer cast
    caches. Replaces the per-call chain of ~26 cast/cat/transpose nodes."""
    ext = load_ext(required=True)
    srcs = (linear.weight, linear.bias, gru.weight_ih, gru.weight_hh,
            gru.bias_ih, gru.bias_hh)
    H = gru.weight_hh.shape[1]

    def alloc():
        shapes = {
            "w_e16": (H, H), "b_e16": (H,), "Wcat": (4 * H, 2 * H),
            "WcatT": (2 * H, 4 * H), "b_cat": (4 * H,), "W_eT": (H, H),
            "Wcat_perm": (4 * H, 2 * H), "b_perm": (4 * H,),
        }
        return {k: torch.empty(shp, dtype=torch.bfloat16, device=gru.weight_hh.device)
                for k, shp in shapes.items()}

    def fill(buf):
        ext.pack_gru_weights(
            *(p.detach() for p in srcs),
            buf["w_e16"], buf["b_e16"], buf["Wcat"], buf["WcatT"], buf["b_cat"],
            buf["W_eT"], buf["Wcat_perm"], buf["b_perm"],
        )

    return derived(gru, "_dfa_pack_cache", srcs, alloc, fill)


class _GGNNFused(torch.autograd.Function):
    """Whole n_steps GGNN loop as one autograd node, driven from C++
    (bindings ggnn_fused_fwd/bwd): per step one MFMA gemm_bias for W_e h,
    the CSR segment-sum, one split-A MFMA GEMM against the block weight
    matrix Wcat producing all GRU gate pre-activations, and a fused gate
    kernel. bf16 compute from cached packed weights; weight grads come
    back fp32 (master dtype) directly — no cast chain in either
    direction."""

    @staticmethod
    def forward(ctx, x, w_e, b_e, w_ih, w_hh, b_ih, b_hh, buf, graph, n_steps):
        ext = load_ext(required=True)
        h_final, HH, M, R, Z, Nn, HN = ext.ggnn_fused_fwd(
            graph.indptr, graph.indices, x, buf["w_e16"], buf["b_e16"],
            buf["Wcat_perm"], buf["b_perm"], n_steps,
        )
        ctx.save_for_backward(x, buf["W_eT"], buf["WcatT"], HH, M, R, Z, Nn, HN,
                              graph.t_indptr, graph.t_indices)
        ctx.n_steps = n_steps
        ctx.grad_dtypes = (w_e.dtype, b_e.dtype, w_ih.dtype, w_hh.dtype,
                           b_ih.dtype, b_hh.dtype)
        ctx.we_refs = (w_e, b_e, w_ih, w_hh, b_ih, b_hh)
        return h_final

    @staticmethod
    def backward(ctx, grad_out):
        ext = load_ext(required=True)
        x, W_eT, WcatT, HH, M, R, Z, Nn, HN, t_indptr, t_indices = ctx.saved_tensors
        params = ctx.we_refs
        if direct_grads(*params):
            w_e, b_e, w_ih, w_hh, b_ih, b_hh = params
            grad_x, *_ = ext.ggnn_fused_bwd(
                grad_out.contiguous(), t_indptr, t_indices, x, W_eT, WcatT,
                HH, M, R, Z, Nn, HN, ctx.n_steps,
                out_we=w_e.grad, out_be=b_e.grad,
                gru_outs=[w_ih.grad, w_hh.grad, b_ih.grad, b_hh.grad],
            )
            # every parameter grad accumulated in-kernel (flat .grad views)
            return (grad_x, None, None, None, None, None, None, None, None, None)
        grad_x, gW_e, gb_e, gW_ih, gW_hh, gb_ih, gb_hh = ext.ggnn_fused_bwd(
            grad_out.contiguous(), t_indptr, t_indices, x, W_eT, WcatT,
            HH, M, R, Z, Nn, HN, ctx.n_steps,
        )
        dts = ctx.grad_dtypes
        grads = [gW_e, gb_e, gW_ih, gW_hh, gb_ih, gb_hh]
        grads = [g if g.dtype == dt else g.to(dt) for g, dt in zip(grads, dts)]
        return (grad_x, *grads, None, None, None)


def ggnn_fused(x, graph, linear: torch.nn.Linear, gru: torch.nn.GRUCell, n_steps: int):
    """bf16 fused GGNN path (GPU only)."""
    buf = _ggnn_pack_cache(linear, gru)
    return _GGNNFused.apply(
        x.to(torch.bfloat16).contiguous(),
        linear.weight, linear.bias, gru.weight_ih, gru.weight_hh,
        gru.bias_ih, gru.bias_hh,
        buf, graph, n_steps,
    )


class _AttnPool(torch.autograd.Function):
    """K5: segment softmax over gate logits + weighted segment sum."""

    @staticmethod
    def forward(
        ctx, x: torch.Tensor, gate_logits: torch.Tensor, node_offsets: torch.Tensor
    ) -> torch.Tensor:
        ext = ext_for(x)
        if ext is not None:
            out, alpha = ext.attn_pool_fwd(
                x.contiguous(), gate_logits.contiguous(), node_offsets
            )
        else:
            out, alpha = ref.attn_pool_fwd(x, gate_logits, node_offsets)
        ctx.save_for_backward(x, alpha, node_offsets)
        return out

    @staticmethod
    def backward(ctx, grad_out: torch.Tensor):
        x, alpha, node_offsets = ctx.saved_tensors
        ext = ext_for(grad_out)
        if ext is not None:
            grad_x, grad_gate = ext.attn_pool_bwd(
                grad_out.contiguous(), x, alpha, node_offsets
            )
        else:
            grad_x, grad_gate = ref.attn_pool_bwd(grad_out, x, alpha, node_offsets)
        return grad_x, grad_gate, None


def attn_pool(x: torch.Tensor, gate_logits: torch.Tensor, graph) -> torch.Tensor:
    node_offsets = graph.node_offsets
    return _AttnPool.apply(x, gate_logits, node_offsets)


def segment_max(values: torch.Tensor, graph) -> torch.Tensor:
    """K7 label reduction (no grad)."""
    if values.is_cuda:
        ext = ext_for(values)
        return ext.segment_max(values.contiguous(), graph.node_offsets)
    return ref.segment_max(values, graph.node_offsets)


class _GatePool(torch.autograd.Function):
    """Fused concat + gate linear + segment-softmax attention pool
    (csrc/graph_head.hip gate_pool_*): replaces cat, the (N,256)@(256,1)
    gate GEMV, attn_pool, and their backward glue (~8 nodes each way).
    Gate weight grads come back fp32 (master dtype)."""

    @staticmethod
    def forward(ctx, x1, x2, wg, bg, node_offsets):
        ext = load_ext(required=True)
        x1c, x2c = x1.contiguous(), x2.contiguous()
        out, alpha, pooled32, gid = ext.gate_pool_fwd(
            x1c, x2c, wg.detach().reshape(-1).contiguous(),
            bg.detach().contiguous(), node_offsets)
        ctx.save_for_backward(x1c, x2c, wg, alpha, node_offsets, pooled32, gid)
        ctx.gparams = (wg, bg)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        ext = load_ext(required=True)
        x1, x2, wg, alpha, node_offsets, pooled32, gid = ctx.saved_tensors
        wgp, bgp = ctx.gparams
        if direct_grads(wgp, bgp):
            gx1, gx2, _, _ = ext.gate_pool_bwd(
                grad_out.contiguous(), x1, x2, wg.detach().reshape(-1).contiguous(),
                alpha, node_offsets, pooled32, gid, out_wg=wgp.grad, out_bg=bgp.grad,
            )
            return gx1, gx2, None, None, None
        gx1, gx2, dwg, dbg = ext.gate_pool_bwd(
            grad_out.contiguous(), x1, x2, wg.detach().reshape(-1).contiguous(),
            alpha, node_offsets, pooled32, gid,
        )
        return gx1, gx2, dwg.view_as(wg).to(wg.dtype), dbg.to(wg.dtype), None


def gate_pool(x1, x2, gate_nn: torch.nn.Linear, graph):
    return _GatePool.apply(x1, x2, gate_nn.weight, gate_nn.bias, graph.node_offsets)


class _MLP3(torch.autograd.Function):
    """Fused [Linear(256,256)+ReLU]x2 + Linear(256,1) head
    (csrc/graph_head.hip mlp3_*, f32-input MFMA, master weights read in
    their native (out, in) layout): one kernel per direction plus one
    kernel for all six parameter grads — replaces ~6 hipBLASLt GEMMs + relu
    fwd/bwd + bias reductions at batch-256 launch-floor sizes."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, w3, b3):
        ext = load_ext(required=True)
        xc = x.contiguous()
        logits, h1, h2 = ext.mlp3_fwd(
            xc, w1.detach().contiguous(), b1.detach().contiguous(),
            w2.detach().contiguous(), b2.detach().contiguous(),
            w3.detach().reshape(-1).contiguous(), b3.detach().contiguous(),
        )
        ctx.save_for_backward(xc, h1, h2, w1, w2, w3)
        ctx.mparams = (w1, b1, w2, b2, w3, b3)
        return logits

    @staticmethod
    def backward(ctx, dlogits):
        ext = load_ext(required=True)
        x, h1, h2, w1, w2, w3 = ctx.saved_tensors
        ps = ctx.mparams
        if direct_grads(*ps):
            (dx,) = ext.mlp3_bwd(
                dlogits.float().contiguous(), x, h1, h2, w1.detach().contiguous(),
                w2.detach().contiguous(), w3.detach().reshape(-1).contiguous(),
                outs=[ps[0].grad, ps[1].grad, ps[2].grad, ps[3].grad,
                      ps[4].grad, ps[5].grad],
            )
            return dx, None, None, None, None, None, None
        dx, dW1, dW2, dW3, db1, db2, db3 = ext.mlp3_bwd(
            dlogits.float().contiguous(), x, h1, h2, w1.detach().contiguous(),
            w2.detach().contiguous(), w3.detach().reshape(-1).contiguous(),
        )
        return dx, dW1, db1, dW2, db2, dW3, db3


def mlp3(x, lin1, lin2, lin3):
    return _MLP3.apply(x, lin1.weight, lin1.bias, lin2.weight, lin2.bias,
                       lin3.weight, lin3.bias)


def _node_head_cache(lin1: torch.nn.Linear, lin2: torch.nn.Linear):
    """bf16 operands of the fused node head, cached per module under the
    usual key/refresh protocol (weight versions + weights epoch): (W1, W2) in
    (out, in) layout — the FlatAdamW shadow views when the flat optimizer
    owns the weights, a cast cache otherwise — and their (in, out)-major
    transposes for the backward's dgrad products. Refreshed IN PLACE while
    CAPTURE_REFRESH is set so a captured step's replays re-derive them
    from the updated master weights."""
    w1, w2 = lin1.weight, lin2.weight
    s1, s2 = _shadow_w16(w1), _shadow_w16(w2)

    def alloc():
        bf, dev = torch.bfloat16, w1.device
        buf = {
            "w1t": torch.empty(w1.shape[::-1], dtype=bf, device=dev),
            "w2t": torch.empty(w2.shape[::-1], dtype=bf, device=dev),
        }
        if s1 is None:
            buf["w1"] = torch.empty(w1.shape, dtype=bf, device=dev)
        if s2 is None:
            buf["w2"] = torch.empty(w2.shape, dtype=bf, device=dev)
        return buf

    def fill(buf):
        if s1 is None:
            buf["w1"].copy_(w1.detach())
        if s2 is None:
            buf["w2"].copy_(w2.detach())
        buf["w1t"].copy_((s1 if s1 is not None else buf["w1"]).t())
        buf["w2t"].copy_((s2 if s2 is not None else buf["w2"]).t())

    buf = derived(lin1, "_dfa_nh_cache", (w1, w2), alloc, fill,
                  extra=(s1 is not None, s2 is not None))
    return (s1 if s1 is not None else buf["w1"],
            s2 if s2 is not None else buf["w2"], buf["w1t"], buf["w2t"])


class _NodeHead(torch.autograd.Function):
    """Fused node-level head (csrc/node_head.hip): split-A concat +
    [Linear(256,256)+ReLU]x2 + Linear(256,1) over every node as ONE MFMA
    kernel per direction. The weight grads reuse ext.wgrad (dW1 against the
    [h|fe] tile image the forward materialises once, dW2 against H1) and
    ext.colsum; dW3/db3 are folded into the backward kernel. On CPU the
    fp32 torch reference (ops/reference.py) runs instead."""

    @staticmethod
    def forward(ctx, h, fe, w1, b1, w2, b2, w3, b3, w16):
        ctx.nparams = (w1, b1, w2, b2, w3, b3)
        ctx.d1 = h.shape[1]
        if not h.is_cuda:
            logits, x, h1, h2 = ref.node_head_fwd(h, fe, w1, b1, w2, b2, w3, b3)
            ctx.save_for_backward(x, h1, h2, w1, w2, w3)
            return logits
        ext = load_ext(required=True)
        w1_16, w2_16, w1t, w2t = w16
        w3f = _bias_f32(w3).reshape(-1)
        save = any(ctx.needs_input_grad)
        outs = ext.node_head_fwd(
            h.contiguous(), fe.contiguous(), w1_16, w2_16, _bias_f32(b1),
            _bias_f32(b2), w3f, _bias_f32(b3), save=save,
        )
        if save:
            _, x, h1, h2 = outs
            ctx.save_for_backward(x, h1, h2, w1t, w2t, w3f)
        return outs[0]

    @staticmethod
    def backward(ctx, dlogits):
        ps = ctx.nparams
        if not dlogits.is_cuda:
            x, h1, h2, w1, w2, w3 = ctx.saved_tensors
            grads = ref.node_head_bwd(dlogits, x, h1, h2, w1, w2, w3, ctx.d1)
            return (*grads, None)
        ext = load_ext(required=True)
        x, h1, h2, w1t, w2t, w3f = ctx.saved_tensors
        dl = dlogits.float().contiguous()
        if direct_grads(*ps):
            # every parameter grad accumulates in-kernel into the flat
            # .grad views (atomic epilogues; a live .grad may already hold
            # an earlier micro-batch's contribution)
            w1, b1, w2, b2, w3, b3 = ps
            dh, dfe, dh1, dh2, _, _ = ext.node_head_bwd(
                dl, h1, h2, w1t, w2t, w3f, out_w3=w3.grad.view(-1), out_b3=b3.grad)
            ext.wgrad(dh1, x, out=w1.grad)
            ext.wgrad(dh2, h1, out=w2.grad)
            ext.colsum(dh1, out=b1.grad)
            ext.colsum(dh2, out=b2.grad)
            return dh, dfe, None, None, None, None, None, None, None
        dh, dfe, dh1, dh2, dW3, db3 = ext.node_head_bwd(dl, h1, h2, w1t, w2t, w3f)
        grads = [ext.wgrad(dh1, x), ext.colsum(dh1), ext.wgrad(dh2, h1),
                 ext.colsum(dh2), dW3.view_as(ps[4]), db3]
        grads = [g if g.dtype == q.dtype else g.to(q.dtype) for g, q in zip(grads, ps)]
        return (dh, dfe, *grads, None)


def node_head(h, fe, lin1: torch.nn.Linear, lin2: torch.nn.Linear,
              lin3: torch.nn.Linear):
    """logits (N,) = lin3(relu(lin2(relu(lin1(cat([h, fe], -1)))))).squeeze(-1).
    GPU: h, fe bf16 (N,128), all widths 256 (checked in the binding)."""
    w16 = _node_head_cache(lin1, lin2) if h.is_cuda else None
    return _NodeHead.apply(h, fe, lin1.weight, lin1.bias, lin2.weight, lin2.bias,
                           lin3.weight, lin3.bias, w16)


class _BCELogits(torch.autograd.Function):
    """Fused BCE-with-logits mean (optional pos_weight + per-graph weight
    mask): one kernel per direction vs torch's ~6-node chain at batch-256
    launch-floor sizes. Semantics == F.binary_cross_entropy_with_logits
    (weighted mean = sum w*bce / sum w)."""

    @staticmethod
    def forward(ctx, logits, labels, weight, pos_weight):
        ext = load_ext(required=True)
        l32 = logits.float().contiguous()
        y32 = labels.float().contiguous()
        w32 = weight.float().contiguous() if weight is not None else None
        pw = pos_weight.float().contiguous() if pos_weight is not None else None
        out2 = ext.bce_logits_fwd(l32, y32, w32, pw)
        ctx.save_for_backward(l32, y32, out2)
        ctx.w32 = w32
        ctx.pw = pw
        return out2[0]

    @staticmethod
    def backward(ctx, grad):
        ext = load_ext(required=True)
        l32, y32, out2 = ctx.saved_tensors
        dlogits = ext.bce_logits_bwd(l32, y32, ctx.w32, ctx.pw,
                                     grad.reshape(1).float().contiguous(), out2)
        return dlogits, None, None, None


def bce_with_logits(logits, labels, weight=None, pos_weight=None):
    if weight is not None and weight.shape != logits.shape:
        # the kernels index weight[i] for every logit
        raise ValueError(
            f"bce_with_logits: weight shape {tuple(weight.shape)} != logits "
            f"shape {tuple(logits.shape)}")
    if logits.is_cuda:
        return _BCELogits.apply(logits, labels, weight, pos_weight)
    if weight is not None:
        per = torch.nn.functional.binary_cross_entropy_with_logits(
            logits, labels, pos_weight=pos_weight, reduction="none")
        return (per * weight).sum() / weight.sum().clamp(min=1.0)
    return torch.nn.functional.binary_cross_entropy_with_logits(
        logits, labels, pos_weight=pos_weight)
