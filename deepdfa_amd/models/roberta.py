"""RoBERTa-base encoder (CodeBERT backbone of LineVul), MI355X-native.

Parity target: HF `RobertaModel`/`RobertaForSequenceClassification` as used
by the reference (LineVul/linevul/linevul_model.py:26-69 holds a CodeBERT
`RobertaForSequenceClassification`; linevul_main.py:605-619 loads
microsoft/codebert-base). The module tree and parameter names mirror HF
exactly, so HF state_dicts load 1:1 (tests/test_roberta.py verifies logits
parity against transformers' random-init model).

Compute mapping:
  * QKV / out-proj / FFN projections: rocBLAS/hipBLASLt bf16 GEMMs under
    autocast (plain library GEMMs);
  * scaled masked softmax, LayerNorm, bias+GELU: hand-written HIP kernels
    (deepdfa_amd/ops/transformer.py) with fp32 math;
  * attention scores/context: strided-batched GEMMs; probabilities are
    materialized (needed anyway for the line-level attention-scoring path,
    linevul_model.py:42-48).

Padding contract: suffix padding with pad token id 1 (RoBERTa); the mask is
carried as per-example valid lengths.
"""

from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional

import torch
from torch import nn

from ..ops.transformer import (
    bias_gelu,
    flash_attention,
    flash_attention_rect,
    flash_rect_usable,
    flash_usable,
    fused_linear,
    layer_norm,
    layer_norm_res_dropout,
    masked_softmax_dropout,
)


@dataclass
class RobertaConfig:
    vocab_size: int = 50265
    hidden_size: int = 768
    num_hidden_layers: int = 12
    num_attention_heads: int = 12
    intermediate_size: int = 3072
    max_position_embeddings: int = 514
    type_vocab_size: int = 1
    hidden_dropout_prob: float = 0.1
    attention_probs_dropout_prob: float = 0.1
    layer_norm_eps: float = 1e-5
    pad_token_id: int = 1
    num_labels: int = 2


class LayerNorm(nn.Module):
    """LayerNorm module backed by the HIP kernel (fp32 params)."""

    def __init__(self, dim: int, eps: float = 1e-5):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(dim))
        self.bias = nn.Parameter(torch.zeros(dim))
        self.eps = eps

    def forward(self, x):
        return layer_norm(x, self.weight, self.bias, self.eps)


class Embedding(nn.Embedding):
    # nn.Embedding with the custom scatter-add backward on GPU; keeps
    # the module-call path so forward hooks (saliency scoring) fire
    def forward(self, input):
        from ..ops.transformer import embedding_lookup

        return embedding_lookup(input, self.weight, self.padding_idx)


class RobertaEmbeddings(nn.Module):
    def __init__(self, cfg: RobertaConfig):
        super().__init__()
        self.word_embeddings = Embedding(cfg.vocab_size, cfg.hidden_size, padding_idx=cfg.pad_token_id)
        self.position_embeddings = Embedding(
            cfg.max_position_embeddings, cfg.hidden_size, padding_idx=cfg.pad_token_id
        )
        self.token_type_embeddings = nn.Embedding(cfg.type_vocab_size, cfg.hidden_size)
        self.LayerNorm = LayerNorm(cfg.hidden_size, cfg.layer_norm_eps)
        self.dropout = nn.Dropout(cfg.hidden_dropout_prob)
        self.padding_idx = cfg.pad_token_id

    def forward(self, input_ids):
        mask = input_ids.ne(self.padding_idx).long()
        position_ids = torch.cumsum(mask, dim=1) * mask + self.padding_idx
        # token type is always 0 for this model family: broadcasting row 0
        # gives the identical result with a cheap sum-reduce gradient
        # instead of an all-rows-collide scatter
        emb = (
            self.word_embeddings(input_ids)
            + self.position_embeddings(position_ids)
            + self.token_type_embeddings.weight[0]
        )
        return self.dropout(self.LayerNorm(emb))


class RobertaSelfAttention(nn.Module):
    def __init__(self, cfg: RobertaConfig):
        super().__init__()
        self.num_heads = cfg.num_attention_heads
        self.head_dim = cfg.hidden_size // cfg.num_attention_heads
        self.query = nn.Linear(cfg.hidden_size, cfg.hidden_size)
        self.key = nn.Linear(cfg.hidden_size, cfg.hidden_size)
        self.value = nn.Linear(cfg.hidden_size, cfg.hidden_size)
        self.dropout_p = cfg.attention_probs_dropout_prob
        self.dropout = nn.Dropout(cfg.attention_probs_dropout_prob)  # CPU path

    def forward(self, x, valid: Optional[torch.Tensor], output_attentions: bool = False,
                attention_received: bool = False):
        from ..ops.transformer import fused_qkv

        if attention_received:
            return self._forward_received(x, valid)
        B, L, D = x.shape
        H, d = self.num_heads, self.head_dim
        p = self.dropout_p if self.training else 0.0
        qkv = None
        if d == 64 and not output_attentions and L % 64 == 0:
            qkv = fused_qkv(x, self.query.weight, self.key.weight, self.value.weight,
                            self.query.bias, self.key.bias, self.value.bias)
        if qkv is not None:
            from ..ops.transformer import flash_attention_qkv

            out = flash_attention_qkv(qkv, H, valid=valid,
                                      scale=1.0 / math.sqrt(d), dropout_p=p)
            return out, None
        q = fused_linear(x, self.query.weight, self.query.bias)
        k = fused_linear(x, self.key.weight, self.key.bias)
        v = fused_linear(x, self.value.weight, self.value.bias)
        if d == 64 and not output_attentions and flash_usable(q, L):
            out = flash_attention(q, k, v, H, valid=valid, scale=1.0 / math.sqrt(d),
                                  dropout_p=p)
            return out, None
        if d == 64 and not output_attentions and flash_rect_usable(q, d):
            # lengths off the 64 grid: the general kernels (csrc/flash_rect.hip)
            out = flash_attention_rect(q, k, v, H, valid=valid, scale=1.0 / math.sqrt(d),
                                       dropout_p=p)
            return out, None
        # materialized path: CPU / fp32 / attention-probs output

        def split(t):
            return t.view(B, L, H, d).transpose(1, 2)

        q, k, v = split(q), split(k), split(v)
        scores = torch.matmul(q, k.transpose(-1, -2))
        probs, probs_dropped = masked_softmax_dropout(scores, valid, 1.0 / math.sqrt(d), p)
        ctx = torch.matmul(probs_dropped, v)
        out = ctx.transpose(1, 2).reshape(B, L, D)
        return (out, probs) if output_attentions else (out, None)

    def _forward_received(self, x, valid):
        """(out, R) with R[b, h, j] = sum_i probs[b, h, i, j], fp32 (B, H, L):
        the attention each key token receives (line-level localization).
        Flash-usable inputs stay on the fused kernels and never build the
        (B, H, L, L) probabilities; everything else sums the materialised
        ones. An inference output: no gradient, no dropout."""
        from ..ops.transformer import (
            flash_attention_received,
            flash_attention_received_qkv,
            fused_qkv,
        )

        B, L, D = x.shape
        H, d = self.num_heads, self.head_dim
        scale = 1.0 / math.sqrt(d)
        if d == 64 and flash_usable(x, L):
            with torch.no_grad():
                qkv = fused_qkv(x, self.query.weight, self.key.weight, self.value.weight,
                                self.query.bias, self.key.bias, self.value.bias)
                if qkv is not None:
                    return flash_attention_received_qkv(qkv, H, valid=valid, scale=scale)
                q = fused_linear(x, self.query.weight, self.query.bias)
                k = fused_linear(x, self.key.weight, self.key.bias)
                v = fused_linear(x, self.value.weight, self.value.bias)
                return flash_attention_received(q, k, v, H, valid=valid, scale=scale)
        out, probs = self.forward(x, valid, output_attentions=True)
        return out, probs.float().sum(dim=-2)


class RobertaSelfOutput(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.dense = nn.Linear(cfg.hidden_size, cfg.hidden_size)
        self.LayerNorm = LayerNorm(cfg.hidden_size, cfg.layer_norm_eps)
        self.dropout = nn.Dropout(cfg.hidden_dropout_prob)

    def forward(self, hidden, residual):
        h = fused_linear(hidden, self.dense.weight, self.dense.bias)
        p = self.dropout.p if self.training else 0.0
        return layer_norm_res_dropout(h, residual, self.LayerNorm.weight,
                                      self.LayerNorm.bias, p, self.LayerNorm.eps)


class RobertaAttention(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.self = RobertaSelfAttention(cfg)
        self.output = RobertaSelfOutput(cfg)

    def forward(self, x, valid, output_attentions=False, attention_received=False):
        out, probs = self.self(x, valid, output_attentions, attention_received)
        return self.output(out, x), probs


class RobertaIntermediate(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.dense = nn.Linear(cfg.hidden_size, cfg.intermediate_size)

    def forward(self, x):
        # weight-only GEMM; the bias rides in the fused bias+GELU kernel
        return bias_gelu(fused_linear(x, self.dense.weight), self.dense.bias)


class RobertaOutput(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.dense = nn.Linear(cfg.intermediate_size, cfg.hidden_size)
        self.LayerNorm = LayerNorm(cfg.hidden_size, cfg.layer_norm_eps)
        self.dropout = nn.Dropout(cfg.hidden_dropout_prob)

    def forward(self, hidden, residual):
        h = fused_linear(hidden, self.dense.weight, self.dense.bias)
        p = self.dropout.p if self.training else 0.0
        return layer_norm_res_dropout(h, residual, self.LayerNorm.weight,
                                      self.LayerNorm.bias, p, self.LayerNorm.eps)


class RobertaLayer(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.attention = RobertaAttention(cfg)
        self.intermediate = RobertaIntermediate(cfg)
        self.output = RobertaOutput(cfg)

    def forward(self, x, valid, output_attentions=False, attention_received=False):
        attn_out, probs = self.attention(x, valid, output_attentions, attention_received)
        return self.output(self.intermediate(attn_out), attn_out), probs


class RobertaEncoder(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.layer = nn.ModuleList([RobertaLayer(cfg) for _ in range(cfg.num_hidden_layers)])

    def forward(self, x, valid, output_attentions=False, attention_received=False,
                stop_after: Optional[int] = None):
        """`attention_received` returns, in place of the per-layer
        probabilities, the per-layer (B, H, L) fp32 attention each key
        receives. `stop_after` = index of the last layer to run (None: all);
        the returned hidden state is then that layer's output."""
        if output_attentions and attention_received:
            raise ValueError("output_attentions and attention_received are exclusive")
        collect = output_attentions or attention_received
        all_probs = [] if collect else None
        for i, lyr in enumerate(self.layer):
            x, probs = lyr(x, valid, output_attentions, attention_received)
            if collect:
                all_probs.append(probs)
            if stop_after is not None and i >= stop_after:
                break
        return x, all_probs


class RobertaModel(nn.Module):
    def __init__(self, cfg: RobertaConfig):
        super().__init__()
        self.config = cfg
        self.embeddings = RobertaEmbeddings(cfg)
        self.encoder = RobertaEncoder(cfg)

    def forward(self, input_ids, attention_mask=None, output_attentions=False,
                attention_received=False, stop_after: Optional[int] = None):
        if output_attentions and attention_received:
            raise ValueError("output_attentions and attention_received are exclusive")
        if attention_mask is None:
            attention_mask = input_ids.ne(self.config.pad_token_id)
        valid = attention_mask.sum(dim=1).to(torch.int32)
        x = self.embeddings(input_ids)
        # dtype policy: fp32 master params; under torch.autocast(bf16) the
        # compute dtype is bf16 from the first layer (the custom linear /
        # flash kernels take bf16 activations against fp32 master weights)
        if x.is_cuda and torch.is_autocast_enabled():
            x = x.to(torch.bfloat16)
        hidden, all_probs = self.encoder(x, valid, output_attentions, attention_received,
                                         stop_after)
        return hidden, all_probs


def init_roberta_weights(module, std: float = 0.02):
    """HF RobertaPreTrainedModel._init_weights semantics."""
    for m in module.modules():
        if isinstance(m, nn.Linear):
            m.weight.data.normal_(0.0, std)
            if m.bias is not None:
                m.bias.data.zero_()
        elif isinstance(m, nn.Embedding):
            m.weight.data.normal_(0.0, std)
            if m.padding_idx is not None:
                m.weight.data[m.padding_idx].zero_()
        elif isinstance(m, LayerNorm):
            m.weight.data.fill_(1.0)
            m.bias.data.zero_()
