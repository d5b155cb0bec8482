from ._ext import has_ext, load_ext
from .flowgnn import attn_pool, embed4, gru_cell, segment_max, spmm_sum
from .transformer import (
    attention_received,
    beam_select,
    lmhead_topk,
    lmhead_topk_usable,
    decode_attention_usable,
    decode_cross_attention,
    decode_self_attention,
    flash_attention_received,
    flash_attention_received_qkv,
    flash_attention_rect,
    flash_attention_rect_kv,
    flash_rect_usable,
)

__all__ = [
    "has_ext",
    "load_ext",
    "embed4",
    "spmm_sum",
    "gru_cell",
    "attn_pool",
    "segment_max",
    "attention_received",
    "flash_attention_received",
    "flash_attention_received_qkv",
    "flash_attention_rect",
    "flash_attention_rect_kv",
    "flash_rect_usable",
    "decode_self_attention",
    "decode_cross_attention",
    "decode_attention_usable",
    "lmhead_topk",
    "lmhead_topk_usable",
    "beam_select",
]
