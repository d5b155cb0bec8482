"""Attention received (column sums of the attention probabilities) on the CPU:
the float64 oracle, the model's `attention_received` output, the batched
line-score driver function and the driver's command line.

1  attn_received_oracle.received_exact against an independent float64
   evaluation (torch.softmax on -inf-masked scores, summed over queries), 1e-12.
2  RobertaModel / linevul.Model with attention_received=True: on the CPU the
   result is written as probs.float().sum(-2), so it is torch.equal to that
   sum of the output_attentions=True probabilities.
3  attention_line_scores_batched against the existing single-example
   attention_line_scores. A line score is a sum of at most H L T non-negative
   fp32 terms (T tokens on the line, L query rows, H heads); two summation
   orders of n non-negative fp32 terms differ by at most n 2^-23 relative, so
   that is the bound.
4  the driver: --do_local_explanation --reasoning_method attention
   --attention_layer 0 runs and writes ifa_records/ifa_attention.txt.
"""

import os

import pytest
import torch

import attn_received_oracle as RO
import flash_oracle as FO
from deepdfa_amd.models.linevul import Model
from deepdfa_amd.models.roberta import RobertaConfig
from deepdfa_amd.train import unixcoder_main as uxc

L = 64


# --------------------------------------------------------------------------
# 1. oracle
# --------------------------------------------------------------------------

@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("with_bias", [False, True])
def test_oracle_against_independent_softmax(causal, with_bias):
    g = torch.Generator().manual_seed(5)
    B, H, Lq, d = 3, 2, 24, 8
    q = torch.randn(B, H, Lq, d, generator=g, dtype=torch.float64)
    k = torch.randn(B, H, Lq, d, generator=g, dtype=torch.float64)
    bias = torch.randn(H, Lq, Lq, generator=g, dtype=torch.float64) if with_bias else None
    valid = torch.tensor([Lq, 7, 0], dtype=torch.int32)
    R, P, lse, s = RO.received_exact(q, k, valid, bias, 0.3, causal)
    assert R.shape == (B, H, Lq) and R.dtype == torch.float64

    sc = 0.3 * torch.einsum("bhid,bhjd->bhij", q, k)
    if with_bias:
        sc = sc + bias
    key = torch.arange(Lq)
    mask = key.view(1, 1, 1, Lq) >= valid.view(B, 1, 1, 1)
    if causal:
        mask = mask | (key.view(1, 1, 1, Lq) > key.view(1, 1, Lq, 1))
    p = torch.softmax(sc.masked_fill(mask, float("-inf")), dim=-1)
    p = torch.nan_to_num(p, nan=0.0)      # dead rows (valid = 0) contribute 0
    ref = p.sum(dim=-2)
    assert float((R - ref).abs().max()) <= 1e-12
    # columns >= valid[b] are exactly 0, the valid = 0 batch row entirely
    for b in range(B):
        assert bool((R[b, :, int(valid[b]):] == 0).all())
    assert bool((R[2] == 0).all()) and bool((lse[2] == 0).all())
    # every live row's probabilities sum to 1, so R sums to the row count
    assert float((R[0].sum(-1) - Lq).abs().max()) <= 1e-12
    assert float((R[1].sum(-1) - Lq).abs().max()) <= 1e-12


def test_op_fallback_matches_oracle():
    """The raw op on the CPU computes the same quantity materialised in fp32;
    lse is ignored there and may be None."""
    from deepdfa_amd.ops import attention_received

    g = torch.Generator().manual_seed(6)
    B, H, Lq = 2, 2, 32
    q = torch.randn(B, Lq, H * 16, generator=g)
    k = torch.randn(B, Lq, H * 16, generator=g)
    bias = torch.randn(H, Lq, Lq, generator=g)             # (H, q, key)
    valid = torch.tensor([Lq, 9], dtype=torch.int32)
    for causal in (False, True):
        got = attention_received(q, k, H, None, valid=valid, bias=FO.bias_to_kernel(bias),
                                 scale=0.25, causal=causal)
        ref = RO.received_exact(FO.to_bhld(q, H), FO.to_bhld(k, H), valid, bias.double(), 0.25,
                                causal)[0]
        assert got.dtype == torch.float32 and got.shape == (B, H, Lq)
        assert float((got.double() - ref).abs().max()) <= 1e-4
        assert bool((got[1, :, 9:] == 0).all())


# --------------------------------------------------------------------------
# 2. model output
# --------------------------------------------------------------------------

def _small_model():
    torch.manual_seed(0)
    cfg = RobertaConfig(vocab_size=1000, hidden_size=128, num_attention_heads=2,
                        num_hidden_layers=2, intermediate_size=256)
    model = Model(config=cfg).eval()
    g = torch.Generator().manual_seed(1)
    ids = torch.randint(3, cfg.vocab_size, (3, L), generator=g)
    ids[:, 0] = 0
    for b, n in enumerate((L, 41, 9)):       # pad lengths, one full row
        ids[b, n:] = cfg.pad_token_id
    return model, ids


def test_model_attention_received_is_column_sum_of_probs():
    model, ids = _small_model()
    with torch.no_grad():
        prob_a, attentions = model(ids, output_attentions=True)
        prob_r, received = model(ids, attention_received=True)
    assert torch.equal(prob_a, prob_r)
    assert isinstance(received, list) and len(received) == len(attentions) == 2
    for R, P in zip(received, attentions):
        assert R.dtype == torch.float32 and R.shape == (3, 2, L)
        assert torch.equal(R, P.float().sum(-2))
    # padded key columns receive nothing
    assert bool((received[0][1, :, 41:] == 0).all()) and bool((received[1][2, :, 9:] == 0).all())

    labels = torch.tensor([0, 1, 1])
    with torch.no_grad():
        loss, prob_l, received_l = model(ids, labels=labels, attention_received=True)
    assert loss.dim() == 0 and torch.equal(prob_l, prob_r)
    assert all(torch.equal(a, b) for a, b in zip(received_l, received))


def test_model_flags_are_exclusive_and_stop_after():
    model, ids = _small_model()
    with pytest.raises(ValueError):
        model(ids, output_attentions=True, attention_received=True)
    with pytest.raises(ValueError):
        model.encoder(ids, output_attentions=True, attention_received=True)
    with torch.no_grad():
        _, full = model.encoder(ids, attention_received=True)
        hidden0, first = model.encoder(ids, attention_received=True, stop_after=0)
    assert len(full) == 2 and len(first) == 1
    assert torch.equal(first[0], full[0])
    assert hidden0.shape == (3, L, 128)


# --------------------------------------------------------------------------
# 3. batched line scores
# --------------------------------------------------------------------------

def _token_lines(ids, pad):
    """8 tokens per line, -1 for CLS, the last real token (SEP) and padding."""
    rows = []
    for b in range(ids.shape[0]):
        n = int((ids[b] != pad).sum())
        rows.append([-1] + [j // 8 for j in range(n - 2)] + [-1] * (L - n + 1))
    return rows


def test_batched_line_scores_match_single_example():
    model, ids = _small_model()
    lines = _token_lines(ids, 1)
    lines_t = torch.tensor(lines, dtype=torch.long)
    got = uxc.attention_line_scores_batched(model, ids, lines_t)          # layer = -1
    n_lines = max(max(r) for r in lines) + 1
    assert got.dtype == torch.float32 and got.shape == (3, n_lines)
    H = 2
    for b in range(3):
        single = uxc.attention_line_scores(model, ids[b], lines[b])
        for ln in range(n_lines):
            T = sum(1 for x in lines[b] if x == ln)
            ref = single.get(ln, 0.0)
            if T == 0:
                assert float(got[b, ln]) == 0.0 and ln not in single
                continue
            tol = H * L * T * 2.0 ** -23 * abs(ref)
            assert abs(float(got[b, ln]) - ref) <= tol, (b, ln, float(got[b, ln]), ref, tol)
    first = uxc.attention_line_scores_batched(model, ids, lines_t, layer=0)
    assert first.shape == got.shape and not torch.equal(first, got)
    assert torch.equal(uxc.attention_line_scores_batched(model, ids, lines_t, layer=1), got)
    with pytest.raises(ValueError):
        uxc.attention_line_scores_batched(model, ids, lines_t, layer=2)


# --------------------------------------------------------------------------
# 4. driver
# --------------------------------------------------------------------------

def test_driver_attention_localization_with_layer_choice(tmp_path):
    out = tmp_path / "uxc"
    res = uxc.main([
        "--do_local_explanation", "--reasoning_method", "attention", "--attention_layer", "0",
        "--n_synthetic", "120", "--num_layers", "1", "--block_size", "64",
        "--eval_batch_size", "8", "--output_dir", str(out),
    ])
    assert {"effort@topk", "recall@topk_loc", "top_k_accuracy", "ifa"} <= set(res)
    rec = out / "ifa_records" / "ifa_attention.txt"
    assert os.path.exists(rec) and rec.read_text().startswith("[")
