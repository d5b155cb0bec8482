"""CPU tests of the in-place, beam-indexed decode path: the float64 oracle
(tests/decode_attn_oracle.py), the distance-indexed bias table, the torch
implementation of ops.decode_self_attention / decode_cross_attention, and
generate(kv_cache="indirect") against the "concat" path.
"""

import math

import pytest
import torch

import decode_attn_oracle as DO
from deepdfa_amd.models.t5 import T5Attention, T5Config, T5ForConditionalGeneration
from deepdfa_amd.ops import (decode_attention_usable, decode_cross_attention,
                             decode_self_attention)

H, D, TMAX = 3, 3 * 64, 12
# beams 3, two sources: the rows permute (step 0), duplicate and drop (1, 2, 4),
# stay (3) and cross over again (5, 6)
PARENTS = [
    [1, 2, 0, 5, 3, 4],
    [0, 0, 1, 4, 4, 4],
    [2, 2, 2, 3, 5, 5],
    [0, 1, 2, 3, 4, 5],
    [1, 1, 0, 5, 4, 5],
    [2, 0, 1, 4, 3, 5],
    [1, 0, 0, 3, 3, 4],
]
R, BEAMS = 6, 3


def _scripted_run(dtype=torch.float32, seed=11):
    """Runs the op for len(PARENTS) + 1 steps the way the model does (store,
    attend, reorder anc) and records every step's inputs and output."""
    g = torch.Generator().manual_seed(seed)
    kc = torch.zeros(R, TMAX, D, dtype=dtype)
    vc = torch.zeros(R, TMAX, D, dtype=dtype)
    rows = torch.arange(R, dtype=torch.int32)
    anc = rows.unsqueeze(1).repeat(1, TMAX)
    bias = DO.random_bias_dist(H, TMAX, g)
    steps = []
    for pos in range(len(PARENTS) + 1):
        q, kn, vn = (torch.randn(R, D, generator=g).to(dtype) * 0.5 for _ in range(3))
        before = (kc.clone(), vc.clone(), anc.clone())
        anc[:, pos] = rows
        out = decode_self_attention(q, kn, vn, kc, vc, anc, bias, pos, H, 1.0)
        steps.append(dict(q=q, kn=kn, vn=vn, kc=before[0], vc=before[1], anc=before[2],
                          pos=pos, out=out))
        if pos < len(PARENTS):
            anc = anc[torch.tensor(PARENTS[pos])].contiguous()
    return steps, bias, kc, vc, anc


def _dense_history_reference(steps, bias):
    """Independent of the oracle and of anc: every row carries its OWN copy
    of its history, copied whole on each reorder (what the concat path does),
    and attention is a python loop over rows and heads in float64."""
    hist_k = [[] for _ in range(R)]
    hist_v = [[] for _ in range(R)]
    outs = []
    for st in steps:
        pos = st["pos"]
        o = torch.zeros(R, H, 64, dtype=torch.float64)
        for r in range(R):
            hist_k[r].append(st["kn"][r].double())
            hist_v[r].append(st["vn"][r].double())
            K = torch.stack(hist_k[r]).view(pos + 1, H, 64)
            V = torch.stack(hist_v[r]).view(pos + 1, H, 64)
            for h in range(H):
                qh = st["q"][r].double().view(H, 64)[h]
                s = torch.stack([(qh * K[j, h]).sum() + bias[h, pos - j].double()
                                 for j in range(pos + 1)])
                p = torch.exp(s - s.max())
                p = p / p.sum()
                o[r, h] = (p.unsqueeze(1) * V[:, h]).sum(0)
        outs.append(o)
        if pos < len(PARENTS):
            par = PARENTS[pos]
            hist_k = [list(hist_k[p]) for p in par]
            hist_v = [list(hist_v[p]) for p in par]
    return outs


def test_history_script_permutes_duplicates_and_drops():
    assert len(PARENTS) >= 6
    assert any(sorted(p) == list(range(R)) and p != list(range(R)) for p in PARENTS)
    assert any(len(set(p)) < R for p in PARENTS)          # a duplicate, so a drop as well
    for p in PARENTS:                                     # beams stay with their source
        assert all(a // BEAMS == r // BEAMS for r, a in enumerate(p))


def test_oracle_matches_dense_history():
    steps, bias, *_ = _scripted_run()
    dense = _dense_history_reference(steps, bias)
    for st, ref in zip(steps, dense):
        O, P, S, _, _ = DO.decode_self_exact(st["q"], st["kn"], st["vn"], st["kc"], st["vc"],
                                             st["anc"], bias, st["pos"], H, 1.0)
        assert tuple(P.shape) == (R, H, st["pos"] + 1)
        assert torch.allclose(P.sum(-1), torch.ones(R, H, dtype=torch.float64), atol=1e-14)
        assert float((O - ref).abs().max()) <= 1e-13
    # the helper that builds the table in one go agrees with the stepwise table
    final = DO.anc_from_parents(PARENTS, R, TMAX)
    assert torch.equal(final[:, :len(PARENTS)], steps[-1]["anc"][:, :len(PARENTS)])


def test_cross_oracle_matches_dense():
    g = torch.Generator().manual_seed(5)
    B, Lk = 2, 10
    q = torch.randn(B * BEAMS, D, generator=g)
    k = torch.randn(B, Lk, D, generator=g)
    v = torch.randn(B, Lk, D, generator=g)
    valid = torch.tensor([7, 0], dtype=torch.int32)
    O, P, _, _, _ = DO.decode_cross_exact(q, k, v, valid, BEAMS, H, 0.5)
    for r in range(B * BEAMS):
        b = r // BEAMS
        n = int(valid[b])
        for h in range(H):
            if n == 0:
                assert bool((O[r, h] == 0).all()) and bool((P[r, h] == 0).all())
                continue
            qh = q[r].double().view(H, 64)[h]
            s = torch.stack([(qh * k[b, j].double().view(H, 64)[h]).sum() * 0.5 for j in range(n)])
            p = torch.exp(s - s.max())
            p = p / p.sum()
            ref = (p.unsqueeze(1) * v[b, :n].double().view(n, H, 64)[:, h]).sum(0)
            assert float((O[r, h] - ref).abs().max()) <= 1e-13
            assert bool((P[r, h, n:] == 0).all())


@pytest.mark.parametrize("t", [1, 2, 33, 129, 160])
def test_bias_table_equals_last_row_of_compute_bias(t):
    torch.manual_seed(0)
    cfg = T5Config(num_heads=H)
    attn = T5Attention(cfg, has_relative_attention_bias=True, causal=True)
    table = attn.decode_bias_table(160, torch.device("cpu"))
    assert table.dtype == torch.float32 and tuple(table.shape) == (H, 160) and table.is_contiguous()
    with torch.no_grad():
        full = attn.compute_bias(t, t, torch.device("cpu"))
    j = torch.arange(t)
    assert torch.equal(table[:, t - 1 - j], full[0, :, t - 1, j])
    if t == 160:      # every bucket regime is in the table: exact, log-spaced, saturated
        nb = cfg.relative_attention_num_buckets
        w = attn.relative_attention_bias.weight
        assert torch.equal(table[:, 5], w[5]) and torch.equal(table[:, 159], w[nb - 1])
        assert torch.equal(table[:, 128], w[nb - 1]) and not torch.equal(table[:, 40], w[nb - 1])


def test_cpu_self_op_against_oracle():
    steps, bias, kc, vc, _ = _scripted_run()
    worst = 0.0
    for st in steps:
        O, P, _, _, Vh = DO.decode_self_exact(st["q"], st["kn"], st["vn"], st["kc"], st["vc"],
                                              st["anc"], bias, st["pos"], H, 1.0)
        # fp32 evaluation of a T-term softmax and a 64-term dot product
        T = st["pos"] + 1
        tol = (64 + 2 * T + 16) * 2.0 ** -23 * torch.einsum("rht,rthd->rhd", P, Vh.abs()) + 1e-30
        err = (st["out"].double().view(R, H, 64) - O).abs()
        worst = max(worst, float((err / tol).max()))
        assert bool((err <= tol).all())
    print(f"[bound] cpu self op: max err / tol {worst:.3f}")
    # the cache holds every step's new rows where they were written, nothing moved
    for st in steps:
        assert torch.equal(kc[:, st["pos"]], st["kn"]) and torch.equal(vc[:, st["pos"]], st["vn"])
    assert bool((kc[:, len(steps):] == 0).all())


def test_cpu_self_op_identity_and_no_bias():
    g = torch.Generator().manual_seed(3)
    kc = torch.randn(4, 8, D, generator=g)
    vc = torch.randn(4, 8, D, generator=g)
    q, kn, vn = (torch.randn(4, D, generator=g) for _ in range(3))
    ref, P, _, _, Vh = DO.decode_self_exact(q, kn, vn, kc, vc, None, None, 5, H, 0.125)
    out = decode_self_attention(q, kn, vn, kc, vc, None, None, 5, H, 0.125)
    tol = 128 * 2.0 ** -23 * torch.einsum("rht,rthd->rhd", P, Vh.abs())
    assert bool(((out.double().view(4, H, 64) - ref).abs() <= tol).all())
    out64 = decode_self_attention(q.double(), kn.double(), vn.double(), kc.double(), vc.double(),
                                  None, None, 5, H, 0.125)
    assert out64.dtype == torch.float64
    assert float((out64.view(4, H, 64) - ref).abs().max()) <= 1e-13
    with pytest.raises(ValueError):
        decode_self_attention(q, kn, vn, kc, vc, None, None, 8, H, 1.0)


def test_cpu_cross_op_against_oracle():
    g = torch.Generator().manual_seed(9)
    B, Lk = 2, 37
    q = torch.randn(B * BEAMS, D, generator=g) * 0.5
    kv = torch.randn(B, Lk, 2 * D, generator=g) * 0.5
    k, v = kv[..., :D], kv[..., D:]                     # slices of one fused buffer
    for valid in (None, torch.tensor([37, 5], dtype=torch.int32),
                  torch.tensor([0, 1], dtype=torch.int32)):
        ref, P, _, _, Vh = DO.decode_cross_exact(q, k, v, valid, BEAMS, H, 1.0)
        out = decode_cross_attention(q, k, v, valid, BEAMS, H, 1.0)
        assert out.dtype == q.dtype and tuple(out.shape) == (B * BEAMS, D)
        tol = (64 + 2 * Lk + 16) * 2.0 ** -23 * torch.einsum("rht,rthd->rhd", P, Vh.abs()) + 1e-30
        assert bool(((out.double().view(-1, H, 64) - ref).abs() <= tol).all())
        if valid is not None and int(valid[0]) == 0:
            assert bool((out[:BEAMS] == 0).all())      # exact zeros, not NaN
    with pytest.raises(ValueError):
        decode_cross_attention(q[:5], k, v, None, BEAMS, H, 1.0)


def test_usable_is_gpu_bf16_d64_only():
    x = torch.zeros(2, 64)
    assert not decode_attention_usable(x, 64)
    assert not decode_attention_usable(x.bfloat16(), 64)     # not on a GPU


def test_grad_guard():
    g = torch.Generator().manual_seed(1)
    kc, vc = torch.zeros(2, 4, D), torch.zeros(2, 4, D)
    q, kn, vn = (torch.randn(2, D, generator=g) for _ in range(3))
    leaf = q.clone().requires_grad_()
    with pytest.raises(ValueError):
        decode_self_attention(leaf, kn, vn, kc, vc, None, None, 0, H, 1.0)
    with pytest.raises(ValueError):
        decode_self_attention(q, kn.clone().requires_grad_(), vn, kc, vc, None, None, 0, H, 1.0)
    k = torch.randn(2, 5, D, generator=g)
    with pytest.raises(ValueError):
        decode_cross_attention(leaf, k, k, None, 1, H, 1.0)
    with pytest.raises(ValueError):
        decode_cross_attention(q, k.clone().requires_grad_(), k, None, 1, H, 1.0)
    with torch.no_grad():                                    # fine without grad mode
        out = decode_self_attention(leaf, kn, vn, kc, vc, None, None, 0, H, 1.0)
        decode_cross_attention(leaf, k, k, None, 1, H, 1.0)
    assert not out.requires_grad
    assert torch.equal(out, vn)                              # one key: the output is its value


# --------------------------------------------------------------------------
# token equality of the two cache modes
# --------------------------------------------------------------------------

GEN_SEED = 27   # the first seed whose smallest gap is above 5e-3 for all three beam widths
MAX_LEN = 12
MARGIN = 1e-3


def _gen_model():
    """TestKVCachedGeneration's size. The LM head is untied and the weights
    scaled up so that the model emits a varied token stream (the tied
    random-init model repeats token 0, which would make beam ancestry
    trivial)."""
    torch.manual_seed(GEN_SEED)
    cfg = T5Config(num_layers=2, num_decoder_layers=2, d_model=64, d_ff=128, num_heads=2,
                   vocab_size=200, tie_word_embeddings=False)
    m = T5ForConditionalGeneration(cfg).eval()
    with torch.no_grad():
        for p in m.parameters():
            if p.dim() == 2:
                p.mul_(2.0)
    ids = torch.randint(3, cfg.vocab_size, (3, 24))
    ids[:, -1] = cfg.eos_token_id
    ids[0, 12:] = cfg.pad_token_id      # ragged sources: the cross-attention mask matters
    ids[2, 20:] = cfg.pad_token_id
    return m, cfg, ids


def _concat_gaps(m, cfg, ids, beams):
    """Runs generate(kv_cache="concat") with a hook on the LM head and replays
    its selection from the recorded logits: the smallest gap, over all steps
    and sources, between the last candidate it keeps and the first it drops.
    Also returns whether any step's parents were not the identity."""
    logits = []
    hook = m.lm_head.register_forward_hook(lambda mod, inp, out: logits.append(out.detach().clone()))
    try:
        seq = m.generate(ids, max_length=MAX_LEN, num_beams=beams, kv_cache="concat")
    finally:
        hook.remove()
    B = ids.shape[0]
    gap, moved = math.inf, False
    if beams == 1:
        done = torch.zeros(B, dtype=torch.bool)
        for lg in logits:
            top = lg.topk(2, dim=-1).values
            gap = min(gap, float((top[:, 0] - top[:, 1])[~done].min()))
            done |= lg.argmax(-1) == cfg.eos_token_id
        return seq, gap, moved
    K = beams
    scores = torch.full((B, K), -1e9)
    scores[:, 0] = 0.0
    done = torch.zeros(B * K, dtype=torch.bool)
    for lg in logits:
        logp = torch.log_softmax(lg, -1).masked_fill(done.unsqueeze(1), 0.0)
        V = logp.shape[-1]
        total = (scores.reshape(-1, 1) + logp).view(B, K * V)
        top, idx = total.topk(K + 1, dim=-1)
        gap = min(gap, float((top[:, :-1] - top[:, 1:]).min()))
        beam_idx, tok = idx[:, :K] // V, idx[:, :K] % V
        moved |= not torch.equal(beam_idx, torch.arange(K).expand(B, K))
        src = (torch.arange(B).unsqueeze(1) * K + beam_idx).view(-1)
        done = done[src] | (tok.reshape(-1) == cfg.eos_token_id)
        scores = top[:, :K]
    return seq, gap, moved


@pytest.mark.parametrize("beams", [1, 3, 4])
def test_indirect_generates_the_same_tokens(beams):
    m, cfg, ids = _gen_model()
    with torch.no_grad():
        want, gap, moved = _concat_gaps(m, cfg, ids, beams)
        # every kept candidate beats the next one by a margin far above the
        # fp32 differences between the two paths: equality is not luck
        print(f"[gap] beams {beams}: smallest selection gap {gap:.4f}")
        assert gap > MARGIN
        if beams > 1:
            assert moved, "the beams never reordered: the test would not see the indirection"
        assert want.unique().numel() > 4
        got = m.generate(ids, max_length=MAX_LEN, num_beams=beams, kv_cache="indirect")
        auto = m.generate(ids, max_length=MAX_LEN, num_beams=beams)
    assert torch.equal(got, want)
    assert torch.equal(auto, want)          # on the CPU "auto" is the concat path


def test_generate_rejects_unknown_mode():
    m, cfg, ids = _gen_model()
    with pytest.raises(ValueError):
        m.generate(ids, max_length=4, kv_cache="paged")
