"""CPU checks of tests/transformer_oracle.py: each float64 oracle against the
op's CPU path in deepdfa_amd/ops/transformer.py, the dropout-mask replica's
statistics, and a proof that the ill-conditioned LayerNorm rows of
test_gpu_transformer_rows.py separate a one-pass variance from a sound one.
"""

import math

import numpy as np
import pytest
import torch

import transformer_oracle as TO
from deepdfa_amd.ops import transformer as T
from oracle_checks import assert_within

F32 = 2.0 ** -24


def _gen(seed=0):
    return torch.Generator().manual_seed(seed)


def _close32(got, ref, terms=1.0, what=""):
    """fp32 agreement: a few ulp of the result plus 8 ulp of the largest
    intermediate magnitude `terms` (a tensor or a number)."""
    bound = 8 * F32 * (ref.abs() + terms)
    assert_within(got, ref, bound, what)


def test_layer_norm_oracle_matches_cpu_op():
    g = _gen(1)
    x = torch.randn(7, 200, generator=g) * 2 + 0.5
    w, b = torch.randn(200, generator=g), torch.randn(200, generator=g)
    ref = TO.layer_norm(x.double(), w.double(), b.double(), 1e-5)
    _close32(T.layer_norm(x, w, b, 1e-5), ref, 4 * w.abs().double(), "layer_norm")


def test_rms_norm_oracle_matches_cpu_op():
    g = _gen(2)
    x = torch.randn(7, 200, generator=g) * 2 + 0.5
    w = torch.randn(200, generator=g)
    ref = TO.rms_norm(x.double(), w.double(), 1e-6)
    _close32(T.rms_norm(x, w, 1e-6), ref, 0.0, "rms_norm")


def test_bias_gelu_oracle_matches_cpu_op():
    g = _gen(3)
    x = torch.randn(5, 64, generator=g) * 4
    b = torch.randn(64, generator=g)
    ref = TO.bias_gelu(x.double(), b.double())
    # fp32 rounds v = x + b before the erf: |gelu'| <= 1.13
    _close32(T.bias_gelu(x, b), ref, 1.13 * (x.abs() + b.abs()).double(), "bias_gelu")


@pytest.mark.parametrize("causal", [False, True])
def test_softmax_oracle_matches_cpu_op(causal):
    g = _gen(4)
    S = torch.randn(3, 2, 8, 8, generator=g) * 3
    S[1, 0, 2] = -float("inf")
    valid = torch.tensor([8, 5, 0], dtype=torch.int32)
    P, Pd = TO.masked_softmax_dropout(S.double(), valid, 0.125, causal=causal)
    p, pd = T.masked_softmax_dropout(S, valid, 0.125, 0.0, causal)
    _close32(p, P, 1e-3, "P")  # 1e-3: the rounding of s - m, |s - m| < 100
    assert torch.equal(P, Pd)
    assert float(P[2].abs().max()) == 0.0 and float(P[1, 0, 2].abs().max()) == 0.0
    assert float(P[1, :, :, 5:].abs().max()) == 0.0
    rows = P.sum(-1)
    assert bool(((rows - 1).abs() < 1e-12)[0].all())


def test_softmax_oracle_applies_keep_and_scale():
    S = torch.zeros(1, 1, 1, 8, dtype=torch.float64)
    keep = TO.keep_tensor((1, 1, 1, 8), 5, 0.5)
    _, Pd = TO.masked_softmax_dropout(S, None, 1.0, keep, TO.drop_scale(0.5))
    assert torch.equal(Pd, keep * 2.0 / 8.0)


def test_ln_res_dropout_and_residual_oracles_match_cpu_ops():
    g = _gen(5)
    h, r = torch.randn(4, 256, generator=g), torch.randn(4, 256, generator=g)
    w, b = torch.randn(256, generator=g), torch.randn(256, generator=g)
    ref = TO.layer_norm_res_dropout(h.double(), r.double(), w.double(), b.double(), 1e-5)
    _close32(T.layer_norm_res_dropout(h, r, w, b, 0.0, 1e-5), ref, 4 * w.abs().double(), "lnrd")
    assert torch.equal(T.dropout_add(h, r, 0.0).double(),
                       (r + h).double())
    _close32(T.dropout_add(h, r, 0.0), TO.dropout_add(h.double(), r.double()), 0.0, "dropout_add")
    x = torch.tensor([-1.0, -0.0, 0.0, 1e-30, -1e-30, 2.5])
    assert torch.equal(T.relu_dropout(x, 0.0).double(), TO.relu_dropout(x.double()))
    keep = TO.keep_tensor((6,), 9, 0.5)
    assert torch.equal(TO.relu_dropout(x.double(), keep, 2.0), torch.relu(x).double() * keep * 2)


def test_relu_oracle_gradient_is_zero_at_zero():
    x = torch.tensor([-1.0, -0.0, 0.0, 1e-30, 3.0], dtype=torch.float64, requires_grad=True)
    TO.relu_dropout(x).sum().backward()
    assert x.grad.tolist() == [0.0, 0.0, 0.0, 1.0, 1.0]


@pytest.mark.parametrize("padding_idx", [None, 3])
def test_embed_scatter_oracle_matches_embedding_backward(padding_idx):
    g = _gen(6)
    idx = torch.randint(0, 10, (4, 9), generator=g)
    idx[0, :4] = 3
    w = torch.randn(10, 16, dtype=torch.float64, requires_grad=True)
    dY = torch.randn(4, 9, 16, generator=g, dtype=torch.float64)
    T.embedding_lookup(idx, w, padding_idx).backward(dY)
    ref = TO.embed_scatter(dY, idx, 10, padding_idx)
    assert_within(w.grad, ref, 1e-13 * (1 + ref.abs()), "embed_scatter")
    if padding_idx is not None:
        assert float(ref[3].abs().max()) == 0.0


def test_relbias_oracle_matches_onehot_matmul():
    g = _gen(7)
    H, NB, Q = 3, 8, 6
    buckets = torch.randint(0, NB - 1, (Q, Q), generator=g)  # bucket NB-1 unused
    dbias = torch.randn(H, Q, Q, generator=g, dtype=torch.float64)
    onehot = torch.nn.functional.one_hot(buckets.reshape(-1), NB).double().t()
    ref = TO.relbias_wgrad(dbias, buckets, NB)
    assert_within(onehot @ dbias.reshape(H, -1).t(), ref, 1e-13 * (1 + ref.abs()), "relbias")
    assert float(ref[NB - 1].abs().max()) == 0.0


def test_colsum_oracle():
    x = torch.arange(12, dtype=torch.float64).view(4, 3)
    assert TO.colsum(x).tolist() == [18.0, 22.0, 26.0]


def test_half_ulp():
    m = torch.tensor([1.0, 1.5, 2.0, 3e-3], dtype=torch.float64)
    assert TO.half_ulp(m, torch.float32).tolist()[:3] == [2.0 ** -24, 2.0 ** -24, 2.0 ** -23]
    assert TO.half_ulp(m, torch.bfloat16).tolist()[:3] == [2.0 ** -8, 2.0 ** -8, 2.0 ** -7]
    for dt in (torch.float32, torch.bfloat16):
        v = torch.rand(4096, generator=_gen(8), dtype=torch.float64) * 50
        assert bool(((v.to(dt).double() - v).abs() <= TO.half_ulp(v, dt)).all())


# ---------------------------------------------------------------------------
# keep_mask_np
# ---------------------------------------------------------------------------

def test_hash4_reference_values():
    """Hand-evaluated with Python integers, independent of the NumPy code."""
    def h4(q, seed):
        m = 0xFFFFFFFF
        h = ((q & m) * 2654435761 + (q >> 32) * 40503 + (seed & m) + (seed >> 32) * 97) & m
        h ^= h >> 16
        h = h * 0x7FEB352D & m
        h ^= h >> 15
        h = h * 0x846CA68B & m
        h ^= h >> 16
        return h
    qs = [0, 1, 12345, 2 ** 31 + 7, 2 ** 32 + 5, 2 ** 40 + 3]
    for seed in (0, 1, 0x7FFFFFFFFFFFFFFF, 123456789012345):
        got = TO.hash4_np(np.array(qs, dtype=np.uint64), seed)
        assert [int(v) for v in got] == [h4(q, seed) for q in qs]
    # byte lane = idx & 3 of the quad's hash
    h = h4(3, 77)
    keep = TO.keep_mask_np(np.arange(12, 16), 77, 0.5)
    assert keep.tolist() == [((h >> (8 * i)) & 0xFF) >= 128 for i in range(4)]


@pytest.mark.parametrize("p", [0.1, 0.5, 1.0 / 512])
def test_keep_mask_rate_and_lane_independence(p):
    n = 1 << 20
    keep = TO.keep_mask_np(np.arange(n, dtype=np.uint64), 20240607, p)
    p8 = TO.p8_of(p)
    assert p8 == {0.1: 25, 0.5: 128}.get(p, 0)
    q = (256 - p8) / 256
    if p8 == 0:
        assert keep.all()
        return
    sigma = math.sqrt(q * (1 - q) / n)
    assert abs(keep.mean() - q) <= 4 * sigma
    lanes = keep.reshape(-1, 4).astype(np.float64)
    m = lanes.shape[0]
    for i in range(4):
        assert abs(lanes[:, i].mean() - q) <= 4 * math.sqrt(q * (1 - q) / m)
        for j in range(i + 1, 4):
            # sample correlation of independent lanes: sigma = 1 / sqrt(m)
            r = np.corrcoef(lanes[:, i], lanes[:, j])[0, 1]
            assert abs(r) <= 4 / math.sqrt(m), (i, j, r)


def test_keep_mask_depends_on_seed_and_is_deterministic():
    idx = np.arange(4096, dtype=np.uint64)
    a = TO.keep_mask_np(idx, 11, 0.5)
    assert np.array_equal(a, TO.keep_mask_np(idx, 11, 0.5))
    assert 0.4 < (a != TO.keep_mask_np(idx, 12, 0.5)).mean() < 0.6
    assert TO.drop_scale(0.1) == 256.0 / 231.0 and TO.drop_scale(1 / 512) == 1.0


# ---------------------------------------------------------------------------
# the ill-conditioned rows tell a one-pass variance from a sound one
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["m30", "m100"])
def test_ill_conditioned_rows_catch_one_pass_variance(kind):
    D, eps = 768, 1e-5
    x = TO.ill_rows(kind, 16, D, _gen(9))
    g = _gen(10)
    w, b = 1 + 0.1 * torch.randn(D, generator=g), 0.1 * torch.randn(D, generator=g)
    ref = TO.layer_norm(x.double(), w.double(), b.double(), eps)
    yard = torch.nn.functional.layer_norm(x, (D,), w, b, eps).double()
    # the GPU test's bound: 4 x the yardstick's per-row error, or the
    # conditioning floor where that is larger, plus the output rounding
    core = torch.maximum(4 * (yard - ref).abs().amax(-1, keepdim=True),
                         TO.ln_conditioning_floor(x.double(), ref, eps)).expand_as(ref)
    bound = core + TO.half_ulp(ref.abs() + core, torch.float32)
    assert_within(yard, ref, bound, "torch fp32")
    one = TO.onepass_layer_norm_f32(x, w, b, eps).double()
    bad = ~torch.isfinite(one) | ((one - ref).abs() > bound)
    assert bool(bad.any()), "one-pass variance passes: the rows prove nothing"
    # and not marginally: most rows are out
    assert float(bad.any(-1).double().mean()) > 0.5
