"""The flash attention oracles (tests/flash_oracle.py) proven on the CPU:
attn_exact against torch's scaled_dot_product_attention and gradcheck, the
hand-written backward of attn_emulated against attn_exact's autograd, and the
conventions the GPU tests rely on (dead rows, padded keys, layouts)."""

import math

import pytest
import torch

import flash_oracle as FO

F64 = torch.float64


def _inputs(B, H, L, d=64, seed=0, quantise=True):
    g = torch.Generator().manual_seed(seed)
    mk = lambda s: torch.randn(B, H, L, d, generator=g, dtype=F64) * s  # noqa: E731
    q, k, v, dO = mk(0.5), mk(0.5), mk(0.5), mk(1.0)
    if quantise:
        q, k, v, dO = (FO.bf16_round(t) for t in (q, k, v, dO))
    bias = torch.randn(H, L, L, generator=g, dtype=F64)
    keep = (torch.randint(0, 256, (B, H, L, L), generator=g) >= 25).to(F64)
    return q, k, v, dO, bias, keep


MODES = [(None, False), ("valid", False), (None, True), ("valid", True)]


@pytest.mark.parametrize("use_valid,causal", MODES)
@pytest.mark.parametrize("use_bias", [False, True])
def test_exact_matches_sdpa(use_valid, causal, use_bias):
    B, H, L = 3, 2, 128
    q, k, v, _, bias, _ = _inputs(B, H, L, seed=1)
    valid = torch.tensor([128, 65, 1], dtype=torch.int32) if use_valid else None
    scale = 0.25
    O, lse = FO.attn_exact(q, k, v, valid, bias if use_bias else None, scale, causal)
    add = torch.zeros(B, H, L, L, dtype=F64)
    if use_bias:
        add = add + bias
    add = add.masked_fill(FO.masked_keys(B, L, valid, causal, q.device), float("-inf"))
    ref = torch.nn.functional.scaled_dot_product_attention(q, k, v, attn_mask=add, scale=scale)
    assert float((O - ref).abs().max()) < 1e-13
    ref_lse = torch.logsumexp(scale * (q @ k.transpose(-1, -2)) + add, -1)
    assert float((lse - ref_lse).abs().max()) < 1e-12


def test_exact_gradcheck():
    B, H, L, d = 2, 2, 8, 4
    g = torch.Generator().manual_seed(2)
    q, k, v = (torch.randn(B, H, L, d, generator=g, dtype=F64, requires_grad=True) for _ in range(3))
    bias = torch.randn(H, L, L, generator=g, dtype=F64, requires_grad=True)
    keep = (torch.rand(B, H, L, L, generator=g) > 0.3).to(F64)
    valid = torch.tensor([8, 5], dtype=torch.int32)
    for causal in (False, True):
        for out in (0, 1):
            fn = lambda q, k, v, b: FO.attn_exact(q, k, v, valid, b, 0.7, causal, keep, 1.25)[out]  # noqa: E731,B023
            assert torch.autograd.gradcheck(fn, (q, k, v, bias), eps=1e-6, atol=1e-7, rtol=1e-5)


@pytest.mark.parametrize("use_valid,causal", MODES)
@pytest.mark.parametrize("use_bias,use_keep", [(False, False), (True, False), (False, True), (True, True)])
def test_emulated_backward_without_rounding_is_autograd(use_valid, causal, use_bias, use_keep):
    B, H, L = 3, 2, 128
    q, k, v, dO, bias, keep = _inputs(B, H, L, seed=3)
    valid = torch.tensor([127, 64, 0], dtype=torch.int32) if use_valid else None
    kw = dict(valid=valid, bias=bias if use_bias else None, scale=1.0, causal=causal,
              keep=keep if use_keep else None, dscale=FO.dropout_scale(0.1))
    ex = FO.exact_with_grads(q, k, v, dO, **kw)
    em = FO.attn_emulated(q, k, v, dO, rounding=False, **kw)
    names = ["O", "lse", "dq", "dk", "dv"] + (["dbias"] if use_bias else [])
    for n in names:
        err = float((em[n] - ex[n]).norm() / ex[n].norm().clamp_min(1e-300))
        assert err < 1e-12, (n, err)
    assert em["dbias"] is None or use_bias
    assert bool((em["abs_ds"] >= 0).all())


def test_emulated_with_rounding_differs_on_every_tensor():
    B, H, L = 2, 2, 192
    q, k, v, dO, bias, keep = _inputs(B, H, L, seed=4)
    valid = torch.tensor([192, 77], dtype=torch.int32)
    kw = dict(valid=valid, bias=bias, scale=1.0, causal=True, keep=keep,
              dscale=FO.dropout_scale(0.1))
    ex = FO.exact_with_grads(q, k, v, dO, **kw)
    em = FO.attn_emulated(q, k, v, dO, **kw)
    for n in ("O", "dq", "dk", "dv", "dbias"):
        err = float((em[n] - ex[n]).norm() / ex[n].norm())
        # bf16 roundings: a few 2^-9 at most, and never nothing
        assert 1e-4 < err < 2e-2, (n, err)
    assert torch.equal(em["lse"], ex["lse"])


def test_dead_rows_and_padded_keys_are_exactly_zero():
    B, H, L = 3, 2, 128
    q, k, v, dO, bias, keep = _inputs(B, H, L, seed=5)
    valid = torch.tensor([128, 70, 0], dtype=torch.int32)
    for causal in (False, True):
        kw = dict(valid=valid, bias=bias, scale=1.0, causal=causal, keep=keep, dscale=1.1)
        for res in (FO.exact_with_grads(q, k, v, dO, **kw), FO.attn_emulated(q, k, v, dO, **kw)):
            for n in ("O", "lse", "dq", "dk", "dv"):
                assert float(res[n][2].abs().max()) == 0.0, n       # valid = 0 batch row
            for n in ("dk", "dv"):
                assert float(res[n][1, :, 70:].abs().max()) == 0.0, n  # padded keys
                assert float(res[n][1, :, :70].abs().min()) > 0.0, n
            assert bool(torch.isfinite(res["dbias"]).all())
            assert float(res["dbias"][:, :, 70:].abs().max()) > 0.0     # batch row 0 reaches them


def test_layout_converters_and_dropout_scale():
    B, H, L, d = 2, 3, 64, 64
    x = torch.arange(B * L * H * d, dtype=F64).view(B, L, H * d)
    y = FO.to_bhld(x, H)
    assert y.shape == (B, H, L, d)
    assert float(y[1, 2, 5, 7]) == float(x[1, 5, 2 * d + 7])
    assert torch.equal(FO.from_bhld(y), x)
    bias = torch.randn(H, L, L, dtype=F64)
    bt = FO.bias_to_kernel(bias)
    assert bt.dtype == torch.float32 and bt.is_contiguous()
    assert float(bt[1, 3, 9]) == float(bias[1, 9, 3].float())
    assert torch.equal(FO.bias_from_kernel(bt), bias.float().double())
    assert FO.dropout_scale(0.1) == 256.0 / 231.0 and FO.dropout_scale(0.0) == 1.0
    assert FO.dropout_scale(0.5) == 2.0
    # bf16_round is round-to-nearest-even on 8 significant bits
    assert float(FO.bf16_round(torch.tensor([1.0 + 2.0 ** -8], dtype=F64))) == 1.0
    assert float(FO.bf16_round(torch.tensor([1.0 + 3 * 2.0 ** -8], dtype=F64))) == 1.0 + 2.0 ** -6
    assert math.isclose(float(FO.bf16_round(torch.tensor([0.3], dtype=F64))), 0.3, rel_tol=2.0 ** -8)
