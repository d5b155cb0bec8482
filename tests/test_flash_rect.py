"""General flash attention off the GPU: the rectangular float64 oracle
(tests/flash_rect_oracle.py) against its own autograd and against the square
oracle, the torch path of flash_attention_rect / flash_attention_rect_kv
against the oracle, and the argument errors of the flash_rect bindings that
CPU tensors reach."""

import pytest
import torch

import flash_oracle as FO
import flash_rect_oracle as FR

H = 2
D = H * 64


def _case(B, Lq, Lk, seed, bias=False, valid=None, dtype=torch.float64):
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(B, H, Lq, 64, generator=g, dtype=torch.float64) * 0.5
    k = torch.randn(B, H, Lk, 64, generator=g, dtype=torch.float64) * 0.5
    v = torch.randn(B, H, Lk, 64, generator=g, dtype=torch.float64) * 0.5
    dO = torch.randn(B, H, Lq, 64, generator=g, dtype=torch.float64)
    b = torch.randn(H, Lq, Lk, generator=g, dtype=torch.float64) if bias else None
    keep = (torch.rand(B, H, Lq, Lk, generator=g) >= 0.1).to(torch.float64)
    vt = None if valid is None else torch.tensor(valid, dtype=torch.int32)
    return q, k, v, dO, b, keep, vt


CASES = [  # (B, Lq, Lk, valid, causal, bias)
    (3, 5, 9, [9, 4, 0], False, False),
    (2, 33, 65, [65, 64], False, False),
    (3, 70, 70, [70, 33, 0], True, True),
]


@pytest.mark.parametrize("B,Lq,Lk,valid,causal,bias", CASES)
def test_oracle_without_rounding_reproduces_autograd(B, Lq, Lk, valid, causal, bias):
    q, k, v, dO, b, keep, vt = _case(B, Lq, Lk, 1, bias, valid)
    args = dict(valid=vt, bias=b, scale=0.7, causal=causal, keep=keep, dscale=FO.dropout_scale(0.1))
    ex = FR.exact_with_grads(q, k, v, dO, **args)
    em = FR.attn_emulated(q, k, v, dO, rounding=False, **args)
    for n in ["O", "lse", "dq", "dk", "dv"] + (["dbias"] if bias else []):
        assert ex[n].shape == em[n].shape
        torch.testing.assert_close(em[n], ex[n], rtol=1e-11, atol=1e-12)
    # dead rows (valid = 0): O = 0, lse = 0, no gradient anywhere
    dead = [i for i, x in enumerate(valid) if x == 0]
    for i in dead:
        assert float(ex["O"][i].abs().max()) == 0 and float(ex["lse"][i].abs().max()) == 0
        assert float(ex["dk"][i].abs().max()) == 0 and float(ex["dq"][i].abs().max()) == 0
    # the rounded emulation differs, by about a bf16 ulp
    er = FR.attn_emulated(q, k, v, dO, **args)
    rel = float((er["O"] - ex["O"]).norm() / ex["O"].norm())
    assert 0.0 < rel < 2.0 ** -6


@pytest.mark.parametrize("causal,bias", [(False, False), (True, True)])
def test_square_equals_flash_oracle(causal, bias):
    L = 70
    q, k, v, dO, b, keep, vt = _case(3, L, L, 2, bias, [70, 1, 0])
    args = dict(valid=vt, bias=b, scale=1.0, causal=causal, keep=keep, dscale=FO.dropout_scale(0.1))
    assert torch.equal(FR.masked_keys(3, L, L, vt, causal, "cpu"), FO.masked_keys(3, L, vt, causal, "cpu"))
    a, c = FR.exact_with_grads(q, k, v, dO, **args), FO.exact_with_grads(q, k, v, dO, **args)
    for n in a:
        assert torch.equal(a[n], c[n]), n
    a, c = FR.attn_emulated(q, k, v, dO, **args), FO.attn_emulated(q, k, v, dO, **args)
    for n in a:
        assert (a[n] is None and c[n] is None) or torch.equal(a[n], c[n]), n
    a, c = FR.forward_terms(q, k, v, **args), FO.forward_terms(q, k, v, **args)
    for n in a:
        assert torch.equal(a[n], c[n]), n


def test_oracle_rejects_rectangular_causal_and_bias():
    q, k, v, dO, _, _, _ = _case(1, 5, 9, 3)
    with pytest.raises(ValueError):
        FR.attn_exact(q, k, v, causal=True)
    with pytest.raises(ValueError):
        FR.attn_exact(q, k, v, bias=torch.zeros(H, 5, 9, dtype=torch.float64))


def _op_inputs(B, Lq, Lk, seed, bias, valid):
    q, k, v, dO, b, _, vt = _case(B, Lq, Lk, seed, bias, valid)
    x = [FO.from_bhld(t).float() for t in (q, k, v, dO)]
    return (q, k, v, dO, b, vt), x


@pytest.mark.parametrize("B,Lq,Lk,valid,causal,bias", CASES)
def test_cpu_path_matches_oracle(B, Lq, Lk, valid, causal, bias):
    from deepdfa_amd.ops import flash_attention_rect, flash_attention_rect_kv, flash_rect_usable

    (q, k, v, dO, b, vt), (q32, k32, v32, dO32) = _op_inputs(B, Lq, Lk, 4, bias, valid)
    assert not flash_rect_usable(q32, 64)
    ex = FR.exact_with_grads(q, k, v, dO, valid=vt, bias=b, scale=0.7, causal=causal)

    def check(got, grads):
        torch.testing.assert_close(FO.to_bhld(got, H), ex["O"], rtol=2e-5, atol=2e-6,
                                   check_dtype=False)
        for g, n in zip(grads, ("dq", "dk", "dv")):
            torch.testing.assert_close(FO.to_bhld(g, H), ex[n], rtol=2e-4, atol=2e-5,
                                       check_dtype=False)

    ql, kl, vl = (t.clone().requires_grad_() for t in (q32, k32, v32))
    bt = None if b is None else FO.bias_to_kernel(b).requires_grad_()
    out = flash_attention_rect(ql, kl, vl, H, valid=vt, bias=bt, scale=0.7, causal=causal)
    assert out.shape == (B, Lq, D) and out.dtype == torch.float32
    out.backward(dO32)
    check(out, (ql.grad, kl.grad, vl.grad))
    if bias:
        torch.testing.assert_close(FO.bias_from_kernel(bt.grad), ex["dbias"], rtol=2e-4,
                                   atol=2e-5, check_dtype=False)
    if not (causal or bias):
        ql = q32.clone().requires_grad_()
        kv = torch.cat([k32, v32], -1).requires_grad_()
        out = flash_attention_rect_kv(ql, kv, H, valid=vt, scale=0.7)
        out.backward(dO32)
        check(out, (ql.grad, kv.grad[..., :D], kv.grad[..., D:]))


def test_cpu_path_rejects_rectangular_causal_and_bias():
    from deepdfa_amd.ops import flash_attention_rect

    q, k = torch.zeros(1, 5, D), torch.zeros(1, 9, D)
    with pytest.raises(ValueError):
        flash_attention_rect(q, k, k, H, causal=True)
    with pytest.raises(ValueError):
        flash_attention_rect(q, k, k, H, bias=torch.zeros(H, 9, 5))


def test_cpu_path_dropout_scales_kept_probabilities():
    from deepdfa_amd.ops import flash_attention_rect

    torch.manual_seed(0)
    q = torch.zeros(1, 4, D)
    k = torch.zeros(1, 50, D)
    v = torch.ones(1, 50, D)
    out = flash_attention_rect(q, k, v, H, dropout_p=0.5)
    # uniform P = 1/50, kept entries scaled by 2: each output is (kept / 50) * 2
    kept = out * 25.0
    assert torch.allclose(kept, kept.round(), atol=1e-4) and 0 < float(out.mean()) < 2


# ---------------------------------------------------------------------------
# binding argument errors that CPU tensors reach: the bindings check shapes,
# dtypes and strides before the device
# ---------------------------------------------------------------------------

def _ext():
    from deepdfa_amd.ops import load_ext

    ext = load_ext()
    if ext is None:
        pytest.skip("deepdfa_amd._C is not built")
    return ext


def _bf(*shape):
    return torch.zeros(*shape, dtype=torch.bfloat16)


def test_binding_argument_errors():
    ext = _ext()
    q, k = _bf(2, 5, D), _bf(2, 9, D)
    ok_tail = (1.0, False, 0.0, 0)

    def fwd(Q, K, V, Hh=H, valid=None, bias=None, causal=False):
        return ext.flash_rect_fwd(Q, K, V, Hh, valid, bias, 1.0, causal, 0.0, 0)

    with pytest.raises(RuntimeError, match="bf16"):
        fwd(q.float(), k, k)
    with pytest.raises(RuntimeError, match="head_dim must be 64"):
        fwd(q, k, k, Hh=4)
    with pytest.raises(RuntimeError, match="same shape and row stride"):
        fwd(q, k, _bf(2, 8, D))
    with pytest.raises(RuntimeError, match="same shape and row stride"):
        fwd(q, k, _bf(2, 9, 2 * D)[..., :D])
    with pytest.raises(RuntimeError, match="batch size"):
        fwd(q, _bf(3, 9, D), _bf(3, 9, D))
    with pytest.raises(RuntimeError, match="must be >= 1"):
        fwd(q, _bf(2, 0, D), _bf(2, 0, D))
    with pytest.raises(RuntimeError, match="65535"):
        fwd(_bf(2, 1, 32768 * 64), _bf(2, 1, 32768 * 64), _bf(2, 1, 32768 * 64), Hh=32768)
    with pytest.raises(RuntimeError, match="causal needs Lq == Lk"):
        fwd(q, k, k, causal=True)
    with pytest.raises(RuntimeError, match="bias needs Lq == Lk"):
        fwd(q, k, k, bias=torch.zeros(H, 9, 5))
    with pytest.raises(RuntimeError, match=r"key-major \(H, Lk, Lq\)"):
        fwd(k, k, k, bias=torch.zeros(H, 9, 8))
    with pytest.raises(RuntimeError, match="contiguous fp32"):
        fwd(k, k, k, bias=torch.zeros(H, 9, 9, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="int32"):
        fwd(q, k, k, valid=torch.tensor([9, 9]))
    with pytest.raises(RuntimeError, match="B lengths"):
        fwd(q, k, k, valid=torch.tensor([9, 9, 9], dtype=torch.int32))
    with pytest.raises(RuntimeError, match="contiguous int32"):
        fwd(q, k, k, valid=torch.tensor([9, 0, 9, 0], dtype=torch.int32)[::2])
    with pytest.raises(RuntimeError, match="row-strided view"):
        fwd(q.transpose(0, 1).contiguous().transpose(0, 1), k, k)
    with pytest.raises(RuntimeError, match="row-strided view"):
        fwd(_bf(2, 5, 2 * D)[..., ::2], k, k)
    # everything above passed: a well-formed CPU call stops at the device check
    with pytest.raises(RuntimeError, match="on one GPU"):
        fwd(q, k, k)
    with pytest.raises(RuntimeError, match="on one GPU"):
        fwd(q, _bf(2, 9, 2 * D)[..., :D], _bf(2, 9, 2 * D)[..., D:])
    # the backward binding runs the same checks
    o, lse = _bf(2, 5, D), torch.zeros(2, H, 5)
    with pytest.raises(RuntimeError, match="causal needs Lq == Lk"):
        ext.flash_rect_bwd(o, q, k, k, o, lse, H, None, None, 1.0, True, 0.0, 0, False)
    with pytest.raises(RuntimeError, match="on one GPU"):
        ext.flash_rect_bwd(o, q, k, k, o, lse, H, None, None, *ok_tail, False, None,
                           kv_fused=True)
