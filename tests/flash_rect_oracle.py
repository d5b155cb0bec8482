"""Float64 oracles for the general flash attention (csrc/flash_rect.hip:
forward, dq and dkv kernels at any query length Lq and key length Lk). Plain
torch, any device, no GPU code and no pytest hooks.

The rectangular versions of tests/flash_oracle.py, with the same conventions
and the same rounding points (see that module's docstring): q is float64
(B, H, Lq, d), k and v (B, H, Lk, d), bias (H, Lq, Lk), keep a 0/1
(B, H, Lq, Lk). Keys >= min(valid[b], Lk) and, with causal (Lq == Lk only),
keys > q are masked; a row with no unmasked key has P = 0, O = 0, lse = 0.
`bf16_round`, `to_bhld`, `from_bhld`, `bias_to_kernel`, `bias_from_kernel`
and `dropout_scale` are flash_oracle's, re-exported.

recover_keep_rect reads the dropout keep mask of a (seed, p, B, H, Lq, Lk)
back from flash_rect_fwd.
"""

import torch

from flash_oracle import (D_HEAD, bf16_round, bias_from_kernel, bias_to_kernel,  # noqa: F401
                          dropout_scale, from_bhld, to_bhld)


def masked_keys(B, Lq, Lk, valid, causal, device):
    """bool (B, 1, Lq, Lk), True where key (last dim) is masked for query."""
    if causal and Lq != Lk:
        raise ValueError("causal needs Lq == Lk")
    key = torch.arange(Lk, device=device).view(1, 1, 1, Lk)
    m = torch.zeros(B, 1, Lq, Lk, dtype=torch.bool, device=device)
    if valid is not None:
        m = m | (key >= valid.to(device).view(B, 1, 1, 1))
    if causal:
        m = m | (key > torch.arange(Lq, device=device).view(1, 1, Lq, 1))
    return m


def _softmax(q, k, valid, bias, scale, causal):
    """P, lse and the masked scores; rows without an unmasked key give 0."""
    B, H, Lq, _ = q.shape
    Lk = k.shape[2]
    if bias is not None and Lq != Lk:
        raise ValueError("bias needs Lq == Lk")
    s = scale * (q @ k.transpose(-1, -2))
    if bias is not None:
        s = s + bias.unsqueeze(0)
    s = s.masked_fill(masked_keys(B, Lq, Lk, valid, causal, q.device), float("-inf"))
    m = s.detach().max(-1, keepdim=True).values
    dead = torch.isinf(m)
    m = torch.where(dead, torch.zeros_like(m), m)
    e = torch.exp(s - m)
    l = e.sum(-1, keepdim=True)
    P = e / torch.where(dead, torch.ones_like(l), l)
    lse = torch.where(dead, torch.zeros_like(l), m + torch.log(torch.where(dead, torch.ones_like(l), l)))
    return P, lse.squeeze(-1), s


def attn_exact(q, k, v, valid=None, bias=None, scale=1.0, causal=False, keep=None, dscale=1.0):
    """Materialized attention under autograd: returns (O, lse)."""
    P, lse, _ = _softmax(q, k, valid, bias, scale, causal)
    Pd = P if keep is None else P * keep * dscale
    return Pd @ v, lse


def exact_with_grads(q, k, v, dO, valid=None, bias=None, scale=1.0, causal=False, keep=None,
                     dscale=1.0):
    """attn_exact and its autograd gradients as a dict of detached tensors."""
    leaves = [t.detach().clone().requires_grad_() for t in (q, k, v)]
    b = None if bias is None else bias.detach().clone().requires_grad_()
    O, lse = attn_exact(*leaves, valid, b, scale, causal, keep, dscale)
    O.backward(dO)
    out = dict(O=O.detach(), lse=lse.detach(), dq=leaves[0].grad, dk=leaves[1].grad,
               dv=leaves[2].grad)
    if b is not None:
        out["dbias"] = b.grad
    return out


def attn_emulated(q, k, v, dO, valid=None, bias=None, scale=1.0, causal=False, keep=None,
                  dscale=1.0, rounding=True):
    """Forward and hand-written backward with the kernels' bf16 roundings
    (rounding=False: none, which must reproduce attn_exact's autograd).
    Returns O, lse, dq, dk, dv, dbias (None without bias) and abs_ds =
    sum_b |dS_b|, the magnitude the dBias accumulation bound needs."""
    r = bf16_round if rounding else (lambda t: t)
    with torch.no_grad():
        P, lse, _ = _softmax(q, k, valid, bias, scale, causal)
        M = 1.0 if keep is None else keep * dscale
        Pd = P * M
        O = r(r(Pd) @ v)
        D = (dO * O).sum(-1, keepdim=True)
        dS = P * ((dO @ v.transpose(-1, -2)) * M - D)
        sdS = r(scale * dS)
        out = dict(O=O, lse=lse,
                   dq=r(sdS @ k),
                   dk=r(sdS.transpose(-1, -2) @ q),
                   dv=r(r(Pd).transpose(-1, -2) @ dO),
                   dbias=None if bias is None else dS.sum(0),
                   abs_ds=dS.abs().sum(0))
    return out


def forward_terms(q, k, v, valid, bias, scale, causal, keep, dscale):
    """What the elementwise forward bound is made of (all float64):
    P, Pd, the masked scores s with their row max m (0 for dead rows), and
    mag = scale sum_d |q k| + |bias|, the magnitude that enters a score."""
    with torch.no_grad():
        P, lse, s = _softmax(q, k, valid, bias, scale, causal)
        Pd = P if keep is None else P * keep * dscale
        mag = scale * (q.abs() @ k.abs().transpose(-1, -2))
        if bias is not None:
            mag = mag + bias.abs().unsqueeze(0)
        m = s.max(-1, keepdim=True).values
        m = torch.where(torch.isinf(m), torch.zeros_like(m), m)
        gap = torch.where(torch.isinf(s), torch.zeros_like(s), (s - m).abs())
    return dict(P=P, Pd=Pd, lse=lse, mag=mag, gap=gap)


def recover_keep_rect(ext, B, H, Lq, Lk, p, seed, device="cuda:0"):
    """The keep mask (float64 0/1, (B, H, Lq, Lk)) the general kernels use for
    this (seed, p, B, H, Lq, Lk), recovered black-box from flash_rect_fwd.

    With Q = 0 and no valid / bias / causal every unnormalised probability is
    exactly 1 and l = Lk. For the 64-key window w (the last one partial),
    V[b, key, h*64 + key%64] = 1 for key // 64 == w and 0 elsewhere, so
    O[b, q, h*64 + d] = keep dscale / Lk for key w*64 + d: non-zero exactly
    when that key was kept."""
    bf = torch.bfloat16
    zq = torch.zeros(B, Lq, H * D_HEAD, dtype=bf, device=device)
    zk = torch.zeros(B, Lk, H * D_HEAD, dtype=bf, device=device)
    keep = torch.empty(B, H, Lq, Lk, dtype=torch.float64, device=device)
    eye = torch.eye(D_HEAD, dtype=bf, device=device).repeat(1, H)      # (64, H*64)
    for w0 in range(0, Lk, D_HEAD):
        n = min(D_HEAD, Lk - w0)
        V = torch.zeros(B, Lk, H * D_HEAD, dtype=bf, device=device)
        V[:, w0:w0 + n] = eye[:n]
        O, _ = ext.flash_rect_fwd(zq, zk, V, H, None, None, 1.0, False, p, seed)
        keep[..., w0:w0 + n] = (
            O.view(B, Lq, H, D_HEAD).transpose(1, 2)[..., :n] != 0).to(torch.float64)
    return keep
