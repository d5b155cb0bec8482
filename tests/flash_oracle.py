"""Float64 oracles for flash attention (csrc/flash_attn.hip: forward, Dterm,
dq and dkv kernels). Plain torch, any device, no GPU code and no pytest hooks.

Everything here is float64 in (B, H, L, d) terms; `to_bhld` / `from_bhld`
convert from and to the kernels' (B, L, H*d) layout and `bias_to_kernel` to
the kernels' key-major (H, Lk, Lq) bias layout.

    s    = scale q k^T + bias        keys >= valid[b] and, with causal,
                                     keys > q are masked
    P    = softmax(s)                a row with no unmasked key has P = 0,
                                     O = 0, lse = 0 (the kernel's convention)
    Pd   = P o keep dscale
    O    = Pd V
    lse  = log sum_k exp(s_k)

attn_exact     autograd, no intermediate rounding.
attn_emulated  the same math with a bf16 rounding wherever the kernels hand a
               bf16 operand to an MFMA or store a bf16 result, and a
               hand-written backward that consumes the rounded O as the Dterm
               kernel does:
                   O   = r(r(Pd) V)
                   D   = sum_d dO O
                   dPd = (dO V^T) o keep dscale
                   dS  = P (dPd - D)
                   dQ  = r(r(scale dS) K)      dK = r(r(scale dS)^T Q)
                   dV  = r(r(Pd)^T dO)         dBias = sum_b dS  (fp32 atomics,
                                                                  not rounded)
recover_keep   the dropout keep mask of a (seed, p, B, H, L), read back from
               the forward kernel itself with inputs that make every output
               element an indicator of one mask bit.

All of them start from what the kernels see: q, k, v, dO already bf16-valued.
"""

import torch

D_HEAD = 64


def bf16_round(t):
    """Round to bf16 through fp32, as the kernels' __float2bfloat16 does."""
    return t.float().to(torch.bfloat16).to(torch.float64)


def to_bhld(x, H):
    """(B, L, H*d) -> float64 (B, H, L, d)."""
    B, L, HD = x.shape
    return x.detach().to(torch.float64).view(B, L, H, HD // H).transpose(1, 2).contiguous()


def from_bhld(x):
    """(B, H, L, d) -> (B, L, H*d)."""
    B, H, L, d = x.shape
    return x.transpose(1, 2).reshape(B, L, H * d)


def bias_to_kernel(bias):
    """(H, Lq, Lk) -> the kernels' contiguous fp32 key-major (H, Lk, Lq)."""
    return bias.transpose(-1, -2).contiguous().float()


def bias_from_kernel(bias_t):
    """Key-major (H, Lk, Lq) -> float64 (H, Lq, Lk)."""
    return bias_t.detach().to(torch.float64).transpose(-1, -2).contiguous()


def dropout_scale(p):
    """The documented quantisation: a key is dropped when its hash byte is
    below floor(256 p), kept ones are scaled by 256 / (256 - floor(256 p))."""
    return 256.0 / (256.0 - float(int(p * 256.0)))


def masked_keys(B, L, valid, causal, device):
    """bool (B, 1, L, L), True where key (last dim) is masked for query."""
    key = torch.arange(L, device=device).view(1, 1, 1, L)
    m = torch.zeros(B, 1, L, L, dtype=torch.bool, device=device)
    if valid is not None:
        m = m | (key >= valid.to(device).view(B, 1, 1, 1))
    if causal:
        m = m | (key > torch.arange(L, device=device).view(1, 1, L, 1))
    return m


def _softmax(q, k, valid, bias, scale, causal):
    """P, lse and the masked scores; rows without an unmasked key give 0."""
    B, H, L, _ = q.shape
    s = scale * (q @ k.transpose(-1, -2))
    if bias is not None:
        s = s + bias.unsqueeze(0)
    s = s.masked_fill(masked_keys(B, L, valid, causal, q.device), float("-inf"))
    m = s.detach().max(-1, keepdim=True).values
    dead = torch.isinf(m)
    m = torch.where(dead, torch.zeros_like(m), m)
    e = torch.exp(s - m)
    l = e.sum(-1, keepdim=True)
    P = e / torch.where(dead, torch.ones_like(l), l)
    lse = torch.where(dead, torch.zeros_like(l), m + torch.log(torch.where(dead, torch.ones_like(l), l)))
    return P, lse.squeeze(-1), s


def attn_exact(q, k, v, valid=None, bias=None, scale=1.0, causal=False, keep=None, dscale=1.0):
    """Materialized attention under autograd: returns (O, lse). q, k, v are
    float64 (B, H, L, d), bias float64 (H, Lq, Lk), keep a 0/1 (B, H, L, L).
    dq, dk, dv, dbias come from O.backward(dO) on leaves that require grad."""
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


def recover_keep(ext, B, H, L, p, seed, device="cuda:0"):
    """The keep mask (float64 0/1, (B, H, Lq, Lk)) the kernels use for this
    (seed, p, B, H, L), recovered black-box from the forward kernel.

    With Q = 0 and no valid / bias / causal every unnormalised probability is
    exactly 1 and l = L. For the 64-key window w, V[b, key, h*64 + key%64] = 1
    for key // 64 == w and 0 elsewhere, so O[b, q, h*64 + d] = keep dscale / L
    for key w*64 + d: non-zero exactly when that key was kept. The mask is a
    function of (seed, floor(256 p), b*H + h, q, key) only, so it is the mask
    of every other call with the same seed, p, B, H and L."""
    bf = torch.bfloat16
    z = torch.zeros(B, L, H * D_HEAD, dtype=bf, device=device)
    keep = torch.empty(B, H, L, L, dtype=torch.float64, device=device)
    eye = torch.eye(D_HEAD, dtype=bf, device=device).repeat(1, H)      # (64, H*64)
    for w in range(L // D_HEAD):
        V = torch.zeros(B, L, H * D_HEAD, dtype=bf, device=device)
        V[:, w * D_HEAD:(w + 1) * D_HEAD] = eye
        O, _ = ext.flash_attn_fwd(z, z, V, H, None, None, 1.0, False, p, seed)
        keep[..., w * D_HEAD:(w + 1) * D_HEAD] = (
            O.view(B, L, H, D_HEAD).transpose(1, 2) != 0).to(torch.float64)
    return keep
