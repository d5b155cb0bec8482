"""Float64 oracles for the transformer row kernels (csrc/transformer_kernels.hip
and colsum in csrc/flowgnn_kernels.hip), as plain torch expressions that
autograd differentiates, plus an exact integer replica of the kernels'
stateless dropout mask.

Inputs are taken AFTER rounding to the kernel's IO dtype (callers pass the
bf16 / fp32 tensors the kernel sees, widened with .double()), so input
quantisation is not counted as error. Everything here runs on whatever device
its arguments live on and needs no GPU.
"""

import math

import numpy as np
import torch

U32 = np.uint64(0xFFFFFFFF)


# ---------------------------------------------------------------------------
# dropout mask: hash4 / keep_mask of transformer_kernels.hip, integer-exact
# ---------------------------------------------------------------------------

def p8_of(p):
    """The kernels' byte threshold: (unsigned)(float(p) * 256.0f)."""
    return int(np.float32(p) * np.float32(256.0))


def drop_scale(p):
    """Byte-quantised inverse keep rate, 256 / (256 - p8); 1 when p8 == 0."""
    p8 = p8_of(p)
    return 256.0 / (256.0 - p8) if p8 > 0 else 1.0


def hash4_np(quad, seed):
    quad = np.asarray(quad, dtype=np.uint64)
    seed = np.uint64(seed)
    h = (quad & U32) * np.uint64(2654435761) & U32
    h = (h + ((quad >> np.uint64(32)) & U32) * np.uint64(40503)) & U32
    h = (h + (seed & U32)) & U32
    h = (h + ((seed >> np.uint64(32)) & U32) * np.uint64(97)) & U32
    h ^= h >> np.uint64(16)
    h = h * np.uint64(0x7FEB352D) & U32
    h ^= h >> np.uint64(15)
    h = h * np.uint64(0x846CA68B) & U32
    h ^= h >> np.uint64(16)
    return h


def keep_mask_np(flat_idx, seed, p):
    """keep[i] for flat element offsets `flat_idx`: byte lane idx & 3 of
    hash4(idx >> 2, seed) compared with p8. p8 == 0 keeps everything."""
    idx = np.asarray(flat_idx, dtype=np.uint64)
    p8 = p8_of(p)
    if p8 == 0:
        return np.ones(idx.shape, dtype=bool)
    h = hash4_np(idx >> np.uint64(2), seed)
    byte = (h >> (np.uint64(8) * (idx & np.uint64(3)))) & np.uint64(0xFF)
    return byte >= np.uint64(p8)


def keep_tensor(shape, seed, p, device="cpu"):
    """float64 0/1 keep mask of a contiguous tensor of `shape`."""
    n = int(np.prod(shape)) if len(shape) else 1
    k = keep_mask_np(np.arange(n, dtype=np.uint64), seed, p).reshape(shape)
    return torch.from_numpy(k.astype(np.float64)).to(device)


# ---------------------------------------------------------------------------
# oracles: float64 in, float64 out, differentiable. Evaluated on fp32
# arguments the same expressions serve as the fp32 yardstick.
# ---------------------------------------------------------------------------

def layer_norm(x, gamma, beta, eps):
    mu = x.mean(-1, keepdim=True)
    c = x - mu
    var = (c * c).mean(-1, keepdim=True)
    return c / torch.sqrt(var + eps) * gamma + beta


def rms_norm(x, gamma, eps):
    return x / torch.sqrt((x * x).mean(-1, keepdim=True) + eps) * gamma


def bias_gelu(x, bias):
    v = x + bias
    return 0.5 * v * (1.0 + torch.erf(v * math.sqrt(0.5)))


def masked_softmax_dropout(S, valid, scale, keep=None, dscale=1.0, causal=False):
    """(P, Pd) of softmax(S * scale) over the last dim of S (B, H, Lq, L):
    key columns >= valid[b] and, with `causal`, columns > the query row are
    masked; -inf scores count as masked; a row with nothing left is all zero.
    Pd = P * keep * dscale."""
    B, H, Lq, L = S.shape
    s = S * scale
    col = torch.arange(L, device=S.device).view(1, 1, 1, L)
    masked = torch.isinf(s) & (s < 0)
    if valid is not None:
        masked = masked | (col >= valid.clamp(0, L).view(B, 1, 1, 1))
    if causal:
        masked = masked | (col > torch.arange(Lq, device=S.device).view(1, 1, Lq, 1))
    s0 = torch.where(masked, torch.zeros_like(s), s)
    m = torch.where(masked, torch.full_like(s, -float("inf")), s0).amax(-1, keepdim=True)
    m = torch.where(torch.isinf(m), torch.zeros_like(m), m).detach()
    e = torch.where(masked, torch.zeros_like(s), torch.exp(s0 - m))
    tot = e.sum(-1, keepdim=True)
    P = torch.where(tot > 0, e / torch.where(tot > 0, tot, torch.ones_like(tot)),
                    torch.zeros_like(e))
    Pd = P if keep is None else P * keep * dscale
    return P, Pd


def layer_norm_res_dropout(h, res, gamma, beta, eps, keep=None, dscale=1.0):
    z = h if keep is None else h * keep * dscale
    return layer_norm(z + res, gamma, beta, eps)


def dropout_add(h, res, keep=None, dscale=1.0):
    return res + (h if keep is None else h * keep * dscale)


def relu_dropout(x, keep=None, dscale=1.0):
    r = torch.relu(x)
    return r if keep is None else r * keep * dscale


def embed_scatter(dY, idx, num_rows, padding_idx=None):
    """dW[idx[n]] += dY[n], rows whose index is padding_idx skipped."""
    dY = dY.reshape(-1, dY.shape[-1])
    idx = idx.reshape(-1)
    if padding_idx is not None:
        sel = idx != padding_idx
        dY, idx = dY[sel], idx[sel]
    out = torch.zeros(num_rows, dY.shape[-1], dtype=dY.dtype, device=dY.device)
    return out.index_add_(0, idx, dY)


def relbias_wgrad(dbias, buckets, num_buckets):
    """dW[b, h] = sum over (q, k) with buckets[q, k] == b of dbias[h, q, k]."""
    H = dbias.shape[0]
    g = dbias.reshape(H, -1).t()
    out = torch.zeros(num_buckets, H, dtype=dbias.dtype, device=dbias.device)
    return out.index_add_(0, buckets.reshape(-1).long(), g)


def colsum(x):
    return x.sum(0)


# ---------------------------------------------------------------------------
# bounds
# ---------------------------------------------------------------------------

def half_ulp(mag, dtype):
    """Half an ulp of `dtype` (bf16 / fp32) at magnitude `mag` (float64)."""
    mant = 7 if dtype == torch.bfloat16 else 23
    e = torch.floor(torch.log2(mag.abs().clamp_min(2.0 ** -126)))
    return torch.exp2(e - mant - 1)


def onepass_layer_norm_f32(x, gamma, beta, eps):
    """fp32 emulation of the one-pass variance s2/D - mu*mu (the formula the
    LayerNorm kernels used): shows what the ill-conditioned rows catch."""
    x = x.float()
    D = x.shape[-1]
    mu = x.sum(-1, keepdim=True) / D
    var = (x * x).sum(-1, keepdim=True) / D - mu * mu
    return (x - mu) * torch.rsqrt(var + torch.tensor(eps, dtype=torch.float32)) \
        * gamma.float() + beta.float()


def ln_conditioning_floor(x, ref, eps):
    """4 (|mean| / std) 2^-24 max|ref_row| per row, std taken as
    sqrt(var + eps) so that constant rows (std = 0) get a finite floor: the
    error one fp32 ulp of the row mean leaves in the normalised row."""
    mu = x.mean(-1, keepdim=True)
    sd = torch.sqrt(((x - mu) ** 2).mean(-1, keepdim=True) + eps)
    return 4.0 * mu.abs() / sd * 2.0 ** -24 * ref.abs().amax(-1, keepdim=True)


def ill_rows(kind, n, d, gen, dtype=torch.float32):
    """The row families of the LayerNorm tests, rounded to `dtype`."""
    if kind == "normal":
        x = 0.5 + 2.0 * torch.randn(n, d, generator=gen)
    elif kind == "m30":
        x = 30.0 + 0.05 * torch.randn(n, d, generator=gen)
    elif kind == "m100":
        x = 100.0 + 0.01 * torch.randn(n, d, generator=gen)
    elif kind == "const":
        x = torch.full((n, d), 3.3)
        x[1::2] = 0.0
        if n == 1:
            x[:, :] = 3.3
    else:
        raise ValueError(kind)
    return x.to(dtype)
