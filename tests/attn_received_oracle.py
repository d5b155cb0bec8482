"""Float64 oracle for the attention-received kernel (csrc/flash_attn.hip:
flash_received_kernel). Plain torch, any device, no GPU code and no pytest
hooks; built on flash_oracle._softmax, so masking and the dead-row convention
are the flash family's.

    s = scale q k^T + bias         keys >= valid[b] and, with causal, keys > q
                                   are masked; padded QUERY rows are not
    P = softmax(s)                 a row with no unmasked key has P = 0, lse = 0
    R[b, h, j] = sum_i P[b, h, i, j]

q, k are float64 (B, H, L, d) (flash_oracle.to_bhld), bias float64 (H, Lq, Lk)
(flash_oracle.bias_from_kernel).
"""

import torch

import flash_oracle as FO


def received_exact(q, k, valid=None, bias=None, scale=1.0, causal=False):
    """(R, P, lse, s): R (B, H, L) the attention each key receives, P the
    probabilities, lse (B, H, L) and the masked scores s (-inf where masked)."""
    with torch.no_grad():
        P, lse, s = FO._softmax(q, k, valid, bias, scale, causal)
        R = P.sum(dim=-2)
    return R, P, lse, s


def received_bound_terms(q, k, P, lse, s, bias, scale):
    """What the elementwise bound of the kernel is made of (float64):
    mag = scale sum_d |q k| + |bias|, the magnitude that enters a score, and
    gap = |s - lse| (0 where the key is masked: P is 0 there)."""
    with torch.no_grad():
        mag = scale * (q.abs() @ k.abs().transpose(-1, -2))
        if bias is not None:
            mag = mag + bias.abs().unsqueeze(0)
        gap = torch.where(torch.isinf(s), torch.zeros_like(s), (s - lse.unsqueeze(-1)).abs())
    return mag, gap
