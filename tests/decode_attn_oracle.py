"""Float64 oracle for the decode attention ops (csrc/decode_attn.hip,
deepdfa_amd.ops.decode_self_attention / decode_cross_attention).

Plain torch, float64, any device. Every function takes the SAME values the
kernel sees (bf16 / fp32 tensors, converted to float64 exactly) and returns
float64. Head dim d = D // H throughout.

    decode_self_exact   O (R, H, d), P (R, H, T), S (R, H, T) with T = pos + 1,
                        plus the gathered histories Kh, Vh (R, T, H, d)
    decode_cross_exact  O (R, H, d), P (R, H, Lk), S (R, H, Lk); dead keys have
                        P = 0 and S = -inf, a valid = 0 source has O = 0
    gather_history      the keys (or values) row r attends to at step pos
    anc_from_parents    the indirection table after a scripted beam history
    random_bias_dist    an (H, Tmax) fp32 distance-indexed bias
    score_magnitudes    |scale| sum_d |q_d k_jd| + |bias_j| for the error bounds
"""

import torch


def gather_history(cache, new, anc, pos):
    """(R, pos + 1, D) float64: position j < pos of row r is
    cache[anc[r, j], j] (anc None = identity), position pos is new[r]. The
    cache's own slot (r, pos) is NOT read."""
    R = new.shape[0]
    dev = new.device
    hist = torch.empty(R, pos + 1, new.shape[1], dtype=torch.float64, device=dev)
    if pos > 0:
        cols = torch.arange(pos, device=dev).unsqueeze(0)
        if anc is None:
            rows = torch.arange(R, device=dev).unsqueeze(1).expand(R, pos)
        else:
            rows = anc[:, :pos].long()
        hist[:, :pos] = cache[rows, cols].double()
    hist[:, pos] = new.double()
    return hist


def _softmax_rows(S):
    """float64 softmax over the last dim; rows that are entirely -inf give 0."""
    m = S.max(dim=-1, keepdim=True).values
    m = torch.where(torch.isfinite(m), m, torch.zeros_like(m))
    e = torch.exp(S - m)
    den = e.sum(dim=-1, keepdim=True)
    return torch.where(den > 0, e / den.clamp_min(1e-300), torch.zeros_like(e))


def decode_self_exact(q, k_new, v_new, k_cache, v_cache, anc, bias_dist, pos, H, scale):
    """The caches are read as they are BEFORE the call (slot pos comes from
    k_new / v_new), so this may run before or after the op under test."""
    R, D = q.shape
    d = D // H
    T = pos + 1
    Kh = gather_history(k_cache, k_new, anc, pos).view(R, T, H, d)
    Vh = gather_history(v_cache, v_new, anc, pos).view(R, T, H, d)
    S = torch.einsum("rhd,rthd->rht", q.double().view(R, H, d), Kh) * scale
    if bias_dist is not None:
        dist = pos - torch.arange(T, device=q.device)
        S = S + bias_dist.double()[:, dist].unsqueeze(0)
    P = _softmax_rows(S)
    O = torch.einsum("rht,rthd->rhd", P, Vh)
    return O, P, S, Kh, Vh


def decode_cross_exact(q, k, v, valid, beams, H, scale):
    R, D = q.shape
    B, Lk, _ = k.shape
    assert R == B * beams
    d = D // H
    src = torch.arange(R, device=q.device) // beams
    Kh = k.double().view(B, Lk, H, d)[src]          # (R, Lk, H, d)
    Vh = v.double().view(B, Lk, H, d)[src]
    S = torch.einsum("rhd,rthd->rht", q.double().view(R, H, d), Kh) * scale
    if valid is not None:
        dead = torch.arange(Lk, device=q.device).view(1, 1, Lk) >= valid[src].view(R, 1, 1)
        S = S.masked_fill(dead, float("-inf"))
        # dead K/V may hold anything (NaN included): they contribute nothing
        Vh = torch.where(dead.transpose(1, 2).unsqueeze(-1).expand(R, Lk, H, 1), 0.0, Vh)
        S = torch.where(dead, torch.full_like(S, float("-inf")), S)
    P = _softmax_rows(S)
    O = torch.einsum("rht,rthd->rhd", P, Vh)
    return O, P, S, Kh, Vh


def score_magnitudes(q, Kh, bias_rht, scale):
    """|scale| sum_d |q_d k_jd| + |bias_j|, (R, H, T) float64."""
    R, T, H, d = Kh.shape
    mag = torch.einsum("rhd,rthd->rht", q.double().view(R, H, d).abs(),
                       torch.nan_to_num(Kh, nan=0.0).abs()) * abs(scale)
    if bias_rht is not None:
        mag = mag + bias_rht.abs()
    return mag


def anc_from_parents(parents, R, Tmax, device="cpu"):
    """The int32 (R, Tmax) indirection table after len(parents) decoded steps:
    at step t every row first owns its slot t, then the rows are re-gathered
    by parents[t] (new row r continues old row parents[t][r])."""
    rows = torch.arange(R, dtype=torch.int32)
    anc = rows.unsqueeze(1).repeat(1, Tmax)
    for t, par in enumerate(parents):
        anc[:, t] = rows
        anc = anc[torch.as_tensor(par, dtype=torch.long)]
    return anc.contiguous().to(device)


def random_parents(R, beams, steps, gen):
    """Per step a parent list that stays inside each source's beam group
    (rows b * beams .. b * beams + beams - 1) and permutes, duplicates and
    drops rows."""
    out = []
    for _ in range(steps):
        base = (torch.arange(R) // beams) * beams
        out.append((base + torch.randint(0, beams, (R,), generator=gen)).tolist())
    return out


def random_bias_dist(H, Tmax, gen, device="cpu"):
    return torch.randn(H, Tmax, generator=gen).float().to(device)
