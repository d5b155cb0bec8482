"""Float64 oracles for the fused GGNN message-passing loop
(csrc/bindings.hip ggnn_fused_fwd / ggnn_fused_bwd). Plain torch, any device.

Per step, with h = HH[s]:
    wh  = h W_e^T + b_e
    m_v = sum_{u->v} wh_u                     (in-CSR segment sum)
    r   = sigmoid(m W_ir^T + h W_hr^T + b_r)  (b_r = b_ir + b_hr, merged)
    z   = sigmoid(m W_iz^T + h W_hz^T + b_z)
    hn  = h W_hn^T + b_hn
    n   = tanh(m W_in^T + b_in + r hn)
    h'  = (1 - z) n + z h

ggnn_exact     autograd, no intermediate rounding.
ggnn_emulated  the same loop with a bf16 rounding at every tensor the
               kernels materialise in bf16, and a hand-written backward that
               consumes the saved, rounded activations as the kernel does.
step_exact     one teacher-forced step from a given HH[s] (and M[s]).

All of them start from what the kernels see: x already bf16-valued, weights
as the pack kernel emits them (bf16 values, here held in float64).
"""

import torch

from deepdfa_amd.graph.batch import BatchedCFG, batch_graphs

SMALL_SIZES = [1, 2, 3, 31, 32, 33, 63, 64, 65, 300]


# --------------------------------------------------------------------------
# graphs
# --------------------------------------------------------------------------

def small_graph():
    """The edge-case batch: returns (graph, info). Chains with self-loops
    except: the 1-node graph has no edge; node 0 of the 33-node graph and
    every 7th node of the 300-node graph have no in-edge; every node of the
    300-node graph points at that graph's node 5 (hub); ten chain edges of
    the 65-node graph are listed twice."""
    graphs, zero_in, offs = [], [], [0]
    hub = None
    for n in SMALL_SIZES:
        base = offs[-1]
        src, dst = [], []
        if n > 1:
            for i in range(n):
                isolated = (n == 33 and i == 0) or (n == 300 and i % 7 == 0)
                if isolated:
                    zero_in.append(base + i)
                    continue
                src.append(i), dst.append(i)          # self-loop
                if i > 0:
                    src.append(i - 1), dst.append(i)  # chain
            if n == 300:
                src += list(range(n))
                dst += [5] * n
                hub = base + 5
            if n == 65:
                src += list(range(10, 20))
                dst += list(range(11, 21))
        else:
            zero_in.append(base)
        graphs.append(BatchedCFG.from_edges(n, src, dst, add_self_loops=False))
        offs.append(base + n)
    g = batch_graphs(graphs)
    info = {"zero_in": sorted(zero_in), "hub": hub, "N": offs[-1]}
    check_small_graph(g, info)
    return g, info


def check_small_graph(g, info):
    """The properties the tests rely on, asserted on the built CSR."""
    N = info["N"]
    assert N == sum(SMALL_SIZES) == g.num_nodes
    assert g.node_offsets.tolist() == [sum(SMALL_SIZES[:i]) for i in range(len(SMALL_SIZES) + 1)]
    deg = (g.indptr[1:] - g.indptr[:-1]).tolist()
    assert [v for v in range(N) if deg[v] == 0] == info["zero_in"]
    assert len(info["zero_in"]) == 1 + 1 + 43
    assert deg[info["hub"]] >= 300
    dst = torch.repeat_interleave(torch.arange(N), torch.tensor(deg))
    pairs = (g.indices.to(torch.int64) * N + dst).tolist()
    dup = len(pairs) - len(set(pairs))
    assert dup >= 10, dup
    # the transpose lists the same multiset of edges
    tdeg = (g.t_indptr[1:] - g.t_indptr[:-1]).tolist()
    tsrc = torch.repeat_interleave(torch.arange(N), torch.tensor(tdeg))
    tpairs = (tsrc * N + g.t_indices.to(torch.int64)).tolist()
    assert sorted(tpairs) == sorted(pairs)


def chain_graph(N, seg=97):
    """Chains with self-loops in graphs of `seg` nodes (the last one shorter)."""
    graphs = []
    left = N
    while left > 0:
        n = min(seg, left)
        i = torch.arange(n)
        src = torch.cat([i, i[:-1]])
        dst = torch.cat([i, i[1:]])
        graphs.append(BatchedCFG.from_edges(n, src, dst, add_self_loops=False))
        left -= n
    g = batch_graphs(graphs)
    assert g.num_nodes == N
    return g


# --------------------------------------------------------------------------
# weights
# --------------------------------------------------------------------------

def make_params(H, seed=0):
    """fp32 master weights (W_e, b_e, W_ih, W_hh, b_ih, b_hh) on the CPU:
    GatedGraphConv.reset_parameters() under a fixed seed, every bias re-drawn
    non-zero (b_e is zero-initialised)."""
    from deepdfa_amd.models.flow_gnn import GatedGraphConv

    torch.manual_seed(seed)
    conv = GatedGraphConv(H, H, 1)
    gen = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        conv.linear.bias.copy_(0.1 * torch.randn(H, generator=gen))
        conv.gru.bias_ih.copy_(0.1 * torch.randn(3 * H, generator=gen))
        conv.gru.bias_hh.copy_(0.1 * torch.randn(3 * H, generator=gen))
    ps = (conv.linear.weight, conv.linear.bias, conv.gru.weight_ih, conv.gru.weight_hh,
          conv.gru.bias_ih, conv.gru.bias_hh)
    return tuple(p.detach().clone() for p in ps)


def make_x(N, H, seed=0):
    gen = torch.Generator().manual_seed(seed + 100)
    return (0.5 * torch.randn(N, H, generator=gen)).to(torch.bfloat16)


def make_grad_out(N, H, seed=0):
    gen = torch.Generator().manual_seed(seed + 200)
    return (torch.randn(N, H, generator=gen) / 16).to(torch.bfloat16)


def pack_reference(W_e, b_e, W_ih, W_hh, b_ih, b_hh):
    """The eight buffers of ops.flowgnn._ggnn_pack_cache built with torch ops
    from the fp32 masters: fp32 -> bf16 round-to-nearest-even casts."""
    H = W_e.shape[0]
    bf = torch.bfloat16
    Wcat = torch.zeros(4 * H, 2 * H, dtype=torch.float32, device=W_e.device)
    Wcat[: 3 * H, :H] = W_ih
    Wcat[: 2 * H, H:] = W_hh[: 2 * H]
    Wcat[3 * H:, H:] = W_hh[2 * H:]
    b_cat = torch.cat([b_ih[: 2 * H] + b_hh[: 2 * H], b_ih[2 * H:], b_hh[2 * H:]])
    Wcat = Wcat.to(bf)
    b_cat = b_cat.to(bf)
    # row j*4+g of the gate-interleaved layout is row g*H+j of Wcat
    Wcat_perm = Wcat.view(4, H, 2 * H).permute(1, 0, 2).reshape(4 * H, 2 * H).contiguous()
    b_perm = b_cat.view(4, H).t().reshape(4 * H).contiguous()
    return {
        "w_e16": W_e.to(bf), "b_e16": b_e.to(bf), "Wcat": Wcat,
        "WcatT": Wcat.t().contiguous(), "b_cat": b_cat,
        "W_eT": W_e.to(bf).t().contiguous(), "Wcat_perm": Wcat_perm, "b_perm": b_perm,
    }


def empty_pack(H, device, fill=float("nan")):
    bf = torch.bfloat16
    shapes = {"w_e16": (H, H), "b_e16": (H,), "Wcat": (4 * H, 2 * H), "WcatT": (2 * H, 4 * H),
              "b_cat": (4 * H,), "W_eT": (H, H), "Wcat_perm": (4 * H, 2 * H), "b_perm": (4 * H,)}
    return {k: torch.full(s, fill, dtype=bf, device=device) for k, s in shapes.items()}


PACK_ORDER = ("w_e16", "b_e16", "Wcat", "WcatT", "b_cat", "W_eT", "Wcat_perm", "b_perm")


def oracle_weights(buf):
    """float64 (W_e, b_e, W_ih, W_hh, b_ih, b_hh) holding exactly the bf16
    values of the packed buffers. The kernels only see the MERGED r/z bias
    bf16(b_ih + b_hh); it is placed in b_ih[:2H] with b_hh[:2H] = 0, so the
    sum the oracle forms is the kernel's value bit for bit."""
    H = buf["w_e16"].shape[0]
    Wcat = buf["Wcat"].double()
    b_cat = buf["b_cat"].double()
    W_ih = Wcat[: 3 * H, :H].clone()
    W_hh = torch.cat([Wcat[: 2 * H, H:], Wcat[3 * H:, H:]])
    b_ih = b_cat[: 3 * H].clone()
    b_hh = torch.cat([torch.zeros_like(b_cat[: 2 * H]), b_cat[3 * H:]])
    return buf["w_e16"].double(), buf["b_e16"].double(), W_ih, W_hh, b_ih, b_hh


# --------------------------------------------------------------------------
# the loop
# --------------------------------------------------------------------------

def spmm(indptr, indices, x):
    """m[v] = sum over in-edges (u -> v) of x[u], in x's dtype."""
    N = indptr.numel() - 1
    deg = (indptr[1:] - indptr[:-1]).to(torch.int64)
    seg = torch.repeat_interleave(torch.arange(N, device=x.device), deg)
    out = torch.zeros(N, x.shape[1], dtype=x.dtype, device=x.device)
    out.index_add_(0, seg, x[indices.to(torch.int64)])
    return out


def _rnd(t):
    return t.to(torch.bfloat16).to(torch.float64)


def _same(t):
    return t


def _gates(m, h, W_ih, W_hh, b_ih, b_hh):
    H = h.shape[1]
    gi = m @ W_ih.t() + b_ih
    gh = h @ W_hh.t() + b_hh
    pre_r = gi[:, :H] + gh[:, :H]
    pre_z = gi[:, H:2 * H] + gh[:, H:2 * H]
    pre_in = gi[:, 2 * H:]
    hn = gh[:, 2 * H:]
    r = torch.sigmoid(pre_r)
    z = torch.sigmoid(pre_z)
    n = torch.tanh(pre_in + r * hn)
    return pre_r, pre_z, pre_in, hn, r, z, n, (1.0 - z) * n + z * h


GRAD_NAMES = ("grad_x", "gW_e", "gb_e", "gW_ih", "gW_hh", "gb_ih", "gb_hh")
OUT_NAMES = ("h_final",) + GRAD_NAMES


def ggnn_exact(x, csr, W_e, b_e, W_ih, W_hh, b_ih, b_hh, S, grad_out=None):
    """Autograd float64 loop. Returns {"h_final"} and, with grad_out, every
    gradient under GRAD_NAMES (loss = <h_final, grad_out>)."""
    leaves = [t.detach().double().clone().requires_grad_(True)
              for t in (x, W_e, b_e, W_ih, W_hh, b_ih, b_hh)]
    h, We, be, Wih, Whh, bih, bhh = leaves
    for _ in range(S):
        wh = h @ We.t() + be
        m = spmm(csr.indptr, csr.indices, wh)
        h = _gates(m, h, Wih, Whh, bih, bhh)[-1]
    out = {"h_final": h.detach()}
    if grad_out is not None:
        (h * grad_out.double()).sum().backward()
        for name, leaf in zip(GRAD_NAMES, leaves):
            out[name] = leaf.grad
    return out


def ggnn_emulated(x, csr, W_e, b_e, W_ih, W_hh, b_ih, b_hh, S, grad_out=None, rounding=True):
    """The loop as the kernels stage it. Forward roundings: wh, M[s], HH[s+1],
    R, Z, Nn, HN (n is computed from the UNROUNDED r and hn, as the fused
    gate epilogue does). Backward roundings: Ggicat[s], grad_A, Gwh[s],
    grad_hd and the running grad_h; weight and bias grads are sums of
    products of those rounded tensors, left unrounded (fp32 outputs)."""
    q = _rnd if rounding else _same
    f64 = torch.float64
    h = x.detach().to(f64)
    W_e, b_e, W_ih, W_hh, b_ih, b_hh = (t.detach().to(f64)
                                        for t in (W_e, b_e, W_ih, W_hh, b_ih, b_hh))
    H = h.shape[1]
    HHs, Ms, Rs, Zs, Ns, HNs = [h], [], [], [], [], []
    for _ in range(S):
        wh = q(h @ W_e.t() + b_e)
        m = q(spmm(csr.indptr, csr.indices, wh))
        _, _, _, hn, r, z, n, h_new = _gates(m, h, W_ih, W_hh, b_ih, b_hh)
        h = q(h_new)
        HHs.append(h), Ms.append(m), Rs.append(q(r)), Zs.append(q(z))
        Ns.append(q(n)), HNs.append(q(hn))
    out = {"h_final": h}
    if grad_out is None:
        return out
    # Wcat (4H, 2H) = [[W_ir|W_hr],[W_iz|W_hz],[W_in|0],[0|W_hn]]
    Wcat = torch.zeros(4 * H, 2 * H, dtype=f64, device=h.device)
    Wcat[: 3 * H, :H] = W_ih
    Wcat[: 2 * H, H:] = W_hh[: 2 * H]
    Wcat[3 * H:, H:] = W_hh[2 * H:]
    gWcat = torch.zeros_like(Wcat)
    cs4 = torch.zeros(4 * H, dtype=f64, device=h.device)
    gW_e = torch.zeros(H, H, dtype=f64, device=h.device)
    gb_e = torch.zeros(H, dtype=f64, device=h.device)
    aWcat, acs4, aW_e, ab_e = (torch.zeros_like(t) for t in (gWcat, cs4, gW_e, gb_e))
    grad_h = grad_out.detach().to(f64)
    for s in range(S - 1, -1, -1):
        hv, m, r, z, n, hn = HHs[s], Ms[s], Rs[s], Zs[s], Ns[s], HNs[s]
        go = grad_h
        dn = go * (1.0 - z)
        dz = go * (hv - n)
        dpn = dn * (1.0 - n * n)
        dpr = dpn * hn * r * (1.0 - r)
        dpz = dz * z * (1.0 - z)
        ggic = q(torch.cat([dpr, dpz, dpn, dpn * r], 1))
        grad_hd = q(go * z)
        grad_A = q(ggic @ Wcat)
        gwh = q(spmm(csr.t_indptr, csr.t_indices, grad_A[:, :H].contiguous()))
        grad_h = q(gwh @ W_e + grad_hd + grad_A[:, H:])
        gWcat += ggic.t() @ torch.cat([m, hv], 1)
        cs4 += ggic.sum(0)
        gW_e += gwh.t() @ hv
        gb_e += gwh.sum(0)
        aWcat += ggic.abs().t() @ torch.cat([m, hv], 1).abs()
        acs4 += ggic.abs().sum(0)
        aW_e += gwh.abs().t() @ hv.abs()
        ab_e += gwh.abs().sum(0)
    # the same reductions over absolute values: sum_k |a_k b_k| per output
    # element, the magnitude an accumulation-order bound scales with
    out["abs"] = dict(
        gW_e=aW_e, gb_e=ab_e, gW_ih=aWcat[: 3 * H, :H],
        gW_hh=torch.cat([aWcat[: 2 * H, H:], aWcat[3 * H:, H:]]),
        gb_ih=acs4[: 3 * H], gb_hh=torch.cat([acs4[: 2 * H], acs4[3 * H:]]),
    )
    out.update(
        grad_x=grad_h, gW_e=gW_e, gb_e=gb_e,
        gW_ih=gWcat[: 3 * H, :H],
        gW_hh=torch.cat([gWcat[: 2 * H, H:], gWcat[3 * H:, H:]]),
        gb_ih=cs4[: 3 * H],
        gb_hh=torch.cat([cs4[: 2 * H], cs4[3 * H:]]),
    )
    return out


def step_exact(h_s, M_s, csr, W_e, b_e, W_ih, W_hh, b_ih, b_hh):
    """One teacher-forced step in float64. `wh` and `m` follow from h_s; the
    gates follow from the GIVEN M_s and h_s (pass the kernel's own tensors).
    The `*_abs` entries are the same sums over absolute values, i.e. the
    magnitudes the fp32 accumulation bounds scale with."""
    f64 = torch.float64
    h = h_s.to(f64)
    M = M_s.to(f64)
    H = h.shape[1]
    wh = h @ W_e.t() + b_e
    wh_abs = h.abs() @ W_e.abs().t() + b_e.abs()
    m = spmm(csr.indptr, csr.indices, wh)
    pre_r, pre_z, pre_in, hn, r, z, n, h_new = _gates(M, h, W_ih, W_hh, b_ih, b_hh)
    gi_abs = M.abs() @ W_ih.abs().t() + b_ih.abs()
    gh_abs = h.abs() @ W_hh.abs().t() + b_hh.abs()
    return {
        "wh": wh, "wh_abs": wh_abs, "m": m,
        "m_abs": spmm(csr.indptr, csr.indices, wh.abs()),
        "m_wh_abs": spmm(csr.indptr, csr.indices, wh_abs),
        "pre_r": pre_r, "pre_z": pre_z, "pre_in": pre_in, "hn": hn,
        "pre_r_abs": gi_abs[:, :H] + gh_abs[:, :H],
        "pre_z_abs": gi_abs[:, H:2 * H] + gh_abs[:, H:2 * H],
        "pre_in_abs": gi_abs[:, 2 * H:], "hn_abs": gh_abs[:, 2 * H:],
        "r": r, "z": z, "n": n, "h_new": h_new,
    }


def rel_l2(got, ref):
    d = (got.double() - ref.double()).norm()
    return float(d / ref.double().norm().clamp_min(1e-300))
