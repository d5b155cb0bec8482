"""Graph-level flow-GNN head (csrc/graph_head.hip): node-chunked gate +
attention pool and the f32-MFMA 3-layer MLP.

Every reference is float64 on the GPU, computed from the SAME inputs the
kernels see (x pre-quantised to bf16, weights fp32).

Pool bounds (per element, computed from the data):
  bf16 outputs  |got - ref| <= 2^-8 |ref| + acc, one bf16 rounding of the
                reference plus a worst-case fp32 accumulation term;
    pooled      acc = n 2^-23 sum_v |alpha_v x_vd|   (n = segment size)
    gx1/gx2     gx_vd = alpha_v go_d + dgate_v wg_d with
                dgate_v = alpha_v (s_v - dot), s_v = <go, x_v> (256 terms),
                dot = <go, pooled> (256 terms over an n-term pooled row):
                acc = 2^-23 |alpha_v go_d|
                    + (256 + n) 2^-23 alpha_v (S_v + sum_u alpha_u S_u) |wg_d|,
                S_v = sum_d |go_d x_vd|
  dwg / dbg     |got - ref| <= N 2^-23 sum_v |dgate_v x_vd|  (resp. |dgate_v|)

MLP bound (per output tensor, relative L2 error against float64):
  err_new <= max(4 err_torch_fp32, L K 2^-24)
with err_torch_fp32 the error of the plain fp32 torch composition on the
GPU, K the longest reduction (256 for activations and dx, B for weight
grads) and L the number of reductions chained on that output's value path:
logits 3 (two layers + GEMV); dx 2 (dh1, dx); dW1, db1 2 (dh1, then the sum
over rows); dW2 2 (h1, then rows); db2 1; dW3 3 (h2's two layers, then
rows); db3 1. dx is bf16, so its bound gains one bf16 rounding (2^-8).
"""

import pytest
import torch
from torch import nn

pytestmark = pytest.mark.gpu

# the issue's sizes, plus 10 and 65: the 10 ends a graph exactly on a
# 64-node chunk boundary (node 256), the 65 starts on that boundary and
# ends one node past the next one
SEGS = [1, 2, 3, 15, 16, 17, 63, 64, 65, 0, 10, 65, 500, 1500]
CHUNK = 64
MLP_BS = [1, 15, 16, 17, 33, 257]


class _Stub:
    def __init__(self, node_offsets):
        self.node_offsets = node_offsets


def _dummy_first(params):
    """A 1-element parameter ahead of the real ones: every flat view then
    sits at an odd element offset (4-byte aligned only)."""
    return [nn.Parameter(torch.zeros(1, device="cuda"))] + list(params)


# --------------------------------------------------------------------------
# pool
# --------------------------------------------------------------------------

_POOL = {}


def _pool_case():
    """Inputs + float64 reference, built once and never modified."""
    if _POOL:
        return _POOL
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(77)
    offs = [0]
    for s in SEGS:
        offs.append(offs[-1] + s)
    N = offs[-1]
    assert offs[11] == 4 * CHUNK and offs[12] == 5 * CHUNK + 1
    x1 = torch.randn(N, 128, generator=gen).to(torch.bfloat16).to(dev)
    x2 = torch.randn(N, 128, generator=gen).to(torch.bfloat16).to(dev)
    torch.manual_seed(77)
    gate = nn.Linear(256, 1)
    wg = gate.weight.detach().reshape(-1).to(dev)
    bg = gate.bias.detach().to(dev)
    go = (torch.randn(len(SEGS), 256, generator=gen) / 16).to(torch.bfloat16).to(dev)
    node_offsets = torch.tensor(offs, dtype=torch.int32, device=dev)

    x = torch.cat([x1, x2], -1).double().requires_grad_(True)
    w64 = wg.double().requires_grad_(True)
    b64 = bg.double().requires_grad_(True)
    logit = x @ w64 + b64
    rows, alphas = [], []
    for i, s in enumerate(SEGS):
        lo, hi = offs[i], offs[i + 1]
        if s == 0:
            rows.append(torch.zeros(256, dtype=torch.float64, device=dev))
            continue
        a = torch.softmax(logit[lo:hi], 0)
        alphas.append(a)
        rows.append((a[:, None] * x[lo:hi]).sum(0))
    pooled = torch.stack(rows)
    (pooled * go.double()).sum().backward()
    alpha = torch.cat(alphas).detach()
    xd = x.detach()
    seg_id = torch.repeat_interleave(
        torch.arange(len(SEGS), device=dev), torch.tensor(SEGS, device=dev))
    n_of = torch.tensor(SEGS, device=dev, dtype=torch.float64)
    # accumulation terms
    ax = alpha[:, None] * xd.abs()
    pooled_acc = torch.zeros(len(SEGS), 256, dtype=torch.float64, device=dev)
    pooled_acc.index_add_(0, seg_id, ax)
    pooled_acc = pooled_acc * n_of[:, None] * 2.0 ** -23
    go_n = go.double()[seg_id]                       # (N, 256)
    S_v = (go_n.abs() * xd.abs()).sum(1)             # (N,)
    aS = torch.zeros(len(SEGS), dtype=torch.float64, device=dev)
    aS.index_add_(0, seg_id, alpha * S_v)
    gx_acc = (2.0 ** -23 * alpha[:, None] * go_n.abs()
              + ((256 + n_of[seg_id]) * 2.0 ** -23 * alpha * (S_v + aS[seg_id]))[:, None]
              * wg.double().abs()[None, :])
    s_v = (go_n * xd).sum(1)
    dot = torch.zeros(len(SEGS), dtype=torch.float64, device=dev)
    dot.index_add_(0, seg_id, alpha * s_v)
    dgate = alpha * (s_v - dot[seg_id])
    dwg_bound = N * 2.0 ** -23 * (dgate.abs()[:, None] * xd.abs()).sum(0)
    dbg_bound = N * 2.0 ** -23 * dgate.abs().sum()
    _POOL.update(
        x1=x1, x2=x2, wg=wg, bg=bg, go=go, node_offsets=node_offsets, N=N,
        pooled=pooled.detach(), gx=x.grad, dwg=w64.grad, dbg=b64.grad,
        pooled_acc=pooled_acc, gx_acc=gx_acc, dwg_bound=dwg_bound, dbg_bound=dbg_bound)
    return _POOL


def _gate_module(c):
    gate = nn.Linear(256, 1).cuda()
    with torch.no_grad():
        gate.weight.copy_(c["wg"][None, :])
        gate.bias.copy_(c["bg"])
    return gate


def _run_pool(c, gate, times=1):
    from deepdfa_amd.ops.flowgnn import gate_pool

    x1 = c["x1"].clone().requires_grad_(True)
    x2 = c["x2"].clone().requires_grad_(True)
    out = None
    for _ in range(times):
        x1.grad = x2.grad = None
        out = gate_pool(x1, x2, gate, _Stub(c["node_offsets"]))
        out.backward(c["go"])
    torch.cuda.synchronize()
    return out.detach(), torch.cat([x1.grad, x2.grad], -1)


def _assert_within(name, got, ref, bound):
    err = (got.double() - ref).abs()
    worst = float((err - bound).max())
    print(f"{name}: max err {float(err.max()):.3e}  max(err - bound) {worst:.3e}")
    assert bool((err <= bound).all()), (name, float(err.max()), worst)


def test_pool_matches_float64():
    c = _pool_case()
    gate = _gate_module(c)
    pooled, gx = _run_pool(c, gate)
    assert pooled.dtype == torch.bfloat16 and gx.dtype == torch.bfloat16
    empty = SEGS.index(0)
    assert float(pooled[empty].float().abs().max()) == 0.0
    _assert_within("pooled", pooled, c["pooled"],
                   2.0 ** -8 * c["pooled"].abs() + c["pooled_acc"])
    _assert_within("gx", gx, c["gx"], 2.0 ** -8 * c["gx"].abs() + c["gx_acc"])
    _assert_within("dwg", gate.weight.grad.reshape(-1), c["dwg"], c["dwg_bound"])
    _assert_within("dbg", gate.bias.grad.reshape(-1), c["dbg"].reshape(-1),
                   c["dbg_bound"].reshape(-1))


def test_pool_grads_accumulate_into_live_views():
    from deepdfa_amd.parallel.optim import FlatAdamW

    c = _pool_case()
    gate = _gate_module(c)
    opt = FlatAdamW(_dummy_first(gate.parameters()), lr=1e-3)
    assert gate.weight.data_ptr() % 16 != 0
    opt.zero_grad()
    _run_pool(c, gate, times=2)
    _assert_within("dwg x2", gate.weight.grad.reshape(-1), 2 * c["dwg"], 2 * c["dwg_bound"])
    _assert_within("dbg x2", gate.bias.grad.reshape(-1), 2 * c["dbg"].reshape(-1),
                   2 * c["dbg_bound"].reshape(-1))
    assert float(gate.weight.grad.abs().max()) > 0


# --------------------------------------------------------------------------
# MLP
# --------------------------------------------------------------------------

_MLP = {}
_NAMES = ["logits", "dx", "dW1", "db1", "dW2", "db2", "dW3", "db3"]
_LAYERS = {"logits": 3, "dx": 2, "dW1": 2, "db1": 2, "dW2": 2, "db2": 1, "dW3": 3, "db3": 1}


def _compose(x, W1, b1, W2, b2, W3, b3, dl):
    x = x.clone().requires_grad_(True)
    ps = [t.clone().requires_grad_(True) for t in (W1, b1, W2, b2, W3, b3)]
    h1 = torch.relu(torch.nn.functional.linear(x, ps[0], ps[1]))
    h2 = torch.relu(torch.nn.functional.linear(h1, ps[2], ps[3]))
    logits = torch.nn.functional.linear(h2, ps[4], ps[5]).squeeze(-1)
    logits.backward(dl)
    return {"logits": logits.detach(), "dx": x.grad, "dW1": ps[0].grad, "db1": ps[1].grad,
            "dW2": ps[2].grad, "db2": ps[3].grad, "dW3": ps[4].grad, "db3": ps[5].grad}


def _mlp_case(B):
    """Inputs, float64 reference and fp32-torch errors for B rows, built once."""
    if B in _MLP:
        return _MLP[B]
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(500 + B)
    torch.manual_seed(500 + B)
    lins = [nn.Linear(256, 256), nn.Linear(256, 256), nn.Linear(256, 1)]
    w = [t.detach().to(dev) for l in lins for t in (l.weight, l.bias)]
    x = torch.randn(B, 256, generator=gen).to(torch.bfloat16).to(dev)
    y = (torch.rand(B, generator=gen) < 0.1).float()
    dl = ((torch.sigmoid(torch.randn(B, generator=gen)) - y) / B).to(dev)
    ref = _compose(x.double(), *[t.double() for t in w], dl.double())
    t32 = _compose(x.float(), *w, dl)
    err32 = {k: _rel(t32[k], ref[k]) for k in _NAMES}
    _MLP[B] = dict(x=x, w=w, dl=dl, ref=ref, err32=err32)
    return _MLP[B]


def _rel(got, ref):
    ref = ref.double().reshape(-1)
    num = torch.linalg.vector_norm(got.double().reshape(-1) - ref)
    return float(num / torch.linalg.vector_norm(ref).clamp(min=1e-300))


def _bound(c, k, B):
    K = 256 if k in ("logits", "dx") else B
    b = max(4 * c["err32"][k], _LAYERS[k] * K * 2.0 ** -24)
    return b + (2.0 ** -8 if k == "dx" else 0.0)


def _lin_modules(c):
    lins = [nn.Linear(256, 256), nn.Linear(256, 256), nn.Linear(256, 1)]
    lins = [l.cuda() for l in lins]
    with torch.no_grad():
        for l, (wt, bs) in zip(lins, zip(c["w"][0::2], c["w"][1::2])):
            l.weight.copy_(wt)
            l.bias.copy_(bs)
    return lins


def _run_mlp(c, lins, times=1):
    from deepdfa_amd.ops.flowgnn import mlp3

    xf = c["x"].clone().requires_grad_(True)
    logits = None
    for _ in range(times):
        xf.grad = None
        logits = mlp3(xf, *lins)
        logits.backward(c["dl"])
    torch.cuda.synchronize()
    got = {"logits": logits.detach(), "dx": xf.grad}
    for i, n in enumerate(("1", "2", "3")):
        got["dW" + n] = lins[i].weight.grad
        got["db" + n] = lins[i].bias.grad
    return got


def _check_mlp(c, got, B, scale=1.0, names=_NAMES):
    bad = []
    for k in names:
        g = got[k].double() / (scale if k not in ("logits", "dx") else 1.0)
        err, bound = _rel(g, c["ref"][k]), _bound(c, k, B)
        print(f"B={B} {k}: err_new={err:.3e} err_torch_fp32={c['err32'][k]:.3e} "
              f"bound={bound:.3e}")
        if not err <= bound:
            bad.append((k, err, bound))
    assert not bad, bad


@pytest.mark.parametrize("B", MLP_BS)
def test_mlp_matches_float64(B):
    c = _mlp_case(B)
    got = _run_mlp(c, _lin_modules(c))
    assert got["logits"].dtype == torch.float32 and got["dx"].dtype == torch.bfloat16
    assert got["logits"].shape == (B,)
    _check_mlp(c, got, B)


@pytest.mark.parametrize("B", [17, 257])
def test_mlp_grads_accumulate_into_live_views(B):
    from deepdfa_amd.parallel.optim import FlatAdamW

    c = _mlp_case(B)
    lins = _lin_modules(c)
    opt = FlatAdamW(_dummy_first(p for l in lins for p in l.parameters()), lr=1e-3)
    assert lins[0].weight.data_ptr() % 8 != 0  # flat views: 4-byte aligned only
    opt.zero_grad()
    got = _run_mlp(c, lins, times=2)
    _check_mlp(c, got, B, scale=2.0)


# --------------------------------------------------------------------------
# capture: no stale derived buffer survives a master-weight update
# --------------------------------------------------------------------------


def test_captured_replay_sees_updated_master_weight():
    from deepdfa_amd.graph.synthetic import synthetic_cfg_batch
    from deepdfa_amd.models import FlowGNNGGNNModule
    from deepdfa_amd.ops import transformer as tops
    from deepdfa_amd.parallel.optim import FlatAdamW

    torch.manual_seed(3)
    dev = torch.device("cuda:0")
    model = FlowGNNGGNNModule(input_dim=1002, hidden_dim=32, n_steps=2,
                              num_output_layers=3).to(dev)
    g = synthetic_cfg_batch(8, seed=0).to(dev)
    label = model.get_label(g)
    opt = FlatAdamW(model.parameters(), lr=1e-3)
    w = model.output_layer[0].weight

    def run():
        with torch.autocast(device_type="cuda", dtype=torch.bfloat16):
            logits = model(g, {})
        loss = model.loss_fn(logits.float(), label)
        opt.zero_grad()
        loss.backward()
        return logits.detach()

    saved = tops.CAPTURE_REFRESH[0]
    tops.CAPTURE_REFRESH[0] = True
    try:
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            run()
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        cg = torch.cuda.CUDAGraph()
        with torch.cuda.graph(cg):
            static_logits = run()
        cg.replay()
        torch.cuda.synchronize()
        first = static_logits.clone()
        with torch.no_grad():
            w.mul_(-1.5)
        cg.replay()
        torch.cuda.synchronize()
        second = static_logits.clone()
        expect = run()
        torch.cuda.synchronize()
    finally:
        tops.CAPTURE_REFRESH[0] = saved
    assert bool(torch.isfinite(second).all())
    assert float((second - first).abs().max()) > 1e-3
    assert torch.allclose(second, expect, atol=1e-4, rtol=1e-3), (
        float((second - expect).abs().max()))
