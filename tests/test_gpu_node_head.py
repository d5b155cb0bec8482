"""Fused node-level head (csrc/node_head.hip) and node-style training on
the GPU.

Kernel numerics use two CPU oracles computed once per N:
  A: fp32 torch with the kernel's rounding points (bf16 inputs/weights,
     H1, H2, dH1, dH2, dh, dfe rounded to bf16, fp32 accumulation; logits
     are taken from the unrounded fp32 layer-2 activations, as the kernel
     takes them from its accumulators);
  B: the same in pure fp32, no intermediate rounding.
The kernel can differ from A only by summation order and the occasional
one-ulp flip of a rounded intermediate — a small subset of the roundings
that separate A from B — so every output must satisfy
  max|kernel - A| <= max|A - B| + 1e-6 * max|A|.
"""

import logging

import pytest
import torch
from torch import nn

pytestmark = pytest.mark.gpu

NS = [1, 63, 64, 65, 247]
NAMES = ["logits", "dh", "dfe", "dW1", "db1", "dW2", "db2", "dW3", "db3"]


def _r(t):
    return t.to(torch.bfloat16).float()


def _oracle(p, rounded):
    r = _r if rounded else (lambda t: t)
    x = torch.cat([p["h"], p["fe"]], -1)
    h1 = r(torch.relu(x @ p["W1"].t() + p["b1"]))
    h2f = torch.relu(h1 @ p["W2"].t() + p["b2"])
    logits = h2f @ p["w3"] + p["b3"]
    h2 = r(h2f)
    dl = p["dl"]
    dh2 = r(dl[:, None] * p["w3"][None, :]) * (h2 > 0)
    dh1 = r((dh2 @ p["W2"]) * (h1 > 0))
    dx = r(dh1 @ p["W1"])
    return {
        "logits": logits, "dh": dx[:, :128], "dfe": dx[:, 128:],
        "dW1": dh1.t() @ x, "db1": dh1.sum(0), "dW2": dh2.t() @ h1,
        "db2": dh2.sum(0), "dW3": (h2.t() @ dl)[None, :], "db3": dl.sum()[None],
        "H1": h1, "H2": h2, "dH1": dh1, "dH2": dh2,
    }


_CASES = {}


def _case(N):
    """Inputs + both oracles for N nodes, built once and never modified."""
    if N in _CASES:
        return _CASES[N]
    gen = torch.Generator().manual_seed(1000 + N)
    torch.manual_seed(1000 + N)
    lins = [nn.Linear(256, 256), nn.Linear(256, 256), nn.Linear(256, 1)]  # nn.Linear init
    p = {
        "h": _r(0.5 * torch.randn(N, 128, generator=gen)),
        "fe": _r(0.5 * torch.randn(N, 128, generator=gen)),
        "W1": _r(lins[0].weight.detach()), "b1": lins[0].bias.detach().clone(),
        "W2": _r(lins[1].weight.detach()), "b2": lins[1].bias.detach().clone(),
        "w3": lins[2].weight.detach().reshape(-1).clone(),
        "b3": lins[2].bias.detach().clone(),
    }
    # BCE-like upstream grads: (sigmoid(z) - y) / N
    y = (torch.rand(N, generator=gen) < 0.1).float()
    p["dl"] = (torch.sigmoid(torch.randn(N, generator=gen)) - y) / N
    with torch.no_grad():
        A, B = _oracle(p, True), _oracle(p, False)
    _CASES[N] = (p, A, B)
    return _CASES[N]


def _gpu_modules(p):
    lins = [nn.Linear(256, 256), nn.Linear(256, 256), nn.Linear(256, 1)]
    with torch.no_grad():
        lins[0].weight.copy_(p["W1"]); lins[0].bias.copy_(p["b1"])
        lins[1].weight.copy_(p["W2"]); lins[1].bias.copy_(p["b2"])
        lins[2].weight.copy_(p["w3"][None, :]); lins[2].bias.copy_(p["b3"])
    return [l.cuda() for l in lins]


def _check(got, A, B, names, N):
    bad = []
    for k in names:
        a, b, g = A[k], B[k], got[k].detach().float().cpu().reshape(A[k].shape)
        err = float((g - a).abs().max())
        bound = float((a - b).abs().max()) + 1e-6 * float(a.abs().max())
        print(f"N={N} {k}: max|kernel-A|={err:.3e} max|A-B|={float((a - b).abs().max()):.3e} "
              f"bound={bound:.3e}")
        if not err <= bound:
            bad.append((k, err, bound))
    assert not bad, bad


@pytest.mark.parametrize("N", NS)
def test_node_head_matches_oracles(N):
    from deepdfa_amd.ops.flowgnn import node_head

    p, A, B = _case(N)
    lin1, lin2, lin3 = _gpu_modules(p)
    h = p["h"].cuda().to(torch.bfloat16).requires_grad_()
    fe = p["fe"].cuda().to(torch.bfloat16).requires_grad_()
    logits = node_head(h, fe, lin1, lin2, lin3)
    assert logits.shape == (N,) and logits.dtype == torch.float32
    logits.backward(p["dl"].cuda())
    got = {
        "logits": logits, "dh": h.grad, "dfe": fe.grad,
        "dW1": lin1.weight.grad, "db1": lin1.bias.grad,
        "dW2": lin2.weight.grad, "db2": lin2.bias.grad,
        "dW3": lin3.weight.grad, "db3": lin3.bias.grad,
    }
    _check(got, A, B, NAMES, N)


def _ext_args(p):
    bf = torch.bfloat16
    return dict(
        h=p["h"].cuda().to(bf), fe=p["fe"].cuda().to(bf),
        W1=p["W1"].cuda().to(bf), W2=p["W2"].cuda().to(bf),
        b1=p["b1"].cuda(), b2=p["b2"].cuda(), w3=p["w3"].cuda(), b3=p["b3"].cuda(),
    )


@pytest.mark.parametrize("N", NS)
def test_no_save_logits_bit_identical(N):
    from deepdfa_amd.ops import load_ext

    ext = load_ext(required=True)
    a = _ext_args(_case(N)[0])
    saved = ext.node_head_fwd(**a, save=True)
    plain = ext.node_head_fwd(**a, save=False)
    assert len(saved) == 4 and len(plain) == 1
    assert torch.equal(saved[0], plain[0])


@pytest.mark.parametrize("N", [65, 247])
def test_tile_geometries_agree(N):
    """The 64-row tile (chosen by itself only from N >= 16384) against the
    32-row tile: same k order per element, so everything that is not an
    atomic sum is bit-identical."""
    from deepdfa_amd.ops import load_ext

    ext = load_ext(required=True)
    p, A, B = _case(N)
    assert ext.node_head_tile_rows(N) == 32 and ext.node_head_tile_rows(16384) == 64
    a = _ext_args(p)
    w1t, w2t = a["W1"].t().contiguous(), a["W2"].t().contiguous()
    dl = p["dl"].cuda()
    outs = {}
    for tile in (32, 64):
        logits, x, h1, h2 = ext.node_head_fwd(**a, save=True, tile_rows=tile)
        dh, dfe, dh1, dh2, dw3, db3 = ext.node_head_bwd(
            dl, h1, h2, w1t, w2t, a["w3"], tile_rows=tile)
        outs[tile] = dict(logits=logits, X=x, H1=h1, H2=h2, dh=dh, dfe=dfe,
                          dH1=dh1, dH2=dh2, dW3=dw3, db3=db3)
    for k in ("logits", "X", "H1", "H2", "dh", "dfe", "dH1", "dH2"):
        assert torch.equal(outs[32][k], outs[64][k]), k
    assert torch.equal(outs[64]["X"].float().cpu(), torch.cat([p["h"], p["fe"]], -1))
    _check(outs[64], A, B, ["logits", "dh", "dfe", "dW3", "db3"], N)
    # H1 depends on the inputs alone: at most one bf16 ulp (2^-7 relative)
    # from oracle A, plus fp32 summation noise around the ReLU's zero
    h1, a1 = outs[64]["H1"].float().cpu(), A["H1"]
    assert bool(((h1 - a1).abs() <= 2.0 ** -7 * a1.abs() + 1e-5).all())


def test_geometry_is_checked():
    from deepdfa_amd.ops import load_ext

    ext = load_ext(required=True)
    a = _ext_args(_case(63)[0])
    a["fe"] = a["fe"][:, :64].contiguous()
    with pytest.raises(RuntimeError, match="D1 = D2 = 128"):
        ext.node_head_fwd(**a, save=False)


def _node_model():
    from deepdfa_amd.models import FlowGNNGGNNModule

    torch.manual_seed(0)
    return FlowGNNGGNNModule(input_dim=1002, label_style="node").to("cuda")


def test_node_direct_grad_matches_autograd():
    """test_ddfa_direct_grad_accumulation_matches_autograd for node style."""
    from deepdfa_amd.graph.synthetic import synthetic_cfg_batch
    from deepdfa_amd.parallel.optim import FlatAdamW

    model = _node_model()
    g = synthetic_cfg_batch(8, seed=0).to("cuda")

    def step():
        with torch.autocast(device_type="cuda", dtype=torch.bfloat16):
            return model.training_step((g, {}))

    loss_ref = step()
    loss_ref.backward()
    ref = {n: p.grad.detach().clone() for n, p in model.named_parameters()}
    for p in model.parameters():
        p.grad = None
    model.metrics["train"].reset()

    opt = FlatAdamW(model.parameters(), lr=1e-3)
    opt.zero_grad()
    loss = step()
    loss.backward()
    assert torch.allclose(loss.float(), loss_ref.float(), atol=1e-4, rtol=1e-4)
    bad = []
    for n, p in model.named_parameters():
        r = ref[n].float()
        tol = 2e-4 + 2e-4 * float(r.abs().max())
        if not torch.allclose(p.grad.float(), r, atol=tol):
            bad.append((n, float((p.grad.float() - r).abs().max())))
    assert not bad, bad


def test_node_direct_grad_sums_over_microbatches():
    """test_direct_grad_accumulation_sums_over_microbatches for node style:
    node_head's wgrad/colsum/dW3/db3 writes must accumulate."""
    from deepdfa_amd.graph.synthetic import synthetic_cfg_batch
    from deepdfa_amd.parallel.optim import FlatAdamW

    model = _node_model()
    g = synthetic_cfg_batch(8, seed=0).to("cuda")
    opt = FlatAdamW(model.parameters(), lr=1e-3)

    def loss_fn():
        with torch.autocast(device_type="cuda", dtype=torch.bfloat16):
            return model.training_step((g, {}))

    opt.zero_grad()
    loss_fn().backward()
    once = opt.flat_g.detach().clone()
    opt.zero_grad()
    loss_fn().backward()
    loss_fn().backward()
    twice = opt.flat_g.detach().clone()
    err = (twice - 2 * once).abs().max() / once.abs().max().clamp(min=1e-8)
    assert float(err) < 1e-3, float(err)
    # the head's own parameters did receive gradient
    for p in model.output_layer.parameters():
        assert float(p.grad.abs().max()) > 0


def test_dispatch(monkeypatch):
    from deepdfa_amd.graph.synthetic import synthetic_cfg_batch
    from deepdfa_amd.models import FlowGNNGGNNModule
    from deepdfa_amd.ops import flowgnn as fops

    calls = []
    real = fops.node_head

    def counting(*a, **k):
        calls.append(1)
        return real(*a, **k)

    monkeypatch.setattr(fops, "node_head", counting)
    g = synthetic_cfg_batch(8, seed=0).to("cuda")
    node = _node_model()
    with torch.autocast(device_type="cuda", dtype=torch.bfloat16):
        out = node(g, {})
    assert len(calls) == 1
    assert out.shape == (g.num_nodes,) and bool(torch.isfinite(out).all())
    with torch.no_grad(), torch.autocast(device_type="cuda", dtype=torch.bfloat16):
        out2 = node(g, {})
    assert len(calls) == 2
    assert torch.allclose(out2, out.detach(), atol=1e-3, rtol=1e-3)

    graph = FlowGNNGGNNModule(input_dim=1002).to("cuda")
    with torch.autocast(device_type="cuda", dtype=torch.bfloat16):
        out = graph(g, {})
    assert len(calls) == 2 and out.shape == (g.num_graphs,)


def _fit(tmp_path, mode, **model_kw):
    from deepdfa_amd.data.datamodule import BigVulDatasetLineVDDataModule
    from deepdfa_amd.models import FlowGNNGGNNModule
    from deepdfa_amd.parallel.optim import FlatAdamW
    from deepdfa_amd.train.trainer import Trainer

    torch.manual_seed(0)
    dm = BigVulDatasetLineVDDataModule(batch_size=32, n_synthetic=400,
                                       undersample="v1.0", seed=0)
    model = FlowGNNGGNNModule(input_dim=dm.input_dim, hidden_dim=32, n_steps=5,
                              num_output_layers=3, label_style="node", **model_kw)
    trainer = Trainer(max_epochs=2, default_root_dir=str(tmp_path / mode),
                      precision="bf16", seed=0, graph_capture=(mode != "eager"))
    opt = FlatAdamW(model.to(trainer.device).parameters(), lr=1e-3,
                    weight_decay=1e-2, l2_mode=True)
    return trainer, trainer.fit(model, dm, optimizer=opt)["history"]


def _epoch_node_counts(epochs=2):
    from deepdfa_amd.data.datamodule import BigVulDatasetLineVDDataModule

    dm = BigVulDatasetLineVDDataModule(batch_size=32, n_synthetic=400,
                                       undersample="v1.0", seed=0)
    gen = torch.Generator().manual_seed(0)  # Trainer(seed=0)
    counts = []
    for _ in range(epochs):
        n = 0
        for batch in dm.train_dataloader(generator=gen, rank=0, world=1):
            g = batch[0] if isinstance(batch, tuple) else batch
            n += g.num_nodes
        counts.append(n)
    return counts


def test_node_fit_graph_capture_parity(tmp_path):
    """test_trainer_fit_graph_capture_parity with label_style="node", same
    bounds; the per-epoch metric totals are the real node counts."""
    results = {}
    for mode in ("eager", "capture"):
        trainer, results[mode] = _fit(tmp_path, mode)
        if mode == "capture":
            assert trainer.n_capture_buckets > 0
    nodes = _epoch_node_counts()
    for r_e, r_c, n in zip(results["eager"], results["capture"], nodes):
        assert abs(r_e["train_loss"] - r_c["train_loss"]) < 0.05, (r_e, r_c)
        tot_e = r_e["train_tp"] + r_e["train_fp"] + r_e["train_tn"] + r_e["train_fn"]
        tot_c = r_c["train_tp"] + r_c["train_fp"] + r_c["train_tn"] + r_c["train_fn"]
        assert tot_e == tot_c == n, (tot_e, tot_c, n)
        assert abs(r_e["train_f1"] - r_c["train_f1"]) < 0.15, (r_e, r_c)
    assert abs(results["eager"][-1]["val_loss"] - results["capture"][-1]["val_loss"]) < 0.05


def test_node_sampling_disables_capture(tmp_path, caplog):
    import math

    with caplog.at_level(logging.INFO, logger="deepdfa_amd.train.trainer"):
        trainer, hist = _fit(tmp_path, "capture", undersample_node_on_loss_factor=2)
    assert len(hist) == 2
    for row in hist:
        assert math.isfinite(row["train_loss"]) and math.isfinite(row["val_loss"])
    assert any("undersample_node_on_loss_factor" in r.getMessage() and "eager" in r.getMessage()
               for r in caplog.records)
    assert not any("step capture enabled" in r.getMessage() for r in caplog.records)
    assert trainer.n_capture_buckets == 0
