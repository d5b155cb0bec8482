"""Stale-cache tests for every op that keeps derived weights through
ops/_weights.py `derived`: after the master weights change — by a FlatAdamW
step (raw kernel write + epoch bump), by a torch optimizer step or by a
torch-level copy_ (version bumps) — the op's next forward must be
BIT-IDENTICAL to the same op on freshly built parameters that hold the same
weights and carry no cache. Both runs launch the same forward kernel on the
same inputs and these forward kernels use no atomics, so no tolerance is
needed. Shapes are the smallest the dispatch rules admit."""

import pytest
import torch
from torch import nn

pytestmark = pytest.mark.gpu


class _Site:
    """One op call over `params`. `modules` are further cache owners.
    `build()` twice gives identical inputs (fixed generator); the parameter
    order is the FlatAdamW layout order."""

    def __init__(self, params, run, modules=()):
        self.params, self.run, self.modules = list(params), run, list(modules)


def _gen():
    return torch.Generator().manual_seed(1234)


def _rand(g, *shape, scale=1.0):
    return (torch.randn(*shape, generator=g) * scale).cuda()


def _par(g, *shape):
    return nn.Parameter(_rand(g, *shape, scale=0.1))


def _linear():
    from deepdfa_amd.ops import transformer as tops

    g = _gen()
    w, b = _par(g, 128, 64), _par(g, 128)
    x = _rand(g, 128, 64).bfloat16()
    return _Site([w, b], lambda: tops.fused_linear(x, w, b))


def _qkv(bias, interleaved=False):
    def build():
        from deepdfa_amd.ops import transformer as tops

        g = _gen()
        ws = [_par(g, 128, 128) for _ in range(3)]
        bs = [_par(g, 128) for _ in range(3)] if bias else [None] * 3
        x = _rand(g, 128, 128).bfloat16()
        if interleaved:  # the nn.Module order: flat shadows are NOT adjacent
            params = [p for pair in zip(ws, bs) for p in pair]
        else:
            params = ws + [b for b in bs if b is not None]
        return _Site(params, lambda: tops.fused_qkv(x, *ws, *bs))

    return build


def _kv(spaced=False):
    def build():
        from deepdfa_amd.ops import transformer as tops

        g = _gen()
        wk, wv = _par(g, 128, 128), _par(g, 128, 128)
        x = _rand(g, 128, 128).bfloat16()
        params = [wk, _par(g, 8), wv] if spaced else [wk, wv]
        return _Site(params, lambda: tops.fused_kv(x, wk, wv))

    return build


def _lmhead():
    from deepdfa_amd.ops import transformer as tops

    g = _gen()
    w = _par(g, 200, 64)  # V = 200 pads to 256
    h = _rand(g, 128, 64).bfloat16()
    tgt = torch.randint(0, 200, (128,), generator=g).cuda()
    tgt[::7] = -100
    return _Site([w], lambda: tops.lmhead_cross_entropy(h, w, tgt, 0.5))


def _node_head():
    from deepdfa_amd.ops import flowgnn as fops

    g = _gen()
    lins = [nn.Linear(256, 256), nn.Linear(256, 256), nn.Linear(256, 1)]
    for lin in lins:
        lin.weight = _par(g, *lin.weight.shape)
        lin.bias = _par(g, *lin.bias.shape)
    h, fe = _rand(g, 64, 128).bfloat16(), _rand(g, 64, 128).bfloat16()
    return _Site([p for lin in lins for p in lin.parameters()],
                 lambda: fops.node_head(h, fe, *lins), modules=lins)


def _tables():
    from deepdfa_amd.models import FlowGNNGGNNModule
    from deepdfa_amd.models.flow_gnn import ALL_FEATS

    g = _gen()
    model = FlowGNNGGNNModule(input_dim=16, hidden_dim=32, n_steps=1).cuda()
    for of in ALL_FEATS:
        model.all_embeddings[of].weight = _par(g, 16, 32)

    class _Graph:
        ndata = {f"_ABS_DATAFLOW_{of}": torch.randint(0, 16, (8,), generator=g).cuda()
                 for of in ALL_FEATS}

    def run():
        with torch.no_grad():  # the no-grad route is the cached one
            return model._embed(_Graph)

    return _Site([model.all_embeddings[of].weight for of in ALL_FEATS], run,
                 modules=[model])


SITES = {
    "linear": _linear,
    "qkv_bias": _qkv(True),
    "qkv_bias_interleaved": _qkv(True, interleaved=True),
    "qkv_nobias": _qkv(False),
    "kv": _kv(),
    "kv_spaced": _kv(spaced=True),
    "lmhead": _lmhead,
    "node_head": _node_head,
    "tables": _tables,
}
# under FlatAdamW these read a zero-copy view of the shadow: nothing cached
VIEW_ONLY_WHEN_FLAT = {"qkv_nobias", "kv"}


def _optimizer(site, flat):
    if flat:
        from deepdfa_amd.parallel.optim import FlatAdamW

        return FlatAdamW(site.params, lr=0.05)
    return torch.optim.SGD(site.params, lr=0.05)


def _step(site, opt, flat):
    g = torch.Generator().manual_seed(99)
    if flat:
        opt.flat_g.copy_(torch.randn(opt.flat_g.numel(), generator=g))
    else:
        for p in site.params:
            p.grad = torch.randn(p.shape, generator=g).cuda()
    opt.step()


def _copy(site, opt, flat):
    g = torch.Generator().manual_seed(98)
    with torch.no_grad():
        for p in site.params:
            p.copy_(torch.randn(p.shape, generator=g) * 0.1)


def _fresh_like(name, site):
    fresh = SITES[name]()
    with torch.no_grad():
        for q, p in zip(fresh.params, site.params):
            q.copy_(p)
    return fresh


def _cached_ptrs(site):
    """data_ptr of every tensor held in any `_dfa_*_cache` slot."""
    def tensors(obj):
        if isinstance(obj, torch.Tensor):
            yield obj
        elif isinstance(obj, dict):
            for v in obj.values():
                yield from tensors(v)
        elif isinstance(obj, (tuple, list)):
            for v in obj:
                yield from tensors(v)

    out = {}
    for i, owner in enumerate(site.params + site.modules):
        for slot, entry in vars(owner).items():
            if slot.startswith("_dfa_") and slot.endswith("_cache"):
                for j, t in enumerate(tensors(entry)):
                    out[(i, slot, j)] = t.data_ptr()
    return out


@pytest.mark.parametrize("change", [_step, _copy], ids=["step", "copy"])
@pytest.mark.parametrize("flat", [False, True], ids=["plain", "flat"])
@pytest.mark.parametrize("name", list(SITES))
def test_forward_after_weight_change_matches_fresh_module(name, flat, change):
    site = SITES[name]()
    opt = _optimizer(site, flat)
    before = site.run().detach().clone()  # populates the cache
    if not (flat and name in VIEW_ONLY_WHEN_FLAT):
        assert _cached_ptrs(site)
    change(site, opt, flat)
    got = site.run().detach()
    want = _fresh_like(name, site).run().detach()
    assert not torch.equal(got, before), "the weight change did not reach the output"
    assert torch.equal(got, want), float((got.float() - want.float()).abs().max())
    # and a second change of the other kind on top of the first
    (_copy if change is _step else _step)(site, opt, flat)
    got = site.run().detach()
    want = _fresh_like(name, site).run().detach()
    assert torch.equal(got, want), float((got.float() - want.float()).abs().max())


@pytest.mark.parametrize("flat", [False, True], ids=["plain", "flat"])
@pytest.mark.parametrize("name", list(SITES))
def test_capture_refresh_keeps_every_cached_buffer_in_place(name, flat):
    from deepdfa_amd.ops import transformer as tops

    site = SITES[name]()
    opt = _optimizer(site, flat)
    site.run()
    ptrs = _cached_ptrs(site)
    if not (flat and name in VIEW_ONLY_WHEN_FLAT):
        assert ptrs
    if flat and name == "qkv_bias":  # the packed fp32 bias over the shadow view
        assert any(slot == "_dfa_qkv_bias_cache" for _, slot, _ in ptrs)
    saved = tops.CAPTURE_REFRESH[0]
    tops.CAPTURE_REFRESH[0] = True
    try:
        _step(site, opt, flat)
        for _ in range(2):
            got = site.run().detach()
            assert _cached_ptrs(site) == ptrs
    finally:
        tops.CAPTURE_REFRESH[0] = saved
    want = _fresh_like(name, site).run().detach()
    assert torch.equal(got, want)
