"""CPU tests for the two protocols of ops/_weights.py: the derived-weight
cache state machine (`derived`) and the direct-gradient predicates
(`direct_grads`, `packed_shadow`, `packed_grad`). The helpers are
device-agnostic; shadows and flat grads are simulated the way FlatAdamW
lays them out on the GPU (parallel/optim.py)."""

import pytest
import torch

from deepdfa_amd.ops import _weights as W
from deepdfa_amd.ops import transformer as tops


class _Owner:
    pass


class _Cache:
    """A derived bf16 cast of one source, counting alloc/fill calls."""

    def __init__(self, src, extra=()):
        self.owner, self.src, self.extra = _Owner(), src, extra
        self.allocs = self.fills = 0

    def _alloc(self):
        self.allocs += 1
        return (torch.empty(self.src.shape, dtype=torch.bfloat16, device=self.src.device),)

    def _fill(self, bufs):
        self.fills += 1
        if bufs[0].device.type != "meta":
            bufs[0].copy_(self.src.detach())

    def get(self, sources=None):
        return W.derived(self.owner, "_slot", sources or (self.src,), self._alloc,
                         self._fill, extra=self.extra)


@pytest.fixture(autouse=True)
def _restore_globals():
    epoch, refresh = W._weights_epoch[0], W.CAPTURE_REFRESH[0]
    yield
    W._weights_epoch[0], W.CAPTURE_REFRESH[0] = epoch, refresh


def test_transformer_reexports_the_same_objects():
    assert tops.CAPTURE_REFRESH is W.CAPTURE_REFRESH
    assert tops._weights_epoch is W._weights_epoch
    assert tops.bump_weights_epoch is W.bump_weights_epoch
    assert tops._shadow_w16 is W._shadow_w16 and tops._bias_f32 is W._bias_f32


def test_derived_hit_returns_same_container_without_fill():
    c = _Cache(torch.nn.Parameter(torch.randn(4, 4)))
    bufs = c.get()
    assert (c.allocs, c.fills) == (1, 1)
    assert torch.equal(bufs[0], c.src.detach().to(torch.bfloat16))
    assert c.get() is bufs and c.get() is bufs
    assert (c.allocs, c.fills) == (1, 1)


def test_derived_source_write_refills_same_storage():
    c = _Cache(torch.nn.Parameter(torch.randn(4, 4)))
    bufs = c.get()
    ptr = bufs[0].data_ptr()
    with torch.no_grad():
        c.src.copy_(torch.randn(4, 4))
    again = c.get()
    assert again is bufs and again[0].data_ptr() == ptr
    assert (c.allocs, c.fills) == (1, 2)
    assert torch.equal(again[0], c.src.detach().to(torch.bfloat16))
    c.get()
    assert c.fills == 2


def test_derived_epoch_bump_refills_same_storage():
    c = _Cache(torch.nn.Parameter(torch.randn(4, 4)))
    bufs = c.get()
    ptr = bufs[0].data_ptr()
    # a raw-kernel write (FlatAdamW): no version bump, only the epoch moves
    c.src.data.add_(1.0)
    ver = c.src._version
    W.bump_weights_epoch()
    assert c.src._version == ver
    again = c.get()
    assert again is bufs and again[0].data_ptr() == ptr
    assert (c.allocs, c.fills) == (1, 2)
    assert torch.equal(again[0], c.src.detach().to(torch.bfloat16))


def test_derived_capture_refresh_refills_every_call_never_reallocates():
    c = _Cache(torch.nn.Parameter(torch.randn(4, 4)))
    bufs = c.get()
    ptr = bufs[0].data_ptr()
    tops.CAPTURE_REFRESH[0] = True  # written through the re-export, as callers do
    for n in range(3):
        assert c.get() is bufs and bufs[0].data_ptr() == ptr
        assert (c.allocs, c.fills) == (1, 2 + n)
    tops.CAPTURE_REFRESH[0] = False
    c.get()
    assert (c.allocs, c.fills) == (1, 4)


def test_derived_extra_change_reallocates():
    c = _Cache(torch.nn.Parameter(torch.randn(4, 4)), extra=(True,))
    bufs = c.get()
    c.extra = (False,)
    other = c.get()
    assert other is not bufs and (c.allocs, c.fills) == (2, 2)
    assert c.get() is other and (c.allocs, c.fills) == (2, 2)


def test_derived_device_change_reallocates():
    c = _Cache(torch.nn.Parameter(torch.randn(4, 4)))
    bufs = c.get()
    c.src = torch.nn.Parameter(torch.empty(4, 4, device="meta"))
    moved = c.get()
    assert moved is not bufs and moved[0].device.type == "meta"
    assert (c.allocs, c.fills) == (2, 2)
    assert c.get() is moved and (c.allocs, c.fills) == (2, 2)


def test_derived_none_sources_are_ignored():
    c = _Cache(torch.nn.Parameter(torch.randn(4, 4)))
    bias = torch.nn.Parameter(torch.randn(4))
    bufs = c.get((c.src, None, bias, None))
    assert c.get((c.src, None, bias, None)) is bufs and c.fills == 1
    with torch.no_grad():
        bias.zero_()  # the non-None entries do key the cache
    assert c.get((c.src, None, bias, None)) is bufs and c.fills == 2


# -- direct grads ------------------------------------------------------------


def _flat_params(shapes, gap_before=None):
    """Parameters laid out the way FlatAdamW lays them out on the GPU: bf16
    shadows and fp32 grads are consecutive views of two flat buffers.
    `gap_before=i` leaves one unused element before parameter i."""
    ps = [torch.nn.Parameter(torch.randn(*s)) for s in shapes]
    total = sum(p.numel() for p in ps) + (1 if gap_before is not None else 0)
    base16 = torch.zeros(total, dtype=torch.bfloat16)
    gbase = torch.zeros(total, dtype=torch.float32)
    off = 0
    for i, p in enumerate(ps):
        if i == gap_before:
            off += 1
        n = p.numel()
        p._dfa_w16 = base16[off:off + n].view(p.shape)
        p._dfa_w16.copy_(p.detach())
        p._dfa_w16_ver = p._version
        p._dfa_w16_base, p._dfa_w16_off = base16, off
        p._dfa_gbase, p._dfa_goff = gbase, off
        p.grad = gbase[off:off + n].view(p.shape)
        off += n
    return ps, base16, gbase


def test_direct_grads_truth_table():
    (good, good2), _, _ = _flat_params([(4, 4), (4,)])
    assert W.direct_grads(good) and W.direct_grads(good, good2)
    no_shadow = torch.nn.Parameter(torch.randn(4))
    no_shadow.grad = torch.zeros(4)
    assert not W.direct_grads(no_shadow)
    (no_grad,), _, _ = _flat_params([(4,)])
    no_grad.grad = None
    assert not W.direct_grads(no_grad)
    assert not W.direct_grads(None)
    for bad in (no_shadow, no_grad, None):
        assert not W.direct_grads(good, bad) and not W.direct_grads(bad, good2)


def test_packed_views_span_adjacent_params():
    ps, base16, gbase = _flat_params([(8, 4), (8, 4), (8, 4)])
    s, g = W.packed_shadow(ps), W.packed_grad(ps)
    assert s.numel() == g.numel() == 96
    assert s.dtype == torch.bfloat16 and g.dtype == torch.float32
    assert s.data_ptr() == base16.data_ptr() and g.data_ptr() == gbase.data_ptr()
    assert torch.equal(s.view(24, 4), torch.cat([p.detach() for p in ps]).to(torch.bfloat16))
    g.fill_(1.0)  # aliases every .grad
    assert all(float(p.grad.sum()) == p.numel() for p in ps)
    # a sub-run that does not start at offset 0
    s2, g2 = W.packed_shadow(ps[1:]), W.packed_grad(ps[1:])
    assert s2.numel() == g2.numel() == 64
    assert s2.data_ptr() == ps[1]._dfa_w16.data_ptr()
    assert g2.data_ptr() == ps[1].grad.data_ptr()


def test_packed_views_none_on_gap():
    ps, _, _ = _flat_params([(8, 4), (8, 4), (8, 4)], gap_before=2)
    assert W.packed_shadow(ps) is None and W.packed_grad(ps) is None
    assert W.packed_shadow(ps[:2]) is not None and W.packed_grad(ps[:2]) is not None


def test_packed_views_none_on_different_base():
    ps, _, _ = _flat_params([(8, 4), (8, 4)])
    (other,), _, _ = _flat_params([(8, 4)])
    other._dfa_w16_off = other._dfa_goff = 64  # right offset, wrong buffer
    assert W.packed_shadow(ps + [other]) is None
    assert W.packed_grad(ps + [other]) is None


def test_packed_views_none_on_missing_shadow():
    ps, _, _ = _flat_params([(8, 4), (8, 4), (8, 4)])
    bare = torch.nn.Parameter(torch.randn(8, 4))
    assert W.packed_shadow([ps[0], bare, ps[2]]) is None
    assert W.packed_grad([ps[0], bare, ps[2]]) is None
    assert W.packed_shadow([bare, ps[1]]) is None and W.packed_grad([bare, ps[1]]) is None


def test_packed_grad_none_on_replaced_or_dropped_grad():
    ps, _, _ = _flat_params([(8, 4), (8, 4), (8, 4)])
    assert W.packed_grad(ps) is not None
    ps[1].grad = torch.zeros(8, 4)  # e.g. zero_grad(set_to_none) + a fresh backward
    assert W.packed_grad(ps) is None
    assert W.packed_shadow(ps) is not None  # the weights view is unaffected
    ps, _, _ = _flat_params([(8, 4), (8, 4)])
    ps[0].grad = None
    assert W.packed_grad(ps) is None


def test_packed_shadow_resyncs_after_torch_level_write():
    ps, base16, _ = _flat_params([(8, 4), (8, 4), (8, 4)])
    with torch.no_grad():
        ps[1].copy_(torch.randn(8, 4))  # checkpoint load: version bump
    s = W.packed_shadow(ps)
    assert s.data_ptr() == base16.data_ptr()
    assert torch.equal(s.view(24, 4), torch.cat([p.detach() for p in ps]).to(torch.bfloat16))
    assert ps[1]._dfa_w16_ver == ps[1]._version
