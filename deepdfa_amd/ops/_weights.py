"""The two protocols every fused op shares with the optimizer and with
hipGraph capture (docs/ARCHITECTURE.md, "Weight caches and direct grads"):
the derived-weight cache `derived`, and direct gradient accumulation into
FlatAdamW's flat `.grad` views — `direct_grads`, `packed_shadow`,
`packed_grad`. Device-agnostic; tests/test_weight_cache.py.
"""

from __future__ import annotations

import torch

# cast-cache invalidation epoch: optimizers that write master weights
# through raw extension kernels (FlatAdamW) bypass torch's version
# counters, so they bump this instead
_weights_epoch = [0]

# hipGraph capture mode: when True, every derived buffer is re-filled on
# every call so the refresh is captured and replays against the updated
# master weights
CAPTURE_REFRESH = [False]


def bump_weights_epoch():
    _weights_epoch[0] += 1


def _shadow_w16(weight):
    """The optimizer-maintained flat bf16 shadow view of `weight`
    (parallel/optim.py FlatAdamW), re-synced if a torch-level write
    (checkpoint load, broadcast) moved the parameter's version counter
    since the last sync. None when no flat optimizer owns the weight."""
    w16 = getattr(weight, "_dfa_w16", None)
    if w16 is None:
        return None
    if weight._version != weight._dfa_w16_ver:
        w16.copy_(weight.detach())
        weight._dfa_w16_ver = weight._version
    return w16


def _bias_f32(bias):
    """Master-fp32 biases are used in place (no copy); anything else is
    cast-copied (rare: only models trained without the flat optimizer)."""
    if bias is None:
        return None
    b = bias.detach()
    if b.dtype == torch.float32 and b.is_contiguous():
        return b
    return b.float().contiguous()


def derived(owner, slot, sources, alloc, fill, extra=()):
    """Buffers derived from `sources`, cached on `owner` under attribute
    `slot`. The key is the sources' `_version`s (None entries skipped), the
    weights epoch and `extra`. `alloc()` builds the buffer container: only
    when nothing is cached, or the sources moved device, or `extra` changed.
    `fill(bufs)` writes INTO the buffers: after `alloc`, and whenever the
    key moved or CAPTURE_REFRESH is set. Otherwise the cached container is
    returned and nothing is launched."""
    srcs, extra = [s for s in sources if s is not None], tuple(extra)
    key = tuple(s._version for s in srcs) + (_weights_epoch[0],) + extra
    device = srcs[0].device
    cache = getattr(owner, slot, None)
    if cache is not None and (cache[1] != device or cache[2] != extra):
        cache = None
    if cache is None:
        bufs = alloc()
    elif CAPTURE_REFRESH[0] or cache[0] != key:
        bufs = cache[3]
    else:
        return cache[3]
    fill(bufs)
    setattr(owner, slot, (key, device, extra, bufs))
    return bufs


def direct_grads(*params) -> bool:
    """True when every param's grad can be accumulated in-kernel: the flat
    optimizer owns it (it has a shadow) and its `.grad` view is live."""
    return all(p is not None and getattr(p, "_dfa_w16", None) is not None
               and p.grad is not None for p in params)


def _packed(ws, base_attr, off_attr):
    """base[off:end] over params whose flat views share `base` back-to-back."""
    base = getattr(ws[0], base_attr, None)
    if base is None:
        return None
    off = end = getattr(ws[0], off_attr)
    for w in ws:
        if getattr(w, base_attr, None) is not base or getattr(w, off_attr) != end:
            return None
        end += w.numel()
    return base[off:end]


def packed_shadow(ws):
    """The zero-copy flat bf16 view spanning `ws` when their shadows sit
    back-to-back in one flat buffer, else None. Each shadow is synced first
    (_shadow_w16) so a torch-level write is reflected in the view."""
    for w in ws:
        _shadow_w16(w)
    return _packed(ws, "_dfa_w16_base", "_dfa_w16_off")


def packed_grad(ws):
    """The same over the flat fp32 grad buffer; additionally every `.grad`
    must be live and still start at its flat offset, so a replaced `.grad`
    disables the path."""
    flat = _packed(ws, "_dfa_gbase", "_dfa_goff")
    if flat is None or any(
        w.grad is None
        or w.grad.data_ptr() != flat.data_ptr() + flat.element_size() * (w._dfa_goff - ws[0]._dfa_goff)
        for w in ws
    ):
        return None
    return flat
