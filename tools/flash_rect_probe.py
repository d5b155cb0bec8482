"""Times the general flash attention (csrc/flash_rect.hip) against the
materialised composition it replaces, forward + backward, at the shapes the
models route to it: B = 32, H = 12, d = 64, p = 0.1.

  cross 128x256        cross-attention, fused K|V buffer, valid lengths
  cross 32x128         the generation drivers' default lengths
  self 150 causal+bias decoder self-attention off the 64 grid (shared dBias buffer)
  self 400 valid       encoder self-attention at the clone task's length

  python tools/flash_rect_probe.py                  # the four shapes
  python tools/flash_rect_probe.py --model          # + a CodeT5-base training step, 128 -> 32

The materialised side is what the models run without the kernels: the head
split transposes, matmul, the bias add, masked_softmax_dropout, matmul and
the transpose back, with autograd's backward (at a key length that is no
multiple of 8 the softmax kernel raises, as the models did: eager torch
softmax + dropout stands in, and the result says so). Both sides run in ONE process,
alternating, after a warm-up of each; every timed region is a forward +
backward between two device events. The result is the median over the timed
iterations, with minimum and maximum, and the ratio materialised / fused.
--model times a whole training step (bf16 autocast, forward + backward) of a
T5 with the general kernels routed and with the routing switched off, which
is the materialised path again. One JSON line at the end.
"""

import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from deepdfa_amd.ops.transformer import (flash_attention_rect, flash_attention_rect_kv,  # noqa: E402
                                         masked_softmax_dropout)

bf = torch.bfloat16
DEV = "cuda:0"


def materialised(q, k, v, H, valid, bias, scale, causal, p):
    """q (B, Lq, D), k, v (B, Lk, D), bias (1, H, Lq, Lk) fp32 or None."""
    B, Lq, D = q.shape
    Lk = k.shape[1]
    d = D // H
    qh = q.view(B, Lq, H, d).transpose(1, 2)
    kh = k.view(B, Lk, H, d).transpose(1, 2)
    vh = v.view(B, Lk, H, d).transpose(1, 2)
    scores = torch.matmul(qh, kh.transpose(-1, -2))
    if bias is not None:
        scores = scores + bias.to(scores.dtype)
    if Lk % 8 == 0:
        _, pd = masked_softmax_dropout(scores, valid, scale, p, causal=causal)
    else:
        # the softmax kernel takes whole 16-B vectors only (bf16: Lk % 8 == 0);
        # the models raised at such a length, so time eager torch instead
        s = scores.float() * scale
        key = torch.arange(Lk, device=q.device)
        if valid is not None:
            s = s.masked_fill(key.view(1, 1, 1, Lk) >= valid.view(-1, 1, 1, 1), float("-inf"))
        if causal:
            s = s.masked_fill(key.view(1, Lk) > torch.arange(Lq, device=q.device).view(Lq, 1),
                              float("-inf"))
        pd = torch.nn.functional.dropout(torch.softmax(s, -1).to(q.dtype), p)
    return torch.matmul(pd, vh).transpose(1, 2).reshape(B, Lq, D)


def make_case(name, B, H, Lq, Lk, kind, p):
    g = torch.Generator().manual_seed(Lq * 1000 + Lk)
    D = H * 64
    mk = lambda L, w=D: (torch.randn(B, L, w, generator=g) * 0.5).to(bf).to(DEV).requires_grad_()  # noqa: E731
    q, dO = mk(Lq), torch.randn(B, Lq, D, generator=g).to(bf).to(DEV)
    valid = (torch.randint(Lk // 2, Lk + 1, (B,), generator=g)).to(torch.int32).to(DEV)
    if kind == "cross":
        kv = mk(Lk, 2 * D)

        def fused():
            return flash_attention_rect_kv(q, kv, H, valid=valid, scale=1.0, dropout_p=p), (q, kv)

        def mat():
            return materialised(q, kv[..., :D], kv[..., D:], H, valid, None, 1.0, False, p), (q, kv)
        return fused, mat, dO
    k, v = mk(Lk), mk(Lk)
    if kind == "causal+bias":
        bias = torch.randn(1, H, Lq, Lk, generator=g).to(DEV).requires_grad_()
        accum = torch.zeros(H, Lk, Lq, device=DEV)

        def fused():
            # as T5Stack does: one transposed copy and one shared dBias buffer per step
            bT = bias.detach().squeeze(0).transpose(-1, -2).contiguous()
            return flash_attention_rect(q, k, v, H, bias=bT, scale=1.0, causal=True,
                                        dropout_p=p, bias_accum=accum), (q, k, v)

        def mat():
            return materialised(q, k, v, H, None, bias, 1.0, True, p), (q, k, v, bias)
        return fused, mat, dO
    scale = 0.125

    def fused():
        return flash_attention_rect(q, k, v, H, valid=valid, scale=scale, dropout_p=p), (q, k, v)

    def mat():
        return materialised(q, k, v, H, valid, None, scale, False, p), (q, k, v)
    return fused, mat, dO


def step(fn, dO):
    out, leaves = fn()
    out.backward(dO)
    for t in leaves:
        t.grad = None


def time_pair(fns, dO_or_none, warmup, iters):
    """Alternating event-timed runs of the callables in `fns` (name -> fn)."""
    run = (lambda f: step(f, dO_or_none)) if dO_or_none is not None else (lambda f: f())
    for _ in range(warmup):
        for f in fns.values():
            run(f)
    torch.cuda.synchronize()
    ms = {n: [] for n in fns}
    for _ in range(iters):
        for n, f in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run(f)
            e1.record()
            e1.synchronize()
            ms[n].append(e0.elapsed_time(e1))
    return {n: dict(median_ms=statistics.median(t), min_ms=min(t), max_ms=max(t))
            for n, t in ms.items()}


def model_step(args):
    import deepdfa_amd.models.t5 as t5

    torch.manual_seed(0)
    cfg = t5.T5Config()                      # CodeT5-base geometry
    model = t5.T5ForConditionalGeneration(cfg).to(DEV).train()
    g = torch.Generator().manual_seed(1)
    src = torch.randint(3, cfg.vocab_size, (args.batch, args.source), generator=g)
    for b in range(args.batch):              # ragged sources, as in the dataset
        src[b, args.source - (b * 5) % (args.source // 2):] = cfg.pad_token_id
    src = src.to(DEV)
    tgt = torch.randint(3, cfg.vocab_size, (args.batch, args.target), generator=g).to(DEV)
    usable = t5.flash_rect_usable

    def run():
        with torch.autocast(device_type="cuda", dtype=bf):
            loss = model(src, labels=tgt)[0]
        loss.backward()
        model.zero_grad(set_to_none=True)

    def routed():
        t5.flash_rect_usable = usable
        run()

    def unrouted():
        t5.flash_rect_usable = lambda x, d: False
        try:
            run()
        finally:
            t5.flash_rect_usable = usable

    return time_pair({"fused": routed, "materialised": unrouted}, None, args.model_warmup,
                     args.model_iters)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--heads", type=int, default=12)
    ap.add_argument("--p", type=float, default=0.1)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--model", action="store_true")
    ap.add_argument("--source", type=int, default=128)
    ap.add_argument("--target", type=int, default=32)
    ap.add_argument("--model-warmup", type=int, default=5)
    ap.add_argument("--model-iters", type=int, default=20)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "the probe measures on the GPU"
    assert args.iters >= 50, "at least 50 timed iterations"

    shapes = [("cross 128x256", 128, 256, "cross"), ("cross 32x128", 32, 128, "cross"),
              ("self 150 causal+bias", 150, 150, "causal+bias"), ("self 400 valid", 400, 400, "valid")]
    result = {"B": args.batch, "H": args.heads, "p": args.p, "iters": args.iters, "shapes": {}}
    for name, Lq, Lk, kind in shapes:
        fused, mat, dO = make_case(name, args.batch, args.heads, Lq, Lk, kind, args.p)
        r = time_pair({"fused": fused, "materialised": mat}, dO, args.warmup, args.iters)
        r["ratio"] = r["materialised"]["median_ms"] / r["fused"]["median_ms"]
        r["baseline"] = "masked_softmax_dropout" if Lk % 8 == 0 else "eager torch softmax"
        result["shapes"][name] = r
        print(f"{name:22s} fused {r['fused']['median_ms']:7.3f} ms "
              f"[{r['fused']['min_ms']:.3f}, {r['fused']['max_ms']:.3f}]  materialised "
              f"{r['materialised']['median_ms']:7.3f} ms [{r['materialised']['min_ms']:.3f}, "
              f"{r['materialised']['max_ms']:.3f}]  x{r['ratio']:.2f}", flush=True)
    if args.model:
        r = model_step(args)
        r["ratio"] = r["materialised"]["median_ms"] / r["fused"]["median_ms"]
        result["t5_step"] = dict(r, batch=args.batch, source=args.source, target=args.target)
        print(f"T5-base step {args.source}->{args.target} fused {r['fused']['median_ms']:.2f} ms "
              f"materialised {r['materialised']['median_ms']:.2f} ms x{r['ratio']:.2f}", flush=True)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
