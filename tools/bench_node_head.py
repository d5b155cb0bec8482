"""Time the node-level head, forward + backward, at N = 12288 nodes (the
node-count class of the headline 256-graph batch) on two paths:

  (a) ops.flowgnn.node_head — the fused MFMA kernels (csrc/node_head.hip)
      plus the wgrad/colsum launches of its backward;
  (b) the eager tail it replaces: torch.cat + output_layer under bf16
      autocast (three library GEMMs each way plus ReLU/bias glue).

Both paths get the same seeded inputs and fp32 master weights, are warmed
up, and are timed alternately with device events over several rounds so
that drift on a shared host hits both; the per-path figure is the median
round. The outputs of the two paths are compared first. Prints one JSON
line.

  python tools/bench_node_head.py [--n 12288] [--iters 200] [--rounds 5]
"""

import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402
from torch import nn  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=12288)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_node_head needs a GPU: nothing is measured on the CPU")

    from deepdfa_amd.ops import load_ext
    from deepdfa_amd.ops.flowgnn import node_head

    ext = load_ext(required=True)
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    N = args.n
    head = nn.Sequential(nn.Linear(256, 256), nn.ReLU(), nn.Linear(256, 256),
                         nn.ReLU(), nn.Linear(256, 1)).to(dev)
    h = (0.5 * torch.randn(N, 128, device=dev)).to(torch.bfloat16)
    fe = (0.5 * torch.randn(N, 128, device=dev)).to(torch.bfloat16)
    dl = torch.randn(N, device=dev) / N

    def fused():
        a, b = h.detach().requires_grad_(), fe.detach().requires_grad_()
        out = node_head(a, b, head[0], head[2], head[4])
        out.backward(dl)
        return out, a.grad, b.grad

    def eager():
        a, b = h.detach().requires_grad_(), fe.detach().requires_grad_()
        with torch.autocast(device_type="cuda", dtype=torch.bfloat16):
            out = head(torch.cat([a, b], dim=-1)).squeeze(-1)
        out.backward(dl.to(out.dtype))
        return out, a.grad, b.grad

    def grads():
        g = [p.grad.detach().clone() for p in head.parameters()]
        for p in head.parameters():
            p.grad = None
        return g

    # same results first (bf16 compute on both sides)
    of = fused()
    gf = grads()
    oe = eager()
    ge = grads()
    diffs = {
        "logits": float((of[0].detach().float() - oe[0].detach().float()).abs().max()),
        "dh": float((of[1].float() - oe[1].float()).abs().max()),
        "param_grads": max(float((x - y).abs().max()) for x, y in zip(gf, ge)),
    }

    def timed(fn):
        start = torch.cuda.Event(enable_timing=True)
        end = torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(args.iters):
            fn()
        end.record()
        torch.cuda.synchronize()
        for p in head.parameters():
            p.grad = None
        return start.elapsed_time(end) * 1e3 / args.iters  # us per fwd+bwd

    for fn in (fused, eager):
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    times = {"fused": [], "eager": []}
    for _ in range(args.rounds):
        times["fused"].append(timed(fused))
        times["eager"].append(timed(eager))
    med = {k: statistics.median(v) for k, v in times.items()}
    print(json.dumps({
        "n": N,
        "tile_rows": int(ext.node_head_tile_rows(N)),
        "iters": args.iters,
        "fused_us": round(med["fused"], 2),
        "eager_us": round(med["eager"], 2),
        "fused_over_eager": round(med["fused"] / med["eager"], 3),
        "fused_rounds_us": [round(t, 2) for t in times["fused"]],
        "eager_rounds_us": [round(t, 2) for t in times["eager"]],
        "max_abs_diff_fused_vs_eager": diffs,
    }))


if __name__ == "__main__":
    main()
