"""Same-build A/B of the GGNN weight grads on the training shape (S = 5,
N = 11 567, H = 128): the one-launch kernel (ext.ggnn_wgrad) against the
wgrad_kernel + wgrad2_kernel pair it replaced (two_launches=True), in the
direct form, plus the sweep of the new kernel's launcher parameters: K rows
per chunk and the epilogue (atomics straight from the MFMA layout, or staged
through LDS into 256-B row segments).

Device events around `--iters` back-to-back calls, `--rounds` alternating
rounds over all variants, median per variant. Back-to-back calls re-read the
same 104 MB of operands, which fit the Infinity Cache; the training step
reads them right after the loop wrote them, so the step's own figure comes
from the kernel trace of bench.py, and this probe ranks the variants.

  python tools/ggnn_wgrad_probe.py [--rounds 7] [--iters 20]
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from deepdfa_amd.ops import load_ext

ap = argparse.ArgumentParser()
ap.add_argument("--S", type=int, default=5)
ap.add_argument("--N", type=int, default=11567)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--chunks", type=int, nargs="*",
                default=[512, 832, 960, 1024, 1088, 1216, 1664, 1856, 2048, 3328])
args = ap.parse_args()

ext = load_ext(required=True)
dev = "cuda"
torch.manual_seed(0)
S, N, H = args.S, args.N, 128
Gg = (torch.randn(S, N, 4 * H, device=dev) / 16).to(torch.bfloat16)
Gwh = (torch.randn(S, N, H, device=dev) / 16).to(torch.bfloat16)
M = torch.randn(S, N, H, device=dev).to(torch.bfloat16)
HH = torch.randn(S + 1, N, H, device=dev).to(torch.bfloat16)
f32 = dict(device=dev, dtype=torch.float32)
outs = dict(out_we=torch.zeros(H, H, **f32), out_be=torch.zeros(H, **f32),
            gru_outs=[torch.zeros(3 * H, H, **f32), torch.zeros(3 * H, H, **f32),
                      torch.zeros(3 * H, **f32), torch.zeros(3 * H, **f32)])

variants = {"old pair": dict(two_launches=True)}
for c in args.chunks:
    z = -(-S * N // c)
    variants[f"new kchunk={c} (z={z}, {7 * z} blocks) lds-epi"] = dict(kchunk=c, lds_epi=1)
    variants[f"new kchunk={c} (z={z}, {7 * z} blocks) direct-epi"] = dict(kchunk=c, lds_epi=0)
variants["new defaults"] = dict()


def batch(kw):
    s, e = torch.cuda.Event(True), torch.cuda.Event(True)
    ext.ggnn_wgrad(Gg, M, HH, Gwh, S, **outs, **kw)
    torch.cuda.synchronize()
    s.record()
    for _ in range(args.iters):
        ext.ggnn_wgrad(Gg, M, HH, Gwh, S, **outs, **kw)
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / args.iters * 1000  # us


# agreement of the two paths before timing anything
a = ext.ggnn_wgrad(Gg, M, HH, Gwh, S)
b = ext.ggnn_wgrad(Gg, M, HH, Gwh, S, two_launches=True)
for name, x, y in zip(("gW_ih", "gW_hh", "gb_ih", "gb_hh", "gW_e", "gb_e"), a, b):
    print(f"agree {name}: max|new-old| {float((x - y).abs().max()):.3e} "
          f"max|old| {float(y.abs().max()):.3e}")

times = {k: [] for k in variants}
for r in range(args.rounds):
    for k, kw in variants.items():
        times[k].append(batch(kw))
print(f"S={S} N={N} K={S * N}  default kchunk={ext.ggnn_wgrad_kchunk(S * N)}  "
      f"rounds={args.rounds} iters={args.iters}  (us per call: median, min, max)")
for k, v in times.items():
    print(f"{k:50s} {statistics.median(v):8.2f} {min(v):8.2f} {max(v):8.2f}")
