"""Times T5 generate() with the two KV-cache modes at the reference's
`summarize` evaluation shape: CodeT5-base, batch 32, source 256, max_length
128, beam 10, EOS suppressed so that all 127 steps run.

  python tools/decode_probe.py                       # concat vs indirect, alternating
  python tools/decode_probe.py --modes indirect --repeats 1 --warmup 0   # under a profiler
  python tools/decode_probe.py --modes indirect+logits,indirect+fused   # the two select modes

Both modes run in ONE process, alternating, after a warm-up of each, with a
device synchronise around every timed region; the result is the per-mode
median, minimum and maximum over the repeats, the peak allocated memory of a
generate call, and (--launches) the kernel launches per generated token from
the difference of two short profiled runs. One JSON line at the end.
"""

import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from deepdfa_amd.models.t5 import T5Config, T5ForConditionalGeneration  # noqa: E402


def split_mode(mode, args):
    """"indirect" or "indirect+fused": (kv_cache, select); --select is the default."""
    kv, _, sel = mode.partition("+")
    return kv, sel or args.select


def timed(model, ids, mode, args):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.perf_counter()
    kv, sel = split_mode(mode, args)
    out = model.generate(ids, max_length=args.max_length, num_beams=args.beams, kv_cache=kv,
                         select=sel)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    assert out.shape[1] == args.max_length, "generation stopped early"
    return dt, torch.cuda.max_memory_allocated(), out


def count_kernels(model, ids, mode, beams, max_length, args):
    from torch.profiler import ProfilerActivity, profile

    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        kv, sel = split_mode(mode, args)
        model.generate(ids, max_length=max_length, num_beams=beams, kv_cache=kv, select=sel)
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA
               and "memcpy" not in e.name.lower() and "memset" not in e.name.lower())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--source", type=int, default=256)
    ap.add_argument("--max-length", type=int, default=128)
    ap.add_argument("--beams", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--modes", default="concat,indirect",
                    help="comma-separated kv_cache modes; KV+SELECT (indirect+fused) "
                         "pins generate(select=...) for that entry")
    ap.add_argument("--select", default="logits", choices=["logits", "fused"],
                    help="generate(select=...) of the entries that do not pin one")
    ap.add_argument("--launches", action="store_true")
    args = ap.parse_args()
    modes = args.modes.split(",")

    torch.manual_seed(0)
    cfg = T5Config(eos_token_id=-1)             # CodeT5-base geometry; EOS never matches
    model = T5ForConditionalGeneration(cfg).cuda().eval()
    g = torch.Generator().manual_seed(1)
    ids = torch.randint(3, cfg.vocab_size, (args.batch, args.source), generator=g)
    for b in range(args.batch):                 # ragged sources, as in the dataset
        ids[b, args.source - (b * 5) % 97:] = cfg.pad_token_id
    ids[:, 0] = 5
    ids = ids.cuda()

    for _ in range(args.warmup):
        for mode in modes:
            timed(model, ids, mode, args)
    times = {m: [] for m in modes}
    peak = {m: 0 for m in modes}
    outs = {}
    for rep in range(args.repeats):
        for mode in modes:
            dt, mem, outs[mode] = timed(model, ids, mode, args)
            times[mode].append(dt)
            peak[mode] = max(peak[mode], mem)
            print(f"rep {rep} {mode:15s} {dt * 1e3:9.1f} ms  peak {mem / 2**30:6.2f} GiB", flush=True)
    result = {"shape": vars(args)}
    steps = args.max_length - 1
    for mode in modes:
        ts = times[mode]
        result[mode] = {
            "median_ms": statistics.median(ts) * 1e3, "min_ms": min(ts) * 1e3,
            "max_ms": max(ts) * 1e3, "ms_per_token": statistics.median(ts) * 1e3 / steps,
            "peak_GiB": peak[mode] / 2**30,
        }
    if len(modes) == 2:
        a, b = (outs[m] for m in modes)
        result["tokens_equal_fraction"] = float((a == b).float().mean())
    if args.launches:
        for mode in modes:
            try:
                n9 = count_kernels(model, ids, mode, args.beams, 9, args)
                n5 = count_kernels(model, ids, mode, args.beams, 5, args)
                result[mode]["launches_per_token"] = (n9 - n5) / 4
            except Exception as e:  # the profiler is optional equipment
                result[mode]["launches_per_token"] = f"unavailable: {type(e).__name__}"
    print(json.dumps(result))


if __name__ == "__main__":
    main()
