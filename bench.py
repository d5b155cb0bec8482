#!/usr/bin/env python3
"""Flagship benchmark (driver contract: bench.py --gpus N --steps K --warmup W).

Models (BASELINE.json configs):
  --model ddfa          DeepDFA flow-GNN training, batch 256 graphs/GPU
                        (default; headline metric train_graphs_per_sec,
                        baseline ~810 graphs/s on RTX 3090)
  --model linevul       LineVul RoBERTa-base 512-token fine-tune, b=16/GPU
                        (train_examples_per_sec; baseline 40.6 ex/s = 150,908
                        fns x 10 epochs / 10h19m on RTX 3090)
  --model linevul_ddfa  combined LineVul+DeepDFA (baseline 39.3 ex/s, 10h40m)

bf16 compute + fp32 master Adam/AdamW, synthetic data (no-network env),
weak scaling (per-GPU batch fixed), RCCL DDP via deepdfa_amd.parallel.

A plain run only sets up, warms up, times --steps steps and prints one JSON
line. --dump-outputs DIR also writes loss, gradients and updated parameters
of the timed path, run on the last timed step's batch from the seeded start
state, as .npy; --full is where any secondary measurement belongs
(docs/BENCH.md).
"""

import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from deepdfa_amd.data import parse_limits  # noqa: E402
from deepdfa_amd.graph import synthetic_cfg_batch  # noqa: E402
from deepdfa_amd.models import FlowGNNGGNNModule  # noqa: E402
from deepdfa_amd.parallel.ddp import DDPEngine, init_distributed, world_size  # noqa: E402

FEAT = "_ABS_DATAFLOW_datatype_all_limitall_1000_limitsubkeys_1000"


def build_ddfa(args, rank, device, use_cuda):
    spec = parse_limits(FEAT)
    model = FlowGNNGGNNModule(
        feat=FEAT, input_dim=spec.input_dim, hidden_dim=32, n_steps=5, num_output_layers=3
    ).to(device)

    def opt_fn(capturable):
        # FlatAdamW is capture-safe (device-side step counter, bias
        # correction computed in the adamw kernel): ONE kernel per step vs
        # torch capturable Adam's ~8 multi_tensor + ~40 elementwise nodes
        from deepdfa_amd.parallel.optim import FlatAdamW

        return FlatAdamW(model.parameters(), lr=1e-3, weight_decay=1e-2, l2_mode=True)
    batches = [
        synthetic_cfg_batch(args.batch, seed=1000 * rank + i, input_dim=spec.input_dim).to(device)
        for i in range(args.n_batches)
    ]
    autocast = torch.autocast(device_type="cuda", dtype=torch.bfloat16) if use_cuda else None

    def make_step(opt, ddp, set_to_none):
        flat = hasattr(opt, "allreduce_grads")

        def fwd_bwd(i):
            g = batches[i % len(batches)]
            label = model.get_label(g)
            if autocast is not None:
                with autocast:
                    logits = model(g, {})
            else:
                logits = model(g, {})
            loss = model.loss_fn(logits.float(), label)
            opt.zero_grad(set_to_none=set_to_none and not flat)
            loss.backward()
            return loss

        def finish():
            if flat:
                opt.allreduce_grads()
            elif ddp is not None:
                ddp.finalize()
            opt.step()

        def step(i):
            loss = fwd_bwd(i)
            finish()
            return loss

        step.fwd_bwd = fwd_bwd
        step.finish = finish
        return step

    meta = dict(
        metric="train_graphs_per_sec",
        unit="graphs/s",
        baseline=810.0,
        per_step_items=args.batch,
        config={
            "model": "DeepDFA-FlowGNN-GGNN(n_steps=5,D=128)",
            "global_batch": args.batch * world_size(),
            "seq_len": None,
            "avg_nodes_per_graph": 45,
            "parallelism": f"dp{world_size()}",
        },
    )
    return model, opt_fn, make_step, meta, True  # graph-capture ok


def build_linevul(args, rank, device, use_cuda, with_ddfa: bool):
    from deepdfa_amd.models.linevul import Model
    from deepdfa_amd.models.roberta import RobertaConfig

    cfg = RobertaConfig()  # codebert-base geometry: 12 x 768, s=512
    fg = None
    if with_ddfa:
        spec = parse_limits(FEAT)
        fg = FlowGNNGGNNModule(
            feat=FEAT, input_dim=spec.input_dim, hidden_dim=32, n_steps=5,
            num_output_layers=3, encoder_mode=True,
        )
    model = Model(config=cfg, flowgnn_encoder=fg).to(device)
    from deepdfa_amd.parallel.optim import FlatAdamW

    opt_fn = lambda capturable: FlatAdamW(model.parameters(), lr=2e-5)  # noqa: E731
    b, s = args.batch, 512
    gen = torch.Generator().manual_seed(1234 + rank)
    batches = []
    for i in range(args.n_batches):
        ids = torch.randint(3, cfg.vocab_size, (b, s), generator=gen)
        lens = torch.randint(64, s + 1, (b,), generator=gen)
        for j in range(b):
            ids[j, lens[j] :] = 1
        ids[:, 0] = 0  # CLS
        labels = torch.randint(0, 2, (b,), generator=gen)
        item = [ids.to(device), labels.to(device)]
        if with_ddfa:
            item.append(synthetic_cfg_batch(b, seed=5000 * rank + i).to(device))
        batches.append(item)
    autocast = torch.autocast(device_type="cuda", dtype=torch.bfloat16) if use_cuda else None

    def make_step(opt, ddp, set_to_none):
        def fwd_bwd(i):
            item = batches[i % len(batches)]
            ids, labels = item[0], item[1]
            g = item[2] if with_ddfa else None
            if autocast is not None:
                with autocast:
                    loss, _prob = model(ids, labels=labels, graphs=g)
            else:
                loss, _prob = model(ids, labels=labels, graphs=g)
            opt.zero_grad(set_to_none=set_to_none)
            loss.backward()
            return loss

        def finish():
            opt.allreduce_grads()
            opt.clip_grad_norm_(1.0)
            opt.step()

        def step(i):
            loss = fwd_bwd(i)
            finish()
            return loss

        step.fwd_bwd = fwd_bwd
        step.finish = finish
        return step

    name = "LineVul+DeepDFA(CodeBERT-base+FlowGNN)" if with_ddfa else "LineVul(CodeBERT-base)"
    meta = dict(
        metric="train_examples_per_sec",
        unit="examples/s",
        baseline=39.3 if with_ddfa else 40.6,
        per_step_items=b,
        config={
            "model": name,
            "global_batch": b * world_size(),
            "seq_len": s,
            "parallelism": f"dp{world_size()}",
        },
    )
    # capture-safe: fixed shapes, FlatAdamW with device bias correction,
    # capture-refresh weight casts (see ops.transformer.CAPTURE_REFRESH)
    return model, opt_fn, make_step, meta, True


def build_codet5(args, rank, device, use_cuda, with_ddfa: bool):
    from deepdfa_amd.models.codet5 import DefectModel
    from deepdfa_amd.models.t5 import T5Config

    cfg = T5Config()  # codet5-base geometry: 12+12 x 768, vocab 32100
    fg = None
    if with_ddfa:
        spec = parse_limits(FEAT)
        fg = FlowGNNGGNNModule(
            feat=FEAT, input_dim=spec.input_dim, hidden_dim=32, n_steps=5,
            num_output_layers=3, encoder_mode=True,
        )
    model = DefectModel(config=cfg, flowgnn_encoder=fg).to(device)
    from deepdfa_amd.parallel.optim import FlatAdamW

    opt_fn = lambda capturable: FlatAdamW(model.parameters(), lr=2e-5)  # noqa: E731
    b, s = args.batch, 512
    gen = torch.Generator().manual_seed(77 + rank)
    batches = []
    for i in range(args.n_batches):
        ids = torch.randint(3, cfg.vocab_size, (b, s), generator=gen)
        lens = torch.randint(64, s + 1, (b,), generator=gen)
        for j in range(b):
            ids[j, lens[j] - 1] = 2  # EOS at last valid position
            ids[j, lens[j] :] = 0
        labels = torch.randint(0, 2, (b,), generator=gen)
        item = [ids.to(device), labels.to(device)]
        if with_ddfa:
            item.append(synthetic_cfg_batch(b, seed=9000 * rank + i).to(device))
        batches.append(item)
    autocast = torch.autocast(device_type="cuda", dtype=torch.bfloat16) if use_cuda else None

    def make_step(opt, ddp, set_to_none):
        def fwd_bwd(i):
            item = batches[i % len(batches)]
            ids, labels = item[0], item[1]
            g = item[2] if with_ddfa else None
            if autocast is not None:
                with autocast:
                    loss, _prob = model(ids, labels=labels, graphs=g)
            else:
                loss, _prob = model(ids, labels=labels, graphs=g)
            opt.zero_grad(set_to_none=set_to_none)
            loss.backward()
            return loss

        def finish():
            opt.allreduce_grads()
            opt.clip_grad_norm_(1.0)
            opt.step()

        def step(i):
            loss = fwd_bwd(i)
            finish()
            return loss

        step.fwd_bwd = fwd_bwd
        step.finish = finish
        return step

    name = "CodeT5+DeepDFA(codet5-base+FlowGNN)" if with_ddfa else "CodeT5(codet5-base)"
    meta = dict(
        metric="train_examples_per_sec",
        unit="examples/s",
        baseline=None,  # reference publishes no CodeT5 train time (paper Table 5)
        per_step_items=b,
        config={
            "model": name,
            "global_batch": b * world_size(),
            "seq_len": s,
            "parallelism": f"dp{world_size()}",
        },
    )
    return model, opt_fn, make_step, meta, False


DUMP_MAX_ELEMS = 4 * 1024 * 1024  # per array: 16 MB fp32, 3 arrays < 64 MB


def snapshot_state(model, opt):
    """Clone the seeded start state: master params, Adam moments, buffers."""
    return {
        "flat_p": opt.flat_p.detach().clone(),
        "m": opt.m.detach().clone(),
        "v": opt.v.detach().clone(),
        "buffers": [b.detach().clone() for b in model.buffers()],
    }


@torch.no_grad()
def rewind_state(model, opt, state):
    """Put the start state back IN PLACE: the captured graphs hold the
    addresses of these tensors (device step counter included), so nothing
    may be re-allocated."""
    opt.flat_p.copy_(state["flat_p"])
    opt.m.copy_(state["m"])
    opt.v.copy_(state["v"])
    opt.flat_g.zero_()
    if opt.flat_p16 is not None:
        opt.flat_p16.copy_(opt.flat_p)
    opt.step_count = 0
    if hasattr(opt, "_step_t"):
        opt._step_t.zero_()
    for b, b0 in zip(model.buffers(), state["buffers"]):
        b.copy_(b0)
    if opt.flat_p.is_cuda:
        from deepdfa_amd.ops.transformer import bump_weights_epoch

        bump_weights_epoch()  # eager path: drop the cached bf16 weight casts


def dump_outputs(out_dir, loss, model):
    """Write what the dump step produced — its loss, the gradients it left
    and the parameters after its optimizer update — as float32 .npy.
    Arrays over DUMP_MAX_ELEMS are reduced to a fixed seeded sample."""
    import numpy as np

    def flat(ts):
        return torch.cat([t.detach().float().flatten() for t in ts]).cpu()

    arrays = {
        "loss": loss.detach().float().reshape(1).cpu(),
        "params": flat(model.parameters()),
        "grads": flat(p.grad for p in model.parameters() if p.grad is not None),
    }
    os.makedirs(out_dir, exist_ok=True)
    for name, a in arrays.items():
        if a.numel() > DUMP_MAX_ELEMS:
            gen = torch.Generator().manual_seed(0)
            idx = torch.randint(0, a.numel(), (DUMP_MAX_ELEMS,), generator=gen)
            a = a[idx]
        np.save(os.path.join(out_dir, f"{name}.npy"), a.numpy().astype(np.float32))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=None)
    ap.add_argument("--warmup", type=int, default=None)
    ap.add_argument("--model", choices=["ddfa", "linevul", "linevul_ddfa", "codet5", "codet5_ddfa"], default="ddfa")
    ap.add_argument("--batch", type=int, default=None)
    ap.add_argument("--n-batches", type=int, default=4)
    ap.add_argument("--no-graph-capture", action="store_true")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, rewind to the seeded start state, "
                         "run the timed path on the last step's batch and write its "
                         "loss, gradients and updated parameters as DIR/<name>.npy")
    ap.add_argument("--full", action="store_true",
                    help="also run every secondary measurement; the benchmark "
                         "has none beyond the headline figure, so this adds nothing yet")
    args = ap.parse_args()
    if args.batch is None:
        args.batch = {"ddfa": 256, "linevul": 16, "linevul_ddfa": 16, "codet5": 8, "codet5_ddfa": 8}[args.model]
    # the ddfa step is ~1.3 ms — default to a seconds-scale timed region so
    # the measurement is robust (VERDICT round-1: >=200 steps)
    if args.steps is None:
        args.steps = 400 if args.model == "ddfa" else 50
    if args.warmup is None:
        args.warmup = 25 if args.model == "ddfa" else 10

    rank = init_distributed()
    ws = world_size()
    if rank == 0:
        print(f"[bench] world_size={ws} ranks visible "
              f"(backend={'nccl/RCCL' if torch.cuda.is_available() else 'gloo'})",
              file=sys.stderr)
    use_cuda = torch.cuda.is_available()
    device = (
        torch.device("cuda", int(os.environ.get("LOCAL_RANK", 0))) if use_cuda else torch.device("cpu")
    )
    if use_cuda:
        torch.cuda.set_device(device)
    torch.manual_seed(0)

    if args.model == "ddfa":
        model, opt_fn, make_step, meta, capture_ok = build_ddfa(args, rank, device, use_cuda)
    elif args.model.startswith("linevul"):
        model, opt_fn, make_step, meta, capture_ok = build_linevul(
            args, rank, device, use_cuda, with_ddfa=(args.model == "linevul_ddfa")
        )
    else:
        model, opt_fn, make_step, meta, capture_ok = build_codet5(
            args, rank, device, use_cuda, with_ddfa=(args.model == "codet5_ddfa")
        )

    use_graphs = use_cuda and capture_ok and not args.no_graph_capture
    opt = opt_fn(capturable=use_graphs)
    if args.model == "ddfa":
        if hasattr(opt, "flat_p"):
            ddp = None  # flat-buffer path: broadcast once, all-reduce flat
            if ws > 1:
                with torch.no_grad():
                    torch.distributed.broadcast(opt.flat_p, src=0)
        else:
            ddp = DDPEngine(model, bucket_cap_mb=64.0)
    else:
        ddp = None  # FlatAdamW: flat grads + one flat all-reduce; broadcast once
        if ws > 1:
            with torch.no_grad():
                torch.distributed.broadcast(opt.flat_p, src=0)
    step = make_step(opt, ddp, set_to_none=not use_graphs)
    start_state = snapshot_state(model, opt) if args.dump_outputs else None

    for i in range(args.warmup):
        step(i)

    if use_graphs:
        from deepdfa_amd.ops import transformer as _tops

        _tops.CAPTURE_REFRESH[0] = True  # weight casts re-run inside the graph
        torch.cuda.synchronize()
        pool = torch.cuda.graph_pool_handle()
        graphs = []
        losses = []  # static loss tensor of each captured step
        # multi-rank: capture the compute only (fwd+bwd); the RCCL
        # all-reduce + optimizer run eagerly between replays so no
        # collective sits inside a hipGraph (and N>1 keeps the captured
        # step rate instead of dropping to ~100 eager launches/step)
        capture_fn = step if ws == 1 else step.fwd_bwd
        finish_fn = None if ws == 1 else step.finish
        try:
            for i in range(args.n_batches):
                cg = torch.cuda.CUDAGraph()
                with torch.cuda.graph(cg, pool=pool):
                    losses.append(capture_fn(i))
                graphs.append(cg)
            torch.cuda.synchronize()

            def step(i):  # noqa: F811 — replay path
                graphs[i % len(graphs)].replay()
                if finish_fn is not None:
                    finish_fn()
                return losses[i % len(graphs)]
        except RuntimeError as e:  # capture unsupported: stay eager
            print(f"[bench] graph capture failed ({e}); running eager",
                  file=sys.stderr)
            torch.cuda.synchronize()

    def barrier_sync():
        if ws > 1:
            torch.distributed.barrier()
        if use_cuda:
            torch.cuda.synchronize()

    barrier_sync()
    t0 = time.perf_counter()
    for i in range(args.steps):
        step(i)
    barrier_sync()
    elapsed = time.perf_counter() - t0

    if args.dump_outputs and args.steps > 0:
        # The float atomics of the weight-gradient kernels make summation
        # order vary, and W+K training steps amplify that until two runs no
        # longer agree. So the dump is the timed path (same replayed graph
        # or step function, same batch as the last timed step) run once
        # more from the seeded start state: identical inputs every run,
        # outputs equal up to fp32 summation order.
        rewind_state(model, opt, start_state)
        dump_loss = step(args.steps - 1)
        barrier_sync()
        if rank == 0:
            dump_outputs(args.dump_outputs, dump_loss, model)

    print(f"[bench] rank {rank}: elapsed {elapsed:.4f}s over {args.steps} steps",
          file=sys.stderr)
    t = torch.tensor([elapsed], device=device if use_cuda else "cpu")
    if ws > 1:
        torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
    elapsed = float(t.item())

    value = meta["per_step_items"] * args.steps * ws / elapsed
    if rank == 0:
        print(
            json.dumps(
                {
                    "metric": meta["metric"],
                    "value": value,
                    "unit": meta["unit"],
                    "n_gpus": ws,
                    "steps": args.steps,
                    "warmup": args.warmup,
                    "ms_per_step": elapsed / args.steps * 1000.0,
                    "higher_is_better": True,
                    "scaling": "weak",
                    "vs_baseline": (value / meta["baseline"]) if meta["baseline"] else None,
                    "dtype": "bf16" if use_cuda else "fp32",
                    "data": "synthetic",
                    "config": meta["config"],
                }
            )
        )
    if ws > 1:
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
