"""Timing of the attention-received path (docs/KERNELS.md, flash family).

  python tools/received_probe.py kernel   flash_received_kernel at B16 L512 H12
                                          (with and without valid) next to the
                                          whole flash backward, device events.
                                          Under `rocprofv3 --kernel-trace
                                          --stats -- python ... kernel none`
                                          (valid=None only) the per-kernel
                                          averages, flash_dkv_kernel among
                                          them, come from the trace.
  python tools/received_probe.py e2e      attention localization over 256
                                          synthetic functions at L = 512, 12
                                          layers: the per-example materialised
                                          loop (attention_line_scores) against
                                          attention_line_scores_batched at
                                          batch 32, layer -1 and layer 0; time
                                          and peak allocated memory of each.

Needs a GPU; prints one JSON line per measurement.
"""

import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from deepdfa_amd.ops import load_ext

DEV = "cuda:0"
bf = torch.bfloat16


def _events(fn, iters, rounds=5):
    """Median over `rounds` of the device-event time of `iters` calls, us per call."""
    out = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / iters)
    out.sort()
    return out[len(out) // 2], out[0], out[-1]


def kernel(only_none=False):
    ext = load_ext(required=True)
    torch.manual_seed(0)
    B, L, H = 16, 512, 12
    q, k, v, dO = (torch.randn(B, L, H * 64, device=DEV, dtype=bf) * 0.3 for _ in range(4))
    full = torch.full((B,), L, dtype=torch.int32, device=DEV)
    mixed = torch.randint(64, L + 1, (B,), generator=torch.Generator().manual_seed(1)).to(
        torch.int32).to(DEV)
    cases = (("valid=None", None), ("valid=L", full), ("valid~U[64,512]", mixed))
    for name, valid in cases[:1] if only_none else cases:
        O, lse = ext.flash_attn_fwd(q, k, v, H, valid, None, 0.125, False, 0.0, 0)
        recv = lambda: ext.flash_attn_received(q, k, lse, H, valid, None, 0.125, False)  # noqa: E731
        bwd = lambda: ext.flash_attn_bwd(dO, q, k, v, O, lse, H, valid, None, 0.125, False, 0.0,  # noqa: E731
                                         0, False, False)
        fwd = lambda: ext.flash_attn_fwd(q, k, v, H, valid, None, 0.125, False, 0.0, 0)  # noqa: E731
        for _ in range(20):
            recv(), bwd(), fwd()
        torch.cuda.synchronize()
        res = {"shape": f"B{B} L{L} H{H}", "valid": name}
        for tag, fn in (("received_us", recv), ("fwd_us", fwd), ("bwd_dterm_dq_dkv_us", bwd)):
            med, lo, hi = _events(fn, 200)
            res[tag] = round(med, 1)
            res[tag + "_min_max"] = [round(lo, 1), round(hi, 1)]
        print(json.dumps(res), flush=True)


def e2e(N=256, L=512, layers=12, dev=DEV):
    from deepdfa_amd.data.text_dataset import synthetic_func_source
    from deepdfa_amd.data.tokenization import HashTokenizer
    from deepdfa_amd.models.linevul import Model
    from deepdfa_amd.train import unixcoder_main as uxc

    torch.manual_seed(0)
    BS = 32
    cfg = uxc.unixcoder_config(layers)
    tok = HashTokenizer(vocab_size=cfg.vocab_size)
    model = Model(config=cfg).to(dev).eval()
    # one synthetic function is ~65 tokens: join eight so the 512-token block is used
    funcs = ["\n".join(synthetic_func_source(8 * i + j, vul=1) for j in range(8))
             for i in range(N)]
    enc = [uxc.encode_with_lines(tok, f, L) for f in funcs]
    ids_all = torch.tensor([e[0] for e in enc], dtype=torch.long, device=dev)
    lines_all = torch.tensor([e[1] for e in enc], dtype=torch.long, device=dev)
    n_tok = (ids_all != tok.pad_token_id).sum(1).float()
    print(json.dumps({"functions": N, "L": L, "mean_tokens": round(float(n_tok.mean()), 1),
                      "min_tokens": int(n_tok.min())}), flush=True)

    def per_example():
        out = []
        for i in range(N):
            out.append(uxc.attention_line_scores(model, ids_all[i], enc[i][1]))
        return out

    def batched(layer):
        out = []
        for c0 in range(0, N, BS):
            out.append(uxc.attention_line_scores_batched(
                model, ids_all[c0:c0 + BS], lines_all[c0:c0 + BS], layer).cpu())
        return out

    runs = (("per-example materialised loop (fp32, layer -1)", per_example),
            ("batched 32, --attention_layer -1", lambda: batched(-1)),
            ("batched 32, --attention_layer 0", lambda: batched(0)))
    for name, fn in runs:
        fn()                                  # warm-up: every shape of the timed window
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        times = []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
        times.sort()
        print(json.dumps({
            "path": name, "seconds_median": round(times[1], 4),
            "seconds_min_max": [round(times[0], 4), round(times[2], 4)],
            "peak_allocated_MiB": round(torch.cuda.max_memory_allocated() / 2 ** 20, 1),
            "resident_before_MiB": round(base / 2 ** 20, 1)}), flush=True)

    # same ranking input: batched bf16 scores against the fp32 per-example ones
    single = per_example()
    got = batched(-1)
    worst = 0.0
    for i in range(N):
        for ln, ref in single[i].items():
            worst = max(worst, abs(float(got[i // BS][i % BS, ln]) - ref) / max(abs(ref), 1e-30))
    print(json.dumps({"max_rel_diff_batched_bf16_vs_per_example_fp32": worst}), flush=True)


if __name__ == "__main__":
    assert torch.cuda.is_available(), "received_probe needs a GPU"
    mode = sys.argv[1] if len(sys.argv) > 1 else "kernel"
    if mode == "kernel":
        kernel(only_none=sys.argv[2:] == ["none"])
    else:
        e2e()
