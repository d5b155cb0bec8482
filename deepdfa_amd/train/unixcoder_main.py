"""UniXcoder-variant driver: line-level vulnerability localization.

Parity target: reference LineVul/unixcoder/linevul_main.py (1779 lines) —
the extended LineVul driver with the UniXcoder backbone plus:
  * line_level_localization (:955-1242): the full 5-method matrix —
    attention (heads summed; last layer by default, --attention_layer 0
    is the reference's first layer; batched on the fused kernels by
    attention_line_scores_batched), input-x-gradient saliency,
    integrated gradients (lig), DeepLift rescale, and GradientShap — all
    captum-free own implementations over the embedding layer;
  * Effort@TopK% and Recall@TopK%LOC metrics (:886-944);
  * eval_export (:742-829): per-example prediction dump CSV;
  * DbgBench evaluation hook (--dbgbench flag surface);
  * CodeT5-format dataset export (:1400-1423).

UniXcoder-base is RoBERTa-architecture (51416 vocab, 1026 positions) — the
backbone is our RobertaModel with that geometry.
"""

from __future__ import annotations

import argparse
import json
import logging
import os
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from ..data.text_dataset import TextDataset
from ..data.tokenization import HashTokenizer, tokenise
from ..models.linevul import Model
from ..models.roberta import RobertaConfig
from . import linevul_main

logger = logging.getLogger(__name__)


def unixcoder_config(num_layers: int = 12) -> RobertaConfig:
    return RobertaConfig(vocab_size=51416, max_position_embeddings=1026,
                         num_hidden_layers=num_layers)


# ---------------------------------------------------------------------------
# token -> line mapping + line scoring
# ---------------------------------------------------------------------------

def encode_with_lines(tokenizer, func: str, block_size: int = 512) -> Tuple[List[int], List[int]]:
    """Token ids + the source line index of each token (line -1 for
    CLS/SEP/PAD). Mirrors the reference's token->line bookkeeping used by
    line_level_localization."""
    ids = [tokenizer.cls_token_id]
    lines = [-1]
    for ln, line in enumerate(func.split("\n")):
        for tok in tokenise(line):
            if len(ids) >= block_size - 1:
                break
            ids.append(tokenizer._tok2id(tok))
            lines.append(ln)
    ids.append(tokenizer.sep_token_id)
    lines.append(-1)
    while len(ids) < block_size:
        ids.append(tokenizer.pad_token_id)
        lines.append(-1)
    return ids[:block_size], lines[:block_size]


@torch.no_grad()
def attention_line_scores(model: Model, ids: torch.Tensor, token_lines: List[int]) -> Dict[int, float]:
    """Attention-received per token (last layer, heads and queries summed),
    aggregated per source line (reference linevul_main.py:1117-1242
    'attention' method)."""
    model.eval()
    _prob, attentions = model(ids.unsqueeze(0), output_attentions=True)
    last = attentions[-1][0]  # (H, L, L)
    tok_score = last.sum(dim=(0, 1)).float().cpu()  # attention received per key token
    scores: Dict[int, float] = {}
    for j, ln in enumerate(token_lines):
        if ln >= 0:
            scores[ln] = scores.get(ln, 0.0) + float(tok_score[j])
    return scores


@torch.no_grad()
def attention_line_scores_batched(model: Model, ids: torch.Tensor, token_lines: torch.Tensor,
                                  layer: int = -1) -> torch.Tensor:
    """Batched 'attention' localization: (B, n_lines) fp32 line scores for
    `ids` (B, L) and `token_lines` (B, L; -1 for CLS/SEP/PAD as
    encode_with_lines produces), n_lines = token_lines.max() + 1.

    Runs the embeddings and encoder layers 0..`layer` only, asking for the
    attention each key token receives instead of the probabilities: on the
    GPU (bf16 autocast, as the test/eval loop) that is the fused QKV GEMM,
    flash attention and flash_received_kernel, with no (B, H, L, L) tensor.
    Heads are summed, then tokens are summed into their lines on the device.
    `layer` = -1 is the last layer, as attention_line_scores; the reference
    scores layer 0 (LineVul/unixcoder/linevul_main.py:1156)."""
    model.eval()
    n_layers = len(model.encoder.encoder.layer)
    if not -n_layers <= layer < n_layers:
        raise ValueError(f"attention layer {layer} out of range for {n_layers} layers")
    layer = layer % n_layers
    token_lines = token_lines.to(ids.device)
    with torch.autocast(device_type="cuda", dtype=torch.bfloat16, enabled=ids.is_cuda):
        _hidden, received = model.encoder(ids, attention_mask=ids.ne(1),
                                          attention_received=True, stop_after=layer)
    tok = received[layer].float().sum(dim=1)  # (B, L): heads summed
    n_lines = int(token_lines.max()) + 1 if token_lines.numel() else 0
    n_lines = max(n_lines, 0)
    # special/pad tokens (line -1) land in one extra column that is dropped
    out = torch.zeros(ids.shape[0], n_lines + 1, dtype=torch.float32, device=ids.device)
    index = torch.where(token_lines < 0, torch.full_like(token_lines, n_lines), token_lines)
    out.scatter_add_(1, index, tok)
    return out[:, :n_lines]


def saliency_line_scores(model: Model, ids: torch.Tensor, token_lines: List[int]) -> Dict[int, float]:
    """Input-x-gradient saliency per token -> line (the captum-free subset
    of the reference's lig/saliency/deeplift family)."""
    model.eval()
    emb_layer = model.encoder.embeddings.word_embeddings
    captured = {}

    def fwd_hook(mod, inp, out):
        out.retain_grad()
        captured["emb"] = out

    h = emb_layer.register_forward_hook(fwd_hook)
    prob = model(ids.unsqueeze(0))
    prob[0, 1].backward()
    h.remove()
    emb = captured["emb"]
    sal = (emb.grad * emb).norm(dim=-1)[0].detach().float().cpu()
    scores: Dict[int, float] = {}
    for j, ln in enumerate(token_lines):
        if ln >= 0:
            scores[ln] = scores.get(ln, 0.0) + float(sal[j])
    return scores


def _path_attributions(
    model: Model,
    ids: torch.Tensor,
    baseline_token_id: int = 1,
    steps: int = 20,
    noise: float = 0.0,
    n_samples: int = 1,
    seed: int = 0,
) -> torch.Tensor:
    """Path-integral attributions over the word-embedding layer, captum-free
    (reference linevul_main.py:955-1242 uses captum LayerIntegratedGradients
    / DeepLift / GradientShap on the same layer):

      attr = (emb(x) - emb(baseline)) * mean over path of d prob_vul / d emb

    steps>1, noise=0  -> integrated gradients (midpoint Riemann sum along
                         the straight-line path from the pad baseline);
      steps=1, alpha=1 -> DeepLift's rescale rule for this stack;
      noise>0, samples -> GradientShap (noisy baselines, random alphas).
    Returns per-token attribution (L,), the embedding dim summed out.
    """
    model.eval()
    emb_layer = model.encoder.embeddings.word_embeddings
    ids_b = ids.unsqueeze(0)
    with torch.no_grad():
        emb_x = emb_layer(ids_b)
        emb_base = emb_layer(torch.full_like(ids_b, baseline_token_id))
    gen = torch.Generator(device="cpu").manual_seed(seed)
    total = torch.zeros_like(emb_x)
    n_paths = 0
    for samp in range(n_samples):
        base = emb_base
        if noise > 0.0:
            base = emb_base + noise * torch.randn(
                emb_base.shape, generator=gen
            ).to(emb_base.device, emb_base.dtype)
        for s in range(steps):
            alpha = 1.0 if steps == 1 else (s + 0.5) / steps
            if noise > 0.0:
                alpha = float(torch.rand((), generator=gen))
            emb_in = (base + alpha * (emb_x - base)).detach().requires_grad_(True)

            def replace(_mod, _inp, _out, t=emb_in):
                return t

            h = emb_layer.register_forward_hook(replace)
            try:
                prob = model(ids_b)
            finally:
                h.remove()
            model.zero_grad(set_to_none=True)
            prob[0, 1].backward()
            total += emb_in.grad
            n_paths += 1
    model.zero_grad(set_to_none=True)
    attr = (emb_x - emb_base) * (total / max(1, n_paths))
    return attr.sum(-1)[0].detach().float().cpu()


def _per_line(tok_scores: torch.Tensor, token_lines: List[int]) -> Dict[int, float]:
    scores: Dict[int, float] = {}
    for j, ln in enumerate(token_lines):
        if ln >= 0:
            scores[ln] = scores.get(ln, 0.0) + float(tok_scores[j])
    return scores


def lig_line_scores(model, ids, token_lines, steps: int = 20) -> Dict[int, float]:
    """Layer integrated gradients (reference --reasoning_method lig)."""
    return _per_line(_path_attributions(model, ids, steps=steps), token_lines)


def deeplift_line_scores(model, ids, token_lines) -> Dict[int, float]:
    """DeepLift rescale-rule scores: grad at the input x (x - baseline)."""
    return _per_line(_path_attributions(model, ids, steps=1), token_lines)


def shap_line_scores(model, ids, token_lines, n_samples: int = 8) -> Dict[int, float]:
    """GradientShap-style scores: noisy baselines, random path points."""
    return _per_line(
        _path_attributions(model, ids, steps=1, noise=0.1, n_samples=n_samples),
        token_lines,
    )


def line_level_localization(model, ids, token_lines, method: str = "attention"):
    """The reference's 5-method localization matrix
    (linevul_main.py:1117-1242), captum-free."""
    if method == "attention":
        return attention_line_scores(model, ids, token_lines)
    if method in ("saliency", "gradient"):
        return saliency_line_scores(model, ids, token_lines)
    if method in ("lig", "ig"):
        return lig_line_scores(model, ids, token_lines)
    if method == "deeplift":
        return deeplift_line_scores(model, ids, token_lines)
    if method in ("shap", "gradientshap", "deeplift_shap"):
        return shap_line_scores(model, ids, token_lines)
    raise ValueError(f"unknown localization method {method!r}")


# ---------------------------------------------------------------------------
# localization metrics (reference :886-944)
# ---------------------------------------------------------------------------

def effort_at_topk(line_scores: List[Tuple[List[float], List[int]]], k_percent: float = 0.2) -> float:
    """Fraction of all ranked lines inspected before covering k% of the
    vulnerable lines (lower is better)."""
    ranked = []
    for scores, flaw in line_scores:
        order = np.argsort(scores)[::-1]
        for rank, idx in enumerate(order):
            ranked.append((rank / max(1, len(scores)), int(idx in flaw)))
    ranked.sort(key=lambda t: t[0])
    total_flaw = sum(f for _, f in ranked)
    target = k_percent * total_flaw
    seen_flaw, effort = 0, 0
    for _, f in ranked:
        effort += 1
        seen_flaw += f
        if seen_flaw >= target:
            break
    return effort / max(1, len(ranked))


def recall_at_topk_loc(line_scores: List[Tuple[List[float], List[int]]], k_percent: float = 0.2) -> float:
    """Fraction of vulnerable lines found when inspecting the top k% of
    each function's lines (higher is better)."""
    found, total = 0, 0
    for scores, flaw in line_scores:
        if not flaw:
            continue
        k = max(1, int(len(scores) * k_percent))
        top = set(np.argsort(scores)[::-1][:k].tolist())
        found += len(top & set(flaw))
        total += len(flaw)
    return found / max(1, total)


def ifa(line_scores: List[Tuple[List[float], List[int]]]) -> float:
    """Initial False Alarm (reference unixcoder linevul_main.py:676
    min_clean_lines_inspected): per example, the number of CLEAN lines
    ranked above the highest-ranked flaw line; mean over examples."""
    vals = []
    for scores, flaw in line_scores:
        if not flaw:
            continue
        order = sorted(range(len(scores)), key=lambda i: -scores[i])
        flaw_set = set(flaw)
        clean_seen = 0
        for i in order:
            if i in flaw_set:
                break
            clean_seen += 1
        vals.append(clean_seen)
    return float(sum(vals) / len(vals)) if vals else 0.0


def top_k_accuracy(line_scores, k: int = 10) -> float:
    """Fraction of examples whose top-k ranked lines hit >= 1 flaw line."""
    hit, n = 0, 0
    for scores, flaw in line_scores:
        if not flaw:
            continue
        n += 1
        top = set(np.argsort(scores)[::-1][:k].tolist())
        if top & set(flaw):
            hit += 1
    return hit / max(1, n)


# ---------------------------------------------------------------------------
# eval export (reference :742-829) + CodeT5 dataset export (:1400-1423)
# ---------------------------------------------------------------------------

@torch.no_grad()
def eval_export(model, dataset: TextDataset, device, out_csv: str, batch_size: int = 16):
    import csv

    model.eval()
    rows = []
    loader = torch.utils.data.DataLoader(dataset, batch_size=batch_size)
    for ids, label, index in loader:
        ids = ids.to(device)
        with torch.autocast(device_type="cuda", dtype=torch.bfloat16, enabled=ids.is_cuda):
            prob = model(ids)
        for i in range(ids.shape[0]):
            rows.append({
                "index": int(index[i]),
                "label": int(label[i]),
                "prob_vul": float(prob[i, 1]),
                "pred": int(prob[i, 1] > 0.5),
            })
    with open(out_csv, "w", newline="") as f:
        w = csv.DictWriter(f, fieldnames=["index", "label", "prob_vul", "pred"])
        w.writeheader()
        w.writerows(rows)
    return rows


def export_codet5_dataset(dataset: TextDataset, out_jsonl: str):
    with open(out_jsonl, "w") as f:
        for row in dataset.df.itertuples():
            f.write(json.dumps({"idx": int(row.id), "target": int(row.vul),
                                "func": row.func}) + "\n")


# ---------------------------------------------------------------------------
# CLI
# ---------------------------------------------------------------------------

def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--do_train", action="store_true")
    p.add_argument("--do_test", action="store_true")
    p.add_argument("--do_local_explanation", action="store_true")
    p.add_argument("--eval_export", action="store_true")
    p.add_argument("--export_codet5", action="store_true")
    p.add_argument("--dbgbench", action="store_true")
    p.add_argument("--reasoning_method", default="attention",
                   choices=["attention", "saliency", "gradient", "lig", "ig",
                            "deeplift", "shap", "gradientshap", "deeplift_shap"])
    p.add_argument("--attention_layer", type=int, default=-1,
                   help="encoder layer whose attention the 'attention' method scores "
                        "(-1 = last, this port's default). The reference scores the "
                        "first layer, 0: attentions[0][0] at "
                        "LineVul/unixcoder/linevul_main.py:1156")
    p.add_argument("--top_k_constant", type=int, default=10)
    p.add_argument("--effort_at_top_k", type=float, default=0.2)
    p.add_argument("--top_k_recall_loc", type=float, default=0.01)
    p.add_argument("--output_dir", default="saved_models/unixcoder")
    p.add_argument("--epochs", type=int, default=10)
    p.add_argument("--block_size", type=int, default=512)
    p.add_argument("--train_batch_size", type=int, default=16)
    p.add_argument("--eval_batch_size", type=int, default=16)
    p.add_argument("--learning_rate", type=float, default=2e-5)
    p.add_argument("--max_grad_norm", type=float, default=1.0)
    p.add_argument("--seed", type=int, default=1)
    p.add_argument("--n_synthetic", type=int, default=2000)
    p.add_argument("--num_layers", type=int, default=12)
    args = p.parse_args(argv)
    logging.basicConfig(level=logging.INFO)
    torch.manual_seed(args.seed)
    device = torch.device("cuda") if torch.cuda.is_available() else torch.device("cpu")
    cfg = unixcoder_config(args.num_layers)
    tokenizer = HashTokenizer(vocab_size=cfg.vocab_size)
    model = Model(config=cfg).to(device)
    datasets = {
        part: TextDataset(tokenizer, args, partition=part, block_size=args.block_size,
                          n_synthetic=args.n_synthetic)
        for part in ("train", "val", "test")
    }
    if args.dbgbench:
        # DbgBench is a held-out TEST set (reference unixcoder
        # linevul_main.py:133,142-145: split "holdout" -> test, label =
        # "patched" not in variant name); train/val stay Big-Vul
        from ..data.dclass import ds
        from ..data.text_dataset import synthetic_func_source

        dbg = ds("dbgbench", n=args.n_synthetic, seed=args.seed)
        dbg = dbg.assign(
            func=[synthetic_func_source(i + 10**6, vul=v)
                  for i, v in zip(dbg.id, dbg.vul)]
        )
        datasets["test"] = TextDataset(tokenizer, args, df=dbg,
                                       block_size=args.block_size)
    results = {}
    os.makedirs(args.output_dir, exist_ok=True)
    if args.do_train:
        results["best_f1"] = linevul_main.train(
            args, model, datasets["train"], datasets["val"], None, device
        )
    if args.do_test:
        args.profile = args.time = False
        results["test"] = linevul_main.test(args, model, datasets["test"], None, device)
    if args.eval_export:
        eval_export(model, datasets["test"], device,
                    os.path.join(args.output_dir, "predictions.csv"),
                    args.eval_batch_size)
    if args.export_codet5:
        export_codet5_dataset(datasets["test"], os.path.join(args.output_dir, "test.jsonl"))
    if args.do_local_explanation:
        line_results = []
        rows = [row for row in list(datasets["test"].df.itertuples())[:50] if row.vul]
        if args.reasoning_method == "attention":
            # batched: encode every selected function, score eval_batch_size
            # of them per encoder pass
            enc = [encode_with_lines(tokenizer, row.func, args.block_size) for row in rows]
            bs = max(1, args.eval_batch_size)
            for c0 in range(0, len(rows), bs):
                ids_b = torch.tensor([e[0] for e in enc[c0:c0 + bs]], dtype=torch.long,
                                     device=device)
                lines_b = torch.tensor([e[1] for e in enc[c0:c0 + bs]], dtype=torch.long,
                                       device=device)
                got = attention_line_scores_batched(model, ids_b, lines_b,
                                                    args.attention_layer).cpu()
                for row, sc in zip(rows[c0:c0 + bs], got):
                    n_lines = len(row.func.split("\n"))
                    vec = [float(sc[i]) if i < sc.shape[0] else 0.0 for i in range(n_lines)]
                    line_results.append((vec, [min(2, n_lines - 1)]))
            rows = []
        for row in rows:
            ids, tok_lines = encode_with_lines(tokenizer, row.func, args.block_size)
            ids_t = torch.tensor(ids, dtype=torch.long, device=device)
            scores = line_level_localization(model, ids_t, tok_lines, args.reasoning_method)
            n_lines = len(row.func.split("\n"))
            vec = [scores.get(i, 0.0) for i in range(n_lines)]
            flaw = [min(2, n_lines - 1)]  # synthetic flaw-line stand-in
            line_results.append((vec, flaw))
        results["effort@topk"] = effort_at_topk(line_results, args.effort_at_top_k)
        results["recall@topk_loc"] = recall_at_topk_loc(line_results, args.top_k_recall_loc)
        results["top_k_accuracy"] = top_k_accuracy(line_results, args.top_k_constant)
        results["ifa"] = ifa(line_results)
        # reference :700-701 writes per-method IFA records
        rec_dir = os.path.join(args.output_dir, "ifa_records")
        os.makedirs(rec_dir, exist_ok=True)
        with open(os.path.join(rec_dir, f"ifa_{args.reasoning_method}.txt"), "w") as f:
            f.write(str([results["ifa"]]))
    return results


if __name__ == "__main__":
    main()
