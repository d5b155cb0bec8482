"""BaseModule: shared train/val/test-step behavior for graph models.

Parity target: reference DDFA/code_gnn/models/base_module.py:26-383 —
BCEWithLogits loss with optional pos_weight, graph-level label reduction
(per-graph max of node _VULN), threshold-0.5 metric collections per split
(plus positive-only / negative-only test clones), PR-curve export and a
classification report at test end. Implemented Lightning-free on top of
our trainer (deepdfa_amd/train/trainer.py); metrics are counter-based so
DDP aggregation is one all_reduce.
"""

from __future__ import annotations

from typing import Dict, Optional

import torch
from torch import nn

from ..ops import segment_max
from ..utils.metrics import BinaryStats, classification_report_dict, pr_curve


class BaseModule(nn.Module):
    def __init__(
        self,
        undersample_node_on_loss_factor=None,
        test_every: bool = False,
        tune_nni: bool = False,
        positive_weight: Optional[float] = None,
        profile: bool = False,
        time: bool = False,
        label_style: str = "graph",
    ):
        super().__init__()
        self.class_threshold = 0.5
        self.label_style = label_style
        self.hparams: Dict = dict(
            undersample_node_on_loss_factor=undersample_node_on_loss_factor,
            test_every=test_every,
            tune_nni=tune_nni,
            positive_weight=positive_weight,
            profile=profile,
            time=time,
            label_style=label_style,
        )
        self.metrics = {
            "train": BinaryStats(self.class_threshold),
            "val": BinaryStats(self.class_threshold),
            "test": BinaryStats(self.class_threshold),
            "test_1": BinaryStats(self.class_threshold),
            "test_0": BinaryStats(self.class_threshold),
        }
        if positive_weight is not None:
            self.register_buffer("pos_weight", torch.tensor([float(positive_weight)]))
        else:
            self.pos_weight = None
        self._test_preds: list = []
        self._test_labels: list = []

    # -- labels --------------------------------------------------------------

    def get_label(self, graph) -> torch.Tensor:
        if self.label_style == "node":
            label = graph.ndata["_VULN"]
        elif self.label_style == "graph":
            label = segment_max(graph.ndata["_VULN"].float(), graph)
        else:
            # dataflow_solution_in/out: the reference's own dataset never
            # attaches _DF_IN/_DF_OUT, so there is nothing to train on
            raise NotImplementedError(
                f"label_style={self.label_style!r} is not supported: only "
                "'graph' and 'node' are; the dataflow_solution_in/out styles "
                "need per-node _DF_IN/_DF_OUT labels that no dataset here (nor "
                "the reference's) attaches"
            )
        return label.float()

    # -- node-level masks -----------------------------------------------------

    @staticmethod
    def node_weight(graph, graph_weight: torch.Tensor) -> torch.Tensor:
        """Expand a per-graph weight (b,) to per-node (N,): node i takes the
        weight of the graph whose [offset, next offset) range holds it.
        Static-shape ops on graph.node_offsets only — recomputed every step,
        so a capture bucket whose static node_offsets are refilled before a
        replay gets the new batch's segments (BatchedCFG.segment_ids()
        caches its result and would go stale there)."""
        offs = graph.node_offsets
        n = graph.ndata["_VULN"].shape[0]
        idx = torch.arange(n, device=offs.device, dtype=offs.dtype)
        seg = torch.bucketize(idx, offs[1:], right=True)
        seg = seg.clamp_(max=graph_weight.shape[0] - 1)
        return graph_weight[seg]

    def undersample_node_mask(
        self, label: torch.Tensor, valid: Optional[torch.Tensor] = None
    ) -> Optional[torch.Tensor]:
        """0/1 node mask for undersample_node_on_loss_factor (reference
        base_module.py:171-199): every positive node plus
        k = min(round(n_pos * factor), n_neg) negatives drawn uniformly
        without replacement. None when the factor is unset. `valid` (0/1
        per node) keeps padding nodes out of the negative pool. The reference
        raises when k > n_neg; here k is clamped (docs/PARITY.md). The
        generator is module-owned and seeded from torch.initial_seed() at
        first use, so seed_everything makes the draws reproducible."""
        factor = self.hparams.get("undersample_node_on_loss_factor")
        if factor is None:
            return None
        gen = getattr(self, "_node_sample_gen", None)
        if gen is None:
            gen = torch.Generator()  # CPU: the draw is index bookkeeping
            gen.manual_seed(torch.initial_seed())
            self._node_sample_gen = gen
        lab = label.detach().to("cpu")
        pos = (lab > 0).nonzero(as_tuple=True)[0]
        is_neg = lab <= 0
        if valid is not None:
            is_neg &= valid.detach().to("cpu") > 0
        neg = is_neg.nonzero(as_tuple=True)[0]
        k = min(int(round(pos.numel() * float(factor))), neg.numel())
        keep = neg[torch.randperm(neg.numel(), generator=gen)[:k]]
        mask = torch.zeros(lab.shape[0], dtype=torch.float32)
        mask[pos] = 1.0
        mask[keep] = 1.0
        return mask.to(label.device)

    # -- loss -----------------------------------------------------------------

    def loss_fn(
        self,
        logits: torch.Tensor,
        label: torch.Tensor,
        weight: Optional[torch.Tensor] = None,
    ) -> torch.Tensor:
        """weight (per-graph 0/1) masks out capture-padding dummy graphs
        (graph/pad.py): the weighted mean equals the unpadded batch mean.
        GPU path = ONE fused kernel each way (ops.flowgnn.bce_with_logits);
        torch's chain was ~6 launch-floor nodes at batch 256."""
        from ..ops.flowgnn import bce_with_logits

        return bce_with_logits(logits, label, weight=weight,
                               pos_weight=self.pos_weight)

    # -- steps (called by the trainer) ---------------------------------------

    def training_step(self, batch) -> torch.Tensor:
        graph, extrafeats = batch if isinstance(batch, tuple) else (batch, {})
        label = self.get_label(graph)
        logits = self(graph, extrafeats)
        mask = self.undersample_node_mask(label) if self.label_style == "node" else None
        loss = self.loss_fn(logits.float(), label, weight=mask)
        with torch.no_grad():
            self.metrics["train"].to(logits.device).update(
                torch.sigmoid(logits.float()), label, mask=mask
            )
        return loss

    def training_step_masked(self, graph, extrafeats, weight: torch.Tensor) -> torch.Tensor:
        """Capture-path training step over a padded batch (graph/pad.py):
        identical math to training_step on the unpadded batch — the dummy
        graphs contribute zero loss, zero gradient and zero metric counts."""
        label = self.get_label(graph)
        logits = self(graph, extrafeats)
        if self.label_style == "node":
            # per-graph 0/1 -> per-node 0/1 (dummy-graph nodes get 0)
            weight = self.node_weight(graph, weight)
            mask = self.undersample_node_mask(label, valid=weight)
            if mask is not None:  # eager only: data-dependent k, never captured
                weight = mask
        loss = self.loss_fn(logits.float(), label, weight=weight)
        with torch.no_grad():
            self.metrics["train"].to(logits.device).update(
                torch.sigmoid(logits.float()), label, mask=weight
            )
        return loss

    @torch.no_grad()
    def validation_step(self, batch) -> torch.Tensor:
        graph, extrafeats = batch if isinstance(batch, tuple) else (batch, {})
        label = self.get_label(graph)
        logits = self(graph, extrafeats)
        loss = self.loss_fn(logits.float(), label)
        self.metrics["val"].to(logits.device).update(torch.sigmoid(logits.float()), label)
        return loss

    @torch.no_grad()
    def test_step(self, batch) -> torch.Tensor:
        graph, extrafeats = batch if isinstance(batch, tuple) else (batch, {})
        label = self.get_label(graph)
        logits = self(graph, extrafeats)
        loss = self.loss_fn(logits.float(), label)
        probs = torch.sigmoid(logits.float())
        self.metrics["test"].to(logits.device).update(probs, label)
        pos, neg = label == 1, label == 0
        if pos.any():
            self.metrics["test_1"].to(logits.device).update(probs[pos], label[pos])
        if neg.any():
            self.metrics["test_0"].to(logits.device).update(probs[neg], label[neg])
        self._test_preds.append(probs.detach().cpu())
        self._test_labels.append(label.detach().cpu())
        return loss

    # -- epoch end ------------------------------------------------------------

    def epoch_metrics(self, split: str, reset: bool = True) -> Dict[str, float]:
        stats = self.metrics[split]
        stats.all_reduce()
        out = {f"{split}_{k}": v for k, v in stats.compute().items()}
        if reset:
            stats.reset()
        return out

    def test_epoch_end(self, out_dir: Optional[str] = None) -> Dict:
        """Compute test metrics + PR curve + classification report, optionally
        exporting pr.csv (base_module.py:358-361 contract)."""
        results = {}
        for split in ("test", "test_1", "test_0"):
            results.update(self.epoch_metrics(split, reset=False))
        if self._test_preds:
            probs = torch.cat(self._test_preds)
            labels = torch.cat(self._test_labels)
            ths, precs, recs = pr_curve(probs, labels)
            results["classification_report"] = classification_report_dict(probs, labels)
            if out_dir is not None:
                import csv
                import os

                with open(os.path.join(out_dir, "pr.csv"), "w", newline="") as f:
                    w = csv.writer(f)
                    w.writerow(["threshold", "precision", "recall"])
                    for row in zip(ths, precs, recs):
                        w.writerow(row)
        self._test_preds.clear()
        self._test_labels.clear()
        return results
