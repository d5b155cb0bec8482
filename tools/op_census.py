"""Print a JSON histogram of the aten ops one steady-state training step
dispatches (forward, backward, optimizer step; after two warm-up steps), for
a tiny graph-label and node-label FlowGNN, a 2-layer RoBERTa and a 2-layer
T5, each with and without FlatAdamW, with CAPTURE_REFRESH off and on.
Host-side dispatch counting only: the extension's kernels are invisible to
it, but every allocation, fill, cast and copy around them is not."""

import collections
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402
from torch.utils._python_dispatch import TorchDispatchMode  # noqa: E402


class Census(TorchDispatchMode):
    def __init__(self):
        super().__init__()
        self.counts = collections.Counter()

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        self.counts[str(func)] += 1
        return func(*args, **(kwargs or {}))


def flowgnn(label_style):
    from deepdfa_amd.graph import synthetic_cfg_batch
    from deepdfa_amd.models import FlowGNNGGNNModule

    model = FlowGNNGGNNModule(input_dim=64, hidden_dim=32, n_steps=2,
                              num_output_layers=3, label_style=label_style).cuda()
    g = synthetic_cfg_batch(8, seed=0, input_dim=64).to("cuda")
    return model, lambda: model.loss_fn(model(g, {}).float(), model.get_label(g))


def transformer(kind):
    from deepdfa_amd.models.linevul import Model
    from deepdfa_amd.models.roberta import RobertaConfig
    from deepdfa_amd.models.t5 import T5Config, T5ForConditionalGeneration

    gen = torch.Generator().manual_seed(1)
    ids = torch.randint(3, 30000, (2, 128), generator=gen).cuda()
    if kind == "roberta":
        model = Model(config=RobertaConfig(num_hidden_layers=2)).cuda()
        labels = torch.randint(0, 2, (2,), generator=gen).cuda()
    else:
        model = T5ForConditionalGeneration(T5Config(num_layers=2, num_decoder_layers=2)).cuda()
        labels = torch.randint(3, 30000, (2, 128), generator=gen).cuda()
    return model, lambda: model(ids, labels=labels)[0]


MODELS = {
    "flowgnn_graph": lambda: flowgnn("graph"),
    "flowgnn_node": lambda: flowgnn("node"),
    "roberta2": lambda: transformer("roberta"),
    "t5_2": lambda: transformer("t5"),
}


def main():
    assert torch.cuda.is_available(), "op_census.py needs a GPU"
    from deepdfa_amd.ops import transformer as tops
    from deepdfa_amd.parallel.optim import FlatAdamW

    result = {}
    for name, build in MODELS.items():
        for flat in (False, True):
            torch.manual_seed(0)
            model, loss_fn = build()
            opt = (FlatAdamW if flat else torch.optim.AdamW)(model.parameters(), lr=1e-4)

            def step():
                with torch.autocast(device_type="cuda", dtype=torch.bfloat16):
                    loss = loss_fn()
                opt.zero_grad()
                loss.backward()
                opt.step()

            for refresh in (False, True):
                tops.CAPTURE_REFRESH[0] = refresh
                try:
                    step()
                    step()
                    with Census() as census:
                        step()
                finally:
                    tops.CAPTURE_REFRESH[0] = False
                row = f"{name}/{'flat' if flat else 'adamw'}/refresh_{'on' if refresh else 'off'}"
                result[row] = dict(census.counts)
    print(json.dumps(result, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
