"""Node-level (statement) training on CPU: padded-step equivalence, the
per-node weight expansion, undersample_node_on_loss_factor and the
node_head op's fp32 route."""

import pytest
import torch
import torch.nn.functional as F

from deepdfa_amd.graph import synthetic_cfg_batch
from deepdfa_amd.graph.pad import bucket_shape, pad_batch
from deepdfa_amd.models import FlowGNNGGNNModule

_STATIC_KEYS = ("node_offsets", "indptr", "indices", "t_indptr", "t_indices")
BUCKET = (9, 64, 256)  # b_pad, node quantum, edge quantum


def _model(seed=0, **kw):
    torch.manual_seed(seed)
    return FlowGNNGGNNModule(input_dim=1002, label_style="node", **kw)


def _total(stats):
    return int(stats.counts.sum())


@pytest.fixture(scope="module")
def batch0():
    g = synthetic_cfg_batch(8, seed=0)
    assert g.num_nodes == 247 and int(g.ndata["_VULN"].sum()) == 12
    return g


def _same_bucket_batch(g0):
    """Another 8-graph batch that pads to g0's bucket but has different
    graph boundaries."""
    shape = bucket_shape(g0, *BUCKET)
    for seed in range(1, 200):
        g = synthetic_cfg_batch(8, seed=seed)
        if bucket_shape(g, *BUCKET) == shape and not torch.equal(
            g.node_offsets, g0.node_offsets
        ):
            return g
    raise AssertionError("no second batch in the same bucket")


def test_padded_step_matches_unpadded(batch0):
    ref = _model()
    loss_ref = ref.training_step(batch0)
    loss_ref.backward()
    assert _total(ref.metrics["train"]) == 247

    m = _model()
    padded, w = pad_batch(batch0, *bucket_shape(batch0, *BUCKET))
    assert padded.num_nodes > 247
    loss = m.training_step_masked(padded, {}, w)
    loss.backward()
    assert abs(float(loss) - float(loss_ref)) < 1e-6
    for (n, p), (_, q) in zip(m.named_parameters(), ref.named_parameters()):
        assert p.grad is not None, n
        assert (p.grad - q.grad).abs().max() < 1e-6, n
    assert _total(m.metrics["train"]) == 247
    assert torch.equal(m.metrics["train"].counts, ref.metrics["train"].counts)


def test_node_weight_follows_refilled_offsets(batch0):
    """One static padded graph refilled in place (as the capture path
    does before a replay): the node weight must come from the NEW
    node_offsets, not from a per-object segment cache."""
    g1 = _same_bucket_batch(batch0)
    shape = bucket_shape(batch0, *BUCKET)
    static_g, static_w = pad_batch(batch0, *shape)
    m = _model()
    m.training_step_masked(static_g, {}, static_w)  # first use of the object

    padded1, w1 = pad_batch(g1, *shape)
    for k in _STATIC_KEYS:
        getattr(static_g, k).copy_(getattr(padded1, k))
    for k, v in padded1.ndata.items():
        static_g.ndata[k].copy_(v)
    static_w.copy_(w1)

    m.metrics["train"].reset()
    loss = m.training_step_masked(static_g, {}, static_w)
    loss_ref = _model().training_step(g1)
    assert abs(float(loss) - float(loss_ref)) < 1e-6
    assert _total(m.metrics["train"]) == g1.num_nodes


def test_node_weight_values(batch0):
    padded, w = pad_batch(batch0, *bucket_shape(batch0, *BUCKET))
    nw = FlowGNNGGNNModule.node_weight(padded, w)
    assert nw.shape == (padded.num_nodes,)
    assert torch.equal(nw[:247], torch.ones(247)) and float(nw[247:].sum()) == 0.0
    # a weight that differs per graph lands on exactly that graph's nodes
    gw = torch.arange(9, dtype=torch.float32)
    assert torch.equal(FlowGNNGGNNModule.node_weight(padded, gw),
                       gw[padded.segment_ids().long()])


def test_undersample_mask_and_loss(batch0):
    label = batch0.ndata["_VULN"].float()
    a = _model(undersample_node_on_loss_factor=2)
    loss = a.training_step(batch0)
    assert _total(a.metrics["train"]) == 36

    b = _model(undersample_node_on_loss_factor=2)  # same seed: same draw
    mask = b.undersample_node_mask(label)
    assert set(mask.unique().tolist()) == {0.0, 1.0}
    assert int(mask[label == 1].sum()) == 12
    assert int(mask[label == 0].sum()) == 24
    keep = mask > 0
    with torch.no_grad():
        logits = b(batch0, {}).float()
    expect = F.binary_cross_entropy_with_logits(logits[keep], label[keep])
    assert abs(float(loss) - float(expect)) < 1e-6

    # consecutive steps draw different negatives
    mask2 = b.undersample_node_mask(label)
    assert int(mask2.sum()) == 36 and not torch.equal(mask, mask2)


def test_undersample_mask_under_padding(batch0):
    """Padding nodes are never sampled as negatives."""
    padded, w = pad_batch(batch0, *bucket_shape(batch0, *BUCKET))
    m = _model(undersample_node_on_loss_factor=2)
    m.training_step_masked(padded, {}, w)
    assert _total(m.metrics["train"]) == 36
    label = padded.ndata["_VULN"].float()
    mask = m.undersample_node_mask(label, valid=m.node_weight(padded, w))
    assert int(mask.sum()) == 36 and float(mask[247:].sum()) == 0.0


def test_undersample_clamps_to_all_negatives(batch0):
    label = batch0.ndata["_VULN"].float()
    m = _model(undersample_node_on_loss_factor=100)  # 1200 > 235 negatives
    mask = m.undersample_node_mask(label)
    assert torch.equal(mask, torch.ones(247))
    loss = m.training_step(batch0)
    assert torch.isfinite(loss) and _total(m.metrics["train"]) == 247


def test_factor_unset_is_unmasked(batch0):
    m = _model()
    assert m.undersample_node_mask(batch0.ndata["_VULN"].float()) is None


def test_unsupported_label_style_message(batch0):
    m = FlowGNNGGNNModule(input_dim=1002, label_style="dataflow_solution_in")
    with pytest.raises(NotImplementedError, match="_DF_IN"):
        m.get_label(batch0)


def test_graph_weight_on_node_logits_is_rejected():
    from deepdfa_amd.ops.flowgnn import bce_with_logits

    with pytest.raises(ValueError, match="weight shape"):
        bce_with_logits(torch.zeros(10), torch.zeros(10), weight=torch.ones(3))


def test_node_head_cpu_matches_output_layer():
    from deepdfa_amd.ops.flowgnn import node_head

    m = _model()
    torch.manual_seed(1)
    h, fe = torch.randn(37, 128), torch.randn(37, 128)
    ol = m.output_layer
    got = node_head(h, fe, ol[0], ol[2], ol[4])
    want = ol(torch.cat([h, fe], -1)).squeeze(-1)
    assert got.shape == (37,)
    assert (got - want).abs().max() < 1e-5

    # and so do the gradients
    hs = [t.clone().requires_grad_() for t in (h, fe)]
    node_head(hs[0], hs[1], ol[0], ol[2], ol[4]).square().sum().backward()
    got_g = [hs[0].grad, hs[1].grad] + [p.grad.clone() for p in ol.parameters()]
    for p in ol.parameters():
        p.grad = None
    hr = [t.clone().requires_grad_() for t in (h, fe)]
    ol(torch.cat(hr, -1)).squeeze(-1).square().sum().backward()
    want_g = [hr[0].grad, hr[1].grad] + [p.grad for p in ol.parameters()]
    for g, w in zip(got_g, want_g):
        assert g.shape == w.shape
        assert (g - w).abs().max() < 1e-4 * max(1.0, float(w.abs().max()))


def test_node_head_cpu_gradcheck():
    from deepdfa_amd.ops.flowgnn import _NodeHead

    torch.manual_seed(0)
    d1, d = 3, 8  # the fp32/fp64 route is width-agnostic
    dd = dict(dtype=torch.float64, requires_grad=True)
    args = [torch.randn(5, d1, **dd), torch.randn(5, d - d1, **dd),
            torch.randn(d, d, **dd), torch.randn(d, **dd),
            torch.randn(d, d, **dd), torch.randn(d, **dd),
            torch.randn(1, d, **dd), torch.randn(1, **dd)]
    assert torch.autograd.gradcheck(lambda *a: _NodeHead.apply(*a, None), args)
