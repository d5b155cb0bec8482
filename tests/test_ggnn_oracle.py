"""CPU checks of the float64 GGNN oracles (tests/ggnn_oracle.py) that the GPU
tests in test_gpu_ggnn.py lean on: the exact loop against torch.nn.GRUCell,
the hand-written emulated backward against autograd, and the size of the
bf16 staging error the "4x" rule is measured in."""

import pytest
import torch

import ggnn_oracle as O
from deepdfa_amd.ops import reference as ref

H = 128
S = 3

_CASE = {}


def _case():
    if _CASE:
        return _CASE
    g, info = O.small_graph()
    buf = O.pack_reference(*O.make_params(H, seed=0))
    _CASE.update(g=g, info=info, buf=buf, w=O.oracle_weights(buf),
                 x=O.make_x(info["N"], H), go=O.make_grad_out(info["N"], H))
    return _CASE


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max())


def test_small_graph_properties():
    g, info = O.small_graph()
    deg = g.indptr[1:] - g.indptr[:-1]
    assert int(deg[0]) == 0                      # the 1-node graph
    assert int(deg[info["hub"]]) == 302          # self-loop + chain + 300 spokes
    assert g.num_nodes == 594


def test_pack_reference_layout():
    W_e, b_e, W_ih, W_hh, b_ih, b_hh = O.make_params(64, seed=3)
    buf = O.pack_reference(W_e, b_e, W_ih, W_hh, b_ih, b_hh)
    Hh = 64
    Wcat = buf["Wcat"]
    assert torch.equal(Wcat[2 * Hh:3 * Hh, Hh:], torch.zeros(Hh, Hh, dtype=torch.bfloat16))
    assert torch.equal(Wcat[3 * Hh:, :Hh], torch.zeros(Hh, Hh, dtype=torch.bfloat16))
    assert torch.equal(Wcat[3 * Hh:, Hh:], W_hh[2 * Hh:].to(torch.bfloat16))
    for gate in range(4):
        for j in (0, 1, 63):
            assert torch.equal(buf["Wcat_perm"][j * 4 + gate], Wcat[gate * Hh + j])
            assert buf["b_perm"][j * 4 + gate] == buf["b_cat"][gate * Hh + j]
    assert float(b_e.abs().min()) > 0.0
    # oracle_weights reproduces the merged bias exactly
    w = O.oracle_weights(buf)
    assert torch.equal((w[4][:2 * Hh] + w[5][:2 * Hh]), buf["b_cat"][:2 * Hh].double())


def test_exact_matches_grucell():
    c = _case()
    g = c["g"]
    W_e, b_e, W_ih, W_hh, b_ih, b_hh = c["w"]
    got = O.ggnn_exact(c["x"], g, *c["w"], S, grad_out=c["go"])

    cell = torch.nn.GRUCell(H, H).double()
    with torch.no_grad():
        cell.weight_ih.copy_(W_ih), cell.weight_hh.copy_(W_hh)
        cell.bias_ih.copy_(b_ih), cell.bias_hh.copy_(b_hh)
    We = W_e.clone().requires_grad_(True)
    be = b_e.clone().requires_grad_(True)
    x = c["x"].double().requires_grad_(True)
    h = x
    for _ in range(S):
        m = ref.spmm_sum(g.indptr, g.indices, h @ We.t() + be)
        h = cell(m, h)
    (h * c["go"].double()).sum().backward()
    want = {"h_final": h.detach(), "grad_x": x.grad, "gW_e": We.grad, "gb_e": be.grad,
            "gW_ih": cell.weight_ih.grad, "gW_hh": cell.weight_hh.grad,
            "gb_ih": cell.bias_ih.grad, "gb_hh": cell.bias_hh.grad}
    for k in O.OUT_NAMES:
        assert _rel(got[k], want[k]) <= 1e-12, k


def test_emulated_without_rounding_is_exact():
    c = _case()
    ex = O.ggnn_exact(c["x"], c["g"], *c["w"], S, grad_out=c["go"])
    em = O.ggnn_emulated(c["x"], c["g"], *c["w"], S, grad_out=c["go"], rounding=False)
    for k in O.OUT_NAMES:
        assert _rel(em[k], ex[k]) <= 1e-12, k


@pytest.mark.parametrize("steps", [1, 5])
def test_emulated_error_is_nonzero_and_small(steps):
    c = _case()
    ex = O.ggnn_exact(c["x"], c["g"], *c["w"], steps, grad_out=c["go"])
    em = O.ggnn_emulated(c["x"], c["g"], *c["w"], steps, grad_out=c["go"])
    for k in O.OUT_NAMES:
        err = O.rel_l2(em[k], ex[k])
        print(f"S={steps} {k}: emulated rel-L2 error {err:.3e}")
        assert 0.0 < err < 0.1, (k, err)


def test_step_exact_consistent_with_loop():
    c = _case()
    ex = O.ggnn_exact(c["x"], c["g"], *c["w"], 1)
    st =O.step_exact(c["x"], O.spmm(c["g"].indptr, c["g"].indices,
                                     c["x"].double() @ c["w"][0].t() + c["w"][1]),
                      c["g"], *c["w"])
    assert _rel(st["h_new"], ex["h_final"]) <= 1e-12
    assert torch.equal(st["m"][c["info"]["zero_in"]],
                       torch.zeros(len(c["info"]["zero_in"]), H, dtype=torch.float64))
    assert bool((st["pre_r_abs"] >= st["pre_r"].abs()).all())
    assert bool((st["m_wh_abs"] >= st["m_abs"] - 1e-12).all())
