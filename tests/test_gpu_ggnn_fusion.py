"""Stage fusion of the GGNN loop (csrc/bindings.hip ggnn_fused_fwd /
ggnn_fused_bwd, `fuse=True`, the default) against the unfused launch
sequence (`fuse=False`) and the float64 oracles of tests/ggnn_oracle.py.

fuse=True forms M[s] in gemm_gru's A staging, Gwh[s] in the grad_h GEMM's A
staging and the gate backward as the prologue of the grad_A GEMM. Every
summation order upstream of the atomic weight-grad epilogues is kept, so:

1  forward outputs and grad_x are BIT-identical between the two paths;
2  grad_out is only read, and grad_x does not alias it;
3  the six weight grads differ by atomic order alone and are held to bound E
   of tests/test_gpu_ggnn.py: relative L2 error against ggnn_exact at most
   4x that of ggnn_emulated.

Graphs, parameters and inputs are those of tests/test_gpu_ggnn.py.
"""

import pytest
import torch

import ggnn_oracle as O

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FWD_NAMES = ("h_final", "HH", "M", "R", "Z", "Nn", "HN")
WGRADS = ("gW_e", "gb_e", "gW_ih", "gW_hh", "gb_ih", "gb_hh")

_GRAPHS, _CASES = {}, {}


def _ext():
    from deepdfa_amd.ops import load_ext

    return load_ext(required=True)


def _graph(name):
    if name not in _GRAPHS:
        g = O.small_graph()[0] if name == "small" else O.chain_graph(int(name[1:]))
        _GRAPHS[name] = g.to(DEV)
    return _GRAPHS[name]


def _case(name, H):
    """Inputs built once and never modified."""
    key = (name, H)
    if key not in _CASES:
        g = _graph(name)
        N = g.num_nodes
        params = [p.to(DEV) for p in O.make_params(H, seed=H)]
        kbuf = O.empty_pack(H, DEV)
        _ext().pack_gru_weights(*params, *[kbuf[k] for k in O.PACK_ORDER])
        _CASES[key] = dict(g=g, N=N, H=H, kbuf=kbuf, w64=O.oracle_weights(O.pack_reference(*params)),
                           x=O.make_x(N, H).to(DEV), go=O.make_grad_out(N, H).to(DEV))
    return _CASES[key]


def _fwd(c, S, fuse):
    g, k = c["g"], c["kbuf"]
    outs = _ext().ggnn_fused_fwd(g.indptr, g.indices, c["x"], k["w_e16"], k["b_e16"],
                                 k["Wcat_perm"], k["b_perm"], S, fuse=fuse)
    return dict(zip(FWD_NAMES, outs))


def _bwd(c, f, S, fuse, go=None):
    g, k = c["g"], c["kbuf"]
    outs = _ext().ggnn_fused_bwd(c["go"] if go is None else go, g.t_indptr, g.t_indices, c["x"],
                                 k["W_eT"], k["WcatT"], f["HH"], f["M"], f["R"], f["Z"], f["Nn"],
                                 f["HN"], S, fuse=fuse)
    return dict(zip(O.GRAD_NAMES, outs))


# small: 45 zero in-degree nodes, a hub of in-degree >= 300, graphs cut by
# tile boundaries; H = 64 and 192 take the column-tail GEMMs. n6081 = 190 x 32
# + 1: row tail, gemm_gru on its 64-row tile and the rest on 32-row tiles.
# n24577 = 384 x 64 + 1: every kernel on its 64-row tile, 97-node chains
# crossing tiles.
BIT_CASES = [("small", 64, 2), ("small", 128, 2), ("small", 192, 2), ("n6081", 128, 2),
             ("n24577", 128, 1)]


@pytest.mark.parametrize("name,H,S", BIT_CASES)
def test_fused_stages_bit_equal(name, H, S):
    c = _case(name, H)
    if name == "small":
        deg = c["g"].indptr[1:] - c["g"].indptr[:-1]
        assert int((deg == 0).sum()) == 45 and int(deg.max()) >= 300
    f1, f0 = _fwd(c, S, True), _fwd(c, S, False)
    for k in FWD_NAMES:
        assert f1[k].shape == f0[k].shape and torch.equal(f1[k], f0[k]), k
    assert f1["M"].shape == (S, c["N"], H)
    assert bool(f1["h_final"].float().abs().sum() > 0)
    # both backwards from the same saved tensors
    b1, b0 = _bwd(c, f0, S, True), _bwd(c, f0, S, False)
    assert b1["grad_x"].dtype == torch.bfloat16 and b1["grad_x"].shape == (c["N"], H)
    assert torch.equal(b1["grad_x"], b0["grad_x"])
    assert bool(b1["grad_x"].float().abs().sum() > 0)
    for k in WGRADS:
        assert b1[k].shape == b0[k].shape and bool(torch.isfinite(b1[k]).all()), k


@pytest.mark.parametrize("fuse", [True, False])
def test_grad_out_is_only_read(fuse):
    c = _case("small", 128)
    S = 2
    f = _fwd(c, S, fuse)
    go = c["go"].clone()
    b = _bwd(c, f, S, fuse, go=go)
    torch.cuda.synchronize()
    assert torch.equal(go, c["go"])
    gx = b["grad_x"]
    assert gx.untyped_storage().data_ptr() != go.untyped_storage().data_ptr()
    lo, hi = gx.data_ptr(), gx.data_ptr() + gx.numel() * gx.element_size()
    glo, ghi = go.data_ptr(), go.data_ptr() + go.numel() * go.element_size()
    assert hi <= glo or ghi <= lo


@pytest.mark.parametrize("name,H,S", [("small", 128, 5), ("small", 192, 2)])
def test_fused_weight_grads_4x(name, H, S):
    c = _case(name, H)
    b = _bwd(c, _fwd(c, S, True), S, True)
    torch.cuda.synchronize()
    exact = O.ggnn_exact(c["x"], c["g"], *c["w64"], S, grad_out=c["go"])
    emu = O.ggnn_emulated(c["x"], c["g"], *c["w64"], S, grad_out=c["go"])
    for k in WGRADS:
        assert b[k].dtype == torch.float32, k
        ek, ee = O.rel_l2(b[k], exact[k]), O.rel_l2(emu[k], exact[k])
        print(f"[ratio] {name} H={H} S={S} {k}: err_kernel {ek:.3e} err_emulated {ee:.3e} "
              f"ratio {ek / ee:.3f}")
        assert ee > 0.0 and ek <= 4.0 * ee, (k, ek, ee)
