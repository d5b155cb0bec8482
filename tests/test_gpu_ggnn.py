"""GGNN message-passing kernels against float64 oracles (tests/ggnn_oracle.py):
pack_gru_weights, spmm_sum, gru_gates / gru_gates2, the gemm_bias 64-row
tile, and the fused loop ggnn_fused_fwd / ggnn_fused_bwd.

Every reference is float64 on the GPU, computed from the SAME inputs the
kernels see (x pre-quantised to bf16, weights = the bf16 values of the
packed buffers, built by torch ops independently of the pack kernel). Every
bound is computed from those inputs and the reference, never from a kernel
output. u = 2^-8 is the bf16 unit roundoff (0 for fp32 tensors); 2^-23 per
accumulated term is twice the fp32 unit roundoff, so the accumulation terms
carry a 2x margin over worst-case sequential summation.

A  pack            bit-exact against the torch construction.
B  spmm_sum        zero in-degree rows exactly 0; otherwise
                   |got - ref| <= u |ref| + deg_v 2^-23 sum_e |x_e|.
C  gates           forward, per output (P = pre-activation, a = n's argument):
                     r, z   u |ref| + eps_fn + 1/4 dP
                     n      u |ref| + eps_fn + da,
                            da = (eps_fn + 1/4 dP_r)|hn| + 2^-22 (|i_n| + |r hn|)
                     h'     u |ref| + |h - n| e_z + (1 - z) e_n + 2^-21 (|n| + |h|)
                   with e_z, e_n the r/z/n bounds without their u term,
                   eps_fn = 2^-20 for the fp32 __expf / tanhf evaluation (a few
                   ulp of a value <= 1, 2^11 below the bf16 term), dP the fp32
                   error of forming P (2^-23 (|gi| + |gh|) for the one add of
                   gru_gates, 0 for gru_gates2 which reads P) and the
                   derivative bounds 1/4 (sigmoid) and 1 (tanh).
                   backward, teacher-forced on the kernel's own saved
                   r, z, n, hn: every output is a product of <= 7 factors,
                     |got - ref| <= u |ref| + 8 2^-23 T,
                   T the same product with every difference (1 - z), (h - n),
                   (1 - n^2), (1 - r) replaced by the sum of its operands'
                   magnitudes (cancellation-safe).
D  fused forward   teacher-forced per step from the kernel's own HH[s]:
                     wh_u (not returned) errs by u |wh_u| + (H+1) 2^-23 W_u,
                       W_u = sum_k |W_jk h_uk| + |b_j|
                     M    (1 + 2^-7) sum_{u->v} [u |wh_u| + (H+1) 2^-23 W_u
                          + deg_v 2^-23 |wh_u|] + u |m|   (0 where deg_v = 0)
                   and from the kernel's own M[s], HH[s], with
                   dP = (2H+1) 2^-23 sum |w a| the fp32 pre-activation error:
                     HN   u |hn| + dP_hn
                     R, Z u |ref| + eps_fn + 1/4 dP
                     Nn   u |n| + eps_fn + da, n from the float64 r,
                          da = dP_in + (eps_fn + 1/4 dP_r)|hn| + dP_hn
                               + 2^-22 (|P_in| + |r hn|)
                     HH[s+1]  as h' in C.
                   All bounds are widened by (1 + 2^-7) for second-order terms.
E  whole loop      relative L2 error against ggnn_exact, per tensor:
                     err_kernel <= 4 err_emulated
                   where ggnn_emulated makes the kernels' bf16 roundings in
                   float64; the two differ only by fp32-vs-float64
                   accumulation and the bf16 flips that causes. 4 is the
                   margin of the MLP bound in test_gpu_graph_head.py.
F  direct accumulation into live fp32 views pre-filled with g0:
                     |got - (g0 + t G)| <= S N 2^-23 (|g0| + t sum_k |a_k b_k|)
                   G the returned-form grads of the same call, t the number of
                   calls, sum_k |a_k b_k| taken from the emulation. The two
                   forms add the same K-chunk partial sums (<= S N / 768 + 1
                   of them, the launchers' kchunk floor) in a different
                   order and on top of g0, so S N terms is a loose cover.
H  gemm_bias       |got - ref| <= (1 + 2^-7)(u |ref| + (K+2) 2^-23
                   (sum_k |a w| + |b| + |addend|)).

err_kernel / err_emulated observed on an MI355X (E and G), in the order
h_final, grad_x, gW_e, gb_e, gW_ih, gW_hh, gb_ih, gb_hh:
  small  H=128 S=5   1.000 1.026 0.984 1.013 0.998 0.983 0.992 0.991
  small  H=128 S=1   1.000 1.000 1.000 1.000 1.000 1.000 1.000 1.001
  n24577 H=128 S=1   1.000 1.000 1.000 0.999 1.000 1.000 1.000 1.002
  n6081  H=128 S=2   1.000 1.000 0.999 0.995 1.000 1.000 0.999 0.997
  small  H=64  S=2   1.000 1.000 1.000 1.000 1.000 1.000 1.000 1.000
  small  H=192 S=2   1.000 1.000 1.000 1.000 1.000 1.000 0.999 1.000
The module-level runs (G) repeat the H=64 and H=192 rows exactly. No ratio
is above 1.03; err_emulated itself lies between 2.4e-3 and 3.2e-2.
"""

import pytest
import torch

import ggnn_oracle as O
from oracle_checks import assert_within as _assert_within

pytestmark = pytest.mark.gpu

U16 = 2.0 ** -8
ACC = 2.0 ** -23
EPS_FN = 2.0 ** -20
SECOND = 1.0 + 2.0 ** -7
DEV = "cuda:0"

FWD_NAMES = ("h_final", "HH", "M", "R", "Z", "Nn", "HN")
BWD_NAMES = O.GRAD_NAMES
WGRADS = ("gW_e", "gb_e", "gW_ih", "gW_hh", "gb_ih", "gb_hh")


def _ext():
    from deepdfa_amd.ops import load_ext

    return load_ext(required=True)


def _u(dtype):
    return U16 if dtype == torch.bfloat16 else 0.0


# --------------------------------------------------------------------------
# cases, built once and never modified
# --------------------------------------------------------------------------

_GRAPHS, _CASES, _RUNS = {}, {}, {}


def _graph(name):
    if name not in _GRAPHS:
        if name == "small":
            g, info = O.small_graph()
        else:
            N = int(name[1:])
            g, info = O.chain_graph(N), {"N": N, "zero_in": [], "hub": None}
        deg = (g.indptr[1:] - g.indptr[:-1]).to(torch.float64).to(DEV)
        _GRAPHS[name] = (g.to(DEV), info, deg)
    return _GRAPHS[name]


def _case(name, H):
    key = (name, H)
    if key in _CASES:
        return _CASES[key]
    ext = _ext()
    g, info, deg = _graph(name)
    params = [p.to(DEV) for p in O.make_params(H, seed=H)]
    kbuf = O.empty_pack(H, DEV)
    ext.pack_gru_weights(*params, *[kbuf[k] for k in O.PACK_ORDER])
    rbuf = O.pack_reference(*params)
    N = info["N"]
    _CASES[key] = dict(
        g=g, info=info, deg=deg, N=N, H=H, params=params, kbuf=kbuf, rbuf=rbuf,
        w64=O.oracle_weights(rbuf), x=O.make_x(N, H).to(DEV), go=O.make_grad_out(N, H).to(DEV))
    return _CASES[key]


def _fwd(c, S):
    g, k = c["g"], c["kbuf"]
    outs = _ext().ggnn_fused_fwd(g.indptr, g.indices, c["x"], k["w_e16"], k["b_e16"],
                                 k["Wcat_perm"], k["b_perm"], S)
    return dict(zip(FWD_NAMES, outs))


def _bwd(c, f, S, **direct):
    g, k = c["g"], c["kbuf"]
    return _ext().ggnn_fused_bwd(c["go"], g.t_indptr, g.t_indices, c["x"], k["W_eT"], k["WcatT"],
                                 f["HH"], f["M"], f["R"], f["Z"], f["Nn"], f["HN"], S, **direct)


def _run(name, H, S):
    """Kernel forward + returned-form backward, and both oracles."""
    key = (name, H, S)
    if key in _RUNS:
        return _RUNS[key]
    c = _case(name, H)
    f = _fwd(c, S)
    b = dict(zip(BWD_NAMES, _bwd(c, f, S)))
    torch.cuda.synchronize()
    exact = O.ggnn_exact(c["x"], c["g"], *c["w64"], S, grad_out=c["go"])
    emu = O.ggnn_emulated(c["x"], c["g"], *c["w64"], S, grad_out=c["go"])
    _RUNS[key] = dict(c=c, f=f, b=b, exact=exact, emu=emu)
    return _RUNS[key]


# the loop cases of D/E (G = the H != 128 rows)
BIG = [("n24577", 128, 1), ("n6081", 128, 2)]
FWD_CASES = [("small", 128, 3)] + BIG + [("small", 64, 2), ("small", 192, 2)]
LOOP_CASES = [("small", 128, 5), ("small", 128, 1)] + BIG + [("small", 64, 2), ("small", 192, 2)]
DIRECT_CASES = [("small", 128, 2), ("n6081", 128, 2), ("small", 64, 2)]


def test_graph_fixtures():
    g, info, deg = _graph("small")
    O.check_small_graph(g.to("cpu"), info)
    assert int(deg[info["hub"]]) >= 300 and info["N"] == 594
    for name, N in (("n24577", 24577), ("n6081", 6081)):
        gb, _, degb = _graph(name)
        assert gb.num_nodes == N and N % 64 == 1
        assert int(degb.min()) == 1 and int(degb.max()) == 2
        assert int(gb.node_offsets[1]) == 97
    # the tile switch of launch_gemm_bias2 / launch_gemm_gru: ceil(N/64) * COL/128 >= 384
    t = lambda N, col: ((N + 63) // 64) * (col // 128)
    assert t(24577, 128) >= 384 and t(24577, 256) >= 384 and t(24577, 512) >= 384
    assert t(6081, 512) >= 384 and t(6081, 256) < 384 and t(6081, 128) < 384
    assert t(6080, 512) < 384 and t(594, 512) < 384


# --------------------------------------------------------------------------
# A. pack_gru_weights
# --------------------------------------------------------------------------

@pytest.mark.parametrize("H", [64, 128, 192])
def test_pack_bit_exact(H):
    c = _case("small", H)
    W_e, b_e, W_ih, W_hh, b_ih, b_hh = c["params"]
    assert float(b_e.abs().min()) > 0 and float(b_hh.abs().min()) > 0
    k, r = c["kbuf"], c["rbuf"]           # k was pre-filled with NaN
    for name in O.PACK_ORDER:
        assert torch.equal(k[name], r[name]), name
    bf = torch.bfloat16
    Wcat = k["Wcat"]
    zero = torch.zeros(H, H, dtype=bf, device=DEV)
    assert torch.equal(Wcat[2 * H:3 * H, H:], zero) and torch.equal(Wcat[3 * H:, :H], zero)
    assert torch.equal(k["b_cat"][:2 * H], (b_ih[:2 * H] + b_hh[:2 * H]).to(bf))
    assert torch.equal(k["b_cat"][2 * H:3 * H], b_ih[2 * H:].to(bf))
    assert torch.equal(k["b_cat"][3 * H:], b_hh[2 * H:].to(bf))
    j = torch.arange(H, device=DEV)
    for gate in range(4):
        assert torch.equal(k["Wcat_perm"][j * 4 + gate], Wcat[gate * H + j])
        assert torch.equal(k["b_perm"][j * 4 + gate], k["b_cat"][gate * H + j])
    assert torch.equal(k["WcatT"], Wcat.t()) and torch.equal(k["W_eT"], k["w_e16"].t())
    assert torch.equal(k["w_e16"], W_e.to(bf)) and torch.equal(k["b_e16"], b_e.to(bf))


# --------------------------------------------------------------------------
# B. spmm_sum
# --------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("D", [2, 64, 128, 130, 192, 256])
@pytest.mark.parametrize("transpose", [False, True])
def test_spmm_sum(transpose, D, dtype):
    g, info, _ = _graph("small")
    indptr, indices = (g.t_indptr, g.t_indices) if transpose else (g.indptr, g.indices)
    gen = torch.Generator().manual_seed(D)
    x = torch.randn(info["N"], D, generator=gen).to(dtype).to(DEV)
    got = _ext().spmm_sum(indptr, indices, x)
    deg = (indptr[1:] - indptr[:-1]).double()
    ref = O.spmm(indptr, indices, x.double())
    bound = _u(dtype) * ref.abs() + deg[:, None] * ACC * O.spmm(indptr, indices, x.double().abs())
    empty = deg == 0
    # forward: the fixture's isolated nodes; transpose: only the 1-node graph
    assert int(empty.sum()) == (1 if transpose else len(info["zero_in"]))
    assert got.dtype == dtype
    assert bool((got[empty] == 0).all()), "zero in-degree rows must be exactly 0"
    assert bool((bound[empty] == 0).all())
    _assert_within(got, ref, bound, f"spmm_sum D={D}")


# --------------------------------------------------------------------------
# C. gru_gates / gru_gates2
# --------------------------------------------------------------------------

def _gate_bounds(u, pre_r, pre_z, i_n, hn, h, dP_r, dP_z):
    """float64 gate outputs and their bounds (module docstring, C)."""
    r, z = torch.sigmoid(pre_r), torch.sigmoid(pre_z)
    n = torch.tanh(i_n + r * hn)
    hnew = (1 - z) * n + z * h
    e_r = EPS_FN + 0.25 * dP_r
    e_z = EPS_FN + 0.25 * dP_z
    e_n = EPS_FN + e_r * hn.abs() + 2 * ACC * (i_n.abs() + (r * hn).abs())
    e_h = (h - n).abs() * e_z + (1 - z) * e_n + 4 * ACC * (n.abs() + h.abs())
    ref = dict(r=r, z=z, n=n, h=hnew)
    bound = {k: SECOND * (u * ref[k].abs() + e) for k, e in
             (("r", e_r), ("z", e_z), ("n", e_n), ("h", e_h))}
    return ref, bound


def _gate_bwd_ref(u, go, h, r, z, n, hn):
    """float64 backward from the given saved activations, and T (docstring C)."""
    go, h, r, z, n, hn = (t.double() for t in (go, h, r, z, n, hn))
    dpn = go * (1 - z) * (1 - n * n)
    dpr = dpn * hn * r * (1 - r)
    dpz = go * (h - n) * z * (1 - z)
    T_dpn = go.abs() * (1 + z.abs()) * (1 + n * n)
    T_dpr = T_dpn * hn.abs() * r.abs() * (1 + r.abs())
    T_dpz = go.abs() * (h.abs() + n.abs()) * z.abs() * (1 + z.abs())
    ref = dict(dpr=dpr, dpz=dpz, dpn=dpn, dpnr=dpn * r, gh=go * z)
    T = dict(dpr=T_dpr, dpz=T_dpz, dpn=T_dpn, dpnr=T_dpn * r.abs(), gh=(go * z).abs())
    bound = {k: u * ref[k].abs() + 8 * ACC * T[k] for k in ref}
    return ref, bound


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("H", [64, 128])
@pytest.mark.parametrize("N", [1, 255, 257])
@pytest.mark.parametrize("kind", ["gru_gates", "gru_gates2"])
def test_gates_fwd_bwd(kind, N, H, dtype):
    ext = _ext()
    u = _u(dtype)
    gen = torch.Generator().manual_seed(1000 * N + H)

    def uni(cols, lim):  # an even spread over [-lim, lim], shuffled
        v = torch.linspace(-lim, lim, N * cols)[torch.randperm(N * cols, generator=gen)]
        return v.view(N, cols).to(dtype).to(DEV)

    h = torch.randn(N, H, generator=gen).to(dtype).to(DEV)
    go = (torch.randn(N, H, generator=gen) / 16).to(dtype).to(DEV)
    if kind == "gru_gates2":
        gicat = uni(4 * H, 12.0)
        g64 = gicat.double()
        pre_r, pre_z, i_n, hn = (g64[:, i * H:(i + 1) * H] for i in range(4))
        assert float(g64[:, :3 * H].abs().max()) > 11.0 and float(g64.abs().min()) < 0.5
        dP_r = dP_z = torch.zeros_like(pre_r)
        h_new, r, z, n, hn_out = ext.gru_gates2_fwd(gicat, h)
        assert torch.equal(hn_out, gicat[:, 3 * H:]), "HN must be the fourth block, unchanged"
        hn_saved = hn_out
    else:
        gi, gh = uni(3 * H, 6.0), uni(3 * H, 6.0)
        gi64, gh64 = gi.double(), gh.double()
        pre_r, pre_z = gi64[:, :H] + gh64[:, :H], gi64[:, H:2 * H] + gh64[:, H:2 * H]
        i_n, hn = gi64[:, 2 * H:], gh64[:, 2 * H:]
        assert float(gi64.abs().max()) == 6.0 and float(gh64.abs().max()) == 6.0
        dP_r = ACC * (gi64[:, :H].abs() + gh64[:, :H].abs())
        dP_z = ACC * (gi64[:, H:2 * H].abs() + gh64[:, H:2 * H].abs())
        h_new, r, z, n = ext.gru_gates_fwd(gi, gh, h)
        hn_saved = gh[:, 2 * H:].contiguous()
    ref, bound = _gate_bounds(u, pre_r, pre_z, i_n, hn, h.double(), dP_r, dP_z)
    for name, got in (("r", r), ("z", z), ("n", n), ("h", h_new)):
        assert got.dtype == dtype and got.shape == (N, H)
        _assert_within(got, ref[name], bound[name], f"{kind} fwd {name}")

    # backward, teacher-forced on the kernel's own saved activations
    bref, bbound = _gate_bwd_ref(u, go, h, r, z, n, hn_saved)
    if kind == "gru_gates2":
        ggic, gh_dir = ext.gru_gates2_bwd(go, h, r, z, n, hn_saved)
        assert ggic.shape == (N, 4 * H)
        blocks = {k: ggic[:, i * H:(i + 1) * H] for i, k in
                  enumerate(("dpr", "dpz", "dpn", "dpnr"))}
    else:
        ggi, ggh, gh_dir = ext.gru_gates_bwd(go, gh, h, r, z, n)
        assert ggi.shape == (N, 3 * H) and ggh.shape == (N, 3 * H)
        blocks = {"dpr": ggi[:, :H], "dpz": ggi[:, H:2 * H], "dpn": ggi[:, 2 * H:],
                  "dpnr": ggh[:, 2 * H:]}
        assert torch.equal(ggh[:, :2 * H], ggi[:, :2 * H])
    blocks["gh"] = gh_dir
    for name, got in blocks.items():
        _assert_within(got, bref[name], bbound[name], f"{kind} bwd {name}")
    # the r factor of the fourth block must be visible above the bound
    sep = (bref["dpn"] - bref["dpnr"]).abs() - bbound["dpn"] - bbound["dpnr"]
    assert float(sep.max()) > 0.0


# --------------------------------------------------------------------------
# D. fused forward, teacher-forced per step
# --------------------------------------------------------------------------

@pytest.mark.parametrize("name,H,S", FWD_CASES)
def test_fused_fwd_teacher_forced(name, H, S):
    c = _case(name, H)
    f = _run(name, H, S)["f"] if (name, H, S) in LOOP_CASES else _fwd(c, S)
    N, deg = c["N"], c["deg"]
    for k in FWD_NAMES[1:]:
        want = (S + 1 if k == "HH" else S, N, H)
        assert tuple(f[k].shape) == want and f[k].dtype == torch.bfloat16, k
    assert torch.equal(f["HH"][0], c["x"]), "HH[0] must be x bit-for-bit"
    assert torch.equal(f["h_final"], f["HH"][S])
    for s in range(S):
        st = O.step_exact(f["HH"][s], f["M"][s], c["g"], *c["w64"])
        what = f"{name} H={H} step {s}"
        m_bound = SECOND * (U16 * st["m_abs"] + (H + 1) * ACC * st["m_wh_abs"]
                            + deg[:, None] * ACC * st["m_abs"]) + U16 * st["m"].abs()
        if c["info"]["zero_in"]:
            zi = torch.tensor(c["info"]["zero_in"], device=DEV)
            assert bool((f["M"][s][zi] == 0).all()) and bool((m_bound[zi] == 0).all())
        _assert_within(f["M"][s], st["m"], m_bound, what + " M")

        dP = {k: (2 * H + 1) * ACC * st[k + "_abs"] for k in ("pre_r", "pre_z", "pre_in", "hn")}
        _assert_within(f["HN"][s], st["hn"], SECOND * (U16 * st["hn"].abs() + dP["hn"]),
                       what + " HN")
        r, z, n, hn = st["r"], st["z"], st["n"], st["hn"]
        e_r = EPS_FN + 0.25 * dP["pre_r"]
        e_z = EPS_FN + 0.25 * dP["pre_z"]
        e_n = (EPS_FN + dP["pre_in"] + e_r * hn.abs() + dP["hn"]
               + 2 * ACC * (st["pre_in"].abs() + (r * hn).abs()))
        h = f["HH"][s].double()
        e_h = (h - n).abs() * e_z + (1 - z) * e_n + 4 * ACC * (n.abs() + h.abs())
        for key, ref, e in (("R", r, e_r), ("Z", z, e_z), ("Nn", n, e_n),
                            ("HH", st["h_new"], e_h)):
            got = f[key][s + 1] if key == "HH" else f[key][s]
            _assert_within(got, ref, SECOND * (U16 * ref.abs() + e), f"{what} {key}")


# --------------------------------------------------------------------------
# E. whole loop and backward, 4x rule
# --------------------------------------------------------------------------

def _ratios(got, exact, emu, names, tag):
    out = {}
    for k in names:
        ek, ee = O.rel_l2(got[k], exact[k]), O.rel_l2(emu[k], exact[k])
        out[k] = (ek, ee)
        print(f"[ratio] {tag} {k}: err_kernel {ek:.3e} err_emulated {ee:.3e} "
              f"ratio {ek / ee:.3f}")
    return out


@pytest.mark.parametrize("name,H,S", LOOP_CASES)
def test_fused_loop_4x(name, H, S):
    run = _run(name, H, S)
    got = dict(run["b"], h_final=run["f"]["h_final"])
    for k in WGRADS:
        assert got[k].dtype == torch.float32, k
    assert got["grad_x"].dtype == torch.bfloat16
    assert tuple(got["gW_ih"].shape) == (3 * H, H) and tuple(got["gW_hh"].shape) == (3 * H, H)
    assert tuple(got["gW_e"].shape) == (H, H) and got["gb_e"].numel() == H
    res = _ratios(got, run["exact"], run["emu"], O.OUT_NAMES, f"{name} H={H} S={S}")
    for k, (ek, ee) in res.items():
        assert 0.0 < ee < 0.1, (k, ee)
        assert ek <= 4.0 * ee, (k, ek, ee)
    # r/z gates add b_ih and b_hh: one column sum feeds both
    assert torch.equal(got["gb_ih"][:2 * H], got["gb_hh"][:2 * H])


@pytest.mark.parametrize("H", [64, 128])
def test_fused_bwd_no_leak_between_blocks(H):
    """With S = 1 and the upper half of x's columns zero, every product
    against those h columns is exactly 0: gW_hh[:, H/2:] and gW_e[:, H/2:]
    must be exact zeros, while the same columns of gW_ih (products against
    m, which is dense) are not. gWcat's [2H,3H) x h block (dpn^T h, non-zero
    in the lower columns) has no place in the returned (3H, H) layouts: the
    n_h rows of gW_hh must carry (dpn r)^T h, checked by the 4x rule."""
    c = dict(_case("small", H))
    x = c["x"].clone()
    x[:, H // 2:] = 0
    c["x"] = x
    f = _fwd(c, 1)
    b = dict(zip(BWD_NAMES, _bwd(c, f, 1)))
    assert bool((b["gW_hh"][:, H // 2:] == 0).all())
    assert bool((b["gW_e"][:, H // 2:] == 0).all())
    assert bool((b["gW_ih"][:, H // 2:] != 0).any(0).all())
    assert float(b["gW_hh"][:, :H // 2].abs().max()) > 0
    exact = O.ggnn_exact(x, c["g"], *c["w64"], 1, grad_out=c["go"])
    emu = O.ggnn_emulated(x, c["g"], *c["w64"], 1, grad_out=c["go"])
    for k in ("gW_hh", "gW_ih", "gW_e"):
        assert O.rel_l2(b[k], exact[k]) <= 4.0 * O.rel_l2(emu[k], exact[k]), k


# --------------------------------------------------------------------------
# F. direct accumulation into live views
# --------------------------------------------------------------------------

@pytest.mark.parametrize("name,H,S", DIRECT_CASES)
def test_fused_bwd_direct_accumulate(name, H, S):
    run = _run(name, H, S)
    c, f, G, emu_abs = run["c"], run["f"], run["b"], run["emu"]["abs"]
    N = c["N"]
    shapes = {"gW_e": (H, H), "gb_e": (H,), "gW_ih": (3 * H, H), "gW_hh": (3 * H, H),
              "gb_ih": (3 * H,), "gb_hh": (3 * H,)}
    total = sum(torch.Size(s).numel() for s in shapes.values())
    gen = torch.Generator().manual_seed(5)
    # one flat buffer, one leading element: every view sits at an odd
    # element offset (4-byte aligned only), as a flat optimizer's would
    flat = (0.25 * torch.randn(1 + total + 1, generator=gen)).to(DEV)
    flat0 = flat.clone()
    views, off = {}, 1
    for k, s in shapes.items():
        n = torch.Size(s).numel()
        views[k] = flat[off:off + n].view(s)
        assert views[k].data_ptr() % 8 == 4
        off += n
    assert off == 1 + total
    g0 = {k: v.double().clone() for k, v in views.items()}
    for times in (1, 2):
        outs = _bwd(c, f, S, out_we=views["gW_e"], out_be=views["gb_e"],
                    gru_outs=[views["gW_ih"], views["gW_hh"], views["gb_ih"], views["gb_hh"]])
        assert torch.equal(outs[0], G["grad_x"]), "grad_x must not depend on the grad sink"
        for k in WGRADS:
            ref = g0[k] + times * G[k].double()
            bound = S * N * ACC * (g0[k].abs() + times * emu_abs[k])
            _assert_within(views[k], ref, bound, f"{name} H={H} direct x{times} {k}")
    # nothing outside the views was touched
    assert flat[0] == flat0[0] and flat[-1] == flat0[-1]


# --------------------------------------------------------------------------
# G. module level at H != 128
# --------------------------------------------------------------------------

@pytest.mark.parametrize("H", [64, 192])
def test_module_fused_path_other_widths(H):
    from deepdfa_amd.models.flow_gnn import GatedGraphConv

    S = 2
    run = _run("small", H, S)
    c = run["c"]
    conv = GatedGraphConv(H, H, S).to(DEV)
    with torch.no_grad():
        for p, v in zip((conv.linear.weight, conv.linear.bias, conv.gru.weight_ih,
                         conv.gru.weight_hh, conv.gru.bias_ih, conv.gru.bias_hh), c["params"]):
            p.copy_(v)
    x = c["x"].float().requires_grad_(True)
    with torch.autocast(device_type="cuda", dtype=torch.bfloat16):
        out = conv(c["g"], x)
    assert out.dtype == torch.bfloat16, "the fused path must engage"
    assert torch.equal(out, run["f"]["h_final"])
    (out.float() * c["go"].float()).sum().backward()
    grads = {"gW_e": conv.linear.weight.grad, "gb_e": conv.linear.bias.grad,
             "gW_ih": conv.gru.weight_ih.grad, "gW_hh": conv.gru.weight_hh.grad,
             "gb_ih": conv.gru.bias_ih.grad, "gb_hh": conv.gru.bias_hh.grad,
             "grad_x": x.grad}
    for k, gk in grads.items():
        assert gk is not None and bool(torch.isfinite(gk).all()), k
        assert bool((gk != 0).any()), k
    res = _ratios(grads, run["exact"], run["emu"], O.GRAD_NAMES, f"module H={H} S={S}")
    for k, (ek, ee) in res.items():
        assert ek <= 4.0 * ee, (k, ek, ee)
    gW, exact, emu = grads["gW_e"], run["exact"]["gW_e"], run["emu"]["gW_e"]
    assert bool((gW != 0).any(1).all()) and bool((gW != 0).any(0).all()), "empty row/col"
    if H > 128:  # the region the 128x128-tile kernel never reached
        for sl in ((slice(128, H), slice(None)), (slice(None), slice(128, H))):
            assert O.rel_l2(gW[sl], exact[sl]) <= 4.0 * O.rel_l2(emu[sl], exact[sl])
        assert bool((grads["gb_e"][128:] != 0).all())


# --------------------------------------------------------------------------
# H. gemm_bias on the 64-row tile
# --------------------------------------------------------------------------

@pytest.mark.parametrize("with_addend", [False, True])
@pytest.mark.parametrize("N,K,COL", [(6145, 256, 512), (24577, 128, 128)])
def test_gemm_bias_64row_tile(N, K, COL, with_addend):
    assert ((N + 63) // 64) * (COL // 128) >= 384 and N % 64 == 1
    gen = torch.Generator().manual_seed(N)
    bf = torch.bfloat16
    A = torch.randn(N, K, generator=gen).to(bf).to(DEV)
    W = (0.1 * torch.randn(COL, K, generator=gen)).to(bf).to(DEV)
    b = torch.randn(COL, generator=gen).to(bf).to(DEV)
    add = torch.randn(N, COL, generator=gen).to(bf).to(DEV) if with_addend else None
    got = _ext().gemm_bias(A, W, b, add)
    ref = A.double() @ W.double().t() + b.double()
    mag = A.double().abs() @ W.double().abs().t() + b.double().abs()
    if with_addend:
        ref = ref + add.double()
        mag = mag + add.double().abs()
    bound = SECOND * (U16 * ref.abs() + (K + 2) * ACC * mag)
    _assert_within(got, ref, bound, f"gemm_bias {N}x{K}x{COL}")
