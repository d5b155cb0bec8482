"""The one-launch GGNN weight-grad kernel (csrc/ggnn_wgrad.hip) against
float64 products of the same bf16 inputs, through the raw binding
ext.ggnn_wgrad, and old against new through ggnn_fused_bwd.

With K = S N rows, r | z | gi_n | gh_n the four H-wide column blocks of
Ggicat, and HH the first S slabs of the hidden states:

  gW_ih = [r|z|gi_n]^T M      gb_ih = colsum [r|z|gi_n]
  gW_hh = [r|z|gh_n]^T HH     gb_hh = colsum [r|z|gh_n]
  gW_e  = Gwh^T HH            gb_e  = colsum Gwh

Bounds come from the inputs and the float64 reference only, in the form of
test_gpu_ggnn.py (ACC = 2^-23 per accumulated term, a 2x margin over
sequential fp32 summation; the bf16 products are exact in fp32):

  returned form   |got - ref| <= K 2^-23 sum_k |a_k b_k|
  direct form     |got - (g0 + t ref)| <= K 2^-23 (|g0| + t sum_k |a_k b_k|)

with b_k = 1 for the bias sums. The kernel adds K-chunk partial sums with
atomics: at most K/64 + 1 of them whatever the chunk, so K terms cover any
chunking and any order.

  1  raw kernel, both output forms, K below / at / past a slice and a chunk
  2  nothing at or beyond row S N is read (NaN behind every operand)
  3  dead tiles stay dead, live tiles go to their own views
  4  direct accumulation into views at odd element offsets, guards intact
  5  ggnn_fused_bwd: fused_wgrad=True against False, rule E of
     test_gpu_ggnn.py (relative L2 error against ggnn_exact at most 4x that
     of ggnn_emulated), grad_x bit-equal
"""

import pytest
import torch

import ggnn_oracle as O
from oracle_checks import assert_within

pytestmark = pytest.mark.gpu

ACC = 2.0 ** -23
DEV = "cuda:0"
H = 128
NAMES = ("gW_ih", "gW_hh", "gb_ih", "gb_hh", "gW_e", "gb_e")
SHAPES = {"gW_ih": (3 * H, H), "gW_hh": (3 * H, H), "gb_ih": (3 * H,), "gb_hh": (3 * H,),
          "gW_e": (H, H), "gb_e": (H,)}


def _ext():
    from deepdfa_amd.ops import load_ext

    return load_ext(required=True)


# --------------------------------------------------------------------------
# inputs and float64 references, built once per (S, N) and never modified
# --------------------------------------------------------------------------

_INPUTS = {}


def make_inputs(S, N, dev):
    """Random bf16 operands of the training magnitudes: gradients about
    1/16, activations about 1. Each has one extra NaN row (HH: one NaN slab)
    right behind row S N, which is where the loop's own buffers end or go on."""
    gen = torch.Generator().manual_seed(1000 * S + N)
    K = S * N

    def rows(cols, scale):
        t = torch.full((K + 1, cols), float("nan"))
        t[:K] = scale * torch.randn(K, cols, generator=gen)
        return t.to(torch.bfloat16).to(dev)

    gg, m, gwh = rows(4 * H, 1 / 16), rows(H, 1.0), rows(H, 1 / 16)
    hh = torch.full((S + 1, N, H), float("nan"))
    hh[:S] = torch.randn(S, N, H, generator=gen)
    return dict(S=S, N=N, K=K, gg_flat=gg, m_flat=m, gwh_flat=gwh,
                Ggicat=gg[:K].view(S, N, 4 * H), M=m[:K].view(S, N, H),
                Gwh=gwh[:K].view(S, N, H), HH=hh.to(torch.bfloat16).to(dev))


def reference(inp):
    """float64 products and the per-element sum_k |a_k b_k| of the bound."""
    K = inp["K"]
    gg = inp["Ggicat"].reshape(K, 4 * H).double()
    m = inp["M"].reshape(K, H).double()
    hh = inp["HH"][:inp["S"]].reshape(K, H).double()
    gwh = inp["Gwh"].reshape(K, H).double()
    a_ih = gg[:, :3 * H]
    a_hh = torch.cat([gg[:, :2 * H], gg[:, 3 * H:]], 1)
    ref = {"gW_ih": a_ih.t() @ m, "gW_hh": a_hh.t() @ hh, "gb_ih": a_ih.sum(0),
           "gb_hh": a_hh.sum(0), "gW_e": gwh.t() @ hh, "gb_e": gwh.sum(0)}
    mag = {"gW_ih": a_ih.abs().t() @ m.abs(), "gW_hh": a_hh.abs().t() @ hh.abs(),
           "gb_ih": a_ih.abs().sum(0), "gb_hh": a_hh.abs().sum(0),
           "gW_e": gwh.abs().t() @ hh.abs(), "gb_e": gwh.abs().sum(0)}
    return ref, mag


def _inputs(S, N):
    if (S, N) not in _INPUTS:
        inp = make_inputs(S, N, DEV)
        inp["ref"], inp["mag"] = reference(inp)
        _INPUTS[(S, N)] = inp
    return _INPUTS[(S, N)]


def _call(inp, views=None, **kw):
    direct = {}
    if views is not None:
        direct = dict(out_we=views["gW_e"], out_be=views["gb_e"],
                      gru_outs=[views[k] for k in ("gW_ih", "gW_hh", "gb_ih", "gb_hh")])
    outs = _ext().ggnn_wgrad(inp["Ggicat"], inp["M"], inp["HH"], inp["Gwh"], inp["S"],
                             **direct, **kw)
    return dict(zip(NAMES, outs))


def _chunk():
    """The launcher's own chunk length for a short K (its rule lengthens the
    chunks only once K / chunk exceeds what the chip can hold at once)."""
    L = int(_ext().ggnn_wgrad_kchunk(1))
    assert L > 0 and L % 64 == 0
    return L


def _flat_views(seed):
    """One flat fp32 buffer with a guard element at each end; every view at
    an odd element offset (4-byte aligned only), as a flat optimizer's."""
    total = sum(torch.Size(s).numel() for s in SHAPES.values())
    gen = torch.Generator().manual_seed(seed)
    flat = (0.25 * torch.randn(1 + total + 1, generator=gen)).to(DEV)
    views, off = {}, 1
    for k, s in SHAPES.items():
        n = torch.Size(s).numel()
        views[k] = flat[off:off + n].view(s)
        assert views[k].data_ptr() % 8 == 4
        off += n
    assert off == 1 + total
    return flat, views


def _check_both_forms(inp, tag):
    K, ref, mag = inp["K"], inp["ref"], inp["mag"]
    got = _call(inp)
    for k in NAMES:
        assert got[k].dtype == torch.float32 and tuple(got[k].shape) == SHAPES[k], k
        assert_within(got[k], ref[k], K * ACC * mag[k], f"{tag} returned {k}")
    # r/z gates add b_ih and b_hh: one accumulated column sum feeds both
    assert torch.equal(got["gb_ih"][:2 * H], got["gb_hh"][:2 * H])
    flat, views = _flat_views(seed=K)
    flat0 = flat.clone()
    g0 = {k: v.double().clone() for k, v in views.items()}
    _call(inp, views)
    for k in NAMES:
        assert_within(views[k], g0[k] + ref[k], K * ACC * (g0[k].abs() + mag[k]),
                      f"{tag} direct {k}")
    assert flat[0] == flat0[0] and flat[-1] == flat0[-1]


# --------------------------------------------------------------------------
# 1. raw kernel against the float64 product
# --------------------------------------------------------------------------

@pytest.mark.parametrize("S,N", [(1, 7), (1, 64), (2, 33), (3, 257)])
def test_raw_slices(S, N):
    _check_both_forms(_inputs(S, N), f"S={S} N={N}")


@pytest.mark.parametrize("case", ["one_chunk", "one_chunk_plus_1", "three_chunks_minus_1"])
def test_raw_chunks(case):
    L = _chunk()
    N = {"one_chunk": L, "one_chunk_plus_1": L + 1, "three_chunks_minus_1": 3 * L - 1}[case]
    assert int(_ext().ggnn_wgrad_kchunk(N)) == L  # K = N rows really are cut at L
    _check_both_forms(_inputs(1, N), f"{case} K={N}")


# --------------------------------------------------------------------------
# 2. nothing beyond S N is read
# --------------------------------------------------------------------------

@pytest.mark.parametrize("S,N", [(2, 33), (3, 257)])
def test_rows_beyond_K_not_read(S, N):
    inp = _inputs(S, N)
    K = inp["K"]
    # the NaN row / slab sits right behind the rows the kernel may read
    assert bool(torch.isnan(inp["HH"][S]).all())
    for flat, view in (("gg_flat", "Ggicat"), ("m_flat", "M"), ("gwh_flat", "Gwh")):
        assert bool(torch.isnan(inp[flat][K]).all())
        assert inp[view].data_ptr() == inp[flat].data_ptr()
        assert bool(torch.isfinite(inp[view].float()).all())
    got = _call(inp)
    for k in NAMES:
        assert_within(got[k], inp["ref"][k], K * ACC * inp["mag"][k], f"S={S} N={N} nan-guard {k}")


# --------------------------------------------------------------------------
# 3. dead tiles stay dead, live tiles stay apart
# --------------------------------------------------------------------------

def test_dead_tiles_and_routing():
    base = _inputs(3, 257)
    S = base["S"]
    hh = base["HH"].clone()
    hh[:S, :, H // 2:] = 0
    got = _call(dict(base, HH=hh))
    assert bool((got["gW_hh"][:, H // 2:] == 0).all())
    assert bool((got["gW_e"][:, H // 2:] == 0).all())
    assert bool((got["gW_ih"][:, H // 2:] != 0).any(0).all())
    assert float(got["gW_hh"][:, :H // 2].abs().max()) > 0

    for dead, live in ((2, 3), (3, 2)):  # column blocks of Ggicat: 2 = gi_n, 3 = gh_n
        gg = base["Ggicat"].clone()
        gg[:, :, dead * H:(dead + 1) * H] = 0
        got = _call(dict(base, Ggicat=gg))
        zero_w, zero_b = ("gW_ih", "gb_ih") if dead == 2 else ("gW_hh", "gb_hh")
        live_w, live_b = ("gW_hh", "gb_hh") if dead == 2 else ("gW_ih", "gb_ih")
        assert bool((got[zero_w][2 * H:] == 0).all()), (dead, zero_w)
        assert bool((got[zero_b][2 * H:] == 0).all()), (dead, zero_b)
        assert bool((got[live_w][2 * H:] != 0).any()), (dead, live_w)
        assert bool((got[live_b][2 * H:] != 0).any()), (dead, live_b)
        # the r/z rows and W_e do not depend on either n block
        for k in ("gW_e", "gb_e"):
            assert_within(got[k], base["ref"][k], base["K"] * ACC * base["mag"][k], f"dead={dead} {k}")
        for k in ("gW_ih", "gW_hh", "gb_ih", "gb_hh"):
            assert_within(got[k][:2 * H], base["ref"][k][:2 * H],
                          base["K"] * ACC * base["mag"][k][:2 * H], f"dead={dead} {k}[:2H]")


# --------------------------------------------------------------------------
# 4. direct accumulation, once and twice
# --------------------------------------------------------------------------

def test_direct_accumulate_twice():
    L = _chunk()
    for inp in (_inputs(3, 257), _inputs(1, L + 1)):
        K, ref, mag = inp["K"], inp["ref"], inp["mag"]
        flat, views = _flat_views(seed=7)
        flat0 = flat.clone()
        g0 = {k: v.double().clone() for k, v in views.items()}
        for times in (1, 2):
            _call(inp, views)
            for k in NAMES:
                assert_within(views[k], g0[k] + times * ref[k],
                              K * ACC * (g0[k].abs() + times * mag[k]),
                              f"K={K} direct x{times} {k}")
        assert flat[0] == flat0[0] and flat[-1] == flat0[-1]


# --------------------------------------------------------------------------
# 5. old against new through ggnn_fused_bwd
# --------------------------------------------------------------------------

@pytest.mark.parametrize("name,Hc,S", [("small", 128, 2), ("n6081", 128, 2), ("small", 64, 2)])
def test_fused_bwd_old_against_new(name, Hc, S):
    import test_gpu_ggnn as T  # its cases and both oracles, built once per session

    run = T._run(name, Hc, S)
    c, f = run["c"], run["f"]
    names = T.BWD_NAMES
    new = dict(zip(names, T._bwd(c, f, S, fused_wgrad=True)))
    old = dict(zip(names, T._bwd(c, f, S, fused_wgrad=False)))
    assert torch.equal(new["grad_x"], old["grad_x"])
    for tag, got in (("new", new), ("old", old)):
        for k in T.WGRADS:
            ek = O.rel_l2(got[k], run["exact"][k])
            ee = O.rel_l2(run["emu"][k], run["exact"][k])
            print(f"[ratio] {name} H={Hc} S={S} {tag} {k}: err_kernel {ek:.3e} "
                  f"err_emulated {ee:.3e} ratio {ek / ee:.3f}")
            assert 0.0 < ee < 0.1, (tag, k, ee)
            assert ek <= 4.0 * ee, (tag, k, ek, ee)
        assert torch.equal(got["gb_ih"][:2 * Hc], got["gb_hh"][:2 * Hc]), tag
