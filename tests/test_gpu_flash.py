"""Flash attention (csrc/flash_attn.hip: forward, Dterm, dq, dkv) against the
float64 oracles of tests/flash_oracle.py.

Every reference is float64 on the GPU, computed from the SAME values the
kernels see: q, k, v, dO are bf16 tensors, the bias an fp32 tensor. Every
bound is computed from those inputs and the references, never from a kernel
output. u = 2^-8 is the bf16 unit roundoff, 2^-23 per accumulated term twice
the fp32 one, eps_fn = 2^-20 covers an fp32 __expf / division / the fp32
value of dscale (a few ulp of a value <= 1, as in test_gpu_ggnn.py).

Shapes: d = 64; L = 64 (one KV tile, half-empty query block), 128, 192 (a
full and a partial query block, three KV tiles = both buffer parities), 320
(three query blocks, five tiles); (B, H) = (3, 3), so gridDim.x * H is no
multiple of 8 in the (b, h, tile) decode, and one (2, 12) case. `valid` takes
L, L-1, 65, 64, 63, 1, 0 and None across the cases; valid = 1 only in dropout
cases (without dropout a one-key softmax makes dQ, dK, dBias cancel to
exactly 0 in float64, where the kernel keeps its fp32 summation noise and no
relative rule is defined). Scores are peaked: q, k ~ 0.5 N(0,1) at scale 1
(T5's), |k| rising or falling with the key index in some cases so the running
max moves in every tile, scale = 1/8 in others; the bias is random, hence
asymmetric.

A  forward O, every element, every query row (the kernel masks keys only, so
   padded query rows are defined):
     |got - ref| <= (1 + 2^-7) [ u |ref|
                     + sum_k (u + 3 eps_fn + d_k + d_row + (L+2) 2^-23) Pd_k |v_k| ]
     d_k   = (64+2) 2^-23 (scale sum_d |q k| + |bias|) + 2^-23 |s_k - m|
     d_row = sum_k P_k d_k
   The kernel rounds the unnormalised e_k keep dscale to bf16 (u, relative:
   the running max only rescales by powers the numerator and the denominator
   share, because the SAME fp32 alpha multiplies o_acc and l), accumulates
   e_k v_k over L keys in fp32 ((L+2) 2^-23 with the alpha products), and
   rounds O = o_acc / l once (u |ref|). d_k is the error of exp(s_k - m_t):
   the fp32 score (64 products, the scale and the bias add) and the rounding
   of the subtraction, |s_k - m_t| <= |s_k - m| for every running max m_t;
   d_row is the same error in l. 3 eps_fn: __expf, the division, dscale.
B  lse against float64. Yardstick: the same log-sum-exp evaluated in fp32 by
   torch from the same inputs; y = max_rows |lse_fp32 - lse_f64|. The kernel
   must stay within LSE_MARGIN * y (see the table below for what it does).
   Rows with no unmasked key: lse == 0 and O == 0 exactly.
C  forward and backward by the emulation rule, error = L2 distance to
   attn_exact:
     err_kernel <= 4 err_emulated     O, dQ, dK, dV, dBias   whole tensor
     err_kernel <= 4 err_emulated     O, dQ, dK, dV          per (b, h, 64-row tile)
     err_kernel <= 4 err_emulated     dBias                  per (h, 64-key block)
     exactly 0                        every tile that is 0 by structure: dK/dV
                                      of key tiles >= valid[b], everything of a
                                      valid = 0 batch row, dBias key blocks no
                                      batch row reaches
   4 is the margin of test_gpu_ggnn.py / test_gpu_graph_head.py. The outputs
   come from at::empty; NaN-filled tensors of the output sizes are allocated
   and freed just before each call so a skipped store shows.
D  dropout: the keep mask is recovered from the forward kernel
   (flash_oracle.recover_keep) and A and C run with it at p = 0.1: forward, dq
   and dkv each rebuild the mask in their own lane layout, so a disagreement
   fails C. Mask properties: same seed -> same mask, other seed -> other mask,
   keep fraction within 6 sigma of 231/256, agreement between neighbouring
   (b, h) and between neighbouring query rows within 6 sigma of
   p^2 + (1-p)^2.
E  layouts, bit-exact at the binding level: fused_grads on slices of one
   (B, L, 3D) buffer and kv_fused on a (B, L, 2D) buffer equal the plain path.
F  dbias_accum pre-filled with g0, t = 2 calls:
     |got - (g0 + t G)| <= (t B + 1) 2^-23 (|g0| + t sum_b |dS_b|).

err_kernel / err_emulated observed on an MI355X, whole tensor (largest tile),
and err_kernel / err_fp32 for lse:
  case                             O             dQ            dK            dV            dBias         lse
  L192-none                        0.778 (0.861) 0.927 (1.063) 0.941 (1.028) 1.000 (1.001) -             1.410
  L192-none-drop                   0.885 (0.959) 0.986 (1.190) 0.991 (1.346) 1.000 (1.000) -             0.889
  L192-none-bias                   0.781 (0.842) 0.876 (1.216) 0.870 (1.160) 1.000 (1.000) 0.816 (0.870) 1.437
  L192-none-bias-drop              0.828 (0.897) 0.844 (1.100) 0.841 (1.396) 1.000 (1.000) 0.803 (1.234) 1.149
  L192-valid                       0.799 (0.859) 0.932 (1.119) 0.946 (1.036) 1.000 (1.000) -             0.749
  L192-valid-drop                  0.970 (1.000) 0.997 (1.172) 0.996 (1.145) 1.000 (1.001) -             0.851
  L192-valid-bias                  0.779 (0.844) 0.893 (1.164) 0.901 (1.106) 1.000 (1.001) 0.719 (1.670) 1.426
  L192-valid-bias-drop             0.963 (1.000) 0.992 (1.105) 0.995 (2.297) 1.000 (1.000) 0.991 (1.293) 0.916
  L192-causal                      0.923 (1.004) 0.968 (1.075) 0.949 (1.049) 1.000 (1.002) -             1.157
  L192-causal-drop                 0.952 (1.019) 0.965 (1.015) 0.954 (1.020) 1.000 (1.000) -             1.168
  L192-causal-bias                 0.785 (0.841) 0.900 (1.072) 0.908 (1.112) 1.000 (1.003) 0.763 (1.254) 1.000
  L192-causal-bias-drop            0.872 (0.981) 0.931 (1.177) 0.928 (1.349) 1.000 (1.000) 0.869 (1.071) 1.049
  L192-valid+causal                0.790 (0.877) 0.879 (1.063) 0.877 (1.225) 1.000 (1.000) -             0.834
  L192-valid+causal-drop           0.953 (1.000) 0.982 (1.420) 0.988 (1.379) 1.000 (1.000) -             1.000
  L192-valid+causal-bias           0.769 (0.829) 0.852 (1.059) 0.870 (1.206) 1.000 (1.000) 0.774 (1.373) 0.845
  L192-valid+causal-bias-drop      0.849 (0.928) 0.882 (1.077) 0.887 (1.148) 1.000 (1.000) 0.851 (1.112) 0.775
  L64-none                         0.810 (0.859) 0.936 (1.073) 0.918 (1.050) 1.000 (1.000) -             1.000
  L64-valid+causal-bias-drop       0.946 (1.000) 0.974 (1.045) 0.971 (1.017) 1.000 (1.000) 0.956 (0.994) 0.477
  L64-valid-bias                   0.792 (0.821) 0.925 (1.027) 0.927 (0.995) 1.000 (1.000) 0.756 (0.803) 0.802
  L128-none                        0.984 (1.008) 1.003 (1.021) 1.000 (1.020) 1.000 (1.001) -             1.174
  L128-valid+causal-bias-drop      0.824 (0.859) 0.806 (1.077) 0.825 (1.053) 1.000 (1.000) 0.768 (1.008) 0.582
  L128-H12-valid+causal-bias-drop  0.867 (0.955) 0.959 (1.323) 0.968 (1.343) 1.000 (1.000) 0.940 (1.672) 1.000
  L320-none                        0.770 (0.825) 0.822 (1.190) 0.830 (2.785) 1.000 (1.002) -             0.855
  L320-valid+causal-bias-drop      0.850 (0.958) 0.849 (1.082) 0.874 (1.328) 1.000 (1.013) 0.814 (0.961) 0.711
  L320-valid-bias                  0.786 (0.859) 0.900 (1.073) 0.918 (1.045) 1.000 (1.000) 0.706 (0.967) 1.165
Whole tensors lie between 0.70 and 1.01 and tiles below 1.7, except two dK
tiles. L320-none dK (b, h, tile) = (2, 2, 1) at 2.785: a float64 emulation
that rounds the unnormalised exp(s - m_t) per 64-key tile, as the kernel's
online softmax does, instead of the normalised P gives 2.785 on the same
tile on the CPU; the tile's reference norm is a third of the median one and
its error is dominated by the different rounding realisation of O in
D = sum dO O. L192-valid-bias-drop dK (0, 2, 1) at 2.297 holds one valid
key (valid = 65); the same emulation with the recovered mask gives 2.297
there as well. The kernel follows its own rounding order to three digits in
both; neither is a reason to move the 4.
lse: the kernel is within 0.48 .. 1.44 of the fp32 yardstick (about 1e-6
absolute). Both are fp32 evaluations of one expression, each error the
maximum over a few thousand rows of a few ulp of |lse|, so the ratio of the
two maxima scatters around 1; __expf / __logf are good to 2 ulp where libm is
to 1, and the kernel sums l in MFMA lane order. LSE_MARGIN = 4, the margin
used everywhere else here, leaves 2.8x over the largest ratio seen, while any
structural defect (a missed tile, a wrong max, a bias or mask slip) moves lse
by 1e-3 or more.
A: the largest |err| / bound per case lies between 0.31 and 0.84.
"""

import math

import pytest
import torch

import flash_oracle as FO

pytestmark = pytest.mark.gpu

bf = torch.bfloat16
U16 = 2.0 ** -8
ACC = 2.0 ** -23
EPS_FN = 2.0 ** -20
SECOND = 1.0 + 2.0 ** -7
LSE_MARGIN = 4.0
DEV = "cuda:0"
P_DROP = 0.1
TILE = 64


def _ext():
    from deepdfa_amd.ops import load_ext

    return load_ext(required=True)


# --------------------------------------------------------------------------
# cases, built once and never modified
# --------------------------------------------------------------------------

def _spec(L, mode, bias, p, valid=None, B=3, H=3, scale=1.0, kshape="flat"):
    assert ("valid" in mode) == (valid is not None)
    return dict(L=L, B=B, H=H, valid=valid, causal="causal" in mode, bias=bias, p=p,
                scale=scale, kshape=kshape)


def _matrix_192():
    """{none, valid, causal, valid+causal} x {no bias, bias} x {p = 0, 0.1}."""
    valids = {  # (mode, bias, dropout) -> valid; valid = 1 only with dropout
        ("valid", 0, 0): [192, 65, 0], ("valid", 1, 0): [191, 64, 63],
        ("valid", 0, 1): [63, 192, 1], ("valid", 1, 1): [65, 1, 191],
        ("valid+causal", 0, 0): [191, 63, 64], ("valid+causal", 1, 0): [0, 192, 65],
        ("valid+causal", 0, 1): [64, 1, 192], ("valid+causal", 1, 1): [192, 77, 0],
    }
    out = {}
    for mode in ("none", "valid", "causal", "valid+causal"):
        for b in (0, 1):
            for d in (0, 1):
                name = f"L192-{mode}{'-bias' if b else ''}{'-drop' if d else ''}"
                extra = {}
                if mode == "causal" and not b:
                    extra["scale"] = 0.125
                if mode == "valid+causal" and b:
                    extra["kshape"] = "rise"
                if mode == "none" and b:
                    extra["kshape"] = "fall"
                out[name] = _spec(192, mode, bool(b), P_DROP * d, valids.get((mode, b, d)), **extra)
    return out


SPECS = _matrix_192()
SPECS.update({
    "L64-none": _spec(64, "none", False, 0.0),
    "L64-valid+causal-bias-drop": _spec(64, "valid+causal", True, P_DROP, [64, 63, 1]),
    "L64-valid-bias": _spec(64, "valid", True, 0.0, [63, 0, 64]),
    "L128-none": _spec(128, "none", False, 0.0, scale=0.125),
    "L128-valid+causal-bias-drop": _spec(128, "valid+causal", True, P_DROP, [127, 65, 0],
                                         kshape="fall"),
    "L128-H12-valid+causal-bias-drop": _spec(128, "valid+causal", True, P_DROP, [128, 64],
                                             B=2, H=12),
    "L320-none": _spec(320, "none", False, 0.0, kshape="rise"),
    "L320-valid+causal-bias-drop": _spec(320, "valid+causal", True, P_DROP, [320, 65, 319],
                                         kshape="rise"),
    "L320-valid-bias": _spec(320, "valid", True, 0.0, [319, 0, 129]),
})
ALL = list(SPECS)
BIAS_CASES = [n for n in ALL if SPECS[n]["bias"]]

_RUNS = {}


def _poison(*shapes_dtypes):
    """Allocate, NaN-fill and free tensors of the coming outputs' sizes: the
    caching allocator hands the same blocks to the kernel's at::empty."""
    ts = [torch.full(s, float("nan"), dtype=dt, device=DEV) for s, dt in shapes_dtypes]
    torch.cuda.synchronize()
    del ts


def _inputs(name):
    s = SPECS[name]
    B, H, L = s["B"], s["H"], s["L"]
    g = torch.Generator().manual_seed(1000 + ALL.index(name))
    mk = lambda sc: torch.randn(B, L, H * 64, generator=g) * sc  # noqa: E731
    q, k, v, dO = mk(0.5), mk(0.5), mk(0.5), mk(1.0)
    ramp = torch.arange(L, dtype=torch.float32).view(1, L, 1) / L
    if s["kshape"] == "rise":
        k = k * (1.0 + 2.0 * ramp)
    elif s["kshape"] == "fall":
        k = k * (3.0 - 2.0 * ramp)
    bias = torch.randn(H, L, L, generator=g) if s["bias"] else None      # (H, q, key)
    q, k, v, dO = (t.to(bf).to(DEV) for t in (q, k, v, dO))
    valid = None if s["valid"] is None else torch.tensor(s["valid"], dtype=torch.int32, device=DEV)
    bias_t = None if bias is None else FO.bias_to_kernel(bias.to(DEV))
    return q, k, v, dO, valid, bias_t


def _kernel(name, inp, seed, **bwd_kw):
    """Forward and backward through the bindings, outputs pre-poisoned."""
    s = SPECS[name]
    ext = _ext()
    q, k, v, dO, valid, bias_t = inp
    B, H, L = s["B"], s["H"], s["L"]
    act, stat = ((B, L, H * 64), bf), ((B, H, L), torch.float32)
    _poison(act, stat)
    O, lse = ext.flash_attn_fwd(q, k, v, H, valid, bias_t, s["scale"], s["causal"], s["p"], seed)
    _poison(act, act, act, stat)
    outs = ext.flash_attn_bwd(dO, q, k, v, O, lse, H, valid, bias_t, s["scale"], s["causal"],
                              s["p"], seed, bias_t is not None, False, **bwd_kw)
    torch.cuda.synchronize()
    return O, lse, outs


def _run(name):
    if name in _RUNS:
        return _RUNS[name]
    s = SPECS[name]
    ext = _ext()
    B, H, L = s["B"], s["H"], s["L"]
    inp = _inputs(name)
    q, k, v, dO, valid, bias_t = inp
    seed = 77000 + ALL.index(name) if s["p"] > 0 else 0
    keep = FO.recover_keep(ext, B, H, L, s["p"], seed, DEV) if s["p"] > 0 else None
    dscale = FO.dropout_scale(s["p"])
    O, lse, outs = _kernel(name, inp, seed)
    assert len(outs) == (4 if s["bias"] else 3)
    got = dict(O=FO.to_bhld(O, H), lse=lse.double(), dq=FO.to_bhld(outs[0], H),
               dk=FO.to_bhld(outs[1], H), dv=FO.to_bhld(outs[2], H))
    for t in (O,) + tuple(outs[:3]):
        assert t.dtype == bf and tuple(t.shape) == (B, L, H * 64)
    if s["bias"]:
        assert outs[3].dtype == torch.float32 and tuple(outs[3].shape) == (H, L, L)
        got["dbias"] = FO.bias_from_kernel(outs[3])
    args = dict(valid=valid, bias=None if bias_t is None else FO.bias_from_kernel(bias_t),
                scale=s["scale"], causal=s["causal"], keep=keep, dscale=dscale)
    q64, k64, v64, dO64 = (FO.to_bhld(t, H) for t in (q, k, v, dO))
    exact = FO.exact_with_grads(q64, k64, v64, dO64, **args)
    emu = FO.attn_emulated(q64, k64, v64, dO64, **args)
    _RUNS[name] = dict(s=s, inp=inp, seed=seed, keep=keep, dscale=dscale, raw=(O, lse, outs),
                       got=got, exact=exact, emu=emu, args=args, x64=(q64, k64, v64, dO64))
    return _RUNS[name]


def _vl(s):
    return s["valid"] if s["valid"] is not None else [s["L"]] * s["B"]


# --------------------------------------------------------------------------
# A. forward, elementwise
# --------------------------------------------------------------------------

@pytest.mark.parametrize("name", ALL)
def test_forward_elementwise(name):
    r = _run(name)
    s, (q, k, v, _) = r["s"], r["x64"]
    t = FO.forward_terms(q, k, v, **r["args"])
    ref, got = r["exact"]["O"], r["got"]["O"]
    delta = (64 + 2) * ACC * t["mag"] + ACC * t["gap"]
    d_row = (t["P"] * delta).sum(-1, keepdim=True)
    fac = U16 + 3 * EPS_FN + delta + d_row + (s["L"] + 2) * ACC
    bound = SECOND * (U16 * ref.abs() + (fac * t["Pd"]) @ v.abs()) + 1e-30
    assert bool(torch.isfinite(got).all()), "non-finite O"
    excess = (got - ref).abs() - bound
    worst = int(excess.argmax())
    print(f"[bound] {name} O: max |err| / bound {float(((got - ref).abs() / bound).max()):.3f}")
    assert float(excess.flatten()[worst]) <= 0.0, (
        f"O element {worst}: got {float(got.flatten()[worst])!r} "
        f"ref {float(ref.flatten()[worst])!r} bound {float(bound.flatten()[worst])!r}")
    # the bound is dominated by its bf16 terms: it cannot hide a wrong fragment
    assert float(bound.max()) < 2.0 ** -5 * float(v.abs().max())


# --------------------------------------------------------------------------
# B. lse
# --------------------------------------------------------------------------

def _lse_fp32(r):
    """The yardstick: the same log-sum-exp in fp32 by torch."""
    s = r["s"]
    q, k, _, _, valid, bias_t = r["inp"]
    B, H, L = s["B"], s["H"], s["L"]
    q32 = q.float().view(B, L, H, 64).transpose(1, 2)
    k32 = k.float().view(B, L, H, 64).transpose(1, 2)
    sc = (q32 @ k32.transpose(-1, -2)) * s["scale"]
    if bias_t is not None:
        sc = sc + bias_t.transpose(-1, -2).unsqueeze(0)
    sc = sc.masked_fill(FO.masked_keys(B, L, valid, s["causal"], DEV), float("-inf"))
    return torch.logsumexp(sc, -1).double()


@pytest.mark.parametrize("name", ALL)
def test_lse(name):
    r = _run(name)
    ref, got = r["exact"]["lse"], r["got"]["lse"]
    assert bool(torch.isfinite(got).all())
    vl = torch.tensor(_vl(r["s"]), device=DEV)
    live = (vl > 0).view(-1, 1, 1).expand_as(ref)
    y32 = _lse_fp32(r)
    yard = float((y32 - ref)[live].abs().max())
    err = float((got - ref)[live].abs().max())
    print(f"[ratio] {name} lse: err_kernel {err:.3e} err_fp32 {yard:.3e} ratio {err / yard:.3f}")
    assert yard > 0.0
    assert err <= LSE_MARGIN * yard, (err, yard)
    # rows with no unmasked key
    assert bool((got[~live] == 0).all()) and bool((ref[~live] == 0).all())
    dead_o = r["got"]["O"][(vl == 0)]
    assert bool((dead_o == 0).all())


# --------------------------------------------------------------------------
# C / D. forward and backward by the emulation rule
# --------------------------------------------------------------------------

def _tile_norms(x, ref, per_bias_block):
    """L2 distance to ref per tile. (B, H, L, d) -> (B, H, L/64);
    dBias (H, Lq, Lk) -> (H, Lk/64)."""
    d = (x - ref) ** 2
    if per_bias_block:
        H, Lq, Lk = d.shape
        return d.view(H, Lq, Lk // TILE, TILE).sum((1, 3)).sqrt()
    B, H, L, dd = d.shape
    return d.view(B, H, L // TILE, TILE, dd).sum((3, 4)).sqrt()


def _structural_zero(r, n):
    """bool per tile: zero by construction (not by cancellation)."""
    s = r["s"]
    B, H, L = s["B"], s["H"], s["L"]
    vl = torch.tensor(_vl(s), device=DEV)
    start = torch.arange(0, L, TILE, device=DEV)
    if n == "dbias":
        return (start >= vl.max()).view(1, -1).expand(H, -1)
    if n in ("dk", "dv"):
        z = start.view(1, 1, -1) >= vl.view(B, 1, 1)
    else:
        z = (vl == 0).view(B, 1, 1).expand(B, 1, L // TILE)
    return z.expand(B, H, L // TILE)


@pytest.mark.parametrize("name", ALL)
def test_emulation_rule(name):
    r = _run(name)
    got, exact, emu = r["got"], r["exact"], r["emu"]
    names = ["O", "dq", "dk", "dv"] + (["dbias"] if r["s"]["bias"] else [])
    for n in names:
        assert bool(torch.isfinite(got[n]).all()), f"{n}: non-finite (a skipped store?)"
        ek = float((got[n] - exact[n]).norm() / exact[n].norm())
        ee = float((emu[n] - exact[n]).norm() / exact[n].norm())
        tk = _tile_norms(got[n], exact[n], n == "dbias")
        te = _tile_norms(emu[n], exact[n], n == "dbias")
        tz = _tile_norms(exact[n], torch.zeros_like(exact[n]), n == "dbias") == 0
        zero = _structural_zero(r, n)
        assert bool(tz[zero].all()), f"{n}: oracle not 0 on a structural-zero tile"
        assert bool((tk[zero] == 0).all()), f"{n}: structural-zero tile not exactly 0"
        live = ~zero
        assert bool((te[live] > 0).all()), f"{n}: emulation exact on a live tile"
        ratio = torch.where(live, tk / te.clamp_min(1e-300), torch.zeros_like(tk))
        worst = tuple(int(i) for i in torch.unravel_index(ratio.argmax(), ratio.shape))
        print(f"[ratio] {name} {n}: err_kernel {ek:.3e} err_emulated {ee:.3e} "
              f"ratio {ek / ee:.3f} tile max {float(ratio.max()):.3f} at {worst} "
              f"min {float(ratio[live].min()):.3f} n={int(live.sum())} zero={int(zero.sum())}")
        assert 0.0 < ee < 0.1, (n, ee)
        assert ek <= 4.0 * ee, (n, ek, ee)
        assert float(ratio.max()) <= 4.0, (n, "tile", worst, float(ratio.max()))


def test_valid_values_covered():
    seen = set()
    for n in ALL:
        s = SPECS[n]
        if s["valid"] is None:
            seen.add(None)
            continue
        for x in s["valid"]:
            seen.add({s["L"]: "L", s["L"] - 1: "L-1"}.get(x, x))
            if x in (63, 64, 65, 1, 0):
                seen.add(x)
    assert {"L", "L-1", 65, 64, 63, 1, 0, None} <= seen
    for n in ALL:  # valid = 1 only where dropout keeps dS from cancelling to 0
        assert SPECS[n]["valid"] is None or 1 not in SPECS[n]["valid"] or SPECS[n]["p"] > 0
    full = {(s["valid"] is not None, s["causal"], s["bias"], s["p"] > 0)
            for s in SPECS.values() if s["L"] == 192}
    assert len(full) == 16


# --------------------------------------------------------------------------
# D. the mask itself
# --------------------------------------------------------------------------

def test_dropout_mask_properties():
    ext = _ext()
    B, H, L = 3, 3, 192
    k1 = FO.recover_keep(ext, B, H, L, P_DROP, 4242, DEV)
    k1b = FO.recover_keep(ext, B, H, L, P_DROP, 4242, DEV)
    k2 = FO.recover_keep(ext, B, H, L, P_DROP, 4243, DEV)
    assert torch.equal(k1, k1b)
    assert not torch.equal(k1, k2)
    ph = 231.0 / 256.0
    assert FO.dropout_scale(P_DROP) == 1.0 / ph

    def within(rate, expect, n, what):
        sigma = math.sqrt(expect * (1.0 - expect) / n)
        print(f"[mask] {what}: {rate:.5f} expected {expect:.5f} "
              f"({(rate - expect) / sigma:+.2f} sigma, n={n})")
        assert abs(rate - expect) <= 6.0 * sigma, (what, rate, expect, sigma)

    agree = ph * ph + (1.0 - ph) * (1.0 - ph)
    for tag, m in (("seed 4242", k1), ("seed 4243", k2)):
        within(float(m.mean()), ph, m.numel(), f"{tag} keep fraction")
        f = m.view(B * H, L, L)
        within(float((f[1:] == f[:-1]).double().mean()), agree, (B * H - 1) * L * L,
               f"{tag} agreement of neighbouring (b, h)")
        within(float((f[0] == f[B * H - 1]).double().mean()), agree, L * L,
               f"{tag} agreement of the first and last (b, h)")
        within(float((f[:, 1:] == f[:, :-1]).double().mean()), agree, B * H * (L - 1) * L,
               f"{tag} agreement of neighbouring query rows")
    within(float((k1 == k2).double().mean()), agree, k1.numel(), "agreement of two seeds")
    # the mask does not depend on q, k, v: recovered masks are what C used
    r = _run("L192-valid+causal-bias-drop")
    assert torch.equal(r["keep"], FO.recover_keep(ext, B, H, L, P_DROP, r["seed"], DEV))


# --------------------------------------------------------------------------
# E. layout paths, bit-exact
# --------------------------------------------------------------------------

def test_fused_grads_bit_exact():
    name = "L192-valid+causal-bias-drop"
    r = _run(name)
    s, ext = r["s"], _ext()
    q, k, v, dO, valid, bias_t = r["inp"]
    B, H, L = s["B"], s["H"], s["L"]
    D = H * 64
    qkv = torch.cat([q, k, v], -1).contiguous()
    qs, ks, vs = qkv[..., :D], qkv[..., D:2 * D], qkv[..., 2 * D:]
    O0, lse0, outs0 = r["raw"]
    O, lse = ext.flash_attn_fwd(qs, ks, vs, H, valid, bias_t, s["scale"], True, s["p"], r["seed"])
    assert torch.equal(O, O0) and torch.equal(lse, lse0)
    _poison(((B, L, 3 * D), bf), ((B, H, L), torch.float32))
    outs = ext.flash_attn_bwd(dO, qs, ks, vs, O, lse, H, valid, bias_t, s["scale"], True,
                              s["p"], r["seed"], True, True)
    assert len(outs) == 2 and tuple(outs[0].shape) == (B, L, 3 * D)
    for i in range(3):
        assert torch.equal(outs[0][..., i * D:(i + 1) * D], outs0[i]), "qkv"[i]
    # dBias is a sum of fp32 atomics in any order: with valid = 0 in one of the
    # three batch rows every element has at most two addends, so it is exact
    assert sorted(s["valid"])[0] == 0 and B == 3
    assert torch.equal(outs[1], outs0[3])


def test_kv_fused_bit_exact():
    name = "L192-valid-drop"
    r = _run(name)
    s, ext = r["s"], _ext()
    q, k, v, dO, valid, _ = r["inp"]
    B, H, L = s["B"], s["H"], s["L"]
    D = H * 64
    kv = torch.cat([k, v], -1).contiguous()
    ks, vs = kv[..., :D], kv[..., D:]
    O0, lse0, outs0 = r["raw"]
    O, lse = ext.flash_attn_fwd(q, ks, vs, H, valid, None, s["scale"], False, s["p"], r["seed"])
    assert torch.equal(O, O0) and torch.equal(lse, lse0)
    _poison(((B, L, D), bf), ((B, L, 2 * D), bf), ((B, H, L), torch.float32))
    outs = ext.flash_attn_bwd(dO, q, ks, vs, O, lse, H, valid, None, s["scale"], False,
                              s["p"], r["seed"], False, False, None, kv_fused=True)
    assert len(outs) == 2 and tuple(outs[1].shape) == (B, L, 2 * D)
    assert torch.equal(outs[0], outs0[0])
    assert torch.equal(outs[1][..., :D], outs0[1]) and torch.equal(outs[1][..., D:], outs0[2])


def test_wrappers_match_bindings():
    """The autograd wrappers (p = 0: no seed to control) give the bindings'
    bits, on contiguous tensors and on the packed QKV path."""
    from deepdfa_amd.ops.transformer import flash_attention, flash_attention_qkv

    name = "L192-valid+causal-bias"
    r = _run(name)
    s = r["s"]
    q, k, v, dO, valid, bias_t = r["inp"]
    O0, _, outs0 = r["raw"]
    D = s["H"] * 64
    ql, kl, vl = (t.clone().requires_grad_() for t in (q, k, v))
    bl = bias_t.clone().requires_grad_()
    O = flash_attention(ql, kl, vl, s["H"], valid=valid, bias=bl, scale=s["scale"], causal=True)
    O.backward(dO)
    assert torch.equal(O, O0)
    for a, b in zip((ql, kl, vl), outs0[:3]):
        assert torch.equal(a.grad, b)
    assert sorted(s["valid"])[0] == 0 and s["B"] == 3   # <= 2 atomic addends: exact
    assert torch.equal(bl.grad, outs0[3])
    qkv = torch.cat([q, k, v], -1).contiguous().requires_grad_()
    O = flash_attention_qkv(qkv, s["H"], valid=valid, bias=bias_t, scale=s["scale"], causal=True)
    O.backward(dO)
    assert torch.equal(O, O0)
    for i in range(3):
        assert torch.equal(qkv.grad[..., i * D:(i + 1) * D], outs0[i])


# --------------------------------------------------------------------------
# F. dbias_accum
# --------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["L192-valid+causal-bias-drop", "L64-valid-bias"])
def test_dbias_accum(name):
    r = _run(name)
    s, ext = r["s"], _ext()
    q, k, v, dO, valid, bias_t = r["inp"]
    B, H, L = s["B"], s["H"], s["L"]
    O, lse, outs0 = r["raw"]
    G = outs0[3].double()
    g0 = torch.randn(H, L, L, generator=torch.Generator().manual_seed(5)).to(DEV)
    buf = g0.clone()
    t = 2
    for _ in range(t):
        outs = ext.flash_attn_bwd(dO, q, k, v, O, lse, H, valid, bias_t, s["scale"], s["causal"],
                                  s["p"], r["seed"], True, False, buf)
        assert len(outs) == 3, "a separate dBias came back next to dbias_accum"
        for a, b in zip(outs, outs0[:3]):
            assert torch.equal(a, b)
    torch.cuda.synchronize()
    abs_ds = r["emu"]["abs_ds"].transpose(-1, -2)
    bound = (t * B + 1) * ACC * (g0.double().abs() + t * abs_ds)
    assert float(abs_ds.max()) > 0 and float(G.abs().max()) > 0
    excess = (buf.double() - (g0.double() + t * G)).abs() - bound
    assert float(excess.max()) <= 0.0, float(excess.max())


# --------------------------------------------------------------------------
# the earlier fp32-oracle tests, unchanged
# --------------------------------------------------------------------------

@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def materialized(q, k, v, H, valid, bias, scale, causal):
    """fp32 oracle in (B, L, H*d) layout."""
    B, L, HD = q.shape
    d = HD // H

    def split(t):
        return t.float().view(B, L, H, d).transpose(1, 2)

    qs, ks, vs = split(q), split(k), split(v)
    s = torch.matmul(qs, ks.transpose(-1, -2)) * scale
    if bias is not None:
        s = s + bias.unsqueeze(0)
    if valid is not None:
        mask = torch.arange(L, device=q.device).view(1, 1, 1, L) >= valid.view(-1, 1, 1, 1)
        s = s.masked_fill(mask, float("-inf"))
    if causal:
        cm = torch.arange(L, device=q.device).view(1, L) > torch.arange(
            L, device=q.device
        ).view(L, 1)
        s = s.masked_fill(cm.view(1, 1, L, L), float("-inf"))
    p = torch.nan_to_num(torch.softmax(s, -1), nan=0.0)
    o = torch.matmul(p, vs)
    return o.transpose(1, 2).reshape(B, L, HD)


def rand_qkv(dev, B=2, H=4, L=128, seed=0, grad=False):
    torch.manual_seed(seed)
    mk = lambda: (torch.randn(B, L, H * 64, device=dev) * 0.5).to(bf).requires_grad_(grad)  # noqa: E731
    return mk(), mk(), mk()


@pytest.mark.parametrize("causal", [False, True])
def test_flash_fwd_parity(dev, causal):
    from deepdfa_amd.ops.transformer import flash_attention

    q, k, v = rand_qkv(dev, seed=1)
    valid = torch.tensor([128, 70], dtype=torch.int32, device=dev)
    scale = 1.0 / math.sqrt(64)
    out = flash_attention(q, k, v, 4, valid=valid, scale=scale, causal=causal)
    ref_o = materialized(q, k, v, 4, valid, None, scale, causal)
    # rows beyond valid are undefined-but-finite; compare valid rows
    m = (torch.arange(128, device=dev).view(1, -1, 1) < valid.view(-1, 1, 1)).float()
    err = ((out.float() - ref_o) * m).abs().max().item()
    assert err < 3e-2, err


def test_flash_fwd_bias(dev):
    from deepdfa_amd.ops.transformer import flash_attention

    q, k, v = rand_qkv(dev, seed=2)
    bias = torch.randn(4, 128, 128, device=dev)
    out = flash_attention(q, k, v, 4, bias=bias.transpose(-1, -2).contiguous(),
                          scale=1.0)
    ref_o = materialized(q, k, v, 4, None, bias, 1.0, False)
    err = (out.float() - ref_o).abs().max().item()
    assert err < 5e-2, err


def test_flash_bwd_parity(dev):
    from deepdfa_amd.ops.transformer import flash_attention

    scale = 1.0 / math.sqrt(64)
    valid = torch.tensor([128, 100], dtype=torch.int32, device=dev)
    q, k, v = rand_qkv(dev, seed=3, grad=True)
    out = flash_attention(q, k, v, 4, valid=valid, scale=scale)
    # mask pad-query-row grads on BOTH sides: those rows' outputs are
    # downstream-masked in the models, so their grads are not defined parity
    m = (torch.arange(128, device=dev).view(1, -1, 1) < valid.view(-1, 1, 1)).float()
    go = torch.randn_like(out)
    gom = (go.float() * m).to(bf)
    out.backward(gom)
    q2 = q.detach().clone().requires_grad_(True)
    k2 = k.detach().clone().requires_grad_(True)
    v2 = v.detach().clone().requires_grad_(True)
    ref_o = materialized(q2, k2, v2, 4, valid, None, scale, False)
    ref_o.backward(gom.float())
    for a, b, name in ((q, q2, "dq"), (k, k2, "dk"), (v, v2, "dv")):
        err = (a.grad.float() - b.grad).abs().max().item()
        ref_mag = b.grad.abs().max().item()
        assert err < 0.05 * max(ref_mag, 1.0), (name, err, ref_mag)


def test_flash_bwd_bias_grad(dev):
    from deepdfa_amd.ops.transformer import flash_attention

    q, k, v = rand_qkv(dev, B=2, seed=4)
    bias = torch.randn(4, 128, 128, device=dev, requires_grad=True)
    out = flash_attention(q, k, v, 4, bias=bias.transpose(-1, -2).contiguous(),
                          scale=1.0, causal=True)
    go = torch.randn_like(out)
    out.backward(go)
    b2 = bias.detach().clone().requires_grad_(True)
    ref_o = materialized(q, k, v, 4, None, b2, 1.0, True)
    ref_o.backward(go.float())
    err = (bias.grad - b2.grad).abs().max().item()
    assert err < 0.05 * max(b2.grad.abs().max().item(), 1.0), err


def test_flash_dropout_consistency(dev):
    from deepdfa_amd.ops.transformer import flash_attention

    q, k, v = rand_qkv(dev, seed=5, grad=True)
    out = flash_attention(q, k, v, 4, scale=0.125, dropout_p=0.5)
    out_ref = flash_attention(q.detach(), k.detach(), v.detach(), 4, scale=0.125)
    # dropout changes the output meaningfully but keeps it finite
    assert torch.isfinite(out.float()).all()
    assert (out.float() - out_ref.float()).abs().max().item() > 0.01
    out.float().square().mean().backward()
    assert torch.isfinite(q.grad.float()).all()


def test_roberta_flash_vs_materialized(dev):
    """Whole encoder: flash path (L=128) vs materialized (output_attentions)."""
    from deepdfa_amd.models.roberta import RobertaConfig, RobertaModel, init_roberta_weights

    torch.manual_seed(0)
    cfg = RobertaConfig(vocab_size=500, hidden_size=256, num_hidden_layers=2,
                        num_attention_heads=4, intermediate_size=512,
                        max_position_embeddings=200)
    model = RobertaModel(cfg)
    init_roberta_weights(model)
    model = model.to(dev).eval()
    ids = torch.randint(3, 500, (2, 128), device=dev)
    ids[0, 90:] = 1
    with torch.no_grad(), torch.autocast(device_type="cuda", dtype=bf):
        out_flash, _ = model(ids)  # flash (no attention output)
        out_mat, _ = model(ids, output_attentions=True)  # materialized
    mask = ids.ne(1).unsqueeze(-1)
    err = ((out_flash.float() - out_mat.float()) * mask).abs().max().item()
    assert err < 0.05, err


@pytest.mark.gpu
def test_flash_strided_qkv_views_match_contiguous():
    """Row-strided Q/K/V (slices of a fused QKV buffer) must give the same
    forward and backward as contiguous tensors."""
    from deepdfa_amd.ops.transformer import flash_attention

    torch.manual_seed(0)
    B, L, H, d = 2, 128, 4, 64
    D = H * d
    qkv = (torch.randn(B, L, 3 * D, device="cuda", dtype=torch.bfloat16) * 0.3
           ).requires_grad_()
    qc = qkv[..., :D].detach().contiguous().requires_grad_()
    kc = qkv[..., D:2 * D].detach().contiguous().requires_grad_()
    vc = qkv[..., 2 * D:].detach().contiguous().requires_grad_()
    valid = torch.tensor([L, 96], dtype=torch.int32, device="cuda")

    o1 = flash_attention(qkv[..., :D], qkv[..., D:2 * D], qkv[..., 2 * D:],
                         H, valid=valid, scale=0.125)
    o2 = flash_attention(qc, kc, vc, H, valid=valid, scale=0.125)
    assert torch.equal(o1, o2)
    g = torch.randn_like(o1)
    o1.backward(g)
    o2.backward(g)
    dq = qkv.grad[..., :D]
    dk = qkv.grad[..., D:2 * D]
    dv = qkv.grad[..., 2 * D:]
    assert torch.equal(dq, qc.grad)
    assert torch.equal(dk, kc.grad)
    assert torch.equal(dv, vc.grad)
