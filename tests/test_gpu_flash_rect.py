"""General flash attention (csrc/flash_rect.hip: forward, dq, dkv at any
query length Lq and key length Lk) against the float64 oracles of
tests/flash_rect_oracle.py.

Rules A, B, C, D and F of tests/test_gpu_flash.py, unchanged, with the
constants of that file (u = 2^-8, 2^-23 per accumulated term, eps_fn = 2^-20,
the second-order factor 1 + 2^-7, LSE_MARGIN = 4, the emulation margin 4, 6
sigma for the mask statistics); see its docstring for their derivation. What
changes with the shape:
  A  the accumulation term is (Lk + 2) 2^-23.
  C  tiles are 64 rows of the tensor's own length: Lq for O and dQ, Lk for dK
     and dV, 64-key blocks for dBias; a partial tail counts as a tile. On top
     of the structural-zero tiles every dK/dV ROW of a key >= valid[b] is
     exactly 0.
  One shape has no defined ratio: at Lk = 1 without dropout P = 1, so
  O = v and dV = dO exactly (kernel, emulation and oracle alike: the rule
  then asks for error 0) and dQ, dK cancel to exactly 0 in float64 while the
  kernel keeps the fp32 summation noise of dO.v - dO.O (this is why valid = 1
  appears only with dropout, here as in test_gpu_flash.py). There
     |dS| <= 2 (64 + 2) 2^-23 sum_d |dO v|,
  the two fp32 dot products of 64 terms that should cancel, and the test
  bounds |dQ| by (1 + 2^-7) scale |dS| |k| and |dK| by the same with |q|.

The table's (150, 320) case names (B, H) = (2, 12) together with three valid
lengths [320, 319, 0]; valid holds B entries, so the case runs at
(B, H) = (3, 12), which keeps every length of the table.

Model level: a T5, a RoBERTa layer and a Seq2SeqDecoderLayer at lengths off
the 64 grid run the general kernels (counted) and match the CPU in fp32.

Observed on an MI355X. C: err_kernel / err_emulated of whole tensors between
0.76 and 1.01, the largest tile 2.135 (129x191-valid-drop dQ, the one-row tail
tile of (b, h) = (2, 1)), every other tile below 1.34; dV at 1.000 throughout.
At L = 128 and 192 the general and the tuned kernels print the same ratios to
every digit. B: lse within 0.82 .. 1.26 of the fp32 yardstick. A: the largest
|err| / bound per case between 0.23 and 0.76 (0 at 1 x 1, which is exact).
Peak memory of the 448 x 513 case 22.9 MiB against the 42.1 MiB limit.
"""

import math

import pytest
import torch

import flash_oracle as FO
import flash_rect_oracle as FR

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

def _spec(Lq, Lk, valid=None, p=0.0, causal=False, bias=False, B=3, H=3, scale=1.0,
          kshape="flat"):
    assert valid is None or len(valid) == B
    assert not (causal or bias) or Lq == Lk
    return dict(Lq=Lq, Lk=Lk, B=B, H=H, valid=valid, causal=causal, bias=bias, p=p,
                scale=scale, kshape=kshape)


SPECS = {
    "1x1": _spec(1, 1),
    "32x128-valid": _spec(32, 128, [128, 65, 0]),
    "33x65-valid-drop": _spec(33, 65, [65, 64, 1], P_DROP),
    "100x37": _spec(100, 37),
    "129x191-valid-drop": _spec(129, 191, [191, 63, 128], P_DROP),
    "64x192-valid-drop": _spec(64, 192, [192, 1, 100], P_DROP),
    "150x320-H12-valid-drop": _spec(150, 320, [320, 319, 0], P_DROP, B=3, H=12, scale=0.125),
    "37-causal-bias-drop": _spec(37, 37, None, P_DROP, causal=True, bias=True),
    "150-valid+causal-bias-drop": _spec(150, 150, [150, 77, 0], P_DROP, causal=True, bias=True,
                                        kshape="rise"),
    "200-valid-bias": _spec(200, 200, [199, 0, 64], 0.0, bias=True),
    # the tuned kernels' ground, for the comparison of the two kernel sets
    "128-valid+causal-bias-drop": _spec(128, 128, [127, 65, 0], P_DROP, causal=True, bias=True),
    "192-valid+causal-bias-drop": _spec(192, 192, [192, 77, 0], P_DROP, causal=True, bias=True),
}
ALL = list(SPECS)
TABLE = ALL[:10]
BIAS_CASES = [n for n in ALL if SPECS[n]["bias"]]

_RUNS = {}
_INPUTS = {}
_REFS = {}


def _poison(*shapes_dtypes):
    """Allocate, NaN-fill and free tensors of the coming outputs' sizes: the
    caching allocator hands the same blocks to the kernel's at::empty."""
    ts = [torch.full(s, float("nan"), dtype=dt, device=DEV) for s, dt in shapes_dtypes]
    torch.cuda.synchronize()
    del ts


def _inputs(name):
    if name in _INPUTS:
        return _INPUTS[name]
    s = SPECS[name]
    B, H, Lq, Lk = s["B"], s["H"], s["Lq"], s["Lk"]
    g = torch.Generator().manual_seed(2000 + ALL.index(name))
    mk = lambda L, sc: torch.randn(B, L, H * 64, generator=g) * sc  # noqa: E731
    q, k, v, dO = mk(Lq, 0.5), mk(Lk, 0.5), mk(Lk, 0.5), mk(Lq, 1.0)
    ramp = torch.arange(Lk, dtype=torch.float32).view(1, Lk, 1) / Lk
    if s["kshape"] == "rise":
        k = k * (1.0 + 2.0 * ramp)
    bias = torch.randn(H, Lq, Lk, generator=g) if s["bias"] else None      # (H, q, key)
    q, k, v, dO = (t.to(bf).to(DEV) for t in (q, k, v, dO))
    valid = None if s["valid"] is None else torch.tensor(s["valid"], dtype=torch.int32, device=DEV)
    bias_t = None if bias is None else FO.bias_to_kernel(bias.to(DEV))
    _INPUTS[name] = (q, k, v, dO, valid, bias_t)
    return _INPUTS[name]


def _seed(name):
    return 88000 + ALL.index(name) if SPECS[name]["p"] > 0 else 0


def _kernel(name, inp, seed, tuned=False, **bwd_kw):
    """Forward and backward through the bindings, outputs pre-poisoned."""
    s = SPECS[name]
    ext = _ext()
    q, k, v, dO, valid, bias_t = inp
    B, H, Lq, Lk = s["B"], s["H"], s["Lq"], s["Lk"]
    qa, ka, stat = ((B, Lq, H * 64), bf), ((B, Lk, H * 64), bf), ((B, H, Lq), torch.float32)
    _poison(qa, stat)
    fwd = ext.flash_attn_fwd if tuned else ext.flash_rect_fwd
    O, lse = fwd(q, k, v, H, valid, bias_t, s["scale"], s["causal"], s["p"], seed)
    _poison(qa, ka, ka, stat)
    if tuned:
        outs = ext.flash_attn_bwd(dO, q, k, v, O, lse, H, valid, bias_t, s["scale"], s["causal"],
                                  s["p"], seed, bias_t is not None, False, **bwd_kw)
    else:
        outs = ext.flash_rect_bwd(dO, q, k, v, O, lse, H, valid, bias_t, s["scale"], s["causal"],
                                  s["p"], seed, bias_t is not None, **bwd_kw)
    torch.cuda.synchronize()
    return O, lse, outs


def _reference(name):
    """keep mask, float64 oracle and emulation: once per case."""
    if name in _REFS:
        return _REFS[name]
    s = SPECS[name]
    q, k, v, dO, valid, bias_t = _inputs(name)
    H = s["H"]
    seed = _seed(name)
    keep = (FR.recover_keep_rect(_ext(), s["B"], H, s["Lq"], s["Lk"], s["p"], seed, DEV)
            if s["p"] > 0 else None)
    args = dict(valid=valid, bias=None if bias_t is None else FO.bias_from_kernel(bias_t),
                scale=s["scale"], causal=s["causal"], keep=keep, dscale=FO.dropout_scale(s["p"]))
    x64 = tuple(FO.to_bhld(t, H) for t in (q, k, v, dO))
    _REFS[name] = dict(seed=seed, keep=keep, args=args, x64=x64,
                       exact=FR.exact_with_grads(*x64, **args),
                       emu=FR.attn_emulated(*x64, **args))
    return _REFS[name]


def _as_got(s, O, lse, outs):
    B, H, Lq, Lk = s["B"], s["H"], s["Lq"], s["Lk"]
    assert len(outs) == (4 if s["bias"] else 3)
    for t, L in ((O, Lq), (outs[0], Lq), (outs[1], Lk), (outs[2], Lk)):
        assert t.dtype == bf and tuple(t.shape) == (B, L, H * 64)
    assert lse.dtype == torch.float32 and tuple(lse.shape) == (B, H, Lq)
    got = dict(O=FO.to_bhld(O, H), lse=lse.double(), dq=FO.to_bhld(outs[0], H),
               dk=FO.to_bhld(outs[1], H), dv=FO.to_bhld(outs[2], H))
    if s["bias"]:
        assert outs[3].dtype == torch.float32 and tuple(outs[3].shape) == (H, Lk, Lq)
        got["dbias"] = FO.bias_from_kernel(outs[3])
    return got


def _run(name):
    if name in _RUNS:
        return _RUNS[name]
    s = SPECS[name]
    ref = _reference(name)
    inp = _inputs(name)
    O, lse, outs = _kernel(name, inp, ref["seed"])
    _RUNS[name] = dict(ref, s=s, inp=inp, raw=(O, lse, outs), got=_as_got(s, O, lse, outs))
    return _RUNS[name]


def _vl(s):
    return [min(x, s["Lk"]) for x in s["valid"]] if s["valid"] is not None else [s["Lk"]] * s["B"]


# --------------------------------------------------------------------------
# A. forward, elementwise
# --------------------------------------------------------------------------

@pytest.mark.parametrize("name", TABLE)
def test_forward_elementwise(name):
    r = _run(name)
    s, (q, k, v, _) = r["s"], r["x64"]
    t = FR.forward_terms(q, k, v, **r["args"])
    ref, got = r["exact"]["O"], r["got"]["O"]
    delta = (64 + 2) * ACC * t["mag"] + ACC * t["gap"]
    d_row = (t["P"] * delta).sum(-1, keepdim=True)
    fac = U16 + 3 * EPS_FN + delta + d_row + (s["Lk"] + 2) * ACC
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
    B, H, Lq, Lk = s["B"], s["H"], s["Lq"], s["Lk"]
    q32 = q.float().view(B, Lq, H, 64).transpose(1, 2)
    k32 = k.float().view(B, Lk, H, 64).transpose(1, 2)
    sc = (q32 @ k32.transpose(-1, -2)) * s["scale"]
    if bias_t is not None:
        sc = sc + bias_t.transpose(-1, -2).unsqueeze(0)
    sc = sc.masked_fill(FR.masked_keys(B, Lq, Lk, valid, s["causal"], DEV), float("-inf"))
    return torch.logsumexp(sc, -1).double()


@pytest.mark.parametrize("name", TABLE)
def test_lse(name):
    r = _run(name)
    ref, got = r["exact"]["lse"], r["got"]["lse"]
    assert bool(torch.isfinite(got).all())
    vl = torch.tensor(_vl(r["s"]), device=DEV)
    live = (vl > 0).view(-1, 1, 1).expand_as(ref)
    y32 = _lse_fp32(r)
    yard = float((y32 - ref)[live].abs().max())
    err = float((got - ref)[live].abs().max())
    print(f"[ratio] {name} lse: err_kernel {err:.3e} err_fp32 {yard:.3e} "
          f"ratio {err / max(yard, 1e-300):.3f}")
    if r["s"]["Lk"] > 1:
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
    """L2 distance to ref per 64-row tile, a partial tail tile included.
    (B, H, L, d) -> (B, H, ceil(L/64)); dBias (H, Lq, Lk) -> (H, ceil(Lk/64))."""
    d = (x - ref) ** 2
    if per_bias_block:
        H, Lq, Lk = d.shape
        pad = -Lk % TILE
        d = torch.nn.functional.pad(d, (0, pad))
        return d.view(H, Lq, (Lk + pad) // TILE, TILE).sum((1, 3)).sqrt()
    B, H, L, dd = d.shape
    pad = -L % TILE
    d = torch.nn.functional.pad(d, (0, 0, 0, pad))
    return d.view(B, H, (L + pad) // TILE, TILE, dd).sum((3, 4)).sqrt()


def _structural_zero(s, n):
    """bool per tile: zero by construction (not by cancellation)."""
    B, H, Lq, Lk = s["B"], s["H"], s["Lq"], s["Lk"]
    vl = torch.tensor(_vl(s), device=DEV)
    if n == "dbias":
        start = torch.arange(0, Lk, TILE, device=DEV)
        return (start >= vl.max()).view(1, -1).expand(H, -1)
    if n in ("dk", "dv"):
        start = torch.arange(0, Lk, TILE, device=DEV)
        z = start.view(1, 1, -1) >= vl.view(B, 1, 1)
        return z.expand(B, H, -1)
    nt = (Lq + TILE - 1) // TILE
    return (vl == 0).view(B, 1, 1).expand(B, H, nt)


def _check_rule_c(name, got, exact, emu, x64, tag=""):
    s = SPECS[name]
    names = ["O", "dq", "dk", "dv"] + (["dbias"] if s["bias"] else [])
    degenerate = s["Lk"] == 1 and s["p"] == 0      # P = 1: see the module docstring
    q, k, v, dO = x64
    for n in names:
        assert bool(torch.isfinite(got[n]).all()), f"{n}: non-finite (a skipped store?)"
        if degenerate and n in ("dq", "dk"):
            assert float(exact[n].abs().max()) == 0 and float(emu[n].abs().max()) == 0
            ds = 2 * (64 + 2) * ACC * (dO.abs() * v.abs()).sum(-1, keepdim=True)   # (B, H, Lq, 1)
            other = k.abs() if n == "dq" else q.abs()
            bound = SECOND * s["scale"] * (ds * other if n == "dq"
                                           else (ds * other).sum(2, keepdim=True))
            print(f"[bound] {name}{tag} {n}: max |got| {float(got[n].abs().max()):.3e} "
                  f"bound min {float(bound.min()):.3e}")
            assert bool((got[n].abs() <= bound).all()), n
            continue
        ek = float((got[n] - exact[n]).norm() / exact[n].norm())
        ee = float((emu[n] - exact[n]).norm() / exact[n].norm())
        tk = _tile_norms(got[n], exact[n], n == "dbias")
        te = _tile_norms(emu[n], exact[n], n == "dbias")
        tz = _tile_norms(exact[n], torch.zeros_like(exact[n]), n == "dbias") == 0
        zero = _structural_zero(s, n)
        assert zero.shape == tk.shape
        assert bool(tz[zero].all()), f"{n}: oracle not 0 on a structural-zero tile"
        assert bool((tk[zero] == 0).all()), f"{n}: structural-zero tile not exactly 0"
        live = ~zero
        if not degenerate:
            assert bool((te[live] > 0).all()), f"{n}: emulation exact on a live tile"
            assert 0.0 < ee < 0.1, (n, ee)
        ratio = torch.where(live & (te > 0), tk / te.clamp_min(1e-300), torch.zeros_like(tk))
        worst = tuple(int(i) for i in torch.unravel_index(ratio.argmax(), ratio.shape))
        print(f"[ratio] {name}{tag} {n}: err_kernel {ek:.3e} err_emulated {ee:.3e} "
              f"ratio {ek / max(ee, 1e-300):.3f} tile max {float(ratio.max()):.3f} at {worst} "
              f"n={int(live.sum())} zero={int(zero.sum())}")
        assert ek <= 4.0 * ee, (n, ek, ee)
        assert bool((tk <= 4.0 * te)[live].all()), (n, "tile", worst, float(ratio.max()))
    # every dK / dV row of a key >= valid[b], inside a live tile too
    vl = torch.tensor(_vl(s), device=DEV)
    dead_key = torch.arange(s["Lk"], device=DEV).view(1, 1, -1) >= vl.view(-1, 1, 1)
    for n in ("dk", "dv"):
        rows = got[n].abs().sum(-1)                     # (B, H, Lk)
        assert bool((rows[dead_key.expand_as(rows)] == 0).all()), f"{n}: masked key row not 0"


@pytest.mark.parametrize("name", TABLE)
def test_emulation_rule(name):
    r = _run(name)
    _check_rule_c(name, r["got"], r["exact"], r["emu"], r["x64"])


def test_cases_cover_the_table():
    shapes = [(SPECS[n]["Lq"], SPECS[n]["Lk"]) for n in TABLE]
    assert shapes == [(1, 1), (32, 128), (33, 65), (100, 37), (129, 191), (64, 192),
                      (150, 320), (37, 37), (150, 150), (200, 200)]
    for n in ALL:  # valid = 1 only where dropout keeps dS from cancelling to 0
        assert SPECS[n]["valid"] is None or 1 not in SPECS[n]["valid"] or SPECS[n]["p"] > 0


# --------------------------------------------------------------------------
# D. the mask itself
# --------------------------------------------------------------------------

def test_dropout_mask_equals_tuned_kernels_at_square():
    ext = _ext()
    B, H, L = 3, 3, 128
    a = FR.recover_keep_rect(ext, B, H, L, L, P_DROP, 4242, DEV)
    b = FO.recover_keep(ext, B, H, L, P_DROP, 4242, DEV)
    assert 0.0 < float(a.mean()) < 1.0
    assert torch.equal(a, b)


def test_dropout_mask_properties():
    ext = _ext()
    B, H, Lq, Lk = 3, 3, 129, 191
    k1 = FR.recover_keep_rect(ext, B, H, Lq, Lk, P_DROP, 4242, DEV)
    k1b = FR.recover_keep_rect(ext, B, H, Lq, Lk, P_DROP, 4242, DEV)
    k2 = FR.recover_keep_rect(ext, B, H, Lq, Lk, P_DROP, 4243, DEV)
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
        f = m.view(B * H, Lq, Lk)
        within(float((f[1:] == f[:-1]).double().mean()), agree, (B * H - 1) * Lq * Lk,
               f"{tag} agreement of neighbouring (b, h)")
        within(float((f[0] == f[B * H - 1]).double().mean()), agree, Lq * Lk,
               f"{tag} agreement of the first and last (b, h)")
        within(float((f[:, 1:] == f[:, :-1]).double().mean()), agree, B * H * (Lq - 1) * Lk,
               f"{tag} agreement of neighbouring query rows")
    within(float((k1 == k2).double().mean()), agree, k1.numel(), "agreement of two seeds")
    # the mask does not depend on q, k, v: recovered masks are what C used
    r = _run("129x191-valid-drop")
    assert torch.equal(r["keep"], FR.recover_keep_rect(ext, B, H, Lq, Lk, P_DROP, r["seed"], DEV))


# --------------------------------------------------------------------------
# the two kernel sets on the tuned kernels' ground
# --------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["128-valid+causal-bias-drop", "192-valid+causal-bias-drop"])
def test_both_kernel_sets_satisfy_rule_c(name):
    s = SPECS[name]
    r = _run(name)
    # one mask for both: the square index is the tuned kernels' own
    assert torch.equal(r["keep"], FO.recover_keep(_ext(), s["B"], s["H"], s["Lq"], s["p"],
                                                  r["seed"], DEV))
    _check_rule_c(name, r["got"], r["exact"], r["emu"], r["x64"], " rect")
    O, lse, outs = _kernel(name, r["inp"], r["seed"], tuned=True)
    got = _as_got(s, O, lse, outs)
    _check_rule_c(name, got, r["exact"], r["emu"], r["x64"], " tuned")


# --------------------------------------------------------------------------
# layouts, bit-exact; determinism
# --------------------------------------------------------------------------

def test_kv_fused_and_strided_inputs_bit_exact():
    name = "64x192-valid-drop"
    r = _run(name)
    s, ext = r["s"], _ext()
    q, k, v, dO, valid, _ = r["inp"]
    B, H, Lq, Lk = s["B"], s["H"], s["Lq"], s["Lk"]
    D = H * 64
    kv = torch.cat([k, v], -1).contiguous()
    ks, vs = kv[..., :D], kv[..., D:]
    qs = torch.cat([q, q], -1)[..., D:]          # a strided Q as well
    O0, lse0, outs0 = r["raw"]
    _poison(((B, Lq, D), bf), ((B, H, Lq), torch.float32))
    O, lse = ext.flash_rect_fwd(qs, ks, vs, H, valid, None, s["scale"], False, s["p"], r["seed"])
    assert torch.equal(O, O0) and torch.equal(lse, lse0)
    _poison(((B, Lq, D), bf), ((B, Lk, 2 * D), bf), ((B, H, Lq), torch.float32))
    outs = ext.flash_rect_bwd(dO, qs, ks, vs, O, lse, H, valid, None, s["scale"], False,
                              s["p"], r["seed"], False, None, kv_fused=True)
    assert len(outs) == 2 and tuple(outs[1].shape) == (B, Lk, 2 * D)
    assert torch.equal(outs[0], outs0[0])
    assert torch.equal(outs[1][..., :D], outs0[1]) and torch.equal(outs[1][..., D:], outs0[2])
    # strided halves without kv_fused: three dense grads, the same bits
    outs = ext.flash_rect_bwd(dO, qs, ks, vs, O, lse, H, valid, None, s["scale"], False,
                              s["p"], r["seed"], False)
    assert len(outs) == 3
    for a, b in zip(outs, outs0):
        assert a.is_contiguous() and torch.equal(a, b)
    with pytest.raises(RuntimeError, match="kv_fused"):
        ext.flash_rect_bwd(dO, q, k, v, O, lse, H, valid, None, s["scale"], False,
                           s["p"], r["seed"], False, None, kv_fused=True)


@pytest.mark.parametrize("name", ["129x191-valid-drop", "150-valid+causal-bias-drop"])
def test_deterministic(name):
    r = _run(name)
    O0, lse0, outs0 = r["raw"]
    O, lse, outs = _kernel(name, r["inp"], r["seed"])
    assert torch.equal(O, O0) and torch.equal(lse, lse0)
    for a, b in zip(outs[:3], outs0[:3]):
        assert torch.equal(a, b)


def test_wrappers_match_bindings():
    """The autograd wrappers (p = 0: no seed to control) give the bindings' bits."""
    from deepdfa_amd.ops import flash_attention_rect, flash_attention_rect_kv, flash_rect_usable

    r = _run("200-valid-bias")
    s = r["s"]
    q, k, v, dO, valid, bias_t = r["inp"]
    assert flash_rect_usable(q, 64) and not flash_rect_usable(q.float(), 64)
    assert not flash_rect_usable(q, 32)
    O0, _, outs0 = r["raw"]
    ql, kl, vl = (t.clone().requires_grad_() for t in (q, k, v))
    bl = bias_t.clone().requires_grad_()
    O = flash_attention_rect(ql, kl, vl, s["H"], valid=valid, bias=bl, scale=s["scale"])
    O.backward(dO)
    assert torch.equal(O, O0)
    for a, b in zip((ql, kl, vl), outs0[:3]):
        assert torch.equal(a.grad, b)
    assert sorted(s["valid"])[0] == 0 and s["B"] == 3   # <= 2 atomic addends: exact
    assert torch.equal(bl.grad, outs0[3])

    r = _run("32x128-valid")
    s = r["s"]
    q, k, v, dO, valid, _ = r["inp"]
    O0, _, outs0 = r["raw"]
    D = s["H"] * 64
    ql = q.clone().requires_grad_()
    kv = torch.cat([k, v], -1).contiguous().requires_grad_()
    O = flash_attention_rect_kv(ql, kv, s["H"], valid=valid, scale=s["scale"])
    O.backward(dO)
    assert torch.equal(O, O0) and torch.equal(ql.grad, outs0[0])
    assert torch.equal(kv.grad[..., :D], outs0[1]) and torch.equal(kv.grad[..., D:], outs0[2])


def test_binding_errors_on_the_gpu():
    ext = _ext()
    q = torch.zeros(2, 5, 128, dtype=bf, device=DEV)
    k = torch.zeros(2, 9, 128, dtype=bf, device=DEV)
    with pytest.raises(RuntimeError, match="causal needs Lq == Lk"):
        ext.flash_rect_fwd(q, k, k, 2, None, None, 1.0, True, 0.0, 0)
    with pytest.raises(RuntimeError, match="bias needs Lq == Lk"):
        ext.flash_rect_fwd(q, k, k, 2, None, torch.zeros(2, 9, 5, device=DEV), 1.0, False, 0.0, 0)
    with pytest.raises(RuntimeError, match="on Q's device"):
        ext.flash_rect_fwd(q, k, k, 2, torch.tensor([9, 9], dtype=torch.int32), None, 1.0,
                           False, 0.0, 0)
    with pytest.raises(RuntimeError, match="on one GPU"):
        ext.flash_rect_fwd(q, k.cpu(), k.cpu(), 2, None, None, 1.0, False, 0.0, 0)


# --------------------------------------------------------------------------
# F. dbias_accum
# --------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["150-valid+causal-bias-drop", "200-valid-bias"])
def test_dbias_accum(name):
    r = _run(name)
    s, ext = r["s"], _ext()
    q, k, v, dO, valid, bias_t = r["inp"]
    B, H, L = s["B"], s["H"], s["Lq"]
    O, lse, outs0 = r["raw"]
    G = outs0[3].double()
    g0 = torch.randn(H, L, L, generator=torch.Generator().manual_seed(5)).to(DEV)
    buf = g0.clone()
    t = 2
    for _ in range(t):
        outs = ext.flash_rect_bwd(dO, q, k, v, O, lse, H, valid, bias_t, s["scale"], s["causal"],
                                  s["p"], r["seed"], True, buf)
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
# memory: no (B, H, Lq, Lk) tensor
# --------------------------------------------------------------------------

def test_no_score_tensor_is_allocated():
    from deepdfa_amd.ops import flash_attention_rect_kv

    B, H, Lq, Lk = 8, 12, 448, 513
    D = H * 64
    g = torch.Generator().manual_seed(9)
    q = (torch.randn(B, Lq, D, generator=g) * 0.5).to(bf).to(DEV).requires_grad_()
    kv = (torch.randn(B, Lk, 2 * D, generator=g) * 0.5).to(bf).to(DEV).requires_grad_()
    dO = torch.randn(B, Lq, D, generator=g).to(bf).to(DEV)
    valid = torch.tensor([513, 512, 449, 448, 65, 64, 1, 0], dtype=torch.int32, device=DEV)
    limit = B * H * Lq * Lk * 2          # one bf16 (B, H, Lq, Lk) tensor
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = flash_attention_rect_kv(q, kv, H, valid=valid, scale=0.125, dropout_p=P_DROP)
    out.backward(dO)
    torch.cuda.synchronize()
    used = torch.cuda.max_memory_allocated() - before
    print(f"[memory] forward + backward peak {used / 2**20:.1f} MiB, limit {limit / 2**20:.1f} MiB")
    assert 0 < used < limit, (used, limit)
    assert bool(torch.isfinite(q.grad).all()) and bool(torch.isfinite(kv.grad).all())
    assert float(kv.grad[7].abs().max()) == 0 and float(out[7].abs().max()) == 0


# --------------------------------------------------------------------------
# model level: lengths off the grid run the general kernels
# --------------------------------------------------------------------------

class _Counter:
    """Counts calls of ext.flash_rect_fwd (and of the tuned forward)."""

    def __init__(self, monkeypatch):
        ext = _ext()
        self.rect, self.tuned = [], 0
        rect, tuned = ext.flash_rect_fwd, ext.flash_attn_fwd

        def count_rect(Q, K, *a):
            self.rect.append((Q.shape[1], K.shape[1]))
            return rect(Q, K, *a)

        def count_tuned(*a):
            self.tuned += 1
            return tuned(*a)

        monkeypatch.setattr(ext, "flash_rect_fwd", count_rect)
        monkeypatch.setattr(ext, "flash_attn_fwd", count_tuned)


def _rel(got, ref):
    return float((got.float().cpu() - ref).abs().max() / ref.abs().max().clamp(min=1e-8))


_T5 = {}
T5_BATCH = 128


def _t5_run():
    """One T5 step at source length 100 (padded), target length 37, on the CPU
    in fp32 and on the GPU under bf16 autocast: the flash_rect_fwd calls, both
    losses and err = max |grad - ref| / max |ref| per parameter.

    128 sequences, because the max-norm comparison of a ReLU FFN's weight
    grads needs them: bf16 rounding moves a few pre-activations across 0, and
    each flipped gate adds or removes one token's whole contribution to a row
    of the wi.weight grad. With few tokens one token can carry most of a row.
    The same model under bf16 autocast on the CPU (no GPU code) against fp32
    gives for the worst wi.weight 0.40 at 3 sequences, 0.15 at 8, 0.09 at 32,
    0.057 at 64 and 0.029 at 128 (worst parameter overall 0.038): the
    deviation falls with the square root of the token count, and 128 leaves
    the 0.08 of test_t5_shared_bias_grad_matches_cpu a factor of 2. At 3
    sequences the MI355X gave 0.39 there with every attention parameter at
    0.01 to 0.05."""
    if _T5:
        return _T5
    from deepdfa_amd.models.t5 import T5Config, T5ForConditionalGeneration

    torch.manual_seed(0)
    cfg = T5Config(num_layers=2, num_decoder_layers=2, d_model=128, d_ff=256,
                   num_heads=2, vocab_size=500, dropout_rate=0.0)
    assert cfg.d_kv == 64
    cpu = T5ForConditionalGeneration(cfg)
    gpu = T5ForConditionalGeneration(cfg)
    gpu.load_state_dict(cpu.state_dict())
    gpu = gpu.to(DEV)
    src = torch.randint(3, cfg.vocab_size, (T5_BATCH, 100))
    for i, n in enumerate([100, 99, 65, 64, 63, 50, 37, 30] * (T5_BATCH // 8)):
        src[i, n:] = cfg.pad_token_id
    tgt = torch.randint(3, cfg.vocab_size, (T5_BATCH, 37))
    cpu.train()
    loss_c = cpu(src, labels=tgt)[0]
    loss_c.backward()
    gpu.train()
    with pytest.MonkeyPatch.context() as mp:
        counter = _Counter(mp)
        with torch.autocast(device_type="cuda", dtype=bf):
            loss_g = gpu(src.to(DEV), labels=tgt.to(DEV))[0]
        loss_g.backward()
        torch.cuda.synchronize()
    pc = dict(cpu.named_parameters())
    errs = {}
    for name, p in gpu.named_parameters():
        ref = pc[name].grad
        assert p.grad is not None and ref is not None and float(ref.abs().max()) > 0, name
        errs[name] = _rel(p.grad, ref)
        print(f"[t5] {name}: {errs[name]:.4f}")
    print(f"[t5] loss gpu {float(loss_g):.5f} cpu {float(loss_c):.5f}")
    _T5.update(rect=sorted(counter.rect), tuned=counter.tuned, loss_g=float(loss_g),
               loss_c=float(loss_c), errs=errs)
    return _T5


def test_t5_off_the_grid_runs_the_general_kernels():
    """Every attention layer runs flash_rect_fwd once (encoder self x2, decoder
    self x2, decoder cross x2) and none the tuned set."""
    r = _t5_run()
    assert r["rect"] == [(37, 37), (37, 37), (37, 100), (37, 100), (100, 100), (100, 100)]
    assert r["tuned"] == 0


def test_t5_off_the_grid_matches_cpu():
    """Loss and ALL parameter grads under bf16 autocast against the same model
    on the CPU in fp32, within test_t5_shared_bias_grad_matches_cpu's 0.08 of
    the largest reference entry; that includes both shared relative-bias
    tables."""
    r = _t5_run()
    assert abs(r["loss_g"] - r["loss_c"]) < 0.08 * abs(r["loss_c"])
    assert sum("relative_attention_bias" in n for n in r["errs"]) == 2
    worst = max(r["errs"], key=r["errs"].get)
    print(f"[t5] worst parameter grad {worst}: {r['errs'][worst]:.4f}")
    for n, e in r["errs"].items():
        assert e < 0.08, (n, e)


def _match_cpu(cpu_mod, gpu_mod, run, inputs):
    """forward + backward of `run(module, *inputs)` on both; outputs, input
    grads and parameter grads within 0.08 of the largest reference entry."""
    # activations are bf16 on the GPU, as the models cast them under autocast
    xc = [t.to(bf).float().requires_grad_() if t.is_floating_point() else t for t in inputs]
    xg = [t.to(bf).to(DEV).requires_grad_() if t.is_floating_point() else t.to(DEV)
          for t in inputs]
    out_c = run(cpu_mod, *xc)
    g = torch.randn(out_c.shape, generator=torch.Generator().manual_seed(3))
    out_c.backward(g)
    with torch.autocast(device_type="cuda", dtype=bf):
        out_g = run(gpu_mod, *xg)
    out_g.backward(g.to(DEV).to(out_g.dtype))
    torch.cuda.synchronize()
    assert _rel(out_g, out_c.detach()) < 0.08
    for a, b in zip(xg, xc):
        if b.is_floating_point():
            assert _rel(a.grad, b.grad) < 0.08
    pc = dict(cpu_mod.named_parameters())
    for name, p in gpu_mod.named_parameters():
        ref = pc[name].grad
        if name.endswith("key.bias"):
            # a key bias shifts every score of a row by the same q . b_k: the
            # softmax does not see it and the exact gradient is 0. Both sides
            # hold rounding noise only; measure it on the query bias's scale
            ref_q = pc[name.replace("key.bias", "query.bias")].grad.abs().max()
            assert float(ref.abs().max()) < 1e-3 * float(ref_q), name
            assert float(p.grad.abs().max().cpu()) < 0.08 * float(ref_q), name
            continue
        assert float(ref.abs().max()) > 0, name
        assert _rel(p.grad, ref) < 0.08, name


def test_roberta_layer_off_the_grid(monkeypatch):
    from deepdfa_amd.models.roberta import RobertaConfig, RobertaLayer, init_roberta_weights

    torch.manual_seed(1)
    cfg = RobertaConfig(vocab_size=100, hidden_size=128, num_hidden_layers=1,
                        num_attention_heads=2, intermediate_size=256,
                        hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    cpu = RobertaLayer(cfg)
    init_roberta_weights(cpu, std=0.1)
    gpu = RobertaLayer(cfg)
    gpu.load_state_dict(cpu.state_dict())
    gpu = gpu.to(DEV)
    x = torch.randn(3, 100, 128)
    valid = torch.tensor([100, 64, 7], dtype=torch.int32)
    counter = _Counter(monkeypatch)
    _match_cpu(cpu.train(), gpu.train(), lambda m, x, v: m(x, v)[0], (x, valid))
    assert counter.rect == [(100, 100)] and counter.tuned == 0
    # fp32 and output_attentions keep the materialised path
    with torch.no_grad():
        out, probs = gpu(x.to(DEV), valid.to(DEV), output_attentions=True)
    assert out.dtype == torch.float32 and tuple(probs.shape) == (3, 2, 100, 100)
    assert counter.rect == [(100, 100)]


def test_seq2seq_decoder_layer_off_the_grid(monkeypatch):
    from deepdfa_amd.models.roberta import RobertaConfig, init_roberta_weights
    from deepdfa_amd.models.seq2seq import Seq2SeqDecoderLayer

    torch.manual_seed(2)
    cfg = RobertaConfig(vocab_size=100, hidden_size=128, num_hidden_layers=1,
                        num_attention_heads=2, intermediate_size=256,
                        hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    cpu = Seq2SeqDecoderLayer(cfg)
    init_roberta_weights(cpu, std=0.1)
    gpu = Seq2SeqDecoderLayer(cfg)
    gpu.load_state_dict(cpu.state_dict())
    gpu = gpu.to(DEV)
    x = torch.randn(3, 37, 128)
    mem = torch.randn(3, 100, 128)
    valid = torch.tensor([100, 65, 3], dtype=torch.int32)
    counter = _Counter(monkeypatch)
    _match_cpu(cpu.train(), gpu.train(), lambda m, x, mem, v: m(x, mem, v), (x, mem, valid))
    assert counter.rect == [(37, 37), (37, 100)] and counter.tuned == 0
