"""The transformer row kernels (csrc/transformer_kernels.hip) and colsum
(csrc/flowgnn_kernels.hip) against the float64 oracles of
tests/transformer_oracle.py, at the smallest shapes that reach each code path.

Every comparison is elementwise through oracle_checks.assert_within, with

    bound = max(MARGIN * yardstick, floor) + derived + half ulp(IO dtype)

  yardstick  the same op as plain fp32 torch on the device, its error against
             the oracle taken as the maximum over the row (over the whole
             vector for the column reductions dgamma, dbeta, dbias, colsum)
  MARGIN     4, the margin of the flash and GGNN oracle tests
  floor      LayerNorm only: the conditioning floor
             4 (|mean| / sqrt(var + eps)) 2^-24 scaled by the magnitude of
             the output's terms: what one fp32 ulp of the row mean leaves
  derived    the roundings that can be counted, from the oracle's own
             quantities: a few 2^-24 of the terms of an elementwise
             expression; depth 2^-24 sum|terms| for a summation whose longest
             chain of additions is `depth` (per lane D/64 terms then a 6-step
             wave reduction; per column a 64-row chunk then one atomic per
             row block); the published 1.5e-7 of the Abramowitz-Stegun erf
             and the 2 ulp of __expf for GELU; half an ulp of the IO dtype
             for an intermediate the kernels keep in that dtype (the saved P
             of the softmax, z of LN(dropout(h)+res) for dgamma, dx under
             bias_gelu's dbias)
  half ulp   the rounding of the output itself, at |ref| + the rest

No element is excluded. Masked, dropped, padded and unused entries carry a
zero bound and are checked for exact zeros as well. eps and the dropout scale
enter the oracle with the fp32 / byte-quantised values the kernels use.

Each check records (kernel error net of the output's half ulp) / (yardstick
row error) and the share of its bound that was used; test_zz_ratio_table
prints the worst of both per op and dtype (the table in docs/KERNELS.md).
"""

import functools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import transformer_oracle as TO
from oracle_checks import assert_within, worst_ratio

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
bf = torch.bfloat16
f32 = torch.float32
f64 = torch.float64
DTYPES = [pytest.param(f32, id="fp32"), pytest.param(bf, id="bf16")]
U = 2.0 ** -24
MARGIN = 4.0
SEED = 0x5EED1234ABCD
ERF_ERR = 1.5e-7 + 8 * U  # A-S 7.1.26 + its fp32 evaluation and __expf
RATIOS = {}


def _ext():
    from deepdfa_amd.ops import load_ext

    return load_ext(required=True)


def _T():
    from deepdfa_amd.ops import transformer

    return transformer


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _vec(dt):
    return 4 if dt == f32 else 8


def _name(dt):
    return "fp32" if dt == f32 else "bf16"


@pytest.fixture
def fixed_seed(monkeypatch):
    monkeypatch.setattr(_T(), "_next_seed", lambda: SEED)
    return SEED


@functools.lru_cache(maxsize=None)
def _keep(shape, p):
    """float64 keep mask on the device; built once per (shape, p)."""
    return TO.keep_tensor(tuple(shape), SEED, p, DEV)


def _grads(fn, args, dy, dtype=None):
    """fn on detached copies of `args` (cast to `dtype` if given), backward
    with dy (None: out.sum()); returns (out, [grad per argument])."""
    leaves = [(a.detach().to(dtype) if dtype else a.detach()).requires_grad_(True)
              for a in args]
    out = fn(*leaves)
    if dy is None:
        out.sum().backward()
    else:
        out.backward(dy.to(out.dtype))
    return out.detach(), [leaf.grad for leaf in leaves]


def _check(op, dt, what, got, ref, yard, derived=0.0, floor=None, rows=True):
    ref = ref.double()
    yerr = (yard.double() - ref).abs()
    yrow = yerr.amax(-1, keepdim=True) if (rows and ref.dim() > 1) else yerr.max()
    core = MARGIN * yrow
    if floor is not None:
        core = torch.maximum(core, floor)
    core = (core + derived).expand_as(ref)
    hu = TO.half_ulp(ref.abs() + core, dt if got.dtype == dt else got.dtype)
    bound = core + hu
    # recorded, never asserted on: the kernel's error net of its output
    # rounding over the yardstick's (rows the yardstick gets exactly are left
    # to `used`), and the largest share of any bound that was used up
    if ref.numel():
        net = ((got.double() - ref).abs() - hu).clamp_min(0.0)
        net = net.amax(-1, keepdim=True) if (rows and ref.dim() > 1) else net.max()
        ratio = float(torch.where(yrow > 0, net / yrow.clamp_min(1e-300),
                                  torch.zeros_like(net)).max())
        used = worst_ratio(got, ref, bound)
    else:
        ratio = used = 0.0
    key = (op, _name(dt))
    old = RATIOS.get(key, (0.0, 0.0))
    RATIOS[key] = (max(old[0], ratio), max(old[1], used))
    print(f"{op:10s} {_name(dt)} {what:34s} kernel/yardstick {ratio:8.3f} err/bound {used:6.3f}")
    assert_within(got, ref, bound, f"{op} {_name(dt)} {what}")


# ---------------------------------------------------------------------------
# LayerNorm, RMSNorm
# ---------------------------------------------------------------------------

NORM_N = (1, 5, 67, 130)        # 4-rows-per-block tail, 64-row wgrad chunk tail
# D: < 64, scalar path, 1 and 3 register-cached vector iterations, a partial
# second wgrad column block, and 1280 > 1024: the vector path that re-reads
NORM_D = (40, 200, 256, 300, 768, 1000, 1280)


def _ln_terms(z, w, dy, eps, N, D, mean=True):
    """Magnitudes the LayerNorm / RMSNorm bounds are built from (float64)."""
    mu = z.mean(-1, keepdim=True) if mean else torch.zeros_like(z[..., :1])
    sd = torch.sqrt(((z - mu) ** 2).mean(-1, keepdim=True) + eps)
    xh, rs = (z - mu) / sd, 1.0 / sd
    g = dy * w
    mg, mgx = g.abs().mean(-1, keepdim=True), (g * xh).abs().mean(-1, keepdim=True)
    absdx = rs * (g.abs() + (1 + xh.abs()) * ((mg if mean else 0.0) + mgx))
    cond = 4.0 * mu.abs() / sd * U  # one ulp of the mean, in units of xhat
    depth = math.ceil(D / 64) + 7
    depthc = 20 + math.ceil(N / 64)
    return dict(
        xh=xh, rs=rs, cond=cond, absdx=absdx,
        y=4 * U * (xh * w).abs(),
        y_floor=cond * (xh * w).abs().amax(-1, keepdim=True).clamp_min(w.abs().max()),
        dx=(depth + 4) * U * absdx, dx_floor=cond * absdx,
        dgamma=depthc * U * (dy * xh).abs().sum(0) + (dy.abs() * cond * (1 + xh.abs())).sum(0),
        dbeta=depthc * U * dy.abs().sum(0),
    )


def _norm_case(op, dt, kind, eps, N, D, seed, noncontig=False, sum_loss=False):
    T = _T()
    g = _gen(seed)
    x = TO.ill_rows(kind, N, D, g, dt)
    if noncontig:  # every other column of a twice-as-wide tensor
        x = torch.stack([x, torch.full_like(x, 7.0)], -1).to(DEV)[..., 0]
        assert not x.is_contiguous() or x.numel() == 1
    else:
        x = x.to(DEV)
    w = (1 + 0.2 * torch.randn(D, generator=g)).to(DEV)
    b = (0.3 * torch.randn(D, generator=g)).to(DEV)
    dy = None if sum_loss else torch.randn(N, D, generator=g).to(dt).to(DEV)
    e32 = float(np.float32(eps))
    if op == "layer_norm":
        args = [x, w, b]
        ref_fn = lambda x, w, b: TO.layer_norm(x, w, b, e32)
        yard_fn = lambda x, w, b: F.layer_norm(x, (D,), w, b, e32)
        ker_fn = lambda x, w, b: T.layer_norm(x, w, b, eps)
    else:
        args = [x, w]
        ref_fn = lambda x, w: TO.rms_norm(x, w, e32)
        yard_fn = ref_fn
        ker_fn = lambda x, w: T.rms_norm(x, w, eps)
    ref, gref = _grads(ref_fn, args, dy, f64)
    yard, gyard = _grads(yard_fn, args, dy, f32)
    got, ggot = _grads(ker_fn, args, dy)
    dy64 = torch.ones_like(ref) if dy is None else dy.double()
    t = _ln_terms(x.double(), w.double(), dy64, e32, N, D, mean=(op == "layer_norm"))
    tag = f"{kind} N{N} D{D} eps{eps:g}"
    ln = op == "layer_norm"
    assert got.dtype == dt and ggot[0].dtype == dt and ggot[1].dtype == f32
    _check(op, dt, f"y {tag}", got, ref, yard,
           t["y"] + (2 * U * b.double().abs() if ln else 0.0), t["y_floor"] if ln else None)
    _check(op, dt, f"dx {tag}", ggot[0], gref[0], gyard[0], t["dx"],
           t["dx_floor"] if ln else None)
    _check(op, dt, f"dgamma {tag}", ggot[1], gref[1], gyard[1], t["dgamma"], rows=False)
    if ln:
        _check(op, dt, f"dbeta {tag}", ggot[2], gref[2], gyard[2], t["dbeta"], rows=False)
        if kind == "const":  # var == 0: y is beta, up to the output rounding
            assert_within(got, b.double().expand(N, D), TO.half_ulp(b.double().expand(N, D), dt),
                          "constant rows")


def _norm_params():
    out = []
    for dt in (f32, bf):
        for kind in ("normal", "m30", "m100", "const"):
            if kind == "m100" and dt == bf:
                continue  # fp32 only: bf16 cannot hold 100 +- 0.01
            for eps in (1e-5, 1e-12):
                out.append(pytest.param(dt, kind, eps, id=f"{_name(dt)}-{kind}-eps{eps:g}"))
    return out


@pytest.mark.parametrize("dt,kind,eps", _norm_params())
def test_layer_norm(dt, kind, eps):
    for i, N in enumerate(NORM_N):
        for j, D in enumerate(NORM_D):
            _norm_case("layer_norm", dt, kind, eps, N, D, 100 + 10 * i + j)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("kind", ["normal", "m30", "m100", "const"])
def test_rms_norm(dt, kind):
    if kind == "m100" and dt == bf:
        kind = "m30"  # bf16 cannot hold 100 +- 0.01; run the nearest family
    for i, N in enumerate(NORM_N):
        for j, D in enumerate(NORM_D):
            _norm_case("rms_norm", dt, kind, 1e-6, N, D, 200 + 10 * i + j)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("op", ["layer_norm", "rms_norm"])
def test_norm_noncontiguous_x_and_stride0_dy(op, dt):
    eps = 1e-5 if op == "layer_norm" else 1e-6
    for D in (300, 768):
        _norm_case(op, dt, "normal", eps, 67, D, 300 + D, noncontig=True)
        _norm_case(op, dt, "normal", eps, 67, D, 400 + D, sum_loss=True)
        _norm_case(op, dt, "m30", eps, 5, D, 500 + D, noncontig=True, sum_loss=True)


# ---------------------------------------------------------------------------
# LN(dropout(h) + res)
# ---------------------------------------------------------------------------

def _lnrd_case(dt, kind, N, D, p, seed, eps=1e-5):
    T = _T()
    g = _gen(seed)
    h = (0.05 * torch.randn(N, D, generator=g)).to(dt).to(DEV)
    res = TO.ill_rows(kind, N, D, g, dt).to(DEV)
    w = (1 + 0.2 * torch.randn(D, generator=g)).to(DEV)
    b = (0.3 * torch.randn(D, generator=g)).to(DEV)
    dy = torch.randn(N, D, generator=g).to(dt).to(DEV)
    e32 = float(np.float32(eps))
    keep, ds = _keep((N, D), p), TO.drop_scale(p)
    args = [h, res, w, b]
    ref, gref = _grads(lambda h, r, w, b: TO.layer_norm_res_dropout(h, r, w, b, e32, keep, ds),
                       args, dy, f64)
    yard, gyard = _grads(lambda h, r, w, b: F.layer_norm(
        h * keep.float() * np.float32(ds) + r, (D,), w, b, e32), args, dy, f32)
    got, ggot = _grads(lambda h, r, w, b: T.layer_norm_res_dropout(h, r, w, b, p, eps), args, dy)
    z = h.double() * keep * ds + res.double()
    t = _ln_terms(z, w.double(), dy.double(), e32, N, D)
    # z itself carries the roundings of h * dscale and of the add: in xhat units
    zr = 3 * U * (h.double().abs() * ds + res.double().abs()) * t["rs"]
    wa = w.double().abs()
    tag = f"{kind} N{N} D{D} p{p}"
    op = "ln_res_drop"
    _check(op, dt, f"y {tag}", got, ref, yard, t["y"] + 2 * U * b.double().abs() + zr * wa,
           t["y_floor"])
    # ... and moves dz as a shift of xhat by the row's largest zr does
    dz_extra = t["dx"] + zr.amax(-1, keepdim=True) * t["absdx"]
    _check(op, dt, f"dres {tag}", ggot[1], gref[1], gyard[1], dz_extra, t["dx_floor"])
    # dh = keep * dscale * dz, computed from the fp32 dz (not the rounded one)
    _check(op, dt, f"dh {tag}", ggot[0], gref[0], gyard[0], dz_extra * keep * ds,
           t["dx_floor"] * keep * ds)
    assert bool((ggot[0][keep == 0] == 0).all()), "dh must be exactly 0 where dropped"
    # the wgrad reads z as the backward kernel stored it, in the IO dtype
    zq = (dy.double().abs() * t["rs"] * TO.half_ulp(z, dt)).sum(0)
    _check(op, dt, f"dgamma {tag}", ggot[2], gref[2], gyard[2],
           t["dgamma"] + zq + (dy.double().abs() * zr).sum(0), rows=False)
    _check(op, dt, f"dbeta {tag}", ggot[3], gref[3], gyard[3], t["dbeta"], rows=False)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("p", [0.0, 0.1, 0.5])
def test_layer_norm_res_dropout(dt, p, fixed_seed):
    kinds = ("normal", "m30", "m100") if dt == f32 else ("normal", "m30")
    for k, kind in enumerate(kinds):
        for i, N in enumerate((1, 67)):
            for j, D in enumerate((256, 768, 1280)):  # 1280: rows too wide to cache
                _lnrd_case(dt, kind, N, D, p, 600 + 100 * k + 10 * i + j)


@pytest.mark.parametrize("dt", DTYPES)
def test_layer_norm_res_dropout_fallback_d200(dt, fixed_seed):
    """D % 256 != 0 takes the composed path (LayerNorm kernel on h + res);
    in bf16 that path rounds h + res to the IO dtype before the LayerNorm."""
    T = _T()
    g = _gen(77)
    N, D = 67, 200
    h = torch.randn(N, D, generator=g).to(dt).to(DEV)
    res = torch.randn(N, D, generator=g).to(dt).to(DEV)
    w = (1 + 0.2 * torch.randn(D, generator=g)).to(DEV)
    b = (0.3 * torch.randn(D, generator=g)).to(DEV)
    e32 = float(np.float32(1e-5))
    z = (h + res)  # the fallback's own intermediate, in the IO dtype
    ref = TO.layer_norm(z.double(), w.double(), b.double(), e32)
    yard = F.layer_norm(z.float(), (D,), w, b, e32)
    got = T.layer_norm_res_dropout(h, res, w, b, 0.0, 1e-5)
    t = _ln_terms(z.double(), w.double(), torch.ones_like(ref), e32, N, D)
    _check("ln_res_drop", dt, "y fallback D200", got, ref, yard,
           t["y"] + 2 * U * b.double().abs(), t["y_floor"])
    if dt == f32:  # no intermediate rounding: equals the oracle of the fused op
        ref2 = TO.layer_norm_res_dropout(h.double(), res.double(), w.double(), b.double(), e32)
        _check("ln_res_drop", dt, "y fallback D200 vs fused oracle", got, ref2, yard,
               t["y"] + 2 * U * b.double().abs() + 3 * U * t["rs"] * w.double().abs()
               * (h.double().abs() + res.double().abs()), t["y_floor"])


# ---------------------------------------------------------------------------
# bias + GELU, dbias through colsum
# ---------------------------------------------------------------------------

def _gelu_inputs(dt, N, D, seed):
    g = _gen(seed)
    x = (torch.rand(N, D, generator=g) * 24 - 12)
    x[:, 0] = 0.0
    x[:, 1] = -0.0
    if dt == bf and D > 8:
        x[:, 2] = 40.0
        x[:, 3] = -40.0
        x[:, 4] = 39.75
        x[:, 5] = -40.25
    bias = torch.randn(D, generator=g)
    bias[:2] = 0.0
    dy = torch.randn(N, D, generator=g)
    return x.to(dt).to(DEV), bias.to(DEV), dy.to(dt).to(DEV)


def _gelu_case(dt, N, D, seed):
    T = _T()
    x, bias, dy = _gelu_inputs(dt, N, D, seed)
    ref, gref = _grads(TO.bias_gelu, [x, bias], dy, f64)
    yard, gyard = _grads(lambda x, b: F.gelu(x + b), [x, bias], dy, f32)
    got, ggot = _grads(T.bias_gelu, [x, bias], dy)
    v = (x.double() + bias.double())
    va, dya = v.abs(), dy.double().abs()
    tag = f"N{N} D{D}"
    d_y = 0.5 * va * ERF_ERR + 1.13 * U * va + 2 * U * ref.abs()
    _check("bias_gelu", dt, f"y {tag}", got, ref, yard, d_y)
    d_dx = dya * (0.5 * ERF_ERR + 4 * U + U * va) + 2 * U * gref[0].abs()
    _check("bias_gelu", dt, f"dx {tag}", ggot[0], gref[0], gyard[0], d_dx)
    # dbias = colsum of dx AS STORED (IO dtype): every row's dx bound, rounding
    # included, plus the column summation
    dx_bound = d_dx + MARGIN * (gyard[0].double() - gref[0]).abs().amax(-1, keepdim=True)
    dx_bound = dx_bound + TO.half_ulp(gref[0].abs() + dx_bound, dt)
    d_db = dx_bound.sum(0) + (20 + math.ceil(N / 32)) * U * gref[0].abs().sum(0)
    _check("bias_gelu", dt, f"dbias {tag}", ggot[1], gref[1], gyard[1], d_db, rows=False)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("N,D", [(1, 8), (3, 1000), (67, 3072)])
def test_bias_gelu(dt, N, D):
    _gelu_case(dt, N, D, 900 + N)


@pytest.mark.parametrize("dt", DTYPES)
def test_bias_gelu_outer_loop_wraps(dt):
    """(16384, 3080): nvec exceeds 4 * 4096 * 256 vectors-in-flight per pass,
    so the grid-stride loop runs again with the carried bias column, and
    (stride * VEC) % D != 0 makes that column wrap."""
    N, D = 16384, 3080
    stride = 4096 * 256
    assert (N * D) // _vec(dt) > 4 * stride and (stride * _vec(dt)) % D != 0
    _gelu_case(dt, N, D, 990)


# ---------------------------------------------------------------------------
# masked / causal softmax with dropout
# ---------------------------------------------------------------------------

SM_B, SM_H = 3, 2


def _scores(kind, shape, scale, gen, dt):
    if kind == "normal":
        s = torch.randn(shape, generator=gen) / scale
    elif kind == "big":  # +-3e4 after scaling
        s = (torch.randint(0, 2, shape, generator=gen) * 2 - 1) * (3e4 / scale)
    elif kind == "equal":
        s = torch.full(shape, 1.25 / scale)
    elif kind == "neginf":
        s = torch.randn(shape, generator=gen) / scale
        s[0, 0, 0, :] = -float("inf")
        s[1, 1, -1, :] = -float("inf")
        s[..., 1] = -float("inf")
        s[2, 0, 0, ::2] = -float("inf")
    return s.to(dt).to(DEV)


def _softmax_case(dt, L, Lq, valid, causal, p, kind, scale, seed):
    T = _T()
    g = _gen(seed)
    S = _scores(kind, (SM_B, SM_H, Lq, L), scale, g, dt)
    dPd = torch.randn(S.shape, generator=g).to(dt).to(DEV)
    vt = None if valid is None else torch.tensor(valid, dtype=torch.int32, device=DEV)
    keep = _keep(tuple(S.shape), p) if TO.p8_of(p) else None
    ds = TO.drop_scale(p)
    tag = f"L{L} Lq{Lq} valid{valid} causal{int(causal)} p{p} {kind}"

    def run(dtype):
        leaf = S.detach().to(dtype).requires_grad_(True)
        P, Pd = TO.masked_softmax_dropout(leaf, vt, scale, None if keep is None else
                                          keep.to(dtype), ds, causal)
        Pd.backward(dPd.to(dtype))
        return P.detach(), Pd.detach(), leaf.grad

    P, Pd, dS = run(f64)
    yP, yPd, ydS = run(f32)
    leaf = S.detach().clone().requires_grad_(True)
    gP, gPd = T.masked_softmax_dropout(leaf, vt, scale, p, causal)
    gPd.backward(dPd)
    gdS = leaf.grad
    # derived: exp argument rounding + __expf (|s - m| + 8) 2^-23, the row sum
    depth = math.ceil(L / 64) + 7
    s = S.double() * scale
    sm = torch.where(P > 0, s, torch.zeros_like(s))
    m = torch.where(P > 0, s, torch.full_like(s, -1e300)).amax(-1, keepdim=True)
    rel = ((sm - torch.where(P > 0, m, torch.zeros_like(s))).abs() + 8 + depth) * 2 * U
    dP_ = P * rel
    _check("softmax", dt, f"P {tag}", gP, P, yP, dP_)
    k = 1.0 if keep is None else keep * ds
    _check("softmax", dt, f"Pd {tag}", gPd, Pd, yPd, dP_ * k + 2 * U * Pd)
    # backward reads P as stored (IO dtype): bP is P's full bound
    bP = dP_ + MARGIN * (yP.double() - P).abs().amax(-1, keepdim=True) * (P > 0)
    bP = bP + TO.half_ulp(P + bP, dt) * (P > 0)
    dP = dPd.double() * k
    dot = (dP * P).sum(-1, keepdim=True)
    d_dS = scale * (bP * (dP - dot).abs() + P * (dP.abs() * bP).sum(-1, keepdim=True)
                    + (depth + 4) * U * P * ((dP * P).abs().sum(-1, keepdim=True) + dP.abs()))
    _check("softmax", dt, f"dS {tag}", gdS, dS, ydS, d_dS)
    # structure: masked columns exactly 0 everywhere, dropped entries 0 in Pd
    col = torch.arange(L, device=DEV).view(1, 1, 1, L)
    masked = torch.zeros(S.shape, dtype=torch.bool, device=DEV)
    if vt is not None:
        masked |= col >= vt.view(-1, 1, 1, 1)
    if causal:
        masked |= col > torch.arange(Lq, device=DEV).view(1, 1, Lq, 1)
    for name, t in (("P", gP), ("Pd", gPd), ("dS", gdS)):
        assert bool((t[masked] == 0).all()), f"{name} not 0 at masked columns: {tag}"
    if keep is not None:
        assert bool((gPd[keep == 0] == 0).all()), f"dropped entries not 0: {tag}"
        live = (keep == 1) & (P > 2.0 ** -100)
        assert bool((gPd[live] > 0).all()), f"kept entries dropped: {tag}"
    if valid is not None and valid[-1] == 0:
        assert float(gP[-1].abs().max()) == 0.0 and float(gdS[-1].abs().max()) == 0.0


def _softmax_L():
    return [pytest.param(dt, L, id=f"{_name(dt)}-L{L}")
            for dt, Ls in ((bf, (8, 72, 520, 2048)), (f32, (4, 36, 260, 1024))) for L in Ls]


@pytest.mark.parametrize("dt,L", _softmax_L())
def test_masked_softmax_dropout(dt, L, fixed_seed):
    part = 5 if dt == f32 else 9
    v3 = [L, min(part, L), 0]
    q = min(L, 64)
    #        Lq      valid causal p    scores    scale
    cfgs = [(q,      v3,   False, 0.0, "normal", 0.125),
            (q,      None, False, 0.1, "normal", 1.0),
            (q,      v3,   False, 0.5, "neginf", 0.125),
            (q,      None, False, 0.5, "big",    0.125),
            (q,      v3,   False, 0.1, "equal",  1.0),
            (q,      None, False, 0.0, "neginf", 1.0),
            (L,      v3,   True,  0.0, "normal", 0.125),
            (L,      None, True,  0.0, "big",    1.0),
            (L // 2, v3,   True,  0.5, "equal",  0.125),
            (L // 2, None, True,  0.1, "neginf", 1.0)]
    for i, (Lq, valid, causal, p, kind, scale) in enumerate(cfgs):
        _softmax_case(dt, L, Lq, valid, causal, p, kind, scale, 1000 + i)


@pytest.mark.parametrize("dt", DTYPES)
def test_softmax_row_longer_than_supported_raises(dt):
    L = 64 * _vec(dt) * 4 + _vec(dt)
    S = torch.zeros(1, 1, 2, L, dtype=dt, device=DEV)
    with pytest.raises(RuntimeError, match="unsupported softmax row length"):
        _ext().softmax_mask_fwd(S, None, 1.0, 0.0, 0, False)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("p", [0.0, 0.5])
def test_softmax_valid_beyond_L_is_clamped(dt, p):
    """valid[b] > L must act as valid[b] = L. S is the leading rows of a
    larger buffer whose trailing rows hold +1e4: a read past the row stays
    inside the allocation and would swamp the softmax of the rows before."""
    ext = _ext()
    vec = _vec(dt)
    for L in (vec, 9 * vec):  # one partial vector iteration either way
        Lq = 8
        R = SM_B * SM_H * Lq
        pad_rows = (4 * 64 * vec) // L + 2
        buf = torch.full(((R + pad_rows) * L,), 1e4, dtype=dt, device=DEV)
        buf[:R * L] = torch.randn(R * L, generator=_gen(L)).to(dt).to(DEV)
        S = buf[:R * L].view(SM_B, SM_H, Lq, L)
        assert S.is_contiguous()
        exact = torch.tensor([L, L, L], dtype=torch.int32, device=DEV)
        over = torch.tensor([L + 1, 2 * L + 3, 2 ** 30], dtype=torch.int32, device=DEV)
        P0, Pd0 = ext.softmax_mask_fwd(S, exact, 0.125, p, SEED, False)
        P1, Pd1 = ext.softmax_mask_fwd(S, over, 0.125, p, SEED, False)
        assert torch.equal(P0, P1) and torch.equal(Pd0, Pd1)
        neg = torch.tensor([-1, -7, -2 ** 30], dtype=torch.int32, device=DEV)
        P2, _ = ext.softmax_mask_fwd(S, neg, 0.125, p, SEED, False)
        assert float(P2.abs().max()) == 0.0


# ---------------------------------------------------------------------------
# res + dropout(h), dropout(relu(x))
# ---------------------------------------------------------------------------

FLAT_SHAPES = [(8,), (8, 257), (16384, 768)]  # the last passes the 4096-block grid cap


def _tiny(x):
    flat = x.view(-1)
    vals = torch.tensor([-0.0, 0.0, 1e-30, -1e-30, 2.0 ** -120, -2.0 ** -120, 1.0, -1.0])
    flat[:8] = vals.to(x.dtype)
    return x


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("p", [0.0, 0.1, 0.5])
@pytest.mark.parametrize("shape", FLAT_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_dropout_add(dt, p, shape, fixed_seed):
    T = _T()
    g = _gen(1100)
    h = torch.randn(shape, generator=g).to(dt).to(DEV)
    res = torch.randn(shape, generator=g).to(dt).to(DEV)
    dy = torch.randn(shape, generator=g).to(dt).to(DEV)
    keep, ds = _keep(tuple(shape), p), TO.drop_scale(p)
    ref, gref = _grads(lambda h, r: TO.dropout_add(h, r, keep, ds), [h, res], dy, f64)
    yard, gyard = _grads(lambda h, r: TO.dropout_add(h, r, keep.float(), np.float32(ds)),
                         [h, res], dy, f32)
    got, ggot = _grads(lambda h, r: T.dropout_add(h, r, p), [h, res], dy)
    tag = f"{tuple(shape)} p{p}"
    _check("dropout_add", dt, f"out {tag}", got, ref, yard, 2 * U * (h.double() * keep * ds).abs())
    _check("dropout_add", dt, f"dh {tag}", ggot[0], gref[0], gyard[0], 2 * U * gref[0].abs())
    assert torch.equal(ggot[1], dy)  # d(res) passes through
    # the mask, exactly: dh is 0 where dropped and only there (dy has no zeros
    # to speak of; the few exact ones are excluded from the "kept" side only)
    assert torch.equal(ggot[0] == 0, (keep == 0) | (dy == 0))
    assert torch.equal(got[keep == 0], res[keep == 0])


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("p", [0.0, 0.1, 0.5])
@pytest.mark.parametrize("shape", FLAT_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_relu_dropout(dt, p, shape, fixed_seed):
    T = _T()
    g = _gen(1200)
    x = _tiny(torch.randn(shape, generator=g).to(dt)).to(DEV)
    dy = torch.randn(shape, generator=g).to(dt).to(DEV)
    keep, ds = _keep(tuple(shape), p), TO.drop_scale(p)
    ref, gref = _grads(lambda x: TO.relu_dropout(x, keep, ds), [x], dy, f64)
    yard, gyard = _grads(lambda x: TO.relu_dropout(x, keep.float(), np.float32(ds)), [x], dy, f32)
    got, ggot = _grads(lambda x: T.relu_dropout(x, p, True), [x], dy)
    tag = f"{tuple(shape)} p{p}"
    _check("relu_drop", dt, f"out {tag}", got, ref, yard, 2 * U * ref.abs())
    _check("relu_drop", dt, f"dx {tag}", ggot[0], gref[0], gyard[0], 2 * U * gref[0].abs())
    assert torch.equal(got == 0, (keep == 0) | (x <= 0))
    assert torch.equal(ggot[0] == 0, (keep == 0) | (x <= 0) | (dy == 0))


@pytest.mark.parametrize("dt", DTYPES)
def test_relu_dropout_partial_vector_and_empty(dt):
    """numel % (16-B vector) != 0 takes the composed path: every element is
    defined. The binding itself refuses such a tensor."""
    T = _T()
    x = torch.randn(3, 5, generator=_gen(5)).to(dt).to(DEV)
    y = T.relu_dropout(x, 0.0, True)
    assert torch.equal(y, torch.relu(x))
    xg = x.clone().requires_grad_(True)
    T.relu_dropout(xg, 0.0, True).backward(torch.ones_like(x))
    assert torch.equal(xg.grad, (x > 0).to(dt))
    yd = T.relu_dropout(x, 0.5, True).double()
    r2 = torch.relu(x).double() * 2
    assert bool(((yd == 0) | (yd == r2)).all())
    with pytest.raises(RuntimeError, match="multiple of the 16-B vector"):
        _ext().relu_dropout_fwd(x, 0.5, 1)
    with pytest.raises(RuntimeError, match="multiple of the 16-B vector"):
        _ext().relu_dropout_bwd(x, x, 0.5, 1)
    for shape in ((0,), (0, 8)):
        e = torch.empty(shape, dtype=dt, device=DEV, requires_grad=True)
        out = T.relu_dropout(e, 0.5, True)
        assert out.shape == e.shape and out.dtype == dt
        out.sum().backward()
        assert e.grad.shape == e.shape
        assert T.dropout_add(e.detach(), e.detach(), 0.5).shape == e.shape


# ---------------------------------------------------------------------------
# embedding scatter-add, relative-bias bucket reduce, column sum
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("D", [200, 256, 768])
@pytest.mark.parametrize("N", [1, 513])
def test_embed_scatter(dt, D, N):
    ext = _ext()
    V = 50
    g = _gen(1300 + D + N)
    dY = torch.randn(N, D, generator=g).to(dt).to(DEV)
    patterns = {
        "equal": (torch.full((N,), 7), None),
        "distinct": (torch.arange(N) % V, None),       # each row of dW hit N/V times
        "padding": (torch.where(torch.arange(N) % 3 == 0, 0, torch.randint(1, V, (N,), generator=g)), 0),
        "padding-none": (torch.randint(0, V, (N,), generator=g), None),
    }
    for name, (idx, pad) in patterns.items():
        idx = idx.to(DEV)
        ref = TO.embed_scatter(dY.double(), idx, V, pad)
        yard32 = TO.embed_scatter(dY.float(), idx, V, pad)
        absum = TO.embed_scatter(dY.double().abs(), idx, V, pad)
        cnt = int(torch.bincount(idx, minlength=V).max())
        got = ext.embed_scatter(dY, idx, V, -1 if pad is None else pad)
        assert got.dtype == f32
        _check("embed_scat", dt, f"{name} N{N} D{D}", got, ref, yard32, cnt * U * absum)
        if pad is not None:
            assert float(got[pad].abs().max()) == 0.0
        # out= adds into a pre-filled accumulator
        acc0 = torch.randn(V, D, generator=g).to(DEV)
        acc = acc0.clone()
        ret = ext.embed_scatter(dY, idx, V, -1 if pad is None else pad, out=acc)
        assert ret.data_ptr() == acc.data_ptr()
        _check("embed_scat", dt, f"{name} N{N} D{D} out=", acc, ref + acc0.double(),
               yard32 + acc0, (cnt + 1) * U * (absum + acc0.double().abs()))


@pytest.mark.parametrize("H", [1, 12, 16])
@pytest.mark.parametrize("QK", [64, 64 * 64 + 3])
def test_relbias_wgrad(H, QK):
    ext = _ext()
    NB = 32
    g = _gen(1400 + H + QK)
    dbias = torch.randn(H, QK, generator=g).to(DEV)
    patterns = {
        "one-bucket": torch.full((QK,), 5),
        "all-used": torch.arange(QK) % NB,
        "one-unused": torch.randint(0, NB - 1, (QK,), generator=g),
    }
    depth = min(QK, 8 + 4 + 256)  # per-wave LDS adds, 4 waves, 256 blocks' atomics
    for name, bk in patterns.items():
        bk = bk.to(torch.int32).to(DEV)
        ref = TO.relbias_wgrad(dbias.double(), bk, NB)
        yard = TO.relbias_wgrad(dbias, bk, NB)
        absum = TO.relbias_wgrad(dbias.double().abs(), bk, NB)
        got = ext.relbias_wgrad(dbias, bk, NB)
        assert got.shape == (NB, H)
        _check("relbias", f32, f"{name} H{H} QK{QK}", got, ref, yard, depth * U * absum)
        unused = torch.bincount(bk.long(), minlength=NB) == 0
        assert float(got[unused].abs().max() if unused.any() else 0.0) == 0.0
        if name == "one-unused":
            assert bool(unused[NB - 1])


def test_relbias_wgrad_rejects_more_than_16_heads():
    with pytest.raises(RuntimeError, match="at most 16 heads"):
        _ext().relbias_wgrad(torch.zeros(17, 64, device=DEV),
                             torch.zeros(64, dtype=torch.int32, device=DEV), 32)
    with pytest.raises(RuntimeError, match="LDS"):
        _ext().relbias_wgrad(torch.zeros(16, 64, device=DEV),
                             torch.zeros(64, dtype=torch.int32, device=DEV), 512)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("N", [1, 31, 33, 65, 4097])
def test_colsum(dt, N):
    ext = _ext()
    for C in (8, 64, 100, 128, 300, 384):
        g = _gen(1500 + N + C)
        x = torch.randn(N, C, generator=g).to(dt).to(DEV)
        ref = TO.colsum(x.double())
        yard = x.float().sum(0)
        derived = (20 + math.ceil(N / 32)) * U * x.double().abs().sum(0)
        got = ext.colsum(x)
        assert got.dtype == f32
        _check("colsum", dt, f"N{N} C{C}", got, ref, yard, derived, rows=False)
        acc0 = torch.randn(C, generator=g).to(DEV)
        acc = acc0.clone()
        ext.colsum(x, out=acc)
        _check("colsum", dt, f"N{N} C{C} out=", acc, ref + acc0.double(), yard + acc0,
               derived + U * (ref.abs() + acc0.double().abs()), rows=False)


# ---------------------------------------------------------------------------
# binding checks: every tensor argument, wrong dtype / shape / layout.
# All of these raise before any launch.
# ---------------------------------------------------------------------------

def _binding_table():
    """name -> (call(args), args, {arg position: mutations to skip})"""
    N, D, L = 6, 256, 16
    dev = dict(device=DEV)
    x = torch.zeros(N, D, **dev)
    vD = torch.zeros(D, **dev)
    vN = torch.zeros(N, **dev)
    S = torch.zeros(3, 2, 8, L, **dev)
    valid = torch.zeros(3, dtype=torch.int32, **dev)
    idx = torch.zeros(N, dtype=torch.long, **dev)
    db = torch.zeros(4, 64, **dev)
    bk = torch.zeros(64, dtype=torch.int32, **dev)
    e = _ext()
    solo = {0: ("shape",)}
    return {
        "layernorm_fwd": (lambda a: e.layernorm_fwd(*a, 1e-5), [x, vD, vD], {}),
        "layernorm_bwd": (lambda a: e.layernorm_bwd(*a), [x, x, vD, vN, vN], {}),
        "layernorm_wgrad": (lambda a: e.layernorm_wgrad(*a), [x, x, vN, vN], {}),
        "rmsnorm_fwd": (lambda a: e.rmsnorm_fwd(*a, 1e-6), [x, vD], {}),
        "rmsnorm_bwd": (lambda a: e.rmsnorm_bwd(*a), [x, x, vD, vN], {}),
        "rmsnorm_wgrad": (lambda a: e.rmsnorm_wgrad(*a), [x, x, vN], {}),
        "bias_gelu_fwd": (lambda a: e.bias_gelu_fwd(*a), [x, vD], {}),
        "bias_gelu_bwd": (lambda a: e.bias_gelu_bwd(*a), [x, x, vD], {}),
        "softmax_mask_fwd": (lambda a: e.softmax_mask_fwd(a[0], a[1], 1.0, 0.0, 0, False),
                             [S, valid], solo),
        "softmax_mask_bwd": (lambda a: e.softmax_mask_bwd(*a, 1.0, 0.0, 0), [S, S], {}),
        "ln_res_dropout_fwd": (lambda a: e.ln_res_dropout_fwd(*a, 1e-5, 0.1, 1),
                               [x, x, vD, vD], {}),
        "ln_res_dropout_bwd": (lambda a: e.ln_res_dropout_bwd(*a, 0.1, 1),
                               [x, x, x, vD, vN, vN], {}),
        "ln_res_dropout_wgrad": (lambda a: e.ln_res_dropout_wgrad(*a, 0.1, 1),
                                 [x, x, x, vN, vN], {}),
        "dropout_add_fwd": (lambda a: e.dropout_add_fwd(*a, 0.1, 1), [x, x], {}),
        "dropout_add_bwd": (lambda a: e.dropout_add_bwd(*a, 0.1, 1), [x], solo),
        "relu_dropout_fwd": (lambda a: e.relu_dropout_fwd(*a, 0.1, 1), [x], solo),
        "relu_dropout_bwd": (lambda a: e.relu_dropout_bwd(*a, 0.1, 1), [x, x], {}),
        "embed_scatter": (lambda a: e.embed_scatter(a[0], a[1], 10, -1), [x, idx],
                          {0: ("shape",)}),
        "relbias_wgrad": (lambda a: e.relbias_wgrad(a[0], a[1], 32), [db, bk], {}),
        "colsum": (lambda a: e.colsum(a[0]), [x], solo),
    }


def _mutate(t, how):
    if how == "dtype":
        if t.is_floating_point():
            return t.double()
        return t.long() if t.dtype == torch.int32 else t.int()
    if how == "layout":
        return torch.stack([t, t], -1)[..., 0]
    if t.dtype == torch.int32 and t.numel() == 3:  # valid: 2-D of the same length
        return t.view(-1, 1)
    return torch.cat([t, t], -1)  # a doubled last dimension


BINDINGS = ["layernorm_fwd", "layernorm_bwd", "layernorm_wgrad", "rmsnorm_fwd", "rmsnorm_bwd",
            "rmsnorm_wgrad", "bias_gelu_fwd", "bias_gelu_bwd", "softmax_mask_fwd",
            "softmax_mask_bwd", "ln_res_dropout_fwd", "ln_res_dropout_bwd",
            "ln_res_dropout_wgrad", "dropout_add_fwd", "dropout_add_bwd", "relu_dropout_fwd",
            "relu_dropout_bwd", "embed_scatter", "relbias_wgrad", "colsum"]


@pytest.mark.parametrize("name", BINDINGS)
def test_binding_rejects_bad_arguments(name):
    call, args, skip = _binding_table()[name]
    tried = 0
    for i, t in enumerate(args):
        for how in ("dtype", "shape", "layout"):
            if how in skip.get(i, ()):
                continue
            bad = list(args)
            bad[i] = _mutate(t, how)
            assert how != "layout" or not bad[i].is_contiguous()
            with pytest.raises(RuntimeError):
                call(bad)
            tried += 1
    assert tried >= 2 * len(args)


def test_binding_rejects_oversized_lds_and_bad_valid():
    e = _ext()
    D = 64 * 1024 // 4 + 8
    x = torch.zeros(1, D, dtype=bf, device=DEV)
    b = torch.zeros(D, device=DEV)
    with pytest.raises(RuntimeError, match="LDS"):
        e.bias_gelu_fwd(x, b)
    with pytest.raises(RuntimeError, match="LDS"):
        e.bias_gelu_bwd(x, x, b)
    with pytest.raises(RuntimeError, match="16-B vector"):
        e.bias_gelu_bwd(x[:, :12].contiguous(), x[:, :12].contiguous(), b[:12].contiguous())
    S = torch.zeros(3, 2, 8, 16, device=DEV)
    with pytest.raises(RuntimeError, match="divide"):
        e.softmax_mask_fwd(S, torch.zeros(5, dtype=torch.int32, device=DEV), 1.0, 0.0, 0, False)
    with pytest.raises(RuntimeError, match="256"):
        e.ln_res_dropout_fwd(torch.zeros(2, 200, device=DEV), torch.zeros(2, 200, device=DEV),
                             torch.zeros(200, device=DEV), torch.zeros(200, device=DEV),
                             1e-5, 0.0, 0)


def test_zz_ratio_table():
    """Prints the worst kernel / yardstick ratio per op and dtype seen by the
    tests above (empty when run alone)."""
    for (op, dt), (ratio, used) in sorted(RATIOS.items()):
        print(f"RATIO {op:12s} {dt} kernel/yardstick {ratio:10.3f}  err/bound {used:6.3f}")
