"""The glds-pipeline GEMM kernels against float64 oracles, elementwise:
gemm2 on both row tiles, lmhead_ce_fwd and lmhead_ce_bwd (csrc/mfma_tile.h,
gemm_bf16.hip, lmhead_ce.hip). The register-staged family is pinned by rule H
and the fused-loop rules of test_gpu_ggnn.py.

Conventions of test_gpu_ggnn.py: every reference is float64 on the GPU,
computed from the same bf16 inputs the kernels see; every bound is computed
from those inputs and the reference, never from a kernel output; non-finite
outputs fail. u = 2^-8 (bf16 unit roundoff), 2^-23 per accumulated fp32 term,
eps_fn = 2^-20 per fp32 __expf / __logf evaluation, second-order factor
1 + 2^-7.

I  gemm2           rule H with the fp32 bias b:
                     |got - ref| <= (1 + 2^-7)(u |ref| + (K+2) 2^-23
                                               (sum_k |a w| + |b|)).
                   With an addend the kernel rounds A W^T + b to bf16, adds
                   the bf16 addend in fp32 and rounds to bf16 again, so against
                   ref = ref0 + addend (ref0 the reference without it) the
                   bound above, taken on ref0, widens by u (|ref0| + |addend|).
                   launch_gemm2 takes the 64-row tile below 512 blocks of
                   128 x 128 and the 128-row tile from there on; K = 64 is one
                   slice (no prefetch), 128 uses both buffers once, 192 ends
                   on the other buffer parity.
J  lmhead_ce_fwd   l_ij = scale sum_k h w (float64), and the fp32 error of
                   one logit
                     d_ij = (1 + 2^-7)((K+2) 2^-23 scale sum_k |h w|
                                       + 2^-23 |l_ij|).
                   lse:  |got - ref| <= max_j d_ij + V 2^-23 + 4 eps_fn
                     (moving every logit by <= d moves logsumexp by <= d; the
                     V-term fp32 sum of positive values errs relatively by
                     <= V 2^-24; the __expf / __logf evaluations and the chunk
                     merges add a few eps_fn)
                   loss: the lse bound + d_i,tgt + 2^-22 (|lse| + |l_i,tgt|);
                     exactly 0 on ignored rows (target -1).
K  lmhead_ce_bwd   teacher-forced: lse is the float32 rounding of the reference
                   lse, p = exp(l - lse32) in float64, ref = (p - onehot) g:
                     |got - ref| <= u |ref| + (1 + 2^-7) |g| p (d + 2^-23
                                    (|l| + |lse|) + eps_fn) + 2^-22 |ref|;
                   columns >= V and rows with g = 0 are exactly 0.

The pad rows V..Vp-1 of the vocabulary matrix hold 8.0, not zeros: only the
kernels' mask by V keeps them out of the result.

Largest |got - ref| / bound observed on an MI355X, per rule. The commit
before the kernels moved onto mfma_tile.h gives the same figures: the
kernels' outputs are bit-identical on both.
  I  64-row tile 0.980 (256x64x384, bias), 128-row tile 0.985 (K = 64, bias),
     with addend 0.970 (128-row tile)
  J  lse 0.0044, loss 0.0043 (both M=256 K=64 V=1000; the V 2^-23 term
     dominates the bound)
  K  0.988 (M=128 K=64 V=2048)
The ratios of I and K sit just under 1 because u |ref| is the exact
worst case of one round-to-nearest bf16 store and the fp32 terms are small.
"""

import pytest
import torch

from oracle_checks import assert_within, worst_ratio

pytestmark = pytest.mark.gpu

U16 = 2.0 ** -8
ACC = 2.0 ** -23
EPS_FN = 2.0 ** -20
SECOND = 1.0 + 2.0 ** -7
DEV = "cuda:0"
BF = torch.bfloat16


def _ext():
    from deepdfa_amd.ops import load_ext

    return load_ext(required=True)


def _check(got, ref, bound, what):
    print(f"{what}: max |got - ref| / bound = {worst_ratio(got, ref, bound):.4f}")
    assert_within(got, ref, bound, what)


# --------------------------------------------------------------------------
# I. gemm2
# --------------------------------------------------------------------------

_GEMM2 = {}


def _gemm2_case(N, K, COL):
    """Inputs, float64 product and magnitude sum; built once, never modified."""
    key = (N, K, COL)
    if key not in _GEMM2:
        gen = torch.Generator().manual_seed(N + 7 * K + COL)
        A = torch.randn(N, K, generator=gen).to(BF).to(DEV)
        W = (0.1 * torch.randn(COL, K, generator=gen)).to(BF).to(DEV)
        b = torch.randn(COL, generator=gen).to(DEV)
        add = torch.randn(N, COL, generator=gen).to(BF).to(DEV)
        _GEMM2[key] = dict(A=A, W=W, b=b, add=add, prod=A.double() @ W.double().t(),
                           mag=A.double().abs() @ W.double().abs().t())
    return _GEMM2[key]


def _gemm2_check(N, K, COL, with_bias, with_addend=False):
    c = _gemm2_case(N, K, COL)
    ref, mag = c["prod"], c["mag"]
    if with_bias:
        ref, mag = ref + c["b"].double(), mag + c["b"].double().abs()
    bound = SECOND * (U16 * ref.abs() + (K + 2) * ACC * mag)
    if with_addend:
        bound = bound + U16 * (ref.abs() + c["add"].double().abs())
        ref = ref + c["add"].double()
    got = _ext().gemm2(c["A"], c["W"], c["b"] if with_bias else None,
                       c["add"] if with_addend else None)
    assert got.dtype == BF
    _check(got, ref, bound, f"gemm2 {N}x{K}x{COL} bias={with_bias} addend={with_addend}")


def _blocks128(N, COL):
    return (N // 128) * (COL // 128)


@pytest.mark.parametrize("with_bias", [True, False])
@pytest.mark.parametrize("K", [64, 128, 192])
@pytest.mark.parametrize("COL", [128, 384])
@pytest.mark.parametrize("N", [128, 256])
def test_gemm2_64row_tile(N, COL, K, with_bias):
    assert _blocks128(N, COL) < 512
    _gemm2_check(N, K, COL, with_bias)


@pytest.mark.parametrize("with_bias", [True, False])
@pytest.mark.parametrize("K", [64, 128, 192])
def test_gemm2_128row_tile(K, with_bias):
    assert _blocks128(1024, 8192) == 512    # the first shape past the switch
    _gemm2_check(1024, K, 8192, with_bias)


@pytest.mark.parametrize("N,K,COL", [(256, 192, 384), (1024, 192, 8192)])
def test_gemm2_addend(N, K, COL):
    _gemm2_check(N, K, COL, True, with_addend=True)


# --------------------------------------------------------------------------
# J, K. lmhead_ce
# --------------------------------------------------------------------------

_CE = {}
CE_SHAPES = [(M, K, V) for M in (128, 256) for K in (64, 192) for V in (1000, 1060, 2048)]


def _ce_case(M, K, V):
    key = (M, K, V)
    if key in _CE:
        return _CE[key]
    Vp = (V + 127) // 128 * 128
    gen = torch.Generator().manual_seed(M + 3 * K + V)
    h = torch.randn(M, K, generator=gen).to(BF)
    Wp = torch.full((Vp, K), 8.0, dtype=BF)
    Wp[:V] = torch.randn(V, K, generator=gen).to(BF)
    tgt = torch.randint(0, V, (M,), generator=gen, dtype=torch.int32)
    second_chunk = min(1030, V - 2)         # in chunk 1 whenever there is one
    for i, t in enumerate((-1, 0, V - 1, second_chunk, -1)):
        tgt[i] = t
        tgt[M - 1 - i] = t
    g = torch.randn(M, generator=gen)
    g[tgt < 0] = 0.0
    g[7] = 0.0                              # a live row with zero upstream grad
    h, Wp, tgt, g = h.to(DEV), Wp.to(DEV), tgt.to(DEV), g.to(DEV)
    scale = K ** -0.5
    h64, w64 = h.double(), Wp[:V].double()
    l = scale * (h64 @ w64.t())
    d = SECOND * ((K + 2) * ACC * scale * (h64.abs() @ w64.abs().t()) + ACC * l.abs())
    lse = torch.logsumexp(l, dim=1)
    live = tgt >= 0
    idx = tgt.clamp_min(0).long()[:, None]
    l_tgt, d_tgt = l.gather(1, idx)[:, 0], d.gather(1, idx)[:, 0]
    _CE[key] = dict(h=h, Wp=Wp, tgt=tgt, g=g, scale=scale, Vp=Vp, l=l, d=d, lse=lse,
                    live=live, idx=idx, l_tgt=l_tgt, d_tgt=d_tgt)
    return _CE[key]


def test_lmhead_ce_fixtures():
    for V, Vp, chunks in ((1000, 1024, 1), (1060, 1152, 2), (2048, 2048, 2)):
        c = _ce_case(128, 64, V)
        assert c["Vp"] == Vp and (Vp // 128 + 7) // 8 == chunks
        t = c["tgt"].tolist()
        assert -1 in t and 0 in t and V - 1 in t
        assert chunks == 1 or any(x >= 1024 for x in t)
        assert Vp == V or bool((c["Wp"][V:] == 8.0).all())
    assert 1000 - 7 * 128 == 104 and 1060 - 8 * 128 == 36


@pytest.mark.parametrize("M,K,V", CE_SHAPES)
def test_lmhead_ce_fwd(M, K, V):
    c = _ce_case(M, K, V)
    loss, lse = _ext().lmhead_ce_fwd(c["h"], c["Wp"], c["tgt"], c["scale"], V)
    assert loss.dtype == torch.float32 and lse.dtype == torch.float32
    what = f"lmhead_ce_fwd M={M} K={K} V={V}"
    lse_bound = c["d"].max(dim=1).values + V * ACC + 4 * EPS_FN
    _check(lse, c["lse"], lse_bound, what + " lse")
    live = c["live"]
    assert bool((loss[~live] == 0).all()), "ignored rows must be exactly 0"
    loss_ref = torch.where(live, c["lse"] - c["l_tgt"], torch.zeros_like(c["lse"]))
    loss_bound = lse_bound + c["d_tgt"] + 2.0 ** -22 * (c["lse"].abs() + c["l_tgt"].abs())
    loss_bound = torch.where(live, loss_bound, torch.zeros_like(loss_bound))
    _check(loss, loss_ref, loss_bound, what + " loss")


@pytest.mark.parametrize("M,K,V", CE_SHAPES)
def test_lmhead_ce_bwd(M, K, V):
    c = _ce_case(M, K, V)
    lse32 = c["lse"].float()
    got = _ext().lmhead_ce_bwd(c["h"], c["Wp"], c["tgt"], lse32, c["g"], c["scale"], V)
    assert got.dtype == BF and got.shape == (M, c["Vp"])
    assert bool((got[:, V:] == 0).all()), "columns >= V must be exactly 0"
    assert bool((got[c["g"] == 0] == 0).all()), "rows with gscale = 0 must be exactly 0"
    g = c["g"].double()[:, None]
    lse = lse32.double()[:, None]
    p = torch.exp(c["l"] - lse)
    onehot = torch.zeros_like(p)
    onehot.scatter_(1, c["idx"], c["live"].double()[:, None])
    ref = (p - onehot) * g
    bound = (U16 * ref.abs()
             + SECOND * g.abs() * p * (c["d"] + ACC * (c["l"].abs() + lse.abs()) + EPS_FN)
             + 2.0 ** -22 * ref.abs())
    _check(got[:, :V], ref, bound, f"lmhead_ce_bwd M={M} K={K} V={V}")
