"""lmhead_topk_kernel / lmhead_topk_combine_kernel / beam_select_kernel
(csrc/lmhead_topk.hip), their ops and generate(select="fused") against float64
oracles.

Conventions of test_gpu_gemm_tiles.py: every reference is float64 on the GPU,
computed from the same bf16 inputs the kernel sees; every bound is computed
from those inputs and the reference, never from a kernel output; non-finite
outputs fail. ACC = 2^-23 per accumulated fp32 term, EPS_FN = 2^-20 per fp32
__expf / __logf, SECOND = 1 + 2^-7. With l_ij = scale sum_k h w in float64,
the fp32 error of one logit is rule J's
  d_ij = SECOND ((Kd + 2) ACC scale sum_k |h w| + ACC |l_ij|).

L  lmhead_topk, random cases (M, Kd, V, k, chunk) with M in {6, 128, 130},
   Kd in {64, 192}, V in {1000, 1060, 2048}, k in {1, 3, 10, 16}; chunk is the
   launcher's choice (one 128-column tile at these M) or pinned to the 8 tiles
   of lmhead_ce, which puts V = 1000's pad inside the only chunk and
   V = 1060's 36-column tail in a second one. Pad rows of Wp hold 8.0.
     lse        |got - ref| <= max_j d_ij + V ACC + 4 EPS_FN (rule J)
     values     |val_ic - l[i, idx_ic]| <= d[i, idx_ic]; columns distinct, in
                [0, V); values non-increasing along c
     selection  every column j not returned has
                l_ij - d_ij <= min_c (l[i, idx_ic] + d[i, idx_ic])
     index set  equals the reference's wherever the float64 gap between the
                k-th and (k+1)-th logit exceeds their two d's.
                test_fixture_gaps (CPU) asserts that holds for EVERY row of
                every random case, so the margin-aware rule hides nothing.
P  planted winners: h[:, 0] = 4 and one-hot W rows make four columns beat the
   rest of every row by >= 100 d (asserted), at column 0, V - 1, the last
   column of a chunk and the first of the next, the two halves of a tile row:
   all in one chunk, two per chunk, one per chunk. Index order exact.
T  ties: W rows duplicated inside a scanning thread's 64 columns, across
   tiles of one chunk and across chunks give bit-equal values (asserted on
   the output), returned smaller column first; the whole list equals the
   float64 stable sort.
S  determinism: two calls are bit-equal; outputs have exactly M rows; the op
   equals the binding; bad arguments raise.
B  beam_select: tokens, parents, done and score BITS equal the fp32 torch form
   on the same inputs, B in {1, 3}, K in {1, 3, 10}: no / some / all beams of
   a source finished, the step-0 scores [0, -1e9, ...], ties across parents
   and ranks, a candidate equal to eos.
G  generate(select="fused") as the drivers call it, greedy and 3 beams:
   repeatable, starts with the start token, greedy rows padded after eos, eos
   wins by step 3 with the patched vocabulary matrix. output_scores: each
   mode's own sequences are teacher-forced through a float64 CPU copy,
   e_mode = max |score - float64 log-probability|; e_fused <= 2 e_logits and
   e_logits > 0 (the parent's path is the yardstick, the 2 is the factor
   test_model_forced_decoding grants a fused path over its eager twin).

Observed on an MI355X, largest |got - ref| / bound: random cases lse 0.0039,
values 0.0126 (M=128 Kd=64 V=1060 k=10; the V ACC term dominates the lse
bound, and the MFMA accumulates far below the (Kd + 2) ACC worst case);
planted lse 0.0066, values 0 (exact); ties lse 0.0121, values 0.0308, and the
duplicated rows did give bit-equal logits in every position tried. G:
e_logits 3.99e-03, e_fused 9.41e-04.
"""

import copy

import pytest
import torch

from oracle_checks import assert_within, worst_ratio

gpu = pytest.mark.gpu

ACC = 2.0 ** -23
EPS_FN = 2.0 ** -20
SECOND = 1.0 + 2.0 ** -7
DEV = "cuda:0"
BF = torch.bfloat16

# (M, Kd, V, k, chunk_tiles); 0 = the launcher's choice
CASES = [
    (6, 64, 1000, 1, 0),
    (6, 192, 2048, 16, 0),
    (128, 192, 1060, 3, 8),
    (128, 64, 1060, 10, 2),
    (130, 64, 2048, 10, 8),
    (130, 192, 1000, 16, 8),
    (130, 192, 1060, 1, 0),
    (128, 64, 2048, 3, 0),
]
_CASE = {}


def _ext():
    from deepdfa_amd.ops import load_ext

    return load_ext(required=True)


def _reference(h, Wp, V, scale):
    """l, d, lse of the module docstring on the tensors' device."""
    Kd = h.shape[1]
    h64, w64 = h.double(), Wp[:V].double()
    l = scale * (h64 @ w64.t())
    d = SECOND * ((Kd + 2) * ACC * scale * (h64.abs() @ w64.abs().t()) + ACC * l.abs())
    return l, d, torch.logsumexp(l, dim=1)


def _inputs(M, Kd, V):
    Vp = (V + 127) // 128 * 128
    # the 9000 is chosen for test_fixture_gaps: with most seeds some row of
    # some case has its k-th and (k+1)-th logit within their two d's
    gen = torch.Generator().manual_seed(9000 + 11 * M + 3 * Kd + V)
    h = torch.randn(M, Kd, generator=gen).to(BF)
    Wp = torch.full((Vp, Kd), 8.0, dtype=BF)
    Wp[:V] = torch.randn(V, Kd, generator=gen).to(BF)
    return h, Wp


def _case(M, Kd, V, dev):
    """Inputs and float64 reference on `dev`; built once, never modified."""
    key = (M, Kd, V, dev)
    if key not in _CASE:
        h, Wp = _inputs(M, Kd, V)
        h, Wp = h.to(dev), Wp.to(dev)
        scale = Kd ** -0.5
        l, d, lse = _reference(h, Wp, V, scale)
        _CASE[key] = dict(h=h, Wp=Wp, scale=scale, l=l, d=d, lse=lse)
    return _CASE[key]


def _gaps(l, d, k):
    """Per row: float64 gap between the k-th and (k+1)-th logit, and the sum of
    their two d's."""
    top = torch.sort(l, dim=1, descending=True, stable=True)
    a, b = top.indices[:, k - 1:k], top.indices[:, k:k + 1]
    gap = (top.values[:, k - 1] - top.values[:, k])
    return gap, (d.gather(1, a) + d.gather(1, b))[:, 0], top.indices[:, :k]


def test_fixture_gaps():
    """CPU: in every row of every random case the k-th logit is separated from
    the (k+1)-th by more than their two d's, so test_lmhead_topk_random demands
    the exact index set of every row."""
    seen = {ax: set() for ax in "MKVk"}
    for M, Kd, V, k, ct in CASES:
        c = _case(M, Kd, V, "cpu")
        gap, dd, _ = _gaps(c["l"], c["d"], k)
        assert bool((gap > dd).all()), (M, Kd, V, k, float((gap / dd).min()))
        Vp = c["Wp"].shape[0]
        assert Vp == V or bool((c["Wp"][V:] == 8.0).all())
        for ax, v in zip("MKVk", (M, Kd, V, k)):
            seen[ax].add(v)
    assert seen == dict(M={6, 128, 130}, K={64, 192}, V={1000, 1060, 2048}, k={1, 3, 10, 16})
    assert 1000 - 7 * 128 == 104 and 1060 - 8 * 128 == 36


def _poison(M, k):
    """NaN-fill and free tensors of the outputs' sizes: the caching allocator
    hands the same blocks to the binding's at::empty, so a skipped store shows."""
    ts = [torch.full((M, k), float("nan"), device=DEV), torch.full((M,), float("nan"), device=DEV)]
    torch.cuda.synchronize()
    del ts


def _run(h, Wp, V, scale, k, ct):
    _poison(h.shape[0], k)
    val, idx, lse = _ext().lmhead_topk(h, Wp, V, scale, k, ct)
    torch.cuda.synchronize()
    M = h.shape[0]
    assert val.dtype == torch.float32 and idx.dtype == torch.int32 and lse.dtype == torch.float32
    assert tuple(val.shape) == (M, k) and tuple(idx.shape) == (M, k) and tuple(lse.shape) == (M,)
    return val, idx, lse


def _check_rules(what, val, idx, lse, l, d, lse_ref, V, k):
    assert bool(torch.isfinite(val).all()) and bool(torch.isfinite(lse).all()), what
    lse_bound = d.max(dim=1).values + V * ACC + 4 * EPS_FN
    r_lse = worst_ratio(lse, lse_ref, lse_bound)
    assert_within(lse, lse_ref, lse_bound, what + " lse")
    assert bool(((idx >= 0) & (idx < V)).all()), what + ": column outside [0, V)"
    li = idx.long()
    assert bool((torch.sort(li, dim=1).values.diff(dim=1) > 0).all()), what + ": repeated column"
    assert bool((val.diff(dim=1) <= 0).all()), what + ": values not non-increasing"
    l_sel, d_sel = l.gather(1, li), d.gather(1, li)
    r_val = worst_ratio(val, l_sel, d_sel)
    assert_within(val, l_sel, d_sel, what + " values")
    floor = (l_sel + d_sel).min(dim=1, keepdim=True).values
    rest = torch.ones_like(l, dtype=torch.bool).scatter_(1, li, False)
    excess = torch.where(rest, (l - d) - floor, torch.full_like(l, -1.0))
    assert float(excess.max()) <= 0.0, what + ": a column that must be selected is missing"
    print(f"{what}: max |got - ref| / bound lse {r_lse:.4f} values {r_val:.4f}")


@gpu
@pytest.mark.parametrize("M,Kd,V,k,ct", CASES)
def test_lmhead_topk_random(M, Kd, V, k, ct):
    c = _case(M, Kd, V, DEV)
    val, idx, lse = _run(c["h"], c["Wp"], V, c["scale"], k, ct)
    what = f"lmhead_topk M={M} Kd={Kd} V={V} k={k} chunk={ct}"
    _check_rules(what, val, idx, lse, c["l"], c["d"], c["lse"], V, k)
    gap, dd, want = _gaps(c["l"], c["d"], k)
    clear = gap > dd
    assert bool(clear.all())                            # test_fixture_gaps, on this device
    got_set = torch.sort(idx.long(), dim=1).values
    assert torch.equal(got_set[clear], torch.sort(want, dim=1).values[clear]), what + " index set"
    val2, idx2, lse2 = _run(c["h"], c["Wp"], V, c["scale"], k, ct)
    assert torch.equal(val, val2) and torch.equal(idx, idx2) and torch.equal(lse, lse2)


def _planted(cols_w0, extra=()):
    """M = 130, Kd = 64, V = 2048 (no pad), h[:, 0] = 4. Column j of cols_w0
    gets the one-hot row w0 e_0: its logit is scale * 4 * w0 in every row,
    exactly. `extra` = (dst, src) pairs: W[dst] = W[src] afterwards."""
    M, Kd, V = 130, 64, 2048
    h, Wp = _inputs(M, Kd, V)
    h[:, 0] = 4.0
    for j, w0 in cols_w0:
        Wp[j] = 0.0
        Wp[j, 0] = w0
    for dst, src in extra:
        Wp[dst] = Wp[src]
    h, Wp = h.to(DEV), Wp.to(DEV)
    scale = Kd ** -0.5
    return h, Wp, V, scale, _reference(h, Wp, V, scale)


@gpu
@pytest.mark.parametrize("name,ct,cols", [
    # chunk = 1024 columns: all four in chunk 0, on both sides of a half (63 | 64)
    ("one-chunk", 8, [(0, 28.0), (63, 40.0), (64, 32.0), (1023, 36.0)]),
    # two per chunk: column 0, last of chunk 0, first of chunk 1, V - 1
    ("two-chunks", 8, [(0, 32.0), (1023, 28.0), (1024, 40.0), (2047, 36.0)]),
    # chunk = 256 columns: one winner in each of chunks 0, 1 (its last column),
    # 2 (its first) and 7 (V - 1)
    ("one-per-chunk", 2, [(0, 36.0), (511, 40.0), (512, 28.0), (2047, 32.0)]),
    # the launcher's chunk (one tile): last column of chunk 0, first of chunk 1
    ("tile-chunks", 0, [(0, 40.0), (127, 28.0), (128, 36.0), (2047, 32.0)]),
])
def test_planted_winners(name, ct, cols):
    h, Wp, V, scale, (l, d, lse_ref) = _planted(cols)
    k = len(cols)
    order = [j for j, _ in sorted(cols, key=lambda c: -c[1])]
    planted = torch.zeros(V, dtype=torch.bool, device=DEV)
    planted[order] = True
    margin = l[:, planted].min(dim=1).values - l[:, ~planted].max(dim=1).values
    assert bool((margin >= 100 * d.max(dim=1).values).all())
    steps = l[:, order].diff(dim=1)
    assert bool((-steps >= 100 * d.max(dim=1, keepdim=True).values).all())
    val, idx, lse = _run(h, Wp, V, scale, k, ct)
    _check_rules(f"planted {name}", val, idx, lse, l, d, lse_ref, V, k)
    assert torch.equal(idx.long(), torch.tensor(order, device=DEV).expand(h.shape[0], k))
    assert torch.equal(val.double(), l[:, order])        # one exact product per logit


@gpu
@pytest.mark.parametrize("ct", [8, 0])
def test_ties_smaller_column_first(ct):
    """Three copies of one random W row with W[., 0] = 40 (columns 10 and 20:
    one scanning thread; 700: another tile of chunk 0 at ct = 8), two of another
    with 36 (900 | 1500: two chunks), one with 32 at V - 1. Every row's six
    largest logits are these, group against group by margins asserted here."""
    groups = [(10, 40.0), (900, 36.0), (2047, 32.0)]
    dups = [(20, 10), (700, 10), (1500, 900)]
    M, Kd, V = 130, 64, 2048
    h, Wp = _inputs(M, Kd, V)
    h[:, 0] = 4.0
    for j, w0 in groups:
        Wp[j] *= 0.25                                    # exact in bf16
        Wp[j, 0] = w0
    for dst, src in dups:
        Wp[dst] = Wp[src]
    h, Wp = h.to(DEV), Wp.to(DEV)
    scale = Kd ** -0.5
    l, d, lse_ref = _reference(h, Wp, V, scale)
    k = 6
    assert torch.equal(l[:, 10], l[:, 20]) and torch.equal(l[:, 10], l[:, 700])
    assert torch.equal(l[:, 900], l[:, 1500])
    top = torch.sort(l, dim=1, descending=True, stable=True)
    want = top.indices[:, :k]
    assert torch.equal(torch.sort(want, dim=1).values,
                       torch.tensor([10, 20, 700, 900, 1500, 2047], device=DEV).expand(M, k))
    # distinct neighbours of the first seven are further apart than their d's
    gap = -top.values[:, :k + 1].diff(dim=1)
    dd = d.gather(1, top.indices[:, :k]) + d.gather(1, top.indices[:, 1:k + 1])
    assert bool(((gap == 0) | (gap > dd)).all())
    val, idx, lse = _run(h, Wp, V, scale, k, ct)
    _check_rules(f"ties chunk={ct}", val, idx, lse, l, d, lse_ref, V, k)
    # equal W rows give bit-equal fp32 logits wherever they sit in a tile
    by_col = {j: val.gather(1, (idx == j).long().argmax(dim=1, keepdim=True))[:, 0]
              for j in (10, 20, 700, 900, 1500)}
    assert all(bool((idx == j).any(dim=1).all()) for j in by_col)
    assert torch.equal(by_col[10], by_col[20]) and torch.equal(by_col[10], by_col[700])
    assert torch.equal(by_col[900], by_col[1500])
    assert torch.equal(idx.long(), want), "ties must come smaller column first"


@gpu
def test_op_equals_binding_and_arguments():
    from deepdfa_amd.ops import lmhead_topk, lmhead_topk_usable

    M, Kd, V = 130, 64, 1060
    c = _case(M, Kd, V, DEV)
    weight = c["Wp"][:V].float()                         # exact: the op's bf16 cast restores Wp[:V]
    assert lmhead_topk_usable(c["h"], weight, 10)
    assert not lmhead_topk_usable(c["h"], weight, 17) and not lmhead_topk_usable(c["h"], weight, 0)
    assert not lmhead_topk_usable(c["h"][:, :32], weight[:, :32], 3)
    assert not lmhead_topk_usable(c["h"].cpu(), weight.cpu(), 3)
    Wz = c["Wp"].clone()
    Wz[V:] = 0                                           # the op's cache pads with zeros
    want = _run(c["h"], Wz, V, c["scale"], 10, 0)
    got = lmhead_topk(c["h"], weight, 10, c["scale"])
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    assert all(torch.equal(a, b) for a, b in zip(want, _run(c["h"], c["Wp"], V, c["scale"], 10, 0)))
    assert weight._dfa_vocab_cache[3].shape == (1152, Kd)
    got3 = lmhead_topk(c["h"].view(2, 65, Kd).float(), weight, 10, c["scale"], chunk_tiles=8)
    assert all(torch.equal(a, b) for a, b in zip(got3, _run(c["h"], Wz, V, c["scale"], 10, 8)))
    for k in (0, 17):
        with pytest.raises(ValueError):
            lmhead_topk(c["h"], weight, k)
    with pytest.raises(ValueError):
        lmhead_topk(c["h"], weight[:5], 6)
    with pytest.raises(ValueError):
        lmhead_topk(c["h"], weight.clone().requires_grad_(), 3)
    ext = _ext()
    h, Wp = c["h"], c["Wp"]
    for bad in (lambda: ext.lmhead_topk(h.float(), Wp, V, 1.0, 3, 0),
                lambda: ext.lmhead_topk(h, Wp.float(), V, 1.0, 3, 0),
                lambda: ext.lmhead_topk(h[:, :32].contiguous(), Wp[:, :32].contiguous(), V, 1.0, 3, 0),
                lambda: ext.lmhead_topk(h, Wp[:1100].contiguous(), V, 1.0, 3, 0),
                lambda: ext.lmhead_topk(h, Wp, 1153, 1.0, 3, 0),
                lambda: ext.lmhead_topk(h, Wp, 0, 1.0, 3, 0),
                lambda: ext.lmhead_topk(h, Wp, V, 1.0, 0, 0),
                lambda: ext.lmhead_topk(h, Wp, V, 1.0, 17, 0),
                lambda: ext.lmhead_topk(h, Wp, 2, 1.0, 3, 0),
                lambda: ext.lmhead_topk(h, Wp, V, 1.0, 3, -1),
                lambda: ext.lmhead_topk(h.cpu(), Wp, V, 1.0, 3, 0)):
        with pytest.raises(RuntimeError):
            bad()
    val, idx, lse = ext.lmhead_topk(h[:0], Wp, V, 1.0, 3, 0)
    assert tuple(val.shape) == (0, 3) and tuple(lse.shape) == (0,)


# --------------------------------------------------------------------------
# B. beam_select
# --------------------------------------------------------------------------

def _beam_inputs(B, K, seed, V=50):
    g = torch.Generator().manual_seed(seed)
    val = torch.randn(B * K, K, generator=g).sort(dim=1, descending=True).values
    idx = torch.stack([torch.randperm(V, generator=g)[:K] for _ in range(B * K)]).to(torch.int32)
    lse = val[:, 0] + torch.rand(B * K, generator=g)
    scores = -torch.rand(B, K, generator=g).cumsum(1)
    return val, idx, lse, scores


def _beam_both(val, idx, lse, scores, done, fill=0, eos=2):
    from deepdfa_amd.ops import beam_select

    want = beam_select(val, idx, lse, scores, done, fill, eos)          # fp32 torch form
    B, K = scores.shape
    ts = [torch.full((B * K,), -1, dtype=torch.long, device=DEV) for _ in range(2)]
    del ts
    got = beam_select(val.to(DEV), idx.to(DEV), lse.to(DEV), scores.to(DEV), done.to(DEV),
                      fill, eos)
    for g, w, name in zip(got, want, ("scores", "parent", "tok", "done")):
        assert g.dtype == w.dtype and g.shape == w.shape, name
        if name == "scores":
            assert torch.equal(g.cpu().view(torch.int32), w.view(torch.int32)), name
        else:
            assert torch.equal(g.cpu(), w), name
    return want


@gpu
@pytest.mark.parametrize("B,K", [(1, 1), (3, 1), (1, 3), (3, 3), (1, 10), (3, 10)])
def test_beam_select_equals_torch_form(B, K):
    val, idx, lse, scores = _beam_inputs(B, K, 10 * B + K)
    idx[0, 0] = 2                                        # the best candidate of row 0 is eos
    none = torch.zeros(B * K, dtype=torch.bool)
    s, p, t, d = _beam_both(val, idx, lse, scores, none)
    assert torch.equal(d, t == 2)
    some = none.clone()
    some[::2] = True
    _beam_both(val, idx, lse, scores, some)
    whole = none.clone()
    whole[(B - 1) * K:] = True                           # all beams of the last source
    s, p, t, d = _beam_both(val, idx, lse, scores, whole, fill=7)
    assert t[(B - 1) * K:].tolist() == [7] * K and torch.equal(s[B - 1], scores[B - 1])
    step0 = torch.full((B, K), -1e9)
    step0[:, 0] = 0.0
    s, p, t, d = _beam_both(val, idx, lse, step0, none)
    assert p.view(B, K).tolist() == [[b * K] * K for b in range(B)]


@gpu
def test_beam_select_ties():
    K = 3
    val = torch.tensor([[2.0, 1.0, 1.0], [2.0, 2.0, 0.0], [2.0, 1.0, 0.5]])
    idx = torch.tensor([[5, 6, 7], [8, 2, 9], [10, 11, 12]], dtype=torch.int32)
    lse = torch.full((3,), 4.0)
    s, p, t, d = _beam_both(val, idx, lse, torch.zeros(1, K), torch.zeros(3, dtype=torch.bool))
    assert p.tolist() == [0, 1, 1] and t.tolist() == [5, 8, 2] and d.tolist() == [False, False, True]
    s, p, t, d = _beam_both(val, idx, lse, torch.tensor([[-2.0, 0.0, 0.0]]),
                            torch.tensor([True, False, False]))
    assert p.tolist() == [0, 1, 1] and t.tolist() == [0, 8, 2]
    # ten parents, every candidate of every parent at the same total
    K = 10
    val = torch.zeros(K, K)
    idx = torch.arange(K * K, dtype=torch.int32).view(K, K)
    s, p, t, d = _beam_both(val, idx, torch.zeros(K), torch.zeros(1, K),
                            torch.zeros(K, dtype=torch.bool), eos=-1)
    assert p.tolist() == [0] * K and t.tolist() == list(range(K))
    ext = _ext()
    a = [x.to(DEV) for x in (val, idx, torch.zeros(K), torch.zeros(1, K),
                             torch.zeros(K, dtype=torch.bool))]
    for bad in (lambda: ext.beam_select(a[0].double(), a[1], a[2], a[3], a[4], 0, 2),
                lambda: ext.beam_select(a[0], a[1].long(), a[2], a[3], a[4], 0, 2),
                lambda: ext.beam_select(a[0], a[1], a[2], a[3], a[4].int(), 0, 2),
                lambda: ext.beam_select(a[0], a[1], a[2][:5].contiguous(), a[3], a[4], 0, 2),
                lambda: ext.beam_select(a[0][:, :4].contiguous(), a[1][:, :4].contiguous(), a[2],
                                        a[3], a[4], 0, 2),
                lambda: ext.beam_select(torch.zeros(17, 17, device=DEV),
                                        torch.zeros(17, 17, dtype=torch.int32, device=DEV),
                                        torch.zeros(17, device=DEV), torch.zeros(1, 17, device=DEV),
                                        torch.zeros(17, dtype=torch.bool, device=DEV), 0, 2)):
        with pytest.raises(RuntimeError):
            bad()


# --------------------------------------------------------------------------
# G. end to end
# --------------------------------------------------------------------------

def _small_t5(tie=True):
    from deepdfa_amd.models.t5 import T5Config, T5ForConditionalGeneration

    torch.manual_seed(0)
    cfg = T5Config(num_layers=2, num_decoder_layers=2, d_model=128, d_ff=256, num_heads=2,
                   vocab_size=200, tie_word_embeddings=tie)
    model = T5ForConditionalGeneration(cfg).eval()
    g = torch.Generator().manual_seed(1)
    ids = torch.randint(3, cfg.vocab_size, (2, 64), generator=g)
    ids[:, -1] = cfg.eos_token_id
    ids[1, 41:] = cfg.pad_token_id           # one ragged source
    return model, cfg, ids


@gpu
def test_generate_fused_as_the_drivers_call_it(monkeypatch):
    from deepdfa_amd.ops import transformer as T

    model, cfg, ids = _small_t5()
    model = model.to(DEV)
    src = ids.to(DEV)
    calls = []
    real = T.lmhead_topk_usable
    monkeypatch.setattr(T, "lmhead_topk_usable", lambda *a: calls.append(real(*a)) or calls[-1])
    assert not torch.is_autocast_enabled()
    for beams in (1, 3):
        for kv in ("auto", "concat"):
            out = model.generate(src, max_length=10, num_beams=beams, select="fused", kv_cache=kv)
            assert out.dtype == torch.long and out.shape[0] == 2 and 2 <= out.shape[1] <= 10
            assert bool((out[:, 0] == cfg.decoder_start_token_id).all())
            assert torch.equal(out, model.generate(src, max_length=10, num_beams=beams,
                                                   select="fused", kv_cache=kv))
    assert calls and all(calls), "the kernels did not serve the call"


@gpu
def test_greedy_fused_rows_are_padded_after_eos():
    """As test_greedy_rows_are_padded_after_eos of test_gpu_decode_attn.py,
    through select="fused"."""
    model, cfg, ids = _small_t5(tie=False)
    model = model.to(DEV)
    src = ids.to(DEV)
    first = model.generate(src, max_length=10, select="fused")
    tok = int(first[0, 3])
    with torch.no_grad():
        model.lm_head.weight[cfg.eos_token_id] = 1.25 * model.lm_head.weight[tok]
    out = model.generate(src, max_length=10, select="fused")
    row = out[0].tolist()
    assert cfg.eos_token_id in row[:4], row
    for r in out.tolist():
        if cfg.eos_token_id in r:
            assert all(t == cfg.pad_token_id for t in r[r.index(cfg.eos_token_id) + 1:]), r


def _tf_score(model64, cfg, ids, seq):
    """Float64 CPU log-probability of each row of seq up to and including its
    first eos, teacher-forced through decoder.decode_step on a concat state
    (the float64 path of the model: its full forward takes attention scores
    through fp32)."""
    from deepdfa_amd.models.t5 import _DecodeState

    scale = cfg.d_model ** -0.5 if cfg.tie_word_embeddings else 1.0
    with torch.no_grad():
        valid = ids.ne(cfg.pad_token_id).sum(1).to(torch.int32)
        enc = model64.encoder(ids, valid)
        state = _DecodeState(len(model64.decoder.block))
        total = torch.zeros(seq.shape[0], dtype=torch.float64)
        alive = torch.ones(seq.shape[0], dtype=torch.bool)
        for t in range(seq.shape[1] - 1):
            h = model64.decoder.decode_step(seq[:, t:t + 1], enc, valid, state)[:, -1]
            logp = torch.log_softmax(model64.lm_head(h * scale), -1)
            step = logp.gather(1, seq[:, t + 1:t + 2])[:, 0]
            total = total + torch.where(alive, step, torch.zeros_like(step))
            alive = alive & (seq[:, t + 1] != cfg.eos_token_id)
    return total


@gpu
def test_output_scores_against_float64_teacher():
    model, cfg, ids = _small_t5()
    model64 = copy.deepcopy(model).double()
    gpu_model = copy.deepcopy(model).to(DEV)
    src = ids.to(DEV)
    e = {}
    for mode in ("logits", "fused"):
        errs = []
        for beams in (1, 3):
            seq, score = gpu_model.generate(src, max_length=10, num_beams=beams, select=mode,
                                            output_scores=True)
            assert score.dtype == torch.float32 and tuple(score.shape) == (2,)
            assert bool(torch.isfinite(score).all())
            ref = _tf_score(model64, cfg, ids, seq.cpu())
            errs.append(float((score.double().cpu() - ref).abs().max()))
        e[mode] = max(errs)
    print(f"[scores] e_logits {e['logits']:.4e} e_fused {e['fused']:.4e}")
    assert e["logits"] > 0.0
    assert e["fused"] <= 2.0 * e["logits"]
