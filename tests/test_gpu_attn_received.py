"""flash_received_kernel (csrc/flash_attn.hip) and everything built on it
against the float64 oracle of tests/attn_received_oracle.py.

    R[b, h, j] = sum_i P[b, h, i, j]     the attention key j receives

Every reference is float64 on the GPU, computed from the SAME values the
kernel sees: q, k are bf16 tensors, the bias an fp32 tensor. Every bound is
computed from those inputs and the references, never from a kernel output.
Constants as in test_gpu_flash.py: ACC = 2^-23 per accumulated fp32 term,
EPS_FN = 2^-20 for an fp32 __expf, SECOND = 1 + 2^-7 for second-order terms,
LSE_MARGIN = 4. Outputs come from at::empty; NaN-filled tensors of the output
size are allocated and freed just before each call so a skipped store shows.

Shapes: d = 64; L = 64 (one key tile, half-empty strip interleave), 128, 192
(three key tiles, odd strip count per interleaved wave under causal), 320
(five tiles); (B, H) = (3, 3), so gridDim.x * H is no multiple of 8 in the
(b, h, tile) decode, and one (2, 12) case. q, k ~ 0.5 N(0,1), bias ~ N(0,1).

A  the kernel alone, every element, lse = the oracle's rounded to fp32:
     |got_j - R_j| <= SECOND sum_i P_ij ( d_ij + ACC |lse_i| + ACC |s_ij - lse_i|
                                          + EPS_FN + (L + 8) ACC ) + 1e-30
     d_ij = (64 + 2) ACC ( scale sum_d |q_i k_j| + |bias_hji| )
   d_ij is the fp32 score error (64 products, the scale, the bias add), the
   two ACC terms the fp32 lse input and the rounding of the subtraction,
   EPS_FN __expf, (L + 8) ACC the fp32 accumulation over L rows plus the four
   lane hops and the wave-pair add. Nothing is rounded to bf16. The bound
   cannot hide a structural defect: bound <= 2^-12 R wherever R > 0 is
   asserted (a missed 32-row strip or 16-key fragment moves R by percents).
   Exact zeros: keys >= valid[b], the whole valid = 0 batch row, and under
   valid = 1 every key but 0.
B  with the forward kernel's own lse: A's bound plus SECOND LSE_MARGIN y R_j,
   y = max_rows |lse_fp32 - lse_f64| the fp32 yardstick of test_gpu_flash.py's
   lse test (an lse error e scales every P of that row by exp(e)); that is
   what that test already guarantees of the forward kernel.
C  q, k as slices of one (B, L, 3D) buffer: torch.equal to contiguous copies.
D  two calls on the same inputs: torch.equal (no atomics).
E  flash_attention_received_qkv: O torch.equal to flash_attention_qkv at
   dropout_p = 0, R torch.equal to the raw binding on the forward's lse;
   ValueError with grad enabled on a leaf that requires grad.
F  the model under bf16 autocast: the materialised branch is not entered,
   prob is unchanged, each layer's R passes bound B against the oracle on that
   layer's recorded qkv, padded key columns are exactly 0.
G  attention_line_scores_batched equals the head sum and index_add_ done by
   hand in float64 on R, within H L T 2^-23 relative (T tokens on the line).

Observed on an MI355X, largest |err| / bound: A 0.003 .. 0.008 over the seven
cases, B 0.004 .. 0.009, F 0.023 per layer; largest bound / R 1.62e-4
(2^-12 = 2.44e-4).
"""

import math

import pytest
import torch

import attn_received_oracle as RO
import flash_oracle as FO

pytestmark = pytest.mark.gpu

bf = torch.bfloat16
ACC = 2.0 ** -23
EPS_FN = 2.0 ** -20
SECOND = 1.0 + 2.0 ** -7
LSE_MARGIN = 4.0
DEV = "cuda:0"


def _ext():
    from deepdfa_amd.ops import load_ext

    return load_ext(required=True)


# --------------------------------------------------------------------------
# cases, built once and never modified
# --------------------------------------------------------------------------

def _spec(B, H, L, valid, bias, causal, scale):
    return dict(B=B, H=H, L=L, valid=valid, bias=bias, causal=causal, scale=scale)


SPECS = {
    "L64-valid": _spec(3, 3, 64, [64, 63, 1], False, False, 1.0),
    "L128-valid-bias-causal": _spec(3, 3, 128, [128, 65, 0], True, True, 1.0),
    "L192-none": _spec(3, 3, 192, None, False, False, 1.0),
    "L192-valid-bias-scale": _spec(3, 3, 192, [192, 191, 64], True, False, 0.125),
    "L320-valid-bias-causal": _spec(3, 3, 320, [320, 65, 1], True, True, 1.0),
    "L128-H12-valid-bias": _spec(2, 12, 128, [127, 64], True, False, 1.0),
    "L320-none": _spec(3, 3, 320, None, False, False, 1.0),
}
ALL = list(SPECS)
# B: one with bias, one causal, one with valid
FWD_LSE_CASES = ["L192-valid-bias-scale", "L128-valid-bias-causal", "L64-valid"]

_CASES = {}


def _poison(*shapes_dtypes):
    """Allocate, NaN-fill and free tensors of the coming outputs' sizes: the
    caching allocator hands the same blocks to the kernel's at::empty."""
    ts = [torch.full(s, float("nan"), dtype=dt, device=DEV) for s, dt in shapes_dtypes]
    torch.cuda.synchronize()
    del ts


def _oracle(q, k, H, valid, bias_t, scale, causal):
    """Reference R and the elementwise bound A (both float64 (B, H, L)), plus
    the oracle's lse, from the bf16 q, k (B, L, H*64) and the kernel-layout
    fp32 bias the kernel sees."""
    L = q.shape[1]
    q64, k64 = FO.to_bhld(q, H), FO.to_bhld(k, H)
    bias = None if bias_t is None else FO.bias_from_kernel(bias_t)
    R, P, lse, s = RO.received_exact(q64, k64, valid, bias, scale, causal)
    mag, gap = RO.received_bound_terms(q64, k64, P, lse, s, bias, scale)
    fac = (64 + 2) * ACC * mag + ACC * lse.abs().unsqueeze(-1) + ACC * gap + EPS_FN + (L + 8) * ACC
    bound = SECOND * (P * fac).sum(dim=-2) + 1e-30
    return R, bound, lse


def _lse_yardstick(q, k, H, valid, bias_t, scale, causal, lse64):
    """y of test_gpu_flash.py's lse test: the same log-sum-exp evaluated in
    fp32 by torch from the same inputs, max over live rows of its error."""
    B, L, _ = q.shape
    q32 = q.float().view(B, L, H, 64).transpose(1, 2)
    k32 = k.float().view(B, L, H, 64).transpose(1, 2)
    sc = (q32 @ k32.transpose(-1, -2)) * scale
    if bias_t is not None:
        sc = sc + bias_t.transpose(-1, -2).unsqueeze(0)
    sc = sc.masked_fill(FO.masked_keys(B, L, valid, causal, DEV), float("-inf"))
    y32 = torch.logsumexp(sc, -1).double()
    vl = valid if valid is not None else torch.full((B,), L, device=DEV)
    live = (vl > 0).view(-1, 1, 1).expand_as(lse64)
    return float((y32 - lse64)[live].abs().max())


def _case(name):
    if name in _CASES:
        return _CASES[name]
    s = SPECS[name]
    B, H, L = s["B"], s["H"], s["L"]
    g = torch.Generator().manual_seed(4000 + ALL.index(name))
    q = (torch.randn(B, L, H * 64, generator=g) * 0.5).to(bf).to(DEV)
    k = (torch.randn(B, L, H * 64, generator=g) * 0.5).to(bf).to(DEV)
    v = (torch.randn(B, L, H * 64, generator=g) * 0.5).to(bf).to(DEV)
    bias_t = None
    if s["bias"]:
        bias_t = FO.bias_to_kernel(torch.randn(H, L, L, generator=g).to(DEV))   # from (H, q, key)
    valid = None if s["valid"] is None else torch.tensor(s["valid"], dtype=torch.int32, device=DEV)
    R, bound, lse64 = _oracle(q, k, H, valid, bias_t, s["scale"], s["causal"])
    _CASES[name] = dict(s=s, q=q, k=k, v=v, bias_t=bias_t, valid=valid, R=R, bound=bound,
                        lse64=lse64, lse32=lse64.float().contiguous())
    return _CASES[name]


def _received(c, lse, q=None, k=None):
    s = c["s"]
    _poison(((s["B"], s["H"], s["L"]), torch.float32))
    got = _ext().flash_attn_received(c["q"] if q is None else q, c["k"] if k is None else k, lse,
                                     s["H"], c["valid"], c["bias_t"], s["scale"], s["causal"])
    torch.cuda.synchronize()
    assert got.dtype == torch.float32 and tuple(got.shape) == (s["B"], s["H"], s["L"])
    assert got.is_contiguous()
    return got


def _check(tag, got, ref, bound):
    got = got.double()
    assert bool(torch.isfinite(got).all()), f"{tag}: non-finite R"
    err = (got - ref).abs()
    print(f"[bound] {tag}: max |err| / bound {float((err / bound).max()):.3f}")
    excess = err - bound
    worst = int(excess.argmax())
    assert float(excess.flatten()[worst]) <= 0.0, (
        f"{tag} element {worst}: got {float(got.flatten()[worst])!r} "
        f"ref {float(ref.flatten()[worst])!r} bound {float(bound.flatten()[worst])!r}")


def _check_zeros(got, valid, L):
    """Keys >= valid[b] are exactly 0 (so a valid = 0 batch row entirely, and
    under valid = 1 every key but 0)."""
    if valid is None:
        return
    for b, vl in enumerate(valid.tolist()):
        assert bool((got[b, :, vl:] == 0).all()), f"batch row {b}: keys >= {vl} not exactly 0"
        if vl > 0:
            assert bool((got[b, :, :vl] > 0).all())


# --------------------------------------------------------------------------
# A. the kernel alone
# --------------------------------------------------------------------------

@pytest.mark.parametrize("name", ALL)
def test_kernel_elementwise(name):
    c = _case(name)
    got = _received(c, c["lse32"])
    _check(name, got, c["R"], c["bound"])
    _check_zeros(got, c["valid"], c["s"]["L"])
    # the bound cannot hide a structural defect
    pos = c["R"] > 0
    ratio = float((c["bound"][pos] / c["R"][pos]).max())
    print(f"[bound] {name}: max bound / R {ratio:.3e}")
    assert ratio <= 2.0 ** -12
    assert bool((c["R"][~pos] == 0).all())


# --------------------------------------------------------------------------
# B. with the forward kernel's lse
# --------------------------------------------------------------------------

@pytest.mark.parametrize("name", FWD_LSE_CASES)
def test_with_forward_lse(name):
    c = _case(name)
    s = c["s"]
    B, H, L = s["B"], s["H"], s["L"]
    _poison(((B, L, H * 64), bf), ((B, H, L), torch.float32))
    _O, lse = _ext().flash_attn_fwd(c["q"], c["k"], c["v"], H, c["valid"], c["bias_t"], s["scale"],
                                    s["causal"], 0.0, 0)
    got = _received(c, lse)
    y = _lse_yardstick(c["q"], c["k"], H, c["valid"], c["bias_t"], s["scale"], s["causal"],
                       c["lse64"])
    assert y > 0.0
    bound = c["bound"] + SECOND * LSE_MARGIN * y * c["R"]
    _check(name + " fwd-lse", got, c["R"], bound)
    _check_zeros(got, c["valid"], L)


# --------------------------------------------------------------------------
# C. layout, D. determinism
# --------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["L192-valid-bias-scale", "L128-H12-valid-bias"])
def test_fused_buffer_slices_equal_contiguous(name):
    c = _case(name)
    D = c["s"]["H"] * 64
    qkv = torch.cat([c["q"], c["k"], c["v"]], dim=-1)
    qs, ks = qkv[..., :D], qkv[..., D:2 * D]
    assert not qs.is_contiguous() and qs.stride(1) == 3 * D
    sliced = _received(c, c["lse32"], qs, ks)
    plain = _received(c, c["lse32"])
    assert torch.equal(sliced, plain)


@pytest.mark.parametrize("name", ["L320-valid-bias-causal", "L192-none"])
def test_deterministic(name):
    c = _case(name)
    assert torch.equal(_received(c, c["lse32"]), _received(c, c["lse32"]))


# --------------------------------------------------------------------------
# E. wrappers
# --------------------------------------------------------------------------

def test_wrappers():
    from deepdfa_amd.ops import (attention_received, flash_attention_received,
                                 flash_attention_received_qkv)
    from deepdfa_amd.ops.transformer import flash_attention_qkv

    c = _case("L192-valid-bias-scale")
    s = c["s"]
    H = s["H"]
    qkv = torch.cat([c["q"], c["k"], c["v"]], dim=-1)
    kw = dict(valid=c["valid"], bias=c["bias_t"], scale=s["scale"], causal=s["causal"])
    with torch.no_grad():
        O, R = flash_attention_received_qkv(qkv, H, **kw)
        O_ref = flash_attention_qkv(qkv, H, dropout_p=0.0, **kw)
    assert torch.equal(O, O_ref)
    assert not O.requires_grad and not R.requires_grad
    _O, lse = _ext().flash_attn_fwd(c["q"], c["k"], c["v"], H, c["valid"], c["bias_t"], s["scale"],
                                    s["causal"], 0.0, 0)
    raw = _received(c, lse)
    assert torch.equal(R, raw)
    # the unfused form and the raw op are the same launches
    O2, R2 = flash_attention_received(c["q"], c["k"], c["v"], H, **kw)
    assert torch.equal(O2, O) and torch.equal(R2, R)
    assert torch.equal(attention_received(c["q"], c["k"], H, lse, **kw), R)

    leaf = qkv.clone().requires_grad_()
    with pytest.raises(ValueError):
        flash_attention_received_qkv(leaf, H, **kw)
    with pytest.raises(ValueError):
        flash_attention_received(c["q"].clone().requires_grad_(), c["k"], c["v"], H, **kw)
    with torch.no_grad():   # fine without grad mode
        O3, _ = flash_attention_received_qkv(leaf, H, **kw)
    assert torch.equal(O3, O)


def test_binding_rejects_bad_arguments():
    c = _case("L64-valid")
    ext, s = _ext(), c["s"]
    args = (s["H"], c["valid"], None, 1.0, False)
    with pytest.raises(RuntimeError):
        ext.flash_attn_received(c["q"].float(), c["k"].float(), c["lse32"], *args)
    with pytest.raises(RuntimeError):
        ext.flash_attn_received(c["q"], c["k"], c["lse32"][:, :, :32].contiguous(), *args)
    with pytest.raises(RuntimeError):
        ext.flash_attn_received(c["q"], c["k"], c["lse32"].double(), *args)
    with pytest.raises(RuntimeError):
        ext.flash_attn_received(c["q"][:, :32], c["k"][:, :32], c["lse32"], *args)
    with pytest.raises(RuntimeError):
        ext.flash_attn_received(c["q"], c["k"], c["lse32"], s["H"], c["valid"][:2].contiguous(),
                                None, 1.0, False)


# --------------------------------------------------------------------------
# F. model, G. driver
# --------------------------------------------------------------------------

_MODEL = {}


def _small_model():
    if _MODEL:
        return _MODEL["model"], _MODEL["ids"], _MODEL["valid"]
    from deepdfa_amd.models.linevul import Model
    from deepdfa_amd.models.roberta import RobertaConfig

    torch.manual_seed(0)
    L = 128
    cfg = RobertaConfig(vocab_size=1000, hidden_size=128, num_attention_heads=2,
                        num_hidden_layers=2, intermediate_size=256)
    model = Model(config=cfg).to(DEV).eval()
    g = torch.Generator().manual_seed(2)
    ids = torch.randint(3, cfg.vocab_size, (3, L), generator=g)
    ids[:, 0] = 0
    lens = (L, 70, 9)
    for b, n in enumerate(lens):
        ids[b, n:] = cfg.pad_token_id
    _MODEL.update(model=model, ids=ids.to(DEV),
                  valid=torch.tensor(lens, dtype=torch.int32, device=DEV))
    return _MODEL["model"], _MODEL["ids"], _MODEL["valid"]


def test_model_stays_on_the_fused_path(monkeypatch):
    import deepdfa_amd.models.roberta as roberta
    import deepdfa_amd.ops.transformer as T

    model, ids, valid = _small_model()
    H, L = 2, ids.shape[1]
    with torch.no_grad(), torch.autocast(device_type="cuda", dtype=bf):
        prob_ref = model(ids)

    def boom(*a, **k):
        raise AssertionError("materialised attention branch entered")

    recorded = []
    real_qkv = T.fused_qkv

    def recording_qkv(*a, **k):
        out = real_qkv(*a, **k)
        recorded.append(out)
        return out

    monkeypatch.setattr(roberta, "masked_softmax_dropout", boom)
    monkeypatch.setattr(T, "fused_qkv", recording_qkv)
    with torch.no_grad(), torch.autocast(device_type="cuda", dtype=bf):
        prob, received = model(ids, attention_received=True)
    assert torch.equal(prob, prob_ref)
    assert len(received) == 2 and len(recorded) == 2
    scale = 1.0 / math.sqrt(64)
    for layer, (R, qkv) in enumerate(zip(received, recorded)):
        assert qkv is not None and qkv.dtype == bf and tuple(qkv.shape) == (3, L, 3 * H * 64)
        assert R.dtype == torch.float32 and tuple(R.shape) == (3, H, L) and not R.requires_grad
        q, k = qkv[..., :H * 64].contiguous(), qkv[..., H * 64:2 * H * 64].contiguous()
        ref, bound, lse64 = _oracle(q, k, H, valid, None, scale, False)
        y = _lse_yardstick(q, k, H, valid, None, scale, False, lse64)
        _check(f"model layer {layer}", R, ref, bound + SECOND * LSE_MARGIN * y * ref)
        _check_zeros(R, valid, L)


def test_model_without_fused_qkv_stays_on_flash(monkeypatch):
    """B L = 64 rows is no multiple of the fused QKV GEMM's 128: the layer
    projects q, k, v one by one and still takes flash_attention_received."""
    import deepdfa_amd.models.roberta as roberta
    import deepdfa_amd.ops.transformer as T

    model, ids, _ = _small_model()
    ids1 = ids[1:2, :64].contiguous()           # one row, 64 tokens, none padded
    valid = torch.tensor([64], dtype=torch.int32, device=DEV)
    with torch.no_grad(), torch.autocast(device_type="cuda", dtype=bf):
        prob_ref = model(ids1)

    def boom(*a, **k):
        raise AssertionError("materialised attention branch entered")

    recorded = []
    real = T.flash_attention_received

    def recording(q, k, v, *a, **kw):
        recorded.append((q, k))
        return real(q, k, v, *a, **kw)

    monkeypatch.setattr(roberta, "masked_softmax_dropout", boom)
    monkeypatch.setattr(T, "flash_attention_received", recording)
    with torch.no_grad(), torch.autocast(device_type="cuda", dtype=bf):
        assert T.fused_qkv(torch.zeros(1, 64, 128, device=DEV, dtype=bf),
                           *(torch.zeros(128, 128, device=DEV),) * 3) is None
        prob, received = model(ids1, attention_received=True)
    assert torch.equal(prob, prob_ref)
    assert len(received) == 2 and len(recorded) == 2
    scale = 1.0 / math.sqrt(64)
    for layer, (R, (q, k)) in enumerate(zip(received, recorded)):
        assert q.dtype == bf and tuple(q.shape) == (1, 64, 128) and tuple(R.shape) == (1, 2, 64)
        ref, bound, lse64 = _oracle(q.contiguous(), k.contiguous(), 2, valid, None, scale, False)
        y = _lse_yardstick(q.contiguous(), k.contiguous(), 2, valid, None, scale, False, lse64)
        _check(f"unfused model layer {layer}", R, ref, bound + SECOND * LSE_MARGIN * y * ref)


def test_driver_batched_line_scores():
    from deepdfa_amd.train import unixcoder_main as uxc

    model, ids, valid = _small_model()
    B, L = ids.shape
    H = 2
    lines = torch.full((B, L), -1, dtype=torch.long)
    for b, n in enumerate(valid.tolist()):
        lines[b, 1:n - 1] = torch.arange(n - 2) // 8          # CLS, SEP and padding stay -1
    lines = lines.to(DEV)
    n_lines = int(lines.max()) + 1
    for layer in (-1, 0):
        got = uxc.attention_line_scores_batched(model, ids, lines, layer=layer)
        assert got.dtype == torch.float32 and tuple(got.shape) == (B, n_lines) and got.is_cuda
        with torch.no_grad(), torch.autocast(device_type="cuda", dtype=bf):
            _h, received = model.encoder(ids, attention_received=True)
        tok = received[layer].double().sum(1)                    # (B, L)
        ref = torch.zeros(B, n_lines + 1, dtype=torch.float64, device=DEV)
        for b in range(B):
            ref[b].index_add_(0, torch.where(lines[b] < 0, n_lines, lines[b]), tok[b])
        ref = ref[:, :n_lines]
        T = torch.zeros(B, n_lines + 1, dtype=torch.float64, device=DEV)
        for b in range(B):
            T[b].index_add_(0, torch.where(lines[b] < 0, n_lines, lines[b]),
                            torch.ones(L, dtype=torch.float64, device=DEV))
        tol = H * L * T[:, :n_lines] * 2.0 ** -23 * ref.abs()
        assert bool(((got.double() - ref).abs() <= tol).all())
        assert bool((got[T[:, :n_lines] == 0] == 0).all())
