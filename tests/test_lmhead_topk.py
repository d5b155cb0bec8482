"""generate(select="fused"), output_scores and the plain-torch forms of
lmhead_topk / beam_select (deepdfa_amd/ops/transformer.py), off the GPU.

The torch forms are the oracle the GPU kernels of csrc/lmhead_topk.hip are
compared with (tests/test_gpu_lmhead_topk.py), so here they are checked
against brute force written in plain Python:

A  lmhead_topk: values, columns and lse against a per-row Python sort by
   (value descending, column ascending), with duplicated weight rows; the
   k > 16 and k > V errors.
B  beam_select against a Python beam step that builds every candidate as a
   tuple and sorts by (total descending, parent ascending, rank ascending):
   random inputs, ties across parents and ranks, finished rows (none, some,
   all of a source), the step-0 scores [0, -1e9, ...], a candidate equal to
   eos, K = 1.
C  a float64 tiny T5 whose eos id never matches: no row finishes, and
   generate(select="fused") equals select="logits" token for token, greedy and
   beams, both kv_cache modes.
D  early finish: an untied head whose eos row is 1.25 x another row. Every
   step's whole beam set (captured from beam_select) equals a brute-force beam
   search over all K * V continuations written here, each prefix teacher-forced
   from scratch; a finished hypothesis holds exactly one slot.
E  output_scores equals the teacher-forced float64 log-probability of the
   returned sequence within 1e-12, both select modes, greedy and beams.
F  an unknown select raises; both drivers parse --decode_select and hand it to
   generate.
"""

import pytest
import torch

from deepdfa_amd.models.t5 import T5Config, T5ForConditionalGeneration, _DecodeState
from deepdfa_amd.ops import beam_select, lmhead_topk, lmhead_topk_usable
from deepdfa_amd.ops import transformer as T


# --------------------------------------------------------------------------
# A. lmhead_topk
# --------------------------------------------------------------------------

def _py_topk(row, k):
    order = sorted(range(len(row)), key=lambda j: (-row[j], j))[:k]
    return [row[j] for j in order], order


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_lmhead_topk_torch_against_python_sort(dtype):
    g = torch.Generator().manual_seed(3)
    M, Kd, V, k = 5, 8, 37, 6
    h = torch.randn(M, Kd, generator=g).to(dtype)
    w = torch.randn(V, Kd, generator=g).to(dtype)
    w[30], w[4], w[17] = w[9], w[9], w[2]       # bit-equal logits in every row
    assert not lmhead_topk_usable(h, w, k)
    val, idx, lse = lmhead_topk(h, w, k, scale=0.5)
    assert val.dtype == dtype and idx.dtype == torch.int32 and lse.dtype == dtype
    assert val.shape == (M, k) and idx.shape == (M, k) and lse.shape == (M,)
    logits = (h @ w.t()) * 0.5
    assert torch.equal(logits[:, 30], logits[:, 9]) and torch.equal(logits[:, 4], logits[:, 9])
    saw_tie = False
    for i in range(M):
        want_v, want_i = _py_topk(logits[i].tolist(), k)
        assert idx[i].tolist() == want_i and val[i].tolist() == want_v
        pos = {c: n for n, c in enumerate(want_i)}
        if 4 in pos and 9 in pos:
            saw_tie = True
            assert pos[4] + 1 == pos[9] and (30 not in pos or pos[9] + 1 == pos[30])
    assert saw_tie, "no duplicated column reached a top-k list"
    assert torch.allclose(lse, torch.logsumexp(logits, -1), rtol=0, atol=1e-5)


def test_lmhead_topk_rejects_bad_k_and_grad():
    h, w = torch.randn(2, 8), torch.randn(20, 8)
    for k in (0, 17, 21):
        with pytest.raises(ValueError):
            lmhead_topk(h, w, k)
    with pytest.raises(ValueError):
        lmhead_topk(h, torch.randn(5, 8), 6)            # k > V
    with pytest.raises(ValueError):
        lmhead_topk(h.clone().requires_grad_(), w, 2)
    with torch.no_grad():
        val, _, _ = lmhead_topk(h.clone().requires_grad_(), w, 2)
    assert not val.requires_grad


# --------------------------------------------------------------------------
# B. beam_select
# --------------------------------------------------------------------------

def _py_beam_step(val, idx, lse, scores, done, fill, eos):
    """Every candidate as (total, parent, rank, token), sorted; totals are the
    op's own arithmetic, evaluated one element at a time."""
    B, K = scores.shape
    out_s, out_p, out_t, out_d = [], [], [], []
    for b in range(B):
        cands = []
        for p in range(K):
            r = b * K + p
            if bool(done[r]):
                cands.append((float(scores[b, p]), p, 0, fill))
                continue
            for c in range(K):
                total = scores[b, p] + (val[r, c] - lse[r])
                cands.append((float(total), p, c, int(idx[r, c])))
        cands.sort(key=lambda t: (-t[0], t[1], t[2]))
        for total, p, c, tok in cands[:K]:
            out_s.append(total)
            out_p.append(b * K + p)
            out_t.append(tok)
            out_d.append(bool(done[b * K + p]) or tok == eos)
    return out_s, out_p, out_t, out_d


def _check_beam_step(val, idx, lse, scores, done, fill=0, eos=2):
    s, p, t, d = beam_select(val, idx, lse, scores, done, fill, eos)
    B, K = scores.shape
    assert s.shape == (B, K) and s.dtype == scores.dtype
    assert p.dtype == torch.long and t.dtype == torch.long and d.dtype == torch.bool
    ws, wp, wt, wd = _py_beam_step(val, idx, lse, scores, done, fill, eos)
    assert p.tolist() == wp and t.tolist() == wt and d.tolist() == wd
    assert s.flatten().tolist() == ws
    return s, p, t, d


def _beam_inputs(B, K, seed, dtype=torch.float32, V=50):
    g = torch.Generator().manual_seed(seed)
    val = torch.randn(B * K, K, generator=g).to(dtype).sort(dim=1, descending=True).values
    idx = torch.stack([torch.randperm(V, generator=g)[:K] for _ in range(B * K)]).to(torch.int32)
    lse = val[:, 0] + torch.rand(B * K, generator=g).to(dtype)
    scores = -torch.rand(B, K, generator=g).to(dtype).cumsum(1)
    return val, idx, lse, scores


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("B,K", [(1, 1), (3, 1), (1, 3), (3, 3), (3, 10), (2, 16)])
def test_beam_select_random_and_finished_rows(B, K, dtype):
    val, idx, lse, scores = _beam_inputs(B, K, 10 * B + K, dtype)
    none = torch.zeros(B * K, dtype=torch.bool)
    _check_beam_step(val, idx, lse, scores, none)
    some = none.clone()
    some[::2] = True
    _check_beam_step(val, idx, lse, scores, some)
    whole = none.clone()
    whole[:K] = True                                     # all beams of source 0
    s, p, t, d = _check_beam_step(val, idx, lse, scores, whole, fill=7)
    assert p[:K].tolist() == list(range(K)) and t[:K].tolist() == [7] * K
    assert torch.equal(s[0], scores[0]) and bool(d[:K].all())


def test_beam_select_step0_scores_take_all_winners_from_beam0():
    B, K = 3, 10
    val, idx, lse, _ = _beam_inputs(B, K, 5)
    scores = torch.full((B, K), -1e9)
    scores[:, 0] = 0.0
    s, p, t, d = _check_beam_step(val, idx, lse, scores, torch.zeros(B * K, dtype=torch.bool))
    assert p.view(B, K).tolist() == [[b * K] * K for b in range(B)]
    assert torch.equal(t.view(B, K), idx.view(B, K, K)[:, 0].long())


def test_beam_select_ties_and_eos():
    """Equal totals across parents and across ranks, built from values that add
    exactly: the smaller parent wins, then the smaller rank."""
    K = 3
    val = torch.tensor([[2.0, 1.0, 1.0], [2.0, 2.0, 0.0], [2.0, 1.0, 0.5]])
    idx = torch.tensor([[5, 6, 7], [8, 2, 9], [10, 11, 12]], dtype=torch.int32)
    lse = torch.full((3,), 4.0)
    scores = torch.zeros(1, K)
    # totals: p0 -2 -3 -3 | p1 -2 -2 -4 | p2 -2 -3 -3.5  ->  (p0,0) (p1,0) (p1,1)
    s, p, t, d = _check_beam_step(val, idx, lse, scores, torch.zeros(3, dtype=torch.bool))
    assert p.tolist() == [0, 1, 1] and t.tolist() == [5, 8, 2]
    assert d.tolist() == [False, False, True]            # token 2 is eos
    # a finished parent 0 at the same total still comes first, once
    done = torch.tensor([True, False, False])
    scores = torch.tensor([[-2.0, 0.0, 0.0]])
    s, p, t, d = _check_beam_step(val, idx, lse, scores, done, fill=0)
    assert p.tolist() == [0, 1, 1] and t.tolist() == [0, 8, 2] and d.tolist() == [True, False, True]


def test_beam_select_rejects_bad_shapes():
    val, idx, lse, scores = _beam_inputs(2, 3, 1)
    done = torch.zeros(6, dtype=torch.bool)
    with pytest.raises(ValueError):
        beam_select(val[:, :2], idx[:, :2], lse, scores, done, 0, 2)
    with pytest.raises(ValueError):
        beam_select(val, idx, lse[:5], scores, done, 0, 2)


# --------------------------------------------------------------------------
# C, D, E. generate
# --------------------------------------------------------------------------

def _tiny_t5(eos=2, tie=True, seed=0):
    torch.manual_seed(seed)
    cfg = T5Config(num_layers=1, num_decoder_layers=2, d_model=64, d_ff=128, num_heads=1,
                   vocab_size=60, eos_token_id=eos, tie_word_embeddings=tie)
    model = T5ForConditionalGeneration(cfg).double().eval()
    g = torch.Generator().manual_seed(seed + 1)
    ids = torch.randint(3, cfg.vocab_size, (3, 12), generator=g)
    ids[1, 8:] = cfg.pad_token_id
    return model, cfg, ids


def _tf_logp(model, ids, prefix):
    """(rows, V) float64 log-probabilities of the next token after `prefix`:
    the whole prefix teacher-forced through decoder.decode_step on a fresh
    concat state. (The full forward is no float64 teacher: its eager attention
    takes the scores through fp32, which moves a summed score by ~2e-7.)"""
    cfg = model.config
    scale = cfg.d_model ** -0.5 if cfg.tie_word_embeddings else 1.0
    with torch.no_grad():
        valid = ids.ne(cfg.pad_token_id).sum(1).to(torch.int32)
        enc = model.encoder(ids, valid)
        state = _DecodeState(len(model.decoder.block))
        for t in range(prefix.shape[1]):
            h = model.decoder.decode_step(prefix[:, t:t + 1], enc, valid, state)[:, -1]
        assert h.dtype == torch.float64
        return torch.log_softmax(model.lm_head(h * scale), -1)


def _tf_score(model, cfg, ids, seq):
    """Summed log-probability of each row of seq up to and including its first
    eos."""
    total = torch.zeros(seq.shape[0], dtype=torch.float64)
    alive = torch.ones(seq.shape[0], dtype=torch.bool)
    for t in range(1, seq.shape[1]):
        logp = _tf_logp(model, ids, seq[:, :t]).gather(1, seq[:, t:t + 1])[:, 0]
        total = total + torch.where(alive, logp, torch.zeros_like(logp))
        alive = alive & (seq[:, t] != cfg.eos_token_id)
    return total


@pytest.mark.parametrize("kv_cache", ["concat", "indirect"])
@pytest.mark.parametrize("beams", [1, 3, 10])
def test_fused_equals_logits_when_nothing_finishes(beams, kv_cache):
    model, cfg, ids = _tiny_t5(eos=-1, tie=False)
    a = model.generate(ids, max_length=9, num_beams=beams, kv_cache=kv_cache)
    b = model.generate(ids, max_length=9, num_beams=beams, kv_cache=kv_cache, select="fused")
    assert a.shape == (3, 9), "a row finished"
    assert not bool((a == cfg.eos_token_id).any())
    assert torch.equal(a, b)
    assert len({tuple(r) for r in a.tolist()}) > 1       # the sources matter: not degenerate


def _early_finish_model():
    """Untied head; the eos row is 1.25 x the row of the token greedy decoding
    emits at step 2 of source 0, so eos wins there in some beam."""
    model, cfg, ids = _tiny_t5(tie=False, seed=4)
    first = model.generate(ids, max_length=6)
    tok = int(first[0, 2])
    assert tok != cfg.eos_token_id
    with torch.no_grad():
        model.lm_head.weight[cfg.eos_token_id] = 1.25 * model.lm_head.weight[tok]
    return model, cfg, ids


def _brute_beam_search(model, cfg, ids, K, max_length):
    """Per source a list of K hypotheses (tokens, score, done), every step
    ranking ALL V continuations of every live hypothesis and the single pad
    continuation of a finished one. Yields the beam set after each step."""
    B = ids.shape[0]
    beams = [[([cfg.decoder_start_token_id], 0.0 if p == 0 else -1e9, False) for p in range(K)]
             for _ in range(B)]
    for _ in range(max_length - 1):
        prefix = torch.tensor([h[0] for hyps in beams for h in hyps])
        logp = _tf_logp(model, ids.repeat_interleave(K, 0), prefix)
        new = []
        for b in range(B):
            cands = []
            for p, (toks, score, done) in enumerate(beams[b]):
                if done:
                    cands.append((score, p, 0, cfg.pad_token_id, True))
                    continue
                row = logp[b * K + p]
                for tokn in range(row.shape[0]):
                    cands.append((score + float(row[tokn]), p, tokn, tokn,
                                  tokn == cfg.eos_token_id))
            cands.sort(key=lambda c: (-c[0], c[1]))
            new.append([(beams[b][p][0] + [tokn], s, d) for s, p, _, tokn, d in cands[:K]])
        beams = new
        yield beams
        if all(h[2] for hyps in beams for h in hyps):
            return


@pytest.mark.parametrize("kv_cache", ["concat", "indirect"])
def test_early_finish_matches_brute_force_beam_search(monkeypatch, kv_cache):
    model, cfg, ids = _early_finish_model()
    K, L = 3, 8
    # the in-place state keeps its relative-position bias table in fp32, also
    # in an fp64 model, which moves a score by ~1e-7; the concat path is fp64
    atol = 1e-12 if kv_cache == "concat" else 1e-6
    steps = []
    real = T.beam_select

    def spy(*a):
        out = real(*a)
        steps.append(out)
        return out

    monkeypatch.setattr(T, "beam_select", spy)
    seq, score = model.generate(ids, max_length=L, num_beams=K, kv_cache=kv_cache,
                                select="fused", output_scores=True)
    B = ids.shape[0]
    hyps = [[cfg.decoder_start_token_id] for _ in range(B * K)]
    finished_mid_run = False
    n = 0
    for n, want in enumerate(_brute_beam_search(model, cfg, ids, K, L), 1):
        s, parent, tok, done = steps[n - 1]
        hyps = [hyps[p] + [t] for p, t in zip(parent.tolist(), tok.tolist())]
        for b in range(B):
            got = [(hyps[b * K + j], bool(done[b * K + j])) for j in range(K)]
            assert got == [(h[0], h[2]) for h in want[b]], (n, b)
            assert torch.allclose(s[b], torch.tensor([h[1] for h in want[b]], dtype=s.dtype),
                                  rtol=0, atol=atol)
            fin = [tuple(h[0]) for h in want[b] if h[2]]
            assert len(fin) == len(set(fin)), "a finished hypothesis holds two slots"
            if fin and len(fin) < K and n < L - 1:
                finished_mid_run = True
    assert n == len(steps)
    assert finished_mid_run, "no hypothesis finished while others were live"
    assert seq.tolist() == [hyps[b * K] for b in range(B)]
    assert torch.allclose(score, _tf_score(model, cfg, ids, seq), rtol=0, atol=atol)


@pytest.mark.parametrize("select", ["logits", "fused"])
@pytest.mark.parametrize("beams", [1, 3])
def test_output_scores_are_teacher_forced_log_probabilities(select, beams):
    model, cfg, ids = _early_finish_model()
    seq, score = model.generate(ids, max_length=8, num_beams=beams, select=select,
                                kv_cache="concat", output_scores=True)
    assert score.shape == (3,) and score.dtype == torch.float64
    assert bool((seq == cfg.eos_token_id).any()), "no early finish in this case"
    assert torch.allclose(score, _tf_score(model, cfg, ids, seq), rtol=0, atol=1e-12)
    assert torch.equal(seq, model.generate(ids, max_length=8, num_beams=beams, select=select))
    fp32 = model.float().generate(ids, max_length=4, num_beams=beams, select=select,
                                  output_scores=True)[1]
    assert fp32.dtype == torch.float32


def test_greedy_fused_pads_after_eos():
    model, cfg, ids = _early_finish_model()
    out = model.generate(ids, max_length=8, select="fused")
    assert torch.equal(out, model.generate(ids, max_length=8))
    row = out[0].tolist()
    at = row.index(cfg.eos_token_id)
    assert at <= 2 and all(t == cfg.pad_token_id for t in row[at + 1:])


# --------------------------------------------------------------------------
# F. arguments and drivers
# --------------------------------------------------------------------------

def test_generate_rejects_unknown_select_and_wide_fused_beams():
    model, cfg, ids = _tiny_t5()
    with pytest.raises(ValueError):
        model.generate(ids, max_length=4, select="topk")
    with pytest.raises(ValueError):
        model.generate(ids, max_length=4, num_beams=17, select="fused")
    assert model.generate(ids, max_length=4, num_beams=17).shape[0] == 3    # "logits" serves it


def _spy_generate(monkeypatch):
    seen = []
    real = T5ForConditionalGeneration.generate

    def spy(self, *a, **kw):
        seen.append(kw.get("select"))
        return real(self, *a, **kw)

    monkeypatch.setattr(T5ForConditionalGeneration, "generate", spy)
    return seen


@pytest.mark.parametrize("flag,want", [([], "logits"), (["--decode_select", "fused"], "fused")])
def test_run_gen_passes_decode_select(monkeypatch, tmp_path, flag, want):
    from deepdfa_amd.train import run_gen

    seen = _spy_generate(monkeypatch)
    res = run_gen.main(["--do_test", "--n_synthetic", "8", "--num_layers", "1", "--d_model", "64",
                        "--max_source_length", "24", "--max_target_length", "6",
                        "--output_dir", str(tmp_path / "gen")] + flag)
    assert seen and set(seen) == {want} and 0.0 <= res["bleu4"] <= 1.0
    with pytest.raises(SystemExit):
        run_gen.main(["--decode_select", "topk"])


@pytest.mark.parametrize("flag,want", [([], "logits"), (["--decode_select", "fused"], "fused")])
def test_run_multi_gen_passes_decode_select(monkeypatch, tmp_path, flag, want):
    from deepdfa_amd.train import run_multi_gen

    seen = _spy_generate(monkeypatch)
    run_multi_gen.main(["--tasks", "summarize", "--max_steps", "1", "--eval_every", "1",
                        "--n_synthetic", "4", "--train_batch_size", "2", "--num_layers", "1",
                        "--d_model", "64", "--max_source_length", "32", "--max_target_length", "12",
                        "--output_dir", str(tmp_path / "mg")] + flag)
    assert seen and set(seen) == {want}
