"""Logits processors and stop sequences on the device: lmod_logits_process_bf16 and lmod_gen_push_stop against the plain-torch
statements of tests/_logits_ref.py (exact bf16 bit equality over the whole block, so an element no processor touches was not
written either), then generate() with every new argument against a step-by-step loop written here that drives
forward(use_cache=True) / past_key_values, applies _logits_ref.process_logits to the returned logits and selects with the same
selection kernel: both sides select from bit-identical bf16 rows, so the tokens are equal token for token."""
import functools
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "llava-mod_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _logits_ref as LR  # noqa: E402
from test_generate_gpu import _pair, _prompt  # noqa: E402

DEV = "cuda"
BF = torch.bfloat16
I32 = torch.int32
HL = 720                                          # history buffer width
LONG = list(range(20, 36))                        # the 16-token bad-word entry
EOS = 9


# ------------------------------------------------------------------------------------------------------------- kernel level
@functools.lru_cache(maxsize=None)
def _histories(V, n, which):
    """Rows of (hist [R, HL], n_hist [R]) on the host.  Set "a": empty, one token, 700 tokens with many duplicates, several -200
    entries and the first 15 tokens of LONG at the end (and once before).  Set "b": a history that ends exactly n-1 tokens after an
    earlier copy of itself, then the one-token one, then the long one.  The small shape has two rows: the first and the last of
    set "a", the first two of set "b".  The dead tail of every row holds ids that would change the result."""
    g = torch.Generator().manual_seed(V + 10 * n + (which == "b"))
    long_ = torch.randint(0, 50, (700,), generator=g)
    long_[torch.randint(0, 685, (9,), generator=g)] = -200
    long_[100:115] = torch.tensor(LONG[:15])                # an earlier copy of the ending, followed by 41: every n <= 16 bans 41
    long_[115] = 41
    long_[-15:] = torch.tensor(LONG[:15])
    rep = torch.randperm(V, generator=g)[:40]
    rep = torch.cat([rep, rep[10:10 + n - 1]])
    rows = {"a": [torch.zeros(0, dtype=torch.long), torch.tensor([7]), long_], "b": [rep, torch.tensor([7]), long_]}[which]
    rows = rows[:3] if V > 1000 else ([rows[0], rows[2]] if which == "a" else rows[:2])
    hist = torch.randint(0, V, (len(rows), HL), generator=g).to(I32)
    for r, h in enumerate(rows):
        hist[r, :h.numel()] = h.to(I32)
    return hist, torch.tensor([h.numel() for h in rows], dtype=I32)


@functools.lru_cache(maxsize=None)
def _logits(V, ld, R):
    g = torch.Generator().manual_seed(V + R)
    x = (torch.randn(R, ld, generator=g) * 4).to(BF)
    x[:, 3] = 0.0
    x[:, 21] = -0.0
    x[:, [5, 30, V - 1]] = float("-inf")
    x[0, 7] = -1.5
    x[-1, 7] = 2.25
    return x


def _bad_table(hist, n_hist):
    """A 1-token entry, a 2-token entry that row 0's history completes (when it has a last token) and the 16-token entry that the
    long history completes."""
    last = int(hist[0, int(n_hist[0]) - 1]) if int(n_hist[0]) > 0 else 13
    return [[4], [max(last, 0), 11], LONG]


CASES = {"penalty_1.3": dict(penalty=1.3), "penalty_0.8": dict(penalty=0.8), "ngram_1": dict(ngram=1), "ngram_2": dict(ngram=2),
         "ngram_3": dict(ngram=3), "bad_words": dict(bad=True), "min_new_eos_inside": dict(min_new=2, eos=EOS),
         "min_new_eos_absent": dict(min_new=2, eos=None), "all": dict(penalty=1.3, ngram=3, bad=True, min_new=2, eos=EOS)}


@pytest.mark.parametrize("case", sorted(CASES))
@pytest.mark.parametrize("which", ["a", "b"])
@pytest.mark.parametrize("V,ld,R", [(151936, 151936, 3), (1000, 1008, 2)])
def test_logits_process_kernel_equals_reference_bitwise(V, ld, R, which, case):
    from llavamod import kernels as K
    kw = dict(CASES[case])
    hist, n_hist = _histories(V, kw.get("ngram", 3), which)
    n_gen = torch.tensor([0, 2, 5][:R], dtype=I32)            # below, at and above min_new = 2
    assert hist.shape[0] == R
    table = _bad_table(hist, n_hist) if kw.pop("bad", False) else None
    x = _logits(V, ld, R)
    want = x.clone()
    want[:, :V] = LR.process_logits(x[:, :V], hist, n_hist, n_gen, bad=table, **kw)
    if case != "min_new_eos_absent":
        assert not torch.equal(want.view(torch.int16), x.view(torch.int16)), "the case changes nothing: it would test nothing"
    xd, hd = x.to(DEV), hist.to(DEV)
    got = K.logits_process_(xd[:, :V], hd, n_hist.to(DEV), n_gen.to(DEV), bad=K.seq_table(table, DEV), **kw)
    assert got.data_ptr() == xd.data_ptr()
    diff = (xd.cpu().view(torch.int16) != want.view(torch.int16)).nonzero()
    assert diff.numel() == 0, (diff[:8].tolist(), xd.cpu()[tuple(diff[0])], want[tuple(diff[0])])
    assert torch.equal(hd.cpu(), hist)


def test_logits_process_vocabulary_beyond_the_bitmap():
    """The first-occurrence bitmap of the penalty holds 524288 tokens (64 KB of LDS): beyond that a penalty raises ValueError and
    launches nothing; the other processors do not need the bitmap and run."""
    from llavamod import kernels as K
    V = 524288 + 32
    x = torch.zeros(1, V, dtype=BF, device=DEV)
    hist = torch.tensor([[V - 1, 3, V - 1]], dtype=I32, device=DEV)
    n_hist, n_gen = torch.tensor([3], dtype=I32, device=DEV), torch.zeros(1, dtype=I32, device=DEV)
    with pytest.raises(ValueError, match="524288"):
        K.logits_process_(x, hist, n_hist, n_gen, penalty=1.2)
    assert float(x.abs().sum()) == 0
    K.logits_process_(x, hist, n_hist, n_gen, ngram=1)
    assert torch.isinf(x[0, [3, V - 1]]).all() and int(torch.isinf(x).sum()) == 2


@pytest.mark.parametrize("eos", [EOS, None])
def test_gen_push_stop_kernel_equals_reference(eos):
    """R = 4: a row already done, a row hitting EOS, a row completing a 2-token stop sequence on this push, a row whose match would
    need a prompt token; plus a 1-token stop.  Outputs and every state array equal both host statements."""
    from llavamod import generation as G
    from llavamod import kernels as K
    stops = [[7, 8], [300]]
    hist = torch.full((4, 10), -5, dtype=I32)
    rows = [[1, 2, 3, 4], [1, 2, 3, 4], [1, 2, 3, 7], [1, 2, 7]]
    n_prompt = torch.tensor([3, 3, 3, 3], dtype=I32)
    for r, h in enumerate(rows):
        hist[r, :len(h)] = torch.tensor(h, dtype=I32)
    n_hist = torch.tensor([len(h) for h in rows], dtype=I32)
    n_gen = n_hist - n_prompt
    done = torch.tensor([1, 0, 0, 0], dtype=I32)
    tokens = torch.tensor([8, EOS, 8, 8], dtype=I32)
    want = LR.push_stop(tokens, done, hist, n_hist, n_prompt, n_gen, eos, 77, stops)
    host = G.gen_push_stop(tokens, done, hist, n_hist, n_prompt, n_gen, eos, 77, stops)
    assert want[1].tolist() == [1, int(eos is not None), 1, 0] and want[0].tolist() == [77, EOS, 8, 8]
    dev = [t.to(DEV) for t in (tokens, done, hist, n_hist, n_prompt, n_gen)]
    K.gen_push_stop_(*dev, eos, 77, K.seq_table(stops, DEV))
    got = [dev[i].cpu() for i in (0, 1, 2, 3, 5)]
    for name, g, w, h in zip(("tokens", "done", "hist", "n_hist", "n_gen"), got, want, host):
        assert torch.equal(g, w) and g.dtype == w.dtype, (name, g, w)
        assert torch.equal(h, w), (name, h, w)
    assert torch.equal(dev[4].cpu(), n_prompt)
    # a second push: the 1-token stop on row 3, everything else stays done and turns into pad
    tokens2 = torch.tensor([5, 5, 5, 300], dtype=I32)
    want2 = LR.push_stop(tokens2, *want[1:4], n_prompt, want[4], eos, 77, stops)
    t2 = tokens2.to(DEV)
    K.gen_push_stop_(t2, dev[1], dev[2], dev[3], dev[4], dev[5], eos, 77, K.seq_table(stops, DEV))
    for g, w in zip((t2, dev[1], dev[2], dev[3], dev[5]), want2):
        assert torch.equal(g.cpu(), w)
    assert want2[1].tolist()[2:] == [1, 1]


# ------------------------------------------------------------------------------------------------------------- end to end
N_NEW = 24
PAD = 3


@pytest.fixture(scope="module")
def teacher():
    _, t = _pair()
    t.eval()
    t.generation_budget = N_NEW        # the loop's use_cache prefill then sizes its cache exactly as generate(max_new_tokens=24) does
    return t


@pytest.fixture(scope="module")
def plain(teacher):
    """The unconstrained 24-token greedy output [2, 24] (computed once, never modified)."""
    return teacher.generate(**_prompt(), max_new_tokens=N_NEW).cpu()


def _history(p, n_new, n=1):
    ids = p["input_ids"].to(I32)
    am = p.get("attention_mask")
    n_prompt = am.to(I32).sum(1).to(I32) if am is not None else torch.full((ids.shape[0],), ids.shape[1], dtype=I32)
    hist = torch.zeros((ids.shape[0], ids.shape[1] + n_new), dtype=I32)
    hist[:, :ids.shape[1]] = ids
    return hist.repeat_interleave(n, 0), n_prompt.repeat_interleave(n)


def _loop(model, p, n_new, eos=None, pad=None, stops=(), sample=None, past=None, **proc):
    """generate() restated: HF-style cached forwards, the reference processors on the returned logits (host), the product's
    selection kernel, the reference stop rule.  Returns (tokens [B, <= n_new], token log-probabilities or None)."""
    from llavamod import kernels as K
    hist, n_prompt = _history(p, n_new)
    n_hist, n_gen = n_prompt.clone(), torch.zeros_like(n_prompt)
    done = torch.zeros_like(n_prompt)
    B = hist.shape[0]
    if past is None:
        o = model(input_ids=p["input_ids"], attention_mask=p["attention_mask"], images=p["images"], use_cache=True)
    else:
        # room for the turn and the new tokens, as generate() reserves it (the chunk attention splits its keys by the cache size)
        past.grow(int(past.lens.max()) + p["input_ids"].shape[1] + n_new)
        o = model(input_ids=p["input_ids"], attention_mask=p.get("attention_mask"), past_key_values=past)
    cache = o.past_key_values
    logits = o.logits[:, -1] if past is None else o.logits[torch.arange(B), (n_prompt - 1).long()]
    gen = torch.Generator(device=DEV).manual_seed(sample["seed"]) if sample else None
    out, lps = [], []
    for step in range(n_new):
        x = LR.process_logits(logits.to(BF).cpu(), hist, n_hist, n_gen, eos=eos, **proc).to(DEV)
        if sample:
            u = torch.rand(B, generator=gen, device=DEV)
            tok, st = K.sample(x, u, sample["temperature"], None, sample["top_p"], stats=True)
            xt = x.gather(1, tok.long()[:, None]).squeeze(1).double() / sample["temperature"]
            lp = (xt - st[:, 0].double() - torch.log(st[:, 1].double())).clamp(max=0.0).float()
            lps.append(torch.where(done.to(DEV) != 0, torch.zeros_like(lp), lp))
        else:
            tok = K.row_argmax(x)
        tok, done, hist, n_hist, n_gen = LR.push_stop(tok.cpu(), done, hist, n_hist, n_prompt, n_gen, eos, pad, stops)
        out.append(tok.long())
        if step + 1 == n_new or ((eos is not None or stops) and bool(done.all())):
            break
        logits = model(input_ids=tok.long()[:, None], past_key_values=cache).logits[:, 0]
    return torch.stack(out, 1), (torch.stack(lps, 1).cpu() if lps else None)


def _greedy_cases(plain):
    a, b = plain[0].tolist(), plain[1].tolist()
    eos = a[2]
    return {
        "repetition_penalty": dict(repetition_penalty=1.3),
        "repetition_penalty_below_1": dict(repetition_penalty=0.8),
        "no_repeat_ngram_size_2": dict(no_repeat_ngram_size=2),
        "no_repeat_ngram_size_3": dict(no_repeat_ngram_size=3),
        "bad_words_ids": dict(bad_words_ids=[[a[0]], [b[3], b[4]], [b[0], b[1], b[2]]]),
        "suppress_tokens": dict(suppress_tokens=[a[0], b[0], b[1]]),
        "min_new_tokens": dict(min_new_tokens=5, eos_token_id=eos, pad_token_id=PAD),
        "all": dict(repetition_penalty=1.2, no_repeat_ngram_size=2, bad_words_ids=[[b[3], b[4]]], suppress_tokens=[a[0]],
                    min_new_tokens=5, eos_token_id=eos, pad_token_id=PAD),
    }


@pytest.mark.parametrize("case", ["repetition_penalty", "repetition_penalty_below_1", "no_repeat_ngram_size_2",
                                  "no_repeat_ngram_size_3", "bad_words_ids", "suppress_tokens", "min_new_tokens", "all"])
def test_generate_greedy_with_processors_equals_the_loop(teacher, plain, case):
    from llavamod.generation import check_logits_args
    kw = _greedy_cases(plain)[case]
    p = _prompt()
    got = teacher.generate(**p, max_new_tokens=N_NEW, **kw).cpu()
    eos, pad = kw.get("eos_token_id"), kw.get("pad_token_id")
    plan = check_logits_args(**{k: v for k, v in kw.items() if k != "pad_token_id"}, vocab_size=512)
    want, _ = _loop(teacher, p, N_NEW, eos=eos, pad=pad, penalty=plan.penalty, ngram=plan.ngram, bad=plan.bad, min_new=plan.min_new)
    assert torch.equal(got, want), (got, want)
    print(case, "tokens that differ from the unconstrained output:", int((got != plain[:, :got.shape[1]]).sum()))
    if case != "repetition_penalty_below_1":                              # a penalty below 1 favours what greedy already repeats
        assert not torch.equal(got, plain[:, :got.shape[1]]), "the argument changed no token: the case tests nothing"
    if case == "min_new_tokens":
        assert got.shape[1] >= 5 and not bool((got[:, :5] == eos).any())
        short = teacher.generate(**p, max_new_tokens=N_NEW, eos_token_id=eos, pad_token_id=PAD).cpu()
        first = plain[0].tolist().index(eos)                              # <= 2: without the argument row 0 ends there
        assert int(short[0, first]) == eos and bool((short[0, first + 1:] == PAD).all())


def test_generate_sampling_with_processors_equals_the_loop(teacher):
    p = _prompt()
    out = teacher.generate(**p, max_new_tokens=N_NEW, do_sample=True, seed=7, temperature=0.7, top_p=0.9, repetition_penalty=1.2,
                           no_repeat_ngram_size=2, return_dict_in_generate=True)
    want, lps = _loop(teacher, p, N_NEW, sample=dict(seed=7, temperature=0.7, top_p=0.9), penalty=1.2, ngram=2)
    assert torch.equal(out.sequences.cpu(), want), (out.sequences, want)
    assert torch.equal(out.token_logprobs.cpu(), lps)
    assert out.past_key_values is not None


def test_no_repeat_ngram_size_1_never_repeats_a_token(teacher, plain):
    p = _prompt()
    live = [p["input_ids"][b, :int(p["attention_mask"][b].sum())].tolist() for b in range(2)]
    assert any(len(set(plain[b].tolist())) < N_NEW or set(plain[b].tolist()) & set(live[b]) for b in range(2)), \
        "precondition: the unconstrained greedy output repeats a token"
    got = teacher.generate(**p, max_new_tokens=N_NEW, no_repeat_ngram_size=1).cpu()
    assert got.shape == (2, N_NEW)
    for b in range(2):
        row = got[b].tolist()
        assert len(set(row)) == N_NEW and not set(row) & set(live[b]), (b, row, live[b])


class _Keywords:
    def __init__(self, seqs):
        self.keyword_ids = [torch.tensor(s) for s in seqs]


def _expect_stopped(plain, stops, pad):
    pos = [LR.first_stop(plain[b].tolist(), stops) for b in range(plain.shape[0])]
    assert all(q is not None for q in pos)
    want = torch.full((plain.shape[0], max(pos) + 1), pad, dtype=torch.int64)
    for b, q in enumerate(pos):
        want[b, :q + 1] = plain[b, :q + 1]
    return want, pos


def test_generate_stop_sequences(teacher, plain):
    p = _prompt()
    stops = [plain[0, 5:7].tolist(), [int(plain[1, 9])]]
    want, pos = _expect_stopped(plain, stops, PAD)
    assert max(pos) + 1 < N_NEW
    got = teacher.generate(**p, max_new_tokens=N_NEW, stop_sequences=stops, pad_token_id=PAD).cpu()
    assert torch.equal(got, want), (got, want, pos)
    via = teacher.generate(**p, max_new_tokens=N_NEW, stopping_criteria=[_Keywords(stops)], pad_token_id=PAD).cpu()
    assert torch.equal(via, want)
    with pytest.raises(TypeError, match="only token-level keyword criteria"):
        teacher.generate(**p, max_new_tokens=2, stopping_criteria=[object()])
    with pytest.raises(ValueError, match="num_beams"):
        teacher.generate(**p, max_new_tokens=2, stop_sequences=stops, num_beams=2)
    with pytest.raises(ValueError, match="at most 16"):
        teacher.generate(**p, max_new_tokens=2, stop_sequences=[[1]] * 17)


def test_generate_stop_sequences_in_a_continuation(teacher):
    """The new turn's tokens are this call's prompt: a stop sequence that they complete, or that straddles them and the generated
    tokens, does not fire; the result equals the unconstrained continuation cut at each row's first match."""
    p = _prompt()

    def first_turn():
        o = teacher.generate(**p, max_new_tokens=4, return_dict_in_generate=True)
        turn = torch.cat([o.sequences[:, -1:].cpu(), torch.tensor([[17, 40, 41, 5], [23, 40, 41, 0]])], 1)
        return o.past_key_values, dict(input_ids=turn, attention_mask=torch.tensor([[1, 1, 1, 1, 1], [1, 1, 1, 1, 0]]).bool())

    cache, turn = first_turn()
    free = teacher.generate(**turn, past_key_values=cache, max_new_tokens=N_NEW).cpu()
    # [40, 41] sits in both prompts; [41, first generated token of row 1] straddles prompt and output: neither may fire
    stops = [free[0, 5:7].tolist(), [int(free[1, 9])], [40, 41], [41, int(free[1, 0])]]
    want, pos = _expect_stopped(free, stops, PAD)
    cache, turn = first_turn()
    got = teacher.generate(**turn, past_key_values=cache, max_new_tokens=N_NEW, stop_sequences=stops, pad_token_id=PAD).cpu()
    assert torch.equal(got, want), (got, want, pos)
    cache, turn = first_turn()
    loop, _ = _loop(teacher, turn, N_NEW, pad=PAD, stops=stops, past=cache)
    assert torch.equal(loop, want)


def test_generate_stop_sequences_with_sampled_return_sequences(teacher):
    p = _prompt()
    kw = dict(max_new_tokens=N_NEW, do_sample=True, seed=7, temperature=0.7, top_p=0.9, num_return_sequences=2)
    free = teacher.generate(**p, **kw).cpu()
    assert free.shape == (4, N_NEW)
    pad = min(set(range(512)) - set(free.reshape(-1).tolist()))
    stops = [free[0, 5:7].tolist(), [int(free[2, 9])]]
    got = teacher.generate(**p, **kw, stop_sequences=stops, pad_token_id=pad).cpu()
    pos = [LR.first_stop(got[r].tolist(), stops) for r in range(4)]
    assert pos[0] is not None and pos[2] is not None
    for r, q in enumerate(pos):
        if q is not None:
            assert bool((got[r, q + 1:] == pad).all()) and torch.equal(got[r, :q + 1], free[r, :q + 1]), (r, q, got[r])
        else:
            assert got.shape[1] == N_NEW and torch.equal(got[r], free[r])
    assert got.shape[1] == (N_NEW if any(q is None for q in pos) else max(pos) + 1)
