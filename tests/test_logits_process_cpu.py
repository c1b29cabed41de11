"""Logits processors and stop sequences of generate(), host side (no GPU): the reference statement tests/_logits_ref.py pinned
against transformers' own processors, the stop rule against a plain loop, and the argument checks of generation.check_logits_args."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "llava-mod_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _logits_ref as LR  # noqa: E402
from llavamod import generation as G  # noqa: E402

V = 48
EOS = 5


def _case(n, length, seed):
    """R = 3 histories of `length` live tokens from a small alphabet (duplicates, repeated n-grams) inside a wider buffer whose dead
    tail holds other ids; the last n-1 tokens repeat an earlier stretch when the history is long enough."""
    g = torch.Generator().manual_seed(1000 * n + 10 * length + seed)
    R, L = 3, length + 7
    hist = torch.randint(0, 6, (R, L), generator=g)
    hist[:, length:] = torch.randint(6, V, (R, L - length), generator=g)          # dead tail: must never count
    if length >= 2 * n and n > 1:
        hist[:, length - (n - 1):length] = hist[:, 2:2 + n - 1]
    scores = torch.randn(R, V, generator=g) * 3
    scores[:, 7] = 0.0
    scores[0, 2] = float("-inf")
    return scores, hist, torch.full((R,), length)


def _lengths(n):
    return sorted({x for x in (0, 1, n - 2, n - 1, n, 50) if x >= 0})


@pytest.mark.parametrize("n", [1, 2, 3])
def test_reference_equals_transformers_processors(n):
    pytest.importorskip("transformers")
    from transformers.generation.logits_process import (MinNewTokensLengthLogitsProcessor, NoBadWordsLogitsProcessor,
                                                        NoRepeatNGramLogitsProcessor, RepetitionPenaltyLogitsProcessor)
    ran = 0
    for length in _lengths(n):
        for seed in range(3):
            scores, hist, n_hist = _case(n, length, seed)
            ids = hist[:, :length]
            tail = [int(t) for t in hist[0, max(length - 2, 0):length]]
            # a one-token entry, one that row 0's history completes (when it is long enough), one as long as the limit, [eos] (dropped)
            bad = [[9], tail + [11], list(range(20, 36)), [EOS]]
            n_prompt = max(length - 2, 0)
            n_gen = n_hist - n_prompt
            hf = {"pen": RepetitionPenaltyLogitsProcessor(1.3), "pen_lt1": RepetitionPenaltyLogitsProcessor(0.8),
                  "ngram": NoRepeatNGramLogitsProcessor(n), "bad": NoBadWordsLogitsProcessor(bad, eos_token_id=EOS),
                  "min": MinNewTokensLengthLogitsProcessor(n_prompt, 3, EOS, device="cpu")}
            ours = {"pen": dict(penalty=1.3), "pen_lt1": dict(penalty=0.8), "ngram": dict(ngram=n), "bad": dict(bad=bad[:3]),
                    "min": dict(min_new=3, eos=EOS)}
            for k in hf:
                want = hf[k](ids, scores.clone())
                got = LR.process_logits(scores, hist, n_hist, n_gen, round_bf16=False, **ours[k])
                assert torch.equal(got, want), (k, n, length, seed)
                ran += 1
            want = scores.clone()
            for k in ("pen", "ngram", "bad", "min"):                      # HF's order
                want = hf[k](ids, want)
            got = LR.process_logits(scores, hist, n_hist, n_gen, penalty=1.3, ngram=n, bad=bad[:3], min_new=3, eos=EOS, round_bf16=False)
            assert torch.equal(got, want), ("all", n, length, seed)
            if length >= n:
                assert torch.isinf(got).sum() > torch.isinf(scores).sum()    # something was banned: the comparison is not vacuous
    assert ran == len(_lengths(n)) * 3 * 5


def test_reference_skips_ids_outside_the_vocabulary_and_rounds_once():
    """The image placeholder (-200) is an ordinary integer for the n-gram comparison and is never penalised or banned."""
    hist = torch.tensor([[4, -200, 9, 4, -200, 0, 0]])
    n_hist, n_gen = torch.tensor([5]), torch.tensor([0])
    x = torch.randn(1, V, generator=torch.Generator().manual_seed(0)).to(torch.bfloat16)
    out = LR.process_logits(x, hist, n_hist, n_gen, penalty=1.3, ngram=3)
    assert out.dtype == torch.bfloat16
    want = x.float().clone()
    for t in (4, 9):
        want[0, t] = want[0, t] * torch.tensor(1.3) if want[0, t] < 0 else want[0, t] / torch.tensor(1.3)
    want[0, 9] = float("-inf")                                            # (4, -200) -> 9 already occurred
    assert torch.equal(out, want.to(torch.bfloat16))
    out2 = LR.process_logits(x, torch.tensor([[4, -200, 4, -200, 0]]), torch.tensor([3]), n_gen, ngram=2)
    assert torch.equal(out2, x)                                           # (4,) -> -200 is outside [0, V): nothing to ban


def _loop_push(tok, done, hist, nh, npr, ng, eos, pad, stops):
    """The stop rule as a plain loop over Python lists (modifies them)."""
    for r in range(len(tok)):
        if done[r]:
            tok[r] = pad
            continue
        hist[r][nh[r]] = tok[r]
        nh[r] += 1
        ng[r] += 1
        gen = hist[r][npr[r]:nh[r]]
        if (eos is not None and tok[r] == eos) or any(len(gen) >= len(s) and gen[-len(s):] == list(s) for s in stops):
            done[r] = 1


STOP_CASES = {
    # name: (prompt rows, generated so far, new tokens, stops)
    "match_only_in_prompt": ([[1, 7, 8, 2], [3, 3, 3, 3]], [[4], [4]], [6, 6], [[7, 8]]),
    "match_straddles_prompt_and_generated": ([[1, 2, 3, 7], [1, 2, 3, 4]], [[], [7]], [8, 8], [[7, 8]]),
    "shorter_is_suffix_of_longer": ([[1, 2], [1, 2]], [[9], [5]], [8, 8], [[7, 9, 8], [9, 8]]),
    "eos_pad_and_done_rows": ([[1, 2], [1, 2], [1, 2]], [[4], [4], [4]], [EOS, 6, 6], [[6]]),
}


@pytest.mark.parametrize("case", sorted(STOP_CASES))
@pytest.mark.parametrize("impl", ["reference", "product_host_statement"])
def test_stop_rule_against_a_plain_loop(case, impl):
    prompts, gens, new, stops = STOP_CASES[case]
    R, L = len(prompts), 12
    hist = torch.full((R, L), -1, dtype=torch.int32)
    for r in range(R):
        row = prompts[r] + gens[r]
        hist[r, :len(row)] = torch.tensor(row, dtype=torch.int32)
    npr = torch.tensor([len(p) for p in prompts], dtype=torch.int32)
    ng = torch.tensor([len(g) for g in gens], dtype=torch.int32)
    nh = npr + ng
    done = torch.zeros(R, dtype=torch.int32)
    if case == "eos_pad_and_done_rows":
        done[2] = 1
    tok = torch.tensor(new, dtype=torch.int32)
    f = LR.push_stop if impl == "reference" else G.gen_push_stop
    for eos in (None, EOS):
        state = [tok.tolist(), done.tolist(), hist.tolist(), nh.tolist(), npr.tolist(), ng.tolist()]
        ins = [t.clone() for t in (tok, done, hist, nh, npr, ng)]
        t2, d2, h2, nh2, ng2 = f(tok, done, hist, nh, npr, ng, eos, 99, stops)
        _loop_push(*state, eos, 99, stops)
        assert [t2.tolist(), d2.tolist(), h2.tolist(), nh2.tolist(), ng2.tolist()] == [state[0], state[1], state[2], state[3], state[5]]
        assert all(torch.equal(a, b) for a, b in zip(ins, (tok, done, hist, nh, npr, ng)))         # inputs untouched
        if case == "match_only_in_prompt" or case == "match_straddles_prompt_and_generated":
            assert d2.tolist() == [0, 0] if case == "match_only_in_prompt" else d2.tolist() == [0, 1]
        if case == "shorter_is_suffix_of_longer":
            assert d2.tolist() == [1, 0]
    assert LR.first_stop([3, 7, 8, 7, 8], [[7, 8]]) == 2 and LR.first_stop([3, 7], [[7, 8]]) is None
    assert LR.first_stop([3, EOS, 7, 8], [[7, 8]], eos=EOS) == 1


class _Keywords:
    """What the reference's KeywordsStoppingCriteria holds after __init__: keyword_ids, a list of 1-D tensors."""

    def __init__(self, seqs):
        self.keyword_ids = [torch.tensor(s) for s in seqs]


NEW_ARGS = [dict(repetition_penalty=1.2), dict(no_repeat_ngram_size=3), dict(bad_words_ids=[[4, 5]]), dict(suppress_tokens=[4]),
            dict(min_new_tokens=2), dict(stop_sequences=[[4, 5]]), dict(stopping_criteria=[_Keywords([[4, 5]])])]


def test_defaults_give_no_plan_and_values_are_converted():
    assert G.check_logits_args(vocab_size=V) is None and G.check_logits_args() is None
    plan = G.check_logits_args(repetition_penalty=1.1, no_repeat_ngram_size=3, bad_words_ids=[[4, 5], [EOS]], suppress_tokens=[7],
                               min_new_tokens=2, stop_sequences=[[1, 2]], stopping_criteria=[_Keywords([[3], [4, 5, 6]])],
                               eos_token_id=EOS, vocab_size=V)
    assert (plan.penalty, plan.ngram, plan.min_new, plan.process) == (1.1, 3, 2, True)
    assert plan.bad == [[4, 5], [7]]                                      # [eos] dropped, suppress_tokens appended as one-token entries
    assert plan.stops == [[1, 2], [3], [4, 5, 6]]
    only_stop = G.check_logits_args(stopping_criteria=[_Keywords([[3]])], vocab_size=V)
    assert only_stop.stops == [[3]] and not only_stop.process
    assert G.check_logits_args(min_new_tokens=2, vocab_size=V).min_new == 0            # no eos_token_id: ignored
    assert G.check_logits_args(bad_words_ids=[[EOS]], vocab_size=V).bad == [[EOS]]     # no eos_token_id: nothing to drop


def test_unsupported_stopping_criterion_raises_type_error():
    class MaxLength:
        max_length = 20

    with pytest.raises(TypeError, match="only token-level keyword criteria"):
        G.check_logits_args(stopping_criteria=[MaxLength()], vocab_size=V)
    with pytest.raises(TypeError, match="only token-level keyword criteria"):
        G.check_logits_args(stopping_criteria=[_Keywords([[3]]), lambda ids, scores: False], vocab_size=V)


def test_limits_and_ranges_raise_value_error():
    from llavamod import kernels as K
    assert K.LOGITS_MAX_SEQS == 16 and K.LOGITS_MAX_SEQ_LEN == 16
    ok = G.check_logits_args(bad_words_ids=[[i + 1] for i in range(16)], stop_sequences=[list(range(16))] * 16, vocab_size=V)
    assert len(ok.bad) == 16 and len(ok.stops) == 16
    bad_calls = [dict(bad_words_ids=[[i + 6] for i in range(17)]),
                 dict(bad_words_ids=[[i + 6] for i in range(16)], suppress_tokens=[1]),        # the COMBINED table
                 dict(stop_sequences=[[1]] * 17),
                 dict(stop_sequences=[[1]] * 16, stopping_criteria=[_Keywords([[2]])]),
                 dict(bad_words_ids=[list(range(17))]), dict(stop_sequences=[list(range(17))]),
                 dict(bad_words_ids=[[V]]), dict(suppress_tokens=[-1]), dict(stop_sequences=[[1, V]]), dict(bad_words_ids=[[]]),
                 dict(stopping_criteria=[_Keywords([[V + 3]])]),
                 dict(repetition_penalty=0.0), dict(repetition_penalty=-1.0), dict(no_repeat_ngram_size=-1), dict(min_new_tokens=-2),
                 dict(no_repeat_ngram_size=2.5)]
    for kw in bad_calls:
        with pytest.raises(ValueError):
            G.check_logits_args(vocab_size=V, eos_token_id=EOS, **kw)


@pytest.mark.parametrize("kw", NEW_ARGS, ids=[next(iter(k)) for k in NEW_ARGS])
def test_new_arguments_refuse_beams_and_assistant(kw):
    name = next(iter(kw))
    with pytest.raises(ValueError, match=f"{name}.*num_beams"):
        G.check_logits_args(vocab_size=V, num_beams=2, **kw)
    with pytest.raises(ValueError, match=f"{name}.*assistant_model"):
        G.check_logits_args(vocab_size=V, assistant_model=object(), **kw)
    assert G.check_logits_args(vocab_size=V, **kw) is not None
