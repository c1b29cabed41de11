"""Prompt-lookup decoding without a GPU: the drafting rule (tests/_lookup_ref.py) clause by clause and against HF's
PromptLookupCandidateGenerator, the replay of the loop's rounds, and the argument checks."""
import os
import random
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _lookup_ref as LR  # noqa: E402

V = 100
IMG = -200


def test_longest_ngram_wins_and_falls_back_to_shorter():
    # trailing (7, 8): its only earlier occurrence is at 3; the 1-gram (8) occurs earlier, at 0, but n = 2 is tried first
    h = [8, 1, 2, 7, 8, 4, 5, 6, 7, 8]
    assert LR.ngram_draft(h, 3, 2, V) == [4, 5, 6]
    assert LR.ngram_draft(h, 3, 1, V) == [1, 2, 7]
    # no 2-gram match: falls back to n = 1
    assert LR.ngram_draft([5, 9, 1, 2, 3, 9], 2, 2, V) == [1, 2]
    # max_ngram larger than the history: n starts at L - 1
    assert LR.ngram_draft([4, 4], 3, 8, V) == [4]


def test_earliest_match_wins():
    h = [1, 2, 30, 31, 1, 2, 40, 41, 1, 2]
    assert LR.ngram_draft(h, 2, 2, V) == [30, 31]


def test_continuation_is_never_empty_and_may_be_short():
    # the trailing n-gram itself (i + n == L) is not a match
    assert LR.ngram_draft([1, 2, 3], 4, 2, V) == []
    # a continuation shorter than k: the draft ends where the history ends
    assert LR.ngram_draft([1, 2, 9, 1, 2], 4, 2, V) == [9, 1, 2]
    # a a a a: the window overlaps the trailing n-gram
    assert LR.ngram_draft([6, 6, 6, 6], 4, 3, V) == [6]
    assert LR.ngram_draft([6, 6, 6, 6], 4, 2, V) == [6, 6]
    assert LR.ngram_draft([6, 6, 6, 6], 4, 1, V) == [6, 6, 6]


def test_ids_outside_the_vocabulary_match_but_are_never_drafted():
    # a placeholder inside the matched window is compared like any integer
    assert LR.ngram_draft([IMG, 3, 10, 11, IMG, 3], 2, 2, V) == [10, 11]
    # as a later continuation id: the draft is cut before it
    assert LR.ngram_draft([1, 2, 10, IMG, 11, 1, 2], 4, 2, V) == [10]
    # as the first continuation id: nothing is drafted and the search does NOT fall through to n = 1 (which would give [7])
    assert LR.ngram_draft([2, 7, 1, 2, IMG, 5, 1, 2], 4, 2, V) == []
    # an id >= V is cut the same way
    assert LR.ngram_draft([1, 2, 10, V, 11, 1, 2], 4, 2, V) == [10]
    assert LR.ngram_draft([1, 2, V + 5, 11, 1, 2], 4, 2, V) == []


def test_short_and_done_rows_draft_nothing():
    assert LR.ngram_draft([], 3, 2, V) == [] and LR.ngram_draft([5], 3, 2, V) == [] and LR.ngram_draft([5, 6], 3, 2, V) == []
    assert LR.ngram_draft([5, 5], 3, 2, V) == [5]
    assert LR.draft_arrays([5, 5], True, 3, 2, V) == ([-1, -1, -1], [5, 5, 5, 5], 0)
    assert LR.draft_arrays([5, 5], False, 3, 2, V) == ([5, -1, -1], [5, 5, 5, 5], 1)
    assert LR.draft_arrays([1, 2, 9, 8, 1, 2], False, 3, 2, V) == ([9, 8, 1], [2, 9, 8, 1], 3)
    assert LR.draft_arrays([7], False, 2, 2, V) == ([-1, -1], [7, 7, 7], 0)
    assert LR.draft_arrays([], False, 2, 2, V) == ([-1, -1], [0, 0, 0], 0)


def test_push_block():
    k = 2                                                 # block: tokens [k+1] | n_acc | n_emitted | next | done
    assert LR.push_block([4, 5, 0, 1, 2, 5, 0], k, [1, 2, 0, 0, 0], 2, 5) == ([1, 2, 4, 5, 0], 4)
    assert LR.push_block([0, 0, 0, 0, 0, 0, 1], k, [1, 2, 0, 0, 0], 2, 5) == ([1, 2, 0, 0, 0], 2)          # a done row
    assert LR.push_block([4, 5, 6, 2, 3, 6, 0], k, [1, 2, 3, 0, 0], 3, 5) == ([1, 2, 3, 0, 0], 3)          # would pass ld_hist


def test_reference_equals_hf_prompt_lookup():
    """Random histories over 4 symbols, V large enough that the cut never fires: the rule is HF's."""
    try:
        import torch
        from transformers.generation.candidate_generator import PromptLookupCandidateGenerator
    except Exception:                                     # transformers is optional on a test machine
        pytest.skip("transformers' PromptLookupCandidateGenerator is not importable here")
    rng = random.Random(0)
    for _ in range(300):
        L, k, n = rng.randint(1, 40), rng.randint(1, 6), rng.randint(1, 5)
        h = [rng.randint(0, 3) for _ in range(L)]
        gen = PromptLookupCandidateGenerator(eos_token_id=None, num_output_tokens=k, max_matching_ngram_size=n, max_length=10 ** 6)
        cand, _ = gen.get_candidates(torch.tensor([h]))
        assert cand[0, L:].tolist() == LR.ngram_draft(h, k, n, V), (h, k, n)


def test_simulate_hand_computed():
    """Greedy walks the cycle 1 -> 2 -> 3 -> 1.  Prompt [1, 2, 9, 1, 2, 3, 1, 2], N = 9 greedy tokens 3 1 2 3 1 2 3 1 2, k = 3, n <= 2.
    round 1: history ..1 2 | 3, trailing (2, 3) first at 4: draft 1 2 3, all accepted, emits 1 2 3 1 (4 tokens, 5 so far);
    round 2: trailing (3, 1) first at 5: draft 2 3 1, all accepted, emits 2 3 1 2 (9 so far): 2 rounds, 6 accepted.
    The second row's trailing 1-gram (2) is first seen at 1 with the wrong continuation 9: nothing accepted in round 1."""
    g = [3, 1, 2, 3, 1, 2, 3, 1, 2]
    seqs, rounds, acc = LR.simulate([[1, 2, 9, 1, 2, 3, 1, 2]], [g], 3, 2, V)
    assert (seqs, rounds, acc) == ([g], 2, [6])
    # k = 1 with n = 1: pending 3, first 3 at 5 -> draft [1] ok (2 emitted); pending 2: first 2 at 1 -> draft [9] rejected (1 emitted)
    seqs, rounds, acc = LR.simulate([[1, 2, 9, 1, 2, 3, 1, 2]], [g[:6]], 1, 1, V)
    #   n=1 |3 -> r1: d[1] acc, emit 1 2 (n=3) -> r2: pending 2, d[9] rej, emit 3 (n=4) -> r3: pending 3, d[1] acc, emit 1 2 (n=6)
    assert (seqs, rounds, acc) == ([g[:6]], 3, [2])
    # eos inside an accepted run cuts the emission and stops the row; the other row keeps the loop going
    seqs, rounds, acc = LR.simulate([[1, 2, 9, 1, 2, 3, 1, 2], [7, 8]], [g, [50, 51, 52, 53, 54, 55, 56, 57, 58]], 3, 2, V, eos=2)
    assert seqs[0] == [3, 1, 2] and acc == [2, 0] and rounds == 8 and seqs[1] == [50, 51, 52, 53, 54, 55, 56, 57, 58]
    # max_new_tokens cuts a round: N = 3 takes 2 of round 1's 4 tokens, both drafts
    seqs, rounds, acc = LR.simulate([[1, 2, 9, 1, 2, 3, 1, 2]], [g[:3]], 3, 2, V)
    assert (seqs, rounds, acc) == ([g[:3]], 1, [2])
    # a first token that is eos, or N = 1: no round at all
    assert LR.simulate([[1, 2]], [[3, 4]], 3, 2, V, eos=3) == ([[3]], 0, [0])
    assert LR.simulate([[1, 2]], [[3]], 3, 2, V) == ([[3]], 0, [0])


def test_simulate_agrees_with_the_bookkeeper():
    """The replay's counts are AssistedBookkeeper's when it is fed the blocks generation.spec_accept builds from the same drafts."""
    import torch
    from llavamod.generation import AssistedBookkeeper, spec_accept
    rng = random.Random(1)
    for trial in range(40):
        k, n_max, N, eos = rng.randint(1, 4), rng.randint(1, 3), rng.randint(1, 14), rng.choice([None, 2])
        period = rng.randint(2, 5)
        prompts = [[rng.randint(0, 5) for _ in range(rng.randint(1, 12))] for _ in range(2)]
        greedy = [[(p[-1] + 1 + i) % period for i in range(N)] for p in prompts]      # greedy walks 0 -> 1 -> .. -> period-1 -> 0
        seqs, rounds, acc = LR.simulate(prompts, greedy, k, n_max, V, eos)
        book = AssistedBookkeeper(2, k, N, eos, 99)
        done = book.first(torch.tensor([g[0] for g in greedy]))
        hist = [p + [g[0]] for p, g in zip(prompts, greedy)]
        while not book.finished:
            rows = [LR.draft_arrays(h, bool(d), k, n_max, V) for h, d in zip(hist, done)]
            draft = torch.tensor([r[0] for r in rows])
            # the target's argmax after [pending, draft...]: greedy's next token while the fed prefix is greedy's own
            target = torch.zeros((2, k + 1), dtype=torch.long)
            for b in range(2):
                n = int(book.n[b])
                g_at = lambda j, b=b: (prompts[b][-1] + 1 + j) % period              # greedy's j-th token, beyond N too
                for i in range(k + 1):
                    fed_ok = all(int(draft[b, j]) == g_at(n + j) for j in range(i))
                    target[b, i] = g_at(n + i) if fed_ok else 77                      # 77: never a draft
            block, _, _, _, _ = spec_accept(draft, target, done, eos, 99, torch.zeros(2), torch.zeros(2))
            for b in range(2):
                hist[b] = hist[b] + block[b, :int(block[b, k + 2])].tolist()
            book.update(block)
            done = book.stopped.clone()
        got = [book.seq[b, :int(book.n[b])].tolist() for b in range(2)]
        assert got == seqs and book.num_rounds == rounds and book.num_accepted.tolist() == acc, (trial, got, seqs)


def test_argument_errors():
    from llavamod.generation import check_batch_args, check_prompt_lookup_args
    T, NG = 16, 8
    check_prompt_lookup_args(1, 1, T, NG)
    check_prompt_lookup_args(T - 1, NG, T, NG)
    for k in (0, T, -1, 2.0, True, None):
        with pytest.raises(ValueError, match="prompt_lookup_num_tokens"):
            check_prompt_lookup_args(k, 2, T, NG)
    for n in (0, NG + 1, 1.5, True, None):
        with pytest.raises(ValueError, match="max_matching_ngram_size"):
            check_prompt_lookup_args(4, n, T, NG)
    with pytest.raises(ValueError, match="greedy"):
        check_prompt_lookup_args(4, 2, T, NG, do_sample=True)
    with pytest.raises(ValueError, match="greedy"):
        check_prompt_lookup_args(4, 2, T, NG, num_beams=2)
    with pytest.raises(ValueError, match="one sequence"):
        check_prompt_lookup_args(4, 2, T, NG, num_return_sequences=2)
    with pytest.raises(ValueError, match="assistant_model"):
        check_prompt_lookup_args(4, 2, T, NG, assistant_model=object())
    with pytest.raises(ValueError, match="speculative_sampling"):
        check_prompt_lookup_args(4, 2, T, NG, speculative_sampling=True)
    for name, value in (("repetition_penalty", 1.2), ("no_repeat_ngram_size", 2), ("bad_words_ids", [[1]]), ("suppress_tokens", [1]),
                        ("min_new_tokens", 1), ("stop_sequences", [[1, 2]]), ("stopping_criteria", [object()])):
        with pytest.raises(ValueError, match=name):
            check_prompt_lookup_args(4, 2, T, NG, **{name: value})
    check_prompt_lookup_args(4, 2, T, NG, repetition_penalty=1.0, no_repeat_ngram_size=0, bad_words_ids=None, suppress_tokens=None,
                             min_new_tokens=0, stop_sequences=None, stopping_criteria=None)
    import torch
    with pytest.raises(ValueError, match="prompt_lookup_num_tokens"):
        check_batch_args([dict(input_ids=torch.tensor([1, 2]))], prompt_lookup_num_tokens=4)
