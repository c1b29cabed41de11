"""generate_batch(prompt_lookup_num_tokens=k) without a GPU: the two bookkeeping kernels' rule (tests/_batch_lookup_ref.py) clause by
clause, the replay of a whole call against tests/_lookup_ref.simulate, the scheduler's variable advance and the argument checks."""
import os
import random
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _batch_lookup_ref as BR  # noqa: E402
import _lookup_ref as LR  # noqa: E402

V = 100


# ------------------------------------------------------------------------------------------------ lmod_batch_lookup_first
def test_first_fresh_running_and_done_slots():
    # fresh: the token becomes the pending token
    assert BR.first_row(7, 0, [1, 2], 2, 0, 5) == (7, 0, [1, 2, 7], 1)
    # running (n_gen > 0) and done slots: -1, nothing touched
    assert BR.first_row(7, 0, [1, 2, 8], 2, 1, 5) == (-1, 0, [1, 2, 8], 1)
    assert BR.first_row(7, 1, [1, 2], 2, 0, 5) == (-1, 1, [1, 2], 0)
    assert BR.first_row(7, 1, [1, 2, 8, 9], 2, 2, 5) == (-1, 1, [1, 2, 8, 9], 2)


def test_first_end_conditions():
    assert BR.first_row(7, 0, [1, 2], 2, 0, 1) == (7, 1, [1, 2, 7], 1)                        # budget 1
    assert BR.first_row(9, 0, [1, 2], 2, 0, 5, eos=9) == (9, 1, [1, 2, 9], 1)                 # eos first
    assert BR.first_row(7, 0, [1, 2], 2, 0, 5, eos=9, stops=[[7]]) == (7, 1, [1, 2, 7], 1)    # a one-token stop sequence
    # a two-token stop sequence whose first token is the prompt's last: the match would reach into the prompt
    assert BR.first_row(7, 0, [1, 6], 2, 0, 5, stops=[[6, 7]]) == (7, 0, [1, 6, 7], 1)
    # a full history row: left as it is, marked done
    assert BR.first_row(7, 0, [1, 2], 2, 0, 5, ld_hist=2) == (-1, 1, [1, 2], 0)


# ------------------------------------------------------------------------------------------------ lmod_batch_lookup_round
def test_round_rows_by_hand_k4():
    """The eight hand-built slots at k = 4, every number written out: block row, done, history, n_gen, cache length."""
    k = 4
    rows = BR.clause_rows(k)
    assert len(rows) == 8
    block, done, hist, n_gen, lens = BR.run_rows(rows, k)
    exp = [
        # emitted .. pad             n_acc n_emit next fin first | done  history                       n_gen lens
        ([0, 0, 0, 0, 0, 0, 0, 0, 1, 77], 1, [1, 2, 3, 77], 1, 20),
        ([43, 0, 0, 0, 0, 0, 1, 43, 0, -1], 0, [5, 41, 42, 43], 2, 3),
        ([10, 11, 12, 13, 60, 4, 5, 60, 0, -1], 0, [1, 2, 3, 4, 30, 10, 11, 12, 13, 60], 6, 9),
        ([10, 11, 61, 0, 0, 2, 3, 0, 1, -1], 1, [1, 2, 31, 32, 10, 11, 61], 5, 6),
        ([10, 9, 0, 0, 0, 4, 2, 0, 1, -1], 1, [1, 2, 3, 33, 10, 9], 3, 5),
        ([10, 11, 9, 0, 0, 2, 3, 0, 1, -1], 1, [1, 34, 10, 11, 9], 4, 4),
        ([10, 11, 0, 0, 0, 4, 2, 0, 1, -1], 1, [1, 2, 35, 36, 37, 10, 11], 5, 6),
        ([43, 0, 0, 0, 0, 4, 1, 0, 1, -1], 1, [1, 2, 38, 41, 42, 43], 4, 5),
    ]
    for s, e in enumerate(exp):
        assert (block[s], done[s], hist[s], n_gen[s], lens[s]) == e, (s, rows[s]["name"], block[s], done[s], hist[s], n_gen[s], lens[s])


@pytest.mark.parametrize("k", [1, 4, 15])
def test_round_rows_keep_their_kind_at_every_k(k):
    """The same eight slots at the k the GPU test uses: each row is still the kind its name says."""
    rows = BR.clause_rows(k)
    block, done, hist, n_gen, lens = BR.run_rows(rows, k)
    n_acc, n_emit, nxt, fin, first = ([b[k + 1 + j] for b in block] for j in range(5))
    assert all(len(b) == k + 6 for b in block)
    assert (n_emit[0], fin[0], first[0], lens[0]) == (0, 1, 77, 20) and hist[0] == rows[0]["hist"]          # done: lens stay at L0
    assert (n_acc[1], n_emit[1], fin[1], nxt[1]) == (0, 1, 0, 43)                                            # the prompt's 41 does not count
    assert (n_acc[2], n_emit[2], fin[2], nxt[2]) == (k, k + 1, 0, 60)
    assert n_acc[3] == min(2, k - 1) and n_emit[3] == n_acc[3] + 1 and fin[3] == 1 and n_gen[3] == rows[3]["budget"]
    assert n_acc[4] == k and block[4][n_emit[4] - 1] == BR.EOS and fin[4] == 1 and n_emit[4] <= k
    assert n_acc[5] == k // 2 and n_emit[5] == n_acc[5] + 1 and block[5][n_emit[5] - 1] == BR.EOS and fin[5] == 1
    assert n_acc[6] == k and n_emit[6] < k + 1 and fin[6] == 1 and n_gen[6] == rows[6]["budget"]
    assert (n_emit[7], fin[7]) == (1, 1) and hist[7][-3:] == [41, 42, 43]
    for s, r in enumerate(rows):
        assert lens[s] == r["cache_len"] - (k + 1) + n_emit[s]
        assert block[s][n_emit[s]:k + 1] == [BR.PAD] * (k + 1 - n_emit[s])
        assert (nxt[s] == BR.PAD) if fin[s] else (nxt[s] == block[s][n_emit[s] - 1])
        assert done[s] == fin[s]


def test_round_stop_looks_back_across_rounds_but_not_into_the_prompt():
    stops = [[41, 42, 43]]
    # generated 41 42, then 43 in this round: fires
    row, done, hist, n_gen, lens = BR.round_row([-1, -1], [43, 5, 5], -1, 2, 0, [1, 41, 42], 1, 2, 9, 5, stops=stops)
    assert (row, done, n_gen, lens) == ([43, 0, 0, 0, 1, 0, 1, -1], 1, 3, 3)
    # the 41 is the prompt's last token: does not fire, the row goes on
    row, done, hist, n_gen, lens = BR.round_row([-1, -1], [43, 5, 5], -1, 2, 0, [1, 41, 42], 2, 1, 9, 5, stops=stops)
    assert (row, done, n_gen, lens) == ([43, 0, 0, 0, 1, 43, 0, -1], 0, 2, 3)
    # a full history row ends the slot where it stands
    row, done, hist, n_gen, lens = BR.round_row([7, 8], [7, 8, 9], -1, 2, 0, [1, 2, 3], 1, 2, 9, 5, ld_hist=4)
    assert (row, done, hist, n_gen, lens) == ([7, 0, 0, 2, 1, 0, 1, -1], 1, [1, 2, 3, 7], 3, 3)


# ------------------------------------------------------------------------------------------------ the replay
def _cyclic_case(rng, R):
    """Prompts over a small alphabet whose greedy continuation follows a fixed successor map: drafts are partly right."""
    succ = {t: (t * 3 + 1) % 11 for t in range(11)}
    prompts, greedy = [], []
    for _ in range(R):
        p = [rng.randint(0, 10) for _ in range(rng.randint(2, 20))]
        g, t = [], p[-1]
        for _ in range(24):
            t = succ[t] if rng.random() < 0.85 else rng.randint(0, 10)
            g.append(t)
        prompts.append(p)
        greedy.append(g)
    return prompts, greedy


@pytest.mark.parametrize("k,n_max,eos", [(4, 2, None), (4, 2, 5), (1, 1, None), (15, 3, 7), (3, 8, None)])
def test_replay_equals_simulate_when_everything_is_admitted_at_once(k, n_max, eos):
    """max_batch_size >= len(requests), equal budgets: row by row the single-call loop's replay, which is pinned against
    transformers; the rounds are the slowest row's."""
    rng = random.Random(1000 * k + n_max)
    hits = 0
    for trial in range(20):
        R, N = rng.randint(1, 5), rng.choice([2, 7, 24])
        prompts, greedy = _cyclic_case(rng, R)
        g = [x[:N] for x in greedy]
        seqs, rounds, acc = LR.simulate(prompts, g, k, n_max, V, eos)
        toks, adm, r2, acc2, lens = BR.replay(prompts, g, k, n_max, V, [N] * R, R + rng.randint(0, 2), eos=eos)
        assert toks == seqs and acc2 == acc, (trial, toks, seqs, acc2, acc)
        assert adm == [(0, r, r) for r in range(R)]
        if rounds:                                                   # simulate counts no round for rows that end on their first token
            assert r2 == rounds, (trial, r2, rounds)
        else:
            assert r2 == 1
        for r in range(R):                                           # the cache holds the prompt and every token but the last
            assert lens[-1][r] == len(prompts[r]) + len(toks[r]) - 1
        hits += sum(acc)
    assert hits > 0


def test_replay_refills_slots_and_cuts_inside_a_run():
    """Two slots, five requests, per-request budgets: a cycle walked twice accepts everything, so its requests end early and their
    slots are refilled while the others run."""
    cyc = [3, 4, 5, 6, 7]
    prompts = [cyc * 2 + cyc[:2], [20, 21, 22], cyc * 2, [30, 31], cyc * 2 + cyc[:1]]
    nxt = {t: cyc[(cyc.index(t) + 1) % 5] for t in cyc}

    def cont(p, n):
        out, t = [], p[-1]
        for i in range(n):
            t = nxt[t] if t in nxt else 40 + i
            out.append(t)
        return out
    budgets = [11, 3, 24, 1, 7]
    greedy = [cont(p, b) for p, b in zip(prompts, budgets)]
    toks, adm, rounds, acc, lens = BR.replay(prompts, greedy, 4, 2, V, budgets, 2)
    assert toks == greedy
    # request 0: 1 + 5 + 5 tokens in rounds 0-1; request 1 (no match: 1 + 1, then 1) ends in round 1 too; 3 has budget 1 and ends in
    # the round it is admitted in
    assert adm == [(0, 0, 0), (0, 1, 1), (2, 2, 0), (2, 3, 1), (3, 4, 1)], adm
    assert acc[0] == 8 and acc[1] == 0 and acc[3] == 0 and acc[2] >= 16
    # request 2 (admitted in iteration 2) emits 1 + 5, 5, 5, 5, 3 tokens: five rounds; request 4 (iteration 3) 1 + 5, 1
    assert rounds == 7 and len(lens) == 7
    # slot 1 is idle from iteration 5 on: it stays where request 4 left it
    assert len({l[1] for l in lens[4:]}) == 1 and lens[4][1] == len(prompts[4]) + 7 - 1
    # a stop sequence inside an accepted run ends the request there (request 2: first token 3, then 4 5 | 6 7 3 of one run), and every
    # request is plain greedy cut behind the first place its generated tokens end with the sequence
    def cut(g, stop):
        for n in range(len(stop), len(g) + 1):
            if g[n - len(stop):n] == stop:
                return g[:n]
        return g
    toks2, *_ = BR.replay(prompts, greedy, 4, 2, V, budgets, 2, stops=[[4, 5]])
    assert toks2 == [cut(g, [4, 5]) for g in greedy] and toks2[2] == [3, 4, 5] and toks2[1] == greedy[1]
    toks3, *_ = BR.replay(prompts, greedy, 4, 2, V, budgets, 2, eos=40)
    assert toks3[1] == [40] and toks3[3] == [40] and toks3[0] == greedy[0]


# ------------------------------------------------------------------------------------------------ the scheduler
def test_scheduler_variable_advance_freeing_refill_and_counters():
    from llavamod.generation import LookupSlotScheduler, SlotScheduler
    s = LookupSlotScheduler([11, 3, 24, 1, 7], 2)
    assert isinstance(s, SlotScheduler)
    assert s.admit() == [(0, 0), (1, 1)]
    assert s.advance({0: 6, 1: 2}) == [] and s.n_gen == [6, 2]
    assert s.admit() == []
    assert s.advance({0: 5, 1: 1}, ended=[0]) == [(0, 0), (1, 1)]          # 0 reported by the device, 1 at its budget
    assert s.admit() == [(2, 0), (3, 1)]
    assert s.advance({0: 6, 1: 1}, ended=[1]) == [(3, 1)]
    assert s.admit() == [(4, 1)]
    assert s.advance({0: 5, 1: 4}, ended=[1]) == [(4, 1)]                   # an EOS before the budget
    assert s.admit() == [] and not s.finished and s.live == {0: 2}
    assert s.advance({0: 13}, ended=[0]) == [(2, 0)] and s.finished
    assert (s.num_rounds, s.num_target_forwards, s.num_admissions, s.num_prefills) == (5, 5, 5, 3)
    assert (s.live_row_steps, s.total_row_steps, s.tokens_emitted) == (9, 10, 43) and s.live_fraction == 0.9
    assert s.num_decode_steps == 0 and s.num_decode_forwards == 0


def test_scheduler_advance_rejects_what_cannot_happen():
    from llavamod.generation import LookupSlotScheduler
    s = LookupSlotScheduler([4, 4], 2)
    with pytest.raises(RuntimeError):
        s.advance({})
    s.admit()
    for emitted, ended in (({0: 1}, ()), ({0: 1, 1: 0}, ()), ({0: 5, 1: 1}, ()), ({0: 1, 1: 1, 2: 1}, ())):
        with pytest.raises(ValueError):
            s.advance(emitted, ended)
    s.advance({0: 4, 1: 1})
    with pytest.raises(ValueError):
        s.advance({1: 1}, ended=[0])                                        # slot 0 holds no request any more
    assert s.num_rounds == 1


def test_scheduler_step_is_unchanged():
    """step() on the sibling class is SlotScheduler's: the same returns and counters for the same calls."""
    from llavamod.generation import LookupSlotScheduler, SlotScheduler
    a, b = SlotScheduler([3, 1, 3], 2), LookupSlotScheduler([3, 1, 3], 2)
    for sch in (a, b):
        sch.trace = [sch.admit(), sch.step(), sch.admit(), sch.step([1]), sch.admit(), sch.step()]
    assert a.trace == b.trace
    for c in ("num_decode_steps", "num_decode_forwards", "num_admissions", "num_prefills", "live_row_steps", "total_row_steps"):
        assert getattr(a, c) == getattr(b, c), c
    assert b.num_rounds == 0


def test_batch_output_carries_the_round_counters():
    from llavamod.generation import BatchOutput, LookupSlotScheduler, SlotScheduler
    s = LookupSlotScheduler([2], 1)
    s.admit()
    s.advance({0: 2})
    o = BatchOutput(["x"], None, s, [1])
    assert (o.num_rounds, o.num_target_forwards, o.num_accepted, o.token_logprobs) == (1, 1, [1], None)
    assert (o.num_admissions, o.num_prefills, o.num_decode_steps) == (1, 1, 0)
    assert not hasattr(BatchOutput([], None, SlotScheduler([1], 1)), "num_rounds")


# ------------------------------------------------------------------------------------------------ argument checks
BAD = [(dict(do_sample=True), "do_sample"), (dict(repetition_penalty=1.3), "repetition_penalty"),
       (dict(no_repeat_ngram_size=2), "no_repeat_ngram_size"), (dict(bad_words_ids=[[5]]), "bad_words_ids"),
       (dict(suppress_tokens=[5]), "suppress_tokens"), (dict(min_new_tokens=2), "min_new_tokens")]


def test_check_batch_lookup_args():
    import torch
    from llavamod import kernels as K
    from llavamod.generation import RequestParams, check_batch_args, check_batch_lookup_args
    T, NG = K.APPEND_T_MAX, K.NGRAM_MAX
    assert (T, NG) == (16, 8)
    rq = [dict(input_ids=torch.tensor([1, 2, 3]), max_new_tokens=3), dict(input_ids=torch.tensor([4]))]
    check_batch_lookup_args(rq, 1, 1, T, NG)
    check_batch_lookup_args(rq, T - 1, NG, T, NG, do_sample=False, repetition_penalty=1.0, no_repeat_ngram_size=0, bad_words_ids=None,
                            suppress_tokens=None, min_new_tokens=0)
    for kw, pat in BAD:
        with pytest.raises(ValueError, match=pat):
            check_batch_lookup_args(rq, 4, 2, T, NG, **kw)
    with pytest.raises(ValueError, match="params"):
        check_batch_lookup_args(rq + [dict(input_ids=torch.tensor([1]), params=RequestParams(temperature=0.5))], 4, 2, T, NG)
    for k in (0, 16, -1, True, 2.0):
        with pytest.raises(ValueError, match="prompt_lookup_num_tokens"):
            check_batch_lookup_args(rq, k, 2, T, NG)
    for n in (0, 9, True, None):
        with pytest.raises(ValueError, match="max_matching_ngram_size"):
            check_batch_lookup_args(rq, 4, n, T, NG)
    with pytest.raises(ValueError, match="prompt_lookup_num_tokens"):       # the argument alone: the refusal it always got
        check_batch_lookup_args(rq, 4, None, T, NG)
    # check_batch_args itself keeps refusing the argument: generate_batch calls it without
    with pytest.raises(ValueError, match="prompt_lookup_num_tokens"):
        check_batch_args(rq, prompt_lookup_num_tokens=4)
    assert check_batch_args(rq, 2, 16) == [3, 16]


def test_generate_batch_refuses_before_any_device_work():
    """No model state is needed to get to the ValueError: `self` is None."""
    import torch
    from llavamod.generation import RequestParams
    from llavamod.model.language_model.llava_qwen2 import LlavaQwen2ForCausalLM
    rq = [dict(input_ids=torch.tensor([1, 2, 3]))]
    for kw, pat in BAD:
        with pytest.raises(ValueError, match=pat):
            LlavaQwen2ForCausalLM.generate_batch(None, rq, prompt_lookup_num_tokens=4, max_matching_ngram_size=2, **kw)
    with pytest.raises(ValueError, match="params"):
        LlavaQwen2ForCausalLM.generate_batch(None, [dict(input_ids=torch.tensor([1]), params=RequestParams(top_k=3))],
                                             prompt_lookup_num_tokens=4, max_matching_ngram_size=2)
    for k in (0, 16):
        with pytest.raises(ValueError, match="prompt_lookup_num_tokens"):
            LlavaQwen2ForCausalLM.generate_batch(None, rq, prompt_lookup_num_tokens=k, max_matching_ngram_size=2)
    with pytest.raises(ValueError, match="prompt_lookup_num_tokens"):       # without the n-gram size: refused, as before this mode
        LlavaQwen2ForCausalLM.generate_batch(None, rq, prompt_lookup_num_tokens=4)
    for n in (0, 9):
        with pytest.raises(ValueError, match="max_matching_ngram_size"):
            LlavaQwen2ForCausalLM.generate_batch(None, rq, prompt_lookup_num_tokens=4, max_matching_ngram_size=n)
    # the modes generate_batch refuses anyway
    for kw, pat in ((dict(num_beams=2), "num_beams"), (dict(assistant_model=object()), "assistant_model"),
                    (dict(num_return_sequences=2), "num_return_sequences"), (dict(past_key_values=object()), "past_key_values"),
                    (dict(max_batch_size=0), "max_batch_size")):
        with pytest.raises(ValueError, match=pat):
            LlavaQwen2ForCausalLM.generate_batch(None, rq, prompt_lookup_num_tokens=4, max_matching_ngram_size=2, **kw)
