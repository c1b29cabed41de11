"""generate(constraint=, constraint_draft_tokens=k) without a GPU: the argument checks, TokenConstraint.forced on hand-built states,
and the reference of tests/_constrain_draft_ref.py held against the one-token-at-a-time rule of tests/_constrain_ref.py (the draft
against TokenConstraint.walk, the concatenated rounds of accept against a walk that emits one token per step)."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "llava-mod_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _constrain_draft_ref as DR  # noqa: E402
import _constrain_ref as CR  # noqa: E402

T_MAX = 16


def _gen():
    from llavamod import generation
    return generation


def test_check_constraint_draft_args_raises_for_every_unsupported_combination():
    G = _gen()
    c = G.TokenConstraint.from_choices([[5, 6], [7]])
    chk = G.check_constraint_draft_args
    chk(None, None, T_MAX)                                       # the default: nothing to check
    chk(None, c, T_MAX, do_sample=True, repetition_penalty=1.3)  # ... whatever else is given
    chk(1, c, T_MAX)
    chk(T_MAX - 1, c, T_MAX, repetition_penalty=1.0)
    with pytest.raises(ValueError, match="needs a constraint"):
        chk(4, None, T_MAX)
    for k in (0, T_MAX, -1, 2.0, True, "4"):
        with pytest.raises(ValueError, match=r"constraint_draft_tokens must be an int in 1\.\.15"):
            chk(k, c, T_MAX)
    for kw, word in ((dict(do_sample=True), "greedy decoding only"), (dict(num_beams=2), "greedy decoding only"),
                     (dict(num_return_sequences=2), "one sequence per prompt"), (dict(assistant_model=object()), "assistant_model"),
                     (dict(speculative_sampling=True), "speculative_sampling"),
                     (dict(prompt_lookup_num_tokens=3), "prompt_lookup_num_tokens"),
                     (dict(repetition_penalty=1.3), "repetition_penalty"), (dict(stop_sequences=[[5, 6]]), "stop_sequences"),
                     (dict(stopping_criteria=[object()]), "stopping_criteria")):
        with pytest.raises(ValueError, match=word):
            chk(4, c, T_MAX, **kw)


def test_existing_constraint_refusals_keep_their_messages():
    G = _gen()
    c = G.TokenConstraint.from_choices([[5, 6], [7]])
    with pytest.raises(ValueError, match="constraint cannot be combined with prompt_lookup_num_tokens: that loop verifies or scores"):
        G.check_constraint_args(c, 512, prompt_lookup_num_tokens=3)
    with pytest.raises(ValueError, match="constraint cannot be combined with assistant_model"):
        G.check_constraint_args(c, 512, assistant_model=object())


# states of the hand-built automaton (V = 100, eos = 9 where one is given):
#   0 one edge                      1 one edge + accepting            2 one allowed edge + one banned edge (next -1)
#   3 one edge inside V + one >= V  4 open, one listed edge           5 terminal
#   6 accepting, its only edge >= V: nothing but eos is allowed       7 two allowed edges
#   8 one edge whose token is eos   9 only banned edges, accepting: terminal by the rule
HAND = (10, [(0, 11, 1), (1, 12, 2), (2, 13, 3), (2, 14, -1), (3, 15, 4), (3, 150, 4), (4, 16, 5), (6, 170, 0), (7, 17, 0), (7, 18, 5),
             (8, 9, 0), (9, 19, -1)], [1, 5, 6, 9], {4: 0})
EOS, V = 9, 100
FORCED = {  # state: (without eos, with eos)
    0: ((11, 1), (11, 1)), 1: ((12, 2), None), 2: ((13, 3), (13, 3)), 3: ((15, 4), (15, 4)), 4: (None, None), 5: (None, None),
    6: (None, None), 7: (None, None), 8: ((9, 0), None), 9: (None, None)}


def test_forced_on_hand_built_states():
    G = _gen()
    c, aut = G.TokenConstraint(*HAND), CR.automaton(*HAND)
    assert c.terminal[5] and c.terminal[9] and not c.terminal[6] and c.default_next[4] == 0
    for s, (plain, with_eos) in FORCED.items():
        assert c.forced(s, None, V) == plain == DR.forced(aut, s, None, V), s
        assert c.forced(s, EOS, V) == with_eos == DR.forced(aut, s, EOS, V), s
    # no vocabulary bound: the edge with token 150 counts, so state 3 has two allowed tokens and state 6 one
    assert c.forced(3) is None and DR.forced(aut, 3) is None
    assert c.forced(6) == (170, 0) == DR.forced(aut, 6) and c.forced(6, EOS) is None
    # an eos outside the vocabulary is no token: the accepting state 1 stays forced
    assert c.forced(1, 100, V) == (12, 2) == DR.forced(aut, 1, 100, V)
    assert c.forced(-1) is None and c.forced(10) is None and DR.forced(aut, -1) is None and DR.forced(aut, 10) is None
    # what forced() returns is what the mask leaves: exactly one allowed token, and it is that token
    for s in range(10):
        for eos in (None, EOS):
            f = c.forced(s, eos, V)
            ok = [t for t in range(V) if CR.allowed(aut, s, t, eos)]
            if f is not None:
                assert ok == [f[0]] and CR.step(aut, s, f[0]) == f[1], (s, eos)
            elif aut[s]["default"] < 0 and len(ok) == 1:
                assert ok == [eos], (s, eos)                     # a single allowed token that is not drafted: only ever eos


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_reference_draft_walks_what_the_constraint_walks(seed):
    """Random from_choices tries: from every state the drafted run is accepted by TokenConstraint.walk, ends where walk ends, stops
    exactly where the trie branches, may stop, or ends, and vstate names the states on the way."""
    G = _gen()
    rng = np.random.default_rng(seed)
    seqs = [[int(t) for t in rng.integers(0, 6, int(rng.integers(1, 10)))] for _ in range(12)]
    c = G.TokenConstraint.from_choices(seqs)
    aut = DR.automaton_of(c)
    n_forced = 0
    for k in (1, 4, 15):
        for s in range(c.n_states):
            for eos in (None, 7):
                dr, ch, vs, n = DR.draft_row(aut, 3, s, False, k, eos, 512)
                run = dr[:n]
                assert dr[n:] == [-1] * (k - n) and ch == [3] + run + [3] * (k - n)
                end, ok = c.walk(run, state=s)
                assert ok
                states = [c.walk(run[:j], state=s)[0] for j in range(n + 1)]
                assert all(c.forced(states[j], eos, 512) == (run[j], states[j + 1]) for j in range(n))
                assert n == k or c.forced(end, eos, 512) is None
                assert vs[:n] == states[:n] and vs[n] == (-1 if c.terminal[end] else end) and vs[n + 1:] == [-1] * (k - n)
                n_forced += n
    assert n_forced > 0
    assert DR.draft_row(aut, 3, 0, True, 4, None, 512) == ([-1] * 4, [3] * 5, [-1] * 5, 0)
    assert DR.draft_row(aut, 3, -1, False, 4, None, 512) == ([-1] * 4, [3] * 5, [-1] * 5, 0)
    assert DR.draft_row(aut, 3, c.n_states, False, 4, None, 512) == ([-1] * 4, [3] * 5, [-1] * 5, 0)


def _one_token_walk(aut, stream, s, eos, max_new):
    """Plain constrained greedy's bookkeeping, one token per step: the push (EOS finishes the row before the automaton sees the token),
    then tests/_constrain_ref.advance; stops at max_new tokens.  Returns (emitted, final state, why it stopped)."""
    out = []
    for tok in stream:
        out.append(tok)
        if eos is not None and tok == eos:
            return out, s, "eos"
        done, state = CR.advance(aut, [tok], [0], [s])
        if done[0] and int(state[0]) == s and CR.step(aut, s, tok) < 0:
            return out, s, "left"
        s = int(state[0])
        if done[0]:
            return out, s, "terminal"
        if len(out) >= max_new:
            return out, s, "budget"
    raise AssertionError("the stream ran out before the row ended")


def _rounds(aut, stream, s, k, eos, max_new, drafted):
    """The loop over accept_row with every draft accepted: drafts are the stream's own next tokens (`drafted` of them per round, then
    -1), the target is the stream.  Returns (emitted, final state, per-round (n_acc, n_emit), lens_target - L0)."""
    out, n_gen, done, lens, per_round = [stream[0]], 1, 0, 0, []
    first, s, why = _one_token_walk(aut, stream[:1], s, eos, 1)
    done = int(why != "budget" or max_new == 1)
    while not done:
        n = len(out)
        dr = stream[n:n + drafted] + [-1] * (k - drafted)
        tg = stream[n:n + k + 1]
        block, nxt, done, s, n_gen, lens = DR.accept_row(aut, dr, tg, False, s, n_gen, max_new, lens + k + 1, k, eos, 0)
        ne = block[k + 2]
        assert block[:ne] == stream[n:n + ne] and block[ne:k + 1] == [0] * (k + 1 - ne) and block[k + 4] == done
        assert block[k + 3] == nxt == (0 if done else block[ne - 1]) and 1 <= ne <= block[k + 1] + 1
        out += block[:ne]
        per_round.append((block[k + 1], ne))
        assert n_gen == len(out) and lens == len(out) - 1       # the cache holds every emitted token but the last
    return out, s, per_round, lens


# a chain 0 -5-> 1 -6-> 2 -7-> 3 -8-> 4 -9-> 5 -10-> 6 -11-> 7(terminal); state 3 also accepts; state 2 is open (default 2 -> stays)
CHAIN = (8, [(i, 5 + i, i + 1) for i in range(7)], [3, 7], {2: 2})
STREAM = [5, 6, 7, 8, 9, 10, 11, 5, 5, 5, 5, 5, 5, 5, 5, 5, 5, 5, 5, 5]


@pytest.mark.parametrize("k", [1, 3, 4, 15])
@pytest.mark.parametrize("case", ["terminal", "eos", "budget", "left"])
def test_concatenated_rounds_equal_the_one_token_walk(case, k):
    """Each of the four cuts in the middle of an accepted run (for k >= 3 the cutting token is an accepted DRAFT behind which more
    accepted drafts follow): the emitted tokens, the final state and the reason are the one-token walk's."""
    aut = CR.automaton(*CHAIN)
    stream, eos, max_new = list(STREAM), None, 50
    if case == "eos":
        eos = 8                                                 # state 3 accepts: emitted from it, the row ends in state 3
    elif case == "budget":
        max_new = 3
    elif case == "left":
        stream[3] = 99                                          # state 3 is closed and has no edge for 99
    want, want_state, why = _one_token_walk(aut, stream, 0, eos, max_new)
    assert why == case and want_state == {"terminal": 7, "eos": 3, "budget": 3, "left": 3}[case]
    for drafted in sorted({k, max(k - 1, 0), 0}):
        got, state, per_round, _ = _rounds(aut, stream, 0, k, eos, max_new, drafted)
        assert got == want and state == want_state, (drafted, got, want, state)
        if k >= 3 and drafted == k:
            n_acc, ne = per_round[0]
            # the cutting token is an accepted draft, not the target behind the run (the chain's terminal state lies 6 tokens in)
            assert n_acc == k and (ne <= n_acc or (case == "terminal" and k < 6)), per_round


def test_concatenated_rounds_on_random_automata():
    hits = set()
    for seed in range(4):
        rng = np.random.default_rng(seed)
        aut = CR.automaton(*CR.random_automaton(rng, 12, 10, max_edges=5))
        for trial in range(200):
            stream = [int(t) for t in rng.integers(0, 11, 40)]
            s0, k = int(rng.integers(0, 12)), int(rng.choice([1, 2, 4, 15]))
            eos = None if rng.random() < 0.5 else 10
            max_new = int(rng.integers(1, 12))
            want, want_state, why = _one_token_walk(aut, stream, s0, eos, max_new)
            got, state, _, _ = _rounds(aut, stream, s0, k, eos, max_new, int(rng.integers(0, k + 1)))
            assert got == want and state == want_state, (seed, trial, got, want, state, want_state, why)
            hits.add(why)
    assert hits == {"eos", "left", "terminal", "budget"}, hits


def test_simulate_counts_rounds_and_accepted_tokens():
    G = _gen()
    c = G.TokenConstraint.from_choices([[1, 2, 3, 4, 5, 6, 7, 8], [1, 9]])
    # after 1 the trie branches (2 or 9); after 2 everything is forced: 6 forced tokens behind [1, 2]
    rows = [[1, 2, 3, 4, 5, 6, 7, 8], [1, 9, 0, 0, 0, 0, 0, 0]]
    seqs, rounds, acc, states = DR.simulate(c, rows, 4)
    # row 0: first 1; round 1 no draft -> 2; round 2 drafts 3 4 5 6, all accepted, + 7; round 3 drafts 8 (terminal), accepted
    assert seqs == [[1, 2, 3, 4, 5, 6, 7, 8], [1, 9]] and rounds == 3 and acc == [5, 0]
    assert states == [c.walk(rows[0])[0], c.walk([1, 9])[0]] and all(c.terminal[s] for s in states)
    seqs, rounds, acc, states = DR.simulate(c, rows, 15)
    assert rounds == 2 and acc == [6, 0]
    seqs, rounds, acc, states = DR.simulate(c, [r[:5] for r in rows], 4, max_new=5)     # the budget cuts inside the forced run
    assert seqs == [[1, 2, 3, 4, 5], [1, 9]] and rounds == 2 and acc == [3, 0] and states[0] == c.walk([1, 2, 3, 4, 5])[0]
    seqs, rounds, acc, states = DR.simulate(c, [[1, 2, 3, 4, 5, 6, 7, 8]], 4, max_new=1)
    assert seqs == [[1]] and rounds == 0 and acc == [0] and states == [c.walk([1])[0]]


def test_assisted_output_keeps_its_positional_arguments():
    G = _gen()
    o = G.AssistedOutput("seq", 3, 4, "acc")
    assert (o.sequences, o.num_rounds, o.num_target_forwards, o.num_accepted, o.past_key_values, o.constraint_states) == \
        ("seq", 3, 4, "acc", None, None)
    o = G.AssistedOutput("seq", 3, 4, "acc", "cache", "states")
    assert o.past_key_values == "cache" and o.constraint_states == "states"
