"""generation.TokenConstraint on the host: the three constructors' CSR packing on hand-built cases, merge, walk against the
dict-of-dicts reference of tests/_constrain_ref.py on random automata, and every ValueError of the constraint arguments of generate()
and generate_batch().  No GPU, no HIP library."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "llava-mod_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _constrain_ref as CR  # noqa: E402
from llavamod import generation as G  # noqa: E402

TC = G.TokenConstraint
V = 512
IDS = torch.tensor([5, 6, 7])


def _rq(params=None, **kw):
    d = dict(input_ids=IDS, **kw)
    if params is not None:
        d["params"] = params
    return d


# ---------------------------------------------------------------------------------------------- constructors
def test_general_constructor_packs_csr_with_ascending_tokens_and_flags():
    # state 0 closed, 1 open (default 2, token 9 banned, token 4 redirected to 0), 2 closed + accepting with an edge, 3 terminal
    c = TC(4, [(0, 30, 1), (0, 7, 2), (0, 11, -1), (1, 9, -1), (1, 4, 0), (2, 5, 3)], accepting=[2, 3], default={1: 2})
    assert c.n_states == 4 and c.start == 0
    assert c.edge_off == [0, 3, 5, 6, 6]
    assert c.edge_tok == [7, 11, 30, 4, 9, 5]                       # ascending inside every state, whatever order they came in
    assert c.edge_next == [2, -1, 1, 0, -1, 3]
    assert c.default_next == [-1, 2, -1, -1]
    assert c.accept == [False, False, True, True] and c.terminal == [False, False, False, True]
    assert c.flags == [0, 0, 1, 3]
    assert c.has_closed and c.has_terminal
    assert c.edges() == [(0, 7, 2), (0, 11, -1), (0, 30, 1), (1, 4, 0), (1, 9, -1), (2, 5, 3)]
    for s in range(4):
        toks = c.edge_tok[c.edge_off[s]:c.edge_off[s + 1]]
        assert toks == sorted(set(toks))
    # the other forms of `default`, and another start
    assert TC(2, [], [0, 1], default=1, start=1).default_next == [1, 1]
    assert TC(2, [(0, 1, 1)], [1], default=[-1, 0]).default_next == [-1, 0]
    one = TC(1, [], [], default=0)                                  # one open state that bans nothing
    assert one.flags == [0] and not one.has_closed and not one.has_terminal and one.edge_off == [0, 0]


def test_from_choices_builds_a_trie_and_a_prefix_choice_is_accepting_but_not_terminal():
    c = TC.from_choices([[5, 6], [5], [7, 8, 9], [5, 6], torch.tensor([7, 8, 2])])       # a duplicate, a proper prefix, a tensor
    # nodes in order of creation: 0 root, 1 = [5], 2 = [5, 6], 3 = [7], 4 = [7, 8], 5 = [7, 8, 9], 6 = [7, 8, 2]
    assert c.n_states == 7 and c.start == 0
    assert c.edge_off == [0, 2, 3, 3, 4, 6, 6, 6]
    assert c.edge_tok == [5, 7, 6, 8, 2, 9] and c.edge_next == [1, 3, 2, 4, 6, 5]
    assert c.default_next == [-1] * 7
    assert c.accept == [False, True, True, False, False, True, True]
    assert c.terminal == [False, False, True, False, False, True, True]     # [5] may stop or go on to [5, 6]
    assert c.flags == [0, 1, 3, 0, 0, 3, 3]
    assert c.walk([5]) == (1, True) and c.walk([5, 6]) == (2, True) and c.walk([7, 8, 2]) == (6, True)
    assert c.walk([5, 7]) == (1, False) and c.walk([6]) == (0, False) and c.walk([5, 6, 5]) == (2, False)
    assert TC.from_choices([[3], [3]]).n_states == 2                # duplicates are dropped


def test_from_allowed_tokens_is_one_closed_accepting_self_loop():
    c = TC.from_allowed_tokens([40, 3, 17, 3])
    assert c.n_states == 1 and c.edge_off == [0, 3] and c.edge_tok == [3, 17, 40] and c.edge_next == [0, 0, 0]
    assert c.default_next == [-1] and c.flags == [1] and not c.has_terminal and c.has_closed
    assert c.walk([3, 40, 40, 17]) == (0, True) and c.walk([3, 4]) == (0, False)
    assert TC.from_allowed_tokens(torch.tensor([2, 1])).edge_tok == [1, 2]


def test_merge_offsets_states_and_reports_starts():
    a = TC.from_choices([[5, 6], [7]])                              # 4 states
    b = TC.from_allowed_tokens([1, 2])                              # 1 state
    c = TC(3, [(2, 9, 0), (0, 4, -1)], [1], default=[1, -1, -1], start=2)
    m, starts = TC.merge([a, None, b, c, None])
    assert starts == [0, -1, 4, 7, -1] and m.n_states == 8
    assert m.edge_off == [0, 2, 3, 3, 3] + [5] + [6, 6, 7]
    assert m.edge_tok == a.edge_tok + b.edge_tok + c.edge_tok
    assert m.edge_next == a.edge_next + [4, 4] + [-1, 5]
    assert m.default_next == [-1] * 5 + [6, -1, -1]
    assert m.flags == a.flags + b.flags + c.flags
    for part, s0 in ((a, 0), (b, 4), (c, 5)):                       # every part walks as it did alone, shifted
        for toks in ([5, 6], [7], [1, 2, 1], [9, 4], [9, 3, 3]):
            s, ok = part.walk(toks)
            assert m.walk(toks, state=part.start + s0) == (s + s0, ok), (s0, toks)
    assert TC.merge([None, None]) == (None, [-1, -1]) and TC.merge([]) == (None, [])
    with pytest.raises(ValueError, match="TokenConstraint or None"):
        TC.merge([a, "b"])


def test_walk_equals_the_reference_on_random_automata():
    rng = np.random.default_rng(3)
    checked = refused = 0
    for _ in range(60):
        n, edges, accepting, default = CR.random_automaton(rng, int(rng.integers(1, 12)), 20)
        c, aut = TC(n, edges, accepting, default), CR.automaton(n, edges, accepting, default)
        assert c.terminal == [CR.is_terminal(aut, s) for s in range(n)]
        assert c.accept == [aut[s]["accept"] for s in range(n)]
        for _ in range(20):
            toks = rng.integers(0, 20, int(rng.integers(0, 8))).tolist()
            s0 = int(rng.integers(0, n))
            want = CR.walk(aut, toks, s0)
            assert c.walk(toks, state=s0) == want, (edges, default, toks, s0)
            checked += 1
            refused += not want[1]
    assert checked == 1200 and 100 < refused < 1100                 # both outcomes occur


def test_constructor_errors():
    with pytest.raises(ValueError, match="duplicate edge: state 0, token 5"):
        TC(2, [(0, 5, 1), (0, 5, 0)], [1])
    for bad in (dict(edges=[(0, 5, 2)]), dict(edges=[(0, 5, -2)]), dict(edges=[(2, 5, 0)]), dict(default=[2, -1]), dict(default=-2),
                dict(default={0: 2}), dict(start=2), dict(start=-1), dict(accepting=[2])):
        kw = dict(dict(edges=[(0, 5, 1)], accepting=[1]), **bad)
        with pytest.raises(ValueError, match=r"must be an int in \["):
            TC(2, kw["edges"], kw["accepting"], **{k: v for k, v in kw.items() if k in ("default", "start")})
    with pytest.raises(ValueError, match="state 1 is a dead end"):
        TC(2, [(0, 5, 1)], [])                                      # closed, not accepting, no edge at all
    with pytest.raises(ValueError, match="state 0 is a dead end"):
        TC(1, [(0, 5, -1)], [])                                     # its only edge is a ban
    TC(1, [(0, 5, -1)], [0])                                        # accepting: a terminal state, fine
    TC(1, [(0, 5, -1)], [], default=0)                              # open: fine
    with pytest.raises(ValueError, match="n_states"):
        TC(0, [], [])
    with pytest.raises(ValueError, match="default lists 1 states"):
        TC(2, [(0, 5, 1)], [1], default=[-1])
    with pytest.raises(ValueError, match="empty choice"):
        TC.from_choices([[5], []])
    with pytest.raises(ValueError, match="at least one choice"):
        TC.from_choices([])
    with pytest.raises(ValueError, match="at least one token"):
        TC.from_allowed_tokens([])


# ---------------------------------------------------------------------------------------------- generate()
def test_check_constraint_args():
    c = TC.from_choices([[5, 6], [7]])
    assert G.check_constraint_args(None, V, num_beams=4, no_repeat_ngram_size=2) is None           # nothing to check without one
    assert G.check_constraint_args(c, V) is None
    with pytest.raises(ValueError, match=r"token id 600 is not in \[0, 512\)"):
        G.check_constraint_args(TC.from_allowed_tokens([3, 600]), V)
    with pytest.raises(ValueError, match=r"token id -1 is not in \[0, 512\)"):
        G.check_constraint_args(TC(1, [(0, -1, -1)], [], default=0), V)
    with pytest.raises(ValueError, match="TokenConstraint"):
        G.check_constraint_args([[5, 6]], V)
    for kw, word in ((dict(num_beams=2), "num_beams > 1"), (dict(assistant_model=object()), "assistant_model"),
                     (dict(prompt_lookup_num_tokens=3), "prompt_lookup_num_tokens"), (dict(speculative_sampling=True), "speculative_sampling")):
        with pytest.raises(ValueError, match=f"cannot be combined with {word}"):
            G.check_constraint_args(c, V, **kw)
    for kw in (dict(no_repeat_ngram_size=2), dict(bad_words_ids=[[4]]), dict(suppress_tokens=[4]), dict(min_new_tokens=3)):
        with pytest.raises(ValueError, match=f"{next(iter(kw))} cannot be combined with a constraint.*not built yet"):
            G.check_constraint_args(c, V, **kw)
    # a closed state needs the V-bit bitmap; open states do not
    with pytest.raises(ValueError, match="524288"):
        G.check_constraint_args(c, 524288 + 32)
    assert G.check_constraint_args(TC(1, [(0, 4, -1)], [], default=0), 524288 + 32) is None
    assert G.check_constraint_args(c, 524288) is None


def test_check_logits_args_is_unchanged():
    assert G.check_logits_args() is None
    assert G.check_logits_args(vocab_size=V, eos_token_id=2) is None
    plan = G.check_logits_args(repetition_penalty=1.2, vocab_size=V)
    assert plan.process and plan.penalty == 1.2 and plan.stops == [] and plan.bad == []
    trivial = G.LogitsPlan(1.0, 0, [], 0, [])                       # what generate() builds for a constraint alone
    assert not trivial.process and trivial.stops == []


def test_output_objects_keep_their_constructors():
    assert G.GreedyOutput("s").constraint_states is None and G.GreedyOutput("s", "c").past_key_values == "c"
    assert G.SampleOutput("s", "l").constraint_states is None and G.SampleOutput("s", "l", "c").past_key_values == "c"
    assert G.GreedyOutput("s", "c", "x").constraint_states == "x" and G.SampleOutput("s", "l", "c", "x").constraint_states == "x"


# ---------------------------------------------------------------------------------------------- generate_batch()
def test_request_params_round_trip():
    c = TC.from_allowed_tokens([1, 2])
    p = G.RequestParams(constraint=c, temperature=0.5)
    assert p.constraint is c and p.temperature == 0.5 and G.RequestParams().constraint is None
    assert "constraint" not in G.RequestParams.FIELDS               # the automaton state is not a column of the parameter table
    assert "constraint=TokenConstraint(n_states=1, edges=2, start=0)" in repr(p) and "temperature=0.5" in repr(p)
    assert repr(G.RequestParams(constraint=G.NO_CONSTRAINT)) == "RequestParams(constraint=NO_CONSTRAINT)"
    assert G.check_batch_args([_rq(p), _rq()], 2, 16) == [16, 16]
    plan = G.check_request_params([_rq(p), _rq()], vocab_size=V)    # the per-request table knows nothing of it
    assert plan.per_request and plan.records[0].temperature == 1.0 and not hasattr(plan.records[0], "constraint")
    assert len(G.RequestPlan.TABLE_FIELDS) == 11 and len(G.RequestPlan.neutral_table(2)) == 12


def test_check_batch_constraint_args_resolves_and_merges():
    P = G.RequestParams
    a, b, call = TC.from_choices([[5, 6], [7]]), TC.from_allowed_tokens([1, 2]), TC.from_choices([[9]])
    assert G.check_batch_constraint_args([_rq(), _rq(P(temperature=0.3))], None, V) is None          # no constraint anywhere
    assert G.check_batch_constraint_args([], call, V) is None
    assert G.check_batch_constraint_args([_rq(P(constraint=G.NO_CONSTRAINT))], call, V) is None      # turned off by every request
    reqs = [_rq(P(constraint=a)), _rq(P(constraint=b)), _rq(P(constraint=G.NO_CONSTRAINT)), _rq(P(constraint=a)), _rq(),
            _rq(P(temperature=0.3))]
    plan = G.check_batch_constraint_args(reqs, call, V)
    # distinct constraints in order of first use: a (4 states), b (1), the call's (2); a is merged once
    assert plan.merged.n_states == 7 and plan.starts == [0, 4, -1, 0, 5, 5]
    assert plan.merged.walk([5, 6], state=0) == (2, True) and plan.merged.walk([2, 1], state=4) == (4, True)
    assert plan.merged.walk([9], state=5) == (6, True) and plan.merged.terminal[6]
    # without a call-level constraint only the requests that bring one are constrained
    plan = G.check_batch_constraint_args(reqs, None, V)
    assert plan.merged.n_states == 5 and plan.starts == [0, 4, -1, 0, -1, -1]


def test_check_batch_constraint_args_errors():
    P = G.RequestParams
    a = TC.from_choices([[5, 6], [7]])
    with pytest.raises(ValueError, match="prompt_lookup_num_tokens"):
        G.check_batch_constraint_args([_rq()], a, V, prompt_lookup_num_tokens=3)
    with pytest.raises(ValueError, match="prompt_lookup_num_tokens"):
        G.check_batch_constraint_args([_rq(), _rq(P(constraint=a))], None, V, prompt_lookup_num_tokens=3)
    assert G.check_batch_constraint_args([_rq()], None, V, prompt_lookup_num_tokens=3) is None
    with pytest.raises(ValueError, match=r"request 1: constraint: token id 600 is not in \[0, 512\)"):
        G.check_batch_constraint_args([_rq(), _rq(P(constraint=TC.from_allowed_tokens([600])))], None, V)
    with pytest.raises(ValueError, match=r"constraint: token id 600"):
        G.check_batch_constraint_args([_rq()], TC.from_allowed_tokens([600]), V)
    with pytest.raises(ValueError, match="request 0: constraint must be a generation.TokenConstraint"):
        G.check_batch_constraint_args([_rq(P(constraint=[[1]]))], None, V)
    # a banning processor in force on a constrained request: its own, or the call's
    with pytest.raises(ValueError, match="request 1: no_repeat_ngram_size cannot be combined with a constraint.*not built yet"):
        G.check_batch_constraint_args([_rq(), _rq(P(constraint=a, no_repeat_ngram_size=2))], None, V)
    with pytest.raises(ValueError, match="request 0: min_new_tokens cannot be combined"):
        G.check_batch_constraint_args([_rq(P(constraint=a))], None, V, min_new_tokens=2)
    with pytest.raises(ValueError, match="request 0: bad_words_ids, suppress_tokens cannot be combined"):
        G.check_batch_constraint_args([_rq()], a, V, bad_words_ids=[[3]], suppress_tokens=[4])
    # ... unless the request turns the call's processor, or the constraint, off; unconstrained requests may ban
    plan = G.check_batch_constraint_args([_rq(P(constraint=a, no_repeat_ngram_size=0)), _rq(), _rq(P(min_new_tokens=4))], None, V,
                                         no_repeat_ngram_size=2)
    assert plan.starts == [0, -1, -1]
    plan = G.check_batch_constraint_args([_rq(P(constraint=G.NO_CONSTRAINT)), _rq(P(no_repeat_ngram_size=0))], a, V,
                                         no_repeat_ngram_size=2)
    assert plan.starts == [-1, 0]
    plan = G.check_batch_constraint_args([_rq(P(constraint=a, repetition_penalty=1.3, stop_sequences=[[4]]))], None, V)
    assert plan.starts == [0]                                       # the penalty and stop sequences ban nothing
