"""Drafting what a constraint forces, on the GPU: lmod_constrain_draft and lmod_constrain_accept against the plain Python reference of
tests/_constrain_draft_ref.py (integers, compared exactly), then generate(constraint=c, constraint_draft_tokens=k) against
generate(constraint=c) - same tokens, same final states, and the round / accepted counts the reference's replay predicts from the
undrafted run's tokens - on the copy model of tests/test_prompt_lookup_gpu.py and on the golden small teacher with an image prompt.
generate() swallows unknown keyword arguments, so the statistics are what shows that the new loop ran."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "llava-mod_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _attn_ref as AR  # noqa: E402
import _constrain_draft_ref as DR  # noqa: E402
import _constrain_ref as CR  # noqa: E402

DEV = "cuda"
BF = torch.bfloat16
I32 = torch.int32
V = 512
EOS = 9
T_MAX = 16


def _tc():
    from llavamod.generation import TokenConstraint
    return TokenConstraint


def _dev(rows):
    return torch.tensor(rows, dtype=I32, device=DEV)


# ------------------------------------------------------------------------------------------------------------- the automata
# Hand-built states, one per clause of the forced rule (V = 512, eos = 9 where one is given):
#   0 one edge                      1 one edge + accepting (forced only without eos)     2 one allowed edge + one banned edge
#   3 one edge inside V + one >= V  4 open, one listed edge                              5 terminal
#   6 accepting, its only edge >= V: no allowed edge inside V                            7 two allowed edges
#   8 one edge whose token is eos   9 only a banned edge, accepting: terminal
# then a chain 10 -100-> 11 -101-> ... -119-> 30 (terminal): 20 forced states in a row.
CHAIN0, CHAIN_END = 10, 30
HAND = (31, [(0, 11, 1), (1, 12, 2), (2, 13, 3), (2, 14, -1), (3, 15, 4), (3, 600, 4), (4, 16, 5), (6, 700, 0), (7, 17, 0), (7, 18, 5),
             (8, 9, 0), (9, 19, -1)] + [(s, 90 + s, s + 1) for s in range(CHAIN0, CHAIN_END)], [1, 5, 6, 9, CHAIN_END], {4: 0})


def _merged(seed):
    """The hand-built states followed by a random automaton (states 31 ..): constructor arguments."""
    rng = np.random.default_rng(seed)
    n, edges, accepting, default = CR.random_automaton(rng, 60, 40, max_edges=3, p_open=0.2)
    off = HAND[0]
    edges = list(HAND[1]) + [(s + off, t, nx + off if nx >= 0 else -1) for s, t, nx in edges]
    dflt = {4: 0}
    dflt.update({s + off: d + off for s, d in enumerate(default) if d >= 0})
    return off + n, edges, list(HAND[2]) + [s + off for s in accepting], dflt


def _tables(args):
    from llavamod import kernels as K
    c = _tc()(*args)
    return c, CR.automaton(*args), K.constraint_table(c, DEV)


# ------------------------------------------------------------------------------------------------------------- draft kernel
def _check_draft(table, aut, pending, state, done, k, eos):
    from llavamod import kernels as K
    got = K.constrain_draft(_dev(pending), _dev(state), _dev(done), table, k, eos, V)
    want = DR.draft(aut, pending, state, done, k, eos, V)
    for name, g, w in zip(("draft", "chunk", "vstate", "n_draft"), got, want):
        assert g.dtype == I32 and g.cpu().tolist() == w, (name, k, eos)
    return want


@pytest.mark.parametrize("k", [1, 4, 15])
def test_constrain_draft_kernel_hand_built_rows(k):
    """Every clause of the forced rule as a start state, with and without eos; a chain longer than k; a chain whose terminal state is
    reached after exactly k and after k - 1 tokens; done rows; rows whose state is outside the automaton."""
    c, aut, table = _tables(HAND)
    assert c.terminal[5] and c.terminal[9] and c.terminal[CHAIN_END] and not c.terminal[6]
    state = list(range(10)) + [CHAIN0, CHAIN_END - k, CHAIN_END - (k - 1), CHAIN_END, 0, CHAIN0, -1, 31, -7]
    done = [0] * 14 + [1, 1, 0, 0, 0]
    pending = [200 + r for r in range(len(state))]
    for eos in (None, EOS):
        draft, chunk, vstate, n = _check_draft(table, aut, pending, state, done, k, eos)
        # the reference's answers, spelled out: the test cannot silently leave the cases it names
        assert n[4:8] == [0, 0, 0, 0] and n[9] == 0                                  # open, terminal, no allowed token, two edges
        assert n[1] == (0 if eos is not None else min(k, 3)) and n[8] == (0 if eos is not None else min(k, 5))
        assert draft[0][0] == 11 and draft[2][0] == 13 and draft[3][0] == 15         # the banned and the >= V edge do not count
        assert n[0] == (1 if eos is not None else min(k, 4))                         # 0 -> 1 (accepting: forced only without eos) ...
        assert n[10] == k and vstate[10] == list(range(CHAIN0, CHAIN0 + k + 1))      # the chain is longer than k
        assert n[11] == k and vstate[11][k] == -1 and vstate[11][:k] == list(range(CHAIN_END - k, CHAIN_END))
        assert n[12] == k - 1 and vstate[12][k - 1] == -1 and vstate[12][k] == -1
        assert n[13] == 0 and vstate[13] == [-1] * (k + 1)                           # a terminal start state masks nothing
        for r in (14, 15, 16, 17, 18):                                               # done rows and states outside the automaton
            assert n[r] == 0 and draft[r] == [-1] * k and vstate[r] == [-1] * (k + 1) and chunk[r] == [pending[r]] * (k + 1)


@pytest.mark.parametrize("k", [1, 4, 15])
@pytest.mark.parametrize("R", [1, 5, 300])
def test_constrain_draft_kernel_equals_reference_on_random_rows(R, k):
    """Random automata behind the hand-built states; R = 300 crosses a 256-thread workgroup.  Several launches per case, so that a
    single row (R = 1) still meets many states."""
    args = _merged(R * 16 + k)
    c, aut, table = _tables(args)
    rng = np.random.default_rng(R + k)
    total = 0
    for launch in range(6 if R < 300 else 2):
        state = rng.integers(-1, args[0] + 1, R).tolist()
        done = (rng.random(R) < 0.15).astype(int).tolist()
        pending = rng.integers(0, V, R).tolist()
        if R == 300:
            state[256], done[256] = CHAIN0, 0                                        # the first row of the second workgroup is live
        for eos in (None, EOS):
            total += sum(_check_draft(table, aut, pending, state, done, k, eos)[3])
    assert total > 0 or R == 1


def test_constrain_draft_and_accept_argument_errors():
    from llavamod import _hip, kernels as K
    c, aut, table = _tables(HAND)
    z = lambda *shape: torch.zeros(shape, dtype=I32, device=DEV)
    for k in (0, T_MAX):
        with pytest.raises(RuntimeError, match="LMOD_EINVAL"):
            K.constrain_draft(z(3), z(3), z(3), table, k, None, V)
        with pytest.raises(RuntimeError, match="LMOD_EINVAL"):
            K.constrain_accept(z(3, k), z(3, k + 1), z(3), z(3), table, None, 0, z(3), 8, z(3))
    e = z(0)
    K.constrain_draft(e, e.clone(), e.clone(), table, 4, None, V)                     # R == 0 is a no-op
    K.constrain_accept(z(0, 4), z(0, 5), e.clone(), e.clone(), table, None, 0, e.clone(), 8, e.clone())
    off, tok, nxt, dflt, flags, n, _ = table
    p = lambda t: t.data_ptr()
    a, b4, b5 = z(2), z(2, 4), z(2, 5)
    ok = [p(a), p(a), p(a), p(off), p(tok), p(nxt), p(dflt), p(flags), n, -1, V, 4, p(b4), p(b5), p(b5), p(a), 2]
    for i in (0, 1, 2, 3, 6, 7, 12, 13, 14, 15):                                     # a null pointer
        bad = list(ok)
        bad[i] = None
        assert _hip.call("lmod_constrain_draft", *bad, allow=(-1,)) == -1
    b9 = z(2, 9)
    ok = [p(b4), p(b5), 4, p(a), p(a), p(off), p(tok), p(nxt), p(dflt), p(flags), n, -1, 0, p(a), 8, p(a), p(b9), p(a), 2]
    for i in (0, 1, 3, 4, 5, 8, 9, 13, 15, 16, 17):
        bad = list(ok)
        bad[i] = None
        assert _hip.call("lmod_constrain_accept", *bad, allow=(-1,)) == -1


# ------------------------------------------------------------------------------------------------------------- accept kernel
def _check_accept(table, aut, draft, target, done, state, n_gen, budget, lens, k, eos, pad):
    from llavamod import kernels as K
    d, s, g, L = _dev(done), _dev(state), _dev(n_gen), _dev(lens)
    block, nxt = K.constrain_accept(_dev(draft).view(-1, k), _dev(target).view(-1, k + 1), d, s, table, eos, pad, g, budget, L)
    want = DR.accept(aut, draft, target, done, state, n_gen, budget, lens, k, eos, pad)
    for name, got, w in zip(("block", "next", "done", "state", "n_gen", "lens_target"), (block, nxt, d, s, g, L), want):
        assert got.dtype == I32 and got.cpu().tolist() == w, (name, k, eos)
    return want


# a chain of closed states 0 -100-> 1 -101-> ... -129-> 30 (terminal), nothing accepting on the way
ACHAIN = (31, [(s, 100 + s, s + 1) for s in range(30)], [30], None)


@pytest.mark.parametrize("k", [1, 4, 15])
def test_constrain_accept_kernel_hand_built_rows(k):
    """Each of the four cuts at the first, a middle and the last candidate of a fully accepted run; n_acc = 0 and n_acc = k without a
    cut; a done row, whose lens_target returns to L0."""
    c, aut, table = _tables(ACHAIN)
    pad, budget, L0 = 3, 40, 50
    rows, expect = [], []

    def row(s0, n_acc, done=0, n_gen=1, cut=None, tok_at=None):
        toks = [100 + s0 + j for j in range(k + 1)]
        if tok_at is not None:
            toks[tok_at[0]] = tok_at[1]
        draft = toks[:n_acc] + [-1] * (k - n_acc)
        target = toks[:n_acc + 1] + [499] * (k - n_acc)
        rows.append((draft, target, done, s0, n_gen, L0 + k + 1))
        expect.append(cut)

    for p in sorted({0, k // 2, k}):                                                 # the first, a middle and the last candidate
        row(0, k, cut=("eos", p), tok_at=(p, EOS))
        row(0, k, cut=("left", p), tok_at=(p, 498))
        row(30 - (p + 1), k, cut=("terminal", p))
        row(0, k, n_gen=budget - (p + 1), cut=("budget", p))
    row(0, 0)
    row(0, k)
    row(5, k, done=1)
    row(0, k // 2)
    cols = list(zip(*rows))
    block, nxt, done, state, n_gen, lens = _check_accept(table, aut, *[list(col) for col in cols[:5]], budget, list(cols[5]), k, EOS, pad)
    for r, (cut, (draft, target, was_done, s0, ng, _)) in enumerate(zip(expect, rows)):
        if cut is None:
            continue
        why, p = cut
        assert block[r][k + 2] == p + 1 and done[r] == 1 and nxt[r] == pad and lens[r] == L0 + p + 1, (r, cut, block[r])
        assert block[r][k + 1] == k and n_gen[r] == ng + p + 1
        assert state[r] == {"eos": s0 + p, "left": s0 + p, "terminal": 30, "budget": s0 + p + 1}[why], (r, cut, state[r])
    r = len(rows) - 4
    assert block[r][k + 1:] == [0, 1, 100, 0] and state[r] == 1 and lens[r] == L0 + 1                                   # n_acc = 0
    assert block[r + 1][:k + 1] == [100 + j for j in range(k + 1)] and block[r + 1][k + 1:] == [k, k + 1, 100 + k, 0]  # n_acc = k
    assert state[r + 1] == k + 1 and lens[r + 1] == L0 + k + 1 and n_gen[r + 1] == k + 2
    assert block[r + 2] == [pad] * (k + 1) + [0, 0, pad, 1] and (state[r + 2], n_gen[r + 2], lens[r + 2]) == (5, 1, L0)  # done at entry


@pytest.mark.parametrize("k", [1, 4, 15])
@pytest.mark.parametrize("R", [1, 5, 300])
def test_constrain_accept_kernel_equals_reference_on_random_rows(R, k):
    args = _merged(R * 16 + k + 1)
    c, aut, table = _tables(args)
    rng = np.random.default_rng(R * 3 + k)
    budget, emitted = 8, 0
    for launch in range(6 if R < 300 else 2):
        target = rng.integers(0, 41, (R, k + 1))                                     # 40: no state lists it
        draft = target[:, :k].copy()
        for r in range(R):                                                           # a random accepted prefix, then a mismatch or -1
            m = int(rng.integers(0, k + 1))
            if m < k:
                draft[r, m] = -1 if rng.random() < 0.5 else (target[r, m] + 1) % 41
                draft[r, m + 1:] = rng.integers(-1, 41, k - m - 1)
        state = rng.integers(-1, args[0] + 1, R).tolist()
        done = (rng.random(R) < 0.15).astype(int).tolist()
        n_gen = rng.integers(0, 11, R).tolist()                                      # some rows are at or past the budget already
        lens = rng.integers(k + 1, 200, R).tolist()
        if R == 300:
            state[256], done[256], n_gen[256] = 31, 0, 0
        for eos in (None, 10):
            want = _check_accept(table, aut, draft.tolist(), target.tolist(), done, state, n_gen, budget, lens, k, eos, 2)
            emitted += sum(b[k + 2] for b in want[0])
    assert emitted > 0


# ------------------------------------------------------------------------------------------------------------- generate()
def _plain_with_gaps(model, kw):
    """generate(constraint=c, return_dict_in_generate=True) and, per step, which rows' masked top-2 gap is >= 8 bf16 ulps of the top
    logit (the rule of _greedy_with_gaps in tests/test_assisted_gpu.py; one allowed token: the gap is infinite)."""
    from llavamod import kernels as K
    orig, oks = K.row_argmax, []

    def spy(lg):
        t2 = lg.float().topk(2, -1).values
        oks.append(((t2[:, 0] - t2[:, 1]) >= 8 * AR.ulp_bf16(t2[:, 0].cpu()).to(DEV).float()).cpu().tolist())
        return orig(lg)

    K.row_argmax = spy
    try:
        out = model.generate(**kw, return_dict_in_generate=True)
    finally:
        K.row_argmax = orig
    return out, oks


def _compare(model, fresh, c, k, eos=None, pad=None, max_new=12):
    """fresh(): the call's prompt arguments (a new cache each time when the call continues one).  The plain constrained run first,
    with the precondition on the inputs (every unforced state of that run is decided by >= 8 bf16 ulps), then the drafted run."""
    from llavamod.generation import AssistedOutput, GreedyOutput
    kw = dict(max_new_tokens=max_new, eos_token_id=eos, pad_token_id=pad, constraint=c)
    ref, oks = _plain_with_gaps(model, dict(fresh(), **kw))
    assert isinstance(ref, GreedyOutput)
    seq = ref.sequences.cpu()
    seqs, rounds, acc, states = DR.simulate(c, seq.tolist(), k, eos, max_new)
    assert len(oks) == seq.shape[1]
    for b, row in enumerate(seqs):                                                    # the precondition, on the live steps of each row
        assert seq[b, :len(row)].tolist() == row
        for i in range(len(row)):
            s, ok = c.walk(row[:i])
            assert ok
            if c.forced(s, eos, V) is None:
                assert oks[i][b], ("the plain run's top-2 gap at an unforced state fell below 8 bf16 ulps", b, i, row)
    assert ref.constraint_states.cpu().tolist() == states
    out = model.generate(**fresh(), **kw, constraint_draft_tokens=k, return_dict_in_generate=True)
    assert isinstance(out, AssistedOutput)
    assert torch.equal(out.sequences.cpu(), seq), (out.sequences, seq)
    assert out.constraint_states.dtype == I32 and out.constraint_states.cpu().tolist() == states
    print(f"k {k}: plain {seq.shape[1]} steps -> {out.num_rounds} rounds, accepted {out.num_accepted.tolist()}, rows {seqs}")
    assert out.num_rounds == rounds and out.num_accepted.tolist() == acc, (out.num_rounds, rounds, out.num_accepted, acc)
    assert out.num_target_forwards == out.num_rounds + 1 < seq.shape[1], (out.num_target_forwards, seq.shape)
    assert torch.equal(model.generate(**fresh(), **kw, constraint_draft_tokens=k).cpu(), seq)       # the bare tensor
    return ref, out, (seqs, rounds, acc, states)


def _copy_case():
    """The copy model follows the permutation PI by a wide margin.  A ragged batch of three prompts ending in p0, p1, p2 and ONE
    from_choices constraint: every branch state allows exactly one token equal to pi(previous token) (the root: pi(p_b) for each row,
    so each row takes its own branch) and the forced runs are tokens that are NOT pi(previous): only the mask makes them the argmax.
      row 0: [a, pi(a), y1 .. y7]            9 tokens, the branch after the first token, then 7 forced
      row 1: [b, z1 .. z4, pi(z4), w1, w2]   8 tokens, 4 forced, the branch after the fifth token, 2 forced
      row 2: [c, pi(c), pi(pi(c))]           3 tokens, a branch at every state, nothing forced."""
    from test_prompt_lookup_gpu import PI, walk
    rows = [walk(7, 5), [200, 300, 450], walk(32, 4)[:3] + [60]]
    a, b, cc = (PI[r[-1]] for r in rows)
    y = [100, 110, 120, 130, 140, 150, 160]
    z = [170, 180, 190, 210]
    w = [220, 230]
    decoys = [240, 250, 260, 270, 280, 290]
    choices = [[a, PI[a]] + y, [a, decoys[0], decoys[1]],
               [b] + z + [PI[z[-1]]] + w, [b] + z + [decoys[2]],
               [cc, PI[cc], PI[PI[cc]]], [cc, decoys[3], decoys[4]], [cc, PI[cc], decoys[5]]]
    want = [choices[0], choices[2], choices[4]]
    assert len({a, b, cc}) == 3 and all(PI[s] != t for ch in (y, z, w) for s, t in zip(ch, ch[1:]))
    assert PI[PI[a]] != y[0] and PI[b] != z[0] and PI[PI[z[-1]]] != w[0]
    assert not set(decoys) & {t for ch in want for t in ch}
    return rows, choices, want


@pytest.mark.parametrize("k", [1, 4, 15])
def test_generate_on_the_copy_model_drafts_the_forced_runs(k):
    from test_prompt_lookup_gpu import _copy_model, _pad_rows
    model = _copy_model()
    rows, choices, want = _copy_case()
    assert sorted(len(ch) for ch in want) == [3, 8, 9]
    c = _tc().from_choices(choices)
    ids, am = _pad_rows(rows)
    fresh = lambda: dict(input_ids=ids, attention_mask=am)
    ref, out, (seqs, rounds, acc, states) = _compare(model, fresh, c, k)
    assert seqs == want and all(c.terminal[s] for s in states)
    # the forced tokens are emitted as drafts: 7 in row 0, 4 + 2 in row 1 (k = 1: every second one is the token behind the draft)
    assert acc == {1: [4, 3, 0], 4: [6, 6, 0], 15: [7, 6, 0]}[k] and rounds == {1: 5, 4: 3, 15: 2}[k]
    # the cache holds the prompt and every returned token but each row's last
    n_prompt = torch.tensor([len(r) for r in rows])
    assert out.past_key_values.lens.cpu().tolist() == (n_prompt + torch.tensor([len(s) for s in seqs]) - 1).tolist()


# ---- the golden small teacher with an image prompt
@pytest.fixture(scope="module")
def teacher():
    from test_constrain_gpu import _build_teacher
    return _build_teacher()


def _prompt():
    from test_constrain_gpu import _prompt as p
    return p()


@pytest.fixture(scope="module")
def plain(teacher):
    """The unconstrained greedy output [2, 24] of the image prompt (computed once, never modified)."""
    return teacher.generate(**_prompt(), max_new_tokens=24).cpu()


def _free(plain, *more):
    from test_constrain_gpu import _free_tokens
    return _free_tokens(plain, *more)


def _root_choices(firsts, tails, decoy):
    """One choice per distinct first token (each row's unconstrained argmax: the root's branch is decided by the model) with a forced
    tail of tokens the model would not emit, and a decoy choice."""
    out, seen = [], set()
    for t, tail in zip(firsts, tails):
        if t not in seen:
            out.append([t] + tail)
            seen.add(t)
    return out + [decoy]


@pytest.mark.parametrize("k", [1, 4, 15])
def test_generate_on_the_teacher_with_eos_in_an_accepting_state(teacher, plain, k):
    """The first choice is a proper prefix of the second: behind its forced run sits an accepting state that is not terminal, where
    eos_token_id and the longer choice's next token are both allowed - a branch again, whichever way the model takes it (on the golden
    fixture row 0 takes EOS there: at k >= 3 it is the token behind a fully accepted draft, at k = 1 the token behind the third)."""
    f = _free(plain)
    t0, t1 = int(plain[0, 0]), int(plain[1, 0])
    short = [t0, f[0], f[1], f[2]]
    choices = [short] + _root_choices([t0, t1], [[f[0], f[1], f[2], f[3], f[4], f[5]], [f[6], f[7]]], [f[8], f[9], f[10]])
    c = _tc().from_choices(choices)
    eos = f[11]
    s, _ = c.walk(short)
    assert c.accept[s] and not c.terminal[s] and c.forced(s) is not None and c.forced(s, eos, V) is None
    ref, out, (seqs, rounds, acc, states) = _compare(teacher, _prompt, c, k, eos=eos, pad=3)
    assert seqs[0][:4] == short and acc[0] >= 2 and seqs[0][-1] in (eos, f[5])
    if seqs[0][-1] == eos:
        assert states[0] == s                                                        # ended by EOS: the state stays where it accepted


def test_generate_on_the_teacher_across_two_turns(teacher):
    """Turn 1 is plain greedy (three identical runs, three caches); turn 2 feeds turn 1's last token and a ragged text against that
    cache: unconstrained (its first tokens give the root's branch), constrained, and constrained with drafts."""
    p = _prompt()

    def turn2():
        o = teacher.generate(**p, max_new_tokens=4, return_dict_in_generate=True)
        ids = torch.cat([o.sequences[:, -1:].cpu(), torch.tensor([[17, 40, 41, 5], [23, 40, 41, 0]])], 1)
        return dict(input_ids=ids, attention_mask=torch.tensor([[1, 1, 1, 1, 1], [1, 1, 1, 1, 0]]).bool(), past_key_values=o.past_key_values)

    free_run = teacher.generate(**turn2(), max_new_tokens=8).cpu()
    f = _free(free_run)
    firsts = [int(free_run[0, 0]), int(free_run[1, 0])]
    c = _tc().from_choices(_root_choices(firsts, [[f[0], f[1], f[2], f[3], f[4]], [f[5], f[6], f[7]]], [f[8], f[9]]))
    for k in (1, 4):
        ref, out, (seqs, rounds, acc, states) = _compare(teacher, turn2, c, k)
        assert all(c.terminal[s] for s in states) and sum(acc) > 0
        lens0 = turn2()["past_key_values"].lens.cpu() + torch.tensor([5, 4])           # the cache behind turn 2's live tokens
        assert out.past_key_values.lens.cpu().tolist() == (lens0 + torch.tensor([len(s) for s in seqs]) - 1).tolist()


@pytest.mark.parametrize("k", [1, 4, 15])
def test_generate_on_the_teacher_max_new_tokens_cuts_a_forced_run(teacher, plain, k):
    f = _free(plain)
    t0, t1 = int(plain[0, 0]), int(plain[1, 0])
    c = _tc().from_choices(_root_choices([t0, t1], [[f[0], f[1], f[2], f[3], f[4], f[5]], [f[6], f[7], f[8], f[9], f[10], f[11]]], [f[12]]))
    ref, out, (seqs, rounds, acc, states) = _compare(teacher, _prompt, c, k, max_new=4)
    assert [len(s) for s in seqs] == [4, 4] and not any(c.accept[s] for s in states)  # the caller sees that the answers are incomplete
    assert states == [c.walk(s)[0] for s in seqs] and rounds == {1: 2, 4: 1, 15: 1}[k]
    prompt_lens = teacher.generate(**_prompt(), max_new_tokens=1, return_dict_in_generate=True).past_key_values.lens.cpu()
    assert out.past_key_values.lens.cpu().tolist() == (prompt_lens + 4 - 1).tolist()
    assert torch.equal(out.past_key_values.lens, ref.past_key_values.lens)


# ------------------------------------------------------------------------------------------------------------- off means off
def test_without_the_argument_the_new_kernels_never_run(monkeypatch):
    from llavamod import kernels as K
    from test_prompt_lookup_gpu import _copy_model, _pad_rows, walk
    model = _copy_model()
    rows, choices, _ = _copy_case()
    c = _tc().from_choices(choices)
    ids, am = _pad_rows(rows)
    lookup = dict(input_ids=torch.tensor([walk(7, 12)]), max_new_tokens=11, prompt_lookup_num_tokens=4)
    before = (model.generate(input_ids=ids, attention_mask=am, max_new_tokens=12, constraint=c), model.generate(**lookup))

    def never(*a, **k):
        raise AssertionError("a constraint-draft kernel ran in a call without `constraint_draft_tokens`")

    monkeypatch.setattr(K, "constrain_draft", never)
    monkeypatch.setattr(K, "constrain_accept", never)
    assert torch.equal(model.generate(input_ids=ids, attention_mask=am, max_new_tokens=12, constraint=c), before[0])
    assert torch.equal(model.generate(**lookup), before[1])
    assert model.generate(input_ids=ids, attention_mask=am, max_new_tokens=3).shape == (3, 3)
    with pytest.raises(AssertionError, match="constraint-draft kernel ran"):
        model.generate(input_ids=ids, attention_mask=am, max_new_tokens=12, constraint=c, constraint_draft_tokens=4)


def test_argument_errors_raise_before_any_device_work(monkeypatch):
    from test_prompt_lookup_gpu import _copy_model, walk
    model = _copy_model()
    c = _tc().from_choices([[5, 6], [7]])
    kw = dict(input_ids=torch.tensor([walk(7, 5)]), max_new_tokens=4)

    def never(*a, **k):
        raise AssertionError("device work started before the arguments were checked")

    monkeypatch.setattr(model, "_start", never)
    with pytest.raises(ValueError, match="needs a constraint"):
        model.generate(**kw, constraint_draft_tokens=4)
    for bad, word in ((dict(constraint_draft_tokens=0), "1..15"), (dict(constraint_draft_tokens=T_MAX), "1..15"),
                      (dict(constraint_draft_tokens=4, do_sample=True), "greedy"), (dict(constraint_draft_tokens=4, num_beams=2), "num_beams"),
                      (dict(constraint_draft_tokens=4, num_return_sequences=2), "one sequence per prompt"),
                      (dict(constraint_draft_tokens=4, assistant_model=model), "assistant_model"),
                      (dict(constraint_draft_tokens=4, assistant_model=model, speculative_sampling=True), "speculative_sampling"),
                      (dict(constraint_draft_tokens=4, prompt_lookup_num_tokens=3), "prompt_lookup_num_tokens"),
                      (dict(constraint_draft_tokens=4, repetition_penalty=1.3), "repetition_penalty"),
                      (dict(constraint_draft_tokens=4, stop_sequences=[[5, 6]]), "stop_sequences"),
                      (dict(constraint_draft_tokens=4, no_repeat_ngram_size=2), "no_repeat_ngram_size")):
        with pytest.raises(ValueError, match=word):
            model.generate(**kw, constraint=c, **bad)
    with pytest.raises(AssertionError, match="device work started"):
        model.generate(**kw, constraint=c, constraint_draft_tokens=4)
