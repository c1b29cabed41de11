"""Constrained decoding on the device: lmod_constrain_mask_rows_bf16 and lmod_constrain_advance_rows against the dict-of-dicts
reference of tests/_constrain_ref.py (exact bf16 bit equality over the whole block, padding columns included, so an element the
mask must not touch was not written), then generate(constraint=...) on the golden small teacher against a step-by-step loop written
here (cached forwards, the reference mask on the host, the product's selection kernel, the reference push and advance: both sides
select from bit-identical rows, so the tokens are equal token for token) and generate_batch(constraint=...) against generate() of
every request alone."""
import functools
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
import _constrain_ref as CR  # noqa: E402
import _logits_ref as LR  # noqa: E402
import _util as U  # noqa: E402

DEV = "cuda"
BF = torch.bfloat16
I32 = torch.int32


def _tc():
    from llavamod.generation import TokenConstraint
    return TokenConstraint


def _bits(t):
    """bf16 tensor (any device) -> numpy uint16 of its bit patterns."""
    return t.detach().cpu().contiguous().view(torch.int16).numpy().view(np.uint16)


# ------------------------------------------------------------------------------------------------------------- mask kernel
@functools.lru_cache(maxsize=None)
def _mask_automaton(V):
    """(constructor arguments, eos) of the automaton the mask test walks through state by state:
      0 closed, only token 0            1 closed, only token V-1           2 closed, every token (nothing is written)
      3 closed + accepting, a few tokens around the bitmap's word and byte boundaries (EOS joins them)
      4 terminal: accepting, closed, no edge (only EOS is left)
      5 open, not accepting: two banned tokens, one redirected token that stays, EOS banned
      6 open + accepting: one banned token, EOS stays
      7 closed, not accepting: a whole 8-element vector, a partial one, and listed bans that change nothing in a closed state."""
    t = lambda *ids: sorted({i % V for i in ids})
    eos = 5 % V
    edges = [(0, 0, 0), (1, V - 1, 1)] + [(2, i, 2) for i in range(V)]
    edges += [(3, i, 0) for i in t(1, 31, 32, 33, 63, 64, V - 2, V - 9)]
    edges += [(5, i, -1) for i in t(7, V - 3)] + [(5, i, 6) for i in t(12) if i not in t(7, V - 3)]
    edges += [(6, t(9)[0], -1)]
    keep7 = t(*range(8, 16), 16, 18, 23, 40, V - 1)
    edges += [(7, i, 3) for i in keep7] + [(7, i, -1) for i in t(3, 41, V - 5) if i not in keep7]
    return (8, tuple(edges), (3, 4, 6), (-1, -1, -1, -1, -1, 6, 5, -1)), eos


@functools.lru_cache(maxsize=None)
def _mask_logits(V, ld, R):
    """Random bf16 [R, ld] with NaN, +inf, -inf and -0 planted where states 0, 1, 3 and 7 allow a token (and elsewhere)."""
    g = torch.Generator().manual_seed(V + R)
    x = (torch.randn(R, ld, generator=g) * 4).to(BF)
    x[:, 0] = float("nan")
    x[:, V - 1] = float("-inf")
    x[:, 1 % V] = -0.0
    if V > 64:
        x[:, 32], x[:, 33], x[:, 18], x[:, 40] = float("inf"), float("nan"), -0.0, float("-inf")
        x[:, [2, 50, V - 4]] = float("nan")              # banned in every closed state: they become -inf
    return x


STATES = [-1, 8, 0, 1, 2, 3, 4, 5, 6, 7]                  # -1 and n_states: out of range, untouched


@pytest.mark.parametrize("with_eos", [True, False])
@pytest.mark.parametrize("V,ld,R", [(151936, 151936, 3), (1000, 1008, 4), (1003, 1003, 4), (2, 2, 2)])
def test_constrain_mask_kernel_equals_reference_bitwise(V, ld, R, with_eos):
    """Every state kind at every row position (the launches rotate through STATES): with the odd stride 1003 only row 0 is 16-byte
    aligned, so each kind is swept by the vector path and by the scalar path."""
    from llavamod import kernels as K
    (n, edges, accepting, default), eos = _mask_automaton(V)
    eos = eos if with_eos else None
    c = _tc()(n, list(edges), list(accepting), list(default))
    aut = CR.automaton(n, edges, accepting, list(default))
    assert c.terminal[4] and not c.terminal[3] and c.flags[5] == 0
    table = K.constraint_table(c, DEV)
    x = _mask_logits(V, ld, R)
    xb = _bits(x)
    changed = kept = 0
    for o in range(len(STATES)):
        states = [STATES[(o + r) % len(STATES)] for r in range(R)]
        want = xb.copy()
        want[:, :V] = CR.mask(aut, xb[:, :V], states, eos)
        xd, sd = x.to(DEV), torch.tensor(states, dtype=I32, device=DEV)
        got = K.constrain_mask_(xd[:, :V], sd, table, eos)
        assert got.data_ptr() == xd.data_ptr() and sd.tolist() == states
        gb = _bits(xd)
        diff = np.argwhere(gb != want)
        assert diff.size == 0, (states, diff[:8].tolist(), [(hex(gb[tuple(d)]), hex(want[tuple(d)])) for d in diff[:4]])
        for r, s in enumerate(states):                    # allowed elements kept their bits, NaN / inf / -0 included
            if s in aut:
                ok = [tok for tok in aut[s]["edges"] if CR.allowed(aut, s, tok, eos)][:64]
                assert all(gb[r, tok] == xb[r, tok] for tok in ok), (s, r)
                kept += len(ok)
            else:
                assert np.array_equal(gb[r], xb[r]), (s, r)
        changed += int((gb != xb).sum())
    assert changed > 0 and kept > 0


def test_constrain_mask_vocabulary_beyond_the_bitmap():
    """A closed state's bitmap holds 524288 tokens (64 KB of LDS): beyond that a constraint with a closed state raises ValueError and
    launches nothing; open states need no bitmap and run."""
    from llavamod import kernels as K
    V = 524288 + 32
    x = torch.zeros(2, V, dtype=BF, device=DEV)
    state = torch.zeros(2, dtype=I32, device=DEV)
    closed = K.constraint_table(_tc().from_allowed_tokens([3, V - 1]), DEV)
    with pytest.raises(ValueError, match="524288"):
        K.constrain_mask_(x, state, closed, 7)
    assert float(x.abs().sum()) == 0
    mixed = K.constraint_table(_tc()(2, [(0, 3, -1), (1, 4, 1)], [1], default=[0, -1]), DEV)      # a closed state no row sits in
    with pytest.raises(ValueError, match="524288"):
        K.constrain_mask_(x, state, mixed, 7)
    assert float(x.abs().sum()) == 0
    opened = K.constraint_table(_tc()(1, [(0, 3, -1), (0, V - 1, -1), (0, 9, 0)], [], default=0), DEV)
    K.constrain_mask_(x, state, opened, 7)
    assert torch.isinf(x[:, [3, 7, V - 1]]).all() and int(torch.isinf(x).sum()) == 6


# ------------------------------------------------------------------------------------------------------------- advance kernel
def test_constrain_advance_kernel_hand_built_rows():
    """already done / state -1 / a listed edge / the default edge / a banned edge (done set, state kept) / an edge into a terminal
    state (done set); then the out-of-range state n_states and a token that has no edge in a closed state."""
    from llavamod import kernels as K
    # 0 open (default 1): 5 -> 2, 6 banned; 1 closed: 7 -> 3, 8 -> 0; 2 closed + accepting: 9 -> 2; 3 terminal
    args = (4, [(0, 5, 2), (0, 6, -1), (1, 7, 3), (1, 8, 0), (2, 9, 2)], [2, 3], [1, -1, -1, -1])
    c, aut = _tc()(*args), CR.automaton(*args)
    table = K.constraint_table(c, DEV)
    tokens = [5, 5, 5, 400, 6, 7, 5, 9]
    done = [1, 0, 0, 0, 0, 0, 0, 0]
    state = [0, -1, 0, 0, 0, 1, 4, 1]
    want_done, want_state = CR.advance(aut, tokens, done, state)
    assert want_done.tolist() == [1, 0, 0, 0, 1, 1, 0, 1] and want_state.tolist() == [0, -1, 2, 1, 0, 3, 4, 1]
    t, d, s = (torch.tensor(v, dtype=I32, device=DEV) for v in (tokens, done, state))
    K.constrain_advance_(t, d, s, table)
    assert d.tolist() == want_done.tolist() and s.tolist() == want_state.tolist() and t.tolist() == tokens
    e = torch.zeros(0, dtype=I32, device=DEV)
    K.constrain_advance_(e, e.clone(), e.clone(), table)                        # R == 0 is a no-op


def test_constrain_advance_kernel_random_rows_across_a_block():
    from llavamod import kernels as K
    rng = np.random.default_rng(5)
    args = CR.random_automaton(rng, 50, 40, max_edges=12)
    c, aut = _tc()(*args), CR.automaton(*args)
    table = K.constraint_table(c, DEV)
    R = 257
    tokens = rng.integers(0, 40, R).astype(np.int32)
    done = (rng.random(R) < 0.2).astype(np.int32)
    state = rng.integers(-1, 51, R).astype(np.int32)                            # -1 and 50 are outside the automaton
    state[256] = 3
    done[256] = 0                                                               # the row behind the first block is live
    want_done, want_state = CR.advance(aut, tokens, done, state)
    assert 0 < int((want_state != state).sum()) and int(want_done.sum()) > int(done.sum())
    t, d, s = (torch.from_numpy(v).to(DEV) for v in (tokens, done, state))
    K.constrain_advance_(t, d, s, table)
    assert np.array_equal(d.cpu().numpy(), want_done) and np.array_equal(s.cpu().numpy(), want_state)


# ------------------------------------------------------------------------------------------------------------- generate()
N_NEW = 24
PAD = 3


def _build_teacher():
    """The golden small teacher (tests/golden/gpusmall_teacher.safetensors) as the HIP model."""
    from oracle.decoder import DecoderConfig
    from oracle.vision import VisionConfig
    from llavamod.model import LlavaQwen2ForCausalLM
    vc = VisionConfig(hidden_size=64, intermediate_size=128, num_hidden_layers=3, num_attention_heads=1, image_size=28, patch_size=14,
                      select_layer=-2)
    tc = DecoderConfig(vocab_size=512, hidden_size=128, intermediate_size=256, num_hidden_layers=2, num_attention_heads=2,
                       num_key_value_heads=2)
    model = LlavaQwen2ForCausalLM(U.hip_configs(tc, vc, moe=False)[0], device=DEV)
    mapped = {U.oracle_to_hip_key(k): v for k, v in U.load_golden("gpusmall_teacher.safetensors").items()}
    own = model.state_dict()
    assert set(mapped) == set(own)
    with torch.no_grad():
        for k, t in own.items():
            t.copy_(mapped[k].to(device=t.device, dtype=t.dtype))
    model.eval()
    return model


@pytest.fixture(scope="module")
def teacher():
    t = _build_teacher()
    t.generation_budget = N_NEW        # the loop's use_cache prefill then sizes its cache exactly as generate(max_new_tokens=24) does
    return t


def _prompt():
    g = U.load_golden("gpusmall_mimic.safetensors")
    b = {k.split(".")[-1]: v for k, v in g.items() if k.startswith("ragged_kdlm.batch.")}
    return dict(input_ids=b["input_ids"], attention_mask=b["attention_mask"].bool(), images=b["images"].to(DEV).to(BF))


@pytest.fixture(scope="module")
def plain(teacher):
    """The unconstrained 24-token greedy output [2, 24] (computed once, never modified)."""
    return teacher.generate(**_prompt(), max_new_tokens=N_NEW).cpu()


def _aut_of(c):
    return CR.automaton(c.n_states, c.edges(), [s for s in range(c.n_states) if c.accept[s]], list(c.default_next))


def _loop(model, p, n_new, c, eos=None, pad=None, sample=None, n=1, past=None, penalty=1.0):
    """generate(constraint=c) restated: HF-style cached forwards, the reference processors and the reference mask on the returned
    logits (host), the product's selection kernel, the reference push and advance.  n > 1: the prefill's cache is replicated row by
    row, as generate() does.  Returns (tokens [B*n, <= n_new], token log-probabilities or None, final states)."""
    from llavamod import kernels as K
    from llavamod.model.language_model.qwen2_hip import KVCache
    aut = _aut_of(c)
    ids = p["input_ids"].to(I32)
    am = p.get("attention_mask")
    n_prompt = am.to(I32).sum(1).to(I32) if am is not None else torch.full((ids.shape[0],), ids.shape[1], dtype=I32)
    hist = torch.zeros((ids.shape[0], ids.shape[1] + n_new), dtype=I32)
    hist[:, :ids.shape[1]] = ids
    B = ids.shape[0]
    if past is None:
        o = model(input_ids=p["input_ids"], attention_mask=p["attention_mask"], images=p["images"], use_cache=True)
        logits = o.logits[:, -1]
    else:
        past.grow(int(past.lens.max()) + p["input_ids"].shape[1] + n_new)
        o = model(input_ids=p["input_ids"], attention_mask=p.get("attention_mask"), past_key_values=past)
        logits = o.logits[torch.arange(B), (n_prompt - 1).long()]
    cache = o.past_key_values
    if n > 1:
        cfg = model.config
        pc, cache = cache, KVCache(cfg.num_hidden_layers, B * n, cache.smax, cfg.num_key_value_heads * cfg.head_dim, DEV)
        cache.lens.copy_(pc.lens.repeat_interleave(n))
        K.kv_gather_rows(cache.tensors(), pc.tensors(), torch.arange(B * n, device=DEV, dtype=I32) // n, cache.lens)
        logits, hist, n_prompt = logits.repeat_interleave(n, 0), hist.repeat_interleave(n, 0), n_prompt.repeat_interleave(n)
        B = B * n
    n_hist, n_gen, done = n_prompt.clone(), torch.zeros_like(n_prompt), torch.zeros_like(n_prompt)
    state = np.full(B, c.start, dtype=np.int32)
    gen = torch.Generator(device=DEV).manual_seed(sample["seed"]) if sample else None
    can_stop = eos is not None or c.has_terminal
    out, lps = [], []
    for step in range(n_new):
        x = LR.process_logits(logits.to(BF).cpu(), hist, n_hist, n_gen, penalty=penalty, eos=eos)
        x = torch.from_numpy(CR.mask(aut, _bits(x), state, eos).view(np.int16)).view(BF).to(DEV)
        if sample:
            u = torch.rand(B, generator=gen, device=DEV)
            tok, st = K.sample(x, u, sample["temperature"], None, sample["top_p"], stats=True)
            xt = x.gather(1, tok.long()[:, None]).squeeze(1).double() / sample["temperature"]
            lp = (xt - st[:, 0].double() - torch.log(st[:, 1].double())).clamp(max=0.0).float()
            lps.append(torch.where(done.to(DEV) != 0, torch.zeros_like(lp), lp))
        else:
            tok = K.row_argmax(x)
        tok, done, hist, n_hist, n_gen = LR.push_stop(tok.cpu(), done, hist, n_hist, n_prompt, n_gen, eos, pad, [])
        d, state = CR.advance(aut, tok.numpy(), done.numpy(), state)
        done = torch.from_numpy(d).to(done.dtype)
        out.append(tok.long())
        if step + 1 == n_new or (can_stop and bool(done.all())):
            break
        logits = model(input_ids=tok.long()[:, None], past_key_values=cache).logits[:, 0]
    return torch.stack(out, 1), (torch.stack(lps, 1).cpu() if lps else None), state


def _free_tokens(*outputs):
    """Token ids that none of the given outputs contains, ascending (PAD left out too)."""
    used = {PAD}
    for o in outputs:
        used |= set(int(t) for t in o.reshape(-1).tolist())
    return sorted(set(range(512)) - used)


@pytest.mark.parametrize("with_eos", [False, True])
def test_generate_greedy_with_choices_equals_the_loop(teacher, plain, with_eos):
    """Choices built from tokens the unconstrained output does not contain: the mask decides every step.  One choice is a proper
    prefix of another (an accepting state that is not terminal).  Without an eos_token_id every row runs into a terminal state;
    with one (a token the unconstrained output does not contain either) a row may also end with EOS in an accepting state."""
    f = _free_tokens(plain)
    choices = [[f[0], f[1], f[2]], [f[0], f[1]], [f[3], f[4]], [f[5]], [f[0], f[6], f[7], f[8]]]
    eos = f[9] if with_eos else None
    c = _tc().from_choices(choices)
    p = _prompt()
    out = teacher.generate(**p, max_new_tokens=N_NEW, constraint=c, eos_token_id=eos, pad_token_id=PAD, return_dict_in_generate=True)
    want, _, want_state = _loop(teacher, p, N_NEW, c, eos=eos, pad=PAD)
    got = out.sequences.cpu()
    assert torch.equal(got, want), (got, want)
    assert out.constraint_states.dtype == I32 and out.constraint_states.cpu().tolist() == want_state.tolist()
    assert got.shape[1] <= 5 < N_NEW                                            # the terminal states ended the loop early
    for b in range(got.shape[0]):
        row = got[b].tolist()
        cut = row.index(eos) if eos in row else len(row)
        body = row[:cut]
        while body and body[-1] == PAD and body not in choices:
            body.pop()
        assert body in choices, (b, row)
        assert all(t == PAD for t in row[len(body) + (eos in row):]), (b, row)
        s = int(out.constraint_states[b])
        assert c.walk(body) == (s, True) and c.accept[s] and (c.terminal[s] or eos in row), (b, row, s)
    if not with_eos:
        assert all(c.terminal[int(s)] for s in out.constraint_states)
    assert not torch.equal(got, plain[:, :got.shape[1]])
    # the bare tensor is the same tokens
    assert torch.equal(teacher.generate(**p, max_new_tokens=N_NEW, constraint=c, eos_token_id=eos, pad_token_id=PAD).cpu(), got)


def test_generate_max_new_tokens_cuts_an_answer_short(teacher, plain):
    f = _free_tokens(plain)
    c = _tc().from_choices([[f[0], f[1], f[2], f[3]]])
    out = teacher.generate(**_prompt(), max_new_tokens=2, constraint=c, return_dict_in_generate=True)
    assert out.sequences.cpu().tolist() == [[f[0], f[1]]] * 2
    assert out.constraint_states.cpu().tolist() == [2, 2] and not c.accept[2]       # the caller sees that the answer is incomplete


def test_generate_with_a_constraint_and_a_repetition_penalty_in_a_continuation(teacher):
    """past_key_values: the new turn goes through the chunk path, the state starts at `start` again; repetition_penalty bans nothing and
    combines with the constraint (the penalty runs first, the mask last)."""
    p = _prompt()

    def first_turn():
        o = teacher.generate(**p, max_new_tokens=4, return_dict_in_generate=True)
        turn = torch.cat([o.sequences[:, -1:].cpu(), torch.tensor([[17, 40, 41, 5], [23, 40, 41, 0]])], 1)
        return o.past_key_values, dict(input_ids=turn, attention_mask=torch.tensor([[1, 1, 1, 1, 1], [1, 1, 1, 1, 0]]).bool())

    c = _tc().from_allowed_tokens([17, 40, 41, 200, 300])
    cache, turn = first_turn()
    got = teacher.generate(**turn, past_key_values=cache, max_new_tokens=N_NEW, constraint=c, repetition_penalty=1.3).cpu()
    cache, turn = first_turn()
    want, _, _ = _loop(teacher, turn, N_NEW, c, past=cache, penalty=1.3)
    assert torch.equal(got, want), (got, want)
    assert got.shape == (2, N_NEW) and set(got.reshape(-1).tolist()) <= {17, 40, 41, 200, 300}


def test_an_open_automaton_that_bans_nothing_changes_no_token(teacher, plain):
    c = _tc()(1, [], [], default=0)
    out = teacher.generate(**_prompt(), max_new_tokens=N_NEW, constraint=c, return_dict_in_generate=True)
    assert torch.equal(out.sequences.cpu(), plain)
    assert out.constraint_states.cpu().tolist() == [0, 0]


def test_without_a_constraint_the_constrain_kernels_never_run(teacher, plain, monkeypatch):
    from llavamod import kernels as K

    def never(*a, **k):
        raise AssertionError("a constrain kernel ran in a call without `constraint`")

    for name in ("constrain_mask_", "constrain_advance_", "constraint_table"):
        monkeypatch.setattr(K, name, never)
    p = _prompt()
    assert torch.equal(teacher.generate(**p, max_new_tokens=N_NEW).cpu(), plain)
    out = teacher.generate(**p, max_new_tokens=N_NEW, repetition_penalty=1.2, return_dict_in_generate=True)
    assert out.constraint_states is None and out.sequences.shape == (2, N_NEW)
    reqs, P = _batch_requests([4, 4, 4]), _params()
    assert [len(s) for s in teacher.generate_batch(reqs, max_batch_size=2)] == [4, 4, 4]
    reqs[1]["params"] = P(temperature=0.7, do_sample=True, seed=1)
    assert [len(s) for s in teacher.generate_batch(reqs, max_batch_size=2)] == [4, 4, 4]
    with pytest.raises(AssertionError, match="constrain kernel ran"):
        teacher.generate(**p, max_new_tokens=2, constraint=_tc().from_allowed_tokens([1]))


def test_generate_sampling_with_an_allow_list_equals_the_loop(teacher):
    allow = [11, 57, 130, 256, 400]
    c = _tc().from_allowed_tokens(allow)
    p = _prompt()
    kw = dict(temperature=0.7, top_p=0.9, seed=7)
    out = teacher.generate(**p, max_new_tokens=N_NEW, do_sample=True, num_return_sequences=2, constraint=c, return_dict_in_generate=True,
                           **kw)
    want, lps, state = _loop(teacher, p, N_NEW, c, sample=kw, n=2)
    assert out.sequences.shape == (4, N_NEW) and set(out.sequences.reshape(-1).tolist()) <= set(allow)
    assert torch.equal(out.sequences.cpu(), want), (out.sequences, want)
    assert torch.equal(out.token_logprobs.cpu(), lps)
    assert bool(torch.isfinite(out.token_logprobs).all()) and bool((out.token_logprobs <= 0).all())
    assert out.constraint_states.cpu().tolist() == state.tolist() == [0] * 4
    assert len(set(out.sequences.reshape(-1).tolist())) > 1                      # it sampled: not one token throughout


# ------------------------------------------------------------------------------------------------------------- generate_batch()
NEW = 8
ORDER = [0, 1, 1, 0, 0]                 # the fixture's two prompts, issued as five requests


def _params():
    from llavamod.generation import RequestParams
    return RequestParams


@functools.lru_cache(maxsize=None)
def _batch_teacher():
    return _build_teacher()


@functools.lru_cache(maxsize=None)
def _batch_prompts():
    """The two prompts of tests/golden/append_prompt.safetensors (the tie-free fixture of the generate_batch tests) as single requests."""
    g = U.load_golden("append_prompt.safetensors")
    n = g["attention_mask"].sum(1)
    images = g["images"].to(DEV).to(BF)
    return tuple(dict(input_ids=g["input_ids"][p, :int(n[p])], images=images[p:p + 1]) for p in range(2))


def _batch_requests(budgets):
    return [dict(_batch_prompts()[p], max_new_tokens=m) for p, m in zip(ORDER, budgets)]


def _alone(teacher, p, c, **kw):
    """generate() of prompt p alone under constraint c (None: unconstrained): its tokens cut behind the token that finished it, and the
    number of leading steps whose top-2 gap of the MASKED logits (what lmod_row_argmax_bf16 is given) is >= 8 bf16 ulps - the rule
    the generate_batch tests hold token equality across the two paths to.  One allowed token: the gap is infinite."""
    from llavamod import kernels as K
    pr = _batch_prompts()[p]
    ids = pr["input_ids"][None]
    orig, oks = K.row_argmax, []

    def spy(lg):
        t2 = lg.float().topk(2, -1).values
        oks.append(bool(((t2[:, 0] - t2[:, 1]) >= 8 * AR.ulp_bf16(t2[:, 0].cpu()).to(DEV).float()).all()))
        return orig(lg)

    K.row_argmax = spy
    try:
        out = teacher.generate(input_ids=ids, attention_mask=torch.ones_like(ids, dtype=torch.bool), images=pr["images"],
                               max_new_tokens=NEW, constraint=c, pad_token_id=PAD, return_dict_in_generate=True, **kw)
    finally:
        K.row_argmax = orig
    seq = out.sequences[0].cpu()
    if c is not None and c.terminal[int(out.constraint_states[0])]:
        n = next(i + 1 for i in range(len(seq)) if c.terminal[c.walk(seq[:i + 1].tolist())[0]])
        assert bool((seq[n:] == PAD).all())
        seq = seq[:n]
    return seq, (oks + [False]).index(False)


def _scheduled_steps(budgets, B, lengths):
    """num_decode_steps of the CPU scheduler when request r emits lengths[r] tokens: a slot freed in one step is refilled before the next."""
    from llavamod.generation import SlotScheduler
    sched, emitted = SlotScheduler(budgets, B), [0] * len(budgets)
    while not sched.finished:
        sched.admit()
        live = sched.live
        for r in live.values():
            emitted[r] += 1
        sched.step([s for s, r in live.items() if emitted[r] == lengths[r] < budgets[r]])
    return sched.num_decode_steps


def _batch_constraints(teacher):
    free = [_alone(teacher, p, None)[0] for p in range(2)]
    f = _free_tokens(*free)
    A = _tc().from_choices([[f[0], f[1], f[2]], [f[3], f[4]]])
    Bc = _tc().from_choices([[f[5]], [f[6], f[7], f[8], f[9]], [f[6], f[7]]])
    allow = _tc().from_allowed_tokens([f[10], f[11], f[12], f[13]])
    call = _tc().from_choices([[f[14], f[15]], [f[16]]])
    return free, A, Bc, allow, call


def _check_batch(teacher, out, per_request, budgets):
    """Every request's tokens against its own generate() call over the tie-safe prefix, cut where generate() cuts it; the slots were
    refilled in the steps the scheduler needs for these lengths."""
    lengths = [len(s) for s in out.sequences]
    safe_all = True
    for i, (p, c) in enumerate(zip(ORDER, per_request)):
        ref, safe = _alone(teacher, p, c)
        ref = ref[:budgets[i]]
        n = min(len(ref), safe)
        print(f"request {i}: prompt {p}, {len(ref)} tokens alone, tie-safe for {safe} steps, batch gave {out.sequences[i].tolist()}")
        assert torch.equal(out.sequences[i][:n].cpu(), ref[:n]), (i, out.sequences[i], ref, safe)
        if safe >= len(ref):
            assert lengths[i] == len(ref) and torch.equal(out.sequences[i].cpu(), ref), (i, out.sequences[i], ref)
        else:
            safe_all = False
    # precondition, stated: the fixture and the chosen tokens keep every request tie-free, so each was compared in full
    assert safe_all
    assert out.num_admissions == 5
    assert out.num_decode_steps == _scheduled_steps(budgets, 2, lengths)
    return lengths


def test_generate_batch_with_a_constraint_per_request():
    """Five requests through two slots in `_generate_batch_rows` (a request with `params` forces it): two different choice sets, the
    call's constraint turned off (it refills a slot that served a constrained request and emits its unconstrained tokens), an
    allow-list, and one without `params` that inherits the call's constraint."""
    from llavamod.generation import NO_CONSTRAINT, BatchOutput
    teacher, P = _batch_teacher(), _params()
    free, A, Bc, allow, call = _batch_constraints(teacher)
    budgets = [NEW, NEW, NEW, 5, NEW]
    reqs = _batch_requests(budgets)
    for rq, prm in zip(reqs, [P(constraint=A), P(constraint=Bc), P(constraint=NO_CONSTRAINT), P(constraint=allow), None]):
        if prm is not None:
            rq["params"] = prm
    out = teacher.generate_batch(reqs, max_batch_size=2, constraint=call, pad_token_id=PAD, return_dict_in_generate=True)
    assert isinstance(out, BatchOutput) and len(out.token_logprobs) == 5         # the rows loop ran
    lengths = _check_batch(teacher, out, [A, Bc, None, allow, call], budgets)
    assert lengths[0] <= 3 and lengths[1] <= 4 and lengths[4] <= 2               # finished by a terminal state, and freed
    assert lengths[2] == NEW and torch.equal(out.sequences[2][:6].cpu(), free[ORDER[2]][:6])
    assert lengths[3] == 5 and set(out.sequences[3].tolist()) <= set(allow.edge_tok)
    for seq, c in ((out.sequences[0], A), (out.sequences[1], Bc), (out.sequences[4], call)):
        s, ok = c.walk(seq.tolist())
        assert ok and c.terminal[s], (seq, s)


def test_generate_batch_with_a_call_level_constraint_in_the_plain_loop():
    """No request has `params`: the loop generate_batch always ran, plus the two launches.  Every request inherits the call's choices;
    a slot finished by a terminal state is refilled on the next iteration."""
    teacher = _batch_teacher()
    _, A, _, _, _ = _batch_constraints(teacher)
    budgets = [NEW, 2, NEW, NEW, 1]
    out = teacher.generate_batch(_batch_requests(budgets), max_batch_size=2, constraint=A, pad_token_id=PAD, return_dict_in_generate=True)
    assert out.token_logprobs is None                                            # the plain loop ran
    lengths = _check_batch(teacher, out, [A] * 5, budgets)
    assert all(n <= 3 for n in lengths) and lengths[4] == 1 and lengths[1] == 2
    for i in (0, 2, 3):
        s, ok = A.walk(out.sequences[i].tolist())
        assert ok and A.terminal[s]
    # sampling from an allow-list in the plain loop: every token is in the set, and the call is reproducible
    _, _, _, allow, _ = _batch_constraints(teacher)
    kw = dict(max_batch_size=2, constraint=allow, do_sample=True, temperature=1.5, seed=5, return_dict_in_generate=True)
    a, b = teacher.generate_batch(_batch_requests([4] * 5), **kw), teacher.generate_batch(_batch_requests([4] * 5), **kw)
    assert all(len(s) == 4 and set(s.tolist()) <= set(allow.edge_tok) for s in a.sequences)
    assert all(torch.equal(x, y) for x, y in zip(a.sequences, b.sequences))
    assert all(bool(torch.isfinite(lp).all()) for lp in a.token_logprobs)


# ------------------------------------------------------------------------------------------------------------- argument errors
def test_constraint_argument_errors_raise_before_any_launch(teacher, monkeypatch):
    from llavamod.generation import RequestParams as P
    c = _tc().from_choices([[5, 6], [7]])
    p = _prompt()

    def never(*a, **k):
        raise AssertionError("device work started before the arguments were checked")

    monkeypatch.setattr(teacher, "_start", never)
    for kw, word in ((dict(num_beams=2), "num_beams > 1"), (dict(assistant_model=teacher), "assistant_model"),
                     (dict(prompt_lookup_num_tokens=3), "prompt_lookup_num_tokens"),
                     (dict(assistant_model=teacher, speculative_sampling=True), "speculative_sampling"),
                     (dict(no_repeat_ngram_size=2), "no_repeat_ngram_size"), (dict(bad_words_ids=[[4]]), "bad_words_ids"),
                     (dict(suppress_tokens=[4]), "suppress_tokens"), (dict(min_new_tokens=2, eos_token_id=9), "min_new_tokens")):
        with pytest.raises(ValueError, match=word):
            teacher.generate(**p, max_new_tokens=2, constraint=c, **kw)
    with pytest.raises(ValueError, match=r"token id 512 is not in \[0, 512\)"):
        teacher.generate(**p, max_new_tokens=2, constraint=_tc().from_allowed_tokens([512]))
    with pytest.raises(ValueError, match="TokenConstraint"):
        teacher.generate(**p, max_new_tokens=2, constraint=[[5, 6]])
    reqs = _batch_requests([2] * 5)
    with pytest.raises(ValueError, match="prompt_lookup_num_tokens"):
        teacher.generate_batch(reqs, max_batch_size=2, constraint=c, prompt_lookup_num_tokens=3, max_matching_ngram_size=2)
    with pytest.raises(ValueError, match="request 0: no_repeat_ngram_size cannot be combined with a constraint"):
        teacher.generate_batch(reqs, max_batch_size=2, constraint=c, no_repeat_ngram_size=2)
    reqs[3]["params"] = P(constraint=_tc().from_allowed_tokens([600]))
    with pytest.raises(ValueError, match="request 3: constraint: token id 600"):
        teacher.generate_batch(reqs, max_batch_size=2)
    reqs[3]["params"] = P(constraint=c, min_new_tokens=2)
    with pytest.raises(ValueError, match="request 3: min_new_tokens cannot be combined"):
        teacher.generate_batch(reqs, max_batch_size=2, eos_token_id=9)
