"""generate_batch(prompt_lookup_num_tokens=k) on the GPU: lmod_batch_lookup_first / lmod_batch_lookup_round against their restatement
(tests/_batch_lookup_ref.py, exact), and the loop on the copy model of tests/test_prompt_lookup_gpu.py (greedy continuation known,
tie-free asserted) and on the golden teacher with images: tokens against generate() alone, admissions / rounds / accepted counts
against the replay."""
import functools
import os
import random
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _batch_lookup_ref as BR  # noqa: E402

DEV = "cuda"
FILL = 3                      # dead history positions hold a symbol of the alphabet, not a sentinel


def _dev(x):
    return torch.tensor(x, dtype=torch.int32).to(DEV)


def _hist(rows, ld):
    h = torch.full((len(rows), ld), FILL, dtype=torch.int32)
    for r, row in enumerate(rows):
        h[r, :len(row)] = torch.tensor(row, dtype=torch.int32)
    return h


# ------------------------------------------------------------------------------------------------ lmod_batch_lookup_round
def _check_round(rows, k, eos, pad, stops, ld):
    """rows: dicts as BR.clause_rows builds them.  The kernel's block and every array it updates equal the restatement."""
    from llavamod import kernels as K
    B = len(rows)
    exp_block, exp_done, exp_hist, exp_gen, exp_lens = BR.run_rows(rows, k, eos, pad, stops, ld)
    done, n_hist = _dev([r["done"] for r in rows]), _dev([len(r["hist"]) for r in rows])
    hist, n_prompt = _hist([r["hist"] for r in rows], ld).to(DEV), _dev([r["n_prompt"] for r in rows])
    n_gen, budget, lens = _dev([r["n_gen"] for r in rows]), _dev([r["budget"] for r in rows]), _dev([r["cache_len"] for r in rows])
    block = K.batch_lookup_round_(_dev([r["draft"] for r in rows]).view(B, k), _dev([r["target"] for r in rows]).view(B, k + 1),
                                  _dev([r["first_tok"] for r in rows]), done, hist, n_hist, n_prompt, n_gen, budget, lens, eos, pad,
                                  K.seq_table(stops, DEV))
    got = [t.cpu().tolist() for t in (block, done, n_hist, n_gen, lens)]
    assert got[0] == exp_block, [(s, a, b) for s, (a, b) in enumerate(zip(got[0], exp_block)) if a != b][:3]
    assert got[1] == exp_done and got[2] == [len(h) for h in exp_hist] and got[3] == exp_gen and got[4] == exp_lens
    assert torch.equal(hist.cpu(), _hist(exp_hist, ld))              # the emitted tokens, and nothing behind them
    return exp_block


@pytest.mark.parametrize("k", [1, 4, 15])
def test_round_clause_rows(k):
    """The eight hand-built slots (tests/test_batch_lookup_cpu.py writes their k = 4 results out and pins each row's kind at every k)."""
    rows = BR.clause_rows(k)
    assert len(rows) == 8
    block = _check_round(rows, k, BR.EOS, BR.PAD, BR.STOPS, BR.LD)
    assert block[0][k + 5] == 77 and block[0][k + 4] == 1 and block[2][k + 1] == k and block[1][k + 1] == 0
    _check_round(rows, k, None, 5, [], BR.LD)                         # no eos, no stop table (null pointers), another pad


def _random_rows(rng, B, k, ld):
    rows = []
    for _ in range(B):
        n_prompt, n_gen = rng.randint(1, 8), rng.randint(1, 12)
        hist = [rng.randint(0, 7) for _ in range(n_prompt + n_gen)]
        if rng.random() < 0.05:                                       # a history row that is full, or fills up inside the run
            hist = (hist * ld)[:ld - rng.randint(0, 2)]
            n_gen = len(hist) - n_prompt
        target = [rng.randint(0, 7) for _ in range(k + 1)]
        nd = rng.randint(0, k)
        draft = [target[j] if rng.random() < 0.8 else rng.randint(0, 7) for j in range(nd)] + [-1] * (k - nd)
        rows.append(dict(draft=draft, target=target, first_tok=rng.choice([-1, -1, rng.randint(0, 7)]), done=int(rng.random() < 0.15),
                         hist=hist, n_prompt=n_prompt, n_gen=n_gen, budget=n_gen + rng.randint(1, 6),
                         cache_len=rng.randint(0, 40) + (k + 1 if rng.random() < 0.95 else -rng.randint(0, k))))
    return rows


def test_round_random_rows():
    """B = 257 (two workgroups and a tail), k = 4, 20 seeds: an 8-symbol alphabet, so eos, the three stop sequences, the budget and a
    full history all cut runs; a few rows carry lens below k + 1."""
    k, ld = 4, 24
    fins, cuts = 0, 0
    for seed in range(20):
        rows = _random_rows(random.Random(seed), 257, k, ld)
        block = _check_round(rows, k, 6, 0, [[1, 2], [3], [4, 5, 4]], ld)
        fins += sum(b[k + 4] for b, r in zip(block, rows) if not r["done"])
        cuts += sum(b[k + 2] < b[k + 1] + 1 for b, r in zip(block, rows) if not r["done"])
    assert fins > 500 and cuts > 200, (fins, cuts)                    # the fixture stays in its domain


# ------------------------------------------------------------------------------------------------ lmod_batch_lookup_first
def _check_first(rows, eos, stops, ld):
    """rows: (token, done, hist, n_prompt, n_gen, budget)."""
    from llavamod import kernels as K
    exp = [BR.first_row(t, d, h, p, g, b, eos, stops, ld) for t, d, h, p, g, b in rows]
    done, hist, n_hist = _dev([r[1] for r in rows]), _hist([r[2] for r in rows], ld).to(DEV), _dev([len(r[2]) for r in rows])
    n_prompt, n_gen, budget = _dev([r[3] for r in rows]), _dev([r[4] for r in rows]), _dev([r[5] for r in rows])
    first = K.batch_lookup_first_(_dev([r[0] for r in rows]), done, hist, n_hist, n_prompt, n_gen, budget, eos, K.seq_table(stops, DEV))
    assert first.cpu().tolist() == [e[0] for e in exp] and done.cpu().tolist() == [e[1] for e in exp]
    assert n_hist.cpu().tolist() == [len(e[2]) for e in exp] and n_gen.cpu().tolist() == [e[3] for e in exp]
    assert torch.equal(hist.cpu(), _hist([e[2] for e in exp], ld))
    return exp


def test_first_rows():
    rows = [(7, 0, [1, 2], 2, 0, 5),                 # fresh
            (7, 0, [1, 2, 8], 2, 1, 5),              # running
            (7, 1, [1, 2, 8, 9], 2, 2, 5),           # done
            (7, 1, [1, 2], 2, 0, 5),                 # done before it ever ran (an empty slot)
            (7, 0, [1, 2], 2, 0, 1),                 # budget 1
            (9, 0, [1, 2], 2, 0, 5),                 # eos first
            (4, 0, [1, 2], 2, 0, 5),                 # a one-token stop sequence
            (5, 0, [1, 6], 2, 0, 5),                 # 6 5 would need the prompt's 6
            (7, 0, list(range(16)), 16, 0, 5)]       # a full history row
    exp = _check_first(rows, 9, [[4], [6, 5]], 16)
    assert [e[0] for e in exp] == [7, -1, -1, -1, 7, 9, 4, 5, -1] and [e[1] for e in exp] == [0, 0, 1, 1, 1, 1, 1, 0, 1]
    _check_first(rows, None, [], 16)
    for seed in range(3):                            # two workgroups and a tail
        rng = random.Random(seed)
        many = [(rng.randint(0, 7), int(rng.random() < 0.2), [rng.randint(0, 7) for _ in range(rng.randint(1, 16))], 0,
                 rng.choice([0, 0, 0, 2]), rng.randint(1, 3)) for _ in range(257)]
        many = [(t, d, h, max(len(h) - g, 0), g, b) for t, d, h, _, g, b in many]
        _check_first(many, 6, [[1, 2], [3]], 16)


def test_argument_errors_launch_nothing():
    from llavamod import _hip
    B, k, ld = 4, 4, 8
    z = lambda *s: torch.zeros(s, dtype=torch.int32, device=DEV)
    a = dict(draft=z(B, 15), target=z(B, 16), first=z(B), done=z(B), hist=z(B, ld), n_hist=z(B), n_prompt=z(B), n_gen=z(B),
             budget=z(B) + 9, lens=z(B) + 20, block=z(B, 32), tokens=z(B))
    p = {n: t.data_ptr() for n, t in a.items()}

    def rnd(k=k, B=B, n_stop=0, **null):
        q = {**p, **{n: None for n in null}}
        return _hip.call("lmod_batch_lookup_round", q["draft"], q["target"], q["first"], k, q["done"], q["hist"], ld, q["n_hist"],
                         q["n_prompt"], q["n_gen"], q["budget"], q["lens"], -1, 0, None, None, n_stop, q["block"], B, allow=(-1,))

    def fst(B=B, n_stop=0, **null):
        q = {**p, **{n: None for n in null}}
        return _hip.call("lmod_batch_lookup_first", q["tokens"], q["done"], q["hist"], ld, q["n_hist"], q["n_prompt"], q["n_gen"],
                         q["budget"], -1, None, None, n_stop, q["first"], B, allow=(-1,))
    assert rnd(k=0) == -1 and rnd(k=16) == -1 and rnd(B=-1) == -1 and rnd(n_stop=1) == -1          # LMOD_EINVAL
    for name in ("draft", "target", "first", "done", "hist", "n_hist", "n_prompt", "n_gen", "budget", "lens", "block"):
        assert rnd(**{name: 1}) == -1, name
    for name in ("tokens", "done", "hist", "n_hist", "n_prompt", "n_gen", "budget", "first"):
        assert fst(**{name: 1}) == -1, name
    assert fst(B=-1) == -1 and fst(n_stop=1) == -1
    torch.cuda.synchronize()
    assert all(int(t.sum()) == 0 for n, t in a.items() if n not in ("budget", "lens"))               # nothing was launched
    assert rnd(B=0) == 0 and fst(B=0) == 0 and rnd(k=15) == 0 and rnd(k=1) == 0 and fst() == 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ the loop: the copy model
K_, N_ = 4, 2
CYCLE = None                  # filled by _fix(): the prompts and their plain-greedy continuations


@functools.lru_cache(maxsize=None)
def _fix():
    """The three prompts (a 5-cycle walked more than twice: every draft accepted; the 64-cycle: none; planted wrong continuations:
    part, none and all of a draft) with plain greedy's continuation, tie-free as far as any request below reads it (asserted)."""
    from test_prompt_lookup_gpu import PI, _copy_model, _greedy_with_gaps, walk
    model = _copy_model()
    a, b, c, d, e = walk(7, 5)
    prompts = dict(cycle=walk(7, 12), none=[200, 300, 450], planted=[a, b, 100, 102, 103, a, b, c, 101, 104, d, e])
    need = dict(cycle=24, none=24, planted=12)
    greedy = {}
    for name, p in prompts.items():
        toks, safe = _greedy_with_gaps(model, dict(input_ids=torch.tensor([p])), need[name])
        assert int(safe.min()) == need[name], ("the copy model's top-2 gap fell below 8 bf16 ulps", name, safe)
        greedy[name] = toks[0].tolist()
        assert greedy[name] == walk(PI[p[-1]], need[name])
    return model, prompts, greedy


def _requests(names, budgets):
    _, prompts, _ = _fix()
    return [dict(input_ids=torch.tensor(prompts[n]), max_new_tokens=m) for n, m in zip(names, budgets)]


def _spied(model, fn):
    """Run fn() with `_admit` and `forward_append` spied on: admissions [(iteration, request, slot)] and per verification pass
    (lens before, lens after, smax)."""
    adm, passes = [], []
    orig_admit, orig_fa = model._admit, model.model.forward_append

    def admit(requests, budgets, group, st, **kw):
        adm.extend((len(passes), r, s) for r, s in group)
        return orig_admit(requests, budgets, group, st, **kw)

    def fa(emb, cache, n_new, T=None, max_len=None):
        before = cache.lens.cpu().tolist()
        assert max_len is not None and max(before) <= max_len
        out = orig_fa(emb, cache, n_new, T=T, max_len=max_len)
        passes.append((before, cache.lens.cpu().tolist(), cache.smax))
        assert max(passes[-1][1]) <= cache.smax, passes[-1]
        return out
    model._admit, model.model.forward_append = admit, fa
    try:
        return fn(), adm, passes
    finally:
        model._admit, model.model.forward_append = orig_admit, orig_fa


def _replay(names, budgets, B, **kw):
    _, prompts, greedy = _fix()
    return BR.replay([prompts[n] for n in names], [greedy[n] for n in names], K_, N_, 512, budgets, B, **kw)


def test_loop_mixed_requests():
    """Five requests through two slots: tokens are generate()'s on each request alone and plain generate_batch's; who was admitted
    when, the rounds and the accepted counts are the replay's; fewer rounds than plain decode steps."""
    from llavamod.generation import BatchOutput
    model, prompts, greedy = _fix()
    names, budgets = ["cycle", "none", "cycle", "none", "planted"], [11, 3, 24, 1, 7]
    rq = _requests(names, budgets)
    out, adm, passes = _spied(model, lambda: model.generate_batch(rq, max_batch_size=2, prompt_lookup_num_tokens=K_,
                                                                  max_matching_ngram_size=N_, return_dict_in_generate=True))
    assert isinstance(out, BatchOutput) and out.token_logprobs is None
    plain = model.generate_batch(rq, max_batch_size=2, return_dict_in_generate=True)
    for i, (n, m) in enumerate(zip(names, budgets)):
        alone = model.generate(input_ids=torch.tensor([prompts[n]]), max_new_tokens=m)[0]
        assert alone.tolist() == greedy[n][:m]
        assert out.sequences[i].dtype == torch.int64 and out.sequences[i].tolist() == greedy[n][:m], (i, out.sequences[i])
        assert torch.equal(plain.sequences[i], out.sequences[i])
    toks, r_adm, rounds, acc, _ = _replay(names, budgets, 2)
    assert toks == [s.tolist() for s in out.sequences]
    assert adm == r_adm and out.num_rounds == rounds == len(passes) and out.num_target_forwards == rounds, (adm, r_adm, out.num_rounds)
    assert out.num_accepted == acc and acc[0] == 8 and acc[1] == acc[3] == 0 and acc[2] >= 16 and 0 < acc[4] < 6, acc
    assert out.num_admissions == 5 and out.num_prefills == len({i for i, _, _ in adm})
    assert out.num_rounds < plain.num_decode_steps, (out.num_rounds, plain.num_decode_steps)
    seqs = model.generate_batch(rq, max_batch_size=2, prompt_lookup_num_tokens=K_, max_matching_ngram_size=N_)    # a plain list
    assert isinstance(seqs, list) and all(torch.equal(a, b) for a, b in zip(seqs, out.sequences))
    assert model.generate_batch([], max_batch_size=2, prompt_lookup_num_tokens=K_, max_matching_ngram_size=N_) == []


@pytest.mark.parametrize("how", ["eos", "stop"])
def test_loop_request_ends_inside_an_accepted_run(how):
    """Request 0's first round accepts 4 drafts; eos (or the 2-token stop sequence) is its 3rd token: it ends there, its slot takes
    request 2 in the next iteration, and the request beside it is untouched."""
    model, prompts, greedy = _fix()
    names, budgets = ["cycle", "none", "cycle"], [11, 12, 6]
    g = greedy["cycle"]
    kw = dict(eos_token_id=g[2], pad_token_id=1) if how == "eos" else dict(stop_sequences=[[g[1], g[2]]])
    rkw = dict(eos=g[2], pad=1) if how == "eos" else dict(stops=[[g[1], g[2]]])
    rq = _requests(names, budgets)
    out, adm, passes = _spied(model, lambda: model.generate_batch(rq, max_batch_size=2, prompt_lookup_num_tokens=K_,
                                                                  max_matching_ngram_size=N_, return_dict_in_generate=True, **kw))
    assert [s.tolist() for s in out.sequences] == [g[:3], greedy["none"][:12], g[:3]]
    assert adm == [(0, 0, 0), (0, 1, 1), (1, 2, 0)]                   # slot 0 is refilled in the very next iteration
    toks, r_adm, rounds, acc, _ = _replay(names, budgets, 2, **rkw)
    assert toks == [s.tolist() for s in out.sequences] and adm == r_adm and out.num_rounds == rounds and out.num_accepted == acc
    assert acc[0] == 2 and acc[1] == 0
    plain = model.generate_batch(rq, max_batch_size=2, **kw)
    assert all(torch.equal(a, b) for a, b in zip(plain, out.sequences))
    crit = type("Crit", (), dict(keyword_ids=[torch.tensor([g[1], g[2]])]))()
    if how == "stop":                                                # the reference's criterion object carries the same sequence
        again = model.generate_batch(rq, max_batch_size=2, prompt_lookup_num_tokens=K_, max_matching_ngram_size=N_,
                                     stopping_criteria=[crit])
        assert all(torch.equal(a, b) for a, b in zip(again, out.sequences))


def test_loop_cache_is_bounded_and_an_idle_slot_stays_put():
    """The cycle request ends after two rounds; the 64-cycle request then runs alone for 21 more.  lens <= smax after every pass, the
    cache never grows, every round starts from the replay's cache lengths, and the idle slot's length never moves."""
    model, prompts, greedy = _fix()
    names, budgets = ["cycle", "none"], [11, 24]
    out, adm, passes = _spied(model, lambda: model.generate_batch(_requests(names, budgets), max_batch_size=2,
                                                                  prompt_lookup_num_tokens=K_, max_matching_ngram_size=N_,
                                                                  return_dict_in_generate=True))
    toks, _, rounds, acc, lens = _replay(names, budgets, 2)
    assert [s.tolist() for s in out.sequences] == toks == [greedy["cycle"][:11], greedy["none"][:24]]
    assert out.num_rounds == rounds == 23 == len(passes) and out.num_accepted == acc == [8, 0]
    assert len({p[2] for p in passes}) == 1 and passes[0][2] == max(12 + 11, 3 + 24) + K_ + 1   # smax: never grew
    for i in range(1, rounds):
        assert passes[i][0] == lens[i - 1], (i, passes[i][0], lens[i - 1])
        assert passes[i][1] == [n + K_ + 1 for n in lens[i - 1]]
    idle = [p[0][0] for p in passes[2:]]
    assert len(idle) == 21 and set(idle) == {12 + 11 - 1}


# ------------------------------------------------------------------------------------------------ the loop: the golden teacher
def test_loop_images_and_text_on_the_golden_teacher():
    """The unmodified teacher: its two tie-free image prompts and a text request through two slots; tokens are generate()'s on each
    request alone, over the steps whose top-2 gap keeps the two kernel paths' argmax comparable."""
    from test_assisted_gpu import _greedy_with_gaps
    from test_batch_gpu import _alone, _greedy_refs, _prompts, _teacher
    teacher, refs = _teacher(), _greedy_refs()
    text = _prompts()[0]["input_ids"]
    text = text[text >= 0]
    t_toks, t_safe = _greedy_with_gaps(teacher, dict(input_ids=text[None], attention_mask=None, images=None), 8)
    rq = [dict(_prompts()[0], max_new_tokens=8), dict(input_ids=text, max_new_tokens=5), dict(_prompts()[1], max_new_tokens=6),
          dict(_prompts()[0], max_new_tokens=3)]
    want = [refs[0], (t_toks[0].cpu(), int(t_safe[0])), refs[1], refs[0]]
    assert min(refs[0][1], refs[1][1]) >= 6 and int(t_safe[0]) >= 1
    for k, n_max in ((4, 2), (15, 8)):
        out = teacher.generate_batch(rq, max_batch_size=2, prompt_lookup_num_tokens=k, max_matching_ngram_size=n_max,
                                     return_dict_in_generate=True)
        assert out.num_admissions == 4 and out.num_rounds >= 2 and len(out.num_accepted) == 4
        for i, (seq, (ref, safe)) in enumerate(zip(out.sequences, want)):
            m = rq[i]["max_new_tokens"]
            n = min(m, safe)
            assert seq.shape == (m,) and torch.equal(seq[:n].cpu(), ref[:n]), (k, i, seq, ref)
    assert torch.equal(teacher.generate(**_alone(0), max_new_tokens=8)[0].cpu(), refs[0][0])
