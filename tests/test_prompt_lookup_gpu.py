"""Prompt-lookup decoding on the GPU: lmod_ngram_draft / lmod_hist_push_block against tests/_lookup_ref.py (exact), and the
generate(prompt_lookup_num_tokens=...) loop on a copy model whose greedy continuation is known, and on the golden teacher."""
import os
import random
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _lookup_ref as LR  # noqa: E402
import _util as U  # noqa: E402

DEV = "cuda"
IMG = -200
VK = 100                      # the kernel tests' vocabulary: ids >= 100 are "outside"
T_MAX = 16                    # kernels.APPEND_T_MAX


# ------------------------------------------------------------------------------------------------ kernels
def _run_draft(rows, done, k, max_ngram, V, ld_hist):
    """rows: lists of ints (the live histories).  Returns the kernel's (draft, chunk, n_draft) as lists."""
    from llavamod import kernels as K
    R = len(rows)
    hist = torch.full((R, ld_hist), 3, dtype=torch.int32)             # dead positions hold a symbol of the alphabet, not a sentinel
    for r, h in enumerate(rows):
        hist[r, :len(h)] = torch.tensor(h, dtype=torch.int32)
    n_hist = torch.tensor([len(h) for h in rows], dtype=torch.int32)
    d, c, n = K.ngram_draft(hist.to(DEV), n_hist.to(DEV), torch.tensor(done, dtype=torch.int32).to(DEV), k, max_ngram, V)
    return d.cpu().tolist(), c.cpu().tolist(), n.cpu().tolist()


def _check_draft(rows, done, k, max_ngram, V, ld_hist):
    got = _run_draft(rows, done, k, max_ngram, V, ld_hist)
    exp = [LR.draft_arrays(h, d, k, max_ngram, V) for h, d in zip(rows, done)]
    for r, e in enumerate(exp):
        assert (got[0][r], got[1][r], got[2][r]) == e, (r, rows[r][-12:], k, max_ngram, (got[0][r], got[1][r], got[2][r]), e)
    return exp


# every clause of the rule, one row each (name, history, done)
CLAUSE_ROWS = [
    ("no match", [1, 2, 3, 4, 5, 6, 7], 0),
    ("match only at n = 1", [9, 4, 5, 6, 8, 4], 0),
    ("two matches, the earliest wins", [1, 2, 30, 31, 1, 2, 40, 41, 1, 2], 0),
    ("longer n-gram later beats shorter earlier", [8, 1, 2, 7, 8, 4, 5, 6, 7, 8], 0),
    ("continuation shorter than k", [1, 2, 9, 1, 2], 0),
    ("a a a a: overlapping window", [6, 6, 6, 6], 0),
    ("-200 is the first continuation id", [2, 7, 1, 2, IMG, 5, 1, 2], 0),
    ("-200 is a later continuation id", [1, 2, 10, IMG, 11, 1, 2], 0),
    ("-200 inside the matched window", [IMG, 3, 10, 11, 12, 13, IMG, 3], 0),
    ("an id >= V in the continuation", [1, 2, 10, 11, VK + 7, 12, 1, 2], 0),
    ("a done row", [1, 2, 30, 31, 1, 2], 1),
    ("n_hist 1", [5], 0),
    ("n_hist 2, no match", [5, 6], 0),
    ("n_hist 2, match", [5, 5], 0),
    ("a full row", [(i * 7) % 11 for i in range(96)], 0),
    ("three-gram needed", [1, 2, 3, 50, 9, 2, 3, 60, 1, 2, 3], 0),
    ("eight-gram", [1, 2, 3, 4, 5, 6, 7, 8, 70, 71, 0, 2, 3, 4, 5, 6, 7, 8, 80, 1, 2, 3, 4, 5, 6, 7, 8], 0),
    ("id >= V first", [1, 2, VK, 11, 1, 2], 0),
]


@pytest.mark.parametrize("max_ngram", [1, 2, 3, 8])
def test_ngram_draft_clauses(max_ngram):
    """R = 6, ld_hist = 96, k = 4: the rows above in groups of six, exact equality of draft, chunk and n_draft; twice, same output."""
    assert len(CLAUSE_ROWS) % 6 == 0
    seen = []
    for g0 in range(0, len(CLAUSE_ROWS), 6):
        grp = CLAUSE_ROWS[g0:g0 + 6]
        rows, done = [r[1] for r in grp], [r[2] for r in grp]
        exp = _check_draft(rows, done, 4, max_ngram, VK, 96)
        assert _run_draft(rows, done, 4, max_ngram, VK, 96) == _run_draft(rows, done, 4, max_ngram, VK, 96)
        seen += [e[2] for e in exp]
    # the fixture stays in its domain: empty, partial and full drafts all occur
    assert 0 in seen and 4 in seen and any(0 < n < 4 for n in seen), seen


def test_ngram_draft_long_history():
    """n_hist = 1100 (more window starts than threads): row 0's only match starts at 1050; row 1's earliest match is at 0 with a later
    one at 1030 - the minimum must be taken over every stride.  The filler 40 + i % 50 never repeats within 50 positions and the
    planted ids are outside it, so the trailing 2-gram (7, 8) is the longest n-gram that occurs earlier, whatever max_ngram allows
    (a window at 0 has nothing in front of it, and position 1029 / 1049 differs from 1097)."""
    L = 1100
    a = [40 + i % 50 for i in range(L)]
    a[1050:1056] = [7, 8, 9, 10, 11, 12]
    a[-2:] = [7, 8]
    b = [40 + i % 50 for i in range(L)]
    b[0:6] = [7, 8, 20, 21, 22, 23]
    b[1030:1036] = [7, 8, 30, 31, 32, 33]
    b[-2:] = [7, 8]
    for max_ngram in (1, 2, 8):
        assert LR.ngram_draft(a, 4, max_ngram, VK) == [9, 10, 11, 12] and LR.ngram_draft(b, 4, max_ngram, VK) == [20, 21, 22, 23]
        _check_draft([a, b], [0, 0], 4, max_ngram, VK, 1104)
    # a longer n-gram that exists only at the later place wins over the earlier 2-gram: still a minimum over all strides, per n
    b[1028:1030], b[-4:-2] = [3, 4], [3, 4]
    assert LR.ngram_draft(b, 4, 8, VK) == [30, 31, 32, 33] and LR.ngram_draft(b, 4, 2, VK) == [20, 21, 22, 23]
    for max_ngram in (2, 4, 8):
        _check_draft([a, b], [0, 0], 4, max_ngram, VK, 1104)


@pytest.mark.parametrize("k,max_ngram", [(4, 1), (4, 2), (4, 3), (4, 8), (1, 2), (T_MAX - 1, 3)])
def test_ngram_draft_random_rows(k, max_ngram):
    rng = random.Random(100 * k + max_ngram)
    rows = [[rng.randint(0, 3) for _ in range(rng.randint(1, 96))] for _ in range(200)]
    rows[0], rows[1] = rows[0][:1], (rows[1] * 96)[:96]
    done = [int(rng.random() < 0.1) for _ in rows]
    _check_draft(rows, done, k, max_ngram, VK, 96)


def test_ngram_draft_argument_errors():
    from llavamod import _hip
    hist = torch.zeros((2, 8), dtype=torch.int32, device=DEV)
    n_hist = torch.full((2,), 4, dtype=torch.int32, device=DEV)
    done = torch.zeros(2, dtype=torch.int32, device=DEV)
    out = [torch.zeros((2, 32), dtype=torch.int32, device=DEV) for _ in range(3)]

    def rc(R, k, n):
        return _hip.call("lmod_ngram_draft", hist.data_ptr(), 8, n_hist.data_ptr(), done.data_ptr(), R, k, n, VK, out[0].data_ptr(),
                         out[1].data_ptr(), out[2].data_ptr(), allow=(-1,))
    assert rc(2, 0, 2) == -1 and rc(2, T_MAX, 2) == -1 and rc(2, 4, 9) == -1 and rc(2, 4, 0) == -1          # LMOD_EINVAL
    assert rc(0, 4, 2) == 0 and rc(2, 4, 2) == 0 and rc(2, T_MAX - 1, 8) == 0 and rc(2, 1, 1) == 0
    torch.cuda.synchronize()


def test_hist_push_block():
    from llavamod import kernels as K
    k, ld = 3, 10
    # block: k+1 tokens | n_acc | n_emitted | next | done
    block = torch.tensor([[11, 12, 0, 0, 1, 2, 12, 0],           # a live row: two tokens
                          [0, 0, 0, 0, 0, 0, 0, 1],              # a done row: n_emitted 0
                          [21, 22, 23, 24, 3, 4, 24, 0],         # a full row: 4 tokens would pass ld_hist
                          [31, 32, 33, 34, 3, 4, 34, 0]],        # exactly fits
                         dtype=torch.int32)
    hist = torch.arange(4 * ld, dtype=torch.int32).view(4, ld) + 100
    n_hist = torch.tensor([4, 5, 7, 6], dtype=torch.int32)
    exp_h, exp_n = hist.clone(), n_hist.clone()
    for r in range(4):                                           # the restatement
        ne = int(block[r, k + 2])
        if ne and int(n_hist[r]) + ne <= ld:
            exp_h[r, int(n_hist[r]):int(n_hist[r]) + ne], exp_n[r] = block[r, :ne], n_hist[r] + ne
    h, n = hist.to(DEV), n_hist.to(DEV)
    K.hist_push_block_(block.to(DEV), k, h, n)
    assert torch.equal(h.cpu(), exp_h) and torch.equal(n.cpu(), exp_n)
    assert exp_n.tolist() == [6, 5, 7, 10]
    for r in range(4):
        assert LR.push_block(block[r].tolist(), k, hist[r].tolist(), int(n_hist[r]), ld) == (exp_h[r].tolist(), int(exp_n[r]))


# ------------------------------------------------------------------------------------------------ the loop: a copy model
# pi: cycles of 3, 4, 5, 6 and 7 consecutive ids over [0, 448), then ONE cycle of 64 ids [448, 512): a row that walks it has no
# match for 64 tokens (the row "without any match" needs one; every other case uses the short cycles).
def _pi():
    pi, t = list(range(512)), 0
    while t < 448:
        for c in (3, 4, 5, 6, 7):
            c = min(c, 448 - t)
            if c <= 0:
                break
            for j in range(c):
                pi[t + j] = t + (j + 1) % c
            t += c
    for j in range(64):
        pi[448 + j] = 448 + (j + 1) % 64
    assert sorted(pi) == list(range(512)) and all(pi[t] != t for t in range(512))
    return pi


PI = _pi()
HEAD_SCALE = 1.0              # lm_head row pi(t) = HEAD_SCALE * embedding row t; 1.0 gives the 8-ulp gap (asserted in every case)


def walk(t, n):
    """n tokens starting at t along pi."""
    out = []
    for _ in range(n):
        out.append(t)
        t = PI[t]
    return out


def copy_state(tsd):
    """The golden teacher's weights with every decoder o_proj and down_proj scaled by 0.1 (the residual stream stays close to the
    token's embedding while the caches still carry real attention) and lm_head row pi(t) = embedding row t: greedy follows pi."""
    sd = {k: v.clone() for k, v in tsd.items()}
    for k in sd:
        if k.startswith("lm.model.layers.") and (k.endswith("self_attn.o_proj.weight") or k.endswith("mlp.down_proj.weight")):
            sd[k] = sd[k] * 0.1
    head = torch.empty_like(sd["lm.lm_head.weight"])
    head[torch.tensor(PI)] = sd["lm.model.embed_tokens.weight"] * HEAD_SCALE
    sd["lm.lm_head.weight"] = head
    return sd


_MODELS = {}


def _copy_model():
    if "copy" not in _MODELS:
        from test_step_parity_gpu import small_cfgs
        vc, sc, tc = small_cfgs()
        tsd = U.load_golden("gpusmall_teacher.safetensors")
        _, m = U.build_hip_pair(U.load_golden("gpusmall_student.safetensors"), copy_state(tsd), sc, tc, vc, DEV)
        _MODELS["copy"] = m.eval()
    return _MODELS["copy"]


def _teacher():
    if "teacher" not in _MODELS:
        from test_generate_gpu import _pair
        _MODELS["teacher"] = _pair()[1].eval()
    return _MODELS["teacher"]


def _greedy_with_gaps(model, pr, n):
    from test_assisted_gpu import _greedy_with_gaps as g
    return g(model, dict(input_ids=pr["input_ids"], attention_mask=pr.get("attention_mask"), images=pr.get("images")), n)


def _pad_rows(rows, pad=0):
    S = max(len(r) for r in rows)
    ids = torch.tensor([r + [pad] * (S - len(r)) for r in rows], dtype=torch.long)
    am = torch.tensor([[1] * len(r) + [0] * (S - len(r)) for r in rows], dtype=torch.bool)
    return ids, am


def _run_case(model, rows, new, k, n_max=2, eos=None, pad=None, images=None, follows_pi=True):
    """Plain greedy (tie-free for all `new` steps: asserted), the lookup loop, and the replay: tokens and counts must agree."""
    from llavamod.generation import AssistedOutput
    ids, am = _pad_rows(rows)
    pr = dict(input_ids=ids, attention_mask=am if len({len(r) for r in rows}) > 1 else None)
    if images is not None:
        pr["images"] = images
    toks, safe = _greedy_with_gaps(model, pr, new)
    assert int(safe.min()) == new, ("the copy model's top-2 gap fell below 8 bf16 ulps", safe)
    if follows_pi:
        for b, r in enumerate(rows):
            assert toks[b].tolist() == walk(PI[r[-1]], new), (b, toks[b])
    kw = dict(max_new_tokens=new, eos_token_id=eos, pad_token_id=pad)
    ref = model.generate(**pr, **kw)
    if eos is None:
        assert torch.equal(ref, toks)
    out = model.generate(**pr, **kw, prompt_lookup_num_tokens=k, max_matching_ngram_size=n_max, return_dict_in_generate=True)
    assert isinstance(out, AssistedOutput) and out.num_target_forwards == out.num_rounds + 1
    assert torch.equal(out.sequences, ref), (out.sequences, ref)
    seqs, rounds, acc = LR.simulate(rows, toks.tolist(), k, n_max, model.lm_head.weight.shape[0], eos)
    assert out.num_rounds == rounds and out.num_accepted.tolist() == acc, (out.num_rounds, rounds, out.num_accepted, acc)
    for b, s in enumerate(seqs):
        assert out.sequences[b, :len(s)].tolist() == s
    return out, (seqs, rounds, acc), pr


def test_loop_cycle_prompt_accepts_every_draft():
    """The prompt walks a 5-cycle more than twice: every round's draft is the cycle's continuation and all k are accepted."""
    model = _copy_model()
    k, new = 4, 11
    out, (seqs, rounds, acc), _ = _run_case(model, [walk(7, 12)], new, k)
    assert rounds == 2 and acc == [8]                                # 1 + 2 * (k + 1) tokens
    # the default max_matching_ngram_size (2) and a plain tensor return
    seq = model.generate(input_ids=torch.tensor([walk(7, 12)]), max_new_tokens=new, prompt_lookup_num_tokens=k)
    assert torch.equal(seq, out.sequences)


def test_loop_planted_wrong_continuations():
    """Cycle (a b c d e) = 7..11.  The prompt plants (a, b, X) with X != pi(b) BEFORE the true continuation and (a, b, c, Y): the rounds
    accept part of a draft, none of it, and all of it."""
    model = _copy_model()
    a, b, c, d, e = walk(7, 5)
    X, Y, q1, q2, q3 = 100, 101, 102, 103, 104
    rows = [[a, b, X, q1, q2, a, b, c, Y, q3, d, e]]
    k, new = 4, 12
    # per-round accepted counts of the replay, recomputed here from its own pieces: the fixture cannot silently leave the domain
    toks = walk(a, new)
    hist, n, per_round = rows[0] + [toks[0]], 1, []
    while n < new:
        dr = LR.ngram_draft(hist, k, 2, 512)
        m = 0
        while m < min(len(dr), new - n) and dr[m] == toks[n + m]:
            m += 1
        per_round.append(m)
        hist += toks[n:n + min(m + 1, new - n)]
        n += min(m + 1, new - n)
    assert 0 in per_round and k in per_round and any(0 < m < k for m in per_round), per_round
    out, (seqs, rounds, acc), _ = _run_case(model, rows, new, k)
    assert rounds == len(per_round) and acc == [sum(per_round)]


def _cache_lens_probe(model, smax_seen):
    orig = model.model.forward_append

    def probed(emb, cache, n_new, T=None, max_len=None):
        out = orig(emb, cache, n_new, T=T, max_len=max_len)
        smax_seen.append((int(cache.lens.max()), cache.smax))
        assert smax_seen[-1][0] <= smax_seen[-1][1], smax_seen[-1]
        return out
    model.model.forward_append = probed
    return orig


def test_loop_ragged_batch_uneven_acceptance_and_cache():
    """B 2, ragged: row 0 accepts every draft, row 1 walks the 64-cycle and never finds a match, so it keeps the loop going long after
    row 0 has reached max_new_tokens.  lens <= smax after every verification pass, and the returned cache is plain greedy's: same
    lens; over [0, lens) V of layer 0 equal and K of every layer within 1 bf16 ulp (the rule of tests/test_append_gpu.py)."""
    import _append_ref as R
    model = _copy_model()
    k, new = 4, 24
    rows = [walk(7, 12), [200, 300, 450]]
    seen = []
    orig = _cache_lens_probe(model, seen)
    try:
        out, (seqs, rounds, acc), pr = _run_case(model, rows, new, k)
    finally:
        model.model.forward_append = orig
    assert acc[1] == 0 and acc[0] >= 4 * k and rounds == new - 1 and len(seen) == rounds
    assert len({s[1] for s in seen}) == 1                            # the reservation was enough: the cache never grew
    g = model.generate(**pr, max_new_tokens=new, return_dict_in_generate=True)
    cl, cg = out.past_key_values, g.past_key_values
    assert torch.equal(cl.lens, cg.lens) and int(cl.lens.max()) <= cl.smax
    for layer in range(len(cg.k)):
        for b in range(2):
            L = int(cg.lens[b])
            kl, kg = cl.k[layer][b, :L].float(), cg.k[layer][b, :L].float()
            assert bool(((kl - kg).abs() <= R.ulp_bf16(kg.cpu()).to(DEV).float()).all()), (layer, b)
            if layer == 0:
                assert torch.equal(cl.v[0][b, :L], cg.v[0][b, :L]), b


def test_loop_eos_inside_an_accepted_run():
    """eos is the second draft token of row 0's first round: the row emits up to it and pads; row 1 goes on."""
    model = _copy_model()
    k, new = 4, 10
    rows = [walk(7, 12), [200, 300, 450]]
    eos = walk(PI[rows[0][-1]], 3)[2]                                 # greedy's third token of row 0
    out, (seqs, rounds, acc), _ = _run_case(model, rows, new, k, eos=eos, pad=1)
    assert seqs[0] == walk(PI[rows[0][-1]], 3) and acc[0] == 2
    assert out.sequences[0, :3].tolist() == seqs[0] and bool((out.sequences[0, 3:] == 1).all())


def test_loop_image_prompt():
    """The copy model keeps the golden teacher's image tower and projector: an image placeholder in front of the cycle."""
    model = _copy_model()
    img = U.load_golden("append_prompt.safetensors")["images"][:1].to(DEV).to(torch.bfloat16)
    out, (seqs, rounds, acc), _ = _run_case(model, [[3, IMG] + walk(7, 12)], 11, 4, images=img)
    assert acc == [8]


def test_loop_two_turns_with_past_key_values():
    """Turn 1 is plain greedy; turn 2 feeds turn 1's last token and a cyclic text against turn 1's cache, once with plain greedy and
    once with the lookup loop (two identical turn-1 caches): equal on the tie-free steps, and the drafts come from turn 2 alone."""
    model = _copy_model()
    ids1 = torch.tensor([[200, 300, 120, 121], [201, 301, 130, 131]])
    N1, new, k = 3, 11, 4
    firsts = [model.generate(input_ids=ids1, max_new_tokens=N1, return_dict_in_generate=True) for _ in range(2)]
    assert torch.equal(firsts[0].sequences, firsts[1].sequences)
    t1 = firsts[0].sequences.cpu()
    turn2 = torch.tensor([walk(7, 12), walk(14, 12)])
    new_ids = torch.cat([t1[:, -1:], turn2], 1)
    ref = model.generate(input_ids=new_ids, past_key_values=firsts[0].past_key_values, max_new_tokens=new)
    out = model.generate(input_ids=new_ids, past_key_values=firsts[1].past_key_values, max_new_tokens=new, prompt_lookup_num_tokens=k,
                         return_dict_in_generate=True)
    whole = torch.cat([ids1, t1, turn2], 1)
    toks, safe = _greedy_with_gaps(model, dict(input_ids=whole), new)
    for b in range(2):
        n = int(safe[b])
        assert n >= 6, (b, n)
        assert torch.equal(out.sequences[b, :n].cpu(), ref[b, :n].cpu()), (b, out.sequences[b], ref[b])
    assert int(safe.min()) == new, safe
    seqs, rounds, acc = LR.simulate(new_ids.tolist(), toks.tolist(), k, 2, 512)
    assert out.num_rounds == rounds and out.num_accepted.tolist() == acc and min(acc) > 0
    assert torch.equal(out.past_key_values.lens, firsts[0].past_key_values.lens)


def test_loop_golden_teacher_equals_greedy():
    """The unmodified golden teacher on the tie-free image prompts: whatever is drafted and accepted, the tokens are plain greedy's."""
    teacher = _teacher()
    g = U.load_golden("append_prompt.safetensors")
    pr = dict(input_ids=g["input_ids"], attention_mask=g["attention_mask"].bool(), images=g["images"].to(DEV).to(torch.bfloat16))
    new = 8
    ref = teacher.generate(**pr, max_new_tokens=new)
    _, safe = _greedy_with_gaps(teacher, pr, new)
    for k, n_max in ((4, 2), (1, 1), (T_MAX - 1, 8)):
        out = teacher.generate(**pr, max_new_tokens=new, prompt_lookup_num_tokens=k, max_matching_ngram_size=n_max,
                               return_dict_in_generate=True)
        assert out.num_rounds >= 1 and out.sequences.shape == ref.shape
        for b in range(ref.shape[0]):
            n = int(safe[b])
            assert n >= 6, (b, n)
            assert torch.equal(out.sequences[b, :n], ref[b, :n]), (k, b, out.sequences[b], ref[b])


def test_loop_argument_errors():
    model = _copy_model()
    ids = torch.tensor([walk(7, 12)])
    kw = dict(input_ids=ids, max_new_tokens=4)
    for bad in (dict(prompt_lookup_num_tokens=0), dict(prompt_lookup_num_tokens=T_MAX), dict(prompt_lookup_num_tokens=4, max_matching_ngram_size=9),
                dict(prompt_lookup_num_tokens=4, max_matching_ngram_size=0), dict(prompt_lookup_num_tokens=4, do_sample=True),
                dict(prompt_lookup_num_tokens=4, num_beams=2), dict(prompt_lookup_num_tokens=4, num_return_sequences=2),
                dict(prompt_lookup_num_tokens=4, assistant_model=model), dict(prompt_lookup_num_tokens=4, speculative_sampling=True),
                dict(prompt_lookup_num_tokens=4, repetition_penalty=1.3), dict(prompt_lookup_num_tokens=4, no_repeat_ngram_size=2),
                dict(prompt_lookup_num_tokens=4, bad_words_ids=[[5]]), dict(prompt_lookup_num_tokens=4, suppress_tokens=[5]),
                dict(prompt_lookup_num_tokens=4, min_new_tokens=2, eos_token_id=3), dict(prompt_lookup_num_tokens=4, stop_sequences=[[5, 6]])):
        with pytest.raises(ValueError):
            model.generate(**kw, **bad)
    with pytest.raises(ValueError, match="prompt_lookup_num_tokens"):
        model.generate_batch([dict(input_ids=ids[0])], max_new_tokens=4, prompt_lookup_num_tokens=4)
