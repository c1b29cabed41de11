"""Continuous batching on the device: the three kernels of csrc/batch.hip against tests/_batch_ref.py, bit for bit, and generate_batch on
the golden small teacher against generate() of every prompt alone (greedy, planted EOS / stop sequence with logits processors, sampling
with the per-request uniform stream)."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _append_ref as R  # noqa: E402
import _batch_ref as BR  # noqa: E402

DEV = "cuda"
BF = torch.bfloat16
NEW = 8
ORDER = [0, 1, 1, 0, 0]                 # the fixture's two prompts, issued as five requests
BUDGETS = [2, 8, 4, 8, 6]


# ---------------------------------------------------------------------------------------------- kernels
def _bits(t):
    return t.view(torch.int16) if t.dtype == BF else t


@pytest.mark.parametrize("R_", [0, 1, 3, 5])
@pytest.mark.parametrize("width", [8, 64, 1032])
@pytest.mark.parametrize("ntensor", [2, 6])
def test_kv_admit_rows_bit_for_bit(ntensor, width, R_, B=5, smax_src=7, smax_dst=19):
    from llavamod import kernels as K
    g = torch.Generator().manual_seed(100 * ntensor + width + R_)
    src = [torch.randn(R_, smax_src, width, generator=g).to(BF).to(DEV) for _ in range(ntensor)]
    dst = [torch.randn(B, smax_dst, width, generator=g).to(BF).to(DEV) for _ in range(ntensor)]          # the sentinel pattern
    lens = [smax_src, 0, 1, 4, 2][:R_]
    rows = [4, 0, 2, 1, 3][:R_]                                                                            # non-monotone
    want = BR.kv_admit_rows(dst, src, rows, lens)
    got = [d.clone() for d in dst]
    K.kv_admit_rows(got, src, rows, torch.tensor(lens, dtype=torch.int32, device=DEV), max(lens, default=0))
    torch.cuda.synchronize()
    for t in range(ntensor):
        assert torch.equal(_bits(got[t]), _bits(want[t])), (t, (_bits(got[t]) != _bits(want[t])).nonzero()[:4])
        for b in set(range(B)) - set(rows):                                     # a slot nobody named keeps every byte
            assert torch.equal(_bits(got[t][b]), _bits(dst[t][b]))
    if R_ == 3:                                                                 # a loose bound is fine as long as both caches hold it
        again = [d.clone() for d in dst]
        K.kv_admit_rows(again, src, rows, torch.tensor(lens, dtype=torch.int32, device=DEV), smax_src)
        assert all(torch.equal(_bits(a), _bits(w)) for a, w in zip(again, want))


def test_kv_admit_rows_rejects_what_it_cannot_hold():
    from llavamod import kernels as K
    g = torch.Generator().manual_seed(3)
    dst = [torch.randn(5, 19, 64, generator=g).to(BF).to(DEV) for _ in range(2)]
    keep = [d.clone() for d in dst]
    lens = torch.tensor([3, 2], dtype=torch.int32, device=DEV)
    long_src = [torch.randn(2, 25, 64, generator=g).to(BF).to(DEV) for _ in range(2)]
    with pytest.raises(RuntimeError, match="LMOD_EINVAL"):                      # max_len 20 > smax_dst 19: nothing runs
        K.kv_admit_rows(dst, long_src, [4, 0], lens, 20)
    short_src = [torch.randn(2, 7, 64, generator=g).to(BF).to(DEV) for _ in range(2)]
    with pytest.raises(RuntimeError, match="LMOD_EINVAL"):                      # max_len 8 > smax_src 7
        K.kv_admit_rows(dst, short_src, [4, 0], lens, 8)
    for rows in ([4, 4], [5, 0], [-1, 0]):                                      # the host's part of the contract
        with pytest.raises(ValueError, match="distinct"):
            K.kv_admit_rows(dst, short_src, rows, lens, 3)
    torch.cuda.synchronize()
    assert all(torch.equal(_bits(d), _bits(k)) for d, k in zip(dst, keep))


@pytest.mark.parametrize("L,S", [(23, 11), (24, 12)])                          # int-by-int rows, and rows of whole 16-byte vectors
@pytest.mark.parametrize("R_", [0, 1, 3])
def test_slot_admit_matches_restatement(R_, L, S, B=5):
    from llavamod import kernels as K
    g = torch.Generator().manual_seed(10 * L + R_)
    ri = lambda *shape: torch.randint(-300, 1000, shape, generator=g).to(torch.int32).to(DEV)              # sentinels everywhere
    state = [ri(B, L), ri(B), ri(B), ri(B), ri(B), ri(B), ri(B)]                # hist, n_prompt, n_hist, n_gen, done, cache_lens, req_id
    rows = [4, 0, 2][:R_]
    prompt = ri(R_, S)
    n_new = torch.tensor([S, 0, 5][:R_], dtype=torch.int32, device=DEV)
    lens_new = torch.tensor([17, 3, 9][:R_], dtype=torch.int32, device=DEV)
    req_new = torch.tensor([7, 2 ** 31 - 1, 0][:R_], dtype=torch.int32, device=DEV)
    want = BR.slot_admit(rows, prompt, n_new, lens_new, req_new, *state)
    got = [t.clone() for t in state]
    K.slot_admit_(rows, prompt, n_new, lens_new, req_new, *got)
    torch.cuda.synchronize()
    for name, a, b in zip(("hist", "n_prompt", "n_hist", "n_gen", "done", "cache_lens", "req_id"), got, want):
        assert torch.equal(a, b), (name, a, b)
    for t, (a, b) in enumerate(zip(got, state)):                                # untouched slots, req_id included
        for s in set(range(B)) - set(rows):
            assert torch.equal(a[s], b[s]), (t, s)
    if R_ == 3:
        assert got[1][0].item() == 0 and torch.equal(got[0][0], state[0][0])    # an empty prompt writes no history


def test_request_uniform_equals_philox_reference():
    from llavamod import kernels as K
    rng = np.random.default_rng(11)
    req = rng.integers(0, 2 ** 31 - 1, 4096).astype(np.int32)
    req[:64] = np.arange(64)                                                    # the ids a request list really has
    gen = rng.integers(0, 4096, 4096).astype(np.int32)
    gen[:128] = np.arange(128) % 2
    for seed in (5, 0x9E3779B97F4A7C15):                                        # the second one uses the key's high word
        u = K.request_uniform(seed, torch.from_numpy(req).to(DEV), torch.from_numpy(gen).to(DEV)).cpu().numpy()
        want = BR.request_uniform(seed, req, gen)
        assert u.dtype == np.float32 and np.array_equal(u.view(np.uint32), want.view(np.uint32)), (seed, np.nonzero(u != want)[0][:5])
        assert u.min() >= 0.0 and u.max() < 1.0
        perm = rng.permutation(4096)                                            # the slot a request sits in does not matter
        up = K.request_uniform(seed, torch.from_numpy(req[perm]).to(DEV), torch.from_numpy(gen[perm]).to(DEV)).cpu().numpy()
        assert np.array_equal(up.view(np.uint32), u[perm].view(np.uint32))
    assert K.request_uniform(5, torch.zeros(0, dtype=torch.int32, device=DEV), torch.zeros(0, dtype=torch.int32, device=DEV)).numel() == 0


# ---------------------------------------------------------------------------------------------- generate_batch
@functools.lru_cache(maxsize=None)
def _teacher():
    from test_assisted_gpu import _pair
    return _pair()[1]


@functools.lru_cache(maxsize=None)
def _prompts():
    """The two prompts of tests/golden/append_prompt.safetensors as single requests (their own length, their own image)."""
    from test_assisted_gpu import _prompt
    pr = _prompt()
    n = pr["attention_mask"].sum(1)
    return tuple(dict(input_ids=pr["input_ids"][p, :int(n[p])], images=pr["images"][p:p + 1]) for p in range(2))


def _requests(budgets):
    return [dict(_prompts()[p], max_new_tokens=m) for p, m in zip(ORDER, budgets)]


def _alone(p):
    pr = _prompts()[p]
    ids = pr["input_ids"][None]
    return dict(input_ids=ids, attention_mask=torch.ones_like(ids, dtype=torch.bool), images=pr["images"])


@functools.lru_cache(maxsize=None)
def _greedy_refs():
    """Per prompt: generate() of the prompt alone ([NEW] tokens) and the number of leading steps whose top-2 gap is >= 8 bf16 ulps."""
    from test_assisted_gpu import _greedy_with_gaps
    teacher, out = _teacher(), []
    for p in range(2):
        toks, safe = _greedy_with_gaps(teacher, _alone(p), NEW)
        ref = teacher.generate(**_alone(p), max_new_tokens=NEW)
        assert torch.equal(ref, toks)
        out.append((ref[0].cpu(), int(safe[0])))
    return out


def _scheduled_steps(budgets, B, lengths=None):
    """num_decode_steps of the CPU scheduler when request r emits lengths[r] tokens (its whole budget by default)."""
    from llavamod.generation import SlotScheduler
    sched, emitted = SlotScheduler(budgets, B), [0] * len(budgets)
    while not sched.finished:
        sched.admit()
        live = sched.live
        for r in live.values():
            emitted[r] += 1
        sched.step([s for s, r in live.items() if lengths is not None and emitted[r] == lengths[r] < budgets[r]])
    return sched.num_decode_steps


def test_generate_batch_greedy_equals_generate_alone():
    from llavamod.generation import BatchOutput
    teacher, refs = _teacher(), _greedy_refs()
    out = teacher.generate_batch(_requests(BUDGETS), max_batch_size=2, return_dict_in_generate=True)
    assert isinstance(out, BatchOutput) and out.token_logprobs is None and len(out.sequences) == 5
    # precondition, stated: the fixture keeps the GPU's decode path tie-free for all NEW steps of either prompt
    assert min(s for _, s in refs) == NEW, refs
    for i, (p, m) in enumerate(zip(ORDER, BUDGETS)):
        seq, (ref, safe) = out.sequences[i], refs[p]
        assert seq.dtype == torch.int64 and seq.shape == (m,), (i, seq)
        n = min(m, safe)
        assert safe >= 6 and torch.equal(seq[:n].cpu(), ref[:n]), (i, seq, ref)
    # the counters prove that slots were refilled: 5 admissions into 2 slots, in the steps the CPU scheduler predicts
    assert out.num_admissions == 5 and out.num_prefills == 4
    assert out.num_decode_steps == _scheduled_steps(BUDGETS, 2) == 14
    assert out.live_row_steps == sum(BUDGETS) and out.total_row_steps == 2 * 14
    plain = teacher.generate_batch(_requests(BUDGETS), max_batch_size=2)
    assert isinstance(plain, list) and all(torch.equal(a, b) for a, b in zip(plain, out.sequences))
    assert teacher.generate_batch([], max_batch_size=2) == []


def _processed_alone(teacher, p, **kw):
    """generate() of prompt p alone with logits processors; also the number of leading steps whose top-2 gap of the PROCESSED logits
    (what lmod_row_argmax_bf16 is given) is >= 8 bf16 ulps — the rule of _greedy_with_gaps on the path that has processors."""
    from llavamod import kernels as K
    orig, oks = K.row_argmax, []

    def spy(lg):
        t2 = lg.float().topk(2, -1).values
        oks.append(bool(((t2[:, 0] - t2[:, 1]) >= 8 * R.ulp_bf16(t2[:, 0].cpu()).to(DEV).float()).all()))
        return orig(lg)

    K.row_argmax = spy
    try:
        seq = teacher.generate(**_alone(p), max_new_tokens=NEW, **kw)[0].cpu()
    finally:
        K.row_argmax = orig
    return seq, (oks + [False]).index(False)


def test_planted_eos_and_stop_sequence_free_their_slots():
    """repetition_penalty and no_repeat_ngram_size read the slot's history: a request admitted into a used slot would emit other tokens
    if the previous occupant's hist / n_hist survived.  EOS: the token prompt 0 emits at step 3; stop: prompt 1's tokens of steps 2-3."""
    teacher = _teacher()
    proc = dict(repetition_penalty=1.3, no_repeat_ngram_size=2)
    base = [_processed_alone(teacher, p, **proc)[0] for p in range(2)]
    eos, stop = int(base[0][3]), [int(t) for t in base[1][2:4]]
    kw = dict(proc, eos_token_id=eos, pad_token_id=1, stop_sequences=[stop])
    refs = []
    for p in range(2):
        seq, safe = _processed_alone(teacher, p, **kw)                          # [<= NEW], pad behind the cut
        cut = len(seq)
        hits = [i for i in range(len(seq)) if int(seq[i]) == eos or (i >= 1 and [int(seq[i - 1]), int(seq[i])] == stop)]
        if hits:
            cut = hits[0] + 1
            assert bool((seq[cut:] == 1).all())
        refs.append((seq[:cut], safe))
    assert len(refs[0][0]) <= 4 and len(refs[1][0]) <= 4, refs                   # both plants cut their row
    out = teacher.generate_batch(_requests([NEW] * 5), max_batch_size=2, return_dict_in_generate=True, **kw)
    lengths = [len(s) for s in out.sequences]
    for i, p in enumerate(ORDER):
        ref, safe = refs[p]
        n = min(len(ref), safe)
        assert torch.equal(out.sequences[i][:n].cpu(), ref[:n]), (i, out.sequences[i], ref, safe)
        if safe >= len(ref):                                                    # cut exactly where generate() cuts it
            assert lengths[i] == len(ref), (i, out.sequences[i], ref)
    # the freed slots were reused: 5 requests through 2 slots, in the steps the scheduler needs for these lengths
    assert out.num_admissions == 5
    assert out.num_decode_steps == _scheduled_steps([NEW] * 5, 2, lengths) < _scheduled_steps([NEW] * 5, 2)


def test_sampling_uniforms_belong_to_the_request():
    """temperature 1.5, top_p 0.9, seed 5.  Every emitted token equals lmod_sample_bf16 on the very logits the step saw (the decode
    step's output, with the admission prefill's rows scattered in) under u = Philox(seed; request index, token index) from the numpy
    reference: the same kernel on the same logits, so it is exact — and it pins the uniform stream to the request, not to the slot."""
    from llavamod import kernels as K
    from llavamod.generation import SlotScheduler
    teacher = _teacher()
    kw = dict(max_batch_size=2, do_sample=True, temperature=1.5, top_p=0.9, seed=5, return_dict_in_generate=True)
    dec, adm = [], []
    orig_dec, orig_start = teacher._decode_step, teacher._start

    def spy_dec(tokens, cache):
        assert int(cache.lens.max()) < cache.smax, (cache.lens, cache.smax)     # the decode step writes at position lens: it must exist
        lg = orig_dec(tokens, cache)
        dec.append(lg.clone())
        return lg

    def spy_start(*a):
        cache, lg = orig_start(*a)
        adm.append(lg.clone())
        return cache, lg

    teacher._decode_step, teacher._start = spy_dec, spy_start
    try:
        out = teacher.generate_batch(_requests(BUDGETS), **kw)
    finally:
        del teacher._decode_step, teacher._start
    again = teacher.generate_batch(_requests(BUDGETS), **kw)
    assert [len(s) for s in out.sequences] == BUDGETS
    assert all(torch.equal(a, b) for a, b in zip(out.sequences, again.sequences))
    assert all(torch.equal(a, b) for a, b in zip(out.token_logprobs, again.token_logprobs))
    for seq, lp in zip(out.sequences, out.token_logprobs):
        assert lp.dtype == torch.float32 and lp.shape == seq.shape
        assert bool(torch.isfinite(lp).all()) and bool((lp <= 0).all()), lp
    # replay the schedule on the host and redraw every token from the recorded logits
    sched, emitted = SlotScheduler(BUDGETS, 2), [0] * 5
    buf = torch.zeros_like(dec[0])
    dec_it, adm_it, checked = iter(dec), iter(adm), 0
    while not sched.finished:
        admitted = sched.admit()
        if admitted:                                                            # every request has an image: one prefill per admission
            lg = next(adm_it)
            assert lg.shape[0] == len(admitted)
            for j, (_, s) in enumerate(admitted):
                buf[s] = lg[j]
        live = sched.live
        req = [live.get(s, 0) for s in range(2)]
        u_ref = BR.request_uniform(5, req, [emitted[r] for r in req])
        tok = K.sample(buf, torch.from_numpy(u_ref).to(DEV), 1.5, None, 0.9, stats=True)[0].cpu()
        for s, r in live.items():
            assert int(tok[s]) == int(out.sequences[r][emitted[r]]), (r, emitted[r], s, tok, out.sequences[r])
            emitted[r] += 1
            checked += 1
        sched.step()
        if sched.live:
            buf = next(dec_it).clone()
    assert checked == sum(BUDGETS) and next(dec_it, None) is None and next(adm_it, None) is None
