"""Per-request parameters of generate_batch on the device.  The four per-row kernels against their per-call counterparts run on one
row at a time with that row's parameters — bit for bit, since a row of lmod_sample_rows_bf16 / lmod_logits_process_rows_bf16 /
lmod_gen_push_stop_rows must not depend on its neighbours — and against the plain references of tests/_logits_ref.py and
tests/_batch_ref.py; then generate_batch on the golden small teacher with a different `params` per request."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "llava-mod_amd"))

import _batch_ref as BR  # noqa: E402
import _logits_ref as LR  # noqa: E402

DEV = "cuda"
BF = torch.bfloat16
I32 = torch.int32
NINF = float("-inf")


def _bits(t):
    return t.view(torch.int16) if t.dtype == BF else t.view(torch.int32)


# ---------------------------------------------------------------------------------------------- lmod_sample_rows_bf16
# row -> (temperature, top_k, top_p, greedy): no filter, temperature only, top-k, top-p, both, top_k >= V (off), top_p = 0 (the
# maximum's tie group), greedy
def _row_params(V):
    return [(1.0, 0, 1.0, 0), (0.3, 0, 1.0, 0), (1.0, 3, 1.0, 0), (1.0, 0, 0.9, 0), (1.0, 50, 0.7, 0), (1.0, V, 1.0, 0),
            (1.0, 0, 0.0, 0), (0.7, 5, 0.5, 1)]                 # the greedy row's sampling values must not reach its result


def _sample_logits(V, ld):
    """[8, V] bf16 on the device with row stride ld, and what was planted.  V >= 64: a tie group across the top-k boundary (row 2),
    a tie group across the top-p boundary (row 3), +0 and -0 as the only maxima (rows 6 and 7, -0 first); V == 1000: row 5 all -inf.
    V == 2: rows 6 and 7 are (-0, +0)."""
    g = torch.Generator().manual_seed(V)
    x = (3.0 * torch.randn(8, V, generator=g)).to(BF)
    if V >= 64:
        x[2] = x[2].clamp(max=6.0)
        x[2, [5, 40]] = torch.tensor([9.0, 8.0], dtype=BF)
        x[2, [7, 20, 63]] = 7.0                                 # ranks 3..5 tie: top_k = 3 keeps 5 tokens
        x[3] = (-20.0 + torch.randn(V, generator=g)).to(BF)
        x[3, 11] = 10.0
        x[3, [3, 9, 17, 25, 33, 41, 50, 62]] = 9.0              # mass 1 + 8 / e: 0.9 of it falls inside this group
        for r in (6, 7):
            x[r] = -x[r].abs() - 0.5
            x[r, 13], x[r, 45] = -0.0, 0.0
    else:
        x[6] = torch.tensor([-0.0, 0.0], dtype=BF)
        x[7] = torch.tensor([-0.0, 0.0], dtype=BF)
    if V == 1000:
        x[5] = NINF
    buf = torch.zeros(8, ld, dtype=BF)
    buf[:, :V] = x
    return buf.to(DEV)[:, :V]


def _run_rows(K, logits, u, params, chunk):
    dev = lambda vals, dt: torch.tensor(vals, dtype=dt, device=DEV)
    tok, st = K.sample_rows(logits, u, dev([p[0] for p in params], torch.float32), dev([p[1] for p in params], I32),
                            dev([p[2] for p in params], torch.float32), dev([p[3] for p in params], I32), stats=True, chunk=chunk)
    torch.cuda.synchronize()
    return tok.cpu(), st.cpu()


@pytest.mark.parametrize("V,ld,chunk", [(2, 2, None), (1000, 1003, None), (4104, 4104, 512), (151936, 151936, None)])
def test_sample_rows_equal_the_scalar_kernel_row_by_row(V, ld, chunk):
    from llavamod import kernels as K
    logits = _sample_logits(V, ld)
    assert logits.stride(0) == ld
    params = _row_params(V)
    u = torch.rand(8, generator=torch.Generator().manual_seed(V + 1))
    u[0], u[4] = 0.0, float(np.nextafter(np.float32(1), np.float32(0)))
    u = u.to(DEV)
    tok, st = _run_rows(K, logits, u, params, chunk)
    assert not torch.isnan(st).any() and bool(((tok >= 0) & (tok < V)).all())
    for r, (T, k, p, greedy) in enumerate(params):
        if greedy:
            want = K.row_argmax(logits[r:r + 1]).cpu()
            assert int(tok[r]) == int(want[0]), (r, tok[r], want)
            lse = torch.logsumexp(logits[r].double(), 0).item()
            assert abs(st[r, 0].item() - lse) <= 2e-6 * abs(lse) + 1e-6, (st[r], lse)       # test_sample_gpu's bound on the lse
            assert st[r, 1:].tolist() == [1.0, float(V), NINF], st[r]
            continue
        wt, ws = K.sample(logits[r:r + 1], u[r:r + 1], T, k, p, stats=True)
        assert int(tok[r]) == int(wt[0]), (r, params[r], tok[r], wt)
        assert torch.equal(_bits(st[r]), _bits(ws.cpu()[0])), (r, params[r], st[r], ws)
    # the plants are where they were meant to be
    if V >= 64:
        assert st[2, 2].item() == 5 and st[2, 3].item() == 7.0                   # the top-k tie group is kept whole
        assert st[3, 2].item() == 9 and st[3, 3].item() == 9.0                   # the top-p prefix ends inside the group of 9.0
        assert st[6, 2].item() == 2 and st[6, 3].item() == 0.0 and int(tok[6]) in (13, 45)
        assert int(tok[7]) == 13                                                 # -0 at 13 and +0 at 45 are one maximum: the first
    else:
        assert int(tok[7]) == 0 and st[6, 2].item() == 2
    if V == 1000:
        assert int(tok[5]) == 0 and st[5, 0].item() == NINF and st[5, 1].item() == 0.0
    # the same rows in another order: a row depends neither on its neighbours nor on its position
    perm = [3, 7, 0, 5, 2, 6, 1, 4]
    buf = torch.zeros(8, ld, dtype=BF, device=DEV)
    buf[:, :V] = logits[perm]
    tok_p, st_p = _run_rows(K, buf[:, :V], u[perm].contiguous(), [params[i] for i in perm], chunk)
    assert torch.equal(tok_p, tok[perm]) and torch.equal(_bits(st_p), _bits(st[perm])), (tok_p, tok[perm])
    # every row greedy, the all -inf row and the ties included
    tok_g, st_g = _run_rows(K, logits, u, [(T, k, p, 1) for T, k, p, _ in params], chunk)
    assert torch.equal(tok_g, K.row_argmax(logits).cpu()) and not torch.isnan(st_g).any()
    assert bool((st_g[:, 1] == 1).all()) and bool((st_g[:, 2] == V).all()) and bool((st_g[:, 3] == NINF).all())
    lse = torch.logsumexp(logits.double(), 1).cpu()
    fin = torch.isfinite(lse)
    assert bool((st_g[~fin, 0] == NINF).all())
    assert bool(((st_g[fin, 0].double() - lse[fin]).abs() <= 2e-6 * lse[fin].abs() + 1e-6).all()), (st_g[:, 0], lse)


def test_sample_rows_arguments():
    from llavamod import _hip, kernels as K
    z = lambda dt: torch.zeros(0, dtype=dt, device=DEV)
    tok = K.sample_rows(torch.zeros(0, 16, dtype=BF, device=DEV), z(torch.float32), z(torch.float32), z(I32), z(torch.float32), z(I32))
    assert tok.numel() == 0                                                     # R == 0 is a no-op
    x = torch.zeros(2, 16, dtype=BF, device=DEV)
    f, i, u0 = torch.ones(2, device=DEV), torch.zeros(2, dtype=I32, device=DEV), torch.zeros(2, device=DEV)
    out, ws = torch.full((2,), -7, dtype=I32, device=DEV), torch.zeros(2 * (64 + 3072 * 3 + 16 * 2), dtype=torch.uint8, device=DEV)
    args = lambda **kw: [kw.get(k, v) for k, v in dict(
        logits=_hip.ptr(x), ld=16, V=16, u=_hip.ptr(u0), R=2, temperature=_hip.ptr(f), top_k=_hip.ptr(i), top_p=_hip.ptr(f),
        greedy=_hip.ptr(i), chunk=8, ws=_hip.ptr(ws), ws_bytes=ws.numel(), out_token=_hip.ptr(out), out_stats=None).items()]
    for bad in (dict(greedy=None), dict(top_k=None), dict(temperature=None), dict(ws_bytes=ws.numel() - 1), dict(chunk=12), dict(V=1),
                dict(ld=8)):
        with pytest.raises(RuntimeError, match="LMOD_EINVAL"):
            _hip.call("lmod_sample_rows_bf16", *args(**bad))
    torch.cuda.synchronize()
    assert out.tolist() == [-7, -7]                                             # nothing was launched
    _hip.call("lmod_sample_rows_bf16", *args())
    torch.cuda.synchronize()
    assert out.tolist() == [0, 0]


# ---------------------------------------------------------------------------------------------- lmod_logits_process_rows_bf16
EOS = 9
# row -> (penalty, ngram, min_new): all neutral, penalty only, n-gram only, min_new only, everything, a penalty below 1 with n = 1
ROWS_PROC = [(1.0, 0, 0), (1.3, 0, 0), (1.0, 2, 0), (1.0, 0, 2), (1.3, 3, 2), (0.8, 1, 0)]


def _proc_inputs(V, ld):
    g = torch.Generator().manual_seed(V + 6)
    x = (torch.randn(6, ld, generator=g) * 4).to(BF)
    x[:, 3], x[:, 21] = 0.0, -0.0
    x[:, [5, V - 1]] = NINF
    L = 64
    hist = torch.randint(0, V, (6, L), generator=g).to(I32)                     # the dead tail would change the result if it were read
    n_hist = torch.tensor([40, 37, 40, 1, 40, 23], dtype=I32)
    for r in range(6):
        n = int(n_hist[r])
        body = torch.randint(0, 12, (n,), generator=g).to(I32)                  # 12 distinct ids in up to 40 places: many repeats
        if n > 8:
            body[4] = -200                                                      # the image placeholder
            body[n - 2:] = body[10:12]                                          # the ending occurred before: n-gram bans for n = 2, 3
            body[n - 3] = body[9]
        hist[r, :n] = body
    return x, hist, n_hist, torch.tensor([0, 1, 5, 0, 1, 3], dtype=I32)


@pytest.mark.parametrize("V,ld", [(1000, 1008), (151936, 151936)])
def test_logits_process_rows_equal_the_scalar_kernel_and_the_reference(V, ld):
    from llavamod import kernels as K
    x, hist, n_hist, n_gen = _proc_inputs(V, ld)
    table = [[4], [int(hist[0, int(n_hist[0]) - 1]), 11]]                       # per call: applies to every row
    bad = K.seq_table(table, DEV)
    dev = lambda vals, dt: torch.tensor(vals, dtype=dt, device=DEV)
    xd, hd, nh, ng = x.to(DEV), hist.to(DEV), n_hist.to(DEV), n_gen.to(DEV)
    got = K.logits_process_rows_(xd[:, :V], hd, nh, ng, dev([p[0] for p in ROWS_PROC], torch.float32), dev([p[1] for p in ROWS_PROC], I32),
                                 dev([p[2] for p in ROWS_PROC], I32), True, bad, EOS)
    assert got.data_ptr() == xd.data_ptr()
    got = xd.cpu()
    for r, (pen, ngram, min_new) in enumerate(ROWS_PROC):
        one = x[r:r + 1].to(DEV)
        K.logits_process_(one[:, :V], hd[r:r + 1], nh[r:r + 1], ng[r:r + 1], pen, ngram, bad, min_new, EOS)
        assert torch.equal(_bits(got[r]), _bits(one.cpu()[0])), (r, ROWS_PROC[r], (_bits(got[r]) != _bits(one.cpu()[0])).nonzero()[:6])
        want = x[r:r + 1].clone()
        want[:, :V] = LR.process_logits(x[r:r + 1, :V], hist[r:r + 1], n_hist[r:r + 1], n_gen[r:r + 1], pen, ngram, table, min_new, EOS)
        diff = (_bits(got[r]) != _bits(want[0])).nonzero()
        assert diff.numel() == 0, (r, ROWS_PROC[r], diff[:6].tolist())
        assert not torch.equal(_bits(want[0]), _bits(x[r])), (r, "the row's processors change nothing: it would test nothing")
    assert torch.equal(hd.cpu(), hist)
    # rows whose penalty is 1 do the same without the bitmap; with every penalty at 1 the flag may be off
    xd2 = x.to(DEV)
    ones = torch.ones(6, device=DEV)
    K.logits_process_rows_(xd2[:, :V], hd, nh, ng, ones, dev([p[1] for p in ROWS_PROC], I32), dev([p[2] for p in ROWS_PROC], I32), False,
                           bad, EOS)
    for r in (0, 2, 3):
        assert torch.equal(_bits(xd2.cpu()[r]), _bits(got[r])), r


def test_logits_process_rows_arguments():
    from llavamod import kernels as K
    z = lambda dt: torch.zeros(0, dtype=dt, device=DEV)
    K.logits_process_rows_(torch.zeros(0, 16, dtype=BF, device=DEV), torch.zeros(0, 4, dtype=I32, device=DEV), z(I32), z(I32),
                           z(torch.float32), z(I32), z(I32), True)              # R == 0 is a no-op
    V = 524288 + 32                                                             # the bitmap rule of the scalar kernel, by the host's flag
    x = torch.zeros(1, V, dtype=BF, device=DEV)
    hist = torch.tensor([[V - 1, 3, V - 1]], dtype=I32, device=DEV)
    n3, n0 = torch.tensor([3], dtype=I32, device=DEV), torch.zeros(1, dtype=I32, device=DEV)
    with pytest.raises(ValueError, match="524288"):
        K.logits_process_rows_(x, hist, n3, n0, torch.tensor([1.2], device=DEV), n0, n0, True)
    assert not bool(torch.isinf(x).any())
    K.logits_process_rows_(x, hist, n3, n0, torch.ones(1, device=DEV), torch.ones(1, dtype=I32, device=DEV), n0, False)
    assert torch.isinf(x[0].float()).nonzero().flatten().tolist() == [3, V - 1]


# ---------------------------------------------------------------------------------------------- lmod_gen_push_stop_rows
def test_gen_push_stop_rows_equal_the_reference_row_by_row():
    from llavamod import kernels as K
    call_stops = [[5, 6]]
    own = [[[7, 8, 9]], [[3]], [], [[3]], [[4, 4], [2, 4]], [[9, 9]], []]
    stops, first, count = list(call_stops), [], []
    for o in own:
        first.append(len(stops) if o else 0)
        count.append(len(o))
        stops += o
    L = 12
    hist = torch.full((7, L), 77, dtype=I32)
    rows = [([1, 7, 8], 3, 9, 0),      # its own stop would need the prompt's 7 8: no stop
            ([1, 2, 3], 2, 3, 1),      # done before: pad, nothing appended, although its own stop is the token
            ([1, 5], 1, 6, 0),         # an empty own range; the call's stop 5 6 lies behind the one-token prompt: stop
            ([1, 2, 9], 1, 3, 0),      # its own one-token stop
            ([8, 2, 2], 1, 4, 0),      # the second of its own two: 2 4
            ([1, 2, 9], 1, 3, 0),      # the token is row 1's and row 3's stop, not this row's
            ([5], 1, 6, 0)]            # the call's stop needs the prompt's 5: no stop
    for r, (h, _, _, _) in enumerate(rows):
        hist[r, :len(h)] = torch.tensor(h, dtype=I32)
    n_hist = torch.tensor([len(h) for h, _, _, _ in rows], dtype=I32)
    n_prompt = torch.tensor([p for _, p, _, _ in rows], dtype=I32)
    tokens = torch.tensor([t for _, _, t, _ in rows], dtype=I32)
    done = torch.tensor([d for _, _, _, d in rows], dtype=I32)
    n_gen = n_hist - n_prompt
    got = [t.clone().to(DEV) for t in (tokens, done, hist, n_hist, n_gen)]
    K.gen_push_stop_rows_(got[0], got[1], got[2], got[3], n_prompt.to(DEV), got[4], None, 1, K.seq_table(stops, DEV), len(call_stops),
                          torch.tensor(first, dtype=I32, device=DEV), torch.tensor(count, dtype=I32, device=DEV))
    torch.cuda.synchronize()
    for r in range(7):
        sl = slice(r, r + 1)
        want = LR.push_stop(tokens[sl], done[sl], hist[sl], n_hist[sl], n_prompt[sl], n_gen[sl], None, 1, call_stops + own[r])
        for name, a, b in zip(("tokens", "done", "hist", "n_hist", "n_gen"), got, want):
            assert torch.equal(a.cpu()[sl], b), (r, name, a.cpu()[sl], b)
    assert got[1].cpu().tolist() == [0, 1, 1, 1, 1, 0, 0] and int(got[0][1]) == 1
    # without any table every row just appends; R == 0 is a no-op
    z = torch.zeros(7, dtype=I32, device=DEV)
    free = [t.clone().to(DEV) for t in (tokens, done, hist, n_hist, n_gen)]
    K.gen_push_stop_rows_(free[0], free[1], free[2], free[3], n_prompt.to(DEV), free[4], None, 1, None, 0, z, z)
    assert free[1].cpu().tolist() == done.tolist() and free[3].cpu().tolist() == (n_hist + (done == 0).to(I32)).tolist()
    e = torch.zeros(0, dtype=I32, device=DEV)
    K.gen_push_stop_rows_(e, e, torch.zeros(0, 4, dtype=I32, device=DEV), e, e, e, None, 1, None, 0, e, e)


# ---------------------------------------------------------------------------------------------- lmod_request_uniform_rows
def test_request_uniform_rows_equal_philox_reference():
    from llavamod import kernels as K
    rng = np.random.default_rng(17)
    N = 1024
    seed = rng.integers(0, 2 ** 63 - 1, N, dtype=np.int64).astype(np.uint64)
    seed[:4] = [5, 9, 2 ** 32 + 1, 0xF0E1D2C3B4A59687]                           # small, above 2^32, the top bit set
    seed[4:64] = 5                                                              # one call's seed under many request indices
    ctr0 = rng.integers(0, 2 ** 31 - 1, N).astype(np.int32)
    ctr0[:128] = np.arange(128) % 7
    gen = rng.integers(0, 4096, N).astype(np.int32)
    ctr = np.stack([ctr0.astype(np.int64), gen.astype(np.int64), np.zeros(N, np.int64), np.zeros(N, np.int64)], -1).astype(np.uint32)
    key = np.stack([seed & np.uint64(0xFFFFFFFF), seed >> np.uint64(32)], -1).astype(np.uint32)
    w = BR.philox4x32_10(ctr, key)[:, 0]
    want = ((w >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)).astype(np.float32)
    sd = torch.from_numpy(seed.view(np.int64)).to(DEV)
    u = K.request_uniform_rows(sd, torch.from_numpy(ctr0).to(DEV), torch.from_numpy(gen).to(DEV)).cpu().numpy()
    assert u.dtype == np.float32 and np.array_equal(u.view(np.uint32), want.view(np.uint32)), np.nonzero(u != want)[0][:5]
    assert u.min() >= 0.0 and u.max() < 1.0
    # a shared key and (request index, k) is lmod_request_uniform's stream
    same = K.request_uniform(5, torch.from_numpy(ctr0[4:64]).to(DEV), torch.from_numpy(gen[4:64]).to(DEV)).cpu().numpy()
    assert np.array_equal(same.view(np.uint32), u[4:64].view(np.uint32))
    e = torch.zeros(0, dtype=I32, device=DEV)
    assert K.request_uniform_rows(torch.zeros(0, dtype=torch.int64, device=DEV), e, e).numel() == 0


# ---------------------------------------------------------------------------------------------- generate_batch
NEW = 8


def _mixed_requests(stop):
    from llavamod.generation import RequestParams as P
    from test_batch_gpu import ORDER, _prompts
    params = [None, P(do_sample=True, temperature=1.5, top_p=0.9), P(do_sample=True, top_k=3, seed=9),
              P(repetition_penalty=1.3, no_repeat_ngram_size=2), P(stop_sequences=[stop])]
    reqs = [dict(_prompts()[p], max_new_tokens=NEW) for p in ORDER]
    for rq, prm in zip(reqs, params):
        if prm is not None:
            rq["params"] = prm
    return reqs


def test_generate_batch_with_a_different_params_per_request():
    """Five requests through two slots: plain greedy, sampled under the call's seed, sampled under its own seed, greedy with
    processors, greedy with its own stop sequence (tokens 2-3 of what it emits unconstrained)."""
    from llavamod import kernels as K
    from llavamod.generation import BatchOutput, SlotScheduler
    from test_batch_gpu import ORDER, _greedy_refs, _processed_alone, _scheduled_steps, _teacher
    teacher, refs = _teacher(), _greedy_refs()
    # precondition, stated: the fixture keeps the GPU's decode path tie-free for all NEW steps of either prompt
    assert min(s for _, s in refs) == NEW, refs
    stop = [int(t) for t in refs[ORDER[4]][0][2:4]]
    kw = dict(max_batch_size=2, seed=5, return_dict_in_generate=True)
    dec, adm = [], []
    orig_dec, orig_start = teacher._decode_step, teacher._start

    def spy_dec(tokens, cache):
        assert int(cache.lens.max()) < cache.smax, (cache.lens, cache.smax)
        lg = orig_dec(tokens, cache)
        dec.append(lg.clone())
        return lg

    def spy_start(*a):
        cache, lg = orig_start(*a)
        adm.append(lg.clone())
        return cache, lg

    teacher._decode_step, teacher._start = spy_dec, spy_start
    try:
        out = teacher.generate_batch(_mixed_requests(stop), **kw)
    finally:
        del teacher._decode_step, teacher._start
    assert isinstance(out, BatchOutput) and len(out.sequences) == 5 and len(out.token_logprobs) == 5
    lengths = [len(s) for s in out.sequences]
    for seq, lp in zip(out.sequences, out.token_logprobs):                      # a list for every request, greedy ones included
        assert seq.dtype == torch.int64 and lp.dtype == torch.float32 and lp.shape == seq.shape
        assert bool(torch.isfinite(lp).all()) and bool((lp <= 0).all()), lp
    # greedy requests: generate() of the prompt alone with the same processors, over the tie-safe prefix
    ref, safe = refs[ORDER[0]]
    assert lengths[0] == NEW and torch.equal(out.sequences[0][:safe].cpu(), ref[:safe]), (out.sequences[0], ref)
    ref, safe = _processed_alone(teacher, ORDER[3], repetition_penalty=1.3, no_repeat_ngram_size=2)
    assert lengths[3] == NEW and safe >= 2 and torch.equal(out.sequences[3][:safe].cpu(), ref[:safe]), (out.sequences[3], ref, safe)
    # the stop request: cut exactly behind its stop sequence
    ref, safe = refs[ORDER[4]]
    cut = LR.first_stop(ref.tolist(), [stop]) + 1
    assert cut <= 4 <= safe and lengths[4] == cut and torch.equal(out.sequences[4].cpu(), ref[:cut]), (out.sequences[4], ref, stop)
    # its slot was reused: 5 requests through 2 slots, in the steps the scheduler needs for these lengths
    assert out.num_admissions == 5
    assert out.num_decode_steps == _scheduled_steps([NEW] * 5, 2, lengths)
    # sampled requests: redraw every token with the SCALAR kernel from the logits the step saw, under the request's own parameters
    # and its own stream: (call seed 5, request index 1) and (own seed 9, counter word 0 = 0 although it is request 2)
    stream = {1: (5, 1, (1.5, None, 0.9)), 2: (9, 0, (1.0, 3, None))}
    sched, emitted = SlotScheduler([NEW] * 5, 2), [0] * 5
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
        for s, r in live.items():
            if r in stream:
                seed, ctr0, (T, k, p) = stream[r]
                u_ref = torch.from_numpy(BR.request_uniform(seed, [ctr0], [emitted[r]])).to(DEV)
                tok = K.sample(buf[s:s + 1], u_ref, T, k, p)
                assert int(tok[0]) == int(out.sequences[r][emitted[r]]), (r, emitted[r], s, tok, out.sequences[r])
                checked += 1
            emitted[r] += 1
        sched.step([s for s, r in live.items() if emitted[r] == lengths[r] < NEW])
        if sched.live:
            buf = next(dec_it).clone()
    assert checked == lengths[1] + lengths[2] == 2 * NEW and next(dec_it, None) is None and next(adm_it, None) is None
    # reproducible
    again = teacher.generate_batch(_mixed_requests(stop), **kw)
    assert all(torch.equal(a, b) for a, b in zip(out.sequences, again.sequences))
    assert all(torch.equal(a, b) for a, b in zip(out.token_logprobs, again.token_logprobs))


def test_without_params_generate_batch_runs_the_existing_kernels(monkeypatch):
    from llavamod import kernels as K
    from test_batch_gpu import BUDGETS, ORDER, _greedy_refs, _teacher
    teacher, refs = _teacher(), _greedy_refs()

    def never(*a, **k):
        raise AssertionError("a per-row kernel ran in a call without `params`")

    for name in ("sample_rows", "logits_process_rows_", "gen_push_stop_rows_", "request_uniform_rows"):
        monkeypatch.setattr(K, name, never)
    stripped = [{k: v for k, v in rq.items() if k != "params"} for rq in _mixed_requests([1, 2])]
    for rq, m in zip(stripped, BUDGETS):
        rq["max_new_tokens"] = m
    out = teacher.generate_batch(stripped, max_batch_size=2, seed=5, return_dict_in_generate=True)
    assert out.token_logprobs is None                                            # the call-wide arguments are greedy: as before
    for i, (p, m) in enumerate(zip(ORDER, BUDGETS)):
        ref, safe = refs[p]
        n = min(m, safe)
        assert out.sequences[i].shape == (m,) and torch.equal(out.sequences[i][:n].cpu(), ref[:n]), (i, out.sequences[i], ref)
    sampled = teacher.generate_batch(stripped, max_batch_size=2, do_sample=True, temperature=1.5, top_p=0.9, seed=5,
                                     return_dict_in_generate=True)                # test_batch_gpu replays this path token by token
    assert [len(s) for s in sampled.sequences] == BUDGETS and len(sampled.token_logprobs) == 5
