"""Per-request parameters of generate_batch on the host: the request dict's `params` key, generation.RequestParams, and what
generation.check_request_params makes of a call (inheritance, validation that names the request, the combined stop table, the
uniform stream of every request, the flags) — and that a call without `params` keeps the existing path.  No GPU, no HIP library."""
import os
import struct
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "llava-mod_amd"))

from llavamod import generation as G  # noqa: E402

V = 100
IDS = torch.tensor([1, 2, 3])


def _rq(params=None, **kw):
    d = dict(input_ids=IDS, **kw)
    if params is not None:
        d["params"] = params
    return d


def test_request_params_defaults_to_inherit_everything():
    p = G.RequestParams()
    assert G.RequestParams.FIELDS == ("do_sample", "temperature", "top_k", "top_p", "seed", "repetition_penalty",
                                      "no_repeat_ngram_size", "min_new_tokens", "stop_sequences")
    assert all(getattr(p, f) is None for f in G.RequestParams.FIELDS)
    assert G.RequestParams(temperature=0.7, top_p=0.9).temperature == 0.7


def test_check_batch_args_accepts_params_and_nothing_else_new():
    assert G.check_batch_args([_rq(G.RequestParams(temperature=0.7)), _rq(None, max_new_tokens=3), _rq()], 2, 16) == [16, 3, 16]
    with pytest.raises(ValueError, match="unknown keys"):                       # a top-level argument is still not a request key
        G.check_batch_args([_rq(temperature=0.7)], 2, 16)
    with pytest.raises(ValueError, match="unknown keys"):
        G.check_batch_args([_rq(G.RequestParams(), stop_sequences=[[1]])], 2, 16)
    with pytest.raises(ValueError, match="request 1.*RequestParams"):
        G.check_batch_args([_rq(), _rq(dict(temperature=0.7))], 2, 16)


def test_a_call_without_params_takes_the_existing_path():
    for kw in (dict(), dict(do_sample=True, temperature=0.2, top_p=0.7, seed=3, repetition_penalty=1.3, stop_sequences=[[4, 5]],
                            eos_token_id=2)):
        plan = G.check_request_params([_rq(), _rq(max_new_tokens=2)], vocab_size=V, **kw)
        assert plan.per_request is False and plan.records is None
    assert G.check_request_params([], vocab_size=V).per_request is False
    assert G.check_request_params([_rq(), _rq(G.RequestParams())], vocab_size=V).per_request is True     # the key alone decides


def test_none_fields_inherit_the_call():
    call = dict(do_sample=True, temperature=0.5, top_k=7, top_p=0.8, seed=5, repetition_penalty=1.2, no_repeat_ngram_size=3,
                min_new_tokens=4, eos_token_id=2, vocab_size=V)
    plan = G.check_request_params([_rq(G.RequestParams()), _rq(G.RequestParams(temperature=1.5, top_k=3, min_new_tokens=0)), _rq(),
                                   _rq(G.RequestParams(do_sample=False, repetition_penalty=1.0, no_repeat_ngram_size=0))], **call)
    a, b, c, d = plan.records
    for r in (a, c):                                                            # empty params and no params: the call's arguments
        assert (r.do_sample, r.temperature, r.top_k, r.top_p) == (True, 0.5, 7, 0.8)
        assert (r.penalty, r.ngram, r.min_new) == (1.2, 3, 4)
    assert (b.do_sample, b.temperature, b.top_k, b.top_p, b.penalty, b.ngram, b.min_new) == (True, 1.5, 3, 0.8, 1.2, 3, 0)
    assert (d.do_sample, d.temperature, d.top_k, d.top_p) == (False, 1.0, 0, 1.0)        # greedy: the neutral sampler values
    assert (d.penalty, d.ngram, d.min_new) == (1.0, 0, 4)
    assert plan.any_sample and plan.any_process and plan.any_penalty and plan.needs_call_seed
    # without an eos_token_id min_new_tokens has nothing to ban, as in generate()
    no_eos = G.check_request_params([_rq(G.RequestParams(min_new_tokens=3))], vocab_size=V)
    assert no_eos.records[0].min_new == 0 and not no_eos.any_process
    # the flags follow the requests, not the call
    greedy = G.check_request_params([_rq(G.RequestParams(no_repeat_ngram_size=2)), _rq()], vocab_size=V)
    assert not greedy.any_sample and greedy.any_process and not greedy.any_penalty and not greedy.needs_call_seed
    bad = G.check_request_params([_rq(G.RequestParams(seed=1))], vocab_size=V, suppress_tokens=[7])
    assert bad.any_process and bad.bad == [[7]] and not bad.any_penalty


def test_validation_errors_name_the_request():
    P = G.RequestParams
    with pytest.raises(ValueError, match="request 1: temperature"):
        G.check_request_params([_rq(), _rq(P(do_sample=True, temperature=0.0))], vocab_size=V)
    with pytest.raises(ValueError, match="request 2: temperature"):                 # the call samples; the request brings the value
        G.check_request_params([_rq(), _rq(P()), _rq(P(temperature=-1.0))], do_sample=True, vocab_size=V)
    with pytest.raises(ValueError, match="request 0: repetition_penalty"):
        G.check_request_params([_rq(P(repetition_penalty=0.0))], vocab_size=V)
    with pytest.raises(ValueError, match="request 1: repetition_penalty"):
        G.check_request_params([_rq(), _rq(P(repetition_penalty=-2))], vocab_size=V)
    with pytest.raises(ValueError, match=rf"request 1: stop_sequences: token id {V}"):
        G.check_request_params([_rq(), _rq(P(stop_sequences=[[3, V]]))], vocab_size=V)
    with pytest.raises(ValueError, match="request 0: top_p"):
        G.check_request_params([_rq(P(do_sample=True, top_p=0.0))], vocab_size=V)
    with pytest.raises(ValueError, match="request 0: top_k"):
        G.check_request_params([_rq(P(do_sample=True, top_k=0))], vocab_size=V)
    with pytest.raises(ValueError, match="request 0: no_repeat_ngram_size"):
        G.check_request_params([_rq(P(no_repeat_ngram_size=-1))], vocab_size=V)
    with pytest.raises(ValueError, match="request 0: seed"):
        G.check_request_params([_rq(P(seed=1.5))], vocab_size=V)
    with pytest.raises(ValueError, match="request 0: stop_sequences"):             # the call's and the request's share one row's budget
        G.check_request_params([_rq(P(stop_sequences=[[i] for i in range(9)]))], stop_sequences=[[50 + i] for i in range(8)],
                               vocab_size=V)
    # a greedy request may carry sampling values it does not use, as generate(do_sample=False, temperature=...) may
    G.check_request_params([_rq(P(temperature=0.0))], vocab_size=V)


def test_one_stop_table_call_wide_first_then_each_requests_own():
    P = G.RequestParams
    reqs = [_rq(P(stop_sequences=[[7, 8], [9]])), _rq(P(temperature=0.5)), _rq(P(stop_sequences=[[5, 6, 7]])), _rq()]
    plan = G.check_request_params(reqs, stop_sequences=[[1, 2], [3]], vocab_size=V)
    assert plan.stops == [[1, 2], [3], [7, 8], [9], [5, 6, 7]] and plan.n_call_stops == 2
    assert [(r.stop_first, r.stop_count) for r in plan.records] == [(2, 2), (0, 0), (4, 1), (0, 0)]
    none = G.check_request_params(reqs, vocab_size=V)                              # no call-wide stops: the table starts with the requests'
    assert none.stops == [[7, 8], [9], [5, 6, 7]] and none.n_call_stops == 0
    assert [(r.stop_first, r.stop_count) for r in none.records] == [(0, 2), (0, 0), (2, 1), (0, 0)]


def test_seed_and_first_counter_word():
    P = G.RequestParams
    reqs = [_rq(P(do_sample=True)), _rq(P(do_sample=True, seed=9)), _rq(), _rq(P(do_sample=True, seed=2 ** 40 + 3))]
    plan = G.check_request_params(reqs, seed=5, vocab_size=V)
    assert [(r.seed, r.ctr0) for r in plan.records] == [(5, 0), (9, 0), (5, 2), (2 ** 40 + 3, 0)]
    assert [r.do_sample for r in plan.records] == [True, True, False, True]
    moved = G.check_request_params([reqs[2], reqs[2], reqs[1], reqs[0]], seed=5, vocab_size=V)
    assert (moved.records[2].seed, moved.records[2].ctr0) == (9, 0)               # an own seed does not see the list index
    assert (moved.records[3].seed, moved.records[3].ctr0) == (5, 3)               # the call's stream is keyed by it
    unseeded = G.check_request_params(reqs, vocab_size=V)                         # generate_batch draws the call's seed when it is needed
    assert unseeded.needs_call_seed and unseeded.records[0].seed is None and unseeded.records[1].seed == 9
    assert not G.check_request_params(reqs[1:3], vocab_size=V).needs_call_seed


def test_device_table_layout():
    """Field-major [TABLE_ROWS, B] int32, floats bit-cast; rows 0-1 hold the B 64-bit keys as one u64 array."""
    P, RP = G.RequestParams, G.RequestPlan
    f32 = lambda x: struct.unpack("<i", struct.pack("<f", x))[0]
    B = 3
    tab = torch.tensor(RP.neutral_table(B), dtype=torch.int32)
    assert tab.shape == (RP.TABLE_ROWS, B) and RP.TABLE_ROWS == 12
    assert tab[RP.row_of("greedy")].tolist() == [1] * B and tab[RP.row_of("temperature")].tolist() == [f32(1.0)] * B
    assert tab[RP.row_of("penalty")].view(torch.float32).tolist() == [1.0] * B and tab[RP.row_of("top_p")].view(torch.float32).tolist() == [1.0] * B
    for f in ("seed", "ctr0", "top_k", "ngram", "min_new", "stop_first", "stop_count"):
        assert tab[RP.row_of(f)].tolist() == [0] * B, f
    reqs = [_rq(), _rq(P(do_sample=True, temperature=0.25, top_k=4, top_p=0.5, seed=(1 << 63) + (7 << 32) + 11, repetition_penalty=1.5,
                         no_repeat_ngram_size=2, min_new_tokens=3, stop_sequences=[[4]])), _rq(P(do_sample=True))]
    plan = G.check_request_params(reqs, stop_sequences=[[1]], eos_token_id=2, vocab_size=V)
    idx, val = plan.columns([(1, 2), (2, 0)], B, 5)
    assert len(idx) == len(val) == 2 * 12 and len(set(idx)) == len(idx) and all(-2 ** 31 <= v < 2 ** 31 for v in val)
    tab.view(-1)[torch.tensor(idx)] = torch.tensor(val, dtype=torch.int32)
    keys = tab[0:2].reshape(-1).view(torch.int64)
    assert [int(k) & (2 ** 64 - 1) for k in keys] == [5, 0, (1 << 63) + (7 << 32) + 11]
    col = lambda f, s: int(tab[RP.row_of(f), s])
    assert [col(f, 2) for f in ("ctr0", "greedy", "top_k", "ngram", "min_new", "stop_first", "stop_count")] == [0, 0, 4, 2, 3, 1, 1]
    assert [col(f, 2) for f in ("temperature", "top_p", "penalty")] == [f32(0.25), f32(0.5), f32(1.5)]
    assert [col(f, 0) for f in ("ctr0", "greedy", "top_k", "stop_count")] == [2, 0, 0, 0]
    assert [col(f, 1) for f in ("greedy", "temperature", "penalty")] == [1, f32(1.0), f32(1.0)]          # slot 1 stays idle: neutral
