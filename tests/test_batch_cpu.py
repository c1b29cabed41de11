"""Continuous batching, host side (no GPU): generation.SlotScheduler against hand-computed and brute-force schedules, the static-batch
step count it is compared with, the numpy Philox of tests/_batch_ref.py against the published test vectors, and the argument checks of
generate_batch."""
import os
import random
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "llava-mod_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _batch_ref as BR  # noqa: E402
from llavamod import generation as G  # noqa: E402

FIRST = [2, 8, 4, 8, 6]


def _run(lengths, B, stops=None):
    """Drive a SlotScheduler to the end.  stops: {request: token count at which it reports EOS}.  Returns (scheduler, admissions
    [(step, request, slot)], per request the steps at which it held a slot)."""
    sched = G.SlotScheduler(lengths, B)
    stops = stops or {}
    admissions, held, emitted = [], {}, [0] * len(lengths)
    while not sched.finished:
        step = sched.num_decode_steps
        for r, s in sched.admit():
            admissions.append((step, r, s))
        live = sched.live
        assert len(set(live.values())) == len(live)                    # no request in two slots
        for s, r in live.items():
            held.setdefault(r, []).append((step, s))
            emitted[r] += 1
        stopped = [s for s, r in live.items() if stops.get(r) == emitted[r]]
        ended = sched.step(stopped)
        for r, s in ended:
            assert live[s] == r
        assert sched.num_decode_steps < 10 ** 6
    return sched, admissions, held


def _check(lengths, B, stops=None):
    sched, admissions, held = _run(lengths, B, stops)
    n = len(lengths)
    want = [min(lengths[r], (stops or {}).get(r, lengths[r])) for r in range(n)]
    assert [r for _, r, _ in admissions] == list(range(n))             # every request once, admitted in request order
    assert sched.num_admissions == n
    assert [t for t, _, _ in admissions] == sorted(t for t, _, _ in admissions)
    for r in range(n):
        steps = [t for t, _ in held[r]]
        assert len({s for _, s in held[r]}) == 1                       # a request never moves
        assert steps == list(range(steps[0], steps[0] + want[r]))     # it runs exactly its tokens, without a gap
    by_slot = {}
    for r in range(n):
        for t, s in held[r]:
            assert by_slot.setdefault((t, s), r) == r                  # no slot holds two requests at one step
    # brute force: request r starts when the slot that frees first (lowest number among equals) is free, in request order
    free_at, end = [0] * B, 0
    for r in range(n):
        s = min(range(B), key=lambda i: (free_at[i], i))
        assert held[r][0] == (free_at[s], s), (r, held[r][0], free_at)
        free_at[s] += want[r]
        end = max(end, free_at[s])
    assert sched.num_decode_steps == end
    assert sched.live_row_steps == sum(want) and sched.total_row_steps == B * end
    assert sched.live_fraction == sum(want) / (B * end)
    assert 1 <= sched.num_prefills <= n and sched.num_decode_forwards <= sched.num_decode_steps - 1
    return sched


def test_scheduler_five_requests_two_slots():
    """Lengths [2, 8, 4, 8, 6] at 2 slots, by hand (steps counted from 1): slot 0 runs request 0 in steps 1-2, request 2 in steps 3-6
    and request 3 in steps 7-14; slot 1 runs request 1 in steps 1-8 and request 4 in steps 9-14.  Both slots end at step 14, and
    every one of the 2 x 14 row-steps emits a token (2 + 4 + 8 = 8 + 6 = 14).  Prefill passes: {0, 1} together, then 2, 3 and 4
    alone = 4.  A decode forward follows every step but the last: 13."""
    sched = _check(FIRST, 2)
    assert sched.num_decode_steps == 14
    assert sched.num_admissions == 5 and sched.num_prefills == 4 and sched.num_decode_forwards == 13
    assert (sched.live_row_steps, sched.total_row_steps) == (28, 28) and sched.live_fraction == 1.0
    _, admissions, _ = _run(FIRST, 2)
    assert admissions == [(0, 0, 0), (0, 1, 1), (2, 2, 0), (6, 3, 0), (8, 4, 1)]          # (steps done before, request, slot)


@pytest.mark.parametrize("B", [1, 3, 8])
def test_scheduler_random_lengths(B):
    rng = random.Random(37 + B)
    lengths = [rng.randint(1, 24) for _ in range(37)]
    sched = _check(lengths, B)
    if B == 1:
        assert sched.num_decode_steps == sum(lengths) and sched.live_fraction == 1.0 and sched.num_decode_forwards == sum(lengths) - 37
    # early stops (EOS) free a slot before the budget is used up
    stops = {r: rng.randint(1, lengths[r]) for r in range(0, 37, 3)}
    _check(lengths, B, stops)


def test_static_batches_never_take_fewer_steps():
    """generate() over consecutive static batches runs every batch until its longest row ends: [2, 8 | 4, 8 | 6] at 2 slots is
    8 + 8 + 6 = 22 steps against the scheduler's 14."""
    assert G.static_batch_steps(FIRST, 2) == 22
    assert G.static_batch_steps(FIRST, 2) > _check(FIRST, 2).num_decode_steps
    rng = random.Random(5)
    for B in (1, 3, 8):
        lengths = [rng.randint(1, 24) for _ in range(37)]
        assert G.static_batch_steps(lengths, B) == sum(max(lengths[i:i + B]) for i in range(0, 37, B))
        assert G.static_batch_steps(lengths, B) >= _check(lengths, B).num_decode_steps


def test_scheduler_argument_errors():
    with pytest.raises(ValueError, match="max_batch_size"):
        G.SlotScheduler([1, 2], 0)
    with pytest.raises(ValueError, match="max_new_tokens"):
        G.SlotScheduler([1, 0], 2)
    sched = G.SlotScheduler([3], 2)
    with pytest.raises(RuntimeError, match="admit"):
        sched.step()
    sched.admit()
    with pytest.raises(ValueError, match="hold no request"):
        sched.step([1])
    assert G.SlotScheduler([], 4).finished


def test_philox_known_answers():
    """Philox4x32-10 test vectors of the Random123 distribution (kat_vectors): counter and key all zero, all ones, and the digits of
    pi.  There is no other Philox restatement in tests/ to compare with; csrc/moe.hip and csrc/batch.hip share one device copy."""
    kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for ctr, key, want in kat:
        got = BR.philox4x32_10(np.array(ctr, dtype=np.uint32), np.array(key, dtype=np.uint32))
        assert tuple(int(x) for x in got) == want, (ctr, [hex(int(x)) for x in got])
    # vectorised over counters = one at a time
    ctr = np.array([[1, 2, 0, 0], [7, 0, 0, 0], [0xfffffffe, 5, 0, 0]], dtype=np.uint32)
    key = np.array([5, 0], dtype=np.uint32)
    both = BR.philox4x32_10(ctr, key)
    for i in range(3):
        assert np.array_equal(both[i], BR.philox4x32_10(ctr[i], key))


def test_request_uniform_reference():
    """u = (word 0 >> 8) * 2^-24: a multiple of 2^-24 in [0, 1), a function of (seed, request, token index) alone."""
    req, gen = np.meshgrid(np.arange(64), np.arange(64), indexing="ij")
    u = BR.request_uniform(5, req.reshape(-1), gen.reshape(-1))
    assert u.dtype == np.float32 and u.min() >= 0.0 and u.max() < 1.0
    assert np.array_equal(u * 2 ** 24, np.floor(u * 2 ** 24))
    assert abs(float(u.mean()) - 0.5) < 4 / np.sqrt(12 * u.size)            # 4 sigma of a uniform mean
    w = BR.philox4x32_10(np.array([3, 9, 0, 0], dtype=np.uint32), np.array([5, 0], dtype=np.uint32))[0]
    assert float(BR.request_uniform(5, [3], [9])[0]) == (int(w) >> 8) / 2 ** 24
    assert BR.request_uniform(5, [3], [9])[0] != BR.request_uniform(5, [9], [3])[0]
    assert BR.request_uniform(5 + (1 << 32), [3], [9])[0] != BR.request_uniform(5, [3], [9])[0]      # the seed's high word is key word 1
    perm = np.random.default_rng(0).permutation(u.size)
    assert np.array_equal(BR.request_uniform(5, req.reshape(-1)[perm], gen.reshape(-1)[perm]), u[perm])


def test_generate_batch_argument_checks():
    """What generate_batch checks before it touches the device: the modes it leaves out, max_batch_size, the request dicts, and the
    sampling / logits arguments through the helpers generate() uses."""
    rq = [dict(input_ids=torch.tensor([1, 2, 3])), dict(input_ids=torch.tensor([4]), max_new_tokens=3)]
    assert G.check_batch_args(rq, 2, 16) == [16, 3]
    assert G.check_batch_args([], 2, 16) == []
    for kw, pat in ((dict(num_beams=2), "num_beams"), (dict(assistant_model=object()), "assistant_model"),
                    (dict(num_return_sequences=2), "num_return_sequences"), (dict(past_key_values=object()), "past_key_values")):
        with pytest.raises(ValueError, match=pat):
            G.check_batch_args(rq, 2, 16, **kw)
    for B in (0, -1, 2.0, True):
        with pytest.raises(ValueError, match="max_batch_size"):
            G.check_batch_args(rq, B, 16)
    with pytest.raises(ValueError, match="max_new_tokens"):
        G.check_batch_args(rq, 2, 0)
    with pytest.raises(ValueError, match="max_new_tokens"):
        G.check_batch_args([dict(input_ids=torch.tensor([1]), max_new_tokens=0)], 2, 16)
    with pytest.raises(ValueError, match="input_ids"):
        G.check_batch_args([dict(images=None)], 2, 16)
    with pytest.raises(ValueError, match="1-D"):
        G.check_batch_args([dict(input_ids=torch.tensor([[1, 2]]))], 2, 16)
    with pytest.raises(ValueError, match="unknown keys"):
        G.check_batch_args([dict(input_ids=torch.tensor([1]), temperature=0.5)], 2, 16)
    # the per-call arguments go through generate()'s own checks
    with pytest.raises(ValueError, match="temperature"):
        G.check_sample_args(True, 0.0, None, None, 1)
    with pytest.raises(ValueError, match="repetition_penalty"):
        G.check_logits_args(repetition_penalty=0.0, vocab_size=10)
    # the method itself raises before any device work: no model state is needed to get there
    from llavamod.model.language_model.llava_qwen2 import LlavaQwen2ForCausalLM
    for kw, pat in ((dict(num_beams=2), "num_beams"), (dict(assistant_model=object()), "assistant_model"),
                    (dict(num_return_sequences=2), "num_return_sequences"), (dict(past_key_values=object()), "past_key_values"),
                    (dict(max_batch_size=0), "max_batch_size")):
        with pytest.raises(ValueError, match=pat):
            LlavaQwen2ForCausalLM.generate_batch(None, rq, **kw)
