"""generate(past_key_values=...) and greedy assisted generation (generate(assistant_model=...)) on the golden small models."""
import math
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _append_ref as R  # noqa: E402
import _util as U  # noqa: E402

DEV = "cuda"
NEW = 8


def _pair():
    from test_generate_gpu import _pair as pair
    student, teacher = pair()
    for m in student.moe_layers():
        m.eval_capacity_factor = 64.0
    student.eval(), teacher.eval()
    return student, teacher


def _prompt():
    """tests/golden/append_prompt.safetensors (tools/make_append_fixture.py): ragged right-padded prompts with images on which the fp32
    oracle's greedy continuation of the teacher keeps every top-2 gap above 8 bf16 ulps for 9 steps."""
    g = U.load_golden("append_prompt.safetensors")
    return dict(input_ids=g["input_ids"], attention_mask=g["attention_mask"].bool(), images=g["images"].to(DEV).to(torch.bfloat16))


def _greedy_with_gaps(model, pr, n):
    """Plain greedy tokens [B, n] and, per sample, the number of leading steps whose top-2 logit gap is at least 8 bf16 ulps of the top
    logit (token equality across two kernel paths is only meaningful up to there)."""
    cache, lg = model._prefill(pr["input_ids"], pr["attention_mask"], pr["images"], n)
    toks, safe = [], None
    for i in range(n):
        t2 = lg.float().topk(2, -1).values
        ok = (t2[:, 0] - t2[:, 1]) >= 8 * R.ulp_bf16(t2[:, 0].cpu()).to(DEV).float()
        safe = ok.long() if safe is None else safe + (ok & (safe == i)).long()
        nxt = lg.argmax(-1).to(torch.int32)
        toks.append(nxt.long())
        if i + 1 < n:
            lg = model._decode_step(nxt.contiguous(), cache)
    return torch.stack(toks, 1), safe


@pytest.mark.parametrize("k", [1, 4])
def test_self_draft_equals_greedy_and_accepts(k):
    """The teacher drafting for itself: the same tokens as plain greedy, nearly every draft accepted — the statistics prove the assisted
    path ran (generate() swallows unknown keyword arguments, so token equality alone would also hold without the feature)."""
    from llavamod.generation import AssistedOutput
    _, teacher = _pair()
    pr = _prompt()
    ref = teacher.generate(**pr, max_new_tokens=NEW)
    toks, safe = _greedy_with_gaps(teacher, pr, NEW)
    assert torch.equal(ref, toks)
    out = teacher.generate(**pr, max_new_tokens=NEW, assistant_model=teacher, num_assistant_tokens=k, return_dict_in_generate=True)
    assert isinstance(out, AssistedOutput) and out.past_key_values is not None
    for b in range(ref.shape[0]):
        n = int(safe[b])
        assert n >= 6, (b, n)
        assert torch.equal(out.sequences[b, :n], ref[b, :n]), (b, out.sequences[b], ref[b])
    # precondition, stated: the fixture keeps the GPU's own decode path tie-free for all NEW steps (the oracle-side search leaves 1.5x
    # headroom); with it every draft must be accepted, so the bound on the target's forwards holds unconditionally
    assert int(safe.min()) == NEW, safe
    assert out.num_target_forwards <= math.ceil(NEW / (k + 1)) + 1, out.num_target_forwards
    assert out.num_rounds >= 1 and bool((out.num_accepted > 0).all()), out.num_accepted


def test_student_draft_equals_greedy_and_stops_at_eos():
    from llavamod.generation import AssistedOutput
    student, teacher = _pair()
    pr = _prompt()
    ref = teacher.generate(**pr, max_new_tokens=NEW)
    _, safe = _greedy_with_gaps(teacher, pr, NEW)
    out = teacher.generate(**pr, max_new_tokens=NEW, assistant_model=student, num_assistant_tokens=3, return_dict_in_generate=True)
    assert isinstance(out, AssistedOutput) and out.num_rounds >= 1 and out.num_target_forwards == out.num_rounds + 1
    assert out.num_accepted.shape == (ref.shape[0],)
    for b in range(ref.shape[0]):
        n = int(safe[b])
        assert n >= 6, (b, n)
        assert torch.equal(out.sequences[b, :n], ref[b, :n]), (b, out.sequences[b], ref[b])
    # a planted EOS: the token sample 0 emits at step 3 ends that row; every row is cut as plain greedy cuts it
    eos = int(ref[0, 3])
    ref_e = teacher.generate(**pr, max_new_tokens=NEW, eos_token_id=eos, pad_token_id=1)
    out_e = teacher.generate(**pr, max_new_tokens=NEW, eos_token_id=eos, pad_token_id=1, assistant_model=student, num_assistant_tokens=3)
    assert int(safe.min()) == NEW, safe                     # precondition, stated: no tie on the GPU's decode path within NEW steps
    assert torch.equal(out_e, ref_e), (out_e, ref_e)
    first = (ref_e[0] == eos).nonzero()[0, 0]
    assert int(first) <= 3 and torch.equal(out_e[0, :int(first) + 1], ref_e[0, :int(first) + 1]) and bool((out_e[0, int(first) + 1:] == 1).all())


def test_uneven_acceptance_never_writes_past_a_cache():
    """B 2 with one sample accepting (nearly) every draft and the other (nearly) none, stopped by max_new_tokens: the fast sample reaches
    max_new_tokens many rounds before the slow one.  It must stop advancing its caches by k + 1 per round (the host's stop reaches the
    device flag), and the draft cache must have room before every draft decode step, whose append is an unchecked indexed copy."""
    _, teacher = _pair()
    _, draft = _pair()                                      # the same weights in a second instance: a draft we can disturb
    pr = _prompt()
    k, new = 4, 24
    orig, seen = draft._decode_step, []

    def disturbed(tokens, cache):
        seen.append((int(cache.lens.max()), cache.smax))
        assert seen[-1][0] < seen[-1][1], seen[-1]          # the decode step writes at position lens: it must exist
        lg = orig(tokens, cache).clone()
        lg[1] = lg[1].roll(1)                               # sample 1's argmax moves to the next token id: its drafts are wrong
        return lg

    draft._decode_step = disturbed
    out = teacher.generate(**pr, max_new_tokens=new, assistant_model=draft, num_assistant_tokens=k, return_dict_in_generate=True)
    assert out.sequences.shape == (2, new) and len(seen) > 0
    assert int(out.num_accepted[0]) > int(out.num_accepted[1]), out.num_accepted
    assert out.num_rounds > math.ceil(new / (k + 1)) + 2, out.num_rounds            # the slow sample kept the loop going
    tc = out.past_key_values
    assert int(tc.lens.max()) <= tc.smax
    # a stopped sample advances one position per round: far fewer than k + 1 per round over the whole run
    plen = pr["attention_mask"].sum(1) + teacher.get_image_tower().num_patches - 1
    assert int(tc.lens[0]) - int(plen[0]) <= new + out.num_rounds, (tc.lens, plen, out.num_rounds)
    ref = teacher.generate(**pr, max_new_tokens=8)
    assert torch.equal(out.sequences[:, :8], ref)           # the fixture's tie-free steps


def test_assistant_argument_errors():
    student, teacher = _pair()
    pr = _prompt()
    with pytest.raises(ValueError, match="greedy"):
        teacher.generate(**pr, max_new_tokens=4, assistant_model=student, do_sample=True)
    with pytest.raises(ValueError, match="greedy"):
        teacher.generate(**pr, max_new_tokens=4, assistant_model=student, num_beams=2)
    with pytest.raises(ValueError, match="num_assistant_tokens"):
        teacher.generate(**pr, max_new_tokens=4, assistant_model=student, num_assistant_tokens=R.T_MAX)


@pytest.mark.parametrize("mode", ["greedy", "beam", "sample"])
def test_two_turn_generate_equals_one_generate_over_the_concatenation(mode):
    """Turn 1 with return_dict_in_generate hands its cache on; turn 2 feeds only the new tokens (turn 1's last token, which was never
    fed, then the new turn's text).  The result equals one generate() over prompt + turn-1 tokens + new text (text-only prompts, so the
    concatenation is a plain token row; equal lengths so that it needs no padding inside)."""
    _, teacher = _pair()
    gold = U.load_golden("append_prompt.safetensors")      # tie-free under the fp32 oracle for both turns (tools/make_append_fixture.py)
    ids, turn2 = gold["two_turn_ids"], gold["two_turn_next"]
    B, N1 = ids.shape[0], 5
    kw = dict(greedy={}, beam=dict(num_beams=2), sample=dict(do_sample=True, top_k=1, seed=5))[mode]
    first = teacher.generate(input_ids=ids, max_new_tokens=N1, return_dict_in_generate=True)
    assert first.past_key_values is not None and first.sequences.shape == (B, N1)
    t1 = first.sequences.cpu()
    new_ids = torch.cat([t1[:, -1:], turn2], 1)
    cont = teacher.generate(input_ids=new_ids, past_key_values=first.past_key_values, max_new_tokens=8, return_dict_in_generate=True, **kw)
    whole = teacher.generate(input_ids=torch.cat([ids, t1, turn2], 1), max_new_tokens=8, **kw)
    assert cont.past_key_values is not None
    _, safe = _greedy_with_gaps(teacher, dict(input_ids=torch.cat([ids, t1, turn2], 1), attention_mask=None, images=None), 8)
    for b in range(B):
        n = int(safe[b])
        assert n >= 6, (b, n)
        assert torch.equal(cont.sequences[b, :n].cpu(), whole[b, :n].cpu()), (mode, b, cont.sequences[b], whole[b])
