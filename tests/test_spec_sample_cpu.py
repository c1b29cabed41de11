"""Speculative sampling on the CPU: the rule itself is exact (the analytic marginal of one round is the target's distribution), the
torch statement generation.spec_sample_rule against the looped fp64 reference of tests/_spec_sample_ref.py, block-layout parity with
spec_accept where every decision is forced, the argument checks, the C header / binding agreement, and the band caps of the GPU tests'
inputs confirmed with a plain torch fp32 stand-in for the kernel (tests/test_spec_sample_gpu.py states the bounds)."""
import os
import re
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "llava-mod_amd"))

import _sample_ref as SR  # noqa: E402
import _spec_sample_ref as SS  # noqa: E402
from llavamod.generation import check_assisted_args, check_spec_sample_args, spec_accept, spec_sample_rule  # noqa: E402

PAD = 3


def _pq(V, seed, T, k, tp, s=3.0):
    p, q = SS.make_logits(V, V, 1, s, seed)
    g = torch.Generator().manual_seed(seed)
    q = (q.float() + 2.0 * torch.randn(1, V, generator=g)).to(SS.BF)            # far enough apart for a real residual
    return SS.warped(p, T, k, tp)[0], SS.warped(q, T, k, tp)[0]


@pytest.mark.parametrize("V", [7, 64])
def test_rule_is_exact_analytic_marginal(V):
    """sum_d q(d) min(1, p(d)/q(d)) [x = d] + (1 - sum_d q(d) min(1, p/q)) r_hat(x) == p(x) to 1e-12, with filters that zero parts of
    either side."""
    n = 0
    for seed in range(6):
        for T, k, tp in [(1.0, None, None), (0.7, 3, None), (1.5, None, 0.6), (1.0, 5, 0.8), (0.2, None, 0.9)]:
            p, q = _pq(V, seed, T, k, tp)
            assert (SS.marginal(p, q) - p).abs().max().item() <= 1e-12, (V, seed, T, k, tp)
            # a different filter on each side: supports that only partly overlap
            q2 = _pq(V, seed + 50, 1.0, 2, None)[1]
            assert (SS.marginal(p, q2) - p).abs().max().item() <= 1e-12, (V, seed, T, k, tp)
            n += int((p == 0).any()) + int((q2 == 0).any())
    assert n > 0                                                   # some case did zero part of a side


def _random_case(B, k, V, seed, eos):
    g = torch.Generator().manual_seed(seed)
    p = torch.softmax(2 * torch.randn(B, k + 1, V, generator=g, dtype=torch.float64), -1)
    q = torch.softmax(2 * torch.randn(B, k, V, generator=g, dtype=torch.float64), -1)
    q = torch.where(torch.rand(B, k, 1, generator=g) < 0.4, p[:, :k], q)          # some positions with q == p: always accepted
    q[0] = p[0, :k]                                                                # sample 0 accepts every draft
    draft = torch.multinomial(q.view(B * k, V), 1, generator=g).view(B, k)
    u_acc, u_draw = torch.rand(B, k, generator=g, dtype=torch.float64), torch.rand(B, generator=g, dtype=torch.float64)
    done = (torch.rand(B, generator=g) < 0.2).int()
    done[0] = 0
    lt, ld = torch.randint(20, 60, (B,), generator=g) + k + 1, torch.randint(20, 60, (B,), generator=g) + k
    return p, q, draft, u_acc, u_draw, done, eos, lt, ld


@pytest.mark.parametrize("k", [1, 4, 15])
def test_rule_statement_equals_bruteforce(k):
    seen = set()
    for seed in range(12):
        p, q, draft, u_acc, u_draw, done, eos, lt, ld = _random_case(5, k, 11, seed, 2 if seed % 2 else None)
        block, nxt, dn, lt2, ld2 = spec_sample_rule(p, q, draft, u_acc, u_draw, done, eos, PAD, lt, ld)
        rows, n2, d2, t2, l2 = SS.block_bruteforce(p, q, draft.tolist(), u_acc.tolist(), u_draw.tolist(), done.tolist(), eos, PAD,
                                                   lt.tolist(), ld.tolist())
        assert block.tolist() == rows and nxt.tolist() == n2 and dn.long().tolist() == d2, (seed, block.tolist(), rows)
        assert lt2.tolist() == t2 and ld2.tolist() == l2
        seen |= set(block[:, k + 1].tolist())
    assert {0, k} <= seen                                           # both the all-rejected and the all-accepted block occurred


@pytest.mark.parametrize("k", [1, 4])
def test_block_parity_with_spec_accept_when_forced(k):
    """q == p: every draft accepted, the block is spec_accept's with target = [drafts, bonus].  Disjoint supports: the first draft is
    rejected, the block is spec_accept's with target[0] = the residual draw (a token the draft cannot propose)."""
    B, V = 4, 12
    p, _, draft, u_acc, u_draw, done, eos, lt, ld = _random_case(B, k, V, 3, 5)
    block, nxt, dn, lt2, ld2 = spec_sample_rule(p, p[:, :k], draft, u_acc, u_draw, done, eos, PAD, lt, ld)
    target = torch.cat([draft, block.new_tensor([SS.draw(p[b, k], float(u_draw[b])) for b in range(B)])[:, None]], 1)
    want = spec_accept(draft, target, done, eos, PAD, lt, ld)
    for a, b in zip((block, nxt, dn, lt2, ld2), want):
        assert torch.equal(a.long(), b.long())
    half = torch.arange(V) < V // 2
    pd = torch.where(half, p, torch.zeros_like(p))
    pd = pd / pd.sum(-1, keepdim=True)
    qd = torch.where(~half, p[:, :k], torch.zeros_like(p[:, :k]))
    qd = qd / qd.sum(-1, keepdim=True)
    draft = torch.multinomial(qd.view(B * k, V), 1).view(B, k)
    block, nxt, dn, lt2, ld2 = spec_sample_rule(pd, qd, draft, u_acc, u_draw, done, eos, PAD, lt, ld)
    assert torch.all(block[:, k + 1] == 0)
    first = block.new_tensor([SS.draw(pd[b, 0], float(u_draw[b])) for b in range(B)])
    target = torch.cat([first[:, None], draft], 1)                  # target[0] != draft[0]: spec_accept rejects at 0 as well
    want = spec_accept(draft, target, done, eos, PAD, lt, ld)
    for a, b in zip((block, nxt, dn, lt2, ld2), want):
        assert torch.equal(a.long(), b.long())


def test_argument_checks():
    ok = dict(num_beams=1, num_assistant_tokens=5, t_max=16)
    check_spec_sample_args(**ok, temperature=0.7, top_k=50, top_p=0.9)
    with pytest.raises(ValueError, match="num_beams"):
        check_spec_sample_args(**dict(ok, num_beams=2))
    with pytest.raises(ValueError, match="num_return_sequences"):
        check_spec_sample_args(**ok, num_return_sequences=2)
    for k in (0, 16, True, 2.0):
        with pytest.raises(ValueError, match="num_assistant_tokens"):
            check_spec_sample_args(**dict(ok, num_assistant_tokens=k))
    with pytest.raises(ValueError, match="temperature"):
        check_spec_sample_args(**ok, temperature=0.0)
    with pytest.raises(ValueError, match="top_k"):
        check_spec_sample_args(**ok, top_k=0)
    with pytest.raises(ValueError, match="top_p"):
        check_spec_sample_args(**ok, top_p=1.5)
    for name, v in (("repetition_penalty", 1.2), ("no_repeat_ngram_size", 2), ("bad_words_ids", [[1]]), ("suppress_tokens", [1]),
                    ("min_new_tokens", 2), ("stop_sequences", [[1, 2]]), ("stopping_criteria", [object()])):
        with pytest.raises(ValueError, match=f"{name}.*out of scope"):
            check_spec_sample_args(**ok, **{name: v})
    check_spec_sample_args(**ok, repetition_penalty=1.0, no_repeat_ngram_size=0, bad_words_ids=None, min_new_tokens=0)
    # the old refusal stands: sampling with an assistant through do_sample=True raises "greedy"
    with pytest.raises(ValueError, match="greedy"):
        check_assisted_args(True, 1, 5, 16)
    with pytest.raises(ValueError, match="greedy"):
        check_spec_sample_args(**ok, do_sample=True)


def test_generate_refuses_before_touching_the_model():
    """speculative_sampling=True without an assistant raises; assistant_model with do_sample=True keeps raising "greedy"."""
    from llavamod.model.language_model.llava_qwen2 import LlavaQwen2ForCausalLM as M

    class Head:
        weight = torch.zeros(8, 2)

    class Fake:
        lm_head = Head()

    with pytest.raises(ValueError, match="assistant_model"):
        M.generate(Fake(), input_ids=torch.zeros(1, 2, dtype=torch.long), speculative_sampling=True)
    with pytest.raises(ValueError, match="greedy"):
        M.generate(Fake(), input_ids=torch.zeros(1, 2, dtype=torch.long), assistant_model=Fake(), do_sample=True)
    with pytest.raises(ValueError, match="greedy"):
        M.generate(Fake(), input_ids=torch.zeros(1, 2, dtype=torch.long), assistant_model=Fake(), do_sample=True,
                   speculative_sampling=True)
    with pytest.raises(ValueError, match="out of scope"):
        M.generate(Fake(), input_ids=torch.zeros(1, 2, dtype=torch.long), assistant_model=Fake(), speculative_sampling=True,
                   stop_sequences=[[1]])


def test_header_binding_and_library_agree():
    from llavamod import _hip
    src = open(os.path.join(ROOT, "include", "lmod_hip.h")).read()
    code = {"p": "*", "i": "int", "q": "long long", "f": "float", "Q": "unsigned long long"}
    for name in ("lmod_spec_sample_bf16", "lmod_spec_uniform"):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", src, flags=re.S)
        assert m, f"{name} is not declared in include/lmod_hip.h"
        sig = ""
        for a in [a.strip() for a in m.group(1).split(",")]:
            t = a.rsplit(" ", 1)[0].replace("const ", "").strip()
            sig += "p" if ("*" in a or t == "hipStream_t") else {v: c for c, v in code.items()}[t]
        assert _hip.SIGNATURES[name] == sig, (name, sig)
        assert hasattr(_hip.load(), name)


@pytest.mark.parametrize("V,ld", SS.SHAPES)
def test_accept_inputs_keep_the_band_below_one_percent(V, ld):
    """The GPU accept test's cap, on the CPU: with the plain torch fp32 evaluation standing in for the kernel, the strata inside
    |u - ratio| < delta are at most 1 % of a row, and outside the band the stand-in decides as fp64 does."""
    us = SS.strata().double()
    for s in SS.SCALES:
        p, q = SS.accept_case(V, ld, s)
        for T, k, tp in SS.grid(V):
            for d in SS.draft_kinds(p, q, T, k, tp):
                r64, r32, floor, delta = SS.accept_band(p, q, d, T, k, tp)
                inside = (us - r64).abs() < delta
                assert int(inside.sum()) <= 0.01 * us.numel(), (V, s, T, k, tp, d, r64, delta)
                assert torch.equal((us < r32)[~inside], (us < r64)[~inside])
            tv = SS.residual_band(p, q, T, k, tp)[-1]
            assert tv >= 0.05, (V, s, T, k, tp, tv)                 # the residual test's precondition


@pytest.mark.parametrize("V,ld", SS.SHAPES)
def test_block_inputs_keep_banded_rows_below_two_percent(V, ld):
    rows = banded = 0
    for k in SS.BLOCK_KS:
        for T, tk, tp in SS.BLOCK_CASES:
            for trial in range(SS.block_trials(V)):
                c = SS.block_case(V, ld, k, T, tk, tp, trial)
                band = SS.block_reference(c, k, T, tk, tp)[-1]
                rows += 3
                banded += sum(b != k + 2 for b in band)
    assert banded <= 0.02 * rows, (banded, rows)
