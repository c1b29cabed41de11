"""Sampling without a GPU: the fp64 reference of tests/_sample_ref.py against kept sets and draws worked out by hand and against a
brute-force enumeration on tiny rows; generate()'s sampling argument checks; the header / binding / exported-symbol triple of
lmod_sample_bf16."""
import math
import os
import re
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "llava-mod_amd"))

import _sample_ref as SR  # noqa: E402

INF = float("inf")


def _row(vals):
    return torch.tensor([vals], dtype=torch.float32).to(torch.bfloat16)


def _kept(vals, T=1.0, top_k=None, top_p=None):
    return [i for i, k in enumerate(SR.keep_mask(_row(vals), T, top_k, top_p)[0].tolist()) if k]


def test_reference_kept_sets_by_hand():
    # a tie straddling the top-k cut: the 2nd largest value is 1 and it is held three times -> all of them stay
    assert _kept([2, 1, 1, 1, 0], top_k=2) == [0, 1, 2, 3]
    cut, n = SR.cutoff_and_count(_row([2, 1, 1, 1, 0]), 1.0, 2, None)
    assert cut.item() == 1.0 and n.item() == 4
    assert _kept([2, 1, 1, 1, 0], top_k=1) == [0]
    assert _kept([2, 1, 1, 1, 0], top_k=5) == [0, 1, 2, 3, 4] and _kept([2, 1, 1, 1, 0], top_k=7) == [0, 1, 2, 3, 4]
    # a tie straddling the top-p cut: p = e/(e+3) = 0.4754, then 0.1749 three times.  top_p = 0.6: token 1 has 0.4754 before it
    # (kept), token 2 has 0.6503 (not in the prefix) but ties with token 1 -> the threshold set keeps all four
    assert _kept([1, 0, 0, 0], top_p=0.6) == [0, 1, 2, 3]
    assert _kept([1, 0, 0, 0], top_p=0.4) == [0]                 # token 1 has 0.4754 > 0.4 before it
    assert _kept([1, 0, 0, -1], top_p=0.6) == [0, 1, 2]          # p = 0.4466, 0.1643, 0.1643, 0.0604: before token 1 0.4466 <= 0.6
    cut, n = SR.cutoff_and_count(_row([1, 0, 0, -1]), 1.0, None, 0.6)
    assert cut.item() == 0.0 and n.item() == 3
    # top_p tiny: the maximum alone, with its ties
    assert _kept([0.5, 3, 1, 3], top_p=1e-9) == [1, 3]
    assert _kept([0.5, 3, 1, 2], top_p=1e-9) == [1]
    # -inf entries weigh nothing and never enter: p over tokens {4, 1, 3} = 0.5761, 0.2119, 0.2119
    assert _kept([-INF, 0, -INF, 0, 1], top_p=0.99) == [1, 3, 4]
    assert _kept([-INF, 0, -INF, 0, 1], top_p=0.5) == [4]
    assert _kept([-INF, 0, -INF, 0, 1], top_k=2) == [1, 3, 4]    # the 2nd largest is 0, held twice
    # temperature comes first: at T = 0.25 the row [1, 0, 0, 0] becomes [4, 0, 0, 0], p0 = 0.9479
    assert _kept([1, 0, 0, 0], T=0.25, top_p=0.9) == [0]
    assert _kept([1, 0, 0, 0], T=1.0, top_p=0.9) == [0, 1, 2, 3]
    # top-k then top-p over the renormalised survivors: [2, 1, 0, -1] with top_k = 2 -> p = 0.7311, 0.2689; top_p = 0.7 keeps one
    # (without the top-k, p0 = 0.6439: token 1 would stay)
    assert _kept([2, 1, 0, -1], top_k=2, top_p=0.7) == [0]
    assert _kept([2, 1, 0, -1], top_p=0.7) == [0, 1]
    # no filter
    cut, n = SR.cutoff_and_count(_row([2, 1, 0, -1]), 1.0, None, None)
    assert cut.item() == -INF and n.item() == 4


def test_reference_draw_by_hand():
    # kept tokens 1, 3, 4 with masses 1, 1, e in token order: CDF 0.2119, 0.4239, 1
    row = _row([-INF, 0, -INF, 0, 1])
    for u, t in ((0.0, 1), (0.2, 1), (0.22, 3), (0.42, 3), (0.43, 4), (0.999999, 4)):
        assert SR.draw(row, torch.tensor([u]), 1.0, None, 0.99).item() == t, u
    # a constant row: uniform over token ids, whatever top_p says (all tied at the cutoff)
    row = _row([0.75] * 8)
    for i in range(8):
        assert SR.draw(row, torch.tensor([(i + 0.5) / 8]), 1.0, None, 0.5).item() == i
    # a row without a finite logit: token 0, lse -inf, kept fraction 0, no NaN
    row = _row([-INF] * 6)
    assert SR.draw(row, torch.tensor([0.7]), 1.0, None, 0.9).item() == 0
    lse, frac = SR.stats(row, 1.0, None, 0.9)
    assert lse.item() == -INF and frac.item() == 0.0
    # stats: [1, 0, 0, -1] at top_p 0.6 keeps e + 2 of e + 2 + 1/e
    lse, frac = SR.stats(_row([1, 0, 0, -1]), 1.0, None, 0.6)
    tot = math.e + 2 + 1 / math.e
    assert abs(lse.item() - math.log(tot)) < 1e-12 and abs(frac.item() - (math.e + 2) / tot) < 1e-12
    lp = SR.warped_logprob(_row([1, 0, 0, -1]), torch.tensor([1]), 1.0, None, 0.6)
    assert abs(lp.item() - math.log(1 / (math.e + 2))) < 1e-12


def _brute(vals, T, top_k, top_p, us):
    """Plain-python enumeration of the contract: (kept ids, drawn token per u)."""
    V = len(vals)
    x = [v / max(T, 1e-6) for v in vals]
    kept = list(range(V))
    if top_k is not None and 0 < top_k < V:
        kth = sorted(x, reverse=True)[top_k - 1]
        kept = [i for i in kept if x[i] >= kth]
    if top_p is not None and top_p < 1.0:
        order = sorted(kept, key=lambda i: (-x[i], i))
        mx = x[order[0]]
        w = [math.exp(x[i] - mx) if x[i] > -INF else 0.0 for i in order]
        tot = sum(w) or 1.0
        before, last = 0.0, order[0]
        for j, i in enumerate(order):
            if j > 0 and (before / tot > top_p or w[j] == 0.0):
                break
            last = i
            before += w[j]
        kept = [i for i in kept if x[i] >= x[last]]
    mx = max(x[i] for i in kept)
    w = [math.exp(x[i] - mx) if (i in kept and x[i] > -INF) else 0.0 for i in range(V)]
    tot = sum(w)
    drawn = []
    for u in us:
        cum, t = 0.0, 0
        lastk = 0
        for i in range(V):
            if w[i] > 0:
                lastk = i
        t = lastk
        for i in range(V):
            cum += w[i]
            if w[i] > 0 and cum > u * tot:
                t = i
                break
        drawn.append(t if tot > 0 else 0)
    return kept, drawn


@pytest.mark.parametrize("seed", range(12))
def test_reference_vs_brute_force_on_tiny_rows(seed):
    g = torch.Generator().manual_seed(seed)
    V = int(torch.randint(2, 17, (1,), generator=g))
    # coarse values (multiples of 0.5) so that ties are common; a few -inf entries
    vals = (torch.randint(-6, 7, (V,), generator=g).float() * 0.5)
    vals[torch.rand(V, generator=g) < 0.15] = -INF
    if not torch.isfinite(vals).any():
        vals[0] = 0.0
    row = vals.to(torch.bfloat16)[None, :]
    # uniforms away from the CDF's steps (the masses here are sums of a few exp(k/2T): a u on a multiple of 1/64 + 1/200 would need
    # a coincidence to sit within 1e-9 of one)
    us = [(i + 0.5) / 32 + 1 / 200 for i in range(31)] + [0.0]
    for T in (0.5, 1.0, 2.0):
        for top_k in (None, 1, 3, 50):
            for top_p in (None, 1e-6, 0.3, 0.7, 0.95, 1.0):
                kept, drawn = _brute(vals.tolist(), T, top_k, top_p, us)
                got = [i for i, k in enumerate(SR.keep_mask(row, T, top_k, top_p)[0].tolist()) if k]
                assert got == kept, (vals.tolist(), T, top_k, top_p, got, kept)
                rows = row.expand(len(us), V)
                t = SR.draw(rows, torch.tensor(us), T, top_k, top_p).tolist()
                assert t == drawn, (vals.tolist(), T, top_k, top_p, t, drawn)
                cut, n = SR.cutoff_and_count(row, T, top_k, top_p)
                assert n.item() == len(kept)


def test_check_sample_args():
    from llavamod.generation import SampleOutput, check_sample_args
    check_sample_args()
    check_sample_args(True, 0.2, None, 0.7, 1)
    check_sample_args(True, 1.5, 50, 1.0, 4)
    check_sample_args(True, 1, 1, None, 1)
    check_sample_args(False, 0.0, None, None, 1)                  # greedy ignores the sampling arguments, as before
    with pytest.raises(ValueError, match="num_return_sequences"):
        check_sample_args(False, 1.0, None, None, 2)              # greedy returns one sequence per prompt (HF raises too)
    for n in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match="num_return_sequences"):
            check_sample_args(True, 1.0, None, None, n)
    for t in (0, 0.0, -1.0, None, float("nan")):
        with pytest.raises(ValueError, match="temperature"):
            check_sample_args(True, t)
    for k in (0, -3, 2.5, True):
        with pytest.raises(ValueError, match="top_k"):
            check_sample_args(True, 1.0, k)
    for p in (0, 0.0, -0.1, 1.01, float("nan"), True):
        with pytest.raises(ValueError, match="top_p"):
            check_sample_args(True, 1.0, None, p)
    o = SampleOutput(torch.zeros(2, 3, dtype=torch.int64), torch.zeros(2, 3))
    assert o.sequences.shape == o.token_logprobs.shape


def test_sample_entry_point_is_declared_bound_and_exported():
    """include/lmod_hip.h, _hip.SIGNATURES and the built library agree on lmod_sample_bf16; kernels.sample and the model's
    switch exist."""
    from llavamod import _hip
    src = open(os.path.join(ROOT, "include", "lmod_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"\bint\s+lmod_sample_bf16\s*\(([^;]*?)\)\s*;", src, flags=re.S)
    assert m, "lmod_sample_bf16 is not declared in include/lmod_hip.h"
    sig = ""
    for p in m.group(1).split(","):
        p = p.strip()
        sig += "p" if ("*" in p or "hipStream_t" in p) else "q" if p.startswith("long long") else "f" if p.startswith("float") else "i"
    assert sig == "pqi" + "pi" + "fif" + "i" + "pq" + "pp" + "p"
    assert _hip.SIGNATURES["lmod_sample_bf16"] == sig
    if not os.path.exists(_hip.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    assert hasattr(_hip.load(), "lmod_sample_bf16")
    assert b"sample_draw_kernel" in open(_hip.LIB_PATH, "rb").read()
    from llavamod import kernels as K
    from llavamod.model import LlavaQwen2ForCausalLM
    assert callable(K.sample) and LlavaQwen2ForCausalLM.sample_on_device is True
    mk = open(os.path.join(ROOT, "llava-mod_amd", "csrc", "Makefile")).read()
    assert "sample.hip" in next(l for l in mk.split("\n") if l.startswith("SRCS ="))
