"""Speculative sampling on the device: lmod_spec_sample_bf16 (llava-mod_amd/csrc/specsample.hip) against the fp64 reference of
tests/_spec_sample_ref.py, and generate(assistant_model=..., speculative_sampling=True) on top of it.

Bounds (the project's standing rule, as in test_sample_gpu.py).  The reference works in fp64 on the exact bf16 logits; the kernel
evaluates exp in fp32 and is exact from there on.  floor = |plain torch fp32 evaluation - fp64| of the very quantity a test bounds
(the accept ratio min(1, p(d)/q(d)); the token-order residual CDF): neither side is the kernel.  delta = 2 * floor, floored at 1e-6;
both are printed per case.  Where the kernel's top-p cutoff (out_stats) lies inside the reference's bracket at top_p +- delta but is
not the reference's own, the fp64 distributions are taken over the threshold set at the kernel's cutoff; before that, the stats of
every p and q row pass test_sample_gpu._check_filter's cutoff checks (`_checked_keep`: the bracket, exact top-k, exact count).
The inputs are made on the CPU from fixed seeds (tests/_spec_sample_ref.py); tests/test_spec_sample_cpu.py confirms their band caps
with the fp32 stand-in.

Measured on an MI355X (every case of every test): no floor exceeded 5e-7, so delta was 1e-6 throughout; at most 1 of the 4098 strata
of a row lay inside an accept band; the worst |u - token interval| over all residual draws was 9.6e-13; no block row was banded.
Every p and q row's cutoff passed `_checked_keep`, and none sat at the edge of its bracket.
"""
import ctypes
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

import _sample_ref as SR  # noqa: E402
import _spec_sample_ref as SS  # noqa: E402

DEV = "cuda"
BF = torch.bfloat16
I32 = dict(device=DEV, dtype=torch.int32)


def _checked_keep(logits, T, k, p, st, tag):
    """The kept set the fp64 distributions of rows `logits` [R, V] are taken over, after the kernel's filter (st [R, 4], its stats
    records of these rows) has passed test_sample_gpu._check_filter's checks: n_kept == count(logit >= cutoff) exactly; without top-p
    the cutoff and the count are the reference's exactly; with top-p the cutoff lies between the reference's cutoffs at top_p + delta
    and top_p - delta, delta = 2 * max |cdf_fp32 - cdf_fp64| of these rows (plain torch softmax + cumsum), floored at 1e-6.  Only then:
    the reference's kept set, or on a row whose admitted cutoff is not the reference's own at top_p the threshold set at the kernel's
    cutoff (test_sample_gpu._eval_keep).  Returns (keep [R, V] on the CPU, rows at the bracket's edge)."""
    x = logits.to(DEV)
    V = x.shape[1]
    lv, cut, n_kept = x.double(), st[:, 3].to(DEV).double(), st[:, 2].to(DEV).double()
    assert not torch.isnan(st).any(), tag
    assert torch.equal(n_kept, (lv >= cut[:, None]).sum(-1).double()), (tag, "n_kept != count(x >= cutoff)", n_kept.tolist())
    cut_ref, n_ref = SR.cutoff_and_count(x, T, k, p)
    if p is None or p >= 1.0:
        assert torch.equal(cut, cut_ref) and torch.equal(n_kept, n_ref.double()), (tag, "cutoff / count not exact", cut.tolist(), cut_ref.tolist())
    else:
        t = max(float(np.float32(T)), 1e-6)
        floor = (torch.softmax(x.float() / t, -1).cumsum(-1).double() - torch.softmax(lv / t, -1).cumsum(-1)).abs().max().item()
        delta = max(2.0 * floor, 1e-6)
        lo_cut, _ = SR.cutoff_and_count(x, T, k, min(p + delta, 1.0))
        hi_cut, _ = SR.cutoff_and_count(x, T, k, max(p - delta, 0.0))
        assert torch.all(lo_cut <= cut) and torch.all(cut <= hi_cut), (tag, "cutoff outside the bracket", lo_cut.tolist(), cut.tolist(), hi_cut.tolist())
    same = cut_ref == cut
    keep = torch.where(same[:, None], SR.keep_mask(x, T, k, p), lv >= cut[:, None])
    return keep.cpu(), int((~same).sum())


def _rep(row, n, ld):
    """One bf16 row [V] replicated to n rows of a [n, ld] device buffer."""
    V = row.shape[-1]
    out = torch.empty(n, ld, device=DEV, dtype=BF)[:, :V]
    out.copy_(row.to(DEV).view(1, V).expand(n, V))
    return out


def _rep2(p2, n, ld):
    """The two p rows of a k = 1 sample replicated to n samples: [2n, ld] with rows 2b = p2[0], 2b + 1 = p2[1]."""
    V = p2.shape[-1]
    out = torch.empty(2 * n, ld, device=DEV, dtype=BF)[:, :V]
    out.view(n, 2, V).copy_(p2.to(DEV).view(1, 2, V).expand(n, 2, V))
    return out


def _state(B, k):
    return (torch.zeros(B, **I32), torch.full((B,), 30 + k + 1, **I32), torch.full((B,), 30 + k, **I32))


def _one_position(P, Q, d, u_acc, u_draw, T, k, tp):
    """k = 1: every sample sees the same rows (P = _rep2(p), Q = _rep(q)) and the draft d; per-sample uniforms.  Returns (n_acc [n],
    next_token [n], stats of the two p rows [2, 4] and of the q row [1, 4])."""
    from llavamod import kernels as K
    n = u_acc.numel()
    done, lt, ldr = _state(n, 1)
    draft = torch.full((n, 1), int(d), **I32)
    block, nxt, st = K.spec_sample(P, Q, draft, u_acc.to(DEV).view(n, 1).contiguous(), u_draw.to(DEV).contiguous(), done, None, 3,
                                   lt, ldr, T, k, tp, stats=True)
    assert not torch.isnan(st).any()
    sp, sq = st[:2 * n].view(n, 2, 4), st[2 * n:]
    assert torch.equal(sp, sp[:1].expand_as(sp)) and torch.equal(sq, sq[:1].expand_as(sq)), "stats differ between copies of one row"
    assert torch.equal(block[:, 4], nxt)
    return block[:, 2].cpu().long(), nxt.cpu().long(), sp[0].cpu(), sq[:1].cpu()


@pytest.mark.parametrize("V,ld", SS.SHAPES)
@pytest.mark.parametrize("s", SS.SCALES)
def test_accept_decision_every_stratum(V, ld, s):
    """k = 1, one (p, q, d) replicated to 4096 + 2 samples with stratified u_acc: accepted whenever u <= ratio - delta, rejected whenever
    u >= ratio + delta; the band in between holds at most 1 % of the strata.  d: drawn from q, a token with p > q, a token outside p's
    kept set (always rejected), the arg-max of q."""
    us = SS.strata()
    n = us.numel()
    p, q = SS.accept_case(V, ld, s)
    P, Q = _rep2(p, n, ld), _rep(q[0], n, ld)
    for T, k, tp in SS.grid(V):
        kinds = SS.draft_kinds(p, q, T, k, tp)
        for kind, d in zip(("from_q", "p>q", "outside_p", "argmax_q"), kinds):
            tag = f"V={V} s={s} T={T} top_k={k} top_p={tp} d={kind}:{d}"
            n_acc, _, sp, sq = _one_position(P, Q, d, us, torch.full((n,), 0.5), T, k, tp)
            (kp, mp), (kq, mq) = _checked_keep(p, T, k, tp, sp, tag), _checked_keep(q, T, k, tp, sq, tag)
            kp = kp[:1]
            ratio, _, floor, delta = SS.accept_band(p, q, d, T, k, tp, kp, kq)
            acc, ud = n_acc == 1, us.double()
            band = int(((ud - ratio).abs() < delta).sum())
            print(f"{tag}: ratio={ratio:.6f} floor={floor:.3e} delta={delta:.3e} accepted={int(acc.sum())}/{n} in_band={band} "
                  f"rows_at_bracket_edge={mp + mq}")
            assert band <= 0.01 * n, (tag, band)
            assert bool(acc[ud <= ratio - delta].all()), (tag, "rejected below ratio - delta")
            assert not bool(acc[ud >= ratio + delta].any()), (tag, "accepted above ratio + delta")
            if kind == "outside_p":
                assert not bool(acc.any()), tag


@pytest.mark.parametrize("V,ld", SS.SHAPES)
@pytest.mark.parametrize("s", SS.SCALES)
def test_residual_draw_every_stratum(V, ld, s):
    """Rejection forced at position 0 (u_acc just below 1, d with q > p), stratified u_draw: every returned token t has
    cdf_lo(t) - delta <= u <= cdf_hi(t) + delta on the fp64 token-order residual CDF and p(t) - q(t) > -delta.  No draw is excluded."""
    us = SS.strata()
    n = us.numel()
    p, q = SS.accept_case(V, ld, s)
    P, Q = _rep2(p, n, ld), _rep(q[0], n, ld)
    for T, k, tp in SS.grid(V):
        tag = f"V={V} s={s} T={T} top_k={k} top_p={tp}"
        P0, Q0 = SS.warped(p[:1], T, k, tp)[0], SS.warped(q, T, k, tp)[0]
        d = int((Q0 - P0).argmax())
        n_acc, tok, sp, sq = _one_position(P, Q, d, torch.full((n,), SS.U_MAX), us, T, k, tp)
        assert bool((n_acc == 0).all()), (tag, "the forced rejection was accepted")
        (kp, mp), (kq, mq) = _checked_keep(p, T, k, tp, sp, tag), _checked_keep(q, T, k, tp, sq, tag)
        kp = kp[:1]
        Pk, Qk, lo, hi, floor, delta, tv = SS.residual_band(p, q, T, k, tp, kp, kq)
        assert tv >= 0.05, (tag, tv)
        assert bool(((tok >= 0) & (tok < V)).all()), tag
        ud = us.double()
        under = (lo[tok] - ud).clamp_min(0).max().item()
        over = (ud - hi[tok]).clamp_min(0).max().item()
        worst = (Pk[tok] - Qk[tok]).min().item()
        print(f"{tag}: tv={tv:.3f} floor={floor:.3e} delta={delta:.3e} worst |u - interval|={max(under, over):.3e} "
              f"min p(t)-q(t)={worst:.3e} distinct tokens={tok.unique().numel()} rows_at_bracket_edge={mp + mq}")
        assert under <= delta and over <= delta, (tag, under, over, delta)
        assert worst > -delta, (tag, worst, delta)


@pytest.mark.parametrize("V,ld", SS.SHAPES)
@pytest.mark.parametrize("k", [1, 4, 15])
def test_bonus_draw_equals_the_sampler(V, ld, k):
    """q_logits identical to p_logits: for every u all k drafts are accepted and next_token is bit-identical to
    lmod_sample_bf16 on the p_k rows with u_draw."""
    from llavamod import kernels as K
    B = 8
    g = torch.Generator().manual_seed(V + k)
    for T, tk, tp in [(1.0, None, None), (0.2, 50, 0.9), (1.5, None, 0.7), (1.0, 50, None)]:
        p, _ = SS.make_logits(V, ld, B * (k + 1), 3.0 if k % 2 else 8.0, 300 + k)
        P = torch.empty(B * (k + 1), ld, device=DEV, dtype=BF)[:, :V]
        P.copy_(p.to(DEV))
        Q = torch.empty(B * k, ld, device=DEV, dtype=BF)[:, :V]
        Q.view(B, k, V).copy_(P.view(B, k + 1, V)[:, :k])
        u_d = torch.rand(B * k, generator=g).to(DEV)
        draft = K.sample(Q, u_d, T, tk, tp).view(B, k).contiguous()
        u_acc = torch.rand(B, k, generator=g)
        u_acc[0] = SS.U_MAX                                           # the largest uniform still accepts when q == p
        u_acc[1] = 0.0
        u_draw = torch.rand(B, generator=g)
        u_draw[0], u_draw[1] = 0.0, SS.U_MAX
        u_draw = u_draw.to(DEV)
        done, lt, ldr = _state(B, k)
        block, nxt = K.spec_sample(P, Q, draft, u_acc.to(DEV), u_draw, done, None, 3, lt, ldr, T, tk, tp)
        assert bool((block[:, k + 1] == k).all()), (T, tk, tp, block[:, k + 1].tolist())
        pk = P.view(B, k + 1, V)[:, k]
        want = K.sample(pk, u_draw, T, tk, tp)
        assert torch.equal(nxt, want), (T, tk, tp, nxt.tolist(), want.tolist())
        assert torch.equal(block[:, :k], draft) and torch.equal(block[:, k], want) and bool((block[:, k + 2] == k + 1).all())
        assert lt.tolist() == [30 + k + 1] * B and ldr.tolist() == [30 + k] * B      # nothing rolled back


@pytest.mark.parametrize("V,ld", SS.SHAPES)
def test_block_semantics(V, ld):
    """B = 3 (sample 2 done, an EOS planted at sample 0's second draft), k in {4, 15}, random uniforms, against the fp64 reference block:
    tokens, n_acc, n_emitted, next_token, done, both lens.  A row with a decision inside its band is compared only up to that position;
    at most 2 % of the rows are."""
    from llavamod import kernels as K
    rows = banded = eos_cut = 0
    for k in SS.BLOCK_KS:
        for T, tk, tp in SS.BLOCK_CASES:
            for trial in range(SS.block_trials(V)):
                c = SS.block_case(V, ld, k, T, tk, tp, trial)
                P = torch.empty(3 * (k + 1), ld, device=DEV, dtype=BF)[:, :V]
                P.copy_(c["p"].to(DEV))
                Q = torch.empty(3 * k, ld, device=DEV, dtype=BF)[:, :V]
                Q.copy_(c["q"].to(DEV))
                done, lt, ldr = c["done"].to(DEV), c["lt"].to(DEV), c["ld"].to(DEV)
                block, nxt, st = K.spec_sample(P, Q, c["draft"].to(DEV), c["u_acc"].to(DEV), c["u_draw"].to(DEV), done, c["eos"], c["pad"],
                                               lt, ldr, T, tk, tp, stats=True)
                st = st.cpu()
                tag = f"V={V} k={k} T={T} top_k={tk} top_p={tp} trial={trial}"
                kp, mp = _checked_keep(c["p"], T, tk, tp, st[:3 * (k + 1)], tag)
                kq, mq = _checked_keep(c["q"], T, tk, tp, st[3 * (k + 1):], tag)
                want, wn, wd, wlt, wld, band = SS.block_reference(c, k, T, tk, tp, kp, kq)
                block, nxt = block.cpu().tolist(), nxt.cpu().tolist()
                print(f"{tag}: rows_at_bracket_edge={mp + mq} n_acc={[r[k + 1] for r in block]} n_emit={[r[k + 2] for r in block]} band={band}")
                for b in range(3):
                    rows += 1
                    if band[b] != k + 2:                               # compared up to the banded position only
                        banded += 1
                        assert block[b][:band[b]] == want[b][:band[b]], (tag, b, block[b], want[b])
                        continue
                    assert block[b] == want[b], (tag, b, block[b], want[b])
                    assert nxt[b] == wn[b] and int(done[b]) == wd[b] and int(lt[b]) == wlt[b] and int(ldr[b]) == wld[b], (tag, b)
                assert block[2] == [c["pad"]] * (k + 1) + [0, 0, c["pad"], 1], (tag, "a done row emits nothing")
                r0 = block[0]
                eos_cut += int(r0[k + 4] == 1 and r0[k + 2] < r0[k + 1] + 1 and r0[r0[k + 2] - 1] == c["eos"])
    assert banded <= 0.02 * rows, (banded, rows)
    assert eos_cut >= 1, "no trial cut a block at the planted EOS"


def _first_two(pl, ql, N, T, tk, tp, seed):
    """N samples of the fixed rows pl [k+1, V] / ql [k, V] in calls of 8192: drafts drawn from q by lmod_sample_bf16 with Philox
    uniforms.  Returns the emitted tokens [N, k+1] and n_emitted [N]."""
    from llavamod import kernels as K
    k, V = ql.shape
    Bc = 8192
    P = torch.empty(Bc * (k + 1), V, device=DEV, dtype=BF)
    P.view(Bc, k + 1, V).copy_(pl.to(DEV)[None].expand(Bc, k + 1, V))
    Q = torch.empty(Bc * k, V, device=DEV, dtype=BF)
    Q.view(Bc, k, V).copy_(ql.to(DEV)[None].expand(Bc, k, V))
    toks, nem = [], []
    for c0 in range(0, N, Bc):
        u_d = K.spec_uniform(seed, Bc, 1, K.SPEC_DRAFT, k, row0=c0).view(-1)
        u_a = K.spec_uniform(seed, Bc, 1, K.SPEC_ACCEPT, k, row0=c0)
        u_n = K.spec_uniform(seed, Bc, 1, K.SPEC_DRAW, 1, row0=c0).view(-1)
        draft = K.sample(Q, u_d, T, tk, tp).view(Bc, k).contiguous()
        done, lt, ldr = _state(Bc, k)
        block, _ = K.spec_sample(P, Q, draft, u_a, u_n, done, None, 0, lt, ldr, T, tk, tp)
        toks.append(block[:, :k + 1].cpu()), nem.append(block[:, k + 2].cpu())
    return torch.cat(toks).long(), torch.cat(nem).long()


def _law_ok(tokens, law, V):
    N = tokens.numel()
    f = torch.bincount(tokens, minlength=V).double() / N
    return bool(((f - law).abs() <= 5 * torch.sqrt(law * (1 - law) / N) + 1.0 / N).all()), N


@pytest.mark.parametrize("T,tk,tp", [(1.0, None, None), (0.8, 20, 0.9)])
def test_emitted_tokens_follow_the_target_distribution(T, tk, tp):
    """The property the feature exists for.  V = 64, k = 3, fixed far-apart rows, N = 65536: the empirical law of the first emitted
    token satisfies |f(x) - p_0(x)| <= 5 sqrt(p(1-p)/N) + 1/N for every x, and the same statistic against q_0 violates it (the test has
    power); the same for the second emitted token, conditioned on the most frequent first token (count >= 4096), against p_1 / q_1."""
    V, k, N = 64, 3, 65536
    g = torch.Generator().manual_seed(11)
    pl = (2.0 * torch.randn(k + 1, V, generator=g)).to(BF)
    ql = (pl[:k].float() + 1.0 * torch.randn(k, V, generator=g)).to(BF)
    toks, nem = _first_two(pl, ql, N, T, tk, tp, seed=2024)
    Pw, Qw = SS.warped(pl, T, tk, tp), SS.warped(ql, T, tk, tp)
    assert 0.5 * (Pw[0] - Qw[0]).abs().sum() > 0.15 and 0.5 * (Pw[1] - Qw[1]).abs().sum() > 0.15          # far apart
    ok_p, _ = _law_ok(toks[:, 0], Pw[0], V)
    ok_q, _ = _law_ok(toks[:, 0], Qw[0], V)
    acc = float((nem - 1).double().mean()) / k
    print(f"T={T} top_k={tk} top_p={tp}: accepted fraction of drafts={acc:.3f} first-token law ok vs p={ok_p} vs q={ok_q}")
    assert ok_p, "the first emitted token does not follow the target's distribution"
    assert not ok_q, "the statistic cannot tell p from q: no power"
    x = int(torch.bincount(toks[:, 0], minlength=V).argmax())
    sel = (toks[:, 0] == x) & (nem >= 2)
    assert int((toks[:, 0] == x).sum()) >= 4096 and int(sel.sum()) >= 1024, (x, int(sel.sum()))
    ok_p, n2 = _law_ok(toks[sel, 1], Pw[1], V)
    ok_q, _ = _law_ok(toks[sel, 1], Qw[1], V)
    print(f"second token given first={x}: N={n2} law ok vs p={ok_p} vs q={ok_q}")
    assert ok_p, "the second emitted token does not follow the target's distribution"
    assert not ok_q, "the second-token statistic has no power"


def test_reproducible_and_edge_rows():
    from llavamod import kernels as K
    V, ld, k, B = 151936, 151936, 5, 4
    p, q = SS.make_logits(V, ld, B * (k + 1), 3.0, 77)
    P, Q = p.to(DEV), q.view(B, k + 1, V)[:, :k].reshape(B * k, V).to(DEV)
    g = torch.Generator().manual_seed(3)
    u_a, u_n = torch.rand(B, k, generator=g).to(DEV), torch.rand(B, generator=g).to(DEV)
    for tk, tp in [(None, None), (50, 0.9)]:
        draft = K.sample(Q, torch.rand(B * k, generator=g).to(DEV), 1.0, tk, tp).view(B, k).contiguous()
        outs = []
        for _ in range(2):
            done, lt, ldr = _state(B, k)
            block, nxt, st = K.spec_sample(P, Q, draft, u_a, u_n, done, 9, 3, lt, ldr, 1.0, tk, tp, stats=True)
            outs.append((block, nxt, st.view(torch.int32), done, lt, ldr))
        for a, b in zip(*outs):
            assert torch.equal(a, b), (tk, tp)
    # a row without a finite logit, on the p side (sample 0, position 0) and on the q side (sample 1, position 0)
    V, ld, k, B = 1003, 1008, 2, 2
    p, q = SS.make_logits(V, ld, B * (k + 1), 3.0, 78)
    q = q.view(B, k + 1, V)[:, :k].reshape(B * k, V).clone()
    p, q = p.clone(), q
    p[0], q[k] = float("-inf"), float("-inf")
    P = torch.empty(B * (k + 1), ld, device=DEV, dtype=BF)[:, :V]
    P.copy_(p.to(DEV))
    Q = torch.empty(B * k, ld, device=DEV, dtype=BF)[:, :V]
    Q.copy_(q.to(DEV))
    for tk, tp in SS.FILTERS:
        done, lt, ldr = _state(B, k)
        draft = torch.tensor([[5, 6], [7, 8]], **I32)
        block, nxt, st = K.spec_sample(P, Q, draft, torch.full((B, k), 0.5, device=DEV), torch.full((B,), 0.5, device=DEV), done, None,
                                       3, lt, ldr, 1.0, tk, tp, stats=True)
        assert not torch.isnan(st).any(), (tk, tp)
        assert block[:, k + 1].tolist() == [0, 0] and bool(((nxt >= 0) & (nxt < V)).all()), (tk, tp, block.tolist())
        assert int(nxt[0]) == 0                                        # nothing to draw from: token 0, as lmod_sample_bf16


def test_argument_errors_run_nothing():
    from llavamod import _hip
    lib = _hip.load()
    V, B, k = 64, 2, 3
    P = torch.zeros(B * (k + 1), V, device=DEV, dtype=BF)
    Q = torch.zeros(B * k, V, device=DEV, dtype=BF)
    draft = torch.zeros(B, k, **I32)
    ua, un = torch.zeros(B, k, device=DEV), torch.zeros(B, device=DEV)
    ws = torch.zeros(1 << 20, device=DEV, dtype=torch.uint8)
    done, lt, ldr = _state(B, k)
    out, nxt = torch.full((B, k + 5), -7, **I32), torch.full((B,), -7, **I32)
    stream = torch.cuda.current_stream().cuda_stream
    R = B * (2 * k + 1)
    need = R * (64 + 16) + B * (32 + 16)

    def run(ld_p=V, ld_q=V, v=V, b=B, kk=k, chunk=64, ws_bytes=ws.numel(), top_k=0, q=Q):
        return lib.lmod_spec_sample_bf16(P.data_ptr(), ld_p, None if q is None else q.data_ptr(), ld_q, v, draft.data_ptr(), ua.data_ptr(),
                                         un.data_ptr(), b, kk, ctypes.c_float(1.0), top_k, ctypes.c_float(1.0), chunk, ws.data_ptr(),
                                         ws_bytes, done.data_ptr(), -1, 0, lt.data_ptr(), ldr.data_ptr(), out.data_ptr(), nxt.data_ptr(),
                                         None, stream)

    assert run(kk=0) == -1 and run(kk=16) == -1 and run(b=-1) == -1 and run(b=65535) == -1
    assert run(v=1) == -1 and run(ld_p=V - 1) == -1 and run(ld_q=V - 1) == -1 and run(chunk=12) == -1 and run(q=None) == -1
    assert run(ws_bytes=need - 1) == -1 and run(ws_bytes=R * (64 + 2 * 3072 + 16) + B * (32 + 16) - 1, top_k=5) == -1
    assert lib.lmod_spec_uniform(1, 0, 0, 3, 1, un.data_ptr(), B, stream) == -1
    assert lib.lmod_spec_uniform(1, 0, 0, 0, 0, un.data_ptr(), B, stream) == -1
    assert run(b=0) == 0
    torch.cuda.synchronize()
    assert out.tolist() == [[-7] * (k + 5)] * B and nxt.tolist() == [-7] * B and lt.tolist() == [30 + k + 1] * B     # nothing ran
    assert run(ws_bytes=need) == 0
    torch.cuda.synchronize()
    # constant rows on both sides, u = 0: every draft accepted (0 * q < p), the bonus draw is the first token
    assert out.tolist() == [[0] * (k + 1) + [k, k + 1, 0, 0]] * B


def test_spec_uniform_is_a_pure_function_of_its_coordinates():
    from llavamod import kernels as K
    a = K.spec_uniform(5, 64, 3, K.SPEC_ACCEPT, 4)
    assert torch.equal(a, K.spec_uniform(5, 64, 3, K.SPEC_ACCEPT, 4))
    assert torch.equal(a[16:48], K.spec_uniform(5, 32, 3, K.SPEC_ACCEPT, 4, row0=16))           # independent of the batch around a row
    assert torch.equal(a[:, :2], K.spec_uniform(5, 64, 3, K.SPEC_ACCEPT, 2))
    for other in (K.spec_uniform(6, 64, 3, K.SPEC_ACCEPT, 4), K.spec_uniform(5, 64, 4, K.SPEC_ACCEPT, 4),
                  K.spec_uniform(5, 64, 3, K.SPEC_DRAFT, 4), K.spec_uniform(5, 64, 3, K.SPEC_DRAW, 4)):
        assert not torch.equal(a, other)
    assert bool(((a >= 0) & (a < 1)).all()) and torch.equal((a * 2 ** 24).frac(), torch.zeros_like(a))   # 24 bits
    u = K.spec_uniform(9, 8192, 1, K.SPEC_DRAW, 8).double()
    assert abs(u.mean().item() - 0.5) < 5 / np.sqrt(12 * u.numel())


def _models():
    from test_assisted_gpu import _pair, _prompt
    student, teacher = _pair()
    return student, teacher, _prompt()


def test_generate_speculative_sampling():
    """generate(..., speculative_sampling=True) on the tiny pair: seed-reproducible, seeds differ, top_k = 1 equals greedy assisted under
    test_assisted_gpu's tie rule, consistent counters, per-row EOS and max_new_tokens honoured mid-round, unsupported arguments raise."""
    from test_assisted_gpu import NEW, _greedy_with_gaps
    from llavamod.generation import AssistedOutput
    student, teacher, pr = _models()
    kw = dict(assistant_model=student, speculative_sampling=True, num_assistant_tokens=3)
    a = teacher.generate(**pr, max_new_tokens=12, temperature=1.5, top_p=0.95, seed=5, return_dict_in_generate=True, **kw)
    assert isinstance(a, AssistedOutput) and a.sequences.shape == (pr["input_ids"].shape[0], 12) and a.sequences.dtype == torch.int64
    assert a.num_target_forwards == 1 + a.num_rounds and a.num_rounds >= 1
    assert bool((a.num_accepted <= 3 * a.num_rounds).all()) and bool((a.num_accepted >= 0).all())
    b = teacher.generate(**pr, max_new_tokens=12, temperature=1.5, top_p=0.95, seed=5, **kw)
    assert torch.equal(a.sequences, b)
    c = teacher.generate(**pr, max_new_tokens=12, temperature=1.5, top_p=0.95, seed=6, **kw)
    assert not torch.equal(b, c)
    # top_k = 1: both warped distributions are point masses on the arg-max: greedy assisted decoding
    greedy = teacher.generate(**pr, max_new_tokens=NEW, assistant_model=student, num_assistant_tokens=3)
    top1 = teacher.generate(**pr, max_new_tokens=NEW, top_k=1, seed=1, return_dict_in_generate=True, **kw)
    _, safe = _greedy_with_gaps(teacher, pr, NEW)
    for r in range(greedy.shape[0]):
        n = int(safe[r])
        assert n >= 6, (r, n)
        assert torch.equal(top1.sequences[r, :n], greedy[r, :n]), (r, top1.sequences[r], greedy[r])
    assert top1.num_target_forwards == 1 + top1.num_rounds and bool((top1.num_accepted <= 3 * top1.num_rounds).all())
    # self-drafting with q == p accepts every draft: rounds = ceil((n - 1) / (k + 1))
    s = teacher.generate(**pr, max_new_tokens=9, temperature=1.0, seed=3, assistant_model=teacher, speculative_sampling=True,
                         num_assistant_tokens=3, return_dict_in_generate=True)
    assert s.num_rounds <= 4 and int(s.num_accepted.min()) >= 3, (s.num_rounds, s.num_accepted)
    # EOS mid-round and max_new_tokens mid-round: the same seed draws the same tokens up to the cut
    eos = int(a.sequences[0, 4])
    e = teacher.generate(**pr, max_new_tokens=12, temperature=1.5, top_p=0.95, seed=5, eos_token_id=eos, pad_token_id=1, **kw)
    for r in range(e.shape[0]):
        hit = (a.sequences[r] == eos).nonzero()
        cut = int(hit[0]) + 1 if hit.numel() else 12
        assert torch.equal(e[r, :min(cut, e.shape[1])], a.sequences[r, :min(cut, e.shape[1])]), (r, e[r], a.sequences[r])
        assert bool((e[r, cut:] == 1).all()), (r, e[r])
    m = teacher.generate(**pr, max_new_tokens=6, temperature=1.5, top_p=0.95, seed=5, **kw)          # 6 = 1 + 4 + 1: cut inside round 2
    assert m.shape[1] == 6 and torch.equal(m, a.sequences[:, :6])
    for bad in (dict(stop_sequences=[[1, 2]]), dict(repetition_penalty=1.3), dict(no_repeat_ngram_size=2), dict(bad_words_ids=[[4]]),
                dict(suppress_tokens=[4]), dict(min_new_tokens=2)):
        with pytest.raises(ValueError, match="out of scope"):
            teacher.generate(**pr, max_new_tokens=4, **kw, **bad)
    with pytest.raises(ValueError, match="num_beams"):
        teacher.generate(**pr, max_new_tokens=4, num_beams=2, **kw)
    with pytest.raises(ValueError, match="assistant_model"):
        teacher.generate(**pr, max_new_tokens=4, speculative_sampling=True)
    with pytest.raises(ValueError, match="greedy"):
        teacher.generate(**pr, max_new_tokens=4, assistant_model=student, do_sample=True)
    first = teacher.generate(**pr, max_new_tokens=2, return_dict_in_generate=True)
    with pytest.raises(ValueError, match="past_key_values"):
        teacher.generate(input_ids=first.sequences[:, -1:], past_key_values=first.past_key_values, max_new_tokens=2, **kw)
