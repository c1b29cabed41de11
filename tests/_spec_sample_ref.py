"""fp64 reference of speculative sampling (lmod_spec_sample_bf16's contract, include/lmod_hip.h), written from the contract on top
of _sample_ref.py: the warped distributions, the accept ratio, the token-order residual CDF and the full block rule with Python
loops.  Also the test inputs (CPU generators, fixed seeds: the CPU and the GPU tests see the same numbers) and a plain torch fp32
evaluation of the same quantities: the noise-floor side of the tolerances and the stand-in with which the CPU tests confirm that the
chosen inputs keep the undecidable bands small.  TEST INFRASTRUCTURE ONLY."""
import numpy as np
import torch

import _sample_ref as SR

BF = torch.bfloat16
NSTRATA = 4096
U_MAX = float(np.nextafter(np.float32(1), np.float32(0)))
SHAPES = [(1003, 1008), (151936, 151936)]
FILTERS = [(None, None), (50, None), (None, 0.7), (None, 0.9), (50, 0.7), (50, 0.9)]
TEMPS = (0.2, 1.0, 1.5)
SCALES = (3.0, 8.0)


def grid(V):
    """(T, top_k, top_p) cases of a vocabulary size: the sampling test's full grid at the small V, a corner of it at the large one."""
    if V > 100000:
        return [(T, k, p) for T in (0.2, 1.0) for k, p in ((None, None), (50, 0.9))]
    return [(T, k, p) for T in TEMPS for k, p in FILTERS]


def strata():
    u = (torch.arange(NSTRATA, dtype=torch.float64) + 0.5) / NSTRATA
    return torch.cat([u, torch.tensor([0.0, U_MAX], dtype=torch.float64)]).to(torch.float32)      # every value is exact in fp32


def make_logits(V, ld, rows, s, seed):
    """p = s * randn, q = bf16(p + 0.5 * randn): (p [rows, V], q [rows, V]) bf16 views of [rows, ld] buffers."""
    g = torch.Generator().manual_seed(seed)
    p = (s * torch.randn(rows, ld, generator=g)).to(BF)
    q = (p.float() + 0.5 * torch.randn(rows, ld, generator=g)).to(BF)
    return p[:, :V], q[:, :V]


def warped(logits, T, k, p, keep=None, dtype=torch.float64):
    """The warped distribution [R, V] of bf16 rows: softmax of logit / T over the kept set (`keep`: a kept set to use instead of the
    reference's own).  dtype fp32: the plain torch fp32 evaluation."""
    keep = SR.keep_mask(logits, T, k, p) if keep is None else keep
    t = max(float(np.float32(T)), 1e-6)
    x = logits.to(dtype) / t
    x = torch.where(keep, x, torch.full_like(x, SR.NEG_INF))
    return torch.softmax(x, -1)


def accept_prob(p, q, d):
    """min(1, p(d) / q(d)) per row; 0 where p(d) = 0 (also when q(d) = 0)."""
    pd, qd = p.gather(1, d[:, None])[:, 0], q.gather(1, d[:, None])[:, 0]
    return torch.where(pd <= 0, torch.zeros_like(pd), torch.where(pd >= qd, torch.ones_like(pd), pd / qd.clamp_min(1e-300)))


def residual(p, q):
    """(r_hat [R, V], cdf_lo, cdf_hi): the normalised residual max(0, p - q) (p itself where that is zero everywhere) and its
    token-order CDF; token t owns [cdf_lo[t], cdf_hi[t])."""
    r = (p - q).clamp_min(0)
    r = torch.where(r.sum(-1, keepdim=True) > 0, r, p)
    hi = r.cumsum(-1)
    tot = hi[:, -1:].clamp_min(1e-300)
    return r / tot, (hi - r) / tot, hi / tot


def draw(r, u):
    """Inverse CDF in token-id order over weights r [V]: the first token whose cumulative mass exceeds u * total (the last token with
    mass if rounding runs past the end)."""
    r = torch.as_tensor(r, dtype=torch.float64)
    cum = r.cumsum(0)
    t = int(torch.searchsorted(cum, (u * cum[-1]).reshape(1), right=True))
    pos = (r > 0).nonzero()
    return min(t, int(pos[-1])) if pos.numel() else 0


def block_bruteforce(p, q, draft, u_acc, u_draw, done, eos, pad, lens_target, lens_draft):
    """lmod_spec_sample_bf16's rule with Python lists and loops on warped distributions p [B][k+1][V], q [B][k][V].  Returns (block rows
    [B][k+5], next_token [B], done [B], lens_target [B], lens_draft [B])."""
    B, k = len(draft), len(draft[0])
    rows, nxt, dn, lt, ld = [], [], [], [], []
    for b in range(B):
        n = 0
        if not done[b]:
            while n < k:
                d = draft[b][n]
                if not (float(u_acc[b][n]) * float(q[b][n][d]) < float(p[b][n][d])):
                    break
                n += 1
        tok = 0
        if not done[b]:
            pn = torch.as_tensor(p[b][n], dtype=torch.float64)
            r = (pn - torch.as_tensor(q[b][n], dtype=torch.float64)).clamp_min(0) if n < k else pn
            tok = draw(r if float(r.sum()) > 0 else pn, float(u_draw[b]))
        emitted = [] if done[b] else list(draft[b][:n]) + [tok]
        fin = bool(done[b])
        if eos is not None and eos in emitted:
            emitted = emitted[:emitted.index(eos) + 1]
            fin = True
        nx = pad if fin else tok
        rows.append(emitted + [pad] * (k + 1 - len(emitted)) + [n, len(emitted), nx, int(fin)])
        nxt.append(nx), dn.append(int(fin)), lt.append(lens_target[b] - k + n), ld.append(lens_draft[b] - k + min(n + 1, k))
    return rows, nxt, dn, lt, ld


def marginal(p, q):
    """The law of the token a one-position round emits, analytically: sum_d q(d) min(1, p(d)/q(d)) [x = d] + (1 - that sum) r_hat(x)."""
    acc = torch.minimum(p, q)                                   # q(d) * min(1, p(d) / q(d))
    r_hat, _, _ = residual(p[None], q[None])
    return acc + (1.0 - acc.sum()) * r_hat[0]


# ---- the accept test's inputs and bands --------------------------------------------------------------------------------------
BAN = 7                       # a token whose p logit is -inf in every case: outside the target's kept set whatever the filter


CASE_SEED = {(1003, 3.0): 1, (1003, 8.0): 12}        # the first seeds at which every grid case has a total variation >= 0.05


def accept_case(V, ld, s, seed=None):
    """One (p row, bonus row, q row) triple for the accept / residual tests: p [2, V], q [1, V]; p[0, BAN] = -inf."""
    seed = CASE_SEED.get((V, s), 0) if seed is None else seed
    p, q = make_logits(V, ld, 2, s, 1000 + V % 977 + int(s) + seed)
    p[0, BAN] = float("-inf")
    return p, q[:1]


def draft_kinds(p, q, T, k, tp, keep_p=None, keep_q=None):
    """The four draft tokens of the accept test from the fp64 distributions: drawn from q (u = 0.37), the token with the largest
    p - q, BAN (outside p's kept set) and the arg-max of q."""
    P, Q = warped(p[:1], T, k, tp, keep_p), warped(q, T, k, tp, keep_q)
    _, _, hi = residual(Q, torch.zeros_like(Q))
    from_q = int(torch.searchsorted(hi[0].contiguous(), torch.tensor([0.37], dtype=torch.float64), right=True).clamp(max=p.shape[1] - 1))
    return [from_q, int((P - Q)[0].argmax()), BAN, int(Q[0].argmax())]


def accept_band(p, q, d, T, k, tp, keep_p=None, keep_q=None):
    """(ratio fp64, the same in plain torch fp32, floor, delta) of the accept test at draft token d: ratio = min(1, p(d)/q(d));
    floor = |fp32 - fp64|; delta = 2 * floor, floored at 1e-6 (test_sample_gpu's rule)."""
    dd = torch.tensor([d])
    r64 = accept_prob(warped(p[:1], T, k, tp, keep_p), warped(q, T, k, tp, keep_q), dd)[0].item()
    r32 = accept_prob(warped(p[:1], T, k, tp, keep_p, torch.float32), warped(q, T, k, tp, keep_q, torch.float32), dd)[0].item()
    floor = abs(r32 - r64)
    return r64, r32, floor, max(2.0 * floor, 1e-6)


def residual_band(p, q, T, k, tp, keep_p=None, keep_q=None):
    """(r_hat, cdf_lo, cdf_hi fp64 [V], floor, delta, total variation) of the residual at position 0: floor = max |cdf32 - cdf64| with
    the fp32 CDF a plain torch evaluation (softmax, subtract, clamp, cumsum, divide)."""
    P, Q = warped(p[:1], T, k, tp, keep_p), warped(q, T, k, tp, keep_q)
    r_hat, lo, hi = residual(P, Q)
    P32, Q32 = warped(p[:1], T, k, tp, keep_p, torch.float32), warped(q, T, k, tp, keep_q, torch.float32)
    _, _, hi32 = residual(P32, Q32)
    floor = (hi32.double() - hi).abs().max().item()
    return P[0], Q[0], lo[0], hi[0], floor, max(2.0 * floor, 1e-6), 0.5 * (P - Q).abs().sum().item()


# ---- the block test's inputs and reference -----------------------------------------------------------------------------------
BLOCK_CASES = [(1.0, None, None), (1.0, 50, 0.9)]
BLOCK_KS = (4, 15)


def block_trials(V):
    """Trials per (k, case).  One at the large V: without a filter a token owns about 1 / V of the CDF there, not much more than the
    draw's delta, so a trial's draw can sit inside its band; trial 0 has none (checked on the CPU in test_spec_sample_cpu.py)."""
    return 1 if V > 100000 else 4


def block_case(V, ld, k, T, tk, tp, trial):
    """B = 3 samples: p [3*(k+1), V], q [3*k, V] (bf16), drafts drawn from q by the fp64 reference, random 24-bit uniforms (sample 0
    accepts whatever the target keeps: u_acc = 0), sample 2 done, an EOS planted at sample 0's second draft, lens."""
    B = 3
    g = torch.Generator().manual_seed(7000 + 13 * trial + k + V % 911)
    p, q = make_logits(V, ld, B * (k + 1), 3.0 if trial % 2 else 8.0, 500 + 17 * trial + k + V % 911)
    q = q.view(B, k + 1, V)[:, :k].reshape(B * k, V)
    u24 = lambda *shape: (torch.randint(0, 1 << 24, shape, generator=g).float() / float(1 << 24))
    u_d, u_acc, u_draw = u24(B * k), u24(B, k), u24(B)
    u_acc[0] = 0.0
    draft = SR.draw(q, u_d, T, tk, tp).view(B, k).to(torch.int32)
    done = torch.tensor([0, 0, 1], dtype=torch.int32)
    lt = torch.tensor([40, 33, 51], dtype=torch.int32) + k + 1
    ld_ = torch.tensor([40, 33, 51], dtype=torch.int32) + k
    return dict(p=p, q=q, draft=draft, u_acc=u_acc, u_draw=u_draw, done=done, eos=int(draft[0, 1]), pad=3, lt=lt, ld=ld_)


def block_reference(c, k, T, tk, tp, keep_p=None, keep_q=None):
    """The fp64 block of a block_case and, per sample, the first emitted position whose decision lies inside its band (k + 2: none):
    an accept test with |u - ratio| < delta, or the draw with u within delta of an end of the drawn token's CDF interval; every delta
    is 2 * |plain torch fp32 - fp64| of that quantity, floored at 1e-6."""
    B, V = 3, c["p"].shape[1]
    P = warped(c["p"], T, tk, tp, keep_p).view(B, k + 1, V)
    Q = warped(c["q"], T, tk, tp, keep_q).view(B, k, V)
    P32 = warped(c["p"], T, tk, tp, keep_p, torch.float32).view(B, k + 1, V)
    Q32 = warped(c["q"], T, tk, tp, keep_q, torch.float32).view(B, k, V)
    rows, nxt, dn, lt, ld = block_bruteforce(P, Q, c["draft"].tolist(), c["u_acc"].double().tolist(), c["u_draw"].double().tolist(),
                                             c["done"].tolist(), c["eos"], c["pad"], c["lt"].tolist(), c["ld"].tolist())
    band = []
    for b in range(B):
        n, pos = rows[b][k + 1], k + 2
        if not c["done"][b]:
            for i in range(min(n + 1, k)):
                d = c["draft"][b, i].long().view(1)
                r64 = accept_prob(P[b, i:i + 1], Q[b, i:i + 1], d).item()
                r32 = accept_prob(P32[b, i:i + 1], Q32[b, i:i + 1], d).item()
                if abs(float(c["u_acc"][b, i]) - r64) < max(2 * abs(r32 - r64), 1e-6) and 0 < r64 < 1:
                    pos = i
                    break
            if pos == k + 2:
                qn = Q[b, n:n + 1] if n < k else torch.zeros_like(P[b, :1])
                qn32 = Q32[b, n:n + 1] if n < k else torch.zeros_like(P32[b, :1])
                _, lo, hi = residual(P[b, n:n + 1], qn)
                _, _, hi32 = residual(P32[b, n:n + 1], qn32)
                delta = max(2 * (hi32.double() - hi).abs().max().item(), 1e-6)
                u = float(c["u_draw"][b])
                res = (P[b, n] - Q[b, n]).clamp_min(0) if n < k else P[b, n]
                t = draw(res if float(res.sum()) > 0 else P[b, n], u)
                if u - lo[0, t].item() < delta or hi[0, t].item() - u < delta:
                    pos = n
        band.append(pos)
    return rows, nxt, dn, lt, ld, band
