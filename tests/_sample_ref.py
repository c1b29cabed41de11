"""fp64 torch reference of the sampling warpers and the draw (lmod_sample_bf16's contract, include/lmod_hip.h), written from the
contract and not from the kernel: it sorts, the kernel does not.

Works on the exact bf16 values of a batch of rows [R, V]:
  x = logit / max(T, 1e-6) in fp64 (T rounded to fp32 first: the C ABI takes a float, so that is the value the kernel is given);
  top-k (0 < k < V): keep x >= the k-th largest x (every tie at that value);
  top-p (p < 1): stable descending sort of the survivors (equal logits: smaller token id first), softmax over them, the prefix of
    tokens whose mass BEFORE them is <= p (never empty: the first token always stays), cutoff = the logit of the prefix's last
    token, keep x >= cutoff (a threshold set: ties at the cutoff all stay);
  draw: weights exp(x - max) of the kept tokens in token-id order, cumulative sum, the first token whose cumulative mass exceeds
    u * kept_mass.
"""
import numpy as np
import torch

NEG_INF = float("-inf")


def scaled(logits, temperature):
    t = max(float(np.float32(temperature)), 1e-6)
    return logits.double() / t


def keep_mask(logits, temperature=1.0, top_k=None, top_p=None):
    """bool [R, V]: the kept set of every row."""
    x = scaled(logits, temperature)
    R, V = x.shape
    keep = torch.ones_like(x, dtype=torch.bool)
    if top_k is not None and 0 < top_k < V:
        kth = torch.topk(x, top_k, dim=-1).values[:, -1:]
        keep &= x >= kth
    if top_p is not None and top_p < 1.0:
        xs = torch.where(keep, x, torch.full_like(x, NEG_INF))
        sv, _ = torch.sort(xs, dim=-1, descending=True, stable=True)
        p = torch.softmax(sv, dim=-1)
        before = p.cumsum(-1) - p
        before[:, 0] = 0.0
        inside = before <= top_p
        inside[:, 0] = True                                   # at least one token
        # `before` does not decrease, so `inside` is a prefix; -inf survivors (weight 0) are never its last token unless the whole
        # row is -inf
        inside &= (sv > NEG_INF) | (torch.arange(V, device=x.device)[None, :] == 0)
        last = inside.sum(-1, keepdim=True) - 1
        keep &= x >= sv.gather(1, last)
    return keep


def cutoff_and_count(logits, temperature=1.0, top_k=None, top_p=None):
    """(cutoff logit [R] fp64: the smallest kept UNSCALED logit, -inf when no filter applies; number of kept tokens [R])."""
    keep = keep_mask(logits, temperature, top_k, top_p)
    V = logits.shape[1]
    n = keep.sum(-1)
    filt = (top_k is not None and 0 < top_k < V) or (top_p is not None and top_p < 1.0)
    lv = logits.double()
    cut = torch.where(keep, lv, torch.full_like(lv, float("inf"))).min(-1).values
    if not filt:
        cut = torch.full_like(cut, NEG_INF)
    return cut, n


def stats(logits, temperature=1.0, top_k=None, top_p=None):
    """(lse of x over all V [R], kept mass / total mass [R]) in fp64; a row without a finite logit: (-inf, 0)."""
    x = scaled(logits, temperature)
    keep = keep_mask(logits, temperature, top_k, top_p)
    m = x.max(-1, keepdim=True).values
    m = torch.where(torch.isfinite(m), m, torch.zeros_like(m))
    w = torch.exp(x - m)
    tot = w.sum(-1)
    kept = torch.where(keep, w, torch.zeros_like(w)).sum(-1)
    lse = torch.where(tot > 0, m.squeeze(-1) + torch.log(tot), torch.full_like(tot, NEG_INF))
    frac = torch.where(tot > 0, kept / tot.clamp_min(1e-300), torch.zeros_like(tot))
    return lse, frac


def kept_cdf(logits, temperature, keep):
    """Token-order CDF of the kept set, normalised: (cdf_lo [R, V], cdf_hi [R, V]) fp64; token t owns [cdf_lo[t], cdf_hi[t])."""
    x = scaled(logits, temperature)
    m = torch.where(keep, x, torch.full_like(x, NEG_INF)).max(-1, keepdim=True).values
    m = torch.where(torch.isfinite(m), m, torch.zeros_like(m))
    w = torch.where(keep, torch.exp(x - m), torch.zeros_like(x))
    hi = w.cumsum(-1)
    tot = hi[:, -1:].clamp_min(1e-300)
    return (hi - w) / tot, hi / tot


def draw(logits, u, temperature=1.0, top_k=None, top_p=None):
    """Tokens int64 [R]: the first kept token whose cumulative kept mass exceeds u * kept_mass (the last kept token if rounding runs
    past the end; 0 for a row without a finite logit)."""
    keep = keep_mask(logits, temperature, top_k, top_p)
    _, hi = kept_cdf(logits, temperature, keep)
    t = torch.searchsorted(hi.contiguous(), u.double()[:, None].contiguous(), right=True).squeeze(-1)
    V = logits.shape[1]
    pos = torch.where(keep & (hi > 0), torch.arange(V, device=logits.device)[None, :], torch.full_like(keep, -1, dtype=torch.long))
    last = pos.max(-1).values
    t = torch.minimum(t, last.clamp_min(0))
    return torch.where(last >= 0, t, torch.zeros_like(t))


def warped_logprob(logits, tokens, temperature=1.0, top_k=None, top_p=None):
    """fp64 [R]: log-probability of `tokens` under the warped distribution (-inf outside the kept set)."""
    x = scaled(logits, temperature)
    keep = keep_mask(logits, temperature, top_k, top_p)
    xk = torch.where(keep, x, torch.full_like(x, NEG_INF))
    return torch.log_softmax(xk, -1).gather(1, tokens.long()[:, None]).squeeze(1)
