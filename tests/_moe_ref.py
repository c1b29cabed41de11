"""Sparse restatement of oracle/moe.py's top1gating / top2gating for kernel tests at step sizes.  TEST INFRASTRUCTURE ONLY.

The dense oracle builds [S, E, C] one-hot tensors: at the step's T = 32768 tokens that is gigabytes.  This module restates the
same gating from index maps, in two parts:

* integer decisions (picks, capacity positions, kept masks, slots, slot_token, exp_counts) computed the way the oracle does:
  argmax of the fp32 softmax (first maximum wins), one-hot cumsum in token order, second picks queued behind all first picks;
* continuous quantities (gates, combine weights, l_aux, gate sums) in fp64 from those decisions, with the top-2 denominator
  clamped at the fp32 eps as in DeepSpeed (its gates are fp32), and gradients by fp64 autograd of the sparse objective
  sum_t (u1 w1 + u2 w2) + d_laux l_aux, so the clamp's gradient comes from torch.

Runs on whatever device the inputs live on.  tests/test_moe_ref_cpu.py checks it against the dense oracle."""
import torch
import torch.nn.functional as F

EPS32 = torch.finfo(torch.float32).eps      # DeepSpeed's gates are fp32: the clamp is at the fp32 eps, also in fp64 here


def _queue_pos(idx, E):
    """cumsum(one_hot(idx), 0) - 1 at each token's own expert: its position in that expert's token-order queue."""
    m = F.one_hot(idx, E)
    return (torch.cumsum(m, 0) - 1).gather(1, idx[:, None]).squeeze(1), m.sum(0)


def top2_maps(logits, C, noise=None):
    """Integer decisions of top2gating with capacity C.  logits [T, E] fp32; noise [T, E] (added for the 2nd pick) or None."""
    T, E = logits.shape
    gates = F.softmax(logits.float(), dim=1)
    idx1 = torch.argmax(gates, dim=1)
    lw = logits.float() if noise is None else logits.float() + noise.float()
    idx2 = torch.argmax(lw.masked_fill(F.one_hot(idx1, E).bool(), float("-inf")), dim=1)
    loc1, cnt1 = _queue_pos(idx1, E)
    loc2, cnt2 = _queue_pos(idx2, E)
    loc2 = loc2 + cnt1[idx2]                                        # second picks queue behind ALL first picks
    return _finish(dict(k=2, T=T, E=E, C=C, idx1=idx1, idx2=idx2, loc1=loc1, loc2=loc2, kept1=loc1 < C, kept2=loc2 < C,
                        exp_counts=cnt1))


def top1_maps(logits, C, rts_noise=None):
    """Integer decisions of top1gating (drop_tokens=True).  rts_noise [T, E] uniform priorities (use_rts=True): per expert the
    C tokens of largest priority keep their slot (ties: earlier token first), survivors numbered in token order; None: the
    first C tokens in token order."""
    T, E = logits.shape
    idx1 = torch.argmax(F.softmax(logits.float(), dim=1), dim=1)
    loc1, cnt1 = _queue_pos(idx1, E)
    if rts_noise is None:
        kept1 = loc1 < C
    else:
        prio = rts_noise.float().gather(1, idx1[:, None]).squeeze(1)
        order = torch.sort(prio, descending=True, stable=True).indices       # stable: ties stay in token order
        rank_sorted, _ = _queue_pos(idx1[order], E)
        rank = torch.empty_like(rank_sorted)
        rank[order] = rank_sorted
        kept1 = rank < C
        loc1 = torch.cumsum(F.one_hot(idx1, E) * kept1[:, None], 0).gather(1, idx1[:, None]).squeeze(1) - 1
    return _finish(dict(k=1, T=T, E=E, C=C, idx1=idx1, idx2=None, loc1=loc1, loc2=None, kept1=kept1, kept2=None,
                        exp_counts=cnt1))


def _finish(m):
    """Slot maps from the picks and positions: slot = expert * C + position for a kept pick, -1 otherwise."""
    E, C, T = m["E"], m["C"], m["T"]
    dev = m["idx1"].device
    m["slot_token"] = torch.full((E * C,), -1, dtype=torch.long, device=dev)
    tok = torch.arange(T, device=dev)
    for j in (1, 2)[:m["k"]]:
        kept = m[f"kept{j}"]
        slot = torch.where(kept, m[f"idx{j}"] * C + m[f"loc{j}"], torch.full_like(tok, -1))
        m[f"slot{j}"] = slot
        m["slot_token"][slot[kept]] = tok[kept]
    if m["k"] == 1:
        m["slot2"] = None
    m["slots_used"] = (m["slot_token"].view(E, C) >= 0).sum(1)
    return m


def weights(m, logits):
    """Continuous part in fp64 from the integer decisions `m`: returns dict(gates, w1, w2, slot_w, l_aux, gate_sum).
    Differentiable in `logits` (pass an fp64 leaf with requires_grad to take gradients)."""
    T, E, C = m["T"], m["E"], m["C"]
    gates = F.softmax(logits.double(), dim=1)
    g1 = gates.gather(1, m["idx1"][:, None]).squeeze(1) * m["kept1"]
    if m["k"] == 2:
        g2 = gates.gather(1, m["idx2"][:, None]).squeeze(1) * m["kept2"]
        den = torch.clamp(g1 + g2, min=EPS32)
        w1, w2 = g1 / den, g2 / den
    else:
        w1, w2 = g1, None
    gate_sum = gates.sum(0)
    # top2gating: mean(me * ce) * E * E ; top1gating: sum(me * ce) * E  — both E * sum_e me_e ce_e
    l_aux = (gate_sum / T * m["exp_counts"].double() / T).sum() * E
    slot_w = torch.zeros(E * C, dtype=torch.float64, device=gates.device)
    for slot, w in ((m["slot1"], w1), (m["slot2"], w2))[:m["k"]]:
        kept = slot >= 0
        slot_w = slot_w.index_put((slot[kept],), w[kept])
    return dict(gates=gates, w1=w1, w2=w2, slot_w=slot_w, l_aux=l_aux, gate_sum=gate_sum)


def gate_grad(m, logits, u1, u2, d_laux):
    """fp64 autograd of sum_t (u1 w1 + u2 w2) + d_laux * l_aux with respect to the logits.  Returns (dlogits, scale): scale is
    each element's natural magnitude g_e (|dg_e| + sum_e' g_e' |dg_e'|), where |dg| sums the absolute values of the terms an
    fp32 backward adds at the softmax output (|u_j| / den and the denominator's (|u1| g1 + |u2| g2) / den^2, which cancel when
    both picks are kept; the l_aux term) — the size at which an fp32 implementation rounds."""
    lg = logits.detach().double().requires_grad_(True)
    r = weights(m, lg)
    obj = (u1.double() * r["w1"]).sum() + float(d_laux) * r["l_aux"]
    if m["k"] == 2:
        obj = obj + (u2.double() * r["w2"]).sum()
    obj.backward()
    T, E = m["T"], m["E"]
    with torch.no_grad():
        gates = r["gates"]
        a = torch.zeros(T, E, dtype=torch.float64, device=gates.device)
        a += abs(float(d_laux)) * E * m["exp_counts"].double() / T / T
        g1 = gates.gather(1, m["idx1"][:, None]).squeeze(1) * m["kept1"]
        if m["k"] == 2:
            g2 = gates.gather(1, m["idx2"][:, None]).squeeze(1) * m["kept2"]
            den = torch.clamp(g1 + g2, min=EPS32)
            cross = (u1.double().abs() * g1 + u2.double().abs() * g2) / den ** 2
            a.scatter_add_(1, m["idx1"][:, None], (m["kept1"] * (u1.double().abs() / den + cross))[:, None])
            a.scatter_add_(1, m["idx2"][:, None], (m["kept2"] * (u2.double().abs() / den + cross))[:, None])
        else:
            a.scatter_add_(1, m["idx1"][:, None], (m["kept1"] * u1.double().abs())[:, None])
        scale = gates * (a + (gates * a).sum(1, keepdim=True))
    return lg.grad, scale
