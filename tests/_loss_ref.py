"""fp64 restatement of the loss-head kernels (csrc/loss.hip) for kernel tests at full vocabulary.  TEST INFRASTRUCTURE ONLY.

The oracle (oracle/losses.py) materialises fp32 [B, S, V] probabilities; at 151936 columns and thousands of rows that is many
gigabytes, and fp32 is what the kernels are measured against.  This module computes the same quantities in fp64 from the same
bf16 / fp32 inputs, row-wise in chunks so that fp64 scratch stays bounded:

* rowloss_fwd's stats: lse over the full row [0, Vs), over the aligned slice [0, Va), the teacher's lse over [0, Va), the
  mimic term x_kd = sum_v m_v p_v logp_v with the reference's isinf(logp) mask m, the finite mass fm = sum_v m_v p_v, CE and
  s[label] (label < 0 or >= Vs: CE = 0, the kernel's documented contract);
* rowloss_bwd's gradient by fp64 autograd of sum_r (-ckd_r x_r + cce_r ce_r);
* segment sums, dpo_loss (by fp64 autograd of oracle.losses.dpo_loss), masked softmax / log-softmax, rowdot_masked, argmax.

Every function also returns the natural scale of each output (the magnitude fp32 rounding errors are relative to), which the
GPU tests use for their bounds.  Runs on whatever device the inputs live on.  tests/test_loss_ref_cpu.py checks it against
the oracle."""
import torch

from oracle import losses as OL

F64 = torch.float64
NEG_INF = float("-inf")


def _chunks(R, V, budget=1 << 26):
    """Row ranges of at most `budget` fp64 elements each (512 MB per [rows, V] temporary)."""
    step = max(1, budget // max(V, 1))
    for lo in range(0, R, step):
        yield lo, min(R, lo + step)


def rowloss_stats(s, Vs, t=None, Va=None, label=None):
    """What lmod_rowloss_fwd computes, per row, in fp64.  s [R, >= Vs] (bf16, strided rows fine), t [R, >= Va] or None,
    label [R] int or None.  Returns a dict of [R] fp64 tensors: lse_f, lse_a, lse_t, x_kd, fm, ce, s_label, and the scales
    x_scale = sum_v m p |s| + |lse_a| fm (x_kd's terms before they cancel) and lse_scale = 1 + max|s| (lse_f / lse_a)."""
    R = s.shape[0]
    Va = Vs if Va is None else Va
    out = {k: torch.zeros(R, dtype=F64, device=s.device) for k in
           ("lse_f", "lse_a", "lse_t", "x_kd", "fm", "ce", "s_label", "x_scale", "lse_scale", "lse_t_scale")}
    out["fm"].fill_(1.0)
    for lo, hi in _chunks(R, Vs):
        sf = s[lo:hi, :Vs].double()
        sa = sf[:, :Va]
        out["lse_f"][lo:hi] = torch.logsumexp(sf, -1)
        lse_a = torch.logsumexp(sa, -1)
        out["lse_a"][lo:hi] = lse_a
        out["lse_scale"][lo:hi] = 1.0 + sf.abs().masked_fill(torch.isinf(sf), 0).amax(-1)
        if t is not None:
            ta = t[lo:hi, :Va].double()
            lse_t = torch.logsumexp(ta, -1)
            out["lse_t"][lo:hi] = lse_t
            out["lse_t_scale"][lo:hi] = 1.0 + ta.abs().masked_fill(torch.isinf(ta), 0).amax(-1)
            p = torch.exp(ta - lse_t[:, None])
            logp = sa - lse_a[:, None]
            m = ~torch.isinf(logp)
            pm = torch.where(m, p, torch.zeros((), dtype=F64, device=s.device))
            out["x_kd"][lo:hi] = torch.where(m, p * logp, torch.zeros((), dtype=F64, device=s.device)).sum(-1)
            fm = pm.sum(-1)
            out["fm"][lo:hi] = fm
            out["x_scale"][lo:hi] = (pm * sa.abs().masked_fill(~m, 0)).sum(-1) + lse_a.abs() * fm
        del sf, sa
    if label is not None:
        lb = label.long()
        ok = (lb >= 0) & (lb < Vs)
        rows = torch.nonzero(ok).squeeze(1)
        sl = s[rows, lb[rows]].double()
        out["s_label"][rows] = sl
        out["ce"][rows] = out["lse_f"][rows] - sl
    return out


def rowloss_grad(s, Vs, t, Va, label, kd_w, ce_w, seg_id, kd_scale, ce_scale):
    """fp64 d/ds of sum_r (-ckd_r x_kd[r] + cce_r ce[r]), ckd = kd_w[r] kd_scale[seg_id[r]], cce = ce_w[r] ce_scale[seg_id[r]]
    (None weights / scales: that term is absent; seg_id None: segment 0) -- what lmod_rowloss_bwd writes.  Returns
    (grad [R, Vs] fp64, scale [R, Vs] fp64 = |ckd| (q_a + p) + |cce| (q_full + [v == label]), lse [R] = max(|lse_f|, |lse_a|))."""
    R = s.shape[0]
    dev = s.device
    sg = seg_id.long() if seg_id is not None else torch.zeros(R, dtype=torch.long, device=dev)
    ckd = (kd_w.double() * kd_scale.double()[sg]) if (t is not None and kd_w is not None and kd_scale is not None) else None
    cce = (ce_w.double() * ce_scale.double()[sg]) if (ce_w is not None and ce_scale is not None) else None
    lb = label.long() if label is not None else torch.full((R,), -1, dtype=torch.long, device=dev)
    grad = torch.zeros(R, Vs, dtype=F64, device=dev)
    scale = torch.zeros(R, Vs, dtype=F64, device=dev)
    lse = torch.zeros(R, dtype=F64, device=dev)
    for lo, hi in _chunks(R, Vs, budget=1 << 24):
        x = s[lo:hi, :Vs].double().requires_grad_(True)
        lse_f = torch.logsumexp(x, -1)
        obj = x.new_zeros(())
        sc = torch.zeros(hi - lo, Vs, dtype=F64, device=dev)
        lse[lo:hi] = lse_f.detach().abs()
        if ckd is not None:
            lp = torch.log_softmax(x[:, :Va], -1)
            p = torch.softmax(t[lo:hi, :Va].double(), -1)
            xk = torch.masked_fill(p * lp, torch.isinf(lp), 0).sum(-1)        # oracle.losses.compute_align_loss's mask
            obj = obj - (ckd[lo:hi] * xk).sum()
            sc[:, :Va] += ckd[lo:hi, None].abs() * (lp.detach().exp() + p)
            lse[lo:hi] = torch.maximum(lse[lo:hi], torch.logsumexp(x[:, :Va].detach(), -1).abs())
        if cce is not None:
            b = lb[lo:hi]
            ok = (b >= 0) & (b < Vs)
            sl = x.gather(1, b.clamp(0, Vs - 1)[:, None]).squeeze(1)
            ce = torch.where(ok, lse_f - sl, torch.zeros((), dtype=F64, device=dev))
            obj = obj + (cce[lo:hi] * ce).sum()
            hot = torch.zeros(hi - lo, Vs, dtype=F64, device=dev)
            hot[torch.nonzero(ok).squeeze(1), b[ok]] = 1.0
            sc += cce[lo:hi, None].abs() * ((x.detach() - lse_f.detach()[:, None]).exp() + hot)
        if obj.requires_grad:
            obj.backward()
            grad[lo:hi] = x.grad
        scale[lo:hi] = sc
    return grad, scale, lse


def segment_sums(val, w, off):
    """out_sum[b] = sum_{r in seg b} w[r] val[r], out_w[b] = sum w[r], scale[b] = sum |w val| (fp64).  val [N] (one column)."""
    v = val.double()
    ww = torch.ones_like(v) if w is None else w.double()
    o = off.long().tolist()
    s, sw, sc = [], [], []
    ca = torch.cat([v.new_zeros(1), torch.cumsum((v * ww).abs(), 0)])
    cw = torch.cat([v.new_zeros(1), torch.cumsum(ww, 0)])
    for b in range(len(o) - 1):
        lo, hi = o[b], o[b + 1]
        # direct sums (not cumsum differences) for the values: cumsum differences cancel at the size of the prefix
        s.append((v[lo:hi] * ww[lo:hi]).sum() if hi > lo else v.new_zeros(()))
        sc.append(ca[hi] - ca[lo])
        sw.append(cw[hi] - cw[lo])
    return torch.stack(s), torch.stack(sw), torch.stack(sc)


def dpo(pc, pr, rc, rr, beta, label_smoothing, loss_type):
    """oracle.losses.dpo_loss in fp64 from the same fp32 inputs, with d(mean(losses)) / d(pc, pr) by fp64 autograd.  beta and
    label_smoothing are rounded to fp32 first (the kernel's arguments are floats).  Returns losses, chosen / rejected rewards,
    d_pc, d_pr."""
    beta = float(torch.tensor(beta, dtype=torch.float32))
    ls = float(torch.tensor(label_smoothing, dtype=torch.float32))
    a = pc.double().requires_grad_(True)
    b = pr.double().requires_grad_(True)
    losses, cr, rj = OL.dpo_loss(a, b, rc.double(), rr.double(), beta, ls, loss_type)
    losses.mean().backward()
    return losses.detach(), cr, rj, a.grad, b.grad


def softmax(x, Va, log):
    """softmax / log_softmax of x[:, :Va] in fp64 (what lmod_row_softmax_f32 writes; -inf entries give 0 / -inf)."""
    xa = x[:, :Va].double()
    return torch.log_softmax(xa, -1) if log else torch.softmax(xa, -1)


def rowdot_masked(p, lp):
    """x[r] = sum_v (isinf(lp) ? 0 : p lp) in fp64, and its scale sum |p lp| over the unmasked entries."""
    pd, ld = p.double(), lp.double()
    m = torch.isinf(ld)
    prod = torch.where(m, torch.zeros((), dtype=F64, device=p.device), pd * ld)
    return prod.sum(-1), prod.abs().sum(-1)


def argmax(x):
    """lmod_row_argmax_bf16's contract: the first maximum wins, NaN never wins, a row without a value > -inf gives 0."""
    v = x.float()
    v = torch.where(torch.isnan(v), torch.full_like(v, NEG_INF), v)
    m = v.amax(-1, keepdim=True)
    first = (v == m).int().argmax(-1)                # argmax of a 0/1 row: torch returns the first maximal index
    return torch.where(m.squeeze(-1) > NEG_INF, first, torch.zeros_like(first))
