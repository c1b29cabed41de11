"""tests/_loss_ref.py (the row-wise fp64 restatement the loss-kernel GPU tests use at full vocabulary) against the oracle
(oracle/losses.py) on the CPU: get_p / get_logp / compute_align_loss / seq_logp / dpo_loss and their autograd gradients,
including -inf student and teacher logits."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle import losses as OL  # noqa: E402
import _loss_ref as R  # noqa: E402


def _logits(Rn, V, seed, scale=3.0):
    """bf16-representable fp32 logits (the kernels read bf16)."""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(Rn, V, generator=g) * scale).to(torch.bfloat16).float()


def _with_inf(s, t, Va):
    """-inf student logits in both slices (column 0, column Va, scattered), -inf teacher logits, rows 0 and 5 left finite."""
    s, t = s.clone(), t.clone()
    s[1, 0] = s[1, 9] = s[2, Va // 2] = float("-inf")
    s[3, Va] = s[3, Va + 3] = float("-inf")          # extra slice only
    t[4, 1] = t[4, Va - 1] = float("-inf")           # teacher only
    s[6, 2] = t[6, 2] = float("-inf")                # both at the same column: 0 * -inf, masked
    s[6, 7] = t[6, 11] = float("-inf")
    return s, t


def _oracle_x(s, t, Va):
    """Per-row mimic term from the oracle's get_p / get_logp / compute_align_loss (one row per call, all tokens distilled)."""
    p = OL.get_p(t[None], Va)
    lp = OL.get_logp(s[None], Va)
    xs = [-OL.compute_align_loss(lp[:, r:r + 1], p[:, r:r + 1], torch.zeros(1, 1), distill_all_tokens=True)
          for r in range(s.shape[0])]
    return torch.stack(xs)


@pytest.mark.parametrize("inf", [False, True])
def test_rowloss_stats_match_oracle(inf):
    Rn, Vs, Va = 7, 72, 64
    s, t = _logits(Rn, Vs, 1), _logits(Rn, Va, 2)
    if inf:
        s, t = _with_inf(s, t, Va)
    label = torch.tensor([0, Va - 1, Va, Vs - 1, -100, 5, Vs], dtype=torch.int32)      # Vs: out of range, CE = 0
    st = R.rowloss_stats(s.to(torch.bfloat16), Vs, t.to(torch.bfloat16), Va, label)
    torch.testing.assert_close(st["x_kd"].float(), _oracle_x(s, t, Va), rtol=2e-6, atol=2e-6)
    torch.testing.assert_close(st["lse_a"].float(), torch.logsumexp(s[:, :Va], -1), rtol=1e-6, atol=1e-6)
    torch.testing.assert_close(st["lse_f"].float(), torch.logsumexp(s, -1), rtol=1e-6, atol=1e-6)
    torch.testing.assert_close(st["lse_t"].float(), torch.logsumexp(t, -1), rtol=1e-6, atol=1e-6)
    p = OL.get_p(t[None], Va)[0]
    fm = torch.where(torch.isinf(s[:, :Va]), torch.zeros(()), p).sum(-1)
    torch.testing.assert_close(st["fm"].float(), fm, rtol=1e-6, atol=1e-7)
    if not inf:
        assert torch.allclose(st["fm"], torch.ones(Rn, dtype=torch.float64), rtol=0, atol=1e-15)
    else:
        assert float(st["fm"][1]) < 1 and float(st["fm"][3]) == pytest.approx(1.0, abs=1e-15)
    # CE / s[label]: the oracle's log_softmax gathered at the label (seq_logp), ignored labels and labels >= Vs give 0
    lsm = F.log_softmax(s, -1)
    for r in range(Rn):
        lb = int(label[r])
        if 0 <= lb < Vs:
            assert float(st["ce"][r]) == pytest.approx(-float(lsm[r, lb]), rel=1e-6, abs=1e-6)
            assert float(st["s_label"][r]) == float(s[r, lb])
        else:
            assert float(st["ce"][r]) == 0.0 and float(st["s_label"][r]) == 0.0


def test_seq_logp_is_minus_ce_sum():
    """seq_logp (DPO per-sample log-prob) = -sum of the per-token CE over the shifted labels: the rows the step feeds the
    row kernel with t = None, Va = Vs."""
    B, S, V = 2, 6, 40
    logits = _logits(B * S, V, 3).view(B, S, V)
    labels = torch.tensor([[-100, 3, 7, -100, 39, 0], [-100, -100, 1, 2, 3, 4]])
    ref = OL.seq_logp(logits, labels)
    rows = logits[:, :-1].reshape(-1, V)
    lab = labels[:, 1:].reshape(-1).to(torch.int32)
    st = R.rowloss_stats(rows.to(torch.bfloat16), V, None, None, lab)
    torch.testing.assert_close((-st["ce"]).view(B, S - 1).sum(-1).float(), ref, rtol=1e-6, atol=1e-5)
    assert bool((st["x_kd"] == 0).all()) and bool((st["fm"] == 1).all())


@pytest.mark.parametrize("inf", [False, True])
def test_rowloss_grad_matches_oracle_autograd(inf):
    """The fp64 gradient of sum_r (-ckd x_kd + cce ce) vs fp32 autograd through the oracle's get_logp / compute_align_loss and a
    log_softmax-gathered CE, with per-segment scales of both signs and zero."""
    Rn, Vs, Va = 7, 72, 64
    s, t = _logits(Rn, Vs, 4), _logits(Rn, Va, 5)
    if inf:
        s, t = _with_inf(s, t, Va)
    label = torch.tensor([0, Va - 1, Va, Vs - 1, -100, 5, 9], dtype=torch.int32)
    kd_w = torch.tensor([1.0, 1, 0.5, 1, 0, 1, 1])
    ce_w = (label >= 0).float()
    seg = torch.tensor([0, 0, 1, 1, 1, 2, 2], dtype=torch.int32)
    kd_scale, ce_scale = torch.tensor([0.37, -1.3, 0.0]), torch.tensor([-0.21, 0.0, 0.9])
    got, scale, _ = R.rowloss_grad(s.to(torch.bfloat16), Vs, t.to(torch.bfloat16), Va, label, kd_w, ce_w, seg, kd_scale, ce_scale)
    sg = s.clone().requires_grad_(True)
    p = OL.get_p(t[None], Va)
    lp = OL.get_logp(sg[None], Va)
    obj = sg.new_zeros(())
    ckd = kd_w * kd_scale[seg.long()]
    cce = ce_w * ce_scale[seg.long()]
    for r in range(Rn):
        x = -OL.compute_align_loss(lp[:, r:r + 1], p[:, r:r + 1], torch.zeros(1, 1), distill_all_tokens=True)
        obj = obj - ckd[r] * x
        lb = int(label[r])
        if 0 <= lb < Vs:
            obj = obj + cce[r] * -F.log_softmax(sg[r], -1)[lb]
    obj.backward()
    assert torch.isfinite(got).all()
    err = (got - sg.grad.double()).abs()
    assert (err <= 2 ** -20 * scale + 1e-12).all(), float((err / scale.clamp_min(1e-300)).max())
    if inf:
        assert float(got[1, 0]) == 0.0 and float(got[1, 9]) == 0.0     # masked column, no CE on it: exactly 0


def test_kd_backward_needs_finite_mass():
    """The repro of the KD backward bug: with -inf student logits in [0, Va) where the teacher has mass, the gradient of
    -x_kd is fm q - m p (m = [s finite], fm = sum m p), not q - p.  The old formula is off at every column of the row."""
    Rn, V = 2, 64
    s, t = _logits(Rn, V, 0, scale=1.0), _logits(Rn, V, 7, scale=1.0)
    s[0, 5] = s[0, 9] = float("-inf")
    ones = torch.ones(Rn)
    got, _, _ = R.rowloss_grad(s.to(torch.bfloat16), V, t.to(torch.bfloat16), V, None, ones, None, None, torch.ones(1), None)
    sg = s.clone().requires_grad_(True)
    lp = OL.get_logp(sg[None], V)
    p = OL.get_p(t[None], V)
    (OL.compute_align_loss(lp, p, torch.zeros(1, Rn), distill_all_tokens=True) * Rn).backward()   # -sum_r x_r
    ref = sg.grad.double()
    sd, td = s.double(), t.double()
    q, pp = torch.softmax(sd, -1), torch.softmax(td, -1)
    m = ~torch.isinf(sd)
    fm = torch.where(m, pp, torch.zeros(())).sum(-1, keepdim=True)
    old = q - pp
    new = fm * q - torch.where(m, pp, torch.zeros(()))
    assert (old[0] - ref[0]).abs().max() > 1e-3                    # the old kernel formula: wrong on the masked row
    assert (old[0, 5] + pp[0, 5]).abs() < 1e-12                   # ... it writes -p at the masked column, where 0 is right
    assert (new - ref).abs().max() < 1e-6                          # the fm formula agrees with the oracle (fp32 autograd)
    assert (new - got).abs().max() < 1e-12                         # and with the fp64 restatement
    assert (old[1] - ref[1]).abs().max() < 1e-6                    # rows without -inf: both formulas agree (fm = 1)


LOSS_TYPES = ["sigmoid", "hinge", "ipo", "kto_pair"]


@pytest.mark.parametrize("loss_type,ls", [(lt, 0.0) for lt in LOSS_TYPES] + [("sigmoid", 0.1)])
def test_dpo_matches_oracle(loss_type, ls):
    g = torch.Generator().manual_seed(11)
    B = 9
    pc, pr, rc, rr = (torch.randn(B, generator=g) * 20 - 50 for _ in range(4))
    losses, cr, rj, dpc, dpr = R.dpo(pc, pr, rc, rr, 0.1, ls, loss_type)
    a, b = pc.clone().requires_grad_(True), pr.clone().requires_grad_(True)
    beta = float(torch.tensor(0.1, dtype=torch.float32))
    L, cr_o, rj_o = OL.dpo_loss(a, b, rc, rr, beta, float(torch.tensor(ls, dtype=torch.float32)), loss_type)
    L.mean().backward()
    torch.testing.assert_close(losses.float(), L.detach(), rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(cr.float(), cr_o, rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(rj.float(), rj_o, rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(dpc.float(), a.grad, rtol=1e-5, atol=1e-7)
    torch.testing.assert_close(dpr.float(), b.grad, rtol=1e-5, atol=1e-7)


def test_kto_pair_clamp_at_zero_passes_gradient():
    """clamp(min=0) at exactly 0 passes the gradient in torch: the fp64 restatement must see the cross term there."""
    pc = torch.tensor([1.0, -1.0, 2.0, -2.0]); rc = torch.zeros(4)       # mean(pc - rc) == 0 exactly
    pr = torch.tensor([3.0, -3.0, 0.5, -0.5]); rr = torch.zeros(4)       # mean(pr - rr) == 0 exactly
    _, _, _, dpc, dpr = R.dpo(pc, pr, rc, rr, 0.5, 0.0, "kto_pair")
    _, _, _, dpc_off, _ = R.dpo(pc, pr - 1.0, rc, rr, 0.5, 0.0, "kto_pair")   # rejected mean < 0: no cross term into pc
    assert (dpc - dpc_off).abs().max() > 1e-4
    a = pc.clone().requires_grad_(True)
    L, _, _ = OL.dpo_loss(a, pr, rc, rr, 0.5, 0.0, "kto_pair")
    L.mean().backward()
    torch.testing.assert_close(dpc.float(), a.grad, rtol=1e-6, atol=1e-7)


def test_softmax_rowdot_argmax_contracts():
    x = _logits(4, 50, 8)
    x[0, 0] = x[1, :10] = x[2, 3::7] = float("-inf")
    for log in (False, True):
        ref = R.softmax(x, 40, log)
        oracle = (OL.get_logp if log else OL.get_p)(x[None], 40)[0]
        torch.testing.assert_close(ref.float(), oracle, rtol=1e-6, atol=1e-7)
        assert bool(torch.isfinite(ref[~torch.isinf(x[:, :40])]).all())
    p, lp = OL.get_p(_logits(4, 40, 9)[None], 40), OL.get_logp(x[None], 40)
    got, _ = R.rowdot_masked(p[0], lp[0])
    torch.testing.assert_close(got.float(), torch.stack([-OL.compute_align_loss(lp[:, r:r + 1], p[:, r:r + 1], torch.zeros(1, 1),
                                                                                 True) for r in range(4)]), rtol=2e-6, atol=2e-6)
    a = torch.tensor([[1.0, 3.0, 3.0, 2.0], [float("nan"), 1.0, float("nan"), 1.0], [float("-inf")] * 4, [float("nan")] * 4,
                      [float("nan"), float("-inf"), -5.0, float("-inf")]])
    assert R.argmax(a).tolist() == [1, 1, 0, 0, 2]
