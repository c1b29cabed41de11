"""tests/_moe_ref.py (the sparse fp64 gating restatement the MoE kernel tests use at step sizes) against the dense oracle
(oracle/moe.py) on the CPU: integer maps bit for bit, weights and logits gradients within fp32 rounding."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle import moe as omoe  # noqa: E402
import _moe_ref as R  # noqa: E402


def _dense(m, w1, w2):
    """[T, E, C] combine tensor from the sparse maps."""
    T, E, C = m["T"], m["E"], m["C"]
    d = torch.zeros(T, E * C, dtype=w1.dtype)
    for slot, w in ((m["slot1"], w1), (m["slot2"], w2))[:m["k"]]:
        kept = slot >= 0
        d[torch.nonzero(kept).squeeze(1), slot[kept]] = w[kept]
    return d.view(T, E, C)


def _check(m, logits, combine, dispatch, exp_counts, l_aux, lg_grad_fn, seed):
    """Compare the sparse maps / weights / gradient with the dense oracle's outputs for the same gating."""
    T, E, C = m["T"], m["E"], m["C"]
    assert combine.shape == (T, E, C)
    assert torch.equal(m["exp_counts"], exp_counts.long())
    # integer maps: the kept (token, expert, position) triples are exactly the oracle's dispatch mask
    live = _dense(m, torch.ones(T), torch.ones(T) if m["k"] == 2 else None).bool()
    assert torch.equal(live, dispatch)
    st = m["slot_token"]
    assert torch.equal(st >= 0, dispatch.any(0).reshape(-1))
    nz = torch.nonzero(dispatch.reshape(T, E * C))
    assert torch.equal(st[nz[:, 1]], nz[:, 0])
    assert torch.equal(m["slots_used"], dispatch.any(0).sum(1))
    assert torch.equal(m["kept1"], (m["slot1"] >= 0))
    # weights: the fp64 restatement within fp32 rounding of the oracle's fp32 einsums
    r = R.weights(m, logits)
    torch.testing.assert_close(_dense(m, r["w1"], r["w2"]).float(), combine, rtol=2e-6, atol=1e-7)
    sw = torch.zeros(E * C, dtype=torch.float64)
    sw[nz[:, 1]] = combine.reshape(T, E * C)[nz[:, 0], nz[:, 1]].double()
    torch.testing.assert_close(r["slot_w"], sw, rtol=2e-6, atol=1e-7)
    torch.testing.assert_close(r["l_aux"].float(), l_aux.float(), rtol=2e-6, atol=1e-7)
    # gradient: dense fp32 autograd of (combine * Rw).sum() + d_laux * l_aux vs the sparse objective with u_j = Rw at slot j
    g = torch.Generator().manual_seed(seed)
    Rw = torch.randn(T, E, C, generator=g)
    dla = 0.75
    ref_grad = lg_grad_fn(Rw, dla)
    Rf = Rw.reshape(T, E * C)
    u = [torch.where(s >= 0, Rf.gather(1, s.clamp_min(0)[:, None]).squeeze(1), torch.zeros(T))
         for s in (m["slot1"], m["slot2"])[:m["k"]]]
    got, scale = R.gate_grad(m, logits, u[0], u[1] if m["k"] == 2 else None, dla)
    # the oracle's fp32 autograd rounds at each element's natural scale (terms that cancel included): a few fp32 ulp of it
    err = (got - ref_grad.double()).abs()
    assert (err <= 2 ** -20 * scale).all(), float((err / scale.clamp_min(1e-300)).max())
    return got


def _top2_case(logits, cf, min_cap, noise, seed):
    T, E = logits.shape
    C = omoe.capacity(T, E, cf * 2, min_cap)
    l_aux, combine, dispatch, cnt = omoe.top2gating(logits, cf, min_cap, noise)
    m = R.top2_maps(logits, C, noise)

    def grad(Rw, dla):
        lg = logits.clone().requires_grad_(True)
        la, comb, _, _ = omoe.top2gating(lg, cf, min_cap, noise)
        ((comb * Rw).sum() + dla * la).backward()
        return lg.grad

    return m, _check(m, logits, combine, dispatch, cnt, l_aux, grad, seed)


@pytest.mark.parametrize("T,E,cf,min_cap,noise", [
    (1, 2, 1.5, 0, False), (5, 4, 1.5, 0, True), (511, 8, 1.5, 0, True), (513, 9, 0.5, 0, True), (700, 17, 1.0, 0, False),
    (2048, 32, 1.5, 0, True), (2048, 4, 0.5, 0, True), (300, 4, 0.5, 200, True), (64, 4, 40.0, 0, False)])
def test_sparse_top2_equals_dense_oracle(T, E, cf, min_cap, noise):
    g = torch.Generator().manual_seed(T * 100 + E)
    logits = torch.randn(T, E, generator=g) * 2
    nz = omoe.gumbel_noise((T, E), g) if noise else None
    _top2_case(logits, cf, min_cap, nz, seed=T)


def test_sparse_top2_equal_logit_rows():
    """Rows of equal logits: the first maximum wins both picks (idx1 = 0, idx2 = 1)."""
    logits = torch.randn(40, 8, generator=torch.Generator().manual_seed(3))
    logits[::3] = 0.5
    m, _ = _top2_case(logits, 1.5, 0, None, seed=3)
    assert (m["idx1"][::3] == 0).all() and (m["idx2"][::3] == 1).all()


def test_clamped_denominator_gradient_is_not_zero():
    """The clamp case: token 2's first pick (expert 0) is dropped at C = 1 and its second pick is forced onto expert 3 with a
    gate of 7.6e-10, below the fp32 eps.  w = g / eps there, so d w / d g = 1 / eps and the logits gradient is nonzero
    (about 2e-3 at expert 0 and 3); a backward that adds nothing for sum < eps gives exactly 0."""
    logits = torch.tensor([[5., 0, 0, 0], [5, 1, 0, 0], [20, 0, 0, -1], [0, 5, 0, 0]])
    noise = torch.zeros(4, 4)
    noise[2, 3] = 100.0
    m, grad = _top2_case(logits, 0.5, 0, noise, seed=0)
    assert m["C"] == 1 and not bool(m["kept1"][2]) and bool(m["kept2"][2]) and int(m["idx2"][2]) == 3
    gates = F.softmax(logits.double(), 1)
    assert gates[2, 3] < R.EPS32
    assert grad[2, 0] < -1e-4 and grad[2, 3] > 1e-4, grad[2]
    # the repro's numbers: objective (combine * R).sum() with R ~ randn at torch.manual_seed(0), no l_aux term
    torch.manual_seed(0)
    Rw = torch.randn(4, 4, 1)
    u2 = Rw[2, 3, 0]
    got, _ = R.gate_grad(m, logits, torch.zeros(4), torch.zeros(4).index_fill(0, torch.tensor([2]), float(u2)), 0.0)
    lg = logits.clone().requires_grad_(True)
    _, comb, _, _ = omoe.top2gating(lg, 0.5, 0, noise)
    (comb[2] * Rw[2]).sum().backward()
    torch.testing.assert_close(got[2].float(), lg.grad[2], rtol=1e-5, atol=1e-12)
    assert abs(float(got[2, 0]) - (-1.96e-3)) < 0.01e-3 and abs(float(got[2, 3]) - 1.96e-3) < 0.01e-3, got[2]


@pytest.mark.parametrize("T,E,cf,rts", [(1, 2, 1.0, True), (513, 4, 1.0, False), (513, 9, 0.5, True), (2048, 32, 1.0, True),
                                        (2048, 8, 4.0, False), (1000, 16, 0.5, True)])
def test_sparse_top1_equals_dense_oracle(T, E, cf, rts):
    g = torch.Generator().manual_seed(T + E)
    logits = torch.randn(T, E, generator=g) * 2
    prio = torch.rand(T, E, generator=g) if rts else None
    C = omoe.capacity(T, E, cf, 0)
    l_aux, combine, dispatch, cnt = omoe.top1gating(logits, cf, 0, prio)
    m = R.top1_maps(logits, C, prio)

    def grad(Rw, dla):
        lg = logits.clone().requires_grad_(True)
        la, comb, _, _ = omoe.top1gating(lg, cf, 0, prio)
        ((comb * Rw).sum() + dla * la).backward()
        return lg.grad

    _check(m, logits, combine, dispatch, cnt, l_aux, grad, seed=T)
