"""MoE routing kernels (csrc/moe.hip) against the sparse fp64 restatement of DeepSpeed's gating (tests/_moe_ref.py) at the
shapes where they go wrong: expert counts across the ME = 8 / 16 / 32 instantiations and partial 8-expert router groups,
token counts across the 512-token scan blocks, the router's 4-token waves and 64-token wgrad slabs, up to the step's 32768
tokens, and hidden sizes that are not multiples of 512.  Integer decisions are compared exactly; fp32 outputs in fp32 ulp or
against each element's natural scale; bf16 outputs in bf16 ulp of the fp64 result rounded where the kernel rounds.

Every bounded check prints `MOE-ERR <check> <measured max> <limit>`; the limits below were set from those figures (each is
within 16x of the largest value measured over the parametrisation on an MI355X, quoted next to it; a bf16 output that
measured 0 keeps the one ulp a double rounding can cost)."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from llavamod import kernels as K  # noqa: E402
from oracle import moe as omoe  # noqa: E402
import _moe_ref as R  # noqa: E402
from test_kernels_gpu import close, rnd  # noqa: E402

DEV = "cuda"
BF = torch.bfloat16
U32 = 2.0 ** -24           # fp32 unit roundoff

# (T, E, H): E in {2, 4, 8, 9, 16, 17, 32} (ME switch points, partial router groups), T in {1, 5, 511, 513, 4099, 32768}
# (scan-block edges, tokens not a multiple of 4 / 64, the step), H in {8, 896, 2048, 2056} (Qwen2-0.5B, not a multiple of 512)
CASES = [(1, 2, 8), (1, 9, 896), (1, 32, 2056), (1, 4, 2048),
         (5, 4, 8), (5, 16, 896), (5, 17, 2048), (5, 8, 2056),
         (511, 2, 2056), (511, 8, 896), (511, 9, 8), (511, 32, 2048), (511, 16, 2048),
         (513, 4, 2048), (513, 8, 8), (513, 16, 2056), (513, 17, 896), (513, 2, 896), (513, 32, 2048),
         (4099, 2, 896), (4099, 4, 2056), (4099, 8, 2048), (4099, 9, 2056), (4099, 16, 8), (4099, 17, 2048),
         (4099, 32, 896), (4099, 8, 8),
         (32768, 4, 2048), (32768, 8, 2048), (32768, 32, 2048), (32768, 2, 896), (32768, 9, 8), (32768, 16, 2056),
         (32768, 17, 896)]
GATE_CASES = sorted({(T, E) for T, E, _ in CASES})
CF = 1.5                   # the step's capacity factor (top-2: C = ceil(T / E * 2 * cf))


def grnd(*shape, seed, scale=1.0, dtype=torch.float32):
    """randn drawn on the device (the T = 32768 inputs are too large to draw on the host for every case)."""
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    return (torch.randn(*shape, generator=g, device=DEV) * scale).to(dtype)


def report(name, err, unit, limit):
    """Print max(err / unit) (the measured figure the limits come from) as `MOE-ERR name value limit`."""
    m = float((err.double() / unit.double().clamp_min(1e-300)).max()) if err.numel() else 0.0
    print(f"MOE-ERR {name} {m:.4g} {limit:.4g}")
    return m


def ulp(v, mant_bits):
    """Spacing of the float grid with `mant_bits` explicit+implicit mantissa bits at |v| (fp32: 24, bf16: 8); zeros get the
    spacing at the smallest normal, so a zero reference leaves no room."""
    a = v.double().abs().clamp_min(2.0 ** -126)
    return torch.ldexp(torch.ones_like(a), torch.frexp(a).exponent - mant_bits)


def assert_ulp(out, ref, name, limit, mant_bits):
    """|out - ref| <= limit ulp(ref) elementwise, compared in fp64 (close() compares in fp32, too coarse for fp32 ulp)."""
    out, ref = out.double(), ref.double()
    assert out.shape == ref.shape, name
    u = ulp(ref, mant_bits)
    err = (out - ref).abs()
    report(name, err, u, limit)
    bad = err > limit * u
    if bad.any():
        i = int(torch.argmax(err / u))
        raise AssertionError(f"{name}: {int(bad.sum())}/{err.numel()} beyond {limit} ulp; worst at {i}: "
                             f"out={out.reshape(-1)[i].item():.9g} ref={ref.reshape(-1)[i].item():.9g}")


def assert_scaled(out, ref, scale, name, c):
    """|out - ref| <= c * scale elementwise (close() with the element's natural magnitude), printing the measured max."""
    report(name, (out.double() - ref.double()).abs(), scale, c)
    close(out, ref, name, rtol=0, afrac=c, scale=scale)


def gate_logits(T, E, seed):
    """randn * 2 on a 2^-8 grid: distinct logits differ by >= 2^-8, so the fp32 softmax of the kernel and of torch cannot order
    two experts differently (no near-ties), while exact ties (first maximum wins) still occur."""
    return torch.round(grnd(T, E, seed=seed) * 512) / 256


def rows(src, slot):
    """src[slot] in fp64, zero rows for slot < 0."""
    keep = (slot >= 0)[:, None]
    return torch.where(keep, src[slot.long().clamp_min(0)].double(), torch.zeros((), dtype=torch.float64, device=DEV))


# ------------------------------------------------------------------------------------------ router logits
@pytest.mark.parametrize("T,E,H", CASES)
def test_router_fwd_vs_fp64(T, E, H):
    x = grnd(T, H, seed=T + H, dtype=BF)
    wg = grnd(E, H, seed=E, scale=0.5)
    logits = K.moe_router_fwd(x, wg)
    ref = x.double() @ wg.double().t()
    scale = x.double().abs() @ wg.double().abs().t()
    # fp32: each lane sums its ceil(H / 512) 8-element chunks in order, then a 64-lane butterfly: at H = 2056 at most
    # 5 * 8 + 6 = 46 roundings, a worst case of 46 * 2^-24 ~ 2^-18.5 of sum |x_h w_eh|.  Measured: 2.4e-7 (limit 2^-18 = 3.8e-6).
    assert_scaled(logits, ref, scale, "router_fwd", 2 ** -18)


# ------------------------------------------------------------------------------------------ gating
def check_gate(st, m, logits, name):
    """Kernel gate state vs the reference maps: integer outputs exactly, fp32 outputs against fp64."""
    for key in ("idx1", "idx2", "slot1", "slot2"):          # the slots carry the capacity positions: slot = e * C + loc
        if m[key] is not None:
            assert torch.equal(getattr(st, key).long(), m[key]), f"{name}: {key}"
    assert torch.equal(st.slot_token.long(), m["slot_token"]), f"{name}: slot_token"
    assert torch.equal(st.exp_counts.long(), m["exp_counts"]), f"{name}: exp_counts"
    assert torch.equal(st.slots_used.long(), m["slots_used"]), f"{name}: slots_used"
    r = R.weights(m, logits)
    # gates: expf, an in-order fp32 sum of E exponentials (up to ~E / 2 ulp of the denominator at E = 32) and one
    # division.  Measured: 10.6 ulp (E = 32).
    assert_ulp(st.gates, r["gates"], f"{name} gates", 16, 24)
    # w = g / clamp(g1 + g2, eps): the gates' error plus one add and one division in fp32; dropped picks exactly 0.
    # Measured: 7.8 ulp.
    assert_ulp(st.w1, r["w1"], f"{name} w1", 16, 24)
    if m["k"] == 2:
        assert_ulp(st.w2, r["w2"], f"{name} w2", 16, 24)
    assert_ulp(st.slot_w, r["slot_w"], f"{name} slot_w", 16, 24)
    # gate_sum: 64-lane butterfly, 8 waves, then ceil(T / 512) block partials in order; l_aux = E * sum_e (gs_e / T)(n_e / T):
    # fp32 sums of at most ~6 + 8 + 64 terms at T = 32768.  Measured: gate_sum 3.7e-7, l_aux 2.3e-7.
    gs = r["gate_sum"]
    report(f"{name} gate_sum(rel)", (st.gate_sum.double() - gs).abs(), gs.abs(), 4e-6)
    assert ((st.gate_sum.double() - gs).abs() <= 4e-6 * gs.abs()).all(), f"{name}: gate_sum {st.gate_sum} vs {gs}"
    la = r["l_aux"].reshape(1)
    report(f"{name} l_aux(rel)", (st.l_aux.double() - la).abs(), la.abs(), 2e-6)
    assert ((st.l_aux.double() - la).abs() <= 2e-6 * la.abs()).all(), f"{name}: l_aux {st.l_aux} vs {la}"
    return r


@pytest.mark.parametrize("mode", ["none", "gumbel", "philox"])
@pytest.mark.parametrize("T,E", GATE_CASES)
def test_gate_top2_vs_fp64(T, E, mode):
    logits = gate_logits(T, E, seed=7 * T + E)
    C = omoe.capacity(T, E, CF * 2, 0)
    if mode == "philox":          # noise drawn in the kernel, then fed to the reference
        st = K.moe_gate(logits, 2, C, None, seed=1000 + E, offset=T, want_noise=True)
        noise = st.noise
    else:
        noise = None if mode == "none" else omoe.gumbel_noise((T, E), torch.Generator().manual_seed(T + E)).to(DEV)
        st = K.moe_gate(logits, 2, C, noise)
    check_gate(st, R.top2_maps(logits, C, noise), logits, f"top2-{mode}")


@pytest.mark.parametrize("mode", ["order", "rts", "rts-philox"])
@pytest.mark.parametrize("T,E", GATE_CASES)
def test_gate_top1_vs_fp64(T, E, mode):
    logits = gate_logits(T, E, seed=5 * T + E)
    C = omoe.capacity(T, E, 1.0, 0)
    if mode == "rts-philox":
        st = K.moe_gate(logits, 1, C, None, seed=77 + E, offset=3 * T, want_noise=True)
        prio = st.noise
    else:
        prio = None if mode == "order" else torch.rand(T, E, generator=torch.Generator().manual_seed(T * E)).to(DEV)
        st = K.moe_gate(logits, 1, C, prio)
    check_gate(st, R.top1_maps(logits, C, prio), logits, f"top1-{mode}")


EDGES = [("C=1", 513, 4), ("C=1", 4099, 17), ("cf=0.5", 4099, 8), ("cf=0.5", 32768, 32), ("C>=T", 4099, 16), ("C>=T", 511, 2),
         ("min_capacity", 511, 32), ("min_capacity", 5, 9), ("equal rows", 513, 9), ("equal rows", 4099, 32)]


@pytest.mark.parametrize("k", [1, 2])
@pytest.mark.parametrize("edge,T,E", EDGES)
def test_gate_capacity_edges(edge, T, E, k):
    logits = gate_logits(T, E, seed=T + 31 * E)
    cf = 0.5 if edge == "cf=0.5" else CF
    C = omoe.capacity(T, E, cf * k, 0)
    if edge == "C=1":
        C = 1
    elif edge == "C>=T":
        C = T
    elif edge == "min_capacity":
        C = omoe.capacity(T, E, cf * k, min_capacity=C + 37)
    elif edge == "equal rows":
        logits[::3] = 0.75
    noise = None if (k == 1 or edge == "equal rows") else \
        omoe.gumbel_noise((T, E), torch.Generator().manual_seed(T)).to(DEV)
    st = K.moe_gate(logits, k, C, noise)
    m = R.top2_maps(logits, C, noise) if k == 2 else R.top1_maps(logits, C, None)
    check_gate(st, m, logits, f"edge {edge} k={k}")
    if edge == "C>=T":
        assert bool((st.slot1 >= 0).all()) and (k == 1 or bool((st.slot2 >= 0).all()))
    if edge == "equal rows":
        assert bool((st.idx1[::3] == 0).all()) and (k == 1 or bool((st.idx2[::3] == 1).all()))
    if edge == "C=1":
        assert int((st.slot_token >= 0).sum()) <= E


# ------------------------------------------------------------------------------------------ combine
def gate_state(T, E, seed):
    logits = gate_logits(T, E, seed=seed)
    C = omoe.capacity(T, E, CF * 2, 0)
    noise = omoe.gumbel_noise((T, E), torch.Generator().manual_seed(seed)).to(DEV)
    return K.moe_gate(logits, 2, C, noise), logits, noise


@pytest.mark.parametrize("T,E,H", CASES)
def test_combine_fwd_bwd_vs_fp64(T, E, H):
    st, _, _ = gate_state(T, E, seed=T + 3 * E)
    S = E * st.C
    y = grnd(S, H, seed=S + H, dtype=BF)
    out = K.moe_combine_fwd(y, st, H)
    a1, a2 = st.w1.to(BF).double()[:, None], st.w2.to(BF).double()[:, None]       # combine_weights.type_as(x)
    y1, y2 = rows(y, st.slot1), rows(y, st.slot2)
    ref = (a1 * y1 + a2 * y2).to(BF)
    # bf16 x bf16 products are exact in fp32; one fp32 add, one rounding to bf16.  Measured: 0 ulp (a double rounding, fp32
    # then bf16, could make it 1).
    assert_ulp(out, ref, "combine_fwd", 1, 8)
    dout = grnd(T, H, seed=T + 11, dtype=BF)
    dy, dw1, dw2 = K.moe_combine_bwd(dout, y, st, H)
    # slot side: bf16(slot_w) * dout[slot_token] is exact in fp32, so the one rounding to bf16 makes it bit-identical
    ref_dy = (st.slot_w.to(BF).double()[:, None] * rows(dout, st.slot_token)).to(BF)
    assert torch.equal(dy.view(torch.int16), ref_dy.view(torch.int16)), \
        f"combine_bwd dy: {int((dy != ref_dy).sum())} elements differ"
    # weight side: <dout[t], y[slot_j(t)]> — per lane ceil(H / 512) chunks of 8 in order, then a 64-lane butterfly: at most
    # ~46 fp32 roundings of sum_h |dout y| in the worst case.  Measured: 8.3e-8 (limit 2^-20 = 9.5e-7).
    d = dout.double()
    for name, dw, yj in (("combine_bwd dw1", dw1, y1), ("combine_bwd dw2", dw2, y2)):
        assert_scaled(dw, (d * yj).sum(1), (d.abs() * yj.abs()).sum(1), name, 2 ** -20)


# ------------------------------------------------------------------------------------------ gate backward
@pytest.mark.parametrize("k", [1, 2])
@pytest.mark.parametrize("T,E", GATE_CASES)
def test_gate_bwd_vs_fp64_autograd(T, E, k):
    logits = gate_logits(T, E, seed=3 * T + E)
    if k == 2:
        C = omoe.capacity(T, E, CF * 2, 0)
        noise = omoe.gumbel_noise((T, E), torch.Generator().manual_seed(E)).to(DEV)
        st, m = K.moe_gate(logits, 2, C, noise), R.top2_maps(logits, C, noise)
    else:
        C = omoe.capacity(T, E, 1.0, 0)
        st, m = K.moe_gate(logits, 1, C, None), R.top1_maps(logits, C, None)
    assert torch.equal(st.slot1.long(), m["slot1"]) and (k == 1 or torch.equal(st.slot2.long(), m["slot2"]))
    u1 = grnd(T, seed=T + 1)
    u2 = grnd(T, seed=T + 2) if k == 2 else None
    dla = torch.tensor([0.75], device=DEV)
    dlog = K.moe_gate_bwd(st, u1, u2, dla)
    ref, scale = R.gate_grad(m, logits, u1, u2, 0.75)
    # fp32 gates (a few ulp), then u / sum - (u1 g1 + u2 g2) / sum^2 and g (dg - <g, dg>): a few roundings at the natural
    # scale (terms that cancel included).  Measured: 1.24e-6 (k = 1), 4.3e-7 (k = 2); limit 2^-19 = 1.9e-6.
    assert_scaled(dlog, ref, scale, f"gate_bwd k={k}", 2 ** -19)


@pytest.mark.parametrize("E", [4, 9])
def test_gate_bwd_clamped_denominator(E):
    """A token whose first pick was dropped for capacity and whose surviving second pick has a gate below the fp32 eps:
    w2 = g2 / eps (the clamp), so d w2 / d g2 = 1 / eps with no cross term and the logits gradient is ~1e-3, not 0.  Built as
    in the CPU repro (tests/test_moe_ref_cpu.py) inside a T = 513 batch: token 512 sits alone in the second scan block, token
    300 in the first."""
    T, C = 513, 64
    logits = gate_logits(T, E, seed=E) * 0.25
    logits[:, 0] += 3.0                       # expert 0 is every token's first pick: tokens >= 64 lose it to capacity
    logits[:, E - 1] = -5.0                   # nobody else picks the last expert second
    noise = torch.zeros(T, E, device=DEV)
    clamp_tok = [300, 512]
    for t in clamp_tok:
        logits[t] = 0.0
        logits[t, 0], logits[t, E - 1] = 20.0, -1.0     # second-pick gate e^-21 / (e^20 + ...) ~ 7.6e-10
        noise[t, E - 1] = 100.0
    st = K.moe_gate(logits, 2, C, noise)
    m = R.top2_maps(logits, C, noise)
    check_gate(st, m, logits, f"clamp E={E}")
    for t in clamp_tok:
        assert int(st.slot1[t]) < 0 and int(st.slot2[t]) >= 0 and int(st.idx2[t]) == E - 1
        assert float(st.gates[t, E - 1]) < R.EPS32
    u1, u2 = grnd(T, seed=1), grnd(T, seed=2)
    dlog = K.moe_gate_bwd(st, u1, u2, torch.tensor([0.75], device=DEV))
    ref, scale = R.gate_grad(m, logits, u1, u2, 0.75)
    for t in clamp_tok:
        assert ref[t].abs().max() > 1e-4, ref[t]
    # same bound as test_gate_bwd_vs_fp64_autograd.  Measured: 3.7e-7.
    assert_scaled(dlog, ref, scale, f"gate_bwd clamp E={E}", 2 ** -19)


# ------------------------------------------------------------------------------------------ dispatch backward
@pytest.mark.parametrize("router", [True, False])
@pytest.mark.parametrize("T,E,H", CASES)
def test_dispatch_bwd_vs_fp64(T, E, H, router):
    st, _, _ = gate_state(T, E, seed=T + 5 * E)
    d_in = grnd(E * st.C, H, seed=H + E, dtype=BF)
    wg = grnd(E, H, seed=E + 1, scale=0.5)
    dl = grnd(T, E, seed=T + 9, scale=0.05) if router else None
    dx = K.moe_dispatch_bwd(d_in, st, dl, wg, H)
    rest = rows(d_in, st.slot1) + rows(d_in, st.slot2)
    if router:
        r64 = dl.double() @ wg.double()
        ref = r64 + rest
        # the kernel rounds the router term (an fp32 sum of E products, error <= E * 2^-24 sum_e |dl w|) to bf16, adds the
        # two rows in fp32 (two roundings at the size of |r| + |d1| + |d2|, which matter when they cancel) and rounds to
        # bf16: half a bf16 ulp of the router term plus half a bf16 ulp of the result, which may round up into the next
        # binade (up to 1.5 units of the larger ulp), plus those fp32 errors.  Measured: 1.0.
        rest_abs = rows(d_in, st.slot1).abs() + rows(d_in, st.slot2).abs()
        lim = 1.5
        u = torch.maximum(ulp(ref, 8), ulp(r64, 8)) + E * U32 * (dl.double().abs() @ wg.double().abs()) + \
            2 * U32 * (r64.abs() + rest_abs)
    else:
        ref, lim = rest, 1.0
        u = ulp(ref, 8)                                  # two bf16 rows added in fp32, one rounding.  Measured: 0.5.
    err = (dx.double() - ref).abs()
    report(f"dispatch_bwd router={router}", err, u, lim)
    close(dx, ref, f"dispatch_bwd router={router}", rtol=0, afrac=lim, scale=u)


# ------------------------------------------------------------------------------------------ router weight gradient
@pytest.mark.parametrize("T,E,H", CASES)
def test_router_wgrad_vs_fp64(T, E, H):
    x = grnd(T, H, seed=T + 2 * H, dtype=BF)
    dl = grnd(T, E, seed=T + E, scale=0.01)
    ref = dl.double().t() @ x.double()
    scale = dl.double().abs().t() @ x.double().abs()
    dwg = torch.full((E, H), float("nan"), device=DEV)
    K.moe_router_wgrad(x, dl, dwg, False)
    # fp32: 64 tokens per slab in order, ceil(slabs / 16) partials per group, 16 groups in order: at T = 32768 at most
    # 64 + 32 + 16 roundings of sum_t |dl x| in the worst case.  Measured: 1.6e-7 (limit 2^-19 = 1.9e-6).
    assert_scaled(dwg, ref, scale, "router_wgrad", 2 ** -19)
    again = torch.zeros(E, H, device=DEV)
    K.moe_router_wgrad(x, dl, again, False)
    assert torch.equal(dwg.view(torch.int32), again.view(torch.int32)), "router_wgrad: not bitwise reproducible"
    base = grnd(E, H, seed=H, scale=0.1)
    acc = base.clone()
    K.moe_router_wgrad(x, dl, acc, True)
    # accumulate: one more fp32 add onto the existing gradient
    assert_scaled(acc, base.double() + ref, scale + base.double().abs(), "router_wgrad accumulate", 2 ** -19)


# ------------------------------------------------------------------------------------------ residual mix, small dgrad
@pytest.mark.parametrize("T,H", [(1, 8), (5, 896), (513, 2056), (4099, 2048), (4099, 8)])
def test_residual_mix_vs_fp64(T, H):
    a, b = rnd(T, H, seed=T), rnd(T, H, seed=T + 1)
    clog = grnd(T, 2, seed=T, scale=2.0)
    cbias = torch.tensor([0.3, -0.2], device=DEV)
    out, p = K.residual_mix_fwd(a, b, clog, cbias)
    # rounding points (moe.hip residual_mix_fwd_kernel): c = bf16(fp32 logit + bias), p = bf16(softmax(c)),
    # out = bf16(bf16(a p0) + bf16(b p1))
    c = (clog + cbias).to(BF).double()
    p_ref = torch.softmax(c, dim=1).to(BF)
    assert_ulp(p, p_ref, "residual_mix p", 1, 8)          # fp32 expf / division vs fp64 before the rounding.  Measured: 0.
    pk = p.double()                                        # the kernel's p from here on: a flipped p is checked above
    ref = ((a.double() * pk[:, :1]).to(BF).double() + (b.double() * pk[:, 1:]).to(BF).double()).to(BF)
    assert_ulp(out, ref, "residual_mix out", 1, 8)        # Measured: 0.
    dout = rnd(T, H, seed=T + 2)
    da, db, dc = K.residual_mix_bwd(dout, a, b, p)
    # d_a = bf16(dout p0), d_b = bf16(dout p1): exact fp32 products, one rounding -> bit-identical
    assert torch.equal(da, (dout.double() * pk[:, :1]).to(BF)) and torch.equal(db, (dout.double() * pk[:, 1:]).to(BF))
    d = dout.double()
    s0, s1 = (d * a.double()).sum(1), (d * b.double()).sum(1)
    S0, S1 = (d * a.double()).abs().sum(1), (d * b.double()).abs().sum(1)
    dot = pk[:, 0] * s0 + pk[:, 1] * s1
    ref_dc = torch.stack([pk[:, 0] * (s0 - dot), pk[:, 1] * (s1 - dot)], 1)
    sc = torch.stack([pk[:, 0] * (S0 + pk[:, 0] * S0 + pk[:, 1] * S1), pk[:, 1] * (S1 + pk[:, 0] * S0 + pk[:, 1] * S1)], 1)
    # fp32 row dots (ceil(H / 512) chunks of 8 per lane, 64-lane butterfly) then the 2-way softmax backward.  Measured: 1.05e-7.
    assert_scaled(dc, ref_dc, sc, "residual_mix dc", 2 ** -20)


@pytest.mark.parametrize("E", [2, 9, 32])
@pytest.mark.parametrize("T,H", [(5, 8), (513, 2056), (4099, 896)])
def test_small_linear_dgrad_vs_fp64(T, H, E):
    dl = grnd(T, E, seed=T + E, scale=0.1)
    w = grnd(E, H, seed=E + H, scale=0.5)
    dx = K.small_linear_dgrad(dl, w)
    ref = dl.double() @ w.double()
    # fp32 sum of E products (<= E * 2^-24 of sum_e |dl w|), then one rounding to bf16.  Measured: 0.5.
    u = ulp(ref, 8) + E * U32 * (dl.double().abs() @ w.double().abs())
    report(f"small_linear_dgrad E={E}", (dx.double() - ref).abs(), u, 1.0)
    close(dx, ref, f"small_linear_dgrad E={E}", rtol=0, afrac=1.0, scale=u)
