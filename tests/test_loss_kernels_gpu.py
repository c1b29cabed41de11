"""Loss-head kernels (csrc/loss.hip) against the fp64 restatement in tests/_loss_ref.py at the shapes where they go wrong:
Qwen2's 151936-column aligned vocabulary read from 152064-column strided rows, a 128-column extra slice, aligned slices of
255 / 256 / 257 chunks of 8 against 256 threads, 8-column rows, up to 4096 rows through the backward and a forward whose
row * ld passes 2^32 elements; values with large offsets, near one-hot rows and -inf logits in every slice.  Integer outputs
are compared exactly; fp32 outputs against each element's natural scale in fp32 unit roundoff; bf16 gradients in bf16 ulp
of the fp64 value plus an fp32 term at the gradient's natural scale.

Every bounded check prints `LOSS-ERR <check> <measured max> <limit>`; each limit below is within 16x of the largest value
measured over the parametrisation on an MI355X, quoted next to it."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from llavamod import kernels as K  # noqa: E402
import _loss_ref as LR  # noqa: E402

DEV = "cuda"
BF = torch.bfloat16
U32 = 2.0 ** -24           # fp32 unit roundoff
NINF = float("-inf")
NAN = float("nan")
VA, VQ = 151936, 152064    # the aligned vocabulary; Qwen2's padded lm_head width


def report(name, err, unit, limit):
    """Print max(err / unit) (the measured figure the limits come from) as `LOSS-ERR name value limit`; assert it."""
    m = float((err.double() / unit.double().clamp_min(1e-300)).max()) if err.numel() else 0.0
    print(f"LOSS-ERR {name} {m:.4g} {limit:.4g}")
    assert m <= limit, f"{name}: {m:.4g} > {limit:.4g}"
    return m


def ulp_bf16(v):
    """bf16 spacing at |v| (zeros: the spacing at the smallest normal)."""
    a = v.double().abs().clamp_min(2.0 ** -126)
    return torch.ldexp(torch.ones_like(a), torch.frexp(a).exponent - 8)


def bits(x):
    return x.contiguous().view(torch.int16)


# ------------------------------------------------------------------------------------------ inputs
def _randn(rows, V, seed):
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    return torch.randn(rows, V, generator=g, device=DEV)


def make_rows(R, V, ld, Va, seed, teacher, shift, chunk=2048):
    """bf16 [R, ld] buffer, columns [V, ld) NaN (must never be read), returned as the [R, V] view.  Row r's kind is
    (r + shift) % 6:
      0  N(0, 3) plus a row offset in [-5, 5] and three peaked tokens (+15);
      1  N(0, 3) + 60 or - 60 (bf16 spacing 0.25 .. 0.5; x_kd = E_p[s] - lse_a fm cancels);
      2  near one-hot: N(0, 0.5) with one column at +40 (the student's and teacher's hot columns differ on odd rows);
      3  student -inf in [0, Va): columns 0 (thread 0's first), 8 (thread 1's first), 2048 (thread 0's second chunk), one more;
      4  student -inf in [Va, V): column Va (thread 0's first in the extra slice), Va + 8 and V - 1 (all-finite aligned slice);
      5  teacher -inf at columns 3 and c, student -inf at c (0 * -inf under the mask) and at column 1 (teacher finite)."""
    buf = torch.full((R, ld), NAN, device=DEV, dtype=BF)
    for lo in range(0, R, chunk):
        hi = min(R, lo + chunk)
        r = torch.arange(lo, hi, device=DEV)
        kind = (r + shift) % 6
        x = _randn(hi - lo, V, seed * 1000003 + lo)
        g = torch.Generator(device=DEV)
        g.manual_seed(seed + 7 * lo)
        off = (torch.rand(hi - lo, 1, generator=g, device=DEV) - 0.5) * 10
        sign = torch.where(r % 2 == 0, 60.0, -60.0)[:, None]
        x = torch.where((kind == 1)[:, None], x * 3 + sign, torch.where((kind == 2)[:, None], x * 0.5 + off, x * 3 + off))
        rr = torch.arange(hi - lo, device=DEV)
        hot = (r * 7919 + (r % 2) * (13 if teacher else 0)) % Va
        x[rr, hot] = torch.where(kind == 2, 40.0, x[rr, hot])
        for k in range(3):
            pk = (r * (97 + k) + 11 * k) % Va
            x[rr, pk] = torch.where(kind == 0, x[rr, pk] + 15.0, x[rr, pk])
        c = (r * 31 + 5) % Va
        if not teacher:
            for col in (0, 8, 2048, None):
                cc = c if col is None else torch.full_like(r, col)
                ok = (kind == 3) & (cc < Va)
                x[rr[ok], cc[ok]] = NINF
            if V > Va:
                for col in (Va, Va + 8, V - 1):
                    if col < V:
                        x[rr[kind == 4], col] = NINF
            x[rr[kind == 5], c[kind == 5]] = NINF
            x[rr[kind == 5], 1] = NINF
        else:
            x[rr[kind == 5], c[kind == 5]] = NINF
            x[rr[kind == 5], 3 % Va] = NINF
        buf[lo:hi, :V] = x.to(BF)
    return buf[:, :V]


def make_labels(s, Vs, Va):
    """Labels cycling 0, Va - 1, Va, Vs - 1, -100 (Va == Vs: label Vs, out of range, CE 0 by contract); a label on a -inf
    student logit gets a finite logit there."""
    R = s.shape[0]
    ch = torch.tensor([0, Va - 1, Va, Vs - 1, -100], device=DEV)
    label = ch[torch.arange(R, device=DEV) % 5].to(torch.int32)
    lb = label.long()
    ok = (lb >= 0) & (lb < Vs)
    rows = torch.nonzero(ok).squeeze(1)
    v = s[rows, lb[rows]]
    s[rows, lb[rows]] = torch.where(torch.isinf(v), torch.zeros_like(v), v)
    return label


# (Vs, Va, ld_s, t width, ld_t): t width None -> t = None (the DPO / LM path, Va = Vs)
GEOMS = {
    "qwen-strided-teacher": (VA, VA, VA, VA, VQ),        # teacher: a [:, :151936] view of a 152064-column lm_head output
    "extra-slice": (VQ, VA, VQ, VA, VA),                 # student 152064 columns, KD over the first 151936
    "va2040": (2048, 2040, 2048, 2040, 2040),            # 255 chunks of 8 against 256 threads
    "va2048-ld": (2048, 2048, 2056, 2048, 2056),         # 256 chunks; strided student and teacher
    "va2056": (2064, 2056, 2064, 2064, 2064),            # 257 chunks
    "vs8": (8, 8, 8, 8, 8),
    "vs16-va8-ld": (16, 8, 24, 8, 16),
    "lm-strided": (VA, VA, VQ, None, None),              # t = None, student read from 152064-column rows
    "lm": (VQ, VQ, VQ, None, None),
}
CASES = [("qwen-strided-teacher", 1), ("qwen-strided-teacher", 7), ("qwen-strided-teacher", 4096),
         ("extra-slice", 1), ("extra-slice", 7), ("extra-slice", 4096),
         ("va2040", 7), ("va2040", 257), ("va2048-ld", 7), ("va2048-ld", 4096), ("va2056", 1), ("va2056", 4096),
         ("vs8", 7), ("vs16-va8-ld", 7), ("vs16-va8-ld", 4096),
         ("lm-strided", 7), ("lm-strided", 4096), ("lm", 1), ("lm", 7)]


def make_case(geom, R, seed):
    Vs, Va, ld_s, tw, ld_t = GEOMS[geom]
    shift = 4 if (R == 1 and Vs > Va) else 3                  # R = 1: a row with -inf where the bugs were
    s = make_rows(R, Vs, ld_s, Va, seed, False, shift)
    t = make_rows(R, tw, ld_t, Va, seed + 1, True, shift) if tw is not None else None
    label = make_labels(s, Vs, Va)
    return Vs, Va, s, t, label


def check_stats(st, ref, s, Va, name):
    assert bool(torch.isfinite(st).all()), f"{name}: non-finite stats"
    # lse, in fp32 ulp of 1 + max|s| (the size of the exponents' arguments): per-thread online (max, sum) with __expf over
    # ceil(V / 2048) chunks, merged over 64 lanes and 4 waves, one logf.  Measured: lse_f 3.6, lse_a 3.6, lse_t 4.0.
    lsc = ref["lse_scale"]
    report(f"{name} lse_f", (st[:, 0].double() - ref["lse_f"]).abs(), lsc * U32, 16)
    report(f"{name} lse_a", (st[:, 1].double() - ref["lse_a"]).abs(), lsc * U32, 16)
    report(f"{name} lse_t", (st[:, 2].double() - ref["lse_t"]).abs(), ref["lse_t_scale"] * U32, 16)
    # x_kd = sum e^(t - m) s / sum e^(t - m) - lse_a fm: fp32 sums of terms of size p |s| then the cancellation against
    # lse_a fm, in fp32 ulp of sum m p |s| + |lse_a| fm.  Measured: 37.1 (R = 28300, offsets of +-60).  Limit 256.
    report(f"{name} x_kd", (st[:, 3].double() - ref["x_kd"]).abs(), ref["x_scale"] * U32, 256)
    # fm: two fp32 sums of the same exponentials, one with the masked columns left out.  Measured: 4.0 ulp of 1.
    report(f"{name} fm", (st[:, 6].double() - ref["fm"]).abs(), torch.full_like(ref["fm"], U32), 32)
    finite_rows = ~torch.isinf(s[:, :Va]).any(1)
    assert bool((st[finite_rows, 6] == 1.0).all()), f"{name}: fm != 1 on a row without -inf"
    # ce = lse_f - s[label]: lse_f's error plus one subtraction.  Measured: 3.3.
    report(f"{name} ce", (st[:, 4].double() - ref["ce"]).abs(), (lsc + ref["s_label"].abs()) * U32, 32)
    assert torch.equal(st[:, 5].double(), ref["s_label"]), f"{name}: s[label] is the bf16 logit, exactly"
    assert bool((st[:, 7] == 0).all())


@pytest.mark.parametrize("geom,R", CASES)
def test_rowloss_fwd_bwd_vs_fp64(geom, R):
    Vs, Va, s, t, label = make_case(geom, R, seed=R + len(geom))
    st = K.rowloss_fwd(s, Vs, t, Va, label)
    ref = LR.rowloss_stats(s, Vs, t, Va, label)
    check_stats(st, ref, s, Va, f"fwd {geom} R={R}")
    nseg = 3
    r = torch.arange(R, device=DEV)
    seg_id = (r * nseg // R).to(torch.int32)
    kd_w = torch.tensor([1.0, 1.0, 0.5, 0.0, 1.0], device=DEV)[r % 5]
    ce_w = ((label >= 0) & (label < Vs)).float()            # the CE rows: forward CE is 0 for labels outside [0, Vs)
    kd_scale = torch.tensor([0.37, -1.3, 0.0], device=DEV)
    ce_scale = torch.tensor([-0.21, 0.0, 0.9], device=DEV)
    modes = {"kd": (kd_scale, None), "ce": (None, ce_scale), "both": (kd_scale, ce_scale)}
    for mode, (ks, cs) in modes.items():
        if t is None and mode == "kd":
            continue
        name = f"bwd {geom} R={R} {mode}"
        ld_ds = s.stride(0) + 8
        ds_buf = torch.full((R, ld_ds), NAN, device=DEV, dtype=BF)
        ds = ds_buf[:, :Vs]
        K.rowloss_bwd(s, Vs, t, Va, label, st, kd_w, ce_w, seg_id, ks, cs, ds)
        assert bool(torch.isnan(ds_buf[:, Vs:].float()).all()), f"{name}: wrote past Vs"
        assert bool(torch.isfinite(ds.float()).all()), f"{name}: non-finite gradient"
        grad, scale, lse = LR.rowloss_grad(s, Vs, t, Va, label, kd_w, ce_w, seg_id, ks, cs)
        # bf16(fp32 value): half a bf16 ulp, plus the fp32 value's error: __expf(s - lse) with lse off by a few fp32 ulp of
        # the row's logit scale, at the gradient's natural scale |ckd| (q_a + p) + |cce| (q_full + [v == label]).
        # Measured: 1.71 (extra-slice, R = 4096).
        u = ulp_bf16(grad) + U32 * ref["lse_scale"][:, None] * scale
        report(name, (ds.double() - grad).abs(), u, 4.0)
        del grad, scale
        # in place over the student logits: bit-identical to the separate output; the padding past Vs is untouched
        s2_buf = torch.full((R, s.stride(0)), NAN, device=DEV, dtype=BF)
        s2 = s2_buf[:, :Vs]
        s2.copy_(s)
        K.rowloss_bwd(s2, Vs, t, Va, label, st, kd_w, ce_w, seg_id, ks, cs)
        assert torch.equal(bits(s2), bits(ds)), f"{name}: in-place result differs from ds"
        assert bool(torch.isnan(s2_buf[:, Vs:].float()).all()), f"{name}: in place, wrote past Vs"
        del s2, s2_buf, ds_buf


def test_rowloss_fwd_past_2e32_elements():
    """R = 28300 rows of 151936 columns: row * ld_s passes 2^32 elements (8.6 GB per bf16 tensor), the teacher's too."""
    Vs, Va, _, _, ld_t = GEOMS["qwen-strided-teacher"]
    R = 28300
    assert (R - 1) * Vs > 2 ** 32
    s = make_rows(R, Vs, Vs, Va, 5, False, 0, chunk=1024)
    t = make_rows(R, Va, ld_t, Va, 6, True, 0, chunk=1024)
    label = make_labels(s, Vs, Va)
    st = K.rowloss_fwd(s, Vs, t, Va, label)
    ref = LR.rowloss_stats(s, Vs, t, Va, label)
    check_stats(st, ref, s, Va, "fwd R=28300")


# ------------------------------------------------------------------------------------------ segment sums
@pytest.mark.parametrize("col", [0, 5])
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("nseg", [1, 16, 256])
def test_segment_wsum_vs_fp64(nseg, weighted, col):
    lens = [0, 1, 255, 256, 257, 2048, 32768]
    ln = [32768] if nseg == 1 else [lens[(b * 3 + col) % len(lens)] for b in range(nseg)]
    off = torch.tensor([0] + ln, device=DEV).cumsum(0).to(torch.int32)
    N = int(off[-1])
    vals = _randn(N, 8, nseg + col) * 4 + 1.0                          # a stats-like [N, 8] table, stride 8
    w = (torch.rand(N, generator=torch.Generator(device=DEV).manual_seed(N), device=DEV) > 0.3).float() if weighted else None
    out, outw = K.segment_wsum(vals, col, w, off)
    ref, refw, sc = LR.segment_sums(vals[:, col], w, off)
    # per-thread fp32 sums over <= 128 rows, then a 64-lane butterfly and 4 waves, in fp32 ulp of sum |w v|.  Measured: 0.71.
    report(f"segment_wsum nseg={nseg} w={weighted} col={col}", (out.double() - ref).abs(), sc * U32 + 1e-300, 8)
    assert torch.equal(outw.double(), refw), "segment_wsum: weight sums are integers below 2^24, exact"
    empty = torch.tensor(ln, device=DEV) == 0
    assert bool((out[empty] == 0).all()) and bool((outw[empty] == 0).all())


# ------------------------------------------------------------------------------------------ DPO
def dpo_inputs(B, beta, seed):
    """fp32 per-sample log-prob sums around -200 with z = (pc - pr) - (rc - rr) spread so that |beta z| reaches ~100."""
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    rc = torch.randn(B, generator=g, device=DEV) * 50 - 200
    rr = torch.randn(B, generator=g, device=DEV) * 50 - 200
    d2 = torch.randn(B, generator=g, device=DEV) * 5
    z = torch.randn(B, generator=g, device=DEV) * (2.0 / beta)
    z[: (B + 1) // 2] = torch.linspace(100.0 / beta, -100.0 / beta, (B + 1) // 2, device=DEV)
    return rc + d2 + z, rr + d2, rc, rr


def check_dpo(pc, pr, rc, rr, beta, ls, lt, name, lim_loss, lim_grad):
    B = pc.numel()
    losses, cr, rj, dpc, dpr = K.dpo_loss(pc, pr, rc, rr, beta, ls, lt)
    rl, rcr, rrj, rdpc, rdpr = LR.dpo(pc, pr, rc, rr, beta, ls, lt)
    b = float(torch.tensor(beta, dtype=torch.float32))
    a4 = pc.double().abs() + pr.double().abs() + rc.double().abs() + rr.double().abs()   # what z's roundings scale with
    if lt == "kto_pair":
        zs = torch.cat([a4, a4]) + a4.mean()
        slope, curv, n = b / 4, b * b / 4, 2 * B
    elif lt == "ipo":
        u = ((pc.double() - pr.double()) - (rc.double() - rr.double())) - 1 / (2 * b)
        zs = a4 + 1 / b
        slope, curv, n = 2 * u.abs(), 2.0, B
    else:
        zs = a4
        slope, curv, n = b, (b * b / 4 if lt == "sigmoid" else 0.0), B
    cross = b / n if lt in ("sigmoid", "kto_pair") else 0.0      # terms that cancel: sigmoid's label smoothing, kto's means
    lsc = (rl.abs() + slope * zs + 1e-30) * U32
    report(f"{name} losses", (losses.double() - rl).abs(), lsc, lim_loss)
    gz = zs[:B] if lt == "kto_pair" else zs
    for nm, got, ref in (("d_pc", dpc, rdpc), ("d_pr", dpr, rdpr)):
        gsc = (ref.abs() + cross + curv * gz / n + 1e-30) * U32
        report(f"{name} {nm}", (got.double() - ref).abs(), gsc, lim_grad)
    for nm, got, ref, (x, y) in (("chosen_rewards", cr, rcr, (pc, rc)), ("rejected_rewards", rj, rrj, (pr, rr))):
        # beta (x - y) in fp32: two roundings.  Measured: 1.51.
        report(f"{name} {nm}", (got.double() - ref).abs(), b * (x.double().abs() + y.double().abs()) * U32, 4)
    return losses, dpc, dpr


# (losses, gradients) limits in fp32 ulp of check_dpo's scales.  Measured (losses, d_pc / d_pr): sigmoid 1.36, 0.58;
# hinge 0.93, 0.99; ipo 1.34, 1.03; kto_pair 0.21, 0.15.
DPO_LIMITS = {"sigmoid": (16, 8), "hinge": (8, 8), "ipo": (16, 16), "kto_pair": (2, 2)}
DPO_CASES = [(B, lt, beta, 0.0) for B in (1, 2, 255, 256) for lt in ("sigmoid", "hinge", "ipo", "kto_pair")
             for beta in (0.01, 0.1, 0.5)] + [(B, "sigmoid", beta, 0.1) for B in (1, 2, 255, 256) for beta in (0.01, 0.1, 0.5)]


@pytest.mark.parametrize("B,lt,beta,ls", DPO_CASES)
def test_dpo_loss_vs_fp64(B, lt, beta, ls):
    pc, pr, rc, rr = dpo_inputs(B, beta, seed=B * 7 + int(beta * 100))
    # z's three fp32 roundings at |pc| + |pr| + |rc| + |rr| times the loss's slope, __expf and log1pf; kto_pair adds the
    # batch means (DPO_LIMITS).
    check_dpo(pc, pr, rc, rr, beta, ls, lt, f"dpo B={B} {lt} beta={beta} ls={ls}", *DPO_LIMITS[lt])


def test_dpo_loss_edges():
    """Hinge exactly at 1 - beta z = 0 (torch's relu passes no gradient there); kto_pair with the chosen and / or rejected
    batch mean exactly 0 (torch's clamp(min=0) passes the gradient at equality).  Integer-valued inputs: exact in fp32."""
    rc = torch.tensor([-10.0, -12.0, -30.0, -8.0], device=DEV)
    rr = torch.tensor([-12.0, -11.0, -20.0, -9.0], device=DEV)
    pc = rc + torch.tensor([4.0, 1.0, 3.0, 0.0], device=DEV)
    pr = rr + torch.tensor([2.0, 5.0, -1.0, 0.0], device=DEV)           # row 0: z = 2, beta 0.5: exactly at the hinge
    losses, dpc, dpr = check_dpo(pc, pr, rc, rr, 0.5, 0.0, "hinge", "dpo hinge kink", *DPO_LIMITS["hinge"])
    assert float(losses[0]) == 0.0 and float(dpc[0]) == 0.0 and float(dpr[0]) == 0.0
    for name, dc, dr in (("both", [1.0, -1.0, 2.0, -2.0], [3.0, -3.0, 0.5, -0.5]),
                         ("chosen", [1.0, -1.0, 2.0, -2.0], [3.0, -1.0, 0.5, 1.5]),
                         ("rejected", [1.0, 3.0, 2.0, -2.0], [3.0, -3.0, 0.5, -0.5])):
        pc = rc + torch.tensor(dc, device=DEV)
        pr = rr + torch.tensor(dr, device=DEV)
        check_dpo(pc, pr, rc, rr, 0.5, 0.0, "kto_pair", f"dpo kto_pair mean0 {name}", *DPO_LIMITS["kto_pair"])


# ------------------------------------------------------------------------------------------ materialising helpers
def softmax_input(R, seed):
    """fp32 [R, 152064] logits read as [:, :151936]; columns past Va are NaN (never read).  Row r % 4: 0 -inf at column 0,
    1 the first 256 columns -inf (every thread's first element), 2 every column of thread 5 -inf, 3 finite."""
    x = _randn(R, VQ, seed) * 3
    x[:, VA:] = NAN
    r = torch.arange(R, device=DEV)
    x[r % 4 == 0, 0] = NINF
    x[(r % 4 == 1).nonzero().squeeze(1)[:, None], torch.arange(256, device=DEV)[None]] = NINF
    x[(r % 4 == 2).nonzero().squeeze(1)[:, None], torch.arange(5, VA, 256, device=DEV)[None]] = NINF
    x[r % 4 != 3, 1000] = NINF
    return x


@pytest.mark.parametrize("log", [False, True])
@pytest.mark.parametrize("R", [1, 7, 300])
def test_row_softmax_f32_vs_fp64(R, log):
    x = softmax_input(R, seed=R)
    out = K.row_softmax_f32(x, VA, log)
    ref = LR.softmax(x, VA, log)
    inf = torch.isinf(x[:, :VA])
    assert bool((out[inf] == (NINF if log else 0.0)).all()), "row_softmax_f32: -inf entries"
    assert bool(torch.isfinite(out[~inf]).all()), "row_softmax_f32: non-finite output"
    xd = x[:, :VA].double().masked_fill(inf, 0).abs()
    lse = torch.logsumexp(x[:, :VA].double(), -1, keepdim=True).abs()
    # x - lse with lse off by a few fp32 ulp of the row scale; softmax: then __expf.  Measured: 3.7 (softmax), 2.4 (log).
    sc = (1 + xd + lse) * (1.0 if log else ref.abs())
    report(f"row_softmax_f32 R={R} log={log}", (out.double() - ref).abs().masked_fill(inf, 0), sc * U32, 32)


@pytest.mark.parametrize("R", [1, 7, 300])
def test_rowdot_masked_vs_fp64(R):
    lp = LR.softmax(softmax_input(R, seed=R + 1), VA, True).float()          # -inf where the student logit is -inf
    p = LR.softmax(_randn(R, VA, R + 2) * 3, VA, False).float()
    x = K.rowdot_masked(p, lp)
    ref, sc = LR.rowdot_masked(p, lp)
    # per-thread fp32 sums of ~594 products, 64-lane butterfly, 4 waves, in fp32 ulp of sum |p lp|.  Measured: 14.5.
    report(f"rowdot_masked R={R}", (x.double() - ref).abs(), sc * U32, 64)


def test_row_argmax_exact():
    """First maximum wins across lanes, waves and a lane's own columns; NaN never wins; no value > -inf gives 0.  Columns
    [V, ld) hold +100 and must never be read."""
    V, ld, R = VQ, VQ + 64, 2048
    buf = (_randn(R, ld, 9) * 3).to(BF)
    buf[:, V:] = 100.0
    x = buf[:, :V]
    x[1, [70000, 1000]] = 50.0                  # tie: thread 112 (wave 1) vs thread 232 (wave 3): 1000 wins
    x[2, [7, 263, 70001]] = 50.0                # tie inside thread 7's own columns: 7
    x[3, [151999, 300, 200]] = 50.0             # 200 (thread 200, wave 3, first pass) beats 300 (thread 44, wave 0)
    x[4] = NINF
    x[5, :11] = NAN
    x[5, 4999] = NAN
    x[5, 5000] = 50.0
    x[6] = NAN
    x[7] = NINF
    x[7, ::3] = NAN
    x[8, V - 1] = 50.0
    x[9] = NINF
    x[9, 150000] = -3.0
    out = K.row_argmax(x)
    ref = LR.argmax(x)
    assert ref[:10].tolist()[1:] == [1000, 7, 200, 0, 5000, 0, 0, V - 1, 150000]
    assert torch.equal(out.long(), ref), f"row_argmax: {int((out.long() != ref).sum())} rows differ"


# ------------------------------------------------------------------------------------------ C-ABI refusals
def test_loss_abi_refusals_and_empty():
    from llavamod import _hip
    lib = _hip.load()
    stream = torch.cuda.current_stream().cuda_stream
    s = torch.zeros(4, 64, device=DEV, dtype=BF)
    t = torch.zeros(4, 64, device=DEV, dtype=BF)
    stats = torch.full((4, 8), 7.0, device=DEV)
    ds = torch.zeros(4, 64, device=DEV, dtype=BF)
    w = torch.ones(4, device=DEV)
    sc = torch.ones(1, device=DEV)

    def fwd(Vs=64, Va=64, ld_s=64, ld_t=64, R=4, tp=t):
        return lib.lmod_rowloss_fwd(s.data_ptr(), ld_s, Vs, tp.data_ptr() if tp is not None else None, ld_t, Va, None,
                                    stats.data_ptr(), R, stream)

    def bwd(Vs=64, Va=64, ld_s=64, ld_t=64, ld_ds=64, R=4):
        return lib.lmod_rowloss_bwd(s.data_ptr(), ld_s, Vs, t.data_ptr(), ld_t, Va, None, stats.data_ptr(), w.data_ptr(), None,
                                    None, sc.data_ptr(), None, ds.data_ptr(), ld_ds, R, stream)

    for f in (fwd, bwd):
        assert f(Va=72) == -1                       # Va > Vs
        assert f(Va=60) == -1 and f(Vs=60, Va=56) == -1     # Va % 8, Vs % 8
        assert f(ld_s=68) == -1 and f(ld_t=60) == -1        # ld_s % 8, ld_t % 8
        assert f(R=0) == 0                          # empty: nothing launched
    assert fwd(ld_t=60, tp=None) == 0 and bwd(ld_ds=60) == -1
    torch.cuda.synchronize()
    stats.fill_(7.0)
    assert fwd(R=0) == 0 and bwd(R=0) == 0
    torch.cuda.synchronize()
    assert bool((stats == 7.0).all()) and bool((ds == 0).all())
    v = torch.zeros(3, device=DEV)

    def dpo(B=3, lt=0):
        return lib.lmod_dpo_loss(*(v.data_ptr(),) * 4, B, 0.1, 0.0, lt, *(v.data_ptr(),) * 5, stream)

    assert dpo(B=257) == -1 and dpo(lt=4) == -1 and dpo(B=0) == -1 and dpo(lt=-1) == -1
    out = torch.full((2,), -5, device=DEV, dtype=torch.int32)
    assert lib.lmod_row_argmax_bf16(s.data_ptr(), 64, 64, out.data_ptr(), 0, stream) == 0
    assert lib.lmod_row_softmax_f32(stats.data_ptr(), 8, 8, 0, stats.data_ptr(), 0, stream) == 0
    assert lib.lmod_rowdot_masked(stats.data_ptr(), stats.data_ptr(), 8, 0, v.data_ptr(), stream) == 0
    torch.cuda.synchronize()
    assert bool((out == -5).all()) and bool((stats == 7.0).all())
