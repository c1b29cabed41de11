"""Sampling on the device: lmod_sample_bf16 (temperature / top-k / top-p filter + inverse-CDF draw, llava-mod_amd/csrc/sample.hip)
against the fp64 reference of tests/_sample_ref.py, and generate(do_sample=True) on top of it.

Bounds.  The reference works in fp64 on the exact bf16 logits; the kernel evaluates exp in fp32.  What fp32 costs on a given row is
measured, not assumed: floor = max |cdf_fp32 - cdf_fp64| with the fp32 CDF a plain torch evaluation (softmax, cumsum) of the same
row: neither side is the code under test.  delta = 2 * floor (the project's standing rule: two times a measured noise floor),
floored at 1e-6; both are printed per case.
  * filter: n_kept == count(logit >= kernel cutoff) exactly; the kernel's cutoff lies between the reference's cutoffs at
    top_p + delta and top_p - delta; for top-k alone (and no filter) cutoff and count are exact; lse and the kept fraction agree
    with fp64 within 2e-6 * |lse| + 1e-6 (test_beam_topk_vs_torch's bound);
  * draw: every one of 4096 stratified uniforms (+ u = 0 and the largest fp32 below 1) per row is checked: the token lies in the
    reference's kept set at top_p + delta, and cdf_lo(t) - delta <= u <= cdf_hi(t) + delta on the fp64 token-order CDF of the
    reference's kept set.  Where the kernel's cutoff is inside the bracket but not the reference's own at top_p (a cumulative mass
    within delta of top_p), the fp64 CDF and kept fraction are taken over the threshold set at the kernel's cutoff: the set the
    bracket admits.  No case and no draw is excluded.

Measured on an MI355X (all 756 cases of each test): the fp32 floor is 3.1e-8 .. 2.4e-6 at V >= 151936 and 1.0e-9 .. 4.2e-7 at
V <= 1003, so delta is 1.0e-6 .. 4.7e-6; the worst |u - token interval| over all draws is 8.0e-9, the worst kept-fraction error
3.6e-8, the worst lse error 7.3e-6 (at T = 0.2, where |lse| is in the hundreds), and no row sat at the edge of its bracket.
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
from test_generate_gpu import _pair, _prompt  # noqa: E402

DEV = "cuda"
BF = torch.bfloat16
SHAPES = [(512, 512), (1000, 1000), (1001, 1001), (1003, 1008), (151936, 151936), (151936, 152064), (152064, 152064)]
FILTERS = [(None, None), (50, None), (None, 0.7), (None, 0.9), (50, 0.7), (50, 0.9)]
TEMPS = (0.2, 1.0, 1.5)
SCALES = (3.0, 8.0)
NSTRATA = 4096


def _logits(V, ld, R, s, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return (s * torch.randn(R, ld, device=DEV, generator=g)).to(BF)[:, :V]


def _noise_floor(logits, T):
    """max |cdf_fp32 - cdf_fp64| over the rows: what a plain fp32 evaluation of this warped row loses."""
    t = max(float(np.float32(T)), 1e-6)
    c32 = torch.softmax(logits.float() / t, -1).cumsum(-1)
    c64 = torch.softmax(logits.double() / t, -1).cumsum(-1)
    floor = (c32.double() - c64).abs().max().item()
    return floor, max(2.0 * floor, 1e-6)


def _eval_keep(logits, T, k, p, cut_kernel):
    """The reference's kept set; on a row whose kernel cutoff differs from the reference's at top_p itself (admitted by the
    bracket), the threshold set at the kernel's cutoff."""
    keep = SR.keep_mask(logits, T, k, p)
    cut_ref, _ = SR.cutoff_and_count(logits, T, k, p)
    same = cut_ref == cut_kernel.double()
    thr = logits.double() >= cut_kernel.double()[:, None]
    return torch.where(same[:, None], keep, thr), same


def _check_filter(logits, T, k, p, tok, st, delta, tag):
    R, V = logits.shape
    lv = logits.double()
    cut = st[:, 3].double()
    n_kept = st[:, 2].double()
    assert not torch.isnan(st).any(), tag
    assert torch.all((tok >= 0) & (tok < V)), tag
    assert torch.equal(n_kept, (lv >= cut[:, None]).sum(-1).double()), (tag, "n_kept != count(x >= cutoff)")
    if p is None or p >= 1.0:
        cut_ref, n_ref = SR.cutoff_and_count(logits, T, k, p)
        assert torch.equal(cut, cut_ref) and torch.equal(n_kept, n_ref.double()), (tag, "top-k cutoff / count not exact")
    else:
        lo_cut, _ = SR.cutoff_and_count(logits, T, k, min(p + delta, 1.0))
        hi_cut, _ = SR.cutoff_and_count(logits, T, k, max(p - delta, 0.0))
        assert torch.all(lo_cut <= cut) and torch.all(cut <= hi_cut), (tag, lo_cut.tolist(), cut.tolist(), hi_cut.tolist())
    keep, same = _eval_keep(logits, T, k, p, st[:, 3])
    x = SR.scaled(logits, T)
    m = x.max(-1, keepdim=True).values
    w = torch.exp(x - m)
    lse = m.squeeze(-1) + torch.log(w.sum(-1))
    frac = torch.where(keep, w, torch.zeros_like(w)).sum(-1) / w.sum(-1)
    tol = 2e-6 * lse.abs().max().item() + 1e-6
    e_lse = (st[:, 0].double() - lse).abs().max().item()
    e_frac = (st[:, 1].double() - frac).abs().max().item()
    assert e_lse <= tol and e_frac <= tol, (tag, e_lse, e_frac, tol)
    assert torch.all(lv.gather(1, tok.long()[:, None]).squeeze(1) >= cut), (tag, "token outside the kept set")
    return e_lse, e_frac, int((~same).sum())


@pytest.mark.parametrize("V,ld", SHAPES)
@pytest.mark.parametrize("R", [1, 3, 16])
def test_sample_filter_and_stats_vs_fp64(V, ld, R):
    from llavamod import kernels as K
    for s in SCALES:
        logits = _logits(V, ld, R, s, V + 31 * R + int(s))
        g = torch.Generator(device=DEV).manual_seed(R + V)
        for T in TEMPS:
            floor, delta = _noise_floor(logits, T)
            for k, p in FILTERS:
                u = torch.rand(R, device=DEV, generator=g)
                tok, st = K.sample(logits, u, T, k, p, stats=True)
                tag = f"V={V} ld={ld} R={R} s={s} T={T} top_k={k} top_p={p}"
                e_lse, e_frac, moved = _check_filter(logits, T, k, p, tok, st, delta, tag)
                print(f"{tag}: floor={floor:.3e} delta={delta:.3e} err_lse={e_lse:.2e} err_frac={e_frac:.2e} "
                      f"n_kept={st[:, 2].int().tolist()[:4]} rows_at_bracket_edge={moved}")


def _strata():
    u = (torch.arange(NSTRATA, dtype=torch.float64) + 0.5) / NSTRATA
    u = torch.cat([u, torch.tensor([0.0, float(np.nextafter(np.float32(1), np.float32(0)))], dtype=torch.float64)])
    return u.to(torch.float32)                                   # every value is exact in fp32


@pytest.mark.parametrize("V,ld", SHAPES)
@pytest.mark.parametrize("R", [1, 3, 16])
def test_sample_every_draw_vs_fp64_cdf(V, ld, R):
    """Each row replicated to 4096 + 2 rows (4 distinct rows per call), stratified uniforms, every returned token checked."""
    from llavamod import kernels as K
    us = _strata().to(DEV)
    n = us.numel()
    for s in SCALES:
        logits = _logits(V, ld, R, s, V + 31 * R + int(s))
        for T in TEMPS:
            floor, delta = _noise_floor(logits, T)
            for k, p in FILTERS:
                tag = f"V={V} ld={ld} R={R} s={s} T={T} top_k={k} top_p={p}"
                worst = 0.0
                for r0 in range(0, R, 4):
                    rows = logits[r0:r0 + 4]
                    nr = rows.shape[0]
                    rep = torch.empty(nr * n, ld, device=DEV, dtype=BF)[:, :V]
                    rep.unflatten(0, (nr, n)).copy_(rows[:, None, :].expand(nr, n, V))
                    tok, st = K.sample(rep, us.repeat(nr), T, k, p, stats=True)
                    tok, st = tok.view(nr, n).long(), st.view(nr, n, 4)
                    assert torch.all((tok >= 0) & (tok < V)), tag
                    assert torch.equal(st, st[:, :1].expand_as(st)), (tag, "stats differ between copies of one row")
                    keep, _ = _eval_keep(rows, T, k, p, st[:, 0, 3])
                    if p is not None and p < 1.0:
                        cut_plus, _ = SR.cutoff_and_count(rows, T, k, min(p + delta, 1.0))
                    else:
                        cut_plus, _ = SR.cutoff_and_count(rows, T, k, p)
                    lo, hi = SR.kept_cdf(rows, T, keep)
                    drawn = rows.double().gather(1, tok)
                    assert torch.all(drawn >= cut_plus[:, None]), (tag, "token outside the kept set at top_p + delta")
                    ud = us.double()[None, :]
                    under = (lo.gather(1, tok) - ud).clamp_min(0).max().item()     # u below the token's interval
                    over = (ud - hi.gather(1, tok)).clamp_min(0).max().item()      # u above it
                    worst = max(worst, under, over)
                    assert under <= delta and over <= delta, (tag, under, over, delta)
                print(f"{tag}: floor={floor:.3e} delta={delta:.3e} worst |u - interval|={worst:.3e}")


def test_sample_is_bit_reproducible():
    from llavamod import kernels as K
    logits = _logits(151936, 151936, 16, 3.0, 99)
    u = torch.rand(16, device=DEV, generator=torch.Generator(device=DEV).manual_seed(1))
    for k, p in FILTERS:
        a, sa = K.sample(logits, u, 1.5, k, p, stats=True)
        for _ in range(3):
            b, sb = K.sample(logits, u, 1.5, k, p, stats=True)
            assert torch.equal(a, b) and torch.equal(sa.view(torch.int32), sb.view(torch.int32)), (k, p)


@pytest.mark.parametrize("V,ld", [(1003, 1008), (151936, 151936)])
def test_sample_edge_rows(V, ld):
    from llavamod import kernels as K
    ninf = float("-inf")
    us = _strata().to(DEV)
    n = us.numel()
    # -inf everywhere except two entries: p = e / (e + 1) for the logit 1, 1 / (e + 1) for the logit 0
    a, b = V // 3, V - 2
    row = torch.full((1, ld), ninf, device=DEV, dtype=BF)[:, :V]
    row[0, a], row[0, b] = 0.0, 1.0
    rep = row.expand(n, V).contiguous()
    for k, p in FILTERS:
        tok, st = K.sample(rep, us, 1.0, k, p, stats=True)
        assert not torch.isnan(st).any()
        ref = SR.draw(rep[:1].expand(n, V), us, 1.0, k, p)
        cut = 1.0 / (1.0 + np.e)
        away = (us.double() - cut).abs() > 1e-6
        assert set(tok.tolist()) <= {a, b} and torch.equal(tok.long()[away], ref[away]), (k, p)
        assert abs(st[0, 0].item() - np.log(1 + np.e)) <= 2e-6 * np.log(1 + np.e) + 1e-6
    # no finite logit: token 0, lse -inf, kept fraction 0, nothing NaN
    row = torch.full((3, ld), ninf, device=DEV, dtype=BF)[:, :V]
    for k, p in FILTERS:
        tok, st = K.sample(row, us[:3].contiguous(), 1.0, k, p, stats=True)
        assert tok.tolist() == [0, 0, 0] and not torch.isnan(st).any(), (k, p, tok.tolist(), st.tolist())
        assert torch.all(st[:, 0] == ninf) and torch.all(st[:, 1] == 0)
    # a constant row: every token ties, top_p = 0.5 keeps all V by the tie rule, the draw is uniform over token ids
    row = torch.full((1, ld), 0.75, device=DEV, dtype=BF)[:, :V]
    rep = row.expand(n, V).contiguous()
    tok, st = K.sample(rep, us, 0.7, None, 0.5, stats=True)
    assert torch.all(st[:, 2] == V) and torch.all(st[:, 3] == 0.75) and torch.all((st[:, 1] - 1).abs() <= 1e-6)
    assert torch.all((tok.long() - torch.floor(us.double() * V).long()).abs() <= 1)
    # top_k = 1 is the arg-max on rows whose maximum is not tied
    logits = _logits(V, ld, 16, 8.0, 5)
    top2 = torch.topk(logits.float(), 2, dim=-1).values
    clear = top2[:, 0] > top2[:, 1]
    assert int(clear.sum()) >= 8
    tok = K.sample(logits, torch.rand(16, device=DEV), 1.0, 1, None)
    assert torch.equal(tok[clear], K.row_argmax(logits)[clear])
    tok = K.sample(logits, torch.rand(16, device=DEV), 0.2, 1, 0.7)
    assert torch.equal(tok[clear], K.row_argmax(logits)[clear])
    # top_p <= 0 through the raw kernel wrapper keeps the maximum
    tok, st = K.sample(logits, torch.rand(16, device=DEV), 1.0, None, 0.0, stats=True)
    assert torch.equal(tok[clear], K.row_argmax(logits)[clear]) and torch.all(st[clear, 2] == 1)


def test_sample_argument_checks():
    from llavamod import _hip
    lib = _hip.load()
    V = 64
    x = torch.zeros(4, V, device=DEV, dtype=BF)
    u = torch.zeros(4, device=DEV)
    ws = torch.zeros(1 << 20, device=DEV, dtype=torch.uint8)
    out = torch.full((4,), -7, device=DEV, dtype=torch.int32)
    stream = torch.cuda.current_stream().cuda_stream

    def run(ld=V, v=V, r=4, chunk=64, ws_bytes=ws.numel(), top_k=0, top_p=1.0):
        return lib.lmod_sample_bf16(x.data_ptr(), ld, v, u.data_ptr(), r, ctypes.c_float(1.0), top_k, ctypes.c_float(top_p), chunk,
                                    ws.data_ptr(), ws_bytes, out.data_ptr(), None, stream)

    assert run(r=65536) == -1 and run(v=1) == -1 and run(ld=V - 1) == -1
    assert run(chunk=0) == -1 and run(chunk=4) == -1 and run(chunk=12) == -1
    assert run(ws_bytes=4 * (64 + 16) - 1) == -1 and run(ws_bytes=4 * (64 + 2 * 3072 + 16) - 1, top_k=5) == -1
    assert run(ws_bytes=4 * (64 + 3 * 3072 + 16) - 1, top_k=5, top_p=0.5) == -1
    assert run(r=0) == 0
    torch.cuda.synchronize()
    assert out.tolist() == [-7] * 4                               # nothing ran
    assert run(ws_bytes=4 * (64 + 16)) == 0 and run(ws_bytes=4 * (64 + 3 * 3072 + 16), top_k=5, top_p=0.5) == 0
    torch.cuda.synchronize()
    assert out.tolist() == [0] * 4                                # u = 0 on a constant row: the first token


def test_generate_sampling_on_device():
    """generate(do_sample=True): num_return_sequences continuations per prompt from one prefill, seed-reproducible, top_k = 1 is
    greedy, token_logprobs from the kernel's stats against the fp64 reference on the prefill logits, log-probabilities 0 after EOS,
    greedy refuses num_return_sequences > 1, and the torch path (sample_on_device = False) still runs."""
    _, teacher = _pair()
    p = _prompt()
    B = p["input_ids"].shape[0]
    a = teacher.generate(**p, max_new_tokens=6, do_sample=True, temperature=1.5, num_return_sequences=3, seed=5)
    assert a.shape == (B * 3, 6) and a.dtype == torch.int64
    for b in range(B):
        r = a[3 * b:3 * b + 3]
        assert not torch.equal(r[0], r[1]) and not torch.equal(r[0], r[2]) and not torch.equal(r[1], r[2]), (b, r)
    assert torch.equal(a, teacher.generate(**p, max_new_tokens=6, do_sample=True, temperature=1.5, num_return_sequences=3, seed=5))
    assert not torch.equal(a, teacher.generate(**p, max_new_tokens=6, do_sample=True, temperature=1.5, num_return_sequences=3, seed=6))
    greedy = teacher.generate(**p, max_new_tokens=6)
    top1 = teacher.generate(**p, max_new_tokens=6, do_sample=True, top_k=1, num_return_sequences=2, seed=1)
    assert torch.equal(top1, greedy.repeat_interleave(2, 0))
    one = teacher.generate(**p, max_new_tokens=6, do_sample=True, temperature=1.5, top_p=0.9, seed=11)
    assert one.shape == (B, 6)                                     # n = 1 keeps the shapes
    # return_dict_in_generate: log-probabilities of the drawn tokens under the warped distribution
    out = teacher.generate(**p, max_new_tokens=5, do_sample=True, temperature=1.5, top_p=0.9, num_return_sequences=2, seed=7,
                           return_dict_in_generate=True)
    assert out.sequences.shape == (B * 2, 5) and out.sequences.dtype == torch.int64
    assert out.token_logprobs.shape == (B * 2, 5) and out.token_logprobs.dtype == torch.float32
    assert torch.all(out.token_logprobs <= 0) and torch.all(torch.isfinite(out.token_logprobs))
    _, logits = teacher._prefill(p["input_ids"], p["attention_mask"], p["images"], 1)
    logits = logits.repeat_interleave(2, 0)
    ref = SR.warped_logprob(logits, out.sequences[:, 0], 1.5, None, 0.9)
    lse, _ = SR.stats(logits, 1.5, None, 0.9)
    tol = 2e-6 * lse.abs().max().item() + 1e-6
    err = (out.token_logprobs[:, 0].double() - ref).abs().max().item()
    print(f"token_logprobs first column: err={err:.3e} tol={tol:.3e}")
    assert err <= tol, (err, tol)
    # EOS: the same seed draws the same tokens; after a row's EOS the tokens are pad and the log-probabilities 0
    eos = int(out.sequences[0, 2])
    out2 = teacher.generate(**p, max_new_tokens=5, do_sample=True, temperature=1.5, top_p=0.9, num_return_sequences=2, seed=7,
                            return_dict_in_generate=True, eos_token_id=eos, pad_token_id=3)
    first = int((out.sequences[0] == eos).nonzero()[0])
    assert torch.equal(out2.sequences[0, :first + 1], out.sequences[0, :first + 1])
    assert torch.all(out2.sequences[0, first + 1:] == 3) and torch.all(out2.token_logprobs[0, first + 1:] == 0)
    assert torch.equal(out2.token_logprobs[0, :first + 1], out.token_logprobs[0, :first + 1])
    with pytest.raises(ValueError, match="num_return_sequences"):
        teacher.generate(**p, max_new_tokens=2, num_return_sequences=2)
    with pytest.raises(ValueError, match="temperature"):
        teacher.generate(**p, max_new_tokens=2, do_sample=True, temperature=0.0)
    # the torch path (the A/B baseline) still runs and draws from the same nucleus
    teacher.sample_on_device = False
    try:
        old = teacher.generate(**p, max_new_tokens=6, do_sample=True, temperature=1.5, top_p=0.9, seed=11)
    finally:
        del teacher.sample_on_device
    assert old.shape == (B, 6)
    _, logits = teacher._prefill(p["input_ids"], p["attention_mask"], p["images"], 1)
    cut, _ = SR.cutoff_and_count(logits, 1.5, None, 0.9 + 1e-5)    # 1e-5: the fp32 noise of the torch path's own softmax / cumsum
    assert torch.all(logits.double().gather(1, old[:, :1]).squeeze(1) >= cut)
    assert torch.all(logits.double().gather(1, one[:, :1]).squeeze(1) >= cut)
