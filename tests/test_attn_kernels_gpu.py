"""Attention kernels (attn_fwd2.hip, attn_bwd2.hip, the delta / head-split reduce / decode kernels of attn.hip, the dS-spill dQ GEMM)
against the fp64 restatement of tests/_attn_ref.py, every element of every output, with per-element bounds:

    bf16 outputs   |out - ref| <= 1/2 ulp_bf16(ref) + L u        (u: the element's unit, _attn_ref's module docstring)
    lse            |out - ref| <= L_lse 2^-24 u_lse
    unit == 0      the element is exactly 0 (rows without a visible key, keys >= len); lse of such a row exactly -inf

L = 4 x the rounding model's largest error (tests/test_attn_ref_cpu.py; _attn_ref.LIMITS): O 0.0104, dQ 0.0092, dK 0.0108, dV 0.0148,
lse 10.4.  Each case prints `ATTN-ERR <case> <output> <max err/unit> <limit>`.

Every case lives in canary buffers: Q | K | V are column blocks of one fused buffer whose row stride exceeds the live width, with NaN
in the unused columns and in guard rows before and after; dO likewise; O, dQ | dK | dV, lse and delta are views into buffers
pre-filled with a bit pattern, with ldo / lddq / lddk / lddv larger than the live width.  After the launches every byte outside the live
regions still holds the pattern and no NaN reached an output.  Every launch is run twice and must be bit-identical.  All canary
regions are inside allocations this file owns.

Backward forms, each against fp64 by name, each asserting the form it took:
    two      lmod_attn_bwd without a workspace: the dK/dV kernel + the dQ kernel, unsplit
    split    lmod_attn_bwd_split with the head-split workspace; lmod_attn_bwd_nsplit(...) > 1 asserted
    spill    lmod_attn_bwd_split with the dS workspace (filled with NaN first); nsplit == 1 and attn_bwd_ds_fusable asserted
    rope     lmod_attn_bwd_rope (two-kernel form + the RoPE gradient map in the epilogues)
    sprope   dS spill + the RoPE gradient map in the dQ GEMM's epilogue (fused RoPE keeps a grouped-query launch unsplit)
    packed   cu_seqlens layout, forward and backward (lmod_attn_bwd)
RoPE forms: the reference is the fp64 gradient pushed through lmod_rope's backward map dx1 = g1 cos1 + g2 sin2, dx2 = g2 cos2 - g1 sin1 in
fp64; the units go through the same map with |cos|, |sin|; the kernel rounds g, both products and the sum to bf16, so the output's own
rounding is 1/2 (ulp(g1) |cos1| + ulp(g2) |sin2| + ulp(g1 cos1) + ulp(g2 sin2) + ulp(dx1)) instead of 1/2 ulp(ref).

The table (TABLE below; B, S, heads / KV heads, hd, causal, lens, input kind, dO kind, form) is chosen so that each kernel form x mask
branch (no mask, causal diagonal, `len` inside a 32 / 64 / 256 block, whole blocks past `len`, len 0 / 1, S = 1, S % 32 != 0) x input
kind appears at least once; S in {1, 31, 32, 33, 64, 65, 255, 256, 257, 577, 1000, 2048}; the step shapes 14/2 hd 64 and 28/4 hd 128 at
B 2, S 2048 causal ragged; the CLIP tower's launch (B 3, S 577, 16 heads, hd 64, non-causal, no lse).

Measured on an MI355X, largest ATTN-ERR per output over the table, beside the limit and the rounding model's own figure:
    O    0.00258 (64-step-14/2)             limit 0.0104    model 0.00257
    dQ   0.00244 (64-S1000-c-spike-14/2)    limit 0.0092    model 0.00225
    dK   0.00239 (128-S2048-c-spike-spill)  limit 0.0108    model 0.00268
    dV   0.00373 (128-S2048-c-hot-spill)    limit 0.0148    model 0.00367
    lse  2.44    (64-S1000-c-spike-14/2)    limit 10.4      model 2.56
    decode O 4.5e-09 (dec-128-14/2-spike; 0 in the other seven cases: inside the output's own half ulp)   limit 0.0104
No shipped kernel is above a limit; every canary is intact, every form deterministic, the decode output agrees with the prefill row.
"""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

from llavamod import _hip  # noqa: E402
from llavamod import kernels as K  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _attn_ref as R  # noqa: E402

DEV = "cuda"
BF = torch.bfloat16
G = 4                       # guard rows before and after every row buffer
PADC = 64                   # unused columns behind the live width
GF = 64                     # guard floats around lse / delta
PAT16, PAT32 = 0x5A5A, 0x5A5A5A5A

# id: (B, S, nh, nkv, hd, causal, lens, kind, do_kind, form)
TABLE = {
    # ---- hd 128
    "128-S1": (2, 1, 4, 4, 128, True, None, "diffuse", "normal", "two"),
    "128-S31-c-hot": (2, 31, 4, 4, 128, True, None, "hot", "normal", "two"),
    "128-S32-nc": (2, 32, 4, 4, 128, False, None, "diffuse", "normal", "two"),
    "128-S33-c-hot-gqa": (2, 33, 4, 1, 128, True, None, "hot", "normal", "split"),
    "128-S64-nc-hot": (2, 64, 4, 4, 128, False, None, "hot", "normal", "two"),
    "128-S65-c-hot-gqa": (2, 65, 4, 1, 128, True, None, "hot", "normal", "split"),
    "128-S255-c-hot": (1, 255, 4, 4, 128, True, None, "hot", "normal", "two"),
    "128-S256-c-hot-spill": (2, 256, 4, 4, 128, True, None, "hot", "normal", "spill"),
    "128-S256-nc-two": (1, 256, 4, 4, 128, False, None, "diffuse", "normal", "two"),
    "128-S257-c-hot": (1, 257, 4, 4, 128, True, None, "hot", "normal", "two"),
    "128-S577-nc-hot-gqa": (1, 577, 4, 1, 128, False, None, "hot", "normal", "split"),
    "128-S1000-c-spike": (1, 1000, 4, 4, 128, True, None, "spike", "normal", "two"),
    "128-S1000-c-creep-gqa": (1, 1000, 4, 1, 128, True, None, "creep", "normal", "split"),
    "128-S1024-nc-creep-spill": (1, 1024, 4, 4, 128, False, None, "creep", "normal", "spill"),
    "128-S2048-c-hot-spill": (1, 2048, 4, 4, 128, True, None, "hot", "normal", "spill"),
    "128-S2048-c-diffuse-two": (1, 2048, 4, 4, 128, True, None, "diffuse", "normal", "two"),
    "128-S2048-nc-hot-gqa": (1, 2048, 4, 1, 128, False, None, "hot", "normal", "split"),
    "128-S2048-c-spike-spill": (1, 2048, 4, 4, 128, True, None, "spike", "normal", "spill"),
    "128-rag-small-c": (5, 320, 4, 4, 128, True, [0, 1, 31, 32, 33], "hot", "normal", "two"),
    "128-rag-mid-c-gqa": (5, 320, 4, 1, 128, True, [63, 64, 65, 255, 256], "hot", "normal", "split"),
    "128-rag-nc": (4, 512, 4, 4, 128, False, [257, 511, 512, 0], "hot", "normal", "two"),
    "128-rag-c-spill": (4, 512, 4, 4, 128, True, [256, 0, 511, 512], "hot", "normal", "spill"),
    "128-rag-padonly-two": (2, 320, 4, 4, 128, True, [33, 255], "diffuse", "pad_only", "two"),
    "128-rag-padonly-gqa": (2, 320, 4, 1, 128, False, [257, 64], "diffuse", "pad_only", "split"),
    "128-rope-c-gqa": (2, 300, 4, 1, 128, True, [300, 65], "hot", "normal", "rope"),
    "128-rope-nc": (1, 257, 4, 4, 128, False, None, "diffuse", "normal", "rope"),
    "128-sprope-c-gqa": (2, 512, 4, 1, 128, True, [300, 512], "hot", "normal", "sprope"),
    "128-packed-c-gqa": (5, 300, 4, 1, 128, True, [1, 31, 257, 64, 300], "hot", "normal", "packed"),
    "128-packed-nc": (3, 256, 4, 4, 128, False, [255, 256, 33], "diffuse", "normal", "packed"),
    "128-step-28/4": (2, 2048, 28, 4, 128, True, [2047, 257], "hot", "normal", "split"),
    # ---- hd 64
    "64-S1": (2, 1, 4, 4, 64, True, None, "diffuse", "normal", "two"),
    "64-S31-c-hot": (2, 31, 4, 4, 64, True, None, "hot", "normal", "two"),
    "64-S33-nc-gqa": (2, 33, 4, 1, 64, False, None, "hot", "normal", "split"),
    "64-S64-c": (2, 64, 4, 4, 64, True, None, "diffuse", "normal", "two"),
    "64-S65-c-hot": (2, 65, 4, 4, 64, True, None, "hot", "normal", "two"),
    "64-S255-nc-hot": (1, 255, 4, 4, 64, False, None, "hot", "normal", "two"),
    "64-S256-c-14/2": (1, 256, 14, 2, 64, True, None, "hot", "normal", "split"),
    "64-S257-nc-16/16": (1, 257, 16, 16, 64, False, None, "hot", "normal", "two"),
    "64-clip-577": (3, 577, 16, 16, 64, False, None, "hot", "normal", "two"),
    "64-S1000-c-spike-14/2": (1, 1000, 14, 2, 64, True, None, "spike", "normal", "split"),
    "64-S2048-c-hot": (1, 2048, 4, 4, 64, True, None, "hot", "normal", "two"),
    "64-S1024-nc-creep": (1, 1024, 4, 4, 64, False, None, "creep", "normal", "two"),
    "64-rag-small-c-14/2": (5, 320, 14, 2, 64, True, [0, 1, 31, 32, 33], "hot", "normal", "split"),
    "64-rag-mid-nc": (5, 320, 4, 4, 64, False, [63, 64, 65, 255, 257], "hot", "normal", "two"),
    "64-rag-padonly": (2, 320, 4, 1, 64, True, [33, 255], "diffuse", "pad_only", "two"),
    "64-step-14/2": (2, 2048, 14, 2, 64, True, [2048, 1000], "hot", "normal", "split"),
}
NO_LSE = {"64-clip-577"}     # the CLIP tower's forward passes lse = NULL; the backward of that case is fed by a second forward with lse


def _pattern_rows(rows, width, ld):
    """[G + rows + G, ld] bf16 buffer full of the bit pattern; returns (buffer as int16, live view [rows, width] as bf16)."""
    raw = torch.full((G + rows + G, ld), PAT16, dtype=torch.int16, device=DEV)
    return raw, raw.view(BF)[G:G + rows, :width]


def _pattern_f32(n):
    raw = torch.full((GF + n + GF,), PAT32, dtype=torch.int32, device=DEV)
    return raw, raw.view(torch.float32)[GF:GF + n]


def _outside_intact(raw, rows, width, what):
    live = torch.zeros(raw.shape, dtype=torch.bool, device=DEV)
    live[G:G + rows, :width] = True
    n = int((raw[~live] != PAT16).sum())
    assert n == 0, f"{what}: {n} elements outside the live region were written"


def _outside_intact_f32(raw, n, what):
    bad = int((raw[:GF] != PAT32).sum()) + int((raw[GF + n:] != PAT32).sum())
    assert bad == 0, f"{what}: {bad} floats outside the live region were written"


def _nan_rows(x, ld):
    """x [T, W] bf16 -> a [G + T + G, ld] buffer with NaN in the guard rows and the columns >= W, and the live view."""
    T, W = x.shape
    buf = torch.full((G + T + G, ld), float("nan"), dtype=BF, device=DEV)
    buf[G:G + T, :W] = x
    return buf, buf[G:G + T, :W]


def _rope_tables(maxpos, hd, theta=1e6):
    inv = 1.0 / (theta ** (torch.arange(0, hd, 2).float() / hd))
    fr = torch.outer(torch.arange(maxpos).float(), inv)
    emb = torch.cat((fr, fr), dim=-1)
    return emb.cos().to(BF).to(DEV), emb.sin().to(BF).to(DEV)


def _rope_bwd64(g, u, cos, sin):
    """g, u [T, n, 128] fp64 (gradient and its unit), cos / sin [T, 1, 128] fp64 -> the gradient through lmod_rope's backward map, its unit
    and the kernel's own rounding (module docstring)."""
    g1, g2, u1, u2 = g[..., :64], g[..., 64:], u[..., :64], u[..., 64:]
    c1, c2, s1, s2 = cos[..., :64], cos[..., 64:], sin[..., :64], sin[..., 64:]
    ulp = R.ulp_bf16
    dx1, dx2 = g1 * c1 + g2 * s2, g2 * c2 - g1 * s1
    ux1, ux2 = u1 * c1.abs() + u2 * s2.abs(), u2 * c2.abs() + u1 * s1.abs()
    sl1 = 0.5 * (ulp(g1) * c1.abs() + ulp(g2) * s2.abs() + ulp(g1 * c1) + ulp(g2 * s2) + ulp(dx1))
    sl2 = 0.5 * (ulp(g2) * c2.abs() + ulp(g1) * s1.abs() + ulp(g2 * c2) + ulp(g1 * s1) + ulp(dx2))
    return torch.cat((dx1, dx2), -1), torch.cat((ux1, ux2), -1), torch.cat((sl1, sl2), -1)


class Report:
    def __init__(self, case):
        self.case, self.fail = case, []

    def bf(self, name, out, ref, unit, slack=None):
        e, idx, nz = R.err_units(out, ref, unit, slack)
        lim = R.LIMITS[name]
        print(f"ATTN-ERR {self.case} {name} {e:.3g} {lim:.3g}" + (f"  NONZERO-AT-ZERO-UNIT {nz}" if nz else ""))
        if nz or not e <= lim:
            self.fail.append(f"{name}: err/unit {e:.4g} > {lim:.4g} at {idx} (out {float(out[idx]):.6g} ref {float(ref[idx]):.6g} "
                             f"unit {float(unit[idx]):.4g}); {nz} nonzero where the unit is 0")
        return e

    def lse(self, out, ref, unit):
        e, idx, nz = R.err_units_lse(out, ref, unit)
        lim = R.LIMITS["lse"]
        print(f"ATTN-ERR {self.case} lse {e:.3g} {lim:.3g}" + (f"  NOT-MINUS-INF {nz}" if nz else ""))
        if nz or not e <= lim:
            self.fail.append(f"lse: err/unit {e:.4g} > {lim:.4g} at {idx} (out {float(out[idx]):.8g} ref {float(ref[idx]):.8g}); "
                             f"{nz} rows without a visible key are not -inf")

    def done(self):
        assert not self.fail, f"{self.case}: " + " | ".join(self.fail)


def _nsplit(B, S, nh, nkv, hd, causal):
    return _hip.load().lmod_attn_bwd_nsplit(B, S, nh, nkv, hd, int(causal))


@pytest.mark.parametrize("case", list(TABLE), ids=list(TABLE))
def test_attn_fwd_bwd_against_fp64(case):
    B, S, nh, nkv, hd, causal, lens, kind, do_kind, form = TABLE[case]
    packed = form == "packed"
    rope = form in ("rope", "sprope")
    q, k, v, do, scale = R.make_case(kind, B, S, nh, nkv, hd, causal, lens, seed=len(case), do_kind=do_kind, device=DEV)
    if packed:                                         # rows >= len do not exist in the packed layout: no gradient enters through them
        do = do * (torch.arange(S, device=DEV)[None, :] < torch.tensor(lens, device=DEV)[:, None])[:, :, None, None].to(BF)
    ref = R.attn_ref64(q, k, v, do, scale, causal, lens)
    W, Wq, Wk = (nh + 2 * nkv) * hd, nh * hd, nkv * hd
    flat = torch.cat((q.reshape(B * S, Wq), k.reshape(B * S, Wk), v.reshape(B * S, Wk)), 1)
    dflat = do.reshape(B * S, Wq)
    keep = None
    seqlens = cu = None
    if packed:
        keep = torch.cat([torch.arange(L, device=DEV) + b * S for b, L in enumerate(lens)])
        flat, dflat = flat[keep], dflat[keep]
        cu = torch.tensor([0] + torch.tensor(lens).cumsum(0).tolist(), dtype=torch.int32, device=DEV)
    elif lens is not None:
        seqlens = torch.tensor(lens, dtype=torch.int32, device=DEV)
    T = flat.shape[0]
    ld = W + PADC
    _, qkv = _nan_rows(flat, ld)
    q2, k2, v2 = qkv[:, :Wq], qkv[:, Wq:Wq + Wk], qkv[:, Wq + Wk:]
    _, do2 = _nan_rows(dflat, Wq + PADC)
    rep = Report(case)

    def fwd(want_lse):
        oraw, o = _pattern_rows(T, Wq, Wq + PADC)
        lraw, lse = _pattern_f32(B * nh * S)
        _hip.call("lmod_attn_fwd", q2.data_ptr(), k2.data_ptr(), v2.data_ptr(), o.data_ptr(), lse.data_ptr() if want_lse else None,
                  _hip.ptr(seqlens), _hip.ptr(cu), B, S, nh, nkv, hd, ld, ld, ld, Wq + PADC, float(scale), int(causal))
        torch.cuda.synchronize()
        _outside_intact(oraw, T, Wq, "O")
        _outside_intact_f32(lraw, B * nh * S if want_lse else 0, "lse")
        return o, lse.view(B, nh, S)

    def rows(x, n):                                    # [T, n*hd] kernel layout -> the reference's [B, S, n, hd] (packed: zeros in the rows that do not exist)
        if not packed:
            return x.reshape(B, S, n, hd)
        full = torch.zeros(B * S, n * hd, dtype=x.dtype, device=DEV)
        full[keep] = x
        return full.reshape(B, S, n, hd)

    def packed_ref(name):                              # the padded reference restricted to the rows that exist
        if not packed:
            return ref[name], ref["u_" + name]
        m = torch.zeros(B * S, dtype=torch.bool, device=DEV)
        m[keep] = True
        m = m.reshape(B, S, 1, 1)
        return ref[name] * m, ref["u_" + name] * m

    o, lse = fwd(True)
    o_again, lse_again = fwd(True)
    assert torch.equal(o.view(torch.int16), o_again.view(torch.int16)) and torch.equal(lse.view(torch.int32), lse_again.view(torch.int32)), \
        "forward is not deterministic"
    if case in NO_LSE:
        o_nolse, _ = fwd(False)
        assert torch.equal(o_nolse.view(torch.int16), o.view(torch.int16)), "O differs without lse"
    rep.bf("O", rows(o, nh), *packed_ref("O"))
    if packed:
        valid = (torch.arange(S, device=DEV)[None, :] < torch.tensor(lens, device=DEV)[:, None])[:, None, :].expand(B, nh, S)
        rep.lse(torch.where(valid, lse, torch.zeros_like(lse)), torch.where(valid, ref["lse"], torch.zeros_like(ref["lse"])), ref["u_lse"])
    else:
        rep.lse(lse, ref["lse"], ref["u_lse"])

    # ---- backward
    ns = _nsplit(B, S, nh, nkv, hd, causal)
    rp = (None, None, None)
    if rope:
        cos, sin = _rope_tables(4096, hd)
        pos = ((torch.arange(T) * 3) % 2500).to(torch.int32).to(DEV)
        rp = (cos.data_ptr(), sin.data_ptr(), pos.data_ptr())
    ws = None
    if form == "split":
        assert ns > 1, f"{case}: expected a head-split launch, lmod_attn_bwd_nsplit = {ns}"
        ws = torch.empty(ns * 2 * B * S * nkv * hd, device=DEV, dtype=torch.float32)
    elif form in ("spill", "sprope"):
        assert (ns == 1 or rope) and K.attn_bwd_ds_fusable(B, S, nh, hd), f"{case}: expected the dS-spill form (nsplit {ns})"
        ws = torch.empty(B * nh * S * S * 2, device=DEV, dtype=torch.uint8)
    else:
        assert not packed or hd == 128

    def bwd():
        draw, d = _pattern_rows(T, W, ld)
        dq, dk, dv = d[:, :Wq], d[:, Wq:Wq + Wk], d[:, Wq + Wk:]
        deraw, delta = _pattern_f32(B * nh * S)
        args = (q2.data_ptr(), k2.data_ptr(), v2.data_ptr(), o.data_ptr(), do2.data_ptr(), lse.data_ptr(), delta.data_ptr(), dq.data_ptr(),
                dk.data_ptr(), dv.data_ptr(), _hip.ptr(seqlens), _hip.ptr(cu), B, S, nh, nkv, hd, ld, ld, ld, Wq + PADC, Wq + PADC,
                ld, ld, ld, float(scale), int(causal))
        if ws is not None:
            ws.view(torch.uint8).fill_(0xFF)           # NaN everywhere: what the launch reads of it, it must have written
            _hip.call("lmod_attn_bwd_split", *args, *rp, ws.data_ptr(), ws.numel() * ws.element_size())
        elif rope:
            _hip.call("lmod_attn_bwd_rope", *args, *rp)
        else:
            _hip.call("lmod_attn_bwd", *args)
        torch.cuda.synchronize()
        _outside_intact(draw, T, W, "dQ | dK | dV")
        _outside_intact_f32(deraw, B * nh * S, "delta")
        return d, dq, dk, dv

    d, dq, dk, dv = bwd()
    d_again = bwd()[0]
    assert torch.equal(d.view(torch.int16), d_again.view(torch.int16)), f"backward form {form} is not deterministic"
    rq, uq = packed_ref("dQ")
    rk, uk = packed_ref("dK")
    rv, uv = packed_ref("dV")
    slq = slk = None
    if rope:
        c = cos[pos.long()].double().reshape(B, S, 1, hd)
        s_ = sin[pos.long()].double().reshape(B, S, 1, hd)
        rq, uq, slq = _rope_bwd64(rq, uq, c, s_)
        rk, uk, slk = _rope_bwd64(rk, uk, c, s_)
    rep.bf("dQ", rows(dq, nh), rq, uq, slq)
    rep.bf("dK", rows(dk, nkv), rk, uk, slk)
    rep.bf("dV", rows(dv, nkv), rv, uv)
    rep.done()


# ------------------------------------------------------------------------------------------ decode
# id: (smax, lens, nh, nkv, hd, kind)
DECODE = {
    "dec-128-4/4-diffuse": (700, [0, 1, 255, 256, 257], 4, 4, 128, "diffuse"),
    "dec-128-8/2-hot": (700, [513, 700, 707, 256, 1], 8, 2, 128, "hot"),
    "dec-64-14/2-hot": (700, [257, 513, 700, 0, 255], 14, 2, 64, "hot"),
    "dec-64-8/2-spike": (700, [600, 600, 301], 8, 2, 64, "spike"),
    "dec-128-14/2-spike": (4096, [600, 4096, 4103, 513], 14, 2, 128, "spike"),
    "dec-64-4/4-hot-4096": (4096, [4096, 257, 0, 4103, 1], 4, 4, 64, "hot"),
    "dec-128-4/4-smax5": (5, [0, 1, 5, 12, 4], 4, 4, 128, "hot"),
    "dec-64-8/2-smax5": (5, [5, 12, 0, 1, 3], 8, 2, 64, "diffuse"),
}


def _decode_launch(q, kc, vc, lens, nh, nkv, hd, scale):
    """Strided q / out, ld_cache = nkv*hd + 64 with NaN in the gap and in the cache rows >= len; out in a pattern buffer."""
    B, smax = q.shape[0], kc.shape[1]
    Wq, Wk = nh * hd, nkv * hd
    _, q2 = _nan_rows(q, Wq + PADC)
    caches = []
    for c in (kc, vc):
        buf = torch.full((B, smax, Wk + 64), float("nan"), dtype=BF, device=DEV)
        for b in range(B):
            L = max(0, min(int(lens[b]), smax))
            buf[b, :L, :Wk] = c[b, :L]
        caches.append(buf)
    lt = torch.tensor(lens, dtype=torch.int32, device=DEV)
    oraw, out = _pattern_rows(B, Wq, Wq + PADC)
    _hip.call("lmod_attn_decode", q2.data_ptr(), caches[0].data_ptr(), caches[1].data_ptr(), lt.data_ptr(), out.data_ptr(), B, nh, nkv, hd,
              smax, Wq + PADC, Wk + 64, Wq + PADC, float(scale))
    torch.cuda.synchronize()
    _outside_intact(oraw, B, Wq, "decode out")
    return out


@pytest.mark.parametrize("case", list(DECODE), ids=list(DECODE))
def test_attn_decode_against_fp64(case):
    smax, lens, nh, nkv, hd, kind = DECODE[case]
    B = len(lens)
    q, kc, vc, scale = R.make_decode_case(kind, B, smax, lens, nh, nkv, hd, seed=len(case), device=DEV)
    ref, unit = R.decode_ref64(q, kc, vc, lens, nh, nkv, hd, scale)
    out = _decode_launch(q, kc, vc, lens, nh, nkv, hd, scale)
    again = _decode_launch(q, kc, vc, lens, nh, nkv, hd, scale)
    assert torch.equal(out.view(torch.int16), again.view(torch.int16)), "decode is not deterministic"
    rep = Report(case)
    rep.bf("O", out, ref, unit)
    # the last token through the prefill kernel: row len - 1 of a causal forward over the same keys and values
    b = max(range(B), key=lambda i: min(lens[i], smax) if min(lens[i], smax) <= 1024 else 0)
    L = min(lens[b], smax)
    if L > 0:
        qq = torch.zeros(L, nh * hd, dtype=BF, device=DEV)
        qq[L - 1] = q[b]
        o, _ = K.attn_fwd(qq, kc[b, :L].contiguous(), vc[b, :L].contiguous(), 1, L, nh, nkv, hd, scale, True)
        d = (o[L - 1].double() - out[b].double()).abs()
        bound = 2 * (0.5 * R.ulp_bf16(ref[b]) + R.LIMITS["O"] * unit[b])          # the sum of both kernels' bounds
        assert (d <= bound).all(), f"{case}: decode vs prefill row {L - 1}: {float((d - bound).max()):.4g} over the bound"
    rep.done()


# ------------------------------------------------------------------------------------------ argument contract
def test_attn_argument_contract():
    """LMOD_EINVAL (-1) / LMOD_EUNSUPPORTED (-3) of the attention entry points, beyond the head-dim case of
    tests/test_kernels_gpu.py::test_abi_error_codes_and_empty_inputs.  Every call returns before the attention kernels are launched
    (the misaligned-workspace call is refused after the small delta pass, which stays inside `lse`)."""
    lib = _hip.load()
    st = torch.cuda.current_stream().cuda_stream
    B, S, nh, nkv, hd = 1, 64, 4, 2, 128
    W = (nh + 2 * nkv) * hd
    x = torch.zeros(B * S, W, device=DEV, dtype=BF)
    o = torch.zeros(B * S, nh * hd, device=DEV, dtype=BF)
    lse = torch.zeros(B * nh * S, device=DEV, dtype=torch.float32)
    i32 = torch.zeros(B + 1, device=DEV, dtype=torch.int32)
    P = x.data_ptr()

    def fwd(B=B, S=S, nh=nh, nkv=nkv, hd=hd, ldq=W, ldk=W, ldv=W, ldo=nh * hd, Q=P, O=o.data_ptr(), sl=None, cu=None):
        return lib.lmod_attn_fwd(Q, P, P, O, lse.data_ptr(), sl, cu, B, S, nh, nkv, hd, ldq, ldk, ldv, ldo, 0.1, 1, st)

    assert fwd(B=0) == -1 and fwd(S=0) == -1 and fwd(nh=0) == -1 and fwd(nkv=0) == -1
    assert fwd(nh=3, nkv=2) == -1                                       # nh % nkv
    assert fwd(Q=None) == -1 and fwd(O=None) == -1
    assert fwd(hd=32) == -3 and fwd(hd=256) == -3
    assert fwd(ldq=W + 4) == -1 and fwd(ldk=W + 4) == -1 and fwd(ldv=W + 4) == -1 and fwd(ldo=nh * hd + 4) == -1      # % 8
    assert fwd(ldq=nh * hd - 8) == -1 and fwd(ldk=nkv * hd - 8) == -1 and fwd(ldv=nkv * hd - 8) == -1 and fwd(ldo=nh * hd - 8) == -1
    assert fwd(S=1 << 20, ldk=2048) == -3                               # S * ld * 2 bytes past the 2 GiB buffer-addressing range
    assert fwd(hd=64, nh=8, nkv=4, cu=i32.data_ptr()) == -3             # cu_seqlens: the hd-128 kernels only
    assert fwd(sl=i32.data_ptr(), cu=i32.data_ptr()) == -3              # cu_seqlens together with seqlens

    def bwd(fn="lmod_attn_bwd", hd=hd, nh=nh, nkv=nkv, lddo=nh * hd, lddq=W, lddk=W, lddv=W, dO=o.data_ptr(), delta=lse.data_ptr(), sl=None,
            cu=None, extra=()):
        return getattr(lib, fn)(P, P, P, o.data_ptr(), dO, lse.data_ptr(), delta, P, P, P, sl, cu, B, S, nh, nkv, hd, W, W, W, nh * hd, lddo,
                                lddq, lddk, lddv, 0.1, 1, *extra, st)

    assert bwd(dO=None) == -1 and bwd(delta=None) == -1
    assert bwd(lddo=nh * hd + 4) == -1 and bwd(lddq=W + 4) == -1 and bwd(lddk=nkv * hd - 8) == -1 and bwd(lddv=W + 2) == -1
    assert bwd(hd=64, nh=8, nkv=4, cu=i32.data_ptr()) == -3 and bwd(sl=i32.data_ptr(), cu=i32.data_ptr()) == -3
    cos = torch.zeros(64, 128, device=DEV, dtype=BF)
    pos = torch.zeros(B * S, device=DEV, dtype=torch.int32)
    assert bwd("lmod_attn_bwd_rope", extra=(None, cos.data_ptr(), pos.data_ptr())) == -1
    assert bwd("lmod_attn_bwd_rope", extra=(cos.data_ptr(), cos.data_ptr(), None)) == -1
    assert bwd("lmod_attn_bwd_rope", hd=64, nh=8, nkv=4, extra=(cos.data_ptr(), cos.data_ptr(), pos.data_ptr())) == -3     # RoPE with hd 64
    assert bwd("lmod_attn_bwd_split", extra=(cos.data_ptr(), None, None, None, 0)) == -1                                  # a partial RoPE triple
    # a head-split launch with a misaligned workspace is refused (B 1, S 64, 4/2 heads: nsplit 2)
    ns = lib.lmod_attn_bwd_nsplit(B, S, nh, nkv, hd, 1)
    assert ns > 1
    ws = torch.zeros(ns * 2 * B * S * nkv * hd + 8, device=DEV, dtype=torch.float32)
    assert bwd("lmod_attn_bwd_split", extra=(None, None, None, ws.data_ptr() + 4, ns * 2 * B * S * nkv * hd * 4)) == -1
    assert lib.lmod_attn_bwd_nsplit(0, S, nh, nkv, hd, 1) == 1 and lib.lmod_attn_bwd_nsplit(B, S, 3, 2, hd, 1) == 1
    # decode
    lt = torch.ones(1, device=DEV, dtype=torch.int32)

    def dec(B=1, nh=nh, nkv=nkv, hd=hd, smax=S, ldq=nh * hd, ldc=nkv * hd, ldo=nh * hd, q=P, kc=P, lens=lt.data_ptr()):
        return lib.lmod_attn_decode(q, kc, P, lens, o.data_ptr(), B, nh, nkv, hd, smax, ldq, ldc, ldo, 0.1, st)

    assert dec(B=-1) == -1 and dec(nh=0) == -1 and dec(nh=3) == -1 and dec(smax=0) == -1
    assert dec(B=0) == 0                                                # empty: nothing launched
    assert dec(q=None) == -1 and dec(lens=None) == -1
    assert dec(hd=96) == -3
    assert dec(ldc=nkv * hd + 4) == -1 and dec(ldc=nkv * hd - 8) == -1 and dec(ldq=nh * hd - 8) == -1 and dec(ldo=nh * hd - 8) == -1
    assert dec(kc=P + 8) == -1                                          # cache not 16-byte aligned
    torch.cuda.synchronize()
    assert float(o.abs().max()) == 0 and float(x.abs().max()) == 0       # nothing was written
