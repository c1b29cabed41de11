"""fp32 model of long-chunk attention against a KV cache (csrc/attn_extend.hip, lmod_attn_extend), its seeded faults and the cases
its tests share.  TEST INFRASTRUCTURE ONLY.

The fp64 statement (`append_ref64`), the inputs (`make_append_case`) and the units (`err_units`, `ulp_bf16`) are tests/_append_ref.py's:
the two kernels share one contract.  A bf16 output element is inside its bound iff |out - ref| <= 1/2 ulp_bf16(ref) + L u_O with
u_O[q, d] = sum_k P_qk |V_kd| from fp64 quantities only; elements whose unit is 0 (no visible key) must be exactly 0.

* `extend_model`: the kernel's arithmetic as its header comment states it and nothing else, in fp32: S = Q K^T, scaled; masked
  scores -inf; p = exp(S - m) in fp32; l = sum p; O = p V with the fp32 p (the kernel's three bf16 terms hold it exactly); ONE
  rounding: out = bf16(O / l).  One softmax over the row: the kernel's running max only moves a factor between p and alpha, at fp32
  roundoff.  Its figures are therefore of lmod_attn_append's size (P in fp32 there too), not of `_attn_ref.attn_model`'s 0.0026: a
  kernel with P rounded once to bf16 was measured first and its next-layer cache rows missed the decode path's by more than one bf16
  ulp in 20 % of the elements, which the chunk path's tests do not allow.
* LIMIT = 4 x the model's largest figure over tests/test_extend_ref_cpu.py's geometries x cases x input kinds (the factor 4 as in
  _attn_ref.py: fp32 summation order, the hardware exp2, the online rescale).  Measured on the CPU, never from the kernel.
"""
import functools

import torch

from _append_ref import append_ref64, make_append_case, err_units, ulp_bf16, _rows  # noqa: F401  (re-exported for the tests)

F64, F32, BF = torch.float64, torch.float32, torch.bfloat16
NEG_INF = float("-inf")
QB = 128          # query rows per workgroup
KT = 64           # keys per tile

# Largest err / unit of extend_model against append_ref64 over test_extend_ref_cpu.py's GEOMS x CASES x KINDS (its EXTEND-MODEL lines,
# measured on the CPU): 5.317e-7 (spike, hd 64, nh 14, nkv 2, case ragged).  Beyond the output's own 1/2 ulp there is only fp32
# roundoff, as for append_model (2e-7 over shorter rows).  test_extend_ref_cpu.py asserts model <= MODEL_MAX.
MODEL_MAX = 5.4e-7
LIMIT = 4.0 * MODEL_MAX

GEOMS = [(128, 28, 4), (64, 14, 2), (128, 4, 4), (64, 2, 2)]          # (hd, nh, nkv)
KINDS = ["diffuse", "hot", "spike"]


def _case(ns, hists, T, flush=False, lens=None):
    lens = [h + n for h, n in zip(hists, ns if ns is not None else [T] * len(hists))] if lens is None else lens
    return dict(ns=ns, lens=lens, T=T, smax=max(lens) if flush else None)


# n_b in {0, 1, 17, 63, 64, 65, 129, 300} x histories lens - n_b in {0, 1, 63, 64, 65, 700}
CASES = {
    "ragged": _case([0, 1, 17, 63, 64, 65, 129, 300], [64, 700, 0, 65, 1, 63, 700, 64], 300),
    "flush": _case([65, 129, 300], [0, 63, 700], 300, flush=True),            # smax = max(lens): the last sample ends at the allocation's end
    "uniform65": _case(None, [0, 64, 700], 65),                               # cu_new = None
    "headless": _case([17, 64, 129], None, 129, lens=[5, 30, 129]),           # lens < n_b: leading rows without a visible key
}


@functools.lru_cache(maxsize=None)
def case_and_ref(kind, name, hd, nh, nkv, poison=False):
    """(inputs on the CPU, (fp64 out, unit)) of one shared case; computed once per process, never modified by a test."""
    c = CASES[name]
    case = make_append_case(kind, c["lens"], c["ns"], c["T"], nh, nkv, hd, smax=c["smax"], seed=3, poison=poison)
    q, kc, vc, lens, cu, scale = case
    return case, append_ref64(q, kc, vc, lens, cu, c["T"], nh, nkv, hd, scale)


def extend_model(q, kc, vc, lens, cu, T, nh, nkv, hd, scale, hooks=None):
    """q [R, >= nh*hd] packed rows, caches [B, smax, >= nkv*hd] bf16, lens [B] (after the append), cu [B+1] or None -> out [R, nh*hd]
    fp32 (bf16 values).  hooks: a seeded fault (FAULTS)."""
    hooks = hooks or {}
    B, smax = kc.shape[0], kc.shape[1]
    group = nh // nkv
    out = torch.zeros(q.shape[0], nh * hd, dtype=F32)
    sc32 = torch.tensor(scale, dtype=F32)
    r = lambda x: x.to(BF).to(F32)
    for b, (r0, n) in enumerate(_rows(cu, B, T)):
        L = max(0, min(int(lens[b]) + hooks.get("len_shift", 0), smax))
        if L == 0 or n == 0:
            continue
        ar, t = torch.arange(L), torch.arange(n)
        lim = (t if hooks.get("no_history") else L - n + t)[:, None]
        vis = (ar[None, :] < lim) if hooks.get("strict_diag") else (ar[None, :] <= lim)
        if hooks.get("unmasked_tile_above"):
            # the first key tile entirely above a query tile's last row is visited and not masked
            for q0 in range(0, n, QB):
                jt = (L - n + min(q0 + QB, n) - 1) // KT + 1
                if jt >= 0:
                    vis[q0:q0 + QB, jt * KT:(jt + 1) * KT] = True
        for h in range(nh):
            hk = hooks["head_map"](h, nh, nkv) if "head_map" in hooks else h // group
            Kh, V = kc[b, :L, hk * hd:(hk + 1) * hd].to(F32), vc[b, :L, hk * hd:(hk + 1) * hd].to(F32)
            Q = q[r0:r0 + n, h * hd:(h + 1) * hd].to(F32)
            s = ((Q @ Kh.T) * sc32).masked_fill(~vis, NEG_INF)
            m = s.amax(-1)
            live = m > NEG_INF
            p = torch.exp(s - torch.where(live, m, torch.zeros_like(m))[:, None])
            l = p.sum(-1)
            o = r((p @ V) / torch.where(live, l, torch.ones_like(l))[:, None])
            if hooks.get("last_tile_shift") and n % QB:
                q0 = (n - 1) // QB * QB                     # the last, partial query tile stores its rows one row late
                o[q0:] = torch.roll(o[q0:], 1, 0)
            out[r0:r0 + n, h * hd:(h + 1) * hd] = o
    return out


# name -> (hooks for extend_model, what the geometry needs: "any" | "gqa")
FAULTS = {
    "diagonal_strict": ({"strict_diag": True}, "any"),                        # `<=` -> `<` on the chunk diagonal
    "history_offset_dropped": ({"no_history": True}, "any"),                  # k <= t instead of k <= lens - n + t
    "lens_minus_one": ({"len_shift": -1}, "any"),
    "lens_plus_one": ({"len_shift": 1}, "any"),
    "gqa_map_modulo": ({"head_map": lambda h, nh, nkv: h % nkv}, "gqa"),
    "tile_above_diagonal_unmasked": ({"unmasked_tile_above": True}, "any"),
    "last_partial_tile_rows_shifted": ({"last_tile_shift": True}, "any"),
}
