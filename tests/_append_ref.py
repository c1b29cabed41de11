"""fp64 restatement of chunk-against-cache attention (csrc/append.hip, lmod_attn_append), an fp32 model of that kernel, and a brute-force
restatement of the acceptance rule of greedy assisted decoding (lmod_spec_accept).  TEST INFRASTRUCTURE ONLY.

Method and units are tests/_attn_ref.py's (`ulp_bf16`, `err_units` are imported from it): a bf16 output element is inside its bound
iff |out - ref| <= 1/2 ulp_bf16(ref) + L u_O with u_O[q, d] = sum_k P_qk |V_kd| from fp64 quantities only; elements whose unit is 0 (no
visible key) must be exactly 0.

* `append_ref64`: sample b brings n_b new tokens (already in the cache); query t sees the keys k <= lens[b] - n_b + t.
* `append_model`: the kernel's arithmetic as its header comment states it and nothing else: q * scale in fp32; scores as fp32 sums in
  ascending d; 64-key chunks dealt to `nsplit` splits in runs of ceil(nchunks / nsplit); per chunk m' = max(m, chunk max),
  alpha = exp(m - m'), p = exp(s - m') kept in fp32 (exp(x) = exp2(fp32(x * log2 e)), as the hardware evaluates it),
  l = l alpha + sum p, acc = acc alpha + sum_k p_k v_k in ascending key order;
  one split: out = bf16(acc * (1 / l)); more: M = max m_s, L = sum l_s exp(m_s - M), out = bf16((sum acc_s exp(m_s - M)) / L) in
  split order.  The sequential sums are fp32 cumsum's last element (no FMA: one rounding more per term than the kernel, never fewer).
* L = 4 x the model's largest figure over tests/test_append_ref_cpu.py's geometries x input kinds (the factor 4 as in _attn_ref.py:
  the hardware exp, FMA contraction and the wave reduction's summation order).  Measured on the CPU, never from the kernel.
"""
import math

import torch

from _attn_ref import err_units, ulp_bf16  # noqa: F401  (re-exported for the tests)

F64, F32, BF = torch.float64, torch.float32, torch.bfloat16
NEG_INF = float("-inf")
T_MAX = 16
KC = 64

# Largest err / unit of append_model against append_ref64 over test_append_ref_cpu.py's GEOMS x KINDS (its APPEND-MODEL lines, measured
# on the CPU): 1.91e-7 (hot, hd 128, group 7, 2049 + n keys, 4 splits).  The figure is small because P stays in fp32: beyond the output's
# own 1/2 ulp there is only fp32 roundoff.  test_append_ref_cpu.py asserts model <= MODEL_MAX.
MODEL_MAX = 2.0e-7
LIMIT = 4.0 * MODEL_MAX


def _rows(cu, B, T):
    """(first packed row, n_b) per sample."""
    if cu is None:
        return [(b * T, T) for b in range(B)]
    return [(int(cu[b]), int(cu[b + 1]) - int(cu[b])) for b in range(B)]


def append_ref64(q, kc, vc, lens, cu, T, nh, nkv, hd, scale):
    """q [R, >= nh*hd] packed rows, caches [B, smax, >= nkv*hd] bf16, lens [B] (after the append), cu [B+1] or None ->
    (out, u_O) [R, nh*hd] fp64."""
    B, smax = kc.shape[0], kc.shape[1]
    group = nh // nkv
    out = torch.zeros(q.shape[0], nh * hd, dtype=F64)
    unit = torch.zeros_like(out)
    for b, (r0, n) in enumerate(_rows(cu, B, T)):
        L = max(0, min(int(lens[b]), smax))
        if L == 0:
            continue
        ar = torch.arange(L)
        for h in range(nh):
            hk = h // group
            Kh, V = kc[b, :L, hk * hd:(hk + 1) * hd].to(F64), vc[b, :L, hk * hd:(hk + 1) * hd].to(F64)
            Q = q[r0:r0 + n, h * hd:(h + 1) * hd].to(F64)
            vis = ar[None, :] <= (L - n + torch.arange(n))[:, None]
            s = ((Q @ Kh.T) * scale).masked_fill(~vis, NEG_INF)
            live = vis.any(-1)
            p = torch.softmax(torch.where(live[:, None], s, torch.zeros_like(s)), -1) * live[:, None]
            out[r0:r0 + n, h * hd:(h + 1) * hd] = p @ V
            unit[r0:r0 + n, h * hd:(h + 1) * hd] = p @ V.abs()
    return out, unit


LOG2E = torch.tensor(1.4426950408889634, dtype=F32)


def _exp(x):
    """The kernel's exp: exp2 of the fp32 product x * log2(e) (the product's rounding is a rounding point of its own)."""
    return torch.exp2(x * LOG2E.to(x.dtype)) if x.dtype == F32 else torch.exp(x)


def _seqsum(x, dim):
    """fp32 sum along `dim` in ascending index order (cumsum's last element)."""
    return x.cumsum(dim).select(dim, x.shape[dim] - 1)


def append_model(q, kc, vc, lens, cu, T, nh, nkv, hd, scale, nsplit=1, hooks=None):
    hooks = hooks or {}
    B, smax = kc.shape[0], kc.shape[1]
    group = nh // nkv
    out = torch.zeros(q.shape[0], nh * hd, dtype=F32)
    sc32 = torch.tensor(scale, dtype=F32)
    for b, (r0, n) in enumerate(_rows(cu, B, T)):
        L = max(0, min(int(lens[b]) + hooks.get("len_shift", 0), smax))
        nchunks = (L + KC - 1) // KC
        cps = (nchunks + nsplit - 1) // nsplit if nchunks else 0
        for h in range(nh):
            hk = hooks["head_map"](h, nh, nkv) if "head_map" in hooks else h // group
            Kh, V = kc[b, :L, hk * hd:(hk + 1) * hd].to(F32), vc[b, :L, hk * hd:(hk + 1) * hd].to(F32)
            Q = q[r0:r0 + n, h * hd:(h + 1) * hd].to(F32) * sc32
            lim = (L - n + torch.arange(n))[:, None]
            parts = []
            for s in range(nsplit):
                m, l, acc = torch.full((n,), NEG_INF, dtype=F32), torch.zeros(n, dtype=F32), torch.zeros(n, hd, dtype=F32)
                for c in range(s * cps, min(nchunks, (s + 1) * cps)):
                    k0, k1 = c * KC, min(L, (c + 1) * KC)
                    ar = torch.arange(k0, k1)
                    sco = _seqsum(Q[:, None, :] * Kh[None, k0:k1, :], 2)
                    vis = (ar[None, :] < lim) if hooks.get("strict_diag") else (ar[None, :] <= lim)
                    sco = sco.masked_fill(~vis, NEG_INF)
                    mn = torch.maximum(m, sco.amax(-1))
                    dead = mn == NEG_INF
                    alpha = torch.where(dead, torch.ones_like(mn), _exp(m - torch.where(dead, torch.zeros_like(mn), mn)))
                    p = torch.where(vis, _exp(sco - torch.where(dead, torch.zeros_like(mn), mn)[:, None]), torch.zeros_like(sco))
                    l = l * alpha + p.sum(-1)
                    acc = acc * alpha[:, None] + _seqsum(p[:, :, None] * V[None, k0:k1, :], 1)
                    m = mn
                parts.append((m, l, acc))
            if nsplit == 1:
                m, l, acc = parts[0]
                inv = torch.where(l > 0, 1.0 / l, torch.zeros_like(l))
                o = acc * inv[:, None]
            else:
                if "drop_split" in hooks:
                    parts = [pt for i, pt in enumerate(parts) if i != hooks["drop_split"]]
                M = torch.stack([pt[0] for pt in parts]).amax(0)
                Ls, O = torch.zeros(n, dtype=F32), torch.zeros(n, hd, dtype=F32)
                for m, l, acc in parts:
                    e = torch.where(m == NEG_INF, torch.zeros_like(m), _exp(m - torch.where(M == NEG_INF, torch.zeros_like(M), M)))
                    Ls = Ls + l * e
                    O = O + acc * e[:, None]
                o = torch.where((Ls > 0)[:, None], O / Ls.clamp_min(1e-38)[:, None], torch.zeros_like(O))
            out[r0:r0 + n, h * hd:(h + 1) * hd] = o.to(BF).to(F32)
    return out


def make_append_case(kind, lens, ns, T, nh, nkv, hd, smax=None, seed=0, device="cpu", poison=False):
    """Deterministic inputs: q [sum n_b, nh*hd] packed, caches [B, smax, nkv*hd] bf16, lens / cu int32, scale.  ns: n_b per sample (None:
    T each, cu None).  kind: diffuse N(0, 1); hot: query t gets +8 in score on ITS OWN key (the chunk diagonal lens - n + t) and the
    position behind the cache's valid range repeats the last key, so a mask that is off by one on either side moves a dominant mass;
    spike: one history key (the middle one) dominates every query by ~40 (q, k ~ 0.3 N(0, 1)).  poison: NaN behind lens."""
    B = len(lens)
    smax = smax or (max(lens) + 3)
    g = torch.Generator().manual_seed(11 + 1000003 * seed + smax + 31 * nh + hd + 7 * T)
    scale = 1.0 / math.sqrt(hd)
    f = 0.3 if kind == "spike" else 1.0
    nlist = [T] * B if ns is None else list(ns)
    R = sum(nlist)
    q = f * torch.randn(R, nh, hd, generator=g)
    kc = f * torch.randn(B, smax, nkv, hd, generator=g)
    vc = torch.randn(B, smax, nkv, hd, generator=g)
    group = nh // nkv
    r0 = 0
    for b in range(B):
        L, n = min(int(lens[b]), smax), nlist[b]
        kb = kc.to(BF).float()
        if kind == "hot" and L > 0:
            for t in range(n):
                key = L - n + t
                if key < 0:
                    continue
                for h in range(nh):
                    kh = kb[b, key, h // group]
                    q[r0 + t, h] += (8.0 / scale) * kh / (kh * kh).sum()
            if L < smax:
                kc[b, L] = kc[b, L - 1]
        elif kind == "spike" and L > 0:
            key = max(0, (L - n) // 2)
            for hk in range(nkv):
                qh = q[r0, hk * group].to(BF).float()
                kc[b, key, hk] = qh * 40.0 / (scale * (qh * qh).sum())
        elif kind not in ("diffuse", "hot", "spike"):
            raise ValueError(kind)
        r0 += n
    kc, vc = kc.reshape(B, smax, nkv * hd).to(BF), vc.reshape(B, smax, nkv * hd).to(BF)
    if poison:
        for b in range(B):
            kc[b, min(int(lens[b]), smax):] = float("nan")
            vc[b, min(int(lens[b]), smax):] = float("nan")
    cu = None
    if ns is not None:
        cu = torch.tensor([0] + list(torch.tensor(nlist).cumsum(0)), dtype=torch.int32).to(device)
    return (q.reshape(R, nh * hd).to(BF).to(device), kc.to(device), vc.to(device),
            torch.tensor([int(x) for x in lens], dtype=torch.int32, device=device), cu, scale)


# name -> (hooks for append_model, what the geometry needs: "any" | "gqa" | "split")
FAULTS = {
    "chunk_diagonal_strict": ({"strict_diag": True}, "any"),          # `<=` -> `<` on the chunk diagonal
    "lens_minus_one": ({"len_shift": -1}, "any"),
    "lens_plus_one": ({"len_shift": 1}, "any"),
    "gqa_map_modulo": ({"head_map": lambda h, nh, nkv: h % nkv}, "gqa"),
    "dropped_split_partial": ({"drop_split": 1}, "split"),
}


# ------------------------------------------------------------------------------------------ acceptance rule, brute force
def spec_accept_bruteforce(draft, target, done, eos, pad, lens_target, lens_draft):
    """lmod_spec_accept restated with Python lists and loops.  Returns (block rows [B][k+5], next_token [B], done [B], lens_target [B],
    lens_draft [B])."""
    B, k = len(draft), len(draft[0])
    block, nxt, dn, lt, ld = [], [], [], [], []
    for b in range(B):
        n_acc = 0
        if not done[b]:
            while n_acc < k and draft[b][n_acc] == target[b][n_acc]:
                n_acc += 1
        emitted = [] if done[b] else list(draft[b][:n_acc]) + [target[b][n_acc]]
        fin = bool(done[b])
        if eos is not None and eos in emitted:
            emitted = emitted[:emitted.index(eos) + 1]
            fin = True
        nx = pad if fin else target[b][n_acc]
        block.append(emitted + [pad] * (k + 1 - len(emitted)) + [n_acc, len(emitted), nx, int(fin)])
        nxt.append(nx)
        dn.append(int(fin))
        lt.append(lens_target[b] - (k + 1) + 1 + n_acc)
        ld.append(lens_draft[b] - k + min(n_acc + 1, k))
    return block, nxt, dn, lt, ld
