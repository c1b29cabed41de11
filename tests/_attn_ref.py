"""fp64 restatement of the attention kernels (csrc/attn.hip, attn_fwd2.hip, attn_bwd2.hip) for kernel tests.  TEST INFRASTRUCTURE ONLY.

* `attn_ref64`: softmax(scale Q K^T + mask) V and its gradients in fp64 from the bf16 inputs, one (batch, head) at a time so that
  S 2048 fits: O, lse, dQ, dK, dV (and P, dP, delta with keep=True).  Mask: key k is visible to query q iff k < lens[b] and
  (not causal or k <= q).  Padded QUERY rows (q >= lens[b]) are ordinary rows under that mask.  Rows without a visible key: O = 0,
  lse = -inf, zero gradients.  GQA: query head h reads KV head h // (nh // nkv).  `decode_ref64`: the single-query form.
* Units: per element, the magnitude rounding acts on, from fp64 quantities only:
      u_O[q,d]  = sum_k P_qk |V_kd|                      u_dV[k,d] = sum_q P_qk |dO_qd|
      D_q = sum_d |dO_qd| |O_qd|,  W_qk = P_qk (|dP_qk| + D_q)
      u_dQ[q,d] = scale sum_k W_qk |K_kd|                u_dK[k,d] = scale sum_q W_qk |Q_qd|   (GQA: summed over the group)
      u_lse[q]  = 1 + |lse_q| + scale max_{k visible} sum_d |Q_qd K_kd|     (in fp32 unit roundoff 2^-24)
  A bf16 output is inside its bound iff |out - ref| <= 1/2 ulp_bf16(ref) + L u; lse iff |out - ref| <= L_lse 2^-24 u_lse.  Elements
  whose unit is 0 (no visible key; keys >= len) must be exactly 0, lse of a row without a visible key exactly -inf.  `err_units`
  returns max over ALL elements of (|out - ref| - 1/2 ulp) / u, which is compared with L.
* `attn_model`: the same math in fp32 with the kernels' documented rounding points and nothing else (attn_fwd2.hip / attn_bwd2.hip
  header comments): P to bf16 before P V, O to bf16, P recomputed from the fp32 lse in the backward, delta from the bf16 O, dS to
  bf16 before the dQ / dK products, P to bf16 before the dV product, outputs to bf16.  Its error against `attn_ref64` in the units
  above is what the limits are derived from: L = 4 x the largest model figure over all input kinds and the geometries of
  tests/test_attn_ref_cpu.py (the factor 4: fp32 summation order over up to 2048 keys, the hardware exp2, probabilities up to 2^6
  before normalisation under the deferred rescale).  The limits come from this model, never from a kernel's output.
* `make_case`: deterministic inputs (diffuse / hot / spike / creep, dO kinds).  `FAULTS`: seeded faults applied to the model.
"""
import math

import torch

F64 = torch.float64
F32 = torch.float32
BF = torch.bfloat16
NEG_INF = float("-inf")

# Largest err / unit of attn_model against attn_ref64 over tests/test_attn_ref_cpu.py's geometries x input kinds (the ATTN-MODEL lines
# of that file, measured on the CPU), and the limits L = 4 x that figure.  test_attn_ref_cpu.py asserts model <= MODEL_MAX.
#   measured:    O 0.00257 (diffuse)   dQ 0.00225 (spike)   dK 0.00268 (diffuse)   dV 0.00367 (diffuse)   lse 2.56 (hot)
MODEL_MAX = {"O": 0.0026, "dQ": 0.0023, "dK": 0.0027, "dV": 0.0037, "lse": 2.6}
LIMITS = {k: 4.0 * v for k, v in MODEL_MAX.items()}
# The decode kernel keeps P in fp32 (its model's error beyond the output rounding measures 0): its output is bound as O is.


# ------------------------------------------------------------------------------------------ bounds
def ulp_bf16(x):
    """Spacing of bf16 (8 significand bits) at |x|, fp64; 0 at 0."""
    _, e = torch.frexp(x.abs().double())
    return torch.where(x == 0, torch.zeros((), dtype=F64, device=x.device), torch.ldexp(torch.ones((), dtype=F64, device=x.device), e - 8))


def err_units(out, ref, unit, slack=None):
    """max over all elements of (|out - ref| - slack) / unit, its index, and the number of elements with unit == 0 that are not exactly
    0.  slack: the output's own rounding, 1/2 ulp_bf16(ref) unless given.  Non-finite outputs count as infinitely wrong."""
    o = out.double()
    err = (o - ref).abs()
    err = torch.where(torch.isfinite(o), err, torch.full_like(err, float("inf")))
    err = (err - (0.5 * ulp_bf16(ref) if slack is None else slack)).clamp_min(0)
    zero = unit == 0
    ratio = torch.where(zero, torch.zeros_like(err), err / unit.clamp_min(1e-300))
    i = int(torch.argmax(ratio))
    idx = tuple(int(x) for x in torch.unravel_index(torch.tensor(i), ratio.shape))
    return float(ratio.reshape(-1)[i]), idx, int((zero & (o != 0)).sum())


def err_units_lse(out, ref, unit):
    """max |out - ref| / (2^-24 u_lse) over rows with a visible key, its index, and the number of rows without one that are not -inf."""
    o = out.double()
    dead = torch.isinf(ref)
    err = torch.where(dead, torch.zeros_like(ref), (o - torch.where(dead, torch.zeros_like(ref), ref)).abs())
    err = torch.where(torch.isfinite(o) | dead, err, torch.full_like(err, float("inf")))
    ratio = torch.where(dead, torch.zeros_like(err), err / (2.0 ** -24 * unit))
    i = int(torch.argmax(ratio))
    idx = tuple(int(x) for x in torch.unravel_index(torch.tensor(i), ratio.shape))
    return float(ratio.reshape(-1)[i]), idx, int((dead & (o != NEG_INF)).sum())


def old_close_count(out, ref, rtol, afrac):
    """How many elements tests/test_kernels_gpu.py's close() (tensor-wide absolute term) would flag."""
    out, ref = out.double(), torch.nan_to_num(ref.double(), neginf=0.0)
    out = torch.nan_to_num(out, neginf=0.0)
    return int(((out - ref).abs() > afrac * ref.abs().max().clamp_min(1e-30) + rtol * ref.abs()).sum())


# ------------------------------------------------------------------------------------------ the math (fp64 reference and fp32 model)
def visible(S, L, causal, device):
    ar = torch.arange(S, device=device)
    vis = (ar[None, :] < L).expand(S, S)
    if causal:
        vis = vis & (ar[None, :] <= ar[:, None])
    return vis


def _attn(q, k, v, do, scale, causal, lens, dt, model, hooks=None, keep=False):
    hooks = hooks or {}
    B, S, nh, hd = q.shape
    nkv = k.shape[2]
    group = nh // nkv
    dev = q.device
    r = (lambda x: x.to(BF).to(dt)) if model else (lambda x: x)
    z = lambda *s: torch.zeros(*s, dtype=dt, device=dev)
    res = {"O": z(B, S, nh, hd), "lse": z(B, nh, S)}
    bwd = do is not None
    if bwd:
        res.update(dQ=z(B, S, nh, hd), dK=z(B, S, nkv, hd), dV=z(B, S, nkv, hd))
    if not model:
        res.update(u_O=z(B, S, nh, hd), u_lse=z(B, nh, S))
        if bwd:
            res.update(u_dQ=z(B, S, nh, hd), u_dK=z(B, S, nkv, hd), u_dV=z(B, S, nkv, hd))
    if keep:
        res.update(P=z(B, nh, S, S), dP=z(B, nh, S, S), delta=z(B, nh, S))
    dk_scale = hooks.get("dk_scale", scale)
    for b in range(B):
        L = S if lens is None else int(lens[b])
        for h in range(nh):
            hk = hooks["head_map"](h, nh, nkv) if "head_map" in hooks else h // group
            vis = visible(S, L, causal, dev)
            if "mask" in hooks:
                vis = hooks["mask"](vis, S, L, causal)
            Q, Kh, V = q[b, :, h].to(dt), k[b, :, hk].to(dt), v[b, :, hk].to(dt)
            s = ((Q @ Kh.T) * scale).masked_fill(~vis, NEG_INF)
            m = s.amax(-1)
            live = m > NEG_INF
            m0 = torch.where(live, m, torch.zeros_like(m))
            p = torch.exp(s - m0[:, None])
            l = p.sum(-1)
            lse0 = m0 + torch.log(l.clamp_min(1e-300 if dt == F64 else 1e-30))
            O = r((r(p) @ V) / torch.where(live, l, torch.ones_like(l))[:, None])
            lse0 = lse0 + hooks.get("lse_shift", 0.0)
            res["O"][b, :, h] = O
            res["lse"][b, h] = torch.where(live, lse0, torch.full_like(lse0, NEG_INF))
            P = torch.exp(s - torch.where(live, lse0, torch.zeros_like(lse0))[:, None])      # masked entries: exp(-inf) = 0
            if not model:
                res["u_O"][b, :, h] = P @ V.abs()
                qk = (Q.abs() @ Kh.abs().T).masked_fill(~vis, 0).amax(-1)
                res["u_lse"][b, h] = 1.0 + torch.where(live, lse0, torch.zeros_like(lse0)).abs() + scale * qk
            if not bwd:
                continue
            dO = do[b, :, h].to(dt)
            dP = dO @ V.T
            delta = (dO * O).sum(-1)
            dS = P * dP if hooks.get("no_delta") else P * (dP - delta[:, None])
            dSr = r(dS)
            res["dQ"][b, :, h] = r(scale * (dSr @ Kh))
            res["dK"][b, :, hk] += dSr.T @ Q
            res["dV"][b, :, hk] += r(P).T @ dO
            if not model:
                D = (dO.abs() * O.abs()).sum(-1)
                W = P * (dP.abs() + D[:, None])
                res["u_dQ"][b, :, h] = scale * (W @ Kh.abs())
                res["u_dK"][b, :, hk] += scale * (W.T @ Q.abs())
                res["u_dV"][b, :, hk] += P.T @ dO.abs()
            if keep:
                res["P"][b, h], res["dP"][b, h], res["delta"][b, h] = P, dP, delta
    if bwd:
        res["dK"] = r(res["dK"] * dk_scale)
        res["dV"] = r(res["dV"])
    return res


def attn_ref64(q, k, v, do, scale, causal, lens=None, keep=False):
    """q [B, S, nh, hd], k / v [B, S, nkv, hd], do [B, S, nh, hd] or None (forward only), bf16 (strided views fine); lens: B ints or
    None.  Returns a dict of fp64 tensors: O, dQ [B, S, nh, hd], lse [B, nh, S], dK, dV [B, S, nkv, hd], the units u_<name> of the same
    shapes, and with keep=True P, dP [B, nh, S, S] and delta [B, nh, S]."""
    return _attn(q, k, v, do, scale, causal, lens, F64, False, None, keep)


def attn_model(q, k, v, do, scale, causal, lens=None, hooks=None):
    """The kernels' arithmetic as their header comments state it: fp32 with bf16 rounding of P (before P V and before the dV product),
    O, dS and the outputs; P in the backward from the fp32 lse; delta from the bf16 O.  hooks: a seeded fault (FAULTS)."""
    return _attn(q, k, v, do, scale, causal, lens, F32, True, hooks)


def _decode(q, kc, vc, lens, nh, nkv, hd, scale, dt, model, hooks=None):
    hooks = hooks or {}
    B, smax = q.shape[0], kc.shape[1]
    group = nh // nkv
    out = torch.zeros(B, nh, hd, dtype=dt, device=q.device)
    unit = torch.zeros(B, nh, hd, dtype=dt, device=q.device)
    for b in range(B):
        L = max(0, min(int(lens[b]), smax))
        if L == 0:
            continue
        for h in range(nh):
            hk = h // group
            Kh, V = kc[b, :L, hk * hd:(hk + 1) * hd].to(dt), vc[b, :L, hk * hd:(hk + 1) * hd].to(dt)
            s = Kh @ (q[b, h * hd:(h + 1) * hd].to(dt) * scale)
            if model:
                # the decode kernel's online softmax over 256-key chunks, fp32 throughout (no bf16 rounding of P), one rounding of the output
                dev = q.device
                m, l, o = torch.tensor(NEG_INF, dtype=dt, device=dev), torch.zeros((), dtype=dt, device=dev), torch.zeros(hd, dtype=dt, device=dev)
                for ci, c0 in enumerate(range(0, L, 256)):
                    sc = s[c0:c0 + 256]
                    mn = torch.maximum(m, sc.amax())
                    alpha = torch.exp(m - mn)
                    if hooks.get("skip_rescale") == ci:
                        alpha = torch.ones((), dtype=dt)
                    p = torch.exp(sc - mn)
                    l = l * alpha + p.sum()
                    o = o * alpha + p @ V[c0:c0 + 256]
                    m = mn
                out[b, h] = (o / l).to(BF).to(dt)
            else:
                p = torch.softmax(s, 0)
                out[b, h] = p @ V
                unit[b, h] = p @ V.abs()
    return out.reshape(B, nh * hd), unit.reshape(B, nh * hd)


def decode_ref64(q, kcache, vcache, lens, nh, nkv, hd, scale):
    """q [B, >= nh*hd], caches [B, smax, >= nkv*hd] (strided views fine), lens [B] -> (out, u_O) [B, nh*hd] fp64.  Keys
    0 .. min(lens[b], smax) - 1 are valid; lens[b] <= 0: zeros (the kernel's contract)."""
    return _decode(q, kcache, vcache, lens, nh, nkv, hd, scale, F64, False)


def decode_model(q, kcache, vcache, lens, nh, nkv, hd, scale, hooks=None):
    return _decode(q, kcache, vcache, lens, nh, nkv, hd, scale, F32, True, hooks)[0]


# ------------------------------------------------------------------------------------------ inputs
def hot_key(qi, L, causal, S):
    """The key query row qi is made hot on (None: no bump), by qi % 4 (ragged launches: % 5): 0 itself (the causal diagonal; non-causal or
    padded rows: the last valid key), 1 key 0, 2 the last key before its 64-key tile boundary, 3 none, 4 the last valid key len - 1."""
    if L <= 0:
        return None
    last = min(qi, L - 1) if causal else L - 1              # the last key this row can see
    c = qi % (5 if L < S else 4)
    if c == 0:
        return last
    if c == 1:
        return 0
    if c == 2:
        t = (last + 1) // 64 * 64 - 1                        # last key of the last COMPLETE 64-key tile in view
        return t if t >= 0 else last
    if c == 3:
        return None
    return L - 1 if (not causal or qi >= L - 1) else last


def make_case(kind, B, S, nh, nkv, hd, causal, lens=None, seed=0, do_kind="normal", device="cpu"):
    """Deterministic inputs q [B, S, nh, hd], k, v [B, S, nkv, hd], do [B, S, nh, hd] (bf16) and scale.  kind:
      diffuse  N(0, 1), scale 1/sqrt(hd): unit-variance scores, a late row spreads its mass over ~S keys;
      hot      diffuse, then every query gets +8 in score on the key `hot_key` names, by a bump on the QUERY side
               (q_i += (8 / scale) k_h / |k_h|^2, so queries sharing a hot key do not collide).  Ragged samples: the pad keys
               k[len:] are copies of k[len - 1] — a hot key for every fifth row — so a key mask that lets key `len` through
               doubles that row's dominant mass instead of adding 1/S of it;
      spike    q, k ~ 0.3 N(0, 1); one late key (0.78 S) dominates one later query (0.88 S) by a score of ~40;
      creep    the running maximum creeps up by ~1.5 per 64-key tile for every query (below the deferred-rescale threshold).
    do_kind: normal N(0, 1); pad_only: zero except on padded query rows (q >= lens[b])."""
    g = torch.Generator().manual_seed(1000003 * seed + 7919 * S + 131 * nh + hd + (1 if causal else 0))
    rn = lambda *s: torch.randn(*s, generator=g)
    scale = 1.0 / math.sqrt(hd)
    q, k, v = rn(B, S, nh, hd), rn(B, S, nkv, hd), rn(B, S, nkv, hd)
    group = nh // nkv
    if kind == "hot":
        k = k.to(BF).float()
        for b in range(B):
            L = S if lens is None else int(lens[b])
            if 0 < L < S:
                k[b, L:] = k[b, L - 1]
            hk = [hot_key(i, L, causal, S) for i in range(S)]
            rows = torch.tensor([i for i in range(S) if hk[i] is not None], dtype=torch.long)
            if rows.numel() == 0:
                continue
            keys = torch.tensor([hk[i] for i in rows.tolist()], dtype=torch.long)
            for h in range(nh):
                kh = k[b, keys, h // group]                                   # [rows, hd]
                q[b, rows, h] += (8.0 / scale) * kh / (kh * kh).sum(-1, keepdim=True)
    elif kind == "spike":
        q, k = 0.3 * q, 0.3 * k
        qi, ki = max(0, int(0.88 * S) - 1), max(0, int(0.78 * S) - 1)
        for h in range(nh):
            k[:, ki, h // group] = q[:, qi, h].to(BF).float() * 40.0 / (scale * (q[:, qi, h].to(BF).float() ** 2).sum(-1, keepdim=True))
    elif kind == "creep":
        d = rn(hd)
        d = d / d.norm()
        q = d * math.sqrt(hd) + 0.05 * q
        k = d * (torch.arange(S)[None, :, None, None] // 64).float() * 1.5 + 0.05 * k
    elif kind != "diffuse":
        raise ValueError(kind)
    do = rn(B, S, nh, hd)
    if do_kind == "pad_only":
        ln = torch.tensor([S] * B if lens is None else [int(x) for x in lens])
        do = do * (torch.arange(S)[None, :] >= ln[:, None])[:, :, None, None]
    elif do_kind != "normal":
        raise ValueError(do_kind)
    return tuple(t.to(BF).to(device) for t in (q, k, v, do)) + (scale,)


def make_decode_case(kind, B, smax, lens, nh, nkv, hd, seed=0, device="cpu"):
    """q [B, nh*hd], kcache / vcache [B, smax, nkv*hd] bf16 and scale.  diffuse: N(0, 1); hot: the LAST valid key gets +8 in score for
    every query head; spike: key 300 of a 600-key sample dominates by ~40 (q, k ~ 0.3 N(0, 1))."""
    g = torch.Generator().manual_seed(7 + 1000003 * seed + smax + 31 * nh + hd)
    scale = 1.0 / math.sqrt(hd)
    f = 0.3 if kind == "spike" else 1.0
    q = f * torch.randn(B, nh, hd, generator=g)
    kc = f * torch.randn(B, smax, nkv, hd, generator=g)
    vc = torch.randn(B, smax, nkv, hd, generator=g)
    group = nh // nkv
    for b in range(B):
        L = max(0, min(int(lens[b]), smax))
        if L == 0:
            continue
        if kind == "hot":
            kb = kc.to(BF).float()
            for h in range(nh):
                kh = kb[b, L - 1, h // group]
                q[b, h] += (8.0 / scale) * kh / (kh * kh).sum()
        elif kind == "spike":
            key = min(300, L - 1)
            for hk in range(nkv):
                qh = q[b, hk * group].to(BF).float()
                kc[b, key, hk] = qh * 40.0 / (scale * (qh * qh).sum())
    return (q.reshape(B, nh * hd).to(BF).to(device), kc.reshape(B, smax, nkv * hd).to(BF).to(device),
            vc.reshape(B, smax, nkv * hd).to(BF).to(device), scale)


# ------------------------------------------------------------------------------------------ seeded faults
def _last_block(S):
    return (S - 1) // 256 * 256


def _f_diag(vis, S, L, causal):               # causal `<=` -> `<` for the queries of the last 256-row block
    vis = vis.clone()
    i = torch.arange(_last_block(S), S, device=vis.device)
    vis[i, i] = False
    return vis


def _f_len_minus(vis, S, L, causal):          # key mask `k < len - 1`
    vis = vis.clone()
    if L >= 1:
        vis[:, L - 1] = False
    return vis


def _f_len_plus(vis, S, L, causal):           # key mask `k < len + 1`
    vis = vis.clone()
    if L < S:
        ar = torch.arange(S, device=vis.device)
        vis[:, L] = (ar >= L) if causal else torch.ones_like(ar, dtype=torch.bool)
    return vis


def _drop(width):
    def f(vis, S, L, causal):                 # the `width` keys that end at the last query block's first row: invisible to that block
        vis = vis.clone()
        o0 = _last_block(S)
        vis[o0:, max(0, o0 - width):o0] = False
        return vis
    return f


# name -> (hooks for attn_model / decode_model, the geometry the fault needs: "causal" | "ragged" | "gqa" | "any" | "decode")
FAULTS = {
    "causal_diag_last_block": ({"mask": _f_diag}, "causal"),
    "len_mask_minus_one": ({"mask": _f_len_minus}, "ragged"),
    "len_mask_plus_one": ({"mask": _f_len_plus}, "ragged"),
    "drop_32_key_tile": ({"mask": _drop(32)}, "causal"),
    "drop_64_key_tile": ({"mask": _drop(64)}, "causal"),
    "gqa_map_modulo": ({"head_map": lambda h, nh, nkv: h % nkv}, "gqa"),
    "dk_without_scale": ({"dk_scale": 1.0}, "any"),
    "ds_without_delta": ({"no_delta": True}, "any"),
    "lse_off_by_2^-7": ({"lse_shift": 2.0 ** -7}, "any"),
    "decode_skipped_rescale": ({"skip_rescale": 1}, "decode"),       # the chunk of keys 256 .. 511 does not rescale what came before
}
