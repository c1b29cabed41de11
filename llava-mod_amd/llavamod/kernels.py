"""Functional (non-autograd) wrappers over the C-ABI kernels: allocate outputs, pass raw pointers.

Every function here launches hand-written HIP kernels through `_hip.call`; there is no torch
compute in this file (torch only allocates device memory).  Tensors are bf16 unless noted.
"""
import os

import torch

from . import _hip
from ._hip import call, ptr

BF16 = torch.bfloat16


def _chk(t, dtype=None):
    assert t.is_cuda and t.is_contiguous(), "device-resident contiguous tensor required"
    if dtype is not None:
        assert t.dtype == dtype, f"expected {dtype}, got {t.dtype}"
    return t


# ------------------------------------------------------------------------------------------ GEMM
def gemm_nt(a, b, bias=None, *, out=None, act=0, out_f32=False, accumulate=False, m_valid=None, k_valid=None,
            M=None, N=None, K=None, lda=None, ldb=None, ldc=None, batch=1, strides=(0, 0, 0)):
    """out[M,N] (+)= act(a[M,K] @ b[N,K]^T + bias).  2-D tensors by default; explicit dims/strides for
    sub-matrix and batched (grouped) use."""
    if M is None:
        M, K = a.shape[-2], a.shape[-1]
        N = b.shape[-2]
        lda, ldb = a.stride(-2), b.stride(-2)
        if a.dim() == 3:
            batch = a.shape[0]
            strides = (a.stride(0), b.stride(0) if b.dim() == 3 else 0, None)
    if out is None:
        shape = (batch, M, N) if (a.dim() == 3) else (M, N)
        out = torch.empty(shape, device=a.device, dtype=torch.float32 if out_f32 else BF16)
    if ldc is None:
        ldc = out.stride(-2)
    sA, sB, sC = strides
    if sC is None:
        sC = out.stride(0) if out.dim() == 3 else 0
    call("lmod_gemm_bf16_nt", ptr(a), ptr(b), ptr(out), ptr(bias), M, N, K, lda, ldb, ldc, batch, sA, sB, sC,
         ptr(m_valid), ptr(k_valid), act, int(out_f32), int(accumulate))
    return out


def gemm_res_fusable(M, w, res):
    """Can `gemm_nt_res` take the projection of a contiguous [M, K] operand through w [N, K] with residual res [M, N]?  Mirrors
    lmod_gemm_bf16_nt's choice of the 4-wave 256-tile kernel (gemm.hip) — the only kernel with the residual epilogue;
    LMOD_GEMM_RES=0 switches the fusion off (A/B runs)."""
    if os.environ.get("LMOD_GEMM_RES", "1") == "0" or os.environ.get("LMOD_GEMM_WAVES", "0") not in ("", "0"):
        return False
    if res is None or res.dim() != 2 or res.stride(1) != 1 or w.dim() != 2 or w.stride(1) != 1:
        return False
    N, Kd = w.shape
    if tuple(res.shape) != (M, N) or N % 8 or Kd % 8 or w.stride(0) % 8 or res.stride(0) % 8 or res.data_ptr() % 16:
        return False
    t256 = ((M + 255) // 256) * ((N + 255) // 256)
    big = M >= 512 and N >= 256 and (t256 >= 160 or (t256 >= 96 and Kd >= 8192)) and \
        ((M + 255) // 256 * 256) * ((N + 255) // 256 * 256) <= M * N * 115 // 100 + 65536
    return big and 255 * Kd * 2 + Kd * 2 < 0x7fffffff and 255 * w.stride(0) * 2 + Kd * 2 < 0x7fffffff


def gemm_nt_res(x, w, res, out=None):
    """out[M, N] = bf16(res + bf16(x @ w^T)): a bias-free projection with the residual add in the GEMM epilogue (bit-identical to
    gemm_nt followed by the residual path of rmsnorm_fwd)."""
    M, Kd = x.shape
    N = w.shape[0]
    if out is None:
        out = torch.empty((M, N), device=x.device, dtype=BF16)
    rc = call("lmod_gemm_bf16_nt_res", ptr(x), ptr(w), ptr(out), None, ptr(res), M, N, Kd, x.stride(0), w.stride(0), out.stride(0),
              res.stride(0), allow=(_hip.UNSUPPORTED,))
    if rc == _hip.UNSUPPORTED:
        # a shape (or a build: G4_ASM=0, LMOD_GEMM_WAVES) the residual-epilogue kernel does not take, although `gemm_res_fusable`
        # — a mirror of the library's test — said yes: the header's two-step form, same roundings (bf16(res + bf16(acc)))
        gemm_nt(x, w, out=out)
        add(out, res if res.is_contiguous() else res.contiguous(), out=out)
    return out


def qkv_rope_fusable(x, w, nrot_heads, hd, out=None):
    """Can `gemm_qkv_rope` take this projection?  (head dim 128; an even number of rotated heads so that the q|k block ends on
    a 256-column tile boundary; enough rows for the 256-tile kernel to be the right choice.)"""
    return hd == 128 and nrot_heads % 2 == 0 and w.shape[0] % 16 == 0 and x.shape[0] >= 512


def gemm_qkv_rope(x, w, bias, cos_t, sin_t, pos, nrot_heads, out=None):
    """out[T, N] = rope(x @ w^T + bias) on the first nrot_heads heads of 128 (q and k), v columns untouched: the fused
    QKV projection with the rotary embedding in the GEMM epilogue (bit-identical to gemm_nt + rope_)."""
    T, Kd = x.shape
    N = w.shape[0]
    if out is None:
        out = torch.empty((T, N), device=x.device, dtype=BF16)
    call("lmod_gemm_qkv_rope_bf16", ptr(x), ptr(w), ptr(out), ptr(bias), T, N, Kd, x.stride(0), w.stride(0), out.stride(0),
         ptr(cos_t), ptr(sin_t), ptr(pos), nrot_heads * 128)
    return out


def gemm_swiglu(x, w_gu, act=None, gu=None, want_gu=False, m_valid=None):
    """act[.., M, I] = silu(x @ Wg^T) * (x @ Wu^T) for the fused gate-over-up weight w_gu [.., 2I, K] in ONE GEMM launch
    (SwiGLU in the epilogue).  x: [M, K] or [E, M, K] (grouped, weights [E, 2I, K] or shared [2I, K]).
    gu (or want_gu): also store the [.., M, 2I] pre-activations for the backward.  Returns (act, gu-or-None)."""
    M, Kd = x.shape[-2], x.shape[-1]
    I = w_gu.shape[-2] // 2
    batch = x.shape[0] if x.dim() == 3 else 1
    lead = (batch,) if x.dim() == 3 else ()
    if act is None:
        act = torch.empty(lead + (M, I), device=x.device, dtype=BF16)
    if gu is None and want_gu:
        gu = torch.empty(lead + (M, 2 * I), device=x.device, dtype=BF16)
    call("lmod_gemm_swiglu_bf16", ptr(x), ptr(w_gu), ptr(act), ptr(gu), M, I, Kd, x.stride(-2), w_gu.stride(-2),
         act.stride(-2), gu.stride(-2) if gu is not None else 0, batch,
         x.stride(0) if x.dim() == 3 else 0, w_gu.stride(0) if w_gu.dim() == 3 else 0,
         act.stride(0) if act.dim() == 3 else 0, (gu.stride(0) if gu.dim() == 3 else 0) if gu is not None else 0,
         ptr(m_valid))
    return act, gu


def gemm_swiglu_bwd(dy, wt_down, gu, out=None, m_valid=None, K=None):
    """dgu[.., M, 2I] = SwiGLU backward of dact = dy[.., M, H] @ wt_down[.., I, Hpad]^T against the saved gu = [gate | up]:
    the down-projection dgrad GEMM with swiglu_bwd in its epilogue.  out may be gu itself (in place)."""
    M, Kd = dy.shape[-2], (K if K is not None else dy.shape[-1])
    I = wt_down.shape[-2]
    batch = dy.shape[0] if dy.dim() == 3 else 1
    if out is None:
        out = torch.empty_like(gu)
    call("lmod_gemm_swiglu_bwd_bf16", ptr(dy), ptr(wt_down), ptr(gu), ptr(out), M, I, Kd, dy.stride(-2), wt_down.stride(-2),
         gu.stride(-2), out.stride(-2), batch, dy.stride(0) if dy.dim() == 3 else 0,
         wt_down.stride(0) if wt_down.dim() == 3 else 0, gu.stride(0) if gu.dim() == 3 else 0,
         out.stride(0) if out.dim() == 3 else 0, ptr(m_valid))
    return out


_WGRAD_WS = {}
WGRAD_WS_BYTES = 512 << 20


def gemm_wgrad(at, b, out, b_kmajor=False, a_kmajor=False):
    """out (fp32 [M, N]) += at[M, K] @ X with X = b[N, K]^T (b_kmajor False) or b[K, N] as autograd holds the layer
    input (b_kmajor True: no transposed copy of it).  a_kmajor: `at` is dY [K, M] as autograd holds it too (dW = dY^T X with no
    transposed copy of either operand: the 4-wave TN kernel).  Deterministic split-K when the output has too few tiles to fill
    the GPU (K = tokens).  One zero-initialised workspace per device, reused by every call on the compute stream."""
    key = at.device.index
    ws = _WGRAD_WS.get(key)
    if ws is None:
        ws = _WGRAD_WS[key] = torch.zeros(WGRAD_WS_BYTES, device=at.device, dtype=torch.uint8)
    if a_kmajor:
        Kd, M = at.shape
        Kd = min(Kd, b.shape[0])
        N = b.shape[1]
        mode = 2
    else:
        M, Kd = at.shape
        if b_kmajor:
            Kd = min(Kd, b.shape[0])              # at is zero-padded to a multiple of 8 tokens by the transpose
        N = b.shape[1] if b_kmajor else b.shape[0]
        mode = int(b_kmajor)
    call("lmod_gemm_wgrad_bf16_nt", ptr(at), ptr(b), ptr(out), M, N, Kd, at.stride(0), b.stride(0),
         out.stride(0), mode, ptr(ws), ws.numel())
    return out


def gemm_tn(a, b, out=None, out_f32=True, accumulate=False, k_valid=None, K=None):
    """out[.., M, N] (+)= a^T @ b with a [.., Kd, M], b [.., Kd, N] (reduction-major: dW = dY^T X without transposes).
    K: reduce over the first K rows only."""
    Kd, M = a.shape[-2], a.shape[-1]
    N = b.shape[-1]
    if K is not None:
        Kd = K
    batch = a.shape[0] if a.dim() == 3 else 1
    if out is None:
        out = torch.empty(((batch,) if a.dim() == 3 else ()) + (M, N), device=a.device,
                          dtype=torch.float32 if out_f32 else BF16)
    call("lmod_gemm_bf16_tn", ptr(a), ptr(b), ptr(out), M, N, Kd, a.stride(-2), b.stride(-2), out.stride(-2), batch,
         a.stride(0) if a.dim() == 3 else 0, b.stride(0) if b.dim() == 3 else 0, out.stride(0) if out.dim() == 3 else 0,
         ptr(k_valid), int(out_f32), int(accumulate))
    return out


def transpose(x, ld_out=None, out=None, r_valid=None):
    """[.., R, C] -> [.., C, roundup(R,8)] (zero padded).  r_valid (int32 [batch]): live rows per batch entry; columns past
    roundup(r_valid, 8) of the result are left untouched (a k_valid GEMM never reads them)."""
    R, C = x.shape[-2], x.shape[-1]
    batch = x.shape[0] if x.dim() == 3 else 1
    if ld_out is None:
        ld_out = (R + 7) // 8 * 8
    if out is None:
        shape = (batch, C, ld_out) if x.dim() == 3 else (C, ld_out)
        out = torch.empty(shape, device=x.device, dtype=BF16)
    call("lmod_transpose_bf16", ptr(x), ptr(out), R, C, x.stride(-2), ld_out, batch,
         x.stride(0) if x.dim() == 3 else 0, out.stride(0) if out.dim() == 3 else 0, ptr(r_valid))
    return out


# ------------------------------------------------------------------------------------------ rows
def rmsnorm_fwd(x, w, eps, res=None, want_h=True):
    T, H = x.shape
    y = torch.empty_like(x)
    rstd = torch.empty(T, device=x.device, dtype=torch.float32)
    h = torch.empty_like(x) if (res is not None and want_h) else None
    call("lmod_rmsnorm_fwd", ptr(x), ptr(res), ptr(w), ptr(h), ptr(y), ptr(rstd), T, H, float(eps))
    return y, rstd, (h if res is not None else x)


def rmsnorm_bwd(dy, h, w, rstd, dres=None):
    T, H = h.shape
    dh = torch.empty_like(h)
    call("lmod_rmsnorm_bwd", ptr(dy), ptr(h), ptr(w), ptr(rstd), ptr(dres), ptr(dh), T, H)
    return dh


def rmsnorm_dw(dy, h, rstd, dw, accumulate=True):
    T, H = h.shape
    ws = torch.empty(64 * H, device=h.device, dtype=torch.float32)
    call("lmod_rmsnorm_dw", ptr(dy), ptr(h), ptr(rstd), ptr(dw), ptr(ws), T, H, int(accumulate))
    return dw


def embed_wgrad(d_embeds, idx, dW):
    call("lmod_embed_wgrad", ptr(d_embeds), ptr(idx), ptr(dW), d_embeds.shape[0], d_embeds.shape[1])
    return dW


def layernorm_fwd(x, w, b, eps):
    T, H = x.shape
    y = torch.empty_like(x)
    call("lmod_layernorm_fwd", ptr(x), ptr(w), ptr(b), ptr(y), T, H, float(eps))
    return y


def rope_(buf, cos_t, sin_t, pos, nheads, hd, backward=False):
    T, ld = buf.shape[0], buf.stride(0)
    call("lmod_rope", ptr(buf), ptr(cos_t), ptr(sin_t), ptr(pos), T, nheads, hd, ld, int(backward))
    return buf


def swiglu_fwd(gate, up, out=None, seg_rows=0, seg_valid=None):
    rows, I = gate.shape
    if out is None:
        out = torch.empty((rows, I), device=gate.device, dtype=BF16)
    call("lmod_swiglu_fwd", ptr(gate), ptr(up), ptr(out), rows, I, gate.stride(0), up.stride(0), out.stride(0),
         seg_rows, ptr(seg_valid))
    return out


def swiglu_bwd(dact, gate, up, dgate=None, dup=None, seg_rows=0, seg_valid=None):
    rows, I = gate.shape
    if dgate is None:
        dgate = torch.empty((rows, I), device=gate.device, dtype=BF16)
    if dup is None:
        dup = torch.empty((rows, I), device=gate.device, dtype=BF16)
    call("lmod_swiglu_bwd", ptr(dact), ptr(gate), ptr(up), ptr(dgate), ptr(dup), rows, I, dact.stride(0),
         gate.stride(0), up.stride(0), dgate.stride(0), dup.stride(0), seg_rows, ptr(seg_valid))
    return dgate, dup


def gelu_fwd(x):
    y = torch.empty_like(x)
    call("lmod_gelu_fwd", ptr(x), ptr(y), x.numel())
    return y


def gelu_bwd(dy, x):
    dx = torch.empty_like(x)
    call("lmod_gelu_bwd", ptr(dy), ptr(x), ptr(dx), x.numel())
    return dx


def add(a, b, out=None):
    if out is None:
        out = torch.empty_like(a)
    call("lmod_add_bf16", ptr(a), ptr(b), ptr(out), a.numel())
    return out


def gather_rows(src_a, src_b, idx, H):
    rows = idx.numel()
    out = torch.empty((rows, H), device=idx.device, dtype=BF16)
    call("lmod_gather_rows", ptr(src_a), ptr(src_b), ptr(idx), ptr(out), rows, H)
    return out


def im2col_patch(pixels, patch, kpad):
    B, _, S, _ = pixels.shape
    G = S // patch
    out = torch.empty((B * G * G, kpad), device=pixels.device, dtype=BF16)
    call("lmod_im2col_patch", ptr(pixels), ptr(out), B, S, patch, kpad)
    return out


def vit_embed(patch_emb, cls, pos, B, n_patches):
    D = patch_emb.shape[-1]
    out = torch.empty((B * (n_patches + 1), D), device=patch_emb.device, dtype=BF16)
    call("lmod_vit_embed", ptr(patch_emb), ptr(cls), ptr(pos), ptr(out), B, n_patches, D)
    return out


def adamw_step(master, param, grad, m, v, lr, beta1, beta2, eps, wd, step, grad_scale=1.0, zero_grad=False,
               dev_scale=None):
    call("lmod_adamw_step", ptr(master), ptr(param), ptr(grad), ptr(m), ptr(v), master.numel(), float(lr),
         float(beta1), float(beta2), float(eps), float(wd), int(step), float(grad_scale), int(zero_grad), ptr(dev_scale))


def sumsq(x, out, partials, accumulate=False):
    """out[0] (+)= sum(x^2) for a contiguous fp32 tensor (deterministic)."""
    call("lmod_sumsq_f32", ptr(x), x.numel(), ptr(partials), ptr(out), int(accumulate))
    return out


def clip_coef(sumsq_t, norm_scale, max_norm, coef, norm_out=None):
    call("lmod_clip_coef", ptr(sumsq_t), float(norm_scale), float(max_norm), ptr(coef), ptr(norm_out))
    return coef


def cast_f32_bf16(src, dst):
    """Elementwise fp32 -> bf16 or bf16 -> fp32 between two contiguous tensors of equal numel."""
    to_bf16 = src.dtype == torch.float32
    assert dst.dtype == (BF16 if to_bf16 else torch.float32) and src.numel() == dst.numel()
    call("lmod_cast_f32_bf16", ptr(src), ptr(dst), src.numel(), int(to_bf16))
    return dst


# ------------------------------------------------------------------------------------------ attention
def attn_fwd(q, k, v, B, S, nh, nkv, hd, scale, causal, seqlens=None, want_lse=True, cu=None):
    """q/k/v: 2-D views [T, ld] whose column 0 is head 0 (views into a fused QKV buffer are fine).  Padded layout: T = B*S,
    sample b at rows b*S.., keys >= seqlens[b] masked.  Packed (cu [B+1] int32, hd 128): T = cu[B], S = longest sample."""
    o = torch.empty((q.shape[0], nh * hd), device=q.device, dtype=BF16)
    lse = torch.empty((B, nh, S), device=q.device, dtype=torch.float32) if want_lse else None
    call("lmod_attn_fwd", ptr(q), ptr(k), ptr(v), ptr(o), ptr(lse), ptr(seqlens), ptr(cu), B, S, nh, nkv, hd, q.stride(0),
         k.stride(0), v.stride(0), o.stride(0), float(scale), int(causal))
    return o, lse


def attn_bwd_rope_fusable(hd):
    """lmod_attn_bwd_rope exists in the hd-128 kernels of attn_bwd2.hip only (not in the generic LMOD_ATTN_BWD=1 path)."""
    import os
    return hd == 128 and os.environ.get("LMOD_ATTN_BWD") != "1"


def attn_bwd(q, k, v, o, do, lse, dq, dk, dv, B, S, nh, nkv, hd, scale, causal, seqlens=None, cu=None, rope=None, split=True):
    """rope = (cos_t, sin_t, pos): also apply the rotary embedding's gradient map to dq / dk in the kernels' epilogues.
    split=False: never use the head-split form of the dK/dV launch (tests, A/B timing)."""
    delta = torch.empty((B, nh, S), device=q.device, dtype=torch.float32)
    args = (ptr(q), ptr(k), ptr(v), ptr(o), ptr(do), ptr(lse), ptr(delta), ptr(dq), ptr(dk), ptr(dv),
            ptr(seqlens), ptr(cu), B, S, nh, nkv, hd, q.stride(0), k.stride(0), v.stride(0), o.stride(0), do.stride(0),
            dq.stride(0), dk.stride(0), dv.stride(0), float(scale), int(causal))
    rp = (ptr(rope[0]), ptr(rope[1]), ptr(rope[2])) if rope is not None else (None, None, None)
    # few KV heads (grouped-query students): the dK/dV kernel's grid is cut along the query-head group, fp32 partial sums in `ws`
    ns = _hip.load().lmod_attn_bwd_nsplit(B, S, nh, nkv, hd, int(causal)) if (cu is None and split and rope is None) else 1
    if ns > 1:
        ws = torch.empty(ns * 2 * B * S * nkv * hd, device=q.device, dtype=torch.float32)
        call("lmod_attn_bwd_split", *args, None, None, None, ptr(ws), ws.numel() * 4)
    elif attn_bwd_ds_fusable(B, S, nh, hd, cu):
        # dS spill: the dK/dV kernel stores dS^T into the (cached, per device) workspace and dQ is one batched TN GEMM; the dQ kernel's
        # recomputation of S, dP and the exponentials is gone (include/lmod_hip.h, lmod_attn_bwd_split)
        ws = _ds_workspace(q.device, B * nh * S * S * 2)
        call("lmod_attn_bwd_split", *args, *rp, ptr(ws), ws.numel())
    elif rope is not None:
        call("lmod_attn_bwd_rope", *args, *rp)
    else:
        call("lmod_attn_bwd", *args)
    return dq, dk, dv


_DS_WS = {}
DS_WS_MAX_BYTES = 8 << 30


def attn_bwd_ds_fusable(B, S, nh, hd, cu=None):
    """The dS-spill form of the attention backward (5 matmuls instead of 7) applies to hd 128, dense layouts and whole 256-row blocks;
    its workspace is B * nh * S^2 bf16 (2.1 GB at B 16, 16 heads, S 2048), bounded here; LMOD_ATTN_DS=0 keeps the two-kernel form."""
    return (hd == 128 and cu is None and S % 256 == 0 and os.environ.get("LMOD_ATTN_DS", "1") != "0"
            and B * nh * S * S * 2 <= DS_WS_MAX_BYTES)


def _ds_workspace(device, nbytes):
    """One workspace per device, grown on demand, shared by every layer's backward (launches on one stream are ordered: the dQ GEMM of
    layer l has read it before layer l - 1's dK/dV kernel writes it)."""
    w = _DS_WS.get(device)
    if w is None or w.numel() < nbytes:
        _DS_WS[device] = w = torch.empty(nbytes, device=device, dtype=torch.uint8)
    return w


def row_argmax(logits):
    R, V = logits.shape
    out = torch.empty(R, device=logits.device, dtype=torch.int32)
    call("lmod_row_argmax_bf16", ptr(logits), logits.stride(0), V, ptr(out), R)
    return out


def attn_decode(q, kcache, vcache, lens, nh, nkv, hd, scale):
    """q [B, nh*hd] (views fine), caches [B, Smax, nkv*hd] with lens[b] valid keys -> out [B, nh*hd]."""
    B = q.shape[0]
    out = torch.empty((B, nh * hd), device=q.device, dtype=BF16)
    call("lmod_attn_decode", ptr(q), ptr(kcache), ptr(vcache), ptr(lens), ptr(out), B, nh, nkv, hd, kcache.shape[1],
         q.stride(0), kcache.stride(1), out.stride(0), float(scale))
    return out


# ------------------------------------------------------------------------------------------ multi-token cache extension
APPEND_T_MAX = 16          # csrc/append.hip: tokens per sample in one chunk; (nh / nkv) * T <= 128 as well
EXTEND_T_MAX = 65535       # csrc/attn_extend.hip: rows per sample in one chunk (a grid dimension)
_APPEND_WS = {}


def attn_append_nsplit(B, nkv, smax):
    """The key-split count lmod_attn_append chooses by itself for these shapes (host-side query)."""
    return int(_hip.load().lmod_attn_append_nsplit(int(B), int(nkv), int(smax)))


def attn_append(q, kcache, vcache, lens, nh, nkv, hd, scale, T, cu_new=None, nsplit=0):
    """A chunk of new queries against caches that already hold the chunk's keys / values.  q [R, nh*hd] packed rows (views fine):
    sample b owns rows cu_new[b] .. cu_new[b+1]-1 (device int32 [B+1]; None: exactly T rows per sample), 0..T rows, T <= APPEND_T_MAX;
    lens [B] int32 = valid positions after the append.  Query t of sample b sees keys k <= lens[b] - n_b + t.  -> out [R, nh*hd].
    nsplit: 0 lets the library split the key range over workgroups, 1..32 forces a count (tests, timing)."""
    B = kcache.shape[0]
    assert q.dtype == BF16 and q.stride(1) == 1 and kcache.dtype == BF16 and vcache.dtype == BF16
    assert kcache.stride(2) == 1 and vcache.stride() == kcache.stride() and kcache.stride(0) == kcache.shape[1] * kcache.stride(1)
    assert lens.dtype == torch.int32 and lens.numel() == B and (cu_new is None or (cu_new.dtype == torch.int32 and cu_new.numel() == B + 1))
    assert cu_new is not None or q.shape[0] == B * T
    out = torch.empty((q.shape[0], nh * hd), device=q.device, dtype=BF16)
    ns = nsplit if nsplit else attn_append_nsplit(B, nkv, kcache.shape[1])
    ws, need = None, ns * B * nh * T * (hd + 2) * 4 if ns > 1 else 0
    if need:
        key = (q.device, _hip.stream())     # one workspace per device AND stream, grown on demand (launches on one stream are ordered)
        ws = _APPEND_WS.get(key)
        if ws is None or ws.numel() < need:
            _APPEND_WS[key] = ws = torch.empty(need, device=q.device, dtype=torch.uint8)
    call("lmod_attn_append", ptr(q), ptr(kcache), ptr(vcache), ptr(lens), ptr(cu_new), ptr(out), B, T, nh, nkv, hd, kcache.shape[1],
         q.stride(0), kcache.stride(1), out.stride(0), float(scale), ns, ptr(ws), need)
    return out


def attn_extend(q, kcache, vcache, lens, nh, nkv, hd, scale, T, cu_new=None):
    """attn_append's contract for chunks of any length (1 <= T <= 65535 rows per sample): the MFMA flash kernel of
    csrc/attn_extend.hip.  q [R, nh*hd] packed rows (views fine, row stride a multiple of 8), sample b owns rows
    cu_new[b] .. cu_new[b+1]-1 (None: exactly T rows each); lens [B] int32 = valid positions after the append.  -> out [R, nh*hd]."""
    B = kcache.shape[0]
    assert q.dtype == BF16 and q.stride(1) == 1 and kcache.dtype == BF16 and vcache.dtype == BF16
    assert kcache.stride(2) == 1 and vcache.stride() == kcache.stride() and kcache.stride(0) == kcache.shape[1] * kcache.stride(1)
    assert lens.dtype == torch.int32 and lens.numel() == B and (cu_new is None or (cu_new.dtype == torch.int32 and cu_new.numel() == B + 1))
    assert cu_new is not None or q.shape[0] == B * T
    out = torch.empty((q.shape[0], nh * hd), device=q.device, dtype=BF16)
    call("lmod_attn_extend", ptr(q), ptr(kcache), ptr(vcache), ptr(lens), ptr(cu_new), ptr(out), B, T, nh, nkv, hd, kcache.shape[1],
         q.stride(0), kcache.stride(1), out.stride(0), float(scale))
    return out


def kv_append_rows(qkv, kcol, vcol, width, kcache, vcache, lens_before, T, max_len_after, cu_new=None):
    """kcache[b, lens_before[b] + t] = qkv[row(b, t), kcol:kcol+width] and the same for vcache / vcol, one launch; row(b, t) =
    cu_new[b] + t (None: b*T + t).  max_len_after: host upper bound of lens_before[b] + n_b — beyond the cache's smax this raises
    (LMOD_EINVAL) instead of clamping."""
    B, smax = kcache.shape[0], kcache.shape[1]
    assert qkv.dtype == BF16 and qkv.stride(1) == 1 and kcache.dtype == BF16 and vcache.stride() == kcache.stride()
    assert kcache.stride(2) == 1 and kcache.stride(0) == smax * kcache.stride(1) and lens_before.dtype == torch.int32
    call("lmod_kv_append_rows", ptr(qkv), qkv.stride(0), kcol, vcol, width, ptr(cu_new), ptr(lens_before), ptr(kcache), ptr(vcache),
         B, T, smax, kcache.stride(1), int(max_len_after))


def spec_accept(draft, target, done, eos, pad, lens_target, lens_draft):
    """Greedy assisted decoding's acceptance rule on the device (lmod_spec_accept in include/lmod_hip.h).  draft [B, k], target
    [B, k+1], done [B], the two caches' lens [B]: int32, contiguous; done and the lens are updated in place.  Returns (block
    [B, k+5] int32: emitted tokens | n_acc | n_emitted | next_token | done, next_token [B] int32)."""
    B, k = draft.shape
    for t in (draft, target, done, lens_target, lens_draft):
        assert t.dtype == torch.int32 and t.is_contiguous()
    assert tuple(target.shape) == (B, k + 1) and done.numel() == B
    out = torch.empty((B, k + 5), device=draft.device, dtype=torch.int32)
    nxt = torch.empty(B, device=draft.device, dtype=torch.int32)
    call("lmod_spec_accept", ptr(draft), ptr(target), k, ptr(done), -1 if eos is None else int(eos), 0 if pad is None else int(pad),
         ptr(lens_target), ptr(lens_draft), ptr(out), ptr(nxt), B)
    return out, nxt


# ------------------------------------------------------------------------------------------ beam search
def beam_topk(logits, beam_scores, nb):
    """logits [B*nb, V] bf16 (row stride may exceed V), beam_scores [B*nb] fp32 -> one int32 block [3, B, 2*nb]: per sample the top
    2*nb of log_softmax(logits) + beam score over nb*V, sorted descending (ties: smaller beam*V + token); row 0 holds the scores
    (fp32 bits), row 1 the beam (0..nb-1), row 2 the token — one block, so the host reads the candidates back with one copy."""
    R, V = logits.shape
    assert logits.dtype == BF16 and logits.stride(1) == 1 and R % nb == 0
    assert beam_scores.dtype == torch.float32 and beam_scores.is_contiguous() and beam_scores.numel() == R
    B, K = R // nb, 2 * nb
    # ~384 workgroups over all rows (4 rows alone would fill 4 of 256 CUs), chunks of at least 512 tokens
    c_target = max(1, min(-(-384 // R), -(-V // 512)))
    chunk = (-(-V // c_target) + 7) // 8 * 8
    C = -(-V // chunk)
    ws = torch.empty(R * C * (2 + 2 * 16), device=logits.device, dtype=torch.float32)
    out = torch.empty((3, B, K), device=logits.device, dtype=torch.int32)
    call("lmod_beam_topk_bf16", ptr(logits), logits.stride(0), V, ptr(beam_scores), B, nb, chunk, ptr(ws), ws.numel() * 4,
         ptr(out[0]), ptr(out[1]), ptr(out[2]))
    return out


def ptr_table(tensors):
    """Device table (int64) of the data pointers of `tensors` (for kv_gather_rows)."""
    return torch.tensor([t.data_ptr() for t in tensors], dtype=torch.int64).to(tensors[0].device)


def kv_gather_rows(dst, src, src_row, lens, tables=None):
    """dst[t][r, :lens[r]] = src[t][src_row[r], :lens[r]] for every tensor pair (lists of contiguous [rows, smax, width] bf16
    caches, one width), one launch; positions >= lens[r] stay as they are.  tables: (ptr_table(dst), ptr_table(src)) when the
    caller keeps them.  dst and src must be different buffers."""
    assert len(dst) == len(src) and len(dst) > 0
    d0, s0 = dst[0], src[0]
    for d, s in zip(dst, src):
        assert d.dtype == BF16 and s.dtype == BF16 and d.is_contiguous() and s.is_contiguous()
        assert d.shape[0] == d0.shape[0] and d.shape[1:] == d0.shape[1:] and s.shape == s0.shape and s.shape[2] == d.shape[2]
    R = d0.shape[0]
    assert src_row.dtype == torch.int32 and lens.dtype == torch.int32 and src_row.numel() == R and lens.numel() == R
    dt, st = tables if tables is not None else (ptr_table(dst), ptr_table(src))
    call("lmod_kv_gather_rows", ptr(dt), ptr(st), len(dst), ptr(src_row.contiguous()), ptr(lens.contiguous()), R, s0.shape[0],
         d0.shape[1], s0.shape[1], d0.shape[2])


# ------------------------------------------------------------------------------------------ sampling
def sample(logits, u, temperature=1.0, top_k=None, top_p=None, stats=False):
    """logits [R, V] bf16 (row stride may exceed V), u [R] fp32 in [0, 1) on the device -> tokens int32 [R]: one draw per row from
    the temperature / top-k / top-p warped distribution (HF's warper order; lmod_sample_bf16 in include/lmod_hip.h).  stats=True
    also returns fp32 [R, 4]: {logsumexp of logits / T, kept mass fraction, number of kept tokens, cutoff logit}."""
    R, V = logits.shape
    assert logits.dtype == BF16 and logits.stride(1) == 1
    assert u.dtype == torch.float32 and u.is_cuda and u.is_contiguous() and u.numel() == R
    k = 0 if top_k is None else max(0, min(int(top_k), 2 ** 31 - 1))
    p = 1.0 if top_p is None else float(top_p)
    tokens = torch.empty(R, device=logits.device, dtype=torch.int32)
    st = torch.empty((R, 4), device=logits.device, dtype=torch.float32) if stats else None
    if R == 0:
        return (tokens, st) if stats else tokens
    # ~384 workgroups over all rows (one row alone would fill 1 of 256 CUs), chunks of at least 512 tokens: as beam_topk
    c_target = max(1, min(-(-384 // R), -(-V // 512)))
    chunk = (-(-V // c_target) + 7) // 8 * 8
    C = -(-V // chunk)
    nf = int(0 < k < V) + int(p < 1.0)
    ws = torch.empty(R * (64 + 3072 * (nf + 1 if nf else 0) + 16 * C), device=logits.device, dtype=torch.uint8)
    call("lmod_sample_bf16", ptr(logits), logits.stride(0), V, ptr(u), R, float(temperature), k, p, chunk, ptr(ws), ws.numel(),
         ptr(tokens), ptr(st))
    return (tokens, st) if stats else tokens


def sample_rows(logits, u, temperature, top_k, top_p, greedy, stats=False, chunk=None):
    """`sample` with the parameters of every row in device arrays [R] (lmod_sample_rows_bf16): temperature / top_p fp32, top_k /
    greedy int32 (top_k <= 0 and top_p >= 1 switch a filter off).  A row with greedy == 0 gets exactly `sample`'s token and stats for
    that row alone under its own parameters; a row with greedy != 0 gets `row_argmax`'s token and the stats {logsumexp of the
    logits, 1, V, -inf}.  Always six launches.  stats=True also returns fp32 [R, 4].  chunk (a multiple of 8; default: `sample`'s
    choice): tokens per workgroup — it changes the grid, never a result."""
    R, V = logits.shape
    assert logits.dtype == BF16 and logits.stride(1) == 1
    assert u.dtype == torch.float32 and u.is_cuda and u.is_contiguous() and u.numel() == R
    for t, dt in ((temperature, torch.float32), (top_k, torch.int32), (top_p, torch.float32), (greedy, torch.int32)):
        assert t.dtype == dt and t.is_cuda and t.is_contiguous() and t.numel() == R
    tokens = torch.empty(R, device=logits.device, dtype=torch.int32)
    st = torch.empty((R, 4), device=logits.device, dtype=torch.float32) if stats else None
    if R == 0:
        return (tokens, st) if stats else tokens
    if chunk is None:
        c_target = max(1, min(-(-384 // R), -(-V // 512)))             # the chunking of `sample`
        chunk = (-(-V // c_target) + 7) // 8 * 8
    C = -(-V // chunk)
    ws = torch.empty(R * (64 + 3072 * 3 + 16 * C), device=logits.device, dtype=torch.uint8)
    call("lmod_sample_rows_bf16", ptr(logits), logits.stride(0), V, ptr(u), R, ptr(temperature), ptr(top_k), ptr(top_p), ptr(greedy),
         chunk, ptr(ws), ws.numel(), ptr(tokens), ptr(st))
    return (tokens, st) if stats else tokens


# ------------------------------------------------------------------------------------------ speculative sampling
def spec_sample(p_logits, q_logits, draft, u_acc, u_draw, done, eos, pad, lens_target, lens_draft, temperature=1.0, top_k=None,
                top_p=None, stats=False):
    """Speculative sampling's verification on the device (lmod_spec_sample_bf16 in include/lmod_hip.h).  p_logits [B*(k+1), V] (the
    target's rows, row b*(k+1)+i) and q_logits [B*k, V] (the draft's, row b*k+i): bf16 with the same V live columns (row strides may
    exceed V); draft [B, k] int32; u_acc [B, k], u_draw [B] fp32 in [0, 1); done [B] and the two caches' lens [B]: int32, updated in
    place.  Accepts position i iff u_acc * q_i(d_i) < p_i(d_i) on the temperature / top-k / top-p warped distributions, draws the
    next token from the residual (or from p_k when every draft was accepted).  Returns (block [B, k+5] int32: emitted tokens | n_acc |
    n_emitted | next_token | done, next_token [B] int32); stats=True adds fp32 [B*(2k+1), 4], `sample`'s record of every row (p rows,
    then q rows)."""
    B, k = draft.shape
    for t in (draft, done, lens_target, lens_draft):
        assert t.dtype == torch.int32 and t.is_cuda and t.is_contiguous()
    for t in (u_acc, u_draw):
        assert t.dtype == torch.float32 and t.is_cuda and t.is_contiguous()
    for t in (p_logits, q_logits):
        assert t.dtype == BF16 and t.is_cuda and t.dim() == 2 and t.stride(1) == 1
    V = p_logits.shape[1]
    assert q_logits.shape[1] == V and p_logits.shape[0] == B * (k + 1) and q_logits.shape[0] == B * k
    assert u_acc.numel() == B * k and u_draw.numel() == B and done.numel() == B and lens_target.numel() == B and lens_draft.numel() == B
    R = B * (2 * k + 1)
    kk = 0 if top_k is None else max(0, min(int(top_k), 2 ** 31 - 1))
    p = 1.0 if top_p is None else float(top_p)
    out = torch.empty((B, k + 5), device=draft.device, dtype=torch.int32)
    nxt = torch.empty(B, device=draft.device, dtype=torch.int32)
    st = torch.empty((R, 4), device=draft.device, dtype=torch.float32) if stats else None
    if B == 0:
        return (out, nxt, st) if stats else (out, nxt)
    # chunks as `sample` cuts them for R rows
    c_target = max(1, min(-(-384 // R), -(-V // 512)))
    chunk = (-(-V // c_target) + 7) // 8 * 8
    C = -(-V // chunk)
    nf = int(0 < kk < V) + int(p < 1.0)
    ws = torch.empty(R * (64 + 3072 * (nf + 1 if nf else 0) + 16 * C) + B * (32 + 16 * C), device=draft.device, dtype=torch.uint8)
    call("lmod_spec_sample_bf16", ptr(p_logits), p_logits.stride(0), ptr(q_logits), q_logits.stride(0), V, ptr(draft), ptr(u_acc),
         ptr(u_draw), B, k, float(temperature), kk, p, chunk, ptr(ws), ws.numel(), ptr(done), -1 if eos is None else int(eos),
         0 if pad is None else int(pad), ptr(lens_target), ptr(lens_draft), ptr(out), ptr(nxt), ptr(st))
    return (out, nxt, st) if stats else (out, nxt)


SPEC_DRAFT, SPEC_ACCEPT, SPEC_DRAW = 0, 1, 2          # lmod_spec_uniform's purposes


def spec_uniform(seed, B, round, purpose, n_pos=1, row0=0, device="cuda", out=None):
    """u [B, n_pos] fp32 in [0, 1): Philox4x32-10 at counter (row0 + b, round, i, purpose) under the 64-bit key `seed` — the uniforms of
    the speculative loop as a pure function of their coordinates (lmod_spec_uniform)."""
    u = torch.empty((B, n_pos), device=device, dtype=torch.float32) if out is None else out
    assert u.dtype == torch.float32 and u.is_cuda and u.is_contiguous() and u.numel() == B * n_pos
    call("lmod_spec_uniform", int(seed) & 0xFFFFFFFFFFFFFFFF, int(row0), int(round), int(purpose), int(n_pos), ptr(u), B)
    return u


# ------------------------------------------------------------------------------------------ logits processors / stop sequences
LOGITS_MAX_SEQS = 16          # sequences in the bad-word table, and in the stop table
LOGITS_MAX_SEQ_LEN = 16       # tokens per sequence


def seq_table(seqs, device):
    """A list of token sequences as the device table the logits kernels read: (flat int32 [sum of lengths], off int32 [n + 1], n);
    None for an empty list.  One host -> device copy."""
    if not seqs:
        return None
    flat, off = [], [0]
    for s in seqs:
        flat.extend(int(t) for t in s)
        off.append(len(flat))
    both = torch.tensor(flat + off, dtype=torch.int32).to(device)
    return both[:len(flat)], both[len(flat):], len(seqs)


def logits_process_(logits, hist, n_hist, n_gen, penalty=1.0, ngram=0, bad=None, min_new=0, eos=None):
    """In place on logits [R, V] bf16 (row stride may exceed V): repetition penalty, no-repeat n-gram bans, bad-word bans and the
    min-new-tokens EOS ban from the history hist [R, L] / n_hist [R] / n_gen [R] (device int32), in HF's order
    (lmod_logits_process_bf16 in include/lmod_hip.h).  bad: a `seq_table` or None.  Returns logits."""
    R, V = logits.shape
    assert logits.dtype == BF16 and logits.is_cuda and logits.stride(1) == 1
    assert hist.dim() == 2 and hist.shape[0] == R and hist.stride(1) == 1
    for t in (hist, n_hist, n_gen):
        assert t.dtype == torch.int32 and t.is_cuda
    assert n_hist.is_contiguous() and n_gen.is_contiguous() and n_hist.numel() == R and n_gen.numel() == R
    bf, bo, nb = bad if bad is not None else (None, None, 0)
    rc = call("lmod_logits_process_bf16", ptr(logits), logits.stride(0), V, R, ptr(hist), hist.stride(0), ptr(n_hist), ptr(n_gen),
              float(penalty), int(ngram), ptr(bf), ptr(bo), nb, int(min_new), -1 if eos is None else int(eos),
              allow=(_hip.UNSUPPORTED,))
    if rc:
        raise ValueError(f"repetition_penalty needs a {V}-bit first-occurrence bitmap in LDS: a vocabulary above 524288 is not supported")
    return logits


def logits_process_rows_(logits, hist, n_hist, n_gen, penalty, ngram, min_new, any_penalty, bad=None, eos=None):
    """`logits_process_` with penalty (fp32, > 0), ngram and min_new (int32, >= 0) per row in device arrays [R]
    (lmod_logits_process_rows_bf16); the bad-word table and eos stay per call.  any_penalty: whether some penalty differs from 1 (the
    host knows; it requests the LDS bitmap).  Row r is exactly `logits_process_` on that row with its own scalars.  Returns logits."""
    R, V = logits.shape
    assert logits.dtype == BF16 and logits.is_cuda and logits.stride(1) == 1
    assert hist.dim() == 2 and hist.shape[0] == R and hist.stride(1) == 1
    for t in (hist, n_hist, n_gen, ngram, min_new):
        assert t.dtype == torch.int32 and t.is_cuda
    assert penalty.dtype == torch.float32 and penalty.is_cuda
    assert all(t.is_contiguous() and t.numel() == R for t in (n_hist, n_gen, penalty, ngram, min_new))
    bf, bo, nb = bad if bad is not None else (None, None, 0)
    rc = call("lmod_logits_process_rows_bf16", ptr(logits), logits.stride(0), V, R, ptr(hist), hist.stride(0), ptr(n_hist), ptr(n_gen),
              ptr(penalty), ptr(ngram), ptr(min_new), int(bool(any_penalty)), ptr(bf), ptr(bo), nb, -1 if eos is None else int(eos),
              allow=(_hip.UNSUPPORTED,))
    if rc:
        raise ValueError(f"repetition_penalty needs a {V}-bit first-occurrence bitmap in LDS: a vocabulary above 524288 is not supported")
    return logits


def gen_push_stop_rows_(tokens, done, hist, n_hist, n_prompt, n_gen, eos, pad, stop, n_call, stop_first, stop_count):
    """`gen_push_stop_` where row r tests the first n_call sequences of the stop table (`seq_table` or None) and its own range
    [stop_first[r], stop_first[r] + stop_count[r]) of it (device int32 [R]; lmod_gen_push_stop_rows)."""
    R = tokens.numel()
    for t in (tokens, done, hist, n_hist, n_prompt, n_gen, stop_first, stop_count):
        assert t.dtype == torch.int32 and t.is_cuda and t.is_contiguous()
    assert hist.dim() == 2 and hist.shape[0] == R
    assert all(t.numel() == R for t in (done, n_hist, n_prompt, n_gen, stop_first, stop_count))
    sf, so, ns = stop if stop is not None else (None, None, 0)
    assert 0 <= int(n_call) <= ns
    call("lmod_gen_push_stop_rows", ptr(tokens), ptr(done), ptr(hist), hist.shape[1], ptr(n_hist), ptr(n_prompt), ptr(n_gen),
         -1 if eos is None else int(eos), 0 if pad is None else int(pad), ptr(sf), ptr(so), int(n_call), ns, ptr(stop_first),
         ptr(stop_count), R)


def gen_push_stop_(tokens, done, hist, n_hist, n_prompt, n_gen, eos, pad, stop=None):
    """One generation step's bookkeeping on the device (lmod_gen_push_stop), everything int32 and updated in place: a done row's
    token becomes pad; a live row's token is appended to its history and done is set on EOS or when the row's generated tokens end
    with a sequence of the stop table (`seq_table` or None)."""
    R = tokens.numel()
    for t in (tokens, done, hist, n_hist, n_prompt, n_gen):
        assert t.dtype == torch.int32 and t.is_cuda and t.is_contiguous()
    assert hist.dim() == 2 and hist.shape[0] == R and all(t.numel() == R for t in (done, n_hist, n_prompt, n_gen))
    sf, so, ns = stop if stop is not None else (None, None, 0)
    call("lmod_gen_push_stop", ptr(tokens), ptr(done), ptr(hist), hist.shape[1], ptr(n_hist), ptr(n_prompt), ptr(n_gen),
         -1 if eos is None else int(eos), 0 if pad is None else int(pad), ptr(sf), ptr(so), ns, R)


# ------------------------------------------------------------------------------------------ constrained decoding
CONSTRAIN_MAX_V = 524288      # csrc/constrain.hip: the V-bit bitmap of a closed state, 64 KB of LDS (the penalty bitmap's limit)


def constraint_table(c, device):
    """A `generation.TokenConstraint` as the device tables the constrain kernels read - `seq_table`'s sibling: (edge_off [n + 1],
    edge_tok [E], edge_next [E], default_next [n], flags [n], n, has_closed), the arrays int32 views of one buffer, n and has_closed
    host values.  One host -> device copy."""
    n, E = c.n_states, len(c.edge_tok)
    both = torch.tensor(c.edge_off + c.edge_tok + c.edge_next + c.default_next + c.flags, dtype=torch.int32).to(device)
    cut = [0, n + 1, n + 1 + E, n + 1 + 2 * E, 2 * n + 1 + 2 * E, 3 * n + 1 + 2 * E]
    return tuple(both[a:b] for a, b in zip(cut, cut[1:])) + (n, c.has_closed)


def _constraint_args(table, state, R):
    off, tok, nxt, dflt, flags, n, _ = table
    for t in (off, tok, nxt, dflt, flags, state):
        assert t.dtype == torch.int32 and t.is_cuda and t.is_contiguous()
    assert off.numel() == n + 1 and dflt.numel() == n and flags.numel() == n and tok.numel() == nxt.numel() and state.numel() == R
    return ptr(off), ptr(tok) if tok.numel() else None, ptr(nxt) if nxt.numel() else None, ptr(dflt), ptr(flags), n


def constrain_mask_(logits, state, table, eos=None):
    """In place on logits [R, V] bf16 (row stride may exceed V): every row whose state [R] (device int32) is inside the automaton
    `table` (`constraint_table`) keeps only what that state allows, everything else becomes -inf; a row with state -1 is not
    touched (lmod_constrain_mask_rows_bf16 in include/lmod_hip.h).  Runs after every other processor.  ValueError, and no launch,
    when the automaton has a closed state and V exceeds the LDS bitmap.  Returns logits."""
    R, V = logits.shape
    assert logits.dtype == BF16 and logits.is_cuda and logits.stride(1) == 1
    args = _constraint_args(table, state, R)
    if table[6] and V > CONSTRAIN_MAX_V:
        raise ValueError(f"a closed constraint state needs a {V}-bit bitmap in LDS: a vocabulary above {CONSTRAIN_MAX_V} is not supported")
    call("lmod_constrain_mask_rows_bf16", ptr(logits), logits.stride(0), V, R, ptr(state), *args, -1 if eos is None else int(eos))
    return logits


def constrain_advance_(tokens, done, state, table):
    """One generation step's automaton bookkeeping on the device (lmod_constrain_advance_rows), after `gen_push_stop_`: a live row
    in a valid state follows its token's edge; done[r] is set when the row enters a terminal state or its token left the automaton.
    tokens / done / state: device int32 [R], done and state updated in place."""
    R = tokens.numel()
    for t in (tokens, done):
        assert t.dtype == torch.int32 and t.is_cuda and t.is_contiguous() and t.numel() == R
    call("lmod_constrain_advance_rows", ptr(tokens), ptr(done), ptr(state), *_constraint_args(table, state, R), R)


def constrain_draft(pending, state, done, table, k, eos, V, out=None):
    """The run of tokens the automaton forces on every row (lmod_constrain_draft in include/lmod_hip.h).  pending / state / done [R]:
    device int32, the row's pending token and the state after it.  Returns (draft [R, k]: the run then -1, chunk [R, k+1]: pending,
    the run, pending again, vstate [R, k+1]: the state that masks each verification row, -1 behind the run, n_draft [R]); out: the
    four tensors to reuse.  k outside 1..APPEND_T_MAX-1 raises (LMOD_EINVAL)."""
    R = pending.numel()
    for t in (pending, done):
        assert t.dtype == torch.int32 and t.is_cuda and t.is_contiguous() and t.numel() == R
    args = _constraint_args(table, state, R)
    k = int(k)
    if out is None:
        out = (torch.empty((R, max(k, 0)), device=pending.device, dtype=torch.int32),
               torch.empty((R, max(k, 0) + 1), device=pending.device, dtype=torch.int32),
               torch.empty((R, max(k, 0) + 1), device=pending.device, dtype=torch.int32),
               torch.empty(R, device=pending.device, dtype=torch.int32))
    draft, chunk, vstate, n_draft = out
    assert all(t.dtype == torch.int32 and t.is_cuda and t.is_contiguous() for t in out)
    assert (k < 1 or (tuple(draft.shape) == (R, k) and tuple(chunk.shape) == (R, k + 1) and tuple(vstate.shape) == (R, k + 1)))
    assert n_draft.numel() == R
    call("lmod_constrain_draft", ptr(pending), ptr(state), ptr(done), *args, -1 if eos is None else int(eos), int(V), k, ptr(draft),
         ptr(chunk), ptr(vstate), ptr(n_draft), R)
    return draft, chunk, vstate, n_draft


def constrain_accept(draft, target, done, state, table, eos, pad, n_gen, budget, lens_target):
    """One constrained draft-and-verify round's acceptance on the device (lmod_constrain_accept): `spec_accept`'s rule and block with
    every emitted token followed through the automaton and cut at EOS, a token that leaves the automaton, a terminal state or
    `budget` tokens.  draft [R, k], target [R, k+1], done / state / n_gen / lens_target [R]: device int32, contiguous; the last four
    are updated in place.  Returns (block [R, k+5] int32: emitted tokens | n_acc | n_emitted | next_token | done, next_token [R])."""
    R, k = draft.shape
    for t in (draft, target, done, n_gen, lens_target):
        assert t.dtype == torch.int32 and t.is_cuda and t.is_contiguous()
    assert tuple(target.shape) == (R, k + 1) and done.numel() == R and n_gen.numel() == R and lens_target.numel() == R
    out = torch.empty((R, k + 5), device=draft.device, dtype=torch.int32)
    nxt = torch.empty(R, device=draft.device, dtype=torch.int32)
    call("lmod_constrain_accept", ptr(draft), ptr(target), k, ptr(done), ptr(state), *_constraint_args(table, state, R),
         -1 if eos is None else int(eos), 0 if pad is None else int(pad), ptr(n_gen), int(budget), ptr(lens_target), ptr(out), ptr(nxt), R)
    return out, nxt


# ------------------------------------------------------------------------------------------ prompt-lookup decoding
NGRAM_MAX = 8              # csrc/lookup.hip: the longest trailing n-gram lmod_ngram_draft looks up


def ngram_draft(hist, n_hist, done, k, max_ngram, V, out=None):
    """The prompt-lookup draft of every row from its own history (lmod_ngram_draft in include/lmod_hip.h).  hist [R, L] / n_hist [R] /
    done [R]: device int32, the history already ending with the row's pending token.  Returns (draft [R, k]: the draft then -1,
    chunk [R, k+1]: pending token, draft, pending token again, n_draft [R]); out: the three tensors to reuse.  k outside
    1..APPEND_T_MAX-1 or max_ngram outside 1..NGRAM_MAX raises (LMOD_EINVAL)."""
    R = hist.shape[0]
    for t in (hist, n_hist, done):
        assert t.dtype == torch.int32 and t.is_cuda and t.is_contiguous()
    assert hist.dim() == 2 and n_hist.numel() == R and done.numel() == R
    k = int(k)
    if out is None:
        out = (torch.empty((R, max(k, 0)), device=hist.device, dtype=torch.int32),
               torch.empty((R, max(k, 0) + 1), device=hist.device, dtype=torch.int32),
               torch.empty(R, device=hist.device, dtype=torch.int32))
    draft, chunk, n_draft = out
    assert all(t.dtype == torch.int32 and t.is_cuda and t.is_contiguous() for t in out)
    assert (k < 1 or (tuple(draft.shape) == (R, k) and tuple(chunk.shape) == (R, k + 1))) and n_draft.numel() == R
    call("lmod_ngram_draft", ptr(hist), hist.shape[1], ptr(n_hist), ptr(done), R, k, int(max_ngram), int(V), ptr(draft), ptr(chunk),
         ptr(n_draft))
    return draft, chunk, n_draft


def hist_push_block_(block, k, hist, n_hist):
    """Append every row's emitted tokens of one assisted round (block [R, k+5] int32, `spec_accept`'s layout) to its history, in
    place (lmod_hist_push_block): hist [R, L] and n_hist [R] device int32; a row that would overflow L is left as it is."""
    R = hist.shape[0]
    for t in (block, hist, n_hist):
        assert t.dtype == torch.int32 and t.is_cuda and t.is_contiguous()
    assert hist.dim() == 2 and tuple(block.shape) == (R, int(k) + 5) and n_hist.numel() == R
    call("lmod_hist_push_block", ptr(block), int(k), ptr(hist), hist.shape[1], ptr(n_hist), R)


# ------------------------------------------------------------------------------------------ continuous batching
def _distinct_slots(dst_row, B):
    """dst_row: a host list of slot numbers — the kernels trust it, so it is checked here."""
    rows = [int(r) for r in dst_row]
    if any(not 0 <= r < B for r in rows) or len(set(rows)) != len(rows):
        raise ValueError(f"slots must be pairwise distinct and in [0, {B}), got {rows}")
    return rows


def kv_admit_rows(dst, src, dst_row, lens, max_len, tables=None):
    """dst[t][dst_row[r], :lens[r]] = src[t][r, :lens[r]] for every tensor pair (lists of contiguous bf16 caches, dst [B, smax_dst,
    width], src [R, smax_src, width]), one launch; everything else in dst stays as it is.  dst_row: a host list of R distinct slots
    in [0, B) (checked here, trusted by the device); lens [R] device int32; max_len: host upper bound of lens — beyond either smax
    this raises (LMOD_EINVAL) instead of clamping.  tables: (ptr_table(dst), ptr_table(src)) when the caller keeps them."""
    assert len(dst) == len(src) and len(dst) > 0
    d0, s0 = dst[0], src[0]
    for d, s in zip(dst, src):
        assert d.dtype == BF16 and s.dtype == BF16 and d.is_contiguous() and s.is_contiguous()
        assert d.shape == d0.shape and s.shape == s0.shape and s.dim() == 3 and d.dim() == 3 and s.shape[2] == d.shape[2]
    R, B = s0.shape[0], d0.shape[0]
    rows = _distinct_slots(dst_row, B)
    assert len(rows) == R and lens.dtype == torch.int32 and lens.numel() == R
    if R == 0:
        return
    dt, st = tables if tables is not None else (ptr_table(dst), ptr_table(src))
    call("lmod_kv_admit_rows", ptr(dt), ptr(st), len(dst), ptr(torch.tensor(rows, dtype=torch.int32).to(d0.device)),
         ptr(lens.contiguous()), R, B, d0.shape[1], s0.shape[1], d0.shape[2], int(max_len))


def slot_admit_(dst_row, prompt_ids, n_prompt_new, lens_new, req_new, hist, n_prompt, n_hist, n_gen, done, cache_lens, req_id):
    """Re-arm the generation state of the slots dst_row (a host list of R distinct slots in [0, B)), in place, one launch
    (lmod_slot_admit): hist[s, :n] = prompt_ids[r, :n] with n = n_prompt_new[r], n_prompt[s] = n_hist[s] = n, n_gen[s] = done[s] = 0,
    cache_lens[s] = lens_new[r], req_id[s] = req_new[r].  Everything int32 on the device; prompt_ids [R, >= max n]."""
    B, R = hist.shape[0], prompt_ids.shape[0]
    rows = _distinct_slots(dst_row, B)
    for t in (prompt_ids, n_prompt_new, lens_new, req_new, hist, n_prompt, n_hist, n_gen, done, cache_lens, req_id):
        assert t.dtype == torch.int32 and t.is_cuda and t.is_contiguous()
    assert len(rows) == R and all(t.numel() == R for t in (n_prompt_new, lens_new, req_new))
    assert all(t.numel() == B for t in (n_prompt, n_hist, n_gen, done, cache_lens, req_id))
    call("lmod_slot_admit", ptr(torch.tensor(rows, dtype=torch.int32).to(hist.device)), ptr(prompt_ids), prompt_ids.shape[1],
         ptr(n_prompt_new), ptr(lens_new), ptr(req_new), R, B, ptr(hist), hist.shape[1], ptr(n_prompt), ptr(n_hist), ptr(n_gen),
         ptr(done), ptr(cache_lens), ptr(req_id))


def _batch_lookup_state(done, hist, n_hist, n_prompt, n_gen, budget):
    B = hist.shape[0]
    for t in (done, hist, n_hist, n_prompt, n_gen, budget):
        assert t.dtype == torch.int32 and t.is_cuda and t.is_contiguous()
    assert hist.dim() == 2 and all(t.numel() == B for t in (done, n_hist, n_prompt, n_gen, budget))
    return B


def batch_lookup_first_(tokens, done, hist, n_hist, n_prompt, n_gen, budget, eos, stop=None, out=None):
    """The first token of the freshly admitted slots of `generate_batch(prompt_lookup_num_tokens=k)` (lmod_batch_lookup_first in
    include/lmod_hip.h), the slot state updated in place: a slot with done == 0 and n_gen == 0 appends tokens[s] (the argmax of its
    logits row) to its history as the pending token, n_gen = 1, and is done when the token is eos, completes a stop sequence (`stop`:
    a `seq_table` or None) or budget[s] is 1.  Returns first_tok [B] int32: that token, -1 for every other slot (`out` to reuse)."""
    B = _batch_lookup_state(done, hist, n_hist, n_prompt, n_gen, budget)
    first = torch.empty(B, device=hist.device, dtype=torch.int32) if out is None else out
    for t in (tokens, first):
        assert t.dtype == torch.int32 and t.is_cuda and t.is_contiguous() and t.numel() == B
    sf, so, ns = stop if stop is not None else (None, None, 0)
    call("lmod_batch_lookup_first", ptr(tokens), ptr(done), ptr(hist), hist.shape[1], ptr(n_hist), ptr(n_prompt), ptr(n_gen),
         ptr(budget), -1 if eos is None else int(eos), ptr(sf), ptr(so), ns, ptr(first), B)
    return first


def batch_lookup_round_(draft, target, first_tok, done, hist, n_hist, n_prompt, n_gen, budget, cache_lens, eos, pad, stop=None,
                        out=None):
    """One round's acceptance, emission and end conditions for every slot (lmod_batch_lookup_round), the slot state and cache_lens
    updated in place.  draft [B, k] (`ngram_draft`'s), target [B, k+1] (argmax of the verification rows), first_tok [B]
    (`batch_lookup_first_`'s), cache_lens [B] as the verification pass left them.  Returns block [B, k+6] int32: columns 0..k the
    emitted tokens then pad, k+1 n_acc, k+2 n_emit, k+3 the next pending token, k+4 fin, k+5 first_tok (`out` to reuse).  k outside
    1..APPEND_T_MAX-1 raises (LMOD_EINVAL)."""
    B = _batch_lookup_state(done, hist, n_hist, n_prompt, n_gen, budget)
    k = int(draft.shape[1])
    block = torch.empty((B, k + 6), device=hist.device, dtype=torch.int32) if out is None else out
    for t in (draft, target, first_tok, cache_lens, block):
        assert t.dtype == torch.int32 and t.is_cuda and t.is_contiguous()
    assert tuple(draft.shape) == (B, k) and target.numel() == B * (k + 1) and tuple(block.shape) == (B, k + 6)
    assert first_tok.numel() == B and cache_lens.numel() == B
    sf, so, ns = stop if stop is not None else (None, None, 0)
    call("lmod_batch_lookup_round", ptr(draft), ptr(target), ptr(first_tok), k, ptr(done), ptr(hist), hist.shape[1], ptr(n_hist),
         ptr(n_prompt), ptr(n_gen), ptr(budget), ptr(cache_lens), -1 if eos is None else int(eos), 0 if pad is None else int(pad),
         ptr(sf), ptr(so), ns, ptr(block), B)
    return block


def request_uniform(seed, req_id, n_gen, out=None):
    """u [B] fp32 in [0, 1): Philox4x32-10 at counter (req_id[s], n_gen[s], 0, 0) under the 64-bit key `seed` — one uniform per
    slot that depends on the request and its token index only (lmod_request_uniform)."""
    B = req_id.numel()
    for t in (req_id, n_gen):
        assert t.dtype == torch.int32 and t.is_cuda and t.is_contiguous() and t.numel() == B
    u = torch.empty(B, device=req_id.device, dtype=torch.float32) if out is None else out
    assert u.dtype == torch.float32 and u.is_contiguous() and u.numel() == B
    call("lmod_request_uniform", int(seed) & 0xFFFFFFFFFFFFFFFF, ptr(req_id), ptr(n_gen), ptr(u), B)
    return u


def request_uniform_rows(seed, ctr0, n_gen, out=None):
    """u [B] fp32 in [0, 1): Philox4x32-10 at counter (ctr0[s], n_gen[s], 0, 0) under the 64-bit key seed[s] (device int64 [B], the
    key's bit pattern; ctr0 / n_gen device int32 [B]) — `request_uniform` with the key and the first counter word per slot
    (lmod_request_uniform_rows)."""
    B = ctr0.numel()
    for t in (ctr0, n_gen):
        assert t.dtype == torch.int32 and t.is_cuda and t.is_contiguous() and t.numel() == B
    assert seed.dtype == torch.int64 and seed.is_cuda and seed.is_contiguous() and seed.numel() == B
    u = torch.empty(B, device=ctr0.device, dtype=torch.float32) if out is None else out
    assert u.dtype == torch.float32 and u.is_contiguous() and u.numel() == B
    call("lmod_request_uniform_rows", ptr(seed), ptr(ctr0), ptr(n_gen), ptr(u), B)
    return u


# ------------------------------------------------------------------------------------------ MoE
def moe_router_fwd(x, wg):
    T, H = x.shape
    E = wg.shape[0]
    logits = torch.empty((T, E), device=x.device, dtype=torch.float32)
    call("lmod_moe_router_fwd", ptr(x), ptr(wg), ptr(logits), T, H, E)
    return logits


class GateState:
    """Index maps produced by lmod_moe_gate (all device tensors)."""
    __slots__ = ("T", "E", "k", "C", "gates", "idx1", "idx2", "slot1", "slot2", "w1", "w2", "slot_token", "slot_w",
                 "exp_counts", "gate_sum", "l_aux", "slots_used", "noise")


def moe_gate(logits, k, C, noise=None, seed=None, offset=0, want_noise=False):
    """noise: explicit [T,E] noise (k=2: added for the 2nd pick; k=1: random-token-selection priorities).  seed (with noise
    None): the kernel draws it (Gumbel for k=2, uniform for k=1) from Philox(seed, offset + token); want_noise returns it as
    st.noise."""
    T, E = logits.shape
    dev = logits.device
    st = GateState()
    st.T, st.E, st.k, st.C = T, E, k, C
    st.gates = torch.empty((T, E), device=dev, dtype=torch.float32)
    i32 = dict(device=dev, dtype=torch.int32)
    f32 = dict(device=dev, dtype=torch.float32)
    st.idx1 = torch.empty(T, **i32); st.slot1 = torch.empty(T, **i32); st.w1 = torch.empty(T, **f32)
    if k == 2:
        st.idx2 = torch.empty(T, **i32); st.slot2 = torch.empty(T, **i32); st.w2 = torch.empty(T, **f32)
    else:
        st.idx2 = st.slot2 = st.w2 = None
    st.slot_token = torch.empty(E * C, **i32); st.slot_w = torch.empty(E * C, **f32)
    st.exp_counts = torch.empty(E, **i32); st.gate_sum = torch.empty(E, **f32); st.l_aux = torch.empty(1, **f32)
    st.slots_used = torch.empty(E, **i32)
    me = 8 if E <= 8 else (16 if E <= 16 else 32)          # expert slots of the routing kernels' instantiation (csrc/moe.hip)
    scratch = torch.empty(4 * T + 3 * me * ((T + 511) // 512), **i32)
    mode = 0 if (noise is not None or seed is None) else (1 if k == 2 else 2)
    st.noise = torch.empty((T, E), **f32) if (mode and want_noise) else None
    call("lmod_moe_gate", ptr(logits), ptr(noise), T, E, k, C, ptr(st.gates), ptr(st.idx1), ptr(st.idx2),
         ptr(st.slot1), ptr(st.slot2), ptr(st.w1), ptr(st.w2), ptr(st.slot_token), ptr(st.slot_w),
         ptr(st.exp_counts), ptr(st.gate_sum), ptr(st.l_aux), ptr(st.slots_used), ptr(scratch), mode,
         int(seed or 0) & 0xFFFFFFFFFFFFFFFF, int(offset) & 0xFFFFFFFFFFFFFFFF, ptr(st.noise))
    return st


def moe_combine_fwd(y, st, H):
    out = torch.empty((st.T, H), device=y.device, dtype=BF16)
    call("lmod_moe_combine_fwd", ptr(y), ptr(st.slot1), ptr(st.slot2), ptr(st.w1), ptr(st.w2), ptr(out), st.T, H)
    return out


def moe_combine_bwd(dout, y, st, H):
    S = st.E * st.C
    dy = torch.empty((S, H), device=y.device, dtype=BF16)
    dw1 = torch.empty(st.T, device=y.device, dtype=torch.float32)
    dw2 = torch.empty(st.T, device=y.device, dtype=torch.float32) if st.k == 2 else None
    call("lmod_moe_combine_bwd", ptr(dout), ptr(y), ptr(st.slot1), ptr(st.slot2), ptr(st.slot_token), ptr(st.slot_w),
         ptr(dy), ptr(dw1), ptr(dw2), st.T, S, H)
    return dy, dw1, dw2


def moe_gate_bwd(st, dw1, dw2, d_laux):
    dlogits = torch.empty((st.T, st.E), device=dw1.device, dtype=torch.float32)
    call("lmod_moe_gate_bwd", ptr(st.gates), ptr(st.idx1), ptr(st.idx2), ptr(st.slot1), ptr(st.slot2), ptr(dw1),
         ptr(dw2), ptr(st.exp_counts), ptr(d_laux), ptr(dlogits), st.T, st.E, st.k)
    return dlogits


def moe_dispatch_bwd(d_in, st, dlogits, wg, H):
    dx = torch.empty((st.T, H), device=d_in.device, dtype=BF16)
    call("lmod_moe_dispatch_bwd", ptr(d_in), ptr(st.slot1), ptr(st.slot2), ptr(dlogits), ptr(wg), ptr(dx), st.T, H,
         st.E)
    return dx


def moe_router_wgrad(x, dlogits, dwg, accumulate):
    T, H = x.shape
    E = dlogits.shape[1]
    ws = torch.empty(((T + 63) // 64) * E * H, device=x.device, dtype=torch.float32)      # one partial per 64-token slab
    call("lmod_moe_router_wgrad", ptr(x), ptr(dlogits), ptr(dwg), ptr(ws), T, H, E, int(accumulate))
    return dwg


def residual_mix_fwd(moe_out, mlp_out, coef_logits, coef_bias):
    T, H = moe_out.shape
    out = torch.empty_like(moe_out)
    p = torch.empty((T, 2), device=moe_out.device, dtype=torch.float32)
    call("lmod_moe_residual_mix_fwd", ptr(moe_out), ptr(mlp_out), ptr(coef_logits), ptr(coef_bias), ptr(out), ptr(p), T, H)
    return out, p


def residual_mix_bwd(dout, moe_out, mlp_out, p):
    T, H = moe_out.shape
    d_moe, d_mlp = torch.empty_like(moe_out), torch.empty_like(moe_out)
    dc = torch.empty((T, 2), device=moe_out.device, dtype=torch.float32)
    call("lmod_moe_residual_mix_bwd", ptr(dout), ptr(moe_out), ptr(mlp_out), ptr(p), ptr(d_moe), ptr(d_mlp), ptr(dc), T, H)
    return d_moe, d_mlp, dc


def small_linear_dgrad(dlogits, w):
    T, E = dlogits.shape
    H = w.shape[1]
    dx = torch.empty((T, H), device=dlogits.device, dtype=BF16)
    call("lmod_small_linear_dgrad", ptr(dlogits), ptr(w), ptr(dx), T, H, E)
    return dx


# ------------------------------------------------------------------------------------------ losses
NSTAT = 8


def rowloss_fwd(s, Vs, t=None, Va=None, label=None):
    R = s.shape[0]
    stats = torch.empty((R, NSTAT), device=s.device, dtype=torch.float32)
    if Va is None:
        Va = Vs
    call("lmod_rowloss_fwd", ptr(s), s.stride(0), Vs, ptr(t), t.stride(0) if t is not None else 0, Va, ptr(label),
         ptr(stats), R)
    return stats


def rowloss_bwd(s, Vs, t, Va, label, stats, kd_w, ce_w, seg_id, kd_scale, ce_scale, ds=None):
    R = s.shape[0]
    if ds is None:
        ds = s                      # in place over the student logits
    call("lmod_rowloss_bwd", ptr(s), s.stride(0), Vs, ptr(t), t.stride(0) if t is not None else 0, Va, ptr(label),
         ptr(stats), ptr(kd_w), ptr(ce_w), ptr(seg_id), ptr(kd_scale), ptr(ce_scale), ptr(ds), ds.stride(0), R)
    return ds


def segment_wsum(stats, col, w, seg_off):
    nseg = seg_off.numel() - 1
    out = torch.empty(nseg, device=stats.device, dtype=torch.float32)
    outw = torch.empty(nseg, device=stats.device, dtype=torch.float32)
    call("lmod_segment_wsum", ptr(stats), stats.stride(0), col, ptr(w), ptr(seg_off), nseg, ptr(out), ptr(outw))
    return out, outw


LOSS_TYPES = {"sigmoid": 0, "hinge": 1, "ipo": 2, "kto_pair": 3}


def dpo_loss(pc, pr, rc, rr, beta, label_smoothing, loss_type):
    B = pc.numel()
    lt = LOSS_TYPES[loss_type]
    dev = pc.device
    losses = torch.empty(2 * B if lt == 3 else B, device=dev, dtype=torch.float32)
    cr = torch.empty(B, device=dev, dtype=torch.float32)
    rj = torch.empty(B, device=dev, dtype=torch.float32)
    dpc = torch.empty(B, device=dev, dtype=torch.float32)
    dpr = torch.empty(B, device=dev, dtype=torch.float32)
    call("lmod_dpo_loss", ptr(pc), ptr(pr), ptr(rc), ptr(rr), B, float(beta), float(label_smoothing), lt, ptr(losses),
         ptr(cr), ptr(rj), ptr(dpc), ptr(dpr))
    return losses, cr, rj, dpc, dpr


def row_softmax_f32(logits_f32, Va, log):
    """[R, V] fp32 -> fp32 softmax / log_softmax over the first Va columns (materialising API parity)."""
    R = logits_f32.shape[0]
    out = torch.empty((R, Va), device=logits_f32.device, dtype=torch.float32)
    call("lmod_row_softmax_f32", ptr(logits_f32), logits_f32.stride(0), Va, int(log), ptr(out), R)
    return out


def rowdot_masked(p, logp):
    R, V = p.shape
    x = torch.empty(R, device=p.device, dtype=torch.float32)
    call("lmod_rowdot_masked", ptr(p), ptr(logp), V, R, ptr(x))
    return x
