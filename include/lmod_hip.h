/* lmod_hip.h — C ABI of the MI355X (gfx950) kernels behind the LLaVA-MoD distillation step.
 *
 * The reference (shufangxun/LLaVA-MoD) is pure Python and has NO native interface of its own:
 * every op below is what the reference reaches through torch / HF transformers / DeepSpeed at the
 * cited call site.  This header is therefore the boundary a maintainer binds with ctypes
 * (see INTEGRATION.md); nothing in it carries a torch type.
 *
 * Conventions: raw device pointers, explicit dims / leading dimensions (in ELEMENTS), the HIP
 * stream to enqueue on, caller-owned outputs and workspaces.  Every function only enqueues work
 * (no allocation, no synchronisation) and returns 0 on success or a negative LMOD_E* code; it
 * never throws.  bf16 tensors are `void*` to raw uint16 bit patterns.
 *
 * State.  No entry point keeps data between calls: every buffer, workspace and counter is the caller's.  What the library
 * does keep, process-wide, is launch CONFIGURATION, all of it idempotent and safe under concurrent first use:
 *   - per kernel instance, a flag "dynamic-LDS attribute already set" (hipFuncSetAttribute is issued once);
 *   - the compute-unit count per device id (the persistent GEMM grid is one workgroup per CU of the CURRENT device);
 *   - the communicator handles behind lmod_comm_* (owned by the caller through their opaque pointers);
 *   - measurement switches from the environment, documented beside their readers in csrc/ — read once at first use:
 *     LMOD_GEMM_WAVES, LMOD_ATTN_FWD, LMOD_ATTN_BWD, LMOD_ATTN_BWD64, LMOD_ATTN_BWD_SPLIT, LMOD_ATTN_XCD, LMOD_WGRAD_SPLIT; read at every launch (so that one test process can
 *     run both arms of an A/B): LMOD_GEMM_PERSIST, LMOD_GEMM_PERSIST_GROUPED, LMOD_GEMM_PERSIST_ROUNDS, LMOD_GEMM_KV4, LMOD_GEMM_SB4, LMOD_GEMM_TN4, LMOD_GEMM_TILE.
 *     Unset, they select the shipped routing.  The GEMM switches' arms are bit-identical; the attention switches choose between kernels
 *     that pass the same tests against the fp32 reference but round differently (tests/test_kernels_gpu.py).
 */
#ifndef LMOD_HIP_H
#define LMOD_HIP_H
#include <hip/hip_runtime_api.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LMOD_OK 0
#define LMOD_EINVAL (-1)       /* bad pointer / shape / alignment */
#define LMOD_ELAUNCH (-2)      /* HIP reported a launch error */
#define LMOD_EUNSUPPORTED (-3) /* valid request outside the compiled envelope */

/* ---- GEMM ------------------------------------------------------------------------------------
 * C[b] (+)= act(A[b] (M x K, row-major, lda) * B[b]^T (N x K, row-major, ldb) + bias[N]).
 * Replaces nn.Linear forward: qwen2/modeling_qwen2.py:262-264,320 (QKV/O), :186-187 (SwiGLU MLP),
 * :1163 (lm_head); multimodal_projector/builder.py:57-61; HF CLIP linears + patch conv
 * (multimodal_encoder/clip_encoder.py:54).  With m_valid/k_valid (device int[batch]) it is the
 * grouped GEMM over DeepSpeed MoE capacity slabs (deepspeed.moe.experts; llava_qwen2_moe.py:536-546).
 * act: 0 none, 1 exact GELU, 2 quick_gelu.  out_f32: C is fp32.  accumulate: C += .
 * Requires K % 8 == 0, lda/ldb % 8 == 0, A/B 16-byte aligned. */
int lmod_gemm_bf16_nt(const void* A, const void* B, void* C, const void* bias, int M, int N, int K, int lda, int ldb,
                      int ldc, int batch, long long strideA, long long strideB, long long strideC, const int* m_valid,
                      const int* k_valid, int act, int out_f32, int accumulate, hipStream_t stream);

/* C[M x N] = bf16(res + bf16(A W^T)): a bias-free projection whose output joins the residual stream — the decoder layer's
 * hidden_states = residual + self_attn(...) / residual + mlp(...) (qwen2/modeling_qwen2.py:757-775; MoE layer:
 * llava_qwen2_moe.py:143-167) with the add in the GEMM epilogue.  Same roundings as lmod_gemm_bf16_nt followed by the residual
 * path of lmod_rmsnorm_fwd (bit-identical); the norm that follows then reads one tensor and writes one.  Only shapes that
 * lmod_gemm_bf16_nt runs on the 4-wave 256-tile kernel (M >= 512, N >= 256, enough tiles): others return LMOD_EUNSUPPORTED and the
 * caller keeps the two-step form.  N % 8 == 0, ldc / ldr % 8 == 0, 16-byte aligned pointers, C != res, bias must be NULL. */
int lmod_gemm_bf16_nt_res(const void* A, const void* W, void* C, const void* bias, const void* res, int M, int N, int K, int lda,
                          int ldw, int ldc, int ldr, hipStream_t stream);

/* Fused q/k/v projection + rotary embedding: C[M x N] = rope(A W^T + bias), W = [Wq; Wk; Wv] stored as ONE [N x K] matrix.
 * Replaces `self.q_proj / k_proj / v_proj` followed by `apply_rotary_pos_emb` (qwen2/modeling_qwen2.py:262-264, :146-171;
 * tables :119-134) in ONE launch: heads are 128 wide, columns [0, rope_cols) hold the q and k heads and are rotated in the GEMM
 * epilogue with the bf16 cos/sin rows [max_pos x 128] of position pos[row] (int32 [M]); columns >= rope_cols (v) are stored
 * as computed.  Results are bit-identical to lmod_gemm_bf16_nt + lmod_rope.
 * Requires K % 8 == 0, N % 16 == 0, rope_cols % 256 == 0, lda/ldw/ldc % 8 == 0, A/W/C 16-byte aligned. */
int lmod_gemm_qkv_rope_bf16(const void* A, const void* W, void* C, const void* bias, int M, int N, int K, int lda, int ldw,
                            int ldc, const void* cos_t, const void* sin_t, const int* pos, int rope_cols, hipStream_t stream);

/* Fused SwiGLU MLP input half: act_out[b] (M x N) = silu(A Wg^T) * (A Wu^T), W = [Wg; Wu] stored as ONE [2N x K]
 * matrix (gate rows first — the fused gate_proj/up_proj weight; qwen2/modeling_qwen2.py:175-187, MoE experts
 * llava_qwen2_moe.py:536-546).  gu_out (may be NULL): [M x 2N] bf16 pre-activations [gate | up] kept for backward.
 * m_valid as in lmod_gemm_bf16_nt; rows m_valid..roundup8(m_valid)-1 of act_out are written as zeros.
 * Requires K % 8 == 0, N % 8 == 0, 16-byte aligned pointers, leading dims % 8 == 0. */
int lmod_gemm_swiglu_bf16(const void* A, const void* W, void* act_out, void* gu_out, int M, int N, int K, int lda,
                          int ldw, int ld_act, int ld_gu, int batch, long long strideA, long long strideW,
                          long long stride_act, long long stride_gu, const int* m_valid, hipStream_t stream);

/* Down-projection dgrad with the SwiGLU backward in its epilogue: dact = A (M x K) * Bt^T (Bt = W_down^T, N x K), then
 * dgu = [dact * up * silu'(gate) | dact * silu(gate)] (M x 2N) from the saved pre-activations gu = [gate | up];
 * d(act) is never written (autograd of `down_proj(act_fn(gate_proj(x)) * up_proj(x))`, qwen2/modeling_qwen2.py:186-187).
 * dgu may alias gu.  Grouped use as lmod_gemm_bf16_nt; rows m_valid..roundup8(m_valid)-1 of dgu are zeroed.
 * Requires K % 8 == 0, N % 16 == 0, 16-byte aligned pointers, leading dims % 8 == 0. */
int lmod_gemm_swiglu_bwd_bf16(const void* A, const void* Bt, const void* gu, void* dgu, int M, int N, int K, int lda,
                              int ldb, int ld_gu, int ld_dgu, int batch, long long strideA, long long strideB,
                              long long stride_gu, long long stride_dgu, const int* m_valid, hipStream_t stream);

/* Weight-gradient accumulate: C (fp32, M x N) += At (M x K) * X, K = tokens (main_grad accumulation of nn.Linear
 * weights, dW = dY^T X; the reference gets this from autograd + DeepSpeed's fp32 gradient accumulation).
 * At = dY^T [M x K] (K-contiguous).  X: b_kmajor 0 -> Bt [N x K] (K-contiguous); b_kmajor 1 -> the layer input as
 * autograd holds it, [K x N] with row stride ldb (read through transposing LDS reads, no transposed copy).
 * b_kmajor 2 -> BOTH operands as autograd holds them: At is dY [K x M] (row stride lda), B is X [K x N]; no transposed
 * copy of either (the step's path: grad_output.t() @ input of nn.Linear's backward, reference linears as in
 * lmod_gemm_bf16_nt).  Mode 2 requires M % 8 == 0, N % 8 == 0, lda / ldb % 8 == 0, ldc % 4 == 0, 16-byte aligned
 * pointers; any K; operand windows past 2 GiB are walked in K chunks.
 * Few-tile outputs use deterministic split-K.  workspace: 16-byte aligned device memory, zeroed ONCE by the caller,
 * used by one stream at a time: 16 KiB of tile semaphores (self-resetting) + up to 8 partial images of 256 KiB per
 * 256x256 tile; its size bounds the split (NULL: no split).  The last split to arrive adds all partials in split
 * order, so the result does not depend on scheduling. */
int lmod_gemm_wgrad_bf16_nt(const void* At, const void* B, float* C, int M, int N, int K, int lda, int ldb, int ldc,
                            int b_kmajor, void* workspace, long long workspace_bytes, hipStream_t stream);

/* Weight-gradient GEMM: C[b] (M x N) (+)= A[b]^T * B[b], A [K x M] (lda), B [K x N] (ldb) — dW = dY^T X on the
 * token-major tensors autograd holds (the implicit grad_output.t() @ input of nn.Linear's backward; reference
 * linears as in lmod_gemm_bf16_nt).  k_valid (device int[batch]): live reduction rows per batch (MoE capacity slots).
 * Split-K: batch = S, strideA = Kc*lda, strideB = Kc*ldb, C = [S, M, N] workspace.
 * Requires M % 8 == 0, N % 8 == 0, lda/ldb % 8 == 0, ldc % 4 == 0, 16-byte aligned pointers. */
int lmod_gemm_bf16_tn(const void* A, const void* B, void* C, int M, int N, int K, int lda, int ldb, int ldc, int batch,
                      long long strideA, long long strideB, long long strideC, const int* k_valid, int out_f32,
                      int accumulate, hipStream_t stream);

/* out[C x ld_out] = in[R x C]^T, zero-filling columns R..ld_out-1 (makes dgrad / wgrad operands
 * K-contiguous for lmod_gemm_bf16_nt; autograd's implicit .t() in the reference).  r_valid (nullable, [batch]): live rows per batch entry (MoE capacity
 * slabs): rows past it are not transposed at all — the k_valid GEMM that consumes the result never reads them — except that
 * the 8-column group holding the boundary is zero-filled. */
int lmod_transpose_bf16(const void* in, void* out, int R, int C, int ld_in, int ld_out, int batch,
                        long long stride_in, long long stride_out, const int* r_valid, hipStream_t stream);

/* ---- row kernels -----------------------------------------------------------------------------
 * Qwen2RMSNorm (qwen2/modeling_qwen2.py:83-97) with the decoder layer's residual add fused
 * (:757-775, llava_qwen2_moe.py:143-167): h = res ? bf16(x+res) : x; y = w * bf16(h*rstd).
 * res, h_out, rstd may be NULL. */
int lmod_rmsnorm_fwd(const void* x, const void* res, const void* w, void* h_out, void* y, float* rstd, int T, int H,
                     float eps, hipStream_t stream);
/* dh = rmsnorm_bwd(dy; h, w, rstd) + dres (dres may be NULL).  Norm weights are frozen in every
 * stage of the reference (llava_qwen2_moe.py:501-506), so no dw. */
int lmod_rmsnorm_bwd(const void* dy, const void* h, const void* w, const float* rstd, const void* dres, void* dh,
                     int T, int H, hipStream_t stream);
/* nn.LayerNorm forward of the frozen CLIP tower (clip_encoder.py:45 runs under no_grad). */
/* Weight gradients of the row parameters (only when they are trainable; the distillation shells freeze them):
 * lmod_rmsnorm_dw: dw[H] (+)= sum_t dy[t,:] * bf16(h[t,:] * rstd[t])  (Qwen2RMSNorm.weight; deterministic; workspace 64*H floats);
 * lmod_embed_wgrad: dW[idx[r], :] += d_embeds[r, :] for idx[r] >= 0  (embed_tokens.weight through the splice map; fp32 atomics). */
int lmod_rmsnorm_dw(const void* dy, const void* h, const float* rstd, float* dw, float* workspace, int T, int H,
                    int accumulate, hipStream_t stream);
int lmod_embed_wgrad(const void* d_embeds, const int* idx, float* dW, long long rows, int H, hipStream_t stream);
int lmod_layernorm_fwd(const void* x, const void* w, const void* b, void* y, int T, int H, float eps,
                       hipStream_t stream);
/* apply_rotary_pos_emb (qwen2/modeling_qwen2.py:146-171), in place on the first `nheads` heads
 * of each row of buf[T x ld]; cos/sin: [max_pos x hd] bf16; pos: int32[T]; backward != 0 applies
 * the gradient map. */
int lmod_rope(void* buf, const void* cos_t, const void* sin_t, const int* pos, int T, int nheads, int hd, int ld,
              int backward, hipStream_t stream);
/* Qwen2MLP activation (qwen2/modeling_qwen2.py:186-187): out = bf16(silu(gate)) * up. */
/* seg_valid (device int[rows/seg_rows]) or NULL: rows r with r % seg_rows >= seg_valid[r / seg_rows] are not
 * read and are written as zeros (dead MoE capacity slots stay finite). */
int lmod_swiglu_fwd(const void* gate, const void* up, void* out, long long rows, int I, int ld_gate, int ld_up,
                    int ld_out, int seg_rows, const int* seg_valid, hipStream_t stream);
int lmod_swiglu_bwd(const void* dact, const void* gate, const void* up, void* dgate, void* dup, long long rows, int I,
                    int ld_dact, int ld_gate, int ld_up, int ld_dgate, int ld_dup, int seg_rows, const int* seg_valid,
                    hipStream_t stream);
/* nn.GELU() of the mlp2x_gelu projector (multimodal_projector/builder.py:57-61). */
int lmod_gelu_fwd(const void* x, void* y, long long n, hipStream_t stream);
int lmod_gelu_bwd(const void* dy, const void* x, void* dx, long long n, hipStream_t stream);
int lmod_add_bf16(const void* a, const void* b, void* out, long long n, hipStream_t stream);
/* out[r] = idx[r] >= 0 ? srcA[idx[r]] : idx[r] <= -2 ? srcB[-(idx[r]+2)] : 0.  Embedding lookup +
 * image-feature splice of prepare_inputs_labels_for_multimodal (llava_arch.py:236-318), the MoE
 * dispatch (einsum 'sec,sm->ecm' of deepspeed MOELayer.forward), and their backward gathers. */
int lmod_gather_rows(const void* srcA, const void* srcB, const int* idx, void* out, long long rows, int H,
                     hipStream_t stream);
/* CLIP patch embedding front end (HF CLIPVisionEmbeddings; call site clip_encoder.py:54). */
int lmod_im2col_patch(const void* pixels, void* out, int B, int image_size, int patch, int Kpad, hipStream_t stream);
int lmod_vit_embed(const void* patch_emb, const void* cls, const void* pos, void* out, int B, int n_patches, int D,
                   hipStream_t stream);
/* torch.optim.AdamW step (HF `adamw_torch`, config/args.py:78) on fp32 master weights with a bf16
 * working copy; grad is fp32, scaled by grad_scale first.  zero_grad != 0: the gradient is cleared in the same pass
 * (the optimizer's zero_grad(), without a separate memset of the gradient buffer).  dev_scale (nullable): one fp32 on
 * the device that multiplies grad_scale — the gradient-clipping coefficient of lmod_clip_coef, read without a host sync. */
int lmod_adamw_step(float* master, void* param_bf16, float* grad, float* m, float* v, long long n, float lr,
                    float beta1, float beta2, float eps, float weight_decay, int step, float grad_scale, int zero_grad,
                    const float* dev_scale, hipStream_t stream);
/* Global gradient-norm clipping (HF Trainer max_grad_norm = 1.0 under DeepSpeed `"gradient_clipping": "auto"`,
 * config/dpconfig/zero2_offload.json; torch.nn.utils.clip_grad_norm_ arithmetic).
 * lmod_sumsq_f32: out[0] (+)= sum(x[i]^2), deterministic (fixed reduction order); partials: >= 1024 floats of scratch.
 * lmod_clip_coef: coef[0] = min(1, max_norm / (sqrt(sumsq[0]) * norm_scale + 1e-6)); norm_out (nullable) gets the norm. */
int lmod_sumsq_f32(const float* x, long long n, float* partials, float* out, int accumulate, hipStream_t stream);
int lmod_clip_coef(const float* sumsq, float norm_scale, float max_norm, float* coef, float* norm_out, hipStream_t stream);
/* fp32 <-> bf16 (round to nearest even) over n elements: gradients are exchanged in bf16 like the reference's bf16
 * engine (DeepSpeed bf16 + ZeRO-2 reduce-scatters bf16 gradients). */
int lmod_cast_f32_bf16(const void* src, void* dst, long long n, int to_bf16, hipStream_t stream);

/* ---- attention -------------------------------------------------------------------------------
 * softmax(Q K^T * scale + mask) V with causal and right-padding masks, GQA (nh % nkv == 0).
 * Replaces F.scaled_dot_product_attention / flash_attn (qwen2/modeling_qwen2.py:700-708,535-581)
 * and CLIP encoder attention.  hd in {64, 128}.  lse: [B, nh, S] fp32 (may be NULL in fwd).
 * cu_seqlens (nullable, hd 128 only): UNPADDED layout — the samples' tokens are packed back to back, sample b occupies rows
 * cu_seqlens[b] .. cu_seqlens[b+1]-1 and S is the longest sample (lse / delta keep the [B, nh, S] layout). */
int lmod_attn_fwd(const void* Q, const void* K, const void* V, void* O, float* lse, const int* seqlens,
                  const int* cu_seqlens, int B, int S, int nh, int nkv, int hd, int ldq, int ldk, int ldv, int ldo, float scale,
                  int causal, hipStream_t stream);
int lmod_attn_bwd(const void* Q, const void* K, const void* V, const void* O, const void* dO, const float* lse,
                  float* delta_ws, void* dQ, void* dK, void* dV, const int* seqlens, const int* cu_seqlens, int B, int S, int nh, int nkv,
                  int hd, int ldq, int ldk, int ldv, int ldo, int lddo, int lddq, int lddk, int lddv, float scale,
                  int causal, hipStream_t stream);
/* lmod_attn_bwd with the gradient map of the rotary embedding (apply_rotary_pos_emb, qwen2/modeling_qwen2.py:146-171) applied to dQ and
 * dK in the backward kernels' epilogues, head dim 128 only: bit-identical to lmod_attn_bwd followed by lmod_rope(backward = 1) on the
 * q and k column blocks.  cos_t / sin_t: [max_pos x 128] bf16, pos: int32 per token row. */
int lmod_attn_bwd_rope(const void* Q, const void* K, const void* V, const void* O, const void* dO, const float* lse,
                       float* delta_ws, void* dQ, void* dK, void* dV, const int* seqlens, const int* cu_seqlens, int B, int S,
                       int nh, int nkv, int hd, int ldq, int ldk, int ldv, int ldo, int lddo, int lddq, int lddk, int lddv,
                       float scale, int causal, const void* cos_t, const void* sin_t, const int* pos, hipStream_t stream);
/* The same backward (cos_t / sin_t / pos all NULL: lmod_attn_bwd; all set: lmod_attn_bwd_rope) with an optional workspace for the
 * HEAD-SPLIT form of the dK/dV kernel.  That kernel's grid is KV heads x key blocks x batch; grouped-query models with few KV heads
 * (the reference's d2s student Qwen2-0.5B, scripts/.../dense2sparse_distillation.sh:21: 14 heads over 2 KV heads) leave half of the
 * CUs without a workgroup.  lmod_attn_bwd_nsplit (host-side, no stream, no device work) returns into how many parts n every group
 * of query heads is cut for these shapes (1: no split); with split_ws_bytes >= n * 2 * B * S * nkv * hd * 4 (16-byte aligned) each
 * part runs as its own workgroup, stores fp32 partial sums into split_ws and a reduction kernel adds them in part order
 * (deterministic).  Without the workspace (NULL / too small), with fused RoPE or with cu_seqlens this is the unsplit launch.
 * The same workspace serves the dS-SPILL form (round 6) when the launch is not head-split: hd 128, no cu_seqlens, S % 256 == 0 and
 * split_ws_bytes >= B * nh * S * S * 2 (16-byte aligned) — the dK/dV kernel then also stores dS^T (bf16, [B * nh][S keys][S queries],
 * exactly the values its dK products consume) and dQ = scale * dS K (+ the fused RoPE gradient map) is ONE batched TN GEMM on the
 * weight-gradient kernel's K loop; the dQ kernel, which recomputes S, dP and the exponentials, is not launched (5 matmuls
 * instead of 7; the autograd of qwen2/modeling_qwen2.py:700-708).  Deterministic; dK / dV are bit-identical to the two-kernel form,
 * dQ differs by fp32 summation order only.  LMOD_ATTN_DS=0 (environment, read once) keeps the two-kernel form. */
int lmod_attn_bwd_nsplit(int B, int S, int nh, int nkv, int hd, int causal);
int lmod_attn_bwd_split(const void* Q, const void* K, const void* V, const void* O, const void* dO, const float* lse,
                        float* delta_ws, void* dQ, void* dK, void* dV, const int* seqlens, const int* cu_seqlens, int B, int S,
                        int nh, int nkv, int hd, int ldq, int ldk, int ldv, int ldo, int lddo, int lddq, int lddk, int lddv,
                        float scale, int causal, const void* cos_t, const void* sin_t, const int* pos, void* split_ws,
                        long long split_ws_bytes, hipStream_t stream);

/* Single-query attention against a KV cache (generation: llava_qwen2_moe.py:453-473 prepare_inputs_for_generation,
 * qwen2/modeling_qwen2.py:290-309 with q_len 1).  q [B, ldq] (head h at column h*hd), caches [B, smax, ld_cache] (kv head
 * at column hk*hd, keys 0 .. lens[b]-1 valid, the new token's key/value already appended), out [B, ldo]. */
int lmod_attn_decode(const void* q, const void* kcache, const void* vcache, const int* lens, void* out, int B, int nh,
                     int nkv, int hd, int smax, int ldq, int ld_cache, int ldo, float scale, hipStream_t stream);

/* ---- multi-token cache extension and greedy assisted decoding (csrc/append.hip) ----------------------------------------
 * lmod_attn_append: attention of a chunk of new queries against a KV cache that already holds the chunk's own keys and values.
 *   Caches [B, smax, ld_cache] (kv head hk at column hk*hd), lens[b] = valid positions AFTER the append.  Sample b brings n_b new
 *   tokens, 0 <= n_b <= T (0: the sample has no row and nothing is computed or written for it): packed query rows q[cu_new[b] + t], t < n_b (cu_new: device int[B+1]; NULL: every sample brings exactly
 *   T tokens, row b*T + t — the cu_seqlens convention of lmod_attn_fwd); output rows are laid out like q.  Query t of sample b sees
 *   the keys k <= lens[b] - n_b + t; a row without a visible key is exactly 0.  hd 64 or 128, nh % nkv == 0,
 *   1 <= T <= T_MAX = 16 and (nh / nkv) * T <= 128 (LMOD_EUNSUPPORTED beyond).  fp32 throughout, one rounding to bf16 at the output.
 *   The key range is split over `nsplit` workgroups per (sample, kv head) whose (m, l, O) partials a second launch merges in split
 *   order (deterministic): nsplit = 0 lets the library choose (lmod_attn_append_nsplit(B, nkv, smax), less if ws is smaller, 1
 *   without ws), 1 <= nsplit <= 32 forces a count.  ws: 16-byte aligned, ws_bytes >= nsplit * B * nh * T * (hd + 2) * 4 when
 *   nsplit > 1.  T = 1 computes what lmod_attn_decode computes (other summation order).
 * lmod_kv_append_rows: the chunk's post-RoPE K and V columns out of the fused QKV buffer (row cu_new[b] + t, K at column kcol, V at
 *   vcol, `width` = nkv*hd columns each, all multiples of 8) into kcache / vcache [B, smax, ld_cache] at position
 *   lens_before[b] + t, one launch for both tensors.  max_len_after: the caller's upper bound of lens_before[b] + n_b;
 *   LMOD_EINVAL if it exceeds smax (grow the cache first) — the device never clamps a position.
 * lmod_spec_accept: the acceptance rule of greedy assisted decoding.  draft [B, k], target [B, k+1] (argmax of the k+1 verification
 *   rows), 1 <= k < T_MAX; done [B] (in/out), eos (< 0: none), pad.  n_acc[b] = length of the longest prefix with
 *   draft[b, i] == target[b, i] (0 for a sample already done).  Emitted: draft[b, 0:n_acc] then target[b, n_acc], cut after the
 *   first eos (which sets done[b]); a sample already done emits nothing.  out [B, k+5] int32: columns 0..k the emitted tokens
 *   (pad behind them), k+1 n_acc, k+2 the number of emitted tokens, k+3 next_token, k+4 done; next_token [B] = target[b, n_acc]
 *   (pad once done).  lens_target (in: after the k+1-token verification append) -= k - n_acc; lens_draft (in: after the k draft
 *   steps) -= k - min(n_acc + 1, k): both caches then hold the prompt and every emitted token except next_token (the draft also
 *   lacks its k-th draft when all k were accepted); positions behind lens are dead and are overwritten by the next round. */
int lmod_attn_append_nsplit(int B, int nkv, int smax);
int lmod_attn_append(const void* q, const void* kcache, const void* vcache, const int* lens, const int* cu_new, void* out, int B,
                     int T, int nh, int nkv, int hd, int smax, int ldq, int ld_cache, int ldo, float scale, int nsplit, void* ws,
                     long long ws_bytes, hipStream_t stream);
int lmod_kv_append_rows(const void* qkv, int ldqkv, int kcol, int vcol, int width, const int* cu_new, const int* lens_before,
                        void* kcache, void* vcache, int B, int T, int smax, int ld_cache, int max_len_after, hipStream_t stream);
int lmod_spec_accept(const int* draft, const int* target, int k, int* done, int eos, int pad, int* lens_target, int* lens_draft,
                     int* out, int* next_token, int B, hipStream_t stream);

/* ---- long-chunk cache extension (csrc/attn_extend.hip) ----------------------------------------
 * lmod_attn_extend: lmod_attn_append's contract without its chunk limit — causal flash attention (MFMA) of a ragged chunk of
 *   1 <= T <= 65535 new queries per sample against a KV cache that already holds a prefix and the chunk's own keys and values: a later
 *   turn of a conversation, images included, in one pass.  Caches [B, smax, ld_cache] (kv head hk at column hk*hd), lens[b] = valid
 *   positions AFTER the append; packed query rows q[cu_new[b] + t], t < n_b, 0 <= n_b <= T (cu_new: device int[B+1]; NULL: every
 *   sample brings exactly T rows, row b*T + t); output rows are laid out like q.  Query t of sample b sees the keys
 *   k <= lens[b] - n_b + t; a row without a visible key is exactly 0; a sample with n_b = 0 writes nothing.  Positions >= lens[b] are
 *   never read (they may hold anything) and no address at or beyond (b + 1) * smax rows is formed.  hd 64 or 128, nh % nkv == 0
 *   (LMOD_EUNSUPPORTED for another hd, T, B or nh > 65535).  ldq, ldo, ld_cache multiples of 8 and q, out, caches 16-byte aligned
 *   (LMOD_EINVAL).  Scores and the online softmax in fp32; P enters the P V MFMAs as three bf16 terms that hold the fp32 value
 *   exactly; one rounding, of O, to bf16.  No key split and no atomics: two calls give the same bits.  Where both apply (T <= 16) it
 *   computes what lmod_attn_append computes (another summation order: the same kind of bound, not the same bits). */
int lmod_attn_extend(const void* q, const void* kcache, const void* vcache, const int* lens, const int* cu_new, void* out, int B,
                     int T, int nh, int nkv, int hd, int smax, int ldq, int ld_cache, int ldo, float scale, hipStream_t stream);

/* ---- multimodal splice / loss-row plans built on the device ----------------------------------------
 * prepare_inputs_labels_for_multimodal (llava_arch.py:155-334) as index maps, from int tensors already on the device.
 * lmod_splice_count: per sample the spliced length (pads stripped by attention_mask, every -200 token replaced by
 *   n_patches rows, cut at max_length if > 0) and the number of image slots it consumes (max(#-200, 1), :238-246).
 * lmod_splice_fill (S = max spliced length, read back by the host): idx[B*S] (>= 0: embedding row; <= -2: projector
 *   row -(idx+2); -1: right padding), new_labels[B*S] (-100 over image rows and padding), new_mask[B*S] (nullable),
 *   inv_idx[n_images_total * n_patches] (position of every projector row, -1 if cut; caller pre-fills with -1).
 * lmod_lossplan_*: rows of the [B*S] hidden states that carry loss (KD row t: labels[t] != -100, or every row when
 *   all_tokens — align_trainer.py:516-522; CE row t: labels[t+1] != -100 — llava_qwen2_moe.py:413-421), compacted in
 *   sample-major order: row_idx[R], inv_row_idx[B*S], kd_w/ce_w[R], ce_label[R] (-1 where no CE), seg_off[B+1], seg_id[R];
 *   R = sum(counts) is read back by the host between the two calls.  attention_mask: bytes (bool). */
int lmod_splice_count(const long long* input_ids, const unsigned char* attention_mask, int B, int T, int n_patches,
                      int max_length, int* lens, int* n_images, hipStream_t stream);
int lmod_splice_fill(const long long* input_ids, const unsigned char* attention_mask, const long long* labels, int B, int T,
                     int n_patches, int S, const int* lens, const int* n_images, int* idx, long long* new_labels,
                     unsigned char* new_mask, int* inv_idx, hipStream_t stream);
int lmod_lossplan_count(const long long* labels, int B, int S, int kd_rows, int ce_rows, int all_tokens, int* counts,
                        hipStream_t stream);
int lmod_lossplan_fill(const long long* labels, int B, int S, int kd_rows, int ce_rows, int all_tokens, const int* counts,
                       int* row_idx, int* inv_row_idx, float* kd_w, float* ce_w, int* ce_label, int* seg_off, int* seg_id,
                       hipStream_t stream);

/* Greedy decoding: out[r] = argmax_v logits[r, v] over bf16 rows (first maximum wins). */
int lmod_row_argmax_bf16(const void* logits, long long ld, int V, int* out, int R, hipStream_t stream);

/* ---- beam search (generate(num_beams > 1); HF GenerationMixin._beam_search, do_sample=False) ---------------------------
 * lmod_beam_topk_bf16: logits [B*nb, ld] bf16 (V <= ld live columns), beam_scores [B*nb] fp32 -> per sample b the top K = 2*nb of
 *   log_softmax(logits[row]) + beam_scores[row] over its nb rows x V tokens, sorted by score descending, equal scores by the
 *   smaller beam*V + token: out_score [B, K] fp32, out_beam [B, K] (0..nb-1), out_token [B, K].  Two launches: the rows are cut
 *   into chunks of `chunk` tokens (a multiple of 8) that reduce to (max, sum exp, top K) in ws (ws_bytes >=
 *   B * nb * ceil(V / chunk) * (2 + 2 * KC) * 4, KC = 2*nb rounded up to a power of two), one workgroup per sample merges them.
 *   1 <= nb <= 8.
 * lmod_kv_gather_rows: for every tensor t < ntensor (device tables dst[t] / src[t] of [rows, smax, width] bf16 caches, 16-byte
 *   aligned) dst[t][r, 0:lens[r], :] = src[t][src_row[r], 0:lens[r], :], r < R, src_row[r] < R_src; positions >= lens[r] are not
 *   touched.  width % 8 == 0.  dst and src must not overlap (a permutation is not gathered in place). */
int lmod_beam_topk_bf16(const void* logits, long long ld, int V, const float* beam_scores, int B, int nb, int chunk, float* ws,
                        long long ws_bytes, float* out_score, int* out_beam, int* out_token, hipStream_t stream);
int lmod_kv_gather_rows(void* const* dst, const void* const* src, int ntensor, const int* src_row, const int* lens, int R,
                        int R_src, int smax_dst, int smax_src, int width, hipStream_t stream);

/* ---- sampling (generate(do_sample=True); HF's temperature -> top-k -> top-p warpers, then one draw per row) ----------------
 * lmod_sample_bf16: logits [R, ld] bf16 (V <= ld live columns), u [R] fp32 in [0, 1) (device; the library keeps no RNG state) ->
 *   out_token [R].  x = logit / max(temperature, 1e-6) in fp32.  top-k applies when 0 < top_k < V and keeps x >= the k-th largest x
 *   (all ties at that value).  top-p applies when top_p < 1: over the top-k survivors, renormalised and ordered by logit descending
 *   (equal logits by the smaller token id), the shortest prefix whose mass reaches top_p (a token stays while the mass before it is
 *   <= top_p); the nucleus is every token with x >= the logit of the prefix's last token, so the kept set is a threshold on the logit
 *   and a tie group at the cutoff is kept whole.  That is at most part of one tie group more than a sort-based sampler keeps (it
 *   cuts inside the group in the sort's unspecified order).  The maximum is always kept (top_p <= 0 keeps only its tie group).  The
 *   draw is the inverse CDF over the kept set in token-id order: the first kept token whose cumulative kept mass exceeds
 *   u * kept_mass (the last kept token if rounding would run past the end).
 *   out_stats (nullable) [R][4] fp32: {logsumexp of x over all V, kept_mass / total_mass, number of kept tokens, cutoff logit
 *   (unscaled bf16 value; -inf without a filter)}: the drawn token's log-probability under the warped distribution is
 *   x[t] - stats[0] - log(stats[1]).
 *   No sort: the cutoffs are thresholds on the 16-bit order-preserving key of the bf16 logit, found by radix selection with 256-bin
 *   count + mass histograms (high byte, then low byte; one low-byte pass per active filter).  Masses are fixed-point integers
 *   (exp(x - max) * 2^40 in 64 bits), so sums, the cutoff search and the inverse-CDF search are exact integer arithmetic and the
 *   result is bit-for-bit reproducible; a token lighter than 2^-41 of the maximum weighs 0.  Rows are cut into chunks of `chunk`
 *   tokens (a multiple of 8), grid = chunks x rows; 3 launches without a filter, 5 with one, 6 with both, no host read-back.
 *   ws (8-byte aligned): ws_bytes >= R * (64 + 3072 * nh + 16 * ceil(V / chunk)), nh = 0 without a filter, 2 with one, 3 with both.
 *   -inf logits are never drawn; a row without a finite logit gives token 0, lse -inf, kept fraction 0; NaN logits are unspecified
 *   (the token stays in [0, V)).  R <= 65535, V >= 2; R == 0 is a no-op. */
int lmod_sample_bf16(const void* logits, long long ld, int V, const float* u, int R, float temperature, int top_k, float top_p,
                     int chunk, void* ws, long long ws_bytes, int* out_token, float* out_stats, hipStream_t stream);
/* lmod_sample_rows_bf16 (csrc/sample_rows.hip): lmod_sample_bf16 with the parameters of every row in device arrays of R entries
 *   (generate_batch with per-request parameters).  greedy[r] == 0: row r's token and stats are bit for bit what lmod_sample_bf16
 *   returns for that row alone with temperature[r], top_k[r], top_p[r] (same normalisation: T = max(T, 1e-6); top_k <= 0 or >= V: off;
 *   top_p >= 1: off) - integer masses and one shared weight expression make a row independent of its neighbours, its position and the
 *   workspace layout.  greedy[r] != 0: the token is lmod_row_argmax_bf16's (the first maximum; +0 and -0 are one value), the stats
 *   {logsumexp(x) at T = 1, 1, V, -inf}; temperature / top_k / top_p of such a row are not read into the result.
 *   Launches: always the 6 of the both-filters case, whatever the mix; a workgroup whose row takes no part in a histogram pass returns
 *   before its first barrier (a function of the row alone: workgroup-uniform).  ws (8-byte aligned): the nh = 3 layout for every row,
 *   ws_bytes >= R * (64 + 3072 * 3 + 16 * ceil(V / chunk)).  R <= 65535, V >= 2, chunk a multiple of 8; R == 0 is a no-op; the edge
 *   cases of lmod_sample_bf16 (a sampled row without a finite logit: token 0, lse -inf, kept fraction 0; a greedy one: token 0, lse
 *   -inf, kept fraction 1). */
int lmod_sample_rows_bf16(const void* logits, long long ld, int V, const float* u, int R, const float* temperature, const int* top_k,
                          const float* top_p, const int* greedy, int chunk, void* ws, long long ws_bytes, int* out_token,
                          float* out_stats, hipStream_t stream);

/* ---- speculative sampling (generate(assistant_model=..., speculative_sampling=True); Leviathan et al. ICML'23, HF's
 *      _speculative_sampling; csrc/specsample.hip) ---------------------------------------------------------------------------
 * lmod_spec_sample_bf16: verifies k draft tokens per sample so that the emitted tokens are distributed exactly as plain sampling
 *   from the target.  p_logits [B*(k+1), ld_p] bf16: the target's verification rows, row b*(k+1)+i; q_logits [B*k, ld_q] bf16: the
 *   rows the draft drew its tokens from, row b*k+i; V <= min(ld_p, ld_q) live columns; draft [B, k], 1 <= k < T_MAX; u_acc [B, k]
 *   and u_draw [B] fp32 in [0, 1) (device; lmod_spec_uniform makes them).  temperature, top_k, top_p, chunk: as in lmod_sample_bf16.
 *   p_i / q_i are the warped distributions of row i on each side: lmod_sample_bf16's kept-set rule, fixed-point weight
 *   w = round(exp((x - rowmax) / T) * 2^40) (0 outside the kept set) and kept mass M.  Position i is accepted iff
 *   u_acc[b,i] * q_i(d_i) < p_i(d_i) (a draft token outside the target's kept set, or outside [0, V), is always rejected);
 *   n_acc[b] = the number of accepted positions before the first rejection, 0 for a sample already done.  n_acc < k: next_token is
 *   the inverse-CDF draw with u_draw[b], in token-id order, from r(x) = max(0, p_n(x) - q_n(x)), n = n_acc; from p_n when r is zero
 *   everywhere.  n_acc == k: the bonus draw from p_k, the token lmod_sample_bf16 returns for that row and that u.
 *   done / eos / pad / lens_target / lens_draft / out [B, k+5] / next_token [B]: exactly lmod_spec_accept's layout and update rules
 *   with target[b, n_acc] = the drawn token: emitted tokens (pad behind) | n_acc | n_emitted | next_token | done.
 *   out_stats (nullable) [B*(2k+1)][4] fp32: lmod_sample_bf16's stats record of every row, the B*(k+1) p rows first, then the B*k q
 *   rows.
 *   Integer-exact and bit-reproducible: U = floor(u * 2^24); accept iff U * w_q(d) * M_p < 2^24 * w_p(d) * M_q (< 2^122, unsigned
 *   __int128; no 128-bit division); residual weight r(x) = max(0, w_p(x) * M_q - w_q(x) * M_p) >> 24 (<= 2^74, a row sum <= 2^92,
 *   target = (U * sum) >> 24): a token with p(x) - q(x) >= 2^-40 never weighs 0.  Per-chunk residual masses are stored as two u64
 *   by one workgroup each; no 128-bit atomics.
 *   Launches: lmod_sample_bf16's filter passes over all B*(2k+1) rows (2 / 4 / 5 launches without a filter / with one / with both),
 *   accept (one workgroup per sample), residual mass (grid chunks x B, rows n_acc[b] only, index read on the device), draw (one
 *   workgroup per sample): 5 / 7 / 8 launches, no host read-back, no allocation.
 *   ws (8-byte aligned): ws_bytes >= B*(2k+1) * (64 + 3072 * nh + 16 * C) + B * (32 + 16 * C), C = ceil(V / chunk), nh as in
 *   lmod_sample_bf16.  B * (2k+1) <= 65535, V >= 2; B == 0 is a no-op.  A row without a finite logit on either side rejects its
 *   position and draws from p_n (token 0 when p_n has none either); nothing is NaN.
 * lmod_spec_uniform: u[b * n_pos + i] = (w >> 8) * 2^-24 in [0, 1), w = word 0 of Philox4x32-10 with counter
 *   (row0 + b, round, i, purpose) and key = seed, b < B, i < n_pos: a pure function of (seed, row, round, position, purpose);
 *   purpose 0: the draft's own draw, 1: the accept test, 2: the residual / bonus draw. */
int lmod_spec_sample_bf16(const void* p_logits, long long ld_p, const void* q_logits, long long ld_q, int V, const int* draft,
                          const float* u_acc, const float* u_draw, int B, int k, float temperature, int top_k, float top_p, int chunk,
                          void* ws, long long ws_bytes, int* done, int eos, int pad, int* lens_target, int* lens_draft, int* out,
                          int* next_token, float* out_stats, hipStream_t stream);
int lmod_spec_uniform(unsigned long long seed, int row0, int round, int purpose, int n_pos, float* u, int B, hipStream_t stream);

/* ---- logits processors and stop sequences (generate(repetition_penalty / no_repeat_ngram_size / bad_words_ids / suppress_tokens /
 *      min_new_tokens / stop_sequences); HF GenerationMixin semantics, transformers 5.x) ----------------------------------------
 * Shared state, all int32 and caller-owned: hist [R, ld_hist] (a row's live prompt ids followed by what it has generated),
 *   n_hist [R] (tokens in the row), n_prompt [R] (how many of them are prompt), n_gen [R] = n_hist - n_prompt, done [R].  A table of
 *   token sequences is `flat` (all tokens back to back) and `off` [n + 1] (sequence e is flat[off[e] .. off[e+1])).
 * lmod_logits_process_bf16: edits logits [R, ld] bf16 (V live columns) in place, one workgroup per row, in this order (barriers
 *   between the phases): (1) penalty != 1: every DISTINCT history token t gets x = x < 0 ? x * penalty : x / penalty once (fp32 on
 *   the bf16 value, IEEE multiply / divide, one round-to-nearest-even to bf16); first occurrences are found with a V-bit bitmap in
 *   LDS: LMOD_EUNSUPPORTED when V > 524288 (64 KB of LDS) and penalty != 1.  (2) ngram = n > 0 and n_hist >= n: the last token of
 *   every history window of n tokens whose first n-1 tokens equal the history's last n-1 tokens is banned (n = 1: every token seen).
 *   (3) the bad-word table: a one-token entry is banned always, a longer entry's last token when n_hist >= its length and the
 *   history ends with its other tokens.  (4) eos >= 0 and n_gen < min_new: eos is banned.  A ban stores bf16 -inf.  History ids
 *   are compared as plain integers; an id outside [0, V) (the negative image placeholder) is never penalised or banned.  Elements
 *   that no phase touches are not written.  penalty > 0.
 * lmod_gen_push_stop: one step's bookkeeping.  A done row's token becomes `pad`.  A live row's token is appended to hist
 *   (n_hist and n_gen advance; the caller keeps n_hist < ld_hist: a full row is left as it is); done[r] is set when the token is
 *   eos (eos >= 0) or when the row's last len tokens equal a stop sequence of length len and all of them were generated
 *   (n_hist - len >= n_prompt): a match that needs a prompt token does not count. */
int lmod_logits_process_bf16(void* logits, long long ld, int V, int R, const int* hist, int ld_hist, const int* n_hist,
                             const int* n_gen, float penalty, int ngram, const int* bad_flat, const int* bad_off, int n_bad,
                             int min_new, int eos, hipStream_t stream);
int lmod_gen_push_stop(int* tokens, int* done, int* hist, int ld_hist, int* n_hist, const int* n_prompt, int* n_gen, int eos,
                       int pad, const int* stop_flat, const int* stop_off, int n_stop, int R, hipStream_t stream);
/* The same two with per-row parameters in device arrays of R entries (generate_batch with per-request parameters):
 * lmod_logits_process_rows_bf16: row r is bit for bit lmod_logits_process_bf16 on that row alone with penalty[r], ngram[r], min_new[r];
 *   the bad-word table and eos stay per call.  any_penalty: the host's "some penalty[r] != 1" - it requests the V-bit LDS bitmap
 *   (LMOD_EUNSUPPORTED when it is set and V > 524288); a row with penalty 1 skips the penalty phase.  The caller keeps penalty[r] > 0
 *   and ngram[r] >= 0 (device arrays are not checked).
 * lmod_gen_push_stop_rows: lmod_gen_push_stop where row r tests the table's entries [0, n_call) (the call's stop sequences) and
 *   [stop_first[r], stop_first[r] + stop_count[r]) (its own); the table holds n_table >= n_call sequences (off [n_table + 1]).  A
 *   range that leaves [0, n_table] is not tested (nothing is clamped). */
int lmod_logits_process_rows_bf16(void* logits, long long ld, int V, int R, const int* hist, int ld_hist, const int* n_hist,
                                  const int* n_gen, const float* penalty, const int* ngram, const int* min_new, int any_penalty,
                                  const int* bad_flat, const int* bad_off, int n_bad, int eos, hipStream_t stream);
int lmod_gen_push_stop_rows(int* tokens, int* done, int* hist, int ld_hist, int* n_hist, const int* n_prompt, int* n_gen, int eos,
                            int pad, const int* stop_flat, const int* stop_off, int n_call, int n_table, const int* stop_first,
                            const int* stop_count, int R, hipStream_t stream);

/* ---- constrained decoding (generate(constraint=) / generate_batch(constraint=): a token automaton says what a row MAY emit;
 *      csrc/constrain.hip) ------------------------------------------------------------------------------------------------------
 * The automaton (generation.TokenConstraint), all int32: edge_off [n_states + 1], edge_tok / edge_next [E] (CSR: state s owns the
 *   edges [edge_off[s], edge_off[s+1]), tokens strictly ascending inside a state), default_next [n_states], flags [n_states] (bit 0
 *   accept: the row may end here, so eos is allowed; bit 1 terminal: a row that enters is finished).  State s is CLOSED when
 *   default_next[s] < 0 - only tokens with a listed edge whose next >= 0 are allowed - and OPEN otherwise: every token is allowed,
 *   an unlisted one leads to default_next[s], a listed edge redirects its token and one with next < 0 bans it.  state [R]: a row's
 *   current state; a value outside [0, n_states) means "unconstrained" (-1 by convention) and is never used as an index.  The
 *   tables are the host's (validated there); the device trusts them.  n_states >= 1; R == 0 is a no-op.
 * lmod_constrain_mask_rows_bf16: edits logits [R, ld] bf16 (V live columns, ld >= V) in place, one workgroup of 256 threads per row,
 *   after every other processor.  A row with state outside [0, n_states) is not touched.  Open state: every listed edge with
 *   next < 0 and 0 <= tok < V gets bf16 -inf, and so does eos (0 <= eos < V) unless the state accepts; nothing else is read or
 *   written.  Closed state: the allowed tokens - edges with next >= 0 and 0 <= tok < V, and eos when the state accepts - are
 *   collected in a V-bit bitmap in LDS, then every element whose bit is clear becomes bf16 -inf (0xff80).  An allowed element
 *   keeps its bits (NaN, -inf, -0 included).  16-byte-aligned rows are swept 8 elements at a time (a vector that is allowed as a
 *   whole is not written, one that is banned as a whole is not read), the last V % 8 elements and unaligned rows (ld * 2 not a
 *   multiple of 16) element by element.  V > 524288 (64 KB of LDS) has no bitmap: open states work as above, a row in a closed
 *   state is left untouched - the caller refuses such a call beforehand (kernels.constrain_mask_ raises).  eos < 0: no such token.
 * lmod_constrain_advance_rows: one thread per row, after lmod_gen_push_stop / lmod_gen_push_stop_rows.  A row with done[r] != 0 (finished
 *   earlier, or by this step's EOS / stop sequence) or with state[r] outside [0, n_states) is left as it is.  Otherwise
 *   ns = edge_next[e] when tokens[r] has an edge e in the state (binary search), else default_next[state[r]].  ns < 0 (the token
 *   left the automaton; with the mask applied only when the row had no allowed token left): done[r] = 1, the state stays.
 *   Otherwise state[r] = ns, and done[r] = 1 when ns is terminal: the row is finished by that token, as by a stop sequence.
 *
 * Drafting what the automaton forces (generate(constraint=, constraint_draft_tokens=k)): a draft-and-verify round that carries the
 * automaton.  Both entry points: one thread per row, int32 and exact, plain vector stores, no atomics, no workspace; every index is
 * checked and none clamped; 1 <= k < T_MAX (16), LMOD_EINVAL outside; R == 0 is a no-op; a null pointer (edge_tok / edge_next only
 * when E == 0) is LMOD_EINVAL.  They do not depend on where a draft came from.
 * A state s in [0, n_states) is FORCED when it is closed, not terminal, and the set lmod_constrain_mask_rows_bf16 would allow in it -
 *   the edges with next >= 0 and 0 <= tok < V, plus eos where the state accepts and 0 <= eos < V - has exactly one element, and that
 *   element is a listed edge (t, ns) and not eos.  The masked distribution of a forced state is a point mass at t.
 * lmod_constrain_draft: pending [R] (the row's pending token, already emitted), state [R] (the state after that token), done [R].
 *   Walk: s_0 = state[r]; while j < k and s_j is forced with edge (t, ns): draft[j] = t, s_{j+1} = ns (the edge list is scanned
 *   linearly and left at the second allowed edge).  A terminal state is not forced, so the walk stops after a token that enters one.
 *   Outputs: n_draft [R]; draft [R, k]: the run, then -1 (never equal to a target token); chunk [R, k+1]: pending, the run, then
 *   pending again (lmod_ngram_draft's rule: a valid id for the embedding gather, rejected and rewound like a rejected draft);
 *   vstate [R, k+1]: vstate[j] = s_j for j <= n_draft, the state that masks verification row j (the `state` argument of ONE
 *   lmod_constrain_mask_rows_bf16 launch over the [R*(k+1), V] verification logits), -1 behind that and -1 at j = n_draft when s_j
 *   is terminal.  A done row, or a row whose state is outside [0, n_states): n_draft 0, draft all -1, vstate all -1, chunk = pending
 *   repeated.
 * lmod_constrain_accept: lmod_spec_accept's contract with the automaton and a budget, cut on the device.  draft [R, k], target
 *   [R, k+1] (the argmax of the masked verification rows), done [R] (in/out), state [R] (in: after pending; out: after the last
 *   emitted token), n_gen [R] (in/out: tokens the row has emitted), budget (max_new_tokens), lens_target [R] (in: L0 + k + 1, as
 *   the verification pass left it).  A live row: n_acc = the longest prefix with draft[j] == target[j]; the candidates
 *   draft[0:n_acc] then target[n_acc] are emitted in order, n_gen advancing by one each, and after each emitted token, tested in this
 *   order: (1) it is eos (eos >= 0): done, the state stays; (2) it has no edge and no default (ns < 0, lmod_constrain_advance_rows's
 *   rule): done, the state stays; otherwise state = ns, and (3) ns terminal: done; (4) n_gen == budget: done.  Emission stops at the
 *   first token that sets done.  A row whose state is outside [0, n_states) is unconstrained: rules (1) and (4) only.
 *   lens_target[r] = L0 + n_emit: the cache holds the prompt and every emitted token but the last (lmod_batch_lookup_round's
 *   invariant).  A row done at entry emits nothing: n_acc = n_emit = 0, next = pad, lens_target[r] = L0; state and n_gen untouched.
 *   out [R, k+5]: lmod_spec_accept's columns - 0..k the emitted tokens then pad, k+1 n_acc, k+2 n_emit, k+3 the next pending token
 *   (the last emitted one; pad once done), k+4 done; next_token [R] = column k+3. */
int lmod_constrain_mask_rows_bf16(void* logits, long long ld, int V, int R, const int* state, const int* edge_off, const int* edge_tok,
                                  const int* edge_next, const int* default_next, const int* flags, int n_states, int eos,
                                  hipStream_t stream);
int lmod_constrain_advance_rows(const int* tokens, int* done, int* state, const int* edge_off, const int* edge_tok, const int* edge_next,
                                const int* default_next, const int* flags, int n_states, int R, hipStream_t stream);
int lmod_constrain_draft(const int* pending, const int* state, const int* done, const int* edge_off, const int* edge_tok,
                         const int* edge_next, const int* default_next, const int* flags, int n_states, int eos, int V, int k, int* draft,
                         int* chunk, int* vstate, int* n_draft, int R, hipStream_t stream);
int lmod_constrain_accept(const int* draft, const int* target, int k, int* done, int* state, const int* edge_off, const int* edge_tok,
                          const int* edge_next, const int* default_next, const int* flags, int n_states, int eos, int pad, int* n_gen,
                          int budget, int* lens_target, int* out, int* next_token, int R, hipStream_t stream);

/* ---- continuous batching (generate_batch(): a finished slot of the running batch is refilled while the others keep decoding;
 *      csrc/batch.hip) -------------------------------------------------------------------------------------------------------
 * lmod_kv_admit_rows: the scatter that lmod_kv_gather_rows is not.  For every tensor t < ntensor (device tables dst[t] / src[t], 16-byte
 *   aligned bf16 caches) dst[t][dst_row[r], 0:lens[r], :] = src[t][r, 0:lens[r], :], r < R; src [R, smax_src, width] is the temporary
 *   cache an admission prefill wrote, dst [B, smax_dst, width] the slot cache; one launch covers all layers' K and V.  dst_row[r] in
 *   [0, B), pairwise distinct: the host checks, the device trusts (a row outside [0, B) is skipped).  Rows of dst that dst_row does not
 *   name and positions >= lens[r] of the named rows are not written.  width % 8 == 0.  max_len: the caller's upper bound of lens[r];
 *   LMOD_EINVAL if it exceeds smax_dst or smax_src (grow the cache first) - the device never clamps a position (a row longer than
 *   max_len is skipped), the rule of lmod_kv_append_rows.  dst and src must not overlap.  R == 0 is a no-op.
 * lmod_slot_admit: re-arms the generation state of the admitted slots, one launch.  For s = dst_row[r], r < R (s in [0, B), distinct):
 *   hist[s, 0:n_prompt_new[r]] = prompt_ids[r, 0:n_prompt_new[r]] (prompt_ids [R, ld_prompt]; the rest of the history row stays as it
 *   is: it is dead behind n_hist), n_prompt[s] = n_hist[s] = n_prompt_new[r], n_gen[s] = 0, done[s] = 0, cache_lens[s] = lens_new[r],
 *   req_id[s] = req_new[r].  hist / n_hist / n_prompt / n_gen / done are the arrays of lmod_logits_process_bf16 and lmod_gen_push_stop,
 *   cache_lens the slot cache's lens, req_id [B] the request each slot serves.  0 <= n_prompt_new[r] <= min(ld_prompt, ld_hist) (a
 *   request outside is skipped as a whole).  Other slots are not touched.  Plain vector stores, no atomics.
 * lmod_request_uniform: u[s] = (w >> 8) * 2^-24 in [0, 1) (24 bits: exact in fp32, never 1), w = word 0 of Philox4x32-10 with counter
 *   (req_id[s], n_gen[s], 0, 0) and key = seed (low word, high word) - the generator of lmod_moe_gate's noise.  A pure function of
 *   (seed, request, token index): independent of the slot, of the requests beside it and of when it was admitted.
 * lmod_request_uniform_rows: the same mapping with counter (ctr0[s], n_gen[s], 0, 0) and key = seed[s] (u64 [B], 8-byte aligned), both
 *   per slot: a request with a seed of its own runs under (its seed, 0) - the same draws at every list index and in every call - one
 *   without under (the call's seed, its request index), lmod_request_uniform's stream. */
int lmod_kv_admit_rows(void* const* dst, const void* const* src, int ntensor, const int* dst_row, const int* lens, int R, int B,
                       int smax_dst, int smax_src, int width, int max_len, hipStream_t stream);
int lmod_slot_admit(const int* dst_row, const int* prompt_ids, int ld_prompt, const int* n_prompt_new, const int* lens_new,
                    const int* req_new, int R, int B, int* hist, int ld_hist, int* n_prompt, int* n_hist, int* n_gen, int* done,
                    int* cache_lens, int* req_id, hipStream_t stream);
int lmod_request_uniform(unsigned long long seed, const int* req_id, const int* n_gen, float* u, int B, hipStream_t stream);
int lmod_request_uniform_rows(const unsigned long long* seed, const int* ctr0, const int* n_gen, float* u, int B, hipStream_t stream);

/* ---- prompt-lookup decoding (generate(prompt_lookup_num_tokens=k); HF PromptLookupCandidateGenerator; csrc/lookup.hip) -----------
 * The assisted loop's draft without a second model: the continuation of an earlier occurrence of the row's trailing n-gram in the
 * row's own history.  All int32 and exact, no atomics, no workspace: two calls give the same output.
 * lmod_ngram_draft: hist [R, ld_hist] / n_hist [R] / done [R] are the arrays of lmod_logits_process_bf16; the row's pending next token
 *   is already its last element hist[r, L-1], L = n_hist[r].  1 <= k < T_MAX (16) and 1 <= max_ngram <= 8 (LMOD_EINVAL outside);
 *   R == 0 is a no-op.  For n = min(max_ngram, L-1) down to 1: the smallest window start i with hist[i:i+n] == hist[L-n:L] and
 *   i + n < L (a non-empty continuation; the window may overlap the trailing n-gram); the first n that has one wins and the draft is
 *   hist[i+n : min(i+n+k, L)], cut before its first id outside [0, V).  Ids are compared as plain integers (the negative image
 *   placeholder can be part of a match) but a placeholder or a pad is never drafted: when the first continuation id is outside
 *   [0, V) n_draft is 0 and the search does NOT fall through to a shorter n.  A done row, L < 2, L > ld_hist or no match: n_draft 0.
 *   Outputs: n_draft [R]; draft [R, k]: the draft, then -1 (never equal to a target token, so lmod_spec_accept stops there);
 *   chunk [R, k+1]: the verification input: the pending token (as stored; 0 when L < 1 or L > ld_hist), the draft, then the pending
 *   token again (a valid id for the embedding gather; those positions are verified, rejected and rewound like a rejected draft).
 *   One workgroup per row, one strided pass over the history for all n, a block-wide min-reduction per n.
 * lmod_hist_push_block: block [R, k+5] is lmod_spec_accept's output; row r's emitted tokens block[r, 0:n_emitted] (n_emitted =
 *   block[r, k+2]) are appended to hist[r] and n_hist[r] advances, so a live row's history again ends with its pending token
 *   (next_token is the last emitted one).  n_emitted == 0 (a done row) changes nothing; a row whose emission would pass ld_hist, or
 *   whose count is outside [0, k+1], is left as it is. */
int lmod_ngram_draft(const int* hist, int ld_hist, const int* n_hist, const int* done, int R, int k, int max_ngram, int V, int* draft,
                     int* chunk, int* n_draft, hipStream_t stream);
int lmod_hist_push_block(const int* block, int k, int* hist, int ld_hist, int* n_hist, int R, hipStream_t stream);

/* ---- prompt-lookup decoding under continuous batching (generate_batch(prompt_lookup_num_tokens=k); csrc/batch_lookup.hip) --------
 * The round bookkeeping of a batch whose slots are admitted, run and ended independently; it does not depend on where the draft came
 * from.  Slot state (all int32 [B] unless noted): done, hist [B, ld_hist], n_hist, n_prompt, n_gen - the arrays of lmod_slot_admit and
 * lmod_gen_push_stop - and budget (the slot's request's max_new_tokens, >= 1).  The stop table is lmod_gen_push_stop's (stop_flat,
 * stop_off [n_stop + 1]) and so is the test (csrc/stop_match.h): the slot's last len tokens equal a sequence of length len and all of
 * them were generated (n_hist - len >= n_prompt), whichever round emitted them.  A token ENDS a slot when it is eos (eos >= 0), or
 * completes a stop sequence, or brings n_gen to budget.  Both: one thread per slot, exact, no atomics, no workspace; every index
 * is checked and none clamped; B == 0 is a no-op; a null pointer (the stop table only when n_stop > 0) is LMOD_EINVAL.
 * lmod_batch_lookup_first: the first token of freshly admitted slots.  tokens [B]: the argmax of the slots' logits rows.  A slot is
 *   FRESH when done == 0 && n_gen == 0.  Fresh: tokens[s] is appended to the history (n_hist + 1), n_gen = 1, first_tok[s] =
 *   tokens[s], done[s] = 1 when the token ends the slot.  Any other slot: first_tok[s] = -1 and nothing else is touched.  The cache
 *   length is not an argument: the pending token is not in the cache.  A fresh slot whose history row is full (n_hist >= ld_hist) is
 *   left as it is and marked done, first_tok -1.
 * lmod_batch_lookup_round: acceptance, emission and every end condition of one round.  draft [B, k] (lmod_ngram_draft's: the draft,
 *   then -1), target [B, k+1] (the argmax of the k+1 verification rows), first_tok [B] (above), cache_lens [B] as the verification pass
 *   left them, L0 + k + 1.  1 <= k < T_MAX (16), LMOD_EINVAL outside.  Output block [B, k+6]: columns 0..k the emitted tokens then
 *   pad, k+1 n_acc, k+2 n_emit, k+3 the next pending token (pad when fin), k+4 fin, k+5 first_tok[s].
 *   A slot done at entry: tokens pad, n_acc = n_emit = 0, next = pad, fin = 1, cache_lens[s] = L0 (an idle slot stays where it is
 *   however many rounds pass); history and n_gen untouched.  A live slot: n_acc = the longest prefix with draft[j] == target[j]; the
 *   candidates draft[0 .. n_acc) then target[n_acc] are emitted in order - appended to the history, n_gen and n_emit advance - and
 *   emission stops after a candidate that ends the slot (fin = 1; otherwise all n_acc + 1 are emitted and fin = 0); done[s] = fin;
 *   cache_lens[s] = L0 + n_emit: the cache holds the prompt and every emitted token but the last, plain greedy's invariant (the next
 *   pending token is the last one emitted).  A history row that fills up stops the emission there and ends the slot; cache_lens below
 *   k + 1 (no verification pass left them) ends the slot and is not written. */
int lmod_batch_lookup_first(const int* tokens, int* done, int* hist, int ld_hist, int* n_hist, const int* n_prompt, int* n_gen,
                            const int* budget, int eos, const int* stop_flat, const int* stop_off, int n_stop, int* first_tok, int B,
                            hipStream_t stream);
int lmod_batch_lookup_round(const int* draft, const int* target, const int* first_tok, int k, int* done, int* hist, int ld_hist,
                            int* n_hist, const int* n_prompt, int* n_gen, const int* budget, int* cache_lens, int eos, int pad,
                            const int* stop_flat, const int* stop_off, int n_stop, int* block, int B, hipStream_t stream);

/* ---- sparse MoE (DeepSpeed 0.9.5 TopKGate/top1gating/top2gating/MOELayer semantics) ------------
 * logits[T,E] = x.float() @ wg^T  (TopKGate.forward; wg kept fp32).
 * Experts per layer: 1 <= E <= 32 (`--num_experts`, config/args.py:46); the per-token kernels are instantiated for
 * ME = 8 / 16 / 32 expert slots and picked by E. */
int lmod_moe_router_fwd(const void* x, const float* wg, float* logits, int T, int H, int E, hipStream_t stream);
/* top-k (k in {1,2}) gating with capacity C: token-order slot assignment, drops, renormalised
 * combine weights, l_aux, exp_counts, slots_used[E] (live rows per capacity slab).
 * k = 2 (top2gating): `noise` [T,E] is added to the logits for the 2nd choice (NULL: none); noise_mode 1 draws
 *   Gumbel(0,1) noise in the kernel (Philox4x32-10 keyed by seed, counter = offset + token) — gumbel_rsample.
 * k = 1 (top1gating): `noise` [T,E] holds the random-token-selection priorities (use_rts=True: per expert the C tokens
 *   with the largest priority keep their slot, survivors numbered in token order; NULL: token order, use_rts=False);
 *   noise_mode 2 draws U(0,1) priorities in the kernel.
 * noise_out (nullable, [T,E]) receives the drawn noise.  scratch: 4*T + 3*ME*ceil(T/512) int32, ME = 8 / 16 / 32 for
 *   E <= 8 / 16 / 32. */
int lmod_moe_gate(const float* logits, const float* noise, int T, int E, int k, int C, float* gates, int* idx1,
                  int* idx2, int* slot1, int* slot2, float* w1, float* w2, int* slot_token, float* slot_w,
                  int* exp_counts, float* gate_sum, float* l_aux, int* slots_used, int* scratch, int noise_mode,
                  unsigned long long seed, unsigned long long offset, float* noise_out, hipStream_t stream);
/* out[t] = bf16(w1)*y[slot1[t]] + bf16(w2)*y[slot2[t]]   (einsum 'sec,ecm->sm'). */
int lmod_moe_combine_fwd(const void* y, const int* slot1, const int* slot2, const float* w1, const float* w2,
                         void* out, int T, int H, hipStream_t stream);
int lmod_moe_combine_bwd(const void* dout, const void* y, const int* slot1, const int* slot2, const int* slot_token,
                         const float* slot_w, void* dy, float* dw1, float* dw2, int T, int S, int H,
                         hipStream_t stream);
int lmod_moe_gate_bwd(const float* gates, const int* idx1, const int* idx2, const int* slot1, const int* slot2,
                      const float* dw1, const float* dw2, const int* exp_counts, const float* d_laux, float* dlogits,
                      int T, int E, int k, hipStream_t stream);
int lmod_moe_dispatch_bwd(const void* d_in, const int* slot1, const int* slot2, const float* dlogits, const float* wg,
                          void* dx, int T, int H, int E, hipStream_t stream);
/* dwg[E,H] (+)= dlogits^T x (fp32 router weight gradient).  workspace: ceil(T/64) * E * H floats.  H % 8 == 0. */
int lmod_moe_router_wgrad(const void* x, const float* dlogits, float* dwg, float* workspace, int T, int H, int E,
                          int accumulate, hipStream_t stream);

/* Residual-MoE (deepspeed.moe.layer.MoE(use_residual=True); flag at config/args.py:54-56, passed through at
 * llava_qwen2_moe.py:536-546): out = moe_out * c0 + mlp_out * c1 with (c0, c1) = softmax(coef_logits + coef_bias), the
 * 2-way `coefficient` Linear(hidden, 2); roundings follow the bf16 module.  p[T,2] (fp32) is saved for the backward,
 * which returns d_moe, d_mlp (bf16) and d_coef_logits[T,2] (fp32).  coef_logits come from lmod_moe_router_fwd (E = 2),
 * the coefficient weight gradient from lmod_moe_router_wgrad, its input gradient from lmod_small_linear_dgrad:
 * dx[T,H] (bf16) = dlogits[T,E] @ w[E,H] (fp32, E <= 32, H % 8 == 0). */
int lmod_moe_residual_mix_fwd(const void* moe_out, const void* mlp_out, const float* coef_logits, const float* coef_bias,
                              void* out, float* p, int T, int H, hipStream_t stream);
int lmod_moe_residual_mix_bwd(const void* dout, const void* moe_out, const void* mlp_out, const float* p, void* d_moe,
                              void* d_mlp, float* d_coef_logits, int T, int H, hipStream_t stream);
int lmod_small_linear_dgrad(const float* dlogits, const float* w, void* dx, int T, int H, int E, hipStream_t stream);

/* ---- distillation losses -----------------------------------------------------------------------
 * One pass per logits row.  stats[R][8] = {lse_s_full, lse_s_align, lse_t_align, x_kd, ce, s[label],
 * finite_mass, 0}:  x_kd = sum_v softmax(t[:Va])_v * log_softmax(s[:Va])_v with the isinf mask
 * (AlignTrainer.get_p/get_logp/compute_align_loss, align_trainer.py:455-528);  ce = lse_full - s[label]
 * (CrossEntropyLoss of llava_qwen2_moe.py:407-421; DPOTrainer.get_logp per-token logp = -ce,
 * dpo_trainer.py:483-495).  t may be NULL (no teacher row). */
int lmod_rowloss_fwd(const void* s, long long ld_s, int Vs, const void* t, long long ld_t, int Va, const int* label,
                     float* stats, int R, hipStream_t stream);
/* ds = kd_w[r]*kd_scale[seg]*(softmax_a(s)-softmax_a(t))[v<Va] + ce_w[r]*ce_scale[seg]*(softmax(s)-onehot). */
int lmod_rowloss_bwd(const void* s, long long ld_s, int Vs, const void* t, long long ld_t, int Va, const int* label,
                     const float* stats, const float* kd_w, const float* ce_w, const int* seg_id,
                     const float* kd_scale, const float* ce_scale, void* ds, long long ld_ds, int R,
                     hipStream_t stream);
/* out_sum[b] = sum_{r in [seg_off[b], seg_off[b+1])} w[r]*val[r*stride+col]; out_w[b] = sum w[r]. */
int lmod_segment_wsum(const float* val, int stride, int col, const float* w, const int* seg_off, int nseg,
                      float* out_sum, float* out_w, hipStream_t stream);
/* Materialising forms of AlignTrainer.get_p / get_logp (align_trainer.py:473-475,497-499): fp32 logits ->
 * fp32 softmax / log_softmax of the first Va columns; and the masked product-sum of compute_align_loss
 * (:509-514).  Slow-path API parity only; training uses lmod_rowloss_*. */
int lmod_row_softmax_f32(const float* logits, long long ld, int Va, int log_flag, float* out, int R,
                         hipStream_t stream);
int lmod_rowdot_masked(const float* p, const float* logp, int V, int R, float* x, hipStream_t stream);
/* DPOTrainer.dpo_loss (dpo_trainer.py:497-562), forward + d(mean loss)/d(policy logps).
 * loss_type: 0 sigmoid, 1 hinge, 2 ipo, 3 kto_pair (losses has 2B entries). */
int lmod_dpo_loss(const float* policy_chosen, const float* policy_rejected, const float* ref_chosen,
                  const float* ref_rejected, int B, float beta, float label_smoothing, int loss_type, float* losses,
                  float* chosen_rewards, float* rejected_rewards, float* d_policy_chosen, float* d_policy_rejected,
                  hipStream_t stream);

/* ---- collectives of the data-parallel step (RCCL over xGMI; bound at run time, no link dependency) -------------------
 * Replace what DeepSpeed's engine does for the reference around each optimizer step (train/align_trainer.py:326-434 builds it
 * from config/dpconfig/zero2*.json: gradient reduce-scatter / all-reduce, parameter all-gather) and the two all-to-alls of
 * deepspeed.moe.sharded_moe.MOELayer.forward (call site llava_qwen2_moe.py:536-546).  One communicator per process / GPU.
 * The Python package drives the same exchanges through torch.distributed; these are the boundary for other hosts. */
/* rank 0: fill the 128-byte communicator id; the host distributes it to the other ranks. */
int lmod_comm_unique_id(void* id128);
/* collective over all `world` ranks (current HIP device = this rank's GPU); *comm receives the handle. */
int lmod_comm_init(void** comm, const void* id128, int rank, int world);
int lmod_comm_destroy(void* comm);
/* buf[0..n) <- SUM over ranks, in place.  dtype: 0 fp32, 1 bf16.  (The mean's 1/world goes into lmod_adamw_step's grad_scale.) */
int lmod_allreduce_grads(void* comm, void* buf, long long n, int dtype, hipStream_t stream);
/* ZeRO-2 gradient phase: span[0 .. world*n_per_rank) -> chunk `rank` of the SUM, in place at span + rank*n_per_rank. */
int lmod_reduce_scatter_grads(void* comm, void* span, long long n_per_rank, int dtype, hipStream_t stream);
/* ZeRO-2 parameter phase: every rank publishes its updated chunk (span + rank*n_per_rank) to all, in place. */
int lmod_allgather_params(void* comm, void* span, long long n_per_rank, int dtype, hipStream_t stream);
/* Expert-parallel exchange of PACKED live rows (bf16, H wide): send_rows[d] consecutive rows of `send` go to peer d, recv_rows[s]
 * rows from peer s land consecutively in `recv` (HOST arrays of `world` counts).  One ncclSend / ncclRecv per peer in one group. */
int lmod_moe_all_to_all(void* comm, const void* send, void* recv, const long long* send_rows, const long long* recv_rows,
                        int H, hipStream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* LMOD_HIP_H */
