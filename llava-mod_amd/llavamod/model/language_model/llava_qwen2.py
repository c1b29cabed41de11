"""LlavaQwen2ForCausalLM — the dense teacher API (reference language_model/llava_qwen2.py:31-130, which wraps
the vendored Qwen2ForCausalLM, qwen2/modeling_qwen2.py:1129-1190).  Same constructor-from-config,
`get_model()`, `forward(input_ids, attention_mask, …, labels, images, return_dict)` and output fields
(`loss`, `logits` fp32 [B,S',V], `labels` after the image splice); execution is on the HIP kernels.
`LlavaQwen1_5ForCausalLM` (llava_qwen1_5.py) is the same class: the two files differ in names only.
"""
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn as nn

from ... import kernels as K
from ... import ops
from ...constants import IGNORE_INDEX
from ...ops import FusedWeight
from ..llava_arch import LlavaMetaForCausalLM, LlavaMetaModel
from ..utils import CausalLMOutputWithPast
from .qwen2_hip import KVCache, Qwen2Config, Qwen2Model, _Linear, init_normal_

BF16 = torch.bfloat16


class LlavaQwen2Config(Qwen2Config):
    model_type = "llava_qwen2"


class LlavaQwen2Model(LlavaMetaModel, Qwen2Model):
    config_class = LlavaQwen2Config

    def __init__(self, config, device="cuda"):
        Qwen2Model.__init__(self, config, device)
        self._init_vision(config, device)


def build_loss_plan(labels_np, lens_np, kd_rows=True, ce_rows=True, distill_all_tokens=False, align_vocab=None,
                    device="cuda"):
    """Which rows of the flattened [B*S'] hidden states carry loss, in sample-major order.
      KD row t  : labels[b,t] != -100          (UNshifted mask, align_trainer.py:522; or every row incl. pads
                                               when distill_all_tokens, :516-520)
      CE row t  : labels[b,t+1] != -100        (shifted LM / DPO rows, llava_qwen2_moe.py:413-421, dpo_trainer.py:483-485)
    """
    if torch.is_tensor(labels_np):
        return build_loss_plan_device(labels_np, kd_rows, ce_rows, distill_all_tokens, align_vocab)
    B, S = labels_np.shape
    valid = labels_np != IGNORE_INDEX
    kd = (np.ones_like(valid) if distill_all_tokens else valid) if kd_rows else np.zeros_like(valid)
    ce = np.zeros_like(valid)
    if ce_rows:
        ce[:, :-1] = valid[:, 1:]
    ce_label = np.full((B, S), -1, dtype=np.int32)
    ce_label[:, :-1] = np.where(valid[:, 1:], labels_np[:, 1:], -1)
    need = kd | ce
    bi, ti = np.nonzero(need)                                   # row-major => sample-major order
    rows = (bi * S + ti).astype(np.int32)
    seg_off = np.zeros(B + 1, dtype=np.int32)
    np.cumsum(np.bincount(bi, minlength=B), out=seg_off[1:])
    inv = np.full(B * S, -1, dtype=np.int32)
    inv[rows] = np.arange(len(rows), dtype=np.int32)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
    return SimpleNamespace(R=len(rows), row_idx=t(rows), inv_row_idx=t(inv), kd_w=t(kd[bi, ti].astype(np.float32)),
                           ce_w=t(ce[bi, ti].astype(np.float32)), ce_label=t(ce_label[bi, ti]),
                           seg_off=t(seg_off), seg_id=t(bi.astype(np.int32)), align_vocab=align_vocab, shape=(B, S),
                           labels_np=labels_np,
                           n_kd=int(kd.sum()), n_ce=int(ce.sum()))


def build_loss_plan_device(labels, kd_rows=True, ce_rows=True, distill_all_tokens=False, align_vocab=None):
    """`build_loss_plan` on the device (csrc/splice.hip) from the spliced labels [B, S'] (device int64): two launches and
    one B-int read-back (R, the number of loss rows, sizes the outputs)."""
    from ..._hip import call, ptr
    dev = labels.device
    B, S = labels.shape
    lb = labels.to(torch.int64).contiguous()
    counts = torch.empty(B, device=dev, dtype=torch.int32)
    flags = (int(bool(kd_rows)), int(bool(ce_rows)), int(bool(distill_all_tokens)))
    call("lmod_lossplan_count", ptr(lb), B, S, *flags, ptr(counts))
    R = int(counts.sum().item())
    i32 = dict(device=dev, dtype=torch.int32)
    row_idx, inv = torch.empty(R, **i32), torch.empty(B * S, **i32)
    kd_w, ce_w = torch.empty(R, device=dev), torch.empty(R, device=dev)
    ce_label, seg_off, seg_id = torch.empty(R, **i32), torch.empty(B + 1, **i32), torch.empty(R, **i32)
    call("lmod_lossplan_fill", ptr(lb), B, S, *flags, ptr(counts), ptr(row_idx), ptr(inv), ptr(kd_w), ptr(ce_w), ptr(ce_label),
         ptr(seg_off), ptr(seg_id))
    return SimpleNamespace(R=R, row_idx=row_idx, inv_row_idx=inv, kd_w=kd_w, ce_w=ce_w, ce_label=ce_label, seg_off=seg_off,
                           seg_id=seg_id, align_vocab=align_vocab, shape=(B, S), labels_np=None, labels_dev=lb,
                           n_kd=None, n_ce=None)


def _inverse_map(packed):
    """packed row -> padded position (int32 [T]), cached on the plan."""
    if getattr(packed, "from_packed", None) is None:
        keep = np.nonzero(packed.to_packed_np >= 0)[0].astype(np.int32)
        packed.from_packed = torch.from_numpy(keep).to(packed.to_packed.device)
    return packed.from_packed


class _CausalLMBase(nn.Module, LlavaMetaForCausalLM):
    """Shared forward machinery of the dense teacher and the MoE student."""

    def _setup_head(self, config, device):
        self.vocab_size = config.vocab_size
        self.lm_head = _Linear(config.hidden_size, config.vocab_size, False, device)
        self._head = FusedWeight([[self.lm_head.weight]])

    def get_model(self):
        return self.model

    def head(self):
        return self._head.ensure()

    # ---- internal fast path -------------------------------------------------------------------
    def forward_hidden(self, input_ids=None, attention_mask=None, labels=None, images=None, inputs_embeds=None,
                       plan_fn=None):
        """Splice + decoder.  Returns (hidden [B*S', H], moe_loss_list, info) — no logits.
        plan_fn(info) -> loss plan: the decoder then returns just the plan's rows ([R, H], `info.plan.pregathered`),
        letting a dense last layer skip (forward and backward) the rows nobody reads."""
        if inputs_embeds is None:
            _, _, attention_mask, _, inputs_embeds, labels = self.prepare_inputs_labels_for_multimodal(
                input_ids, None, attention_mask, None, labels, images)
            plan = self._plan
            if inputs_embeds is None:                          # text-only batch
                dev = self.model.embed_tokens.weight.device
                B, S = input_ids.shape
                idx = input_ids.to(device=dev, dtype=torch.int32).reshape(-1).contiguous()
                inputs_embeds = ops.SpliceEmbed.apply(None, self.model.embed_tokens.weight, idx, None).view(B, S, -1)
        else:
            plan = None
        B, S, H = inputs_embeds.shape
        seqlens = None
        packed = plan is not None and getattr(plan, "cu", None) is not None      # unpadded (varlen) execution
        if packed:
            B, S = plan.B, plan.S                              # embeds arrive as packed rows [1, T, H]
        if plan is not None:
            seqlens = plan.seqlens
        elif attention_mask is not None:
            lens = attention_mask.to(torch.int32).sum(1)
            if bool((lens != S).any()):
                seqlens = lens.to(device=inputs_embeds.device, dtype=torch.int32).contiguous()
        if labels is not None:
            if plan is not None:
                labels_np = plan.labels_np if plan.labels_np is not None else labels      # device-built plan: stay on device
            else:
                labels_np = labels if labels.is_cuda else labels.detach().cpu().numpy()
        else:
            labels_np = None
        lens_np = plan.lens_np if plan is not None else None
        info = SimpleNamespace(B=B, S=S, labels=labels, labels_np=labels_np, lens_np=lens_np,
                               attention_mask=attention_mask, plan=None)
        out_rows = inv_rows = None
        if plan_fn is not None and labels_np is not None:
            info.plan = plan_fn(info)
            if packed:
                from ..llava_arch import pack_loss_plan
                info.plan = pack_loss_plan(info.plan, plan)
            elif getattr(info.plan, "is_packed", False):
                # e.g. a teacher that ran unpadded handing its plan to a student that runs padded: the row indices would
                # address packed rows in a padded buffer
                raise ValueError("loss plan is in packed (unpadded) coordinates but this model executes padded: set `unpad` "
                                 "identically on the teacher and the student")
            info.plan.pregathered = True
            out_rows, inv_rows = info.plan.row_idx, info.plan.inv_row_idx
        if packed:
            info.packed = plan
            hidden, moe_list = self.model(inputs_embeds.reshape(-1, H), B, S, None, out_rows=out_rows, inv_rows=inv_rows,
                                          cu=plan.cu, pos=plan.pos)
        else:
            hidden, moe_list = self.model(inputs_embeds.reshape(B * S, H), B, S, seqlens, out_rows=out_rows,
                                          inv_rows=inv_rows)
        return hidden, moe_list, info

    # ---- generation (KV cache) -------------------------------------------------------------------------------------
    def prepare_inputs_for_generation(self, input_ids, past_key_values=None, inputs_embeds=None, attention_mask=None, **kwargs):
        """HF contract of the reference (llava_qwen2_moe.py:453-473): after the first step only the last token is fed and the
        images are dropped; `images` rides along on the first step."""
        images = kwargs.pop("images", None)
        if past_key_values is not None:
            input_ids = input_ids[:, -1:]
        model_inputs = {"inputs_embeds": inputs_embeds} if (inputs_embeds is not None and past_key_values is None) \
            else {"input_ids": input_ids}
        model_inputs.update({"past_key_values": past_key_values, "use_cache": kwargs.get("use_cache", True),
                             "attention_mask": attention_mask})
        if images is not None and past_key_values is None:
            model_inputs["images"] = images
        return model_inputs

    @torch.no_grad()
    def _prefill(self, input_ids, attention_mask, images, max_new_tokens):
        """Splice + full forward storing K/V; returns (cache, bf16 logits [B, V] of each sample's LAST valid position)."""
        unpad, self.unpad = getattr(self, "unpad", False), False       # the KV cache is laid out per padded sample
        try:
            _, _, am, _, embeds, _ = self.prepare_inputs_labels_for_multimodal(input_ids, None, attention_mask, None, None, images)
        finally:
            self.unpad = unpad
        plan = self._plan
        dev = self.model.embed_tokens.weight.device
        if embeds is None:
            B, S = input_ids.shape
            idx = input_ids.to(device=dev, dtype=torch.int32).reshape(-1).contiguous()
            embeds = K.gather_rows(self.model.embed_tokens.weight, None, idx, self.model.embed_tokens.weight.shape[1]).view(B, S, -1)
            am = attention_mask
        B, S, H = embeds.shape
        if embeds is not None and plan is not None:
            # spliced batch: the plan knows every sample's real length (also when no attention_mask was given but the
            # samples splice to different lengths)
            lens = torch.from_numpy(plan.lens_np.astype("int32")).to(dev)
        elif am is not None:
            amd = am.to(device=dev).to(torch.int32)
            lens = amd.sum(1).to(torch.int32)
            # the cache and the last-token row are addressed as b*S + len-1: RIGHT padding only (the reference's
            # `padding_side="right"`, align_train.py:366).  A left-padded mask would silently read the wrong rows.
            if bool((amd[:, 1:] > amd[:, :-1]).any()):
                raise ValueError("generate/use_cache expects RIGHT-padded prompts (attention_mask must be non-increasing along "
                                 "the sequence); left padding is not supported on this path")
        else:
            lens = torch.full((B,), S, device=dev, dtype=torch.int32)
        seqlens = lens.contiguous() if bool((lens != S).any()) else None
        cfg = self.config
        cache = KVCache(cfg.num_hidden_layers, B, S + max_new_tokens, cfg.num_key_value_heads * cfg.head_dim, dev)
        rows = (torch.arange(B, device=dev, dtype=torch.int32) * S + lens - 1).to(torch.int32).contiguous()
        inv = torch.full((B * S,), -1, device=dev, dtype=torch.int32)
        inv[rows.long()] = torch.arange(B, device=dev, dtype=torch.int32)
        hidden, _ = self.model(embeds.reshape(B * S, H), B, S, seqlens, out_rows=rows, inv_rows=inv, cache=cache)
        cache.lens.copy_(lens)
        return cache, ops.linear_fwd(hidden, self.head())

    generation_budget = 512            # cache positions reserved beyond the prompt by a `use_cache=True` forward
    sample_on_device = True            # generate(do_sample=True) draws with lmod_sample_bf16; False: the torch `_sample` (A/B baseline)

    @torch.no_grad()
    def _cached_forward(self, input_ids, attention_mask, images, past, out_cls):
        """`forward(..., use_cache=True / past_key_values=...)` as HF's generation loop drives it: the first call prefills
        and returns the cache, later calls feed the last token.  logits: [B, 1, V] fp32 (the last position only)."""
        if past is None:
            cache, logits = self._prefill(input_ids, attention_mask, images, self.generation_budget)
        else:
            cache = past
            dev = cache.lens.device
            if input_ids.shape[1] > 1:           # a chunk of new tokens: fp32 logits [B, T, V], rows of padded positions zero; grows the cache
                return out_cls(loss=None, logits=self._append_chunk(input_ids, attention_mask, cache, "all", images=images),
                               past_key_values=cache)
            if int(cache.lens.max()) >= cache.smax:
                raise ValueError("KV cache exhausted: raise `generation_budget` before the prefill")
            logits = self._decode_step(input_ids[:, -1].to(device=dev, dtype=torch.int32), cache)
        return out_cls(loss=None, logits=logits.float().unsqueeze(1), past_key_values=cache)

    extend_min_tokens = 17             # a chunk whose longest sample has at least this many live tokens runs in ONE pass
    #                                    (forward_extend / lmod_attn_extend); shorter ones in pieces of APPEND_T_MAX.  Huge: always pieces

    @torch.no_grad()
    def _append_chunk(self, input_ids, attention_mask, cache, want, reserve=0, images=None):
        """Push input_ids [B, T] (attention_mask None or [B, T], right-padded, covering the chunk only) through the model against
        `cache` — the continuation of a conversation.  Only live rows enter the decoder.  The cache grows if it has to (plus
        `reserve` positions).
        Text-only chunk whose longest sample has fewer than `extend_min_tokens` live tokens: pieces of at most APPEND_T_MAX tokens
        per sample (Qwen2Model.forward_append).  Otherwise ONE pass over the packed live rows (Qwen2Model.forward_extend).
        images: the chunk's IMAGE_TOKEN_INDEX placeholders are spliced exactly as `_prefill` splices a prompt (right-padded, `unpad`
        off, lengths from the splice plan) and the spliced rows go through forward_extend whatever their count; T below is then the
        longest SPLICED length.  An image token without `images` raises.
        want="all": fp32 logits [B, T, V] with zero rows on padded positions; want="last": bf16 logits [B, V] of every sample's last
        live token."""
        from ...constants import IMAGE_TOKEN_INDEX
        dev = cache.lens.device
        ids = input_ids.to(dev)
        B, T = ids.shape
        if B != cache.lens.shape[0]:
            raise ValueError(f"the cache holds {cache.lens.shape[0]} samples, input_ids {B}")
        if attention_mask is not None:
            amd = attention_mask.to(device=dev).to(torch.int32)
            if tuple(amd.shape) != (B, T):
                raise ValueError("with past_key_values and more than one new token the attention_mask covers the chunk only: [B, T]")
            if bool((amd[:, 1:] > amd[:, :-1]).any()):
                raise ValueError("generate/use_cache expects RIGHT-padded prompts (attention_mask must be non-increasing along "
                                 "the sequence); left padding is not supported on this path")
            n_all = amd.sum(1).to(torch.int32)
            if bool((n_all < 1).any()):
                raise ValueError("every sample of a continuation chunk needs at least one live token")
        else:
            n_all = torch.full((B,), T, device=dev, dtype=torch.int32)
        emb = None
        if images is not None:
            unpad, self.unpad = getattr(self, "unpad", False), False       # the KV cache is laid out per padded sample
            try:
                _, _, _, _, embeds, _ = self.prepare_inputs_labels_for_multimodal(input_ids, None, attention_mask, None, None, images)
            finally:
                self.unpad = unpad
            if embeds is not None:
                # spliced chunk: the plan knows every sample's real length; pack the live rows sample-major
                n_all = torch.from_numpy(self._plan.lens_np.astype("int32")).to(dev)
                T = embeds.shape[1]
                emb = embeds[torch.arange(T, device=dev)[None, :] < n_all[:, None]].contiguous()
        if emb is None and bool((ids == IMAGE_TOKEN_INDEX).any()):
            raise ValueError("image tokens in a continuation chunk need their `images`: without them a chunk fed with "
                             "past_key_values is text-only")
        n_host = n_all.cpu()
        hi = int(cache.lens.max())
        if hi + T + reserve > cache.smax:
            cache.grow(hi + T + reserve)
        emb_w = self.model.embed_tokens.weight
        V = self.lm_head.weight.shape[0]
        out = torch.zeros((B, T, V), device=dev, dtype=torch.float32) if want == "all" else torch.empty((B, V), device=dev, dtype=BF16)
        if emb is not None or int(n_host.max()) >= self.extend_min_tokens:
            live = torch.arange(T, device=dev)[None, :] < n_all[:, None]
            if emb is None:
                emb = K.gather_rows(emb_w, None, ids[live].to(torch.int32).contiguous(), emb_w.shape[1])   # packed, sample-major
            uniform = emb.shape[0] == B * T
            hidden = self.model.forward_extend(emb, cache, T if uniform else n_all, T=T, max_len=hi)
            if want == "all":
                out[live] = ops.linear_fwd(hidden, self.head()).float()
                return out
            return ops.linear_fwd(hidden[(n_host.cumsum(0) - 1).to(dev)].contiguous(), self.head())
        for j0 in range(0, T, K.APPEND_T_MAX):
            Tp = min(K.APPEND_T_MAX, T - j0)
            n_p = (n_all - j0).clamp(0, Tp).to(torch.int32)
            nh_p = (n_host - j0).clamp(0, Tp)
            R = int(nh_p.sum())
            if R == 0:
                break
            live = torch.arange(Tp, device=dev)[None, :] < n_p[:, None]
            uniform = R == B * Tp
            tok = ids[:, j0:j0 + Tp][live].to(torch.int32).contiguous()                 # packed, sample-major
            emb = K.gather_rows(emb_w, None, tok, emb_w.shape[1])
            hidden = self.model.forward_append(emb, cache, Tp if uniform else n_p, T=Tp, max_len=hi + j0)
            lg = ops.linear_fwd(hidden, self.head())
            if want == "all":
                out[:, j0:j0 + Tp][live] = lg.float()
            else:
                ends = (nh_p > 0) & (n_host <= j0 + Tp)                                  # samples whose last live token is in this piece
                rows = (nh_p.cumsum(0) - 1)[ends].to(dev)
                out[ends.to(dev)] = lg[rows]
        return out

    def _start(self, input_ids, attention_mask, images, max_new_tokens, past):
        """Where every generation mode begins: the prompt's prefill, or — continuing from `past` — the new turn's tokens (with the
        turn's own `images`, if it has any) through the chunk path.  Returns (cache with room for max_new_tokens more positions, bf16
        logits [B, V] of every sample's last token)."""
        if past is None:
            return self._prefill(input_ids, attention_mask, images, max_new_tokens)
        if input_ids.shape[1] == 1 and images is None:
            if int(past.lens.max()) + 1 + max_new_tokens > past.smax:
                past.grow(int(past.lens.max()) + 1 + max_new_tokens)
            return past, self._decode_step(input_ids[:, 0].to(device=past.lens.device, dtype=torch.int32), past)
        return past, self._append_chunk(input_ids, attention_mask, past, "last", reserve=max_new_tokens, images=images)

    @torch.no_grad()
    def _decode_step(self, tokens, cache):
        """tokens [B] (device int32) -> bf16 logits [B, V] of the next position."""
        emb = K.gather_rows(self.model.embed_tokens.weight, None, tokens.contiguous(), self.model.embed_tokens.weight.shape[1])
        return ops.linear_fwd(self.model.forward_decode(emb, cache), self.head())

    @staticmethod
    def _sample(logits, temperature, top_k, top_p, gen):
        """Next token per row from bf16 logits [B, V] — HF's sampling warpers (temperature, top-k, nucleus) in that order, then
        one multinomial draw.  O(B x V) host-glue torch math on B rows (B = number of sequences being generated)."""
        x = logits.float() / max(float(temperature), 1e-6)
        if top_k is not None and 0 < top_k < x.shape[-1]:
            kth = torch.topk(x, top_k, dim=-1).values[:, -1:]
            x = x.masked_fill(x < kth, float("-inf"))
        if top_p is not None and top_p < 1.0:
            sv, si = torch.sort(x, dim=-1, descending=True)
            cp = torch.softmax(sv, dim=-1).cumsum(-1)
            drop = cp - torch.softmax(sv, dim=-1) > top_p          # keep the smallest prefix whose mass reaches top_p
            sv = sv.masked_fill(drop, float("-inf"))
            x = torch.full_like(x, float("-inf")).scatter(-1, si, sv)
        return torch.multinomial(torch.softmax(x, dim=-1), 1, generator=gen).squeeze(-1).to(torch.int32)

    @torch.no_grad()
    def generate(self, input_ids=None, attention_mask=None, images=None, max_new_tokens=16, eos_token_id=None,
                 pad_token_id=None, do_sample=False, temperature=1.0, top_k=None, top_p=None, seed=None, num_beams=1,
                 num_return_sequences=1, length_penalty=1.0, early_stopping=False, return_dict_in_generate=False,
                 past_key_values=None, assistant_model=None, num_assistant_tokens=5, repetition_penalty=1.0,
                 no_repeat_ngram_size=0, bad_words_ids=None, suppress_tokens=None, min_new_tokens=0, stop_sequences=None,
                 stopping_criteria=None, speculative_sampling=False, prompt_lookup_num_tokens=None, max_matching_ngram_size=2,
                 constraint=None, constraint_draft_tokens=None, **kwargs):
        """Generation with a KV cache (the reference's eval path calls HF `generate` on the Eval model,
        llava_qwen2_moe.py:629-681; its serving code passes do_sample / temperature / top_p, its eval scripts num_beams).
        Greedy by default; do_sample=True draws from the temperature / top-k / top-p filtered distribution (`seed` makes the
        draw reproducible) and returns num_return_sequences independent continuations per prompt; num_beams > 1 is beam search
        (`_beam_generate`).  Every mode selects its tokens on the device (lmod_row_argmax_bf16 / lmod_sample_bf16 /
        lmod_beam_topk_bf16).  Right-padded prompts: every sample continues from its own length.  Returns the NEW tokens
        [B * num_return_sequences, <= max_new_tokens] (int64; sample b's continuations in rows b*n .. b*n+n-1; positions after a
        sequence's EOS hold pad_token_id); with do_sample and return_dict_in_generate a `SampleOutput` (sequences, token_logprobs).

        past_key_values (a KVCache of an earlier generate() / use_cache forward): continue from it — `input_ids` [B, T] (and an
        optional right-padded attention_mask [B, T]) are the NEW turn only and run through the chunk path (`_append_chunk`) instead
        of a prefill; the turn may bring `images` of its own for its IMAGE_TOKEN_INDEX placeholders; every mode works from there.  The cache holds each position that was fed: the prompt
        and every generated token but each row's last, which a caller chaining turns puts in front of the next turn's tokens.
        With return_dict_in_generate every mode's result carries `past_key_values`.  NOTE, a change of an existing path: greedy
        generate(return_dict_in_generate=True) used to return the bare token tensor and now returns a `GreedyOutput` (sequences,
        past_key_values) — the only way to hand a greedy turn's cache on.  Beam search: the cache holds the B * num_beams RUNNING
        beams in their last step's order; its rows are not the rows of `sequences` (finalized hypotheses, best first), so it
        cannot be chained from without picking rows.  Assisted decoding: when max_new_tokens cuts a round short the target's cache
        holds accepted tokens behind the returned ones.

        assistant_model (with num_assistant_tokens = k in 1..APPEND_T_MAX-1): greedy assisted decoding, `_assisted_generate`.
        With speculative_sampling=True (and do_sample left False) the assisted loop SAMPLES: `_speculative_generate` draws the drafts
        from the assistant's temperature / top_k / top_p warped distribution and verifies them with the speculative-sampling rule
        (lmod_spec_sample_bf16), so the tokens are distributed exactly as generate(do_sample=True) of this model alone; `seed` makes
        the run reproducible.  One sequence per prompt, no beams, no logits processors or stop sequences, no past_key_values;
        speculative_sampling=True without assistant_model raises ValueError.  assistant_model with do_sample=True still raises the
        greedy-only error: folding this mode into do_sample=True is left to a later change that may touch the tests pinning it.

        prompt_lookup_num_tokens = k (1..APPEND_T_MAX-1; HF's name) with max_matching_ngram_size (1..kernels.NGRAM_MAX, HF's default
        2): greedy prompt-lookup decoding, `_prompt_lookup_generate` - the assisted loop without an assistant: every round drafts up
        to k tokens from the continuation of an earlier occurrence of the row's trailing n-gram in its own token history
        (lmod_ngram_draft) and verifies them in one pass.  The tokens are plain greedy's away from argmax ties.  Works with images
        and past_key_values; the history is THIS call's input_ids plus what it generates, earlier turns' tokens are not in it.
        Greedy only, one sequence per prompt; with do_sample, num_beams > 1, num_return_sequences > 1, assistant_model,
        speculative_sampling, a logits processor or a stop argument it raises ValueError.  A call without the argument runs the
        code it ran before.

        Logits processors and stop sequences (HF names and semantics, transformers 5.x; greedy and sampling only — with
        num_beams > 1 or assistant_model any of them raises ValueError), applied on the device every step by
        lmod_logits_process_bf16, in this order, before the token is selected:
          repetition_penalty (> 0): every distinct token of the row's history gets x = x * p if x < 0 else x / p, once;
          no_repeat_ngram_size n: every token that would complete an n-gram already in the history is banned (n = 1: every token
            seen; nothing while the history is shorter than n);
          bad_words_ids (list of token lists) and suppress_tokens (list of ids = one-token bad words): a one-token entry is always
            banned, a longer entry's last token when the history ends with the rest of the entry (and, as in HF, holds at least as
            many tokens as the entry); an entry equal to [eos_token_id] is dropped;
          min_new_tokens: eos_token_id is banned while the row has generated fewer tokens (ignored without an eos_token_id).
        A ban sets the logit to -inf.  A row's history is its live `input_ids` of this call (the first attention_mask.sum()
        positions, ids as given: the negative image placeholder is compared like any integer by the n-gram test and skipped by the
        penalty and the bans) followed by what it has generated in this call; with num_return_sequences > 1 it is replicated as the
        cache is.  stop_sequences (list of token lists): once a row's GENERATED tokens (never the prompt) end with one of them the row
        is done — per row, like EOS: the stop tokens stay, later positions hold pad_token_id, the loop ends when every row is done
        (lmod_gen_push_stop).  stopping_criteria: objects exposing `keyword_ids` (the reference's KeywordsStoppingCriteria); their
        sequences join stop_sequences.  Only that token-level test is reproduced: the class's string-level fallback (decode, then
        substring search) and its all() over the batch are not; anything else raises TypeError.  At most kernels.LOGITS_MAX_SEQS
        sequences of at most kernels.LOGITS_MAX_SEQ_LEN tokens per table, ids in [0, V).  A call that uses none of these arguments
        runs the loop below exactly as before.

        constraint (a `generation.TokenConstraint`: a finite automaton over token ids, e.g. `from_choices` over the option letters
        of a multiple-choice prompt or `from_allowed_tokens`): what a row MAY emit.  Every row carries one int32 state on the
        device; per step lmod_constrain_mask_rows_bf16 sets every logit the state does not allow to -inf - after the processors
        above, HF's position for PrefixConstrainedLogitsProcessor, so sampling draws from, and token_logprobs are under, the
        masked distribution - and lmod_constrain_advance_rows follows the selected token's edge after lmod_gen_push_stop.  EOS
        is allowed in accepting states only; a row that enters a terminal state is finished by that token, as by a stop sequence
        (later positions hold pad_token_id).  Greedy and sampling, num_return_sequences, past_key_values, repetition_penalty and stop
        sequences work with it; num_beams > 1, assistant_model, speculative_sampling, prompt_lookup_num_tokens and the banning
        processors (no_repeat_ngram_size, bad_words_ids, suppress_tokens, min_new_tokens) raise ValueError.  With
        return_dict_in_generate the result carries `constraint_states` (int32 [rows]: the final states).  None: nothing new is
        allocated or launched.

        constraint_draft_tokens = k (1..APPEND_T_MAX-1, with a constraint): greedy constrained decoding that drafts what the
        automaton FORCES, `_constraint_draft_generate`.  Where a state allows a single token (`TokenConstraint.forced`: the rest of
        "tabby cat" after "tabby", the fixed keys of a template) the masked distribution is a point mass, so every round drafts the
        forced run behind the pending token (lmod_constrain_draft, up to k tokens), verifies it in one pass over the weights with
        every verification row masked by its own state, and emits 1 to k + 1 tokens (lmod_constrain_accept).  The tokens and
        `constraint_states` are those of generate(constraint=c) wherever the chunk and the decode path agree on the masked argmax
        (away from ties).  Works with images and past_key_values; with return_dict_in_generate an `AssistedOutput` that carries
        `constraint_states`.  Greedy only, one sequence per prompt: do_sample, num_beams > 1, num_return_sequences > 1,
        assistant_model, speculative_sampling, prompt_lookup_num_tokens, repetition_penalty, stop_sequences and stopping_criteria
        raise ValueError with it, and so does the argument without a constraint.  None: nothing new is allocated or launched."""
        from ...generation import check_logits_args
        if constraint is not None:
            from ...generation import check_constraint_args
            check_constraint_args(constraint, self.lm_head.weight.shape[0], num_beams, assistant_model, prompt_lookup_num_tokens,
                                  speculative_sampling, no_repeat_ngram_size, bad_words_ids, suppress_tokens, min_new_tokens)
        if constraint_draft_tokens is not None:
            from ...generation import check_constraint_draft_args
            check_constraint_draft_args(constraint_draft_tokens, constraint, K.APPEND_T_MAX, do_sample, num_beams, num_return_sequences,
                                        assistant_model, speculative_sampling, prompt_lookup_num_tokens, repetition_penalty,
                                        stop_sequences, stopping_criteria)
            return self._constraint_draft_generate(input_ids, attention_mask, images, max_new_tokens, eos_token_id, pad_token_id,
                                                   constraint, constraint_draft_tokens, return_dict_in_generate, past_key_values)
        if prompt_lookup_num_tokens is not None:
            from ...generation import check_prompt_lookup_args
            check_prompt_lookup_args(prompt_lookup_num_tokens, max_matching_ngram_size, K.APPEND_T_MAX, K.NGRAM_MAX, do_sample, num_beams,
                                     num_return_sequences, assistant_model, speculative_sampling,
                                     repetition_penalty=repetition_penalty, no_repeat_ngram_size=no_repeat_ngram_size,
                                     bad_words_ids=bad_words_ids, suppress_tokens=suppress_tokens, min_new_tokens=min_new_tokens,
                                     stop_sequences=stop_sequences, stopping_criteria=stopping_criteria)
            return self._prompt_lookup_generate(input_ids, attention_mask, images, max_new_tokens, eos_token_id, pad_token_id,
                                                prompt_lookup_num_tokens, max_matching_ngram_size, return_dict_in_generate,
                                                past_key_values)
        if speculative_sampling:
            from ...generation import check_spec_sample_args
            if assistant_model is None:
                raise ValueError("speculative_sampling=True needs an assistant_model to draft for this model")
            check_spec_sample_args(num_beams, num_assistant_tokens, K.APPEND_T_MAX, num_return_sequences, temperature, top_k, top_p,
                                   do_sample, repetition_penalty=repetition_penalty, no_repeat_ngram_size=no_repeat_ngram_size,
                                   bad_words_ids=bad_words_ids, suppress_tokens=suppress_tokens, min_new_tokens=min_new_tokens,
                                   stop_sequences=stop_sequences, stopping_criteria=stopping_criteria)
            return self._speculative_generate(input_ids, attention_mask, images, max_new_tokens, eos_token_id, pad_token_id,
                                              assistant_model, num_assistant_tokens, temperature, top_k, top_p, seed,
                                              return_dict_in_generate, past_key_values)
        lplan = check_logits_args(repetition_penalty, no_repeat_ngram_size, bad_words_ids, suppress_tokens, min_new_tokens,
                                  stop_sequences, stopping_criteria, eos_token_id, self.lm_head.weight.shape[0], num_beams,
                                  assistant_model)
        if assistant_model is not None:
            from ...generation import check_assisted_args
            check_assisted_args(do_sample, num_beams, num_assistant_tokens, K.APPEND_T_MAX, num_return_sequences)
            return self._assisted_generate(input_ids, attention_mask, images, max_new_tokens, eos_token_id, pad_token_id,
                                           assistant_model, num_assistant_tokens, return_dict_in_generate, past_key_values)
        if num_beams != 1:
            return self._beam_generate(input_ids, attention_mask, images, max_new_tokens, eos_token_id, pad_token_id, do_sample,
                                       num_beams, num_return_sequences, length_penalty, early_stopping, return_dict_in_generate,
                                       past_key_values)
        from ...generation import GreedyOutput, SampleOutput, check_sample_args
        check_sample_args(do_sample, temperature, top_k, top_p, num_return_sequences)
        if lplan is not None or constraint is not None:
            if lplan is None:
                from ...generation import LogitsPlan
                lplan = LogitsPlan(1.0, 0, [], 0, [])              # no processor, no stop sequence: the constraint alone
            return self._processed_generate(lplan, input_ids, attention_mask, images, max_new_tokens, eos_token_id, pad_token_id,
                                            do_sample, temperature, top_k, top_p, seed, num_return_sequences,
                                            return_dict_in_generate, past_key_values, constraint)
        n = num_return_sequences
        on_device = do_sample and self.sample_on_device
        was_training = self.training
        self.eval()
        cache, logits = self._start(input_ids, attention_mask, images, max_new_tokens, past_key_values)
        B, dev = logits.shape[0], logits.device
        if n > 1:
            # one prefill at B rows, its cache replicated into B*n rows (as the beams of _beam_generate)
            cfg = self.config
            pcache, cache = cache, KVCache(cfg.num_hidden_layers, B * n, cache.smax, cfg.num_key_value_heads * cfg.head_dim, dev)
            cache.lens.copy_(pcache.lens.repeat_interleave(n))
            K.kv_gather_rows(cache.tensors(), pcache.tensors(), torch.arange(B * n, device=dev, dtype=torch.int32) // n, cache.lens)
            del pcache
            logits = logits.repeat_interleave(n, 0)
            B = B * n
        pad = eos_token_id if pad_token_id is None else pad_token_id
        done = torch.zeros(B, dtype=torch.bool, device=dev)
        gen = None
        if do_sample:
            gen = torch.Generator(device=dev)
            # no `seed`: DRAW one from the global generator (deterministic under torch.manual_seed) — never reseed it: torch.seed()
            # would change torch.initial_seed(), from which the MoE layers derive their gating-noise stream, so a sampling
            # generate() between two training steps would silently fork the training run
            gen.manual_seed(int(seed) if seed is not None else int(torch.randint(0, 2 ** 31 - 1, (1,)).item()))
        want_lp = on_device and return_dict_in_generate
        out, lps = [], []
        for step in range(max_new_tokens):
            if on_device:
                # one uniform per row; the draw, its filter and its statistics are lmod_sample_bf16
                u = torch.rand(B, generator=gen, device=dev)
                nxt = K.sample(logits, u, temperature, top_k, top_p, stats=want_lp)
                if want_lp:
                    nxt, st = nxt
                    # log p(token) under the warped distribution: x[t] - lse - log(kept fraction); a gather of B logits
                    x = logits.gather(1, nxt.long()[:, None]).squeeze(1).double() / max(float(temperature), 1e-6)
                    lp = (x - st[:, 0].double() - torch.log(st[:, 1].double())).clamp(max=0.0).float()
                    lps.append(torch.where(done, torch.zeros_like(lp), lp))
            else:
                nxt = self._sample(logits, temperature, top_k, top_p, gen) if do_sample else K.row_argmax(logits)
            tok = nxt.long()
            if eos_token_id is not None:
                tok = torch.where(done, torch.full_like(tok, pad if pad is not None else 0), tok)
                done = done | (tok == eos_token_id)
            out.append(tok)
            if step + 1 == max_new_tokens or (eos_token_id is not None and bool(done.all())):
                break
            logits = self._decode_step(nxt, cache)
        self.train(was_training)
        seq = torch.stack(out, 1)
        if do_sample and return_dict_in_generate:
            return SampleOutput(seq, torch.stack(lps, 1) if lps else None, cache)
        return GreedyOutput(seq, cache) if return_dict_in_generate else seq

    @torch.no_grad()
    def _processed_generate(self, lplan, input_ids, attention_mask, images, max_new_tokens, eos_token_id, pad_token_id, do_sample,
                            temperature, top_k, top_p, seed, n, return_dict_in_generate, past, constraint=None):
        """Greedy / sampling generate() with logits processors and stop sequences (`lplan`, generation.check_logits_args).  The
        token history [rows, prompt + max_new_tokens], its counters and the done flags live on the device, allocated once; per
        step: lmod_logits_process_bf16 in place on the step's logits (when a processor is active), the usual selection
        (lmod_row_argmax_bf16 / lmod_sample_bf16), lmod_gen_push_stop (pad, history append, EOS and stop-sequence test), one
        read-back of the done flags, one decode step.  `logits_glue` (measurement only, tools/bench_generate.py --processors): a
        pair of torch functions (process, push) that stand in for the two kernels, the A/B baseline as `sample_on_device` is.
        constraint (a generation.TokenConstraint): its tables go to the device once, every row's state is one int32 [rows] that
        starts at `constraint.start`; lmod_constrain_mask_rows_bf16 runs last before the selection and
        lmod_constrain_advance_rows right after lmod_gen_push_stop - no read-back and no host -> device copy of their own."""
        from ...generation import GreedyOutput, SampleOutput
        glue = getattr(self, "logits_glue", None)
        on_device = do_sample and self.sample_on_device
        was_training = self.training
        self.eval()
        try:
            cache, logits = self._start(input_ids, attention_mask, images, max_new_tokens, past)
            B, dev = logits.shape[0], logits.device
            ids = input_ids.to(device=dev, dtype=torch.int32)
            S = ids.shape[1]
            n_prompt = (attention_mask.to(dev).to(torch.int32).sum(1).to(torch.int32) if attention_mask is not None
                        else torch.full((B,), S, device=dev, dtype=torch.int32))
            hist = torch.zeros((B, S + max_new_tokens), device=dev, dtype=torch.int32)
            hist[:, :S] = ids
            ctab = cstate = None
            if constraint is not None:
                ctab = K.constraint_table(constraint, dev)
                cstate = torch.full((B,), constraint.start, device=dev, dtype=torch.int32)
            if n > 1:
                cfg = self.config
                pcache, cache = cache, KVCache(cfg.num_hidden_layers, B * n, cache.smax, cfg.num_key_value_heads * cfg.head_dim, dev)
                cache.lens.copy_(pcache.lens.repeat_interleave(n))
                K.kv_gather_rows(cache.tensors(), pcache.tensors(), torch.arange(B * n, device=dev, dtype=torch.int32) // n, cache.lens)
                del pcache
                logits, hist, n_prompt = logits.repeat_interleave(n, 0), hist.repeat_interleave(n, 0), n_prompt.repeat_interleave(n)
                if cstate is not None:
                    cstate = cstate.repeat_interleave(n).contiguous()
                B = B * n
            hist, n_prompt = hist.contiguous(), n_prompt.contiguous()
            n_hist, n_gen = n_prompt.clone(), torch.zeros(B, device=dev, dtype=torch.int32)
            done = torch.zeros(B, device=dev, dtype=torch.int32)
            bad, stop = K.seq_table(lplan.bad, dev), K.seq_table(lplan.stops, dev)
            pad = eos_token_id if pad_token_id is None else pad_token_id
            can_stop = eos_token_id is not None or stop is not None or (constraint is not None and constraint.has_terminal)
            gen = None
            if do_sample:
                gen = torch.Generator(device=dev)
                gen.manual_seed(int(seed) if seed is not None else int(torch.randint(0, 2 ** 31 - 1, (1,)).item()))   # as generate()
            want_lp = on_device and return_dict_in_generate
            out, lps = [], []
            for step in range(max_new_tokens):
                if lplan.process and glue is None:
                    K.logits_process_(logits, hist, n_hist, n_gen, lplan.penalty, lplan.ngram, bad, lplan.min_new, eos_token_id)
                elif lplan.process:
                    logits = glue[0](logits, hist, n_hist, n_gen, penalty=lplan.penalty, ngram=lplan.ngram, bad=lplan.bad,
                                     min_new=lplan.min_new, eos=eos_token_id)
                if ctab is not None:
                    K.constrain_mask_(logits, cstate, ctab, eos_token_id)
                if on_device:
                    u = torch.rand(B, generator=gen, device=dev)
                    nxt = K.sample(logits, u, temperature, top_k, top_p, stats=want_lp)
                    if want_lp:
                        nxt, st = nxt
                        x = logits.gather(1, nxt.long()[:, None]).squeeze(1).double() / max(float(temperature), 1e-6)
                        lp = (x - st[:, 0].double() - torch.log(st[:, 1].double())).clamp(max=0.0).float()
                        lps.append(torch.where(done != 0, torch.zeros_like(lp), lp))
                else:
                    nxt = self._sample(logits, temperature, top_k, top_p, gen) if do_sample else K.row_argmax(logits)
                if glue is None:
                    K.gen_push_stop_(nxt, done, hist, n_hist, n_prompt, n_gen, eos_token_id, pad, stop)
                else:
                    nxt, done, hist, n_hist, n_gen = glue[1](nxt, done, hist, n_hist, n_prompt, n_gen, eos_token_id, pad, lplan.stops)
                if ctab is not None:
                    K.constrain_advance_(nxt, done, cstate, ctab)
                out.append(nxt.long())
                if step + 1 == max_new_tokens or (can_stop and bool(done.all())):
                    break
                logits = self._decode_step(nxt, cache)
        finally:
            self.train(was_training)
        seq = torch.stack(out, 1)
        if do_sample and return_dict_in_generate:
            return SampleOutput(seq, torch.stack(lps, 1) if lps else None, cache, cstate)
        return GreedyOutput(seq, cache, cstate) if return_dict_in_generate else seq

    # ---- continuous batching -------------------------------------------------------------------------------------------
    @torch.no_grad()
    def generate_batch(self, requests, max_batch_size=8, max_new_tokens=16, eos_token_id=None, pad_token_id=None, do_sample=False,
                       temperature=1.0, top_k=None, top_p=None, seed=None, num_beams=1, num_return_sequences=1,
                       return_dict_in_generate=False, past_key_values=None, assistant_model=None, repetition_penalty=1.0,
                       no_repeat_ngram_size=0, bad_words_ids=None, suppress_tokens=None, min_new_tokens=0, stop_sequences=None,
                       stopping_criteria=None, prompt_lookup_num_tokens=None, max_matching_ngram_size=None, constraint=None):
        """Greedy / sampling generation over a LIST of requests with continuous batching: `max_batch_size` slots decode together and
        a slot whose request has ended (EOS, a stop sequence, its max_new_tokens) is refilled with the next request's freshly
        prefilled prompt before the next step, while the other slots keep decoding — `generate()` over a batch runs every row until
        its longest one ends and cannot take a new prompt in.

        requests: a list of dicts — `input_ids` [S_i] (1-D), optional `images` ([n, 3, H, W] or [3, H, W]: the request's own images),
        optional `max_new_tokens` (default: the call's).  The greedy and sampling arguments of `generate()` apply to the whole call,
        with the same checks and semantics (eos_token_id, pad_token_id, do_sample / temperature / top_k / top_p / seed,
        stop_sequences / stopping_criteria, repetition_penalty, no_repeat_ngram_size, bad_words_ids, suppress_tokens,
        min_new_tokens); num_beams > 1, assistant_model, num_return_sequences > 1 and past_key_values raise ValueError.  Returns a
        list, in request order, of 1-D int64 tensors: each request's new tokens, cut after its EOS / stop sequence, no padding; with
        return_dict_in_generate a `BatchOutput` (sequences, token_logprobs when sampling, the scheduler's counters).

        Allocated once: one slot KVCache of max_batch_size rows, the token history / counters / done flags of
        `_processed_generate`, a request id per slot and a [max_batch_size, V] logits buffer; the cache is sized for the largest
        prompt-plus-budget of the list (it grows only if a prefill splices a prompt longer than predicted).  Per step
        (generation.SlotScheduler decides who sits where; all free slots are filled, in request order, before every step):
          admit  `_start` on the admitted prompts alone (their own batch size, right-padded) into a temporary cache, one
                 lmod_kv_admit_rows (every layer's K and V into the slots' rows), one lmod_slot_admit (history, counters, done,
                 cache length, request id), an indexed copy of the prefill's last-position logits into the slots' logits rows;
          step   over all max_batch_size rows: lmod_logits_process_bf16 (when a processor is active), the selection
                 (lmod_row_argmax_bf16, or lmod_request_uniform + lmod_sample_bf16), lmod_gen_push_stop, one read-back (tokens,
                 done flags, log-probabilities), then one `_decode_step` unless no slot is live.
        The decode step always runs at M = max_batch_size, so a request's arithmetic does not depend on how many slots are live.
        A slot without a request stays done: it emits pad, and its cache length is held where it is (a done row rewrites one dead
        position, so the cache never runs out however long the call lasts).  A request that reaches its own max_new_tokens is
        stopped by the host (`done.copy_`, as the assisted loop does).  Sampling: the uniform of a request's k-th token is
        Philox(seed; request index, k) — the same draw whatever slot the request sits in, whichever requests run beside it and
        whenever it was admitted (`seed` None: drawn from torch's global generator, as generate() does).  The admission prefill is
        not overlapped with decoding: the running slots wait for it.  A MoE model routes the rows of idle slots too (they take expert
        capacity in a decode step, as the finished rows of a generate() batch do).

        Per-request parameters: a request may carry `params`, a `generation.RequestParams` (do_sample, temperature, top_k, top_p,
        seed, repetition_penalty, no_repeat_ngram_size, min_new_tokens, stop_sequences; None = the call's argument), so that a greedy
        request and a temperature / top-p request share a batch.  A request's stop_sequences apply in addition to the call's; one
        with its own seed draws its k-th uniform from Philox(its seed; 0, k) — the same tokens at any list index and in any call;
        bad_words_ids, suppress_tokens, eos_token_id and pad_token_id stay per call.  Such a call runs `_generate_batch_rows`: the
        same loop on the per-row kernels, with a fixed launch count per step whatever the mix, and token_logprobs for every request
        (a greedy token: log-softmax of the processed logits).  A call in which no request has `params` runs the loop below with
        the kernels it always ran.

        prompt_lookup_num_tokens = k (1..APPEND_T_MAX-1) TOGETHER WITH max_matching_ngram_size = n (1..kernels.NGRAM_MAX; there is no
        default here: prompt_lookup_num_tokens alone raises ValueError, as it did before these rounds existed): the same list of requests
        in ROUNDS of prompt-lookup decoding, `_generate_batch_lookup` - every round drafts up to k tokens per slot from the slot's
        own history, verifies all slots in one forward_append and emits 1..k+1 tokens per live slot; every request's tokens are
        plain greedy's on that request alone, away from argmax ties.  Greedy only: do_sample, any logits processor and any request
        with `params` raise ValueError; eos / pad, stop_sequences / stopping_criteria, per-request max_new_tokens and images work as
        above.  The BatchOutput then also carries num_rounds, num_target_forwards and num_accepted; token_logprobs is None.

        constraint (a `generation.TokenConstraint`, as in `generate()`): what every request may emit; a request's own
        `params.constraint` overrides it (None inherits, generation.NO_CONSTRAINT turns it off for that request).  The distinct
        constraints of the call are merged once into one set of tables (`TokenConstraint.merge`); the slot state gains `cstate`
        [max_batch_size] int32 (-1: the slot's request is unconstrained, or the slot was never admitted), written with the
        admitted slots' start states by one indexed copy after an admission.  When the call has any constraint, every step makes the
        same two launches in both loops - lmod_constrain_mask_rows_bf16 before the selection, lmod_constrain_advance_rows after
        the push - whichever requests sit in the slots; without one nothing new is allocated or launched.  A slot finished by a
        terminal state is refilled on the next iteration like one finished by EOS.  With prompt_lookup_num_tokens, or with a banning
        processor in force on a constrained request, it raises ValueError."""
        from ...constants import IMAGE_TOKEN_INDEX
        from ...generation import (BatchOutput, SlotScheduler, check_batch_args, check_batch_constraint_args, check_logits_args,
                                   check_request_params, check_sample_args)
        if prompt_lookup_num_tokens is not None:
            from ...generation import check_batch_lookup_args
            budgets = check_batch_args(requests, max_batch_size, max_new_tokens, num_beams, assistant_model, num_return_sequences,
                                       past_key_values)
            check_batch_lookup_args(requests, prompt_lookup_num_tokens, max_matching_ngram_size, K.APPEND_T_MAX, K.NGRAM_MAX, do_sample,
                                    repetition_penalty=repetition_penalty, no_repeat_ngram_size=no_repeat_ngram_size,
                                    bad_words_ids=bad_words_ids, suppress_tokens=suppress_tokens, min_new_tokens=min_new_tokens)
            check_batch_constraint_args(requests, constraint, self.lm_head.weight.shape[0], prompt_lookup_num_tokens)
            lplan = check_logits_args(stop_sequences=stop_sequences, stopping_criteria=stopping_criteria, eos_token_id=eos_token_id,
                                      vocab_size=self.lm_head.weight.shape[0])
            return self._generate_batch_lookup(requests, budgets, max_batch_size, eos_token_id, pad_token_id,
                                               lplan.stops if lplan is not None else [], prompt_lookup_num_tokens,
                                               max_matching_ngram_size, return_dict_in_generate)
        budgets = check_batch_args(requests, max_batch_size, max_new_tokens, num_beams, assistant_model, num_return_sequences,
                                   past_key_values, prompt_lookup_num_tokens)
        check_sample_args(do_sample, temperature, top_k, top_p, 1)
        V = self.lm_head.weight.shape[0]
        lplan = check_logits_args(repetition_penalty, no_repeat_ngram_size, bad_words_ids, suppress_tokens, min_new_tokens,
                                  stop_sequences, stopping_criteria, eos_token_id, V)
        rplan = check_request_params(requests, do_sample, temperature, top_k, top_p, seed, repetition_penalty, no_repeat_ngram_size,
                                     bad_words_ids, suppress_tokens, min_new_tokens, stop_sequences, stopping_criteria, eos_token_id, V)
        cplan = check_batch_constraint_args(requests, constraint, V, None, no_repeat_ngram_size, bad_words_ids, suppress_tokens,
                                            min_new_tokens)
        if rplan.per_request:
            return self._generate_batch_rows(rplan, requests, budgets, max_batch_size, eos_token_id, pad_token_id, seed,
                                             return_dict_in_generate, cplan)
        sched = SlotScheduler(budgets, max_batch_size)
        if not requests:
            return BatchOutput([], [] if do_sample else None, sched) if return_dict_in_generate else []
        B, dev, cfg = max_batch_size, self.model.embed_tokens.weight.device, self.config
        tower = self.get_image_tower()
        extra = tower.num_patches - 1 if tower is not None else 0                     # an image token becomes num_patches rows
        n_ids = [int(rq["input_ids"].numel()) for rq in requests]
        spliced = [n + (int((rq["input_ids"] == IMAGE_TOKEN_INDEX).sum()) * extra if rq.get("images") is not None else 0)
                   for n, rq in zip(n_ids, requests)]
        i32 = dict(device=dev, dtype=torch.int32)
        st = SimpleNamespace(
            cache=KVCache(cfg.num_hidden_layers, B, max(s + m for s, m in zip(spliced, budgets)),
                          cfg.num_key_value_heads * cfg.head_dim, dev),
            hist=torch.zeros((B, -(-max(n + m for n, m in zip(n_ids, budgets)) // 4) * 4), **i32),   # rows of whole 16-byte vectors
            n_prompt=torch.zeros(B, **i32), n_hist=torch.zeros(B, **i32), n_gen=torch.zeros(B, **i32),
            done=torch.ones(B, **i32), req_id=torch.full((B,), -1, **i32),
            logits=torch.zeros((B, V), device=dev, dtype=BF16))
        st.tab = K.ptr_table(st.cache.tensors())
        bad = K.seq_table(lplan.bad, dev) if lplan is not None else None
        stop = K.seq_table(lplan.stops, dev) if lplan is not None else None
        process = lplan is not None and lplan.process
        ctab = None
        if cplan is not None:
            ctab, st.cstate = K.constraint_table(cplan.merged, dev), torch.full((B,), -1, **i32)
        pad = eos_token_id if pad_token_id is None else pad_token_id
        if do_sample:
            seed = int(seed) if seed is not None else int(torch.randint(0, 2 ** 31 - 1, (1,)).item())        # as generate()
            u = torch.empty(B, device=dev, dtype=torch.float32)
        want_lp = do_sample and return_dict_in_generate
        out, lps = [[] for _ in requests], [[] for _ in requests]
        was_training = self.training
        self.eval()
        try:
            while not sched.finished:
                admitted = sched.admit()
                for with_images in (False, True):                # text-only and image requests splice differently: one prefill each
                    group = [(r, s) for r, s in admitted if (requests[r].get("images") is not None) == with_images]
                    if group:
                        self._admit(requests, budgets, group, st)
                if ctab is not None and admitted:
                    meta = torch.tensor([[s for _, s in admitted], [cplan.starts[r] for r, _ in admitted]], dtype=torch.int32).to(dev)
                    st.cstate[meta[0]] = meta[1]                 # int32 indices: no cast launch
                if process:
                    K.logits_process_(st.logits, st.hist, st.n_hist, st.n_gen, lplan.penalty, lplan.ngram, bad, lplan.min_new,
                                      eos_token_id)
                if ctab is not None:
                    K.constrain_mask_(st.logits, st.cstate, ctab, eos_token_id)
                if do_sample:
                    K.request_uniform(seed, st.req_id, st.n_gen, out=u)
                    nxt = K.sample(st.logits, u, temperature, top_k, top_p, stats=want_lp)
                    if want_lp:
                        # log p(token) under the warped distribution, as generate(): x[t] - lse - log(kept fraction)
                        nxt, stats = nxt
                        x = st.logits.gather(1, nxt.long()[:, None]).squeeze(1).double() / max(float(temperature), 1e-6)
                        lp = (x - stats[:, 0].double() - torch.log(stats[:, 1].double())).clamp(max=0.0).float()
                else:
                    nxt = K.row_argmax(st.logits)
                K.gen_push_stop_(nxt, st.done, st.hist, st.n_hist, st.n_prompt, st.n_gen, eos_token_id, pad, stop)
                if ctab is not None:
                    K.constrain_advance_(nxt, st.done, st.cstate, ctab)
                blk = torch.stack([nxt, st.done] + ([lp.view(torch.int32)] if want_lp else [])).cpu()       # the step's one read-back
                live = sched.live
                for s, r in live.items():
                    out[r].append(int(blk[0, s]))
                    if want_lp:
                        lps[r].append(blk[2, s])
                stopped = [s for s in live if int(blk[1, s]) != 0]
                by_budget = [s for _, s in sched.step(stopped) if s not in stopped]
                if by_budget:                                    # the host's stop reaches the device flag
                    flags = blk[1].clone()
                    flags[by_budget] = 1
                    st.done.copy_(flags)
                if sched.live:
                    st.logits.copy_(self._decode_step(nxt, st.cache))
                    st.cache.lens.sub_(st.done)                  # a done row stays at its position: it rewrites one dead entry
        finally:
            self.train(was_training)
        n_out = [len(o) for o in out]
        seqs = list(torch.tensor([t for o in out for t in o], dtype=torch.int64).to(dev).split(n_out))
        if not return_dict_in_generate:
            return seqs
        logprobs = None
        if do_sample:
            flat = torch.stack([v for o in lps for v in o]) if sum(n_out) else torch.zeros(0, dtype=torch.int32)
            logprobs = list(flat.view(torch.float32).to(dev).split(n_out))
        return BatchOutput(seqs, logprobs, sched)

    @torch.no_grad()
    def _generate_batch_rows(self, rplan, requests, budgets, max_batch_size, eos_token_id, pad_token_id, seed, return_dict_in_generate,
                             cplan=None):
        """generate_batch when some request carries `params` (`rplan`: generation.check_request_params).  The loop, the scheduler, the
        admission and the state are generate_batch's; the slots' parameters live in one field-major device table [fields, B] int32
        (floats bit-cast; generation.RequestPlan.TABLE_FIELDS), every field a contiguous [B] array that the per-row kernels read:
          admit  as generate_batch, then the admitted slots' table entries: one host -> device copy (indices and values), one
                 indexed copy; a slot that was never admitted holds the neutral values (greedy, penalty 1, no n-gram, no stops);
          step   lmod_logits_process_rows_bf16 (when any request or the call uses a processor), lmod_request_uniform_rows (when any
                 request samples), lmod_sample_rows_bf16 (always its six launches: greedy rows are its argmax rows),
                 lmod_gen_push_stop_rows, the read-back, the decode step.
        The launches of a step depend on the call (`rplan`'s three flags), never on which requests sit in the slots.  The
        log-probability of a token: x[t] / T - lse - log(kept fraction) under the row's own warp; a greedy row has T = 1 and keeps
        everything, so its entry is x[t] - logsumexp(x) of the processed logits.
        cplan (generation.ConstraintPlan; None: nothing below exists): the slots' automaton states `cstate` [B] int32 sit in the same
        allocation behind the table (an array of their own, not a table column; -1 until a constrained request is admitted), so
        the admitted slots' start states travel in the admission's one host -> device copy and land with its one indexed copy;
        every step then runs lmod_constrain_mask_rows_bf16 after the processors and lmod_constrain_advance_rows after the push."""
        from ...constants import IMAGE_TOKEN_INDEX
        from ...generation import BatchOutput, RequestPlan, SlotScheduler
        sched = SlotScheduler(budgets, max_batch_size)
        V = self.lm_head.weight.shape[0]
        B, dev, cfg = max_batch_size, self.model.embed_tokens.weight.device, self.config
        tower = self.get_image_tower()
        extra = tower.num_patches - 1 if tower is not None else 0
        n_ids = [int(rq["input_ids"].numel()) for rq in requests]
        spliced = [n + (int((rq["input_ids"] == IMAGE_TOKEN_INDEX).sum()) * extra if rq.get("images") is not None else 0)
                   for n, rq in zip(n_ids, requests)]
        i32 = dict(device=dev, dtype=torch.int32)
        st = SimpleNamespace(
            cache=KVCache(cfg.num_hidden_layers, B, max(s + m for s, m in zip(spliced, budgets)),
                          cfg.num_key_value_heads * cfg.head_dim, dev),
            hist=torch.zeros((B, -(-max(n + m for n, m in zip(n_ids, budgets)) // 4) * 4), **i32),
            n_prompt=torch.zeros(B, **i32), n_hist=torch.zeros(B, **i32), n_gen=torch.zeros(B, **i32),
            done=torch.ones(B, **i32), req_id=torch.full((B,), -1, **i32),
            logits=torch.zeros((B, V), device=dev, dtype=BF16))
        st.tab = K.ptr_table(st.cache.tensors())
        ctab = cstate = None
        if cplan is None:
            table = torch.tensor(RequestPlan.neutral_table(B), dtype=torch.int32).to(dev)
        else:
            n_tab = RequestPlan.TABLE_ROWS * B
            buf = torch.tensor([v for r in RequestPlan.neutral_table(B) for v in r] + [-1] * B, dtype=torch.int32).to(dev)
            table, cstate, ctab = buf[:n_tab].view(RequestPlan.TABLE_ROWS, B), buf[n_tab:], K.constraint_table(cplan.merged, dev)
        row = RequestPlan.row_of
        p_seed = table[0:2].view(-1).view(torch.int64)                                # [B] 64-bit keys
        p_ctr0, p_greedy, p_topk = table[row("ctr0")], table[row("greedy")], table[row("top_k")]
        p_temp, p_topp = table[row("temperature")].view(torch.float32), table[row("top_p")].view(torch.float32)
        p_pen, p_ngram, p_minnew = table[row("penalty")].view(torch.float32), table[row("ngram")], table[row("min_new")]
        p_first, p_count = table[row("stop_first")], table[row("stop_count")]
        bad, stop = K.seq_table(rplan.bad, dev), K.seq_table(rplan.stops, dev)
        pad = eos_token_id if pad_token_id is None else pad_token_id
        if rplan.needs_call_seed:
            seed = int(seed) if seed is not None else int(torch.randint(0, 2 ** 31 - 1, (1,)).item())        # as generate()
        u = torch.zeros(B, device=dev, dtype=torch.float32)
        out, lps = [[] for _ in requests], [[] for _ in requests]
        was_training = self.training
        self.eval()
        try:
            while not sched.finished:
                admitted = sched.admit()
                for with_images in (False, True):
                    group = [(r, s) for r, s in admitted if (requests[r].get("images") is not None) == with_images]
                    if group:
                        self._admit(requests, budgets, group, st)
                if admitted and ctab is None:
                    cols = torch.tensor(rplan.columns(admitted, B, seed), dtype=torch.int32).to(dev)
                    table.view(-1)[cols[0]] = cols[1]                      # int32 indices: no cast launch
                elif admitted:
                    idx, val = rplan.columns(admitted, B, seed)
                    cols = torch.tensor([idx + [n_tab + s for _, s in admitted], val + [cplan.starts[r] for r, _ in admitted]],
                                        dtype=torch.int32).to(dev)
                    buf[cols[0]] = cols[1]                                 # the table entries and the start states, one copy
                if rplan.any_process:
                    K.logits_process_rows_(st.logits, st.hist, st.n_hist, st.n_gen, p_pen, p_ngram, p_minnew, rplan.any_penalty, bad,
                                           eos_token_id)
                if ctab is not None:
                    K.constrain_mask_(st.logits, cstate, ctab, eos_token_id)
                if rplan.any_sample:
                    K.request_uniform_rows(p_seed, p_ctr0, st.n_gen, out=u)
                nxt, stats = K.sample_rows(st.logits, u, p_temp, p_topk, p_topp, p_greedy, stats=True)
                x = st.logits.gather(1, nxt.long()[:, None]).squeeze(1).double() / p_temp.clamp_min(1e-6).double()
                lp = (x - stats[:, 0].double() - torch.log(stats[:, 1].double())).clamp(max=0.0).float()
                K.gen_push_stop_rows_(nxt, st.done, st.hist, st.n_hist, st.n_prompt, st.n_gen, eos_token_id, pad, stop,
                                      rplan.n_call_stops, p_first, p_count)
                if ctab is not None:
                    K.constrain_advance_(nxt, st.done, cstate, ctab)
                blk = torch.stack([nxt, st.done, lp.view(torch.int32)]).cpu()                 # the step's one read-back
                live = sched.live
                for s, r in live.items():
                    out[r].append(int(blk[0, s]))
                    lps[r].append(blk[2, s])
                stopped = [s for s in live if int(blk[1, s]) != 0]
                by_budget = [s for _, s in sched.step(stopped) if s not in stopped]
                if by_budget:
                    flags = blk[1].clone()
                    flags[by_budget] = 1
                    st.done.copy_(flags)
                if sched.live:
                    st.logits.copy_(self._decode_step(nxt, st.cache))
                    st.cache.lens.sub_(st.done)
        finally:
            self.train(was_training)
        n_out = [len(o) for o in out]
        seqs = list(torch.tensor([t for o in out for t in o], dtype=torch.int64).to(dev).split(n_out))
        if not return_dict_in_generate:
            return seqs
        flat = torch.stack([v for o in lps for v in o]) if sum(n_out) else torch.zeros(0, dtype=torch.int32)
        return BatchOutput(seqs, list(flat.view(torch.float32).to(dev).split(n_out)), sched)

    @torch.no_grad()
    def _generate_batch_lookup(self, requests, budgets, max_batch_size, eos_token_id, pad_token_id, stops, k, max_ngram,
                               return_dict_in_generate):
        """generate_batch in rounds of prompt-lookup decoding (`generate(prompt_lookup_num_tokens=k)`'s drafter and verification pass
        under generate_batch's scheduler, admission and slot state).  The state is generate_batch's plus `budget` [B] int32 (each
        slot's request's max_new_tokens; admission fills it with one indexed copy), and the slot cache holds k + 1 positions more:
        a verification pass appends k + 1 positions to every row, live or not.  Per iteration, always the same launches whatever
        sits in the slots (generation.LookupSlotScheduler decides who sits where; all free slots are filled in request order first):
          admit   as generate_batch (`_admit`), then the budget copy;
          first   lmod_row_argmax_bf16 over the slots' logits rows, lmod_batch_lookup_first: a freshly admitted slot's first token
                  becomes its pending token (and may already end it: EOS, a one-token stop sequence, a budget of 1);
          draft   lmod_ngram_draft (draft and verification chunk; a done slot drafts nothing);
          verify  the chunk's embeddings, ONE forward_append with T = k + 1 for every slot, the head, lmod_row_argmax_bf16;
          round   lmod_batch_lookup_round: acceptance, emission into the history, EOS / stop sequence / budget possibly in the middle
                  of an accepted run, the cache length (a live slot: the prompt and every emitted token but the last; an idle slot:
                  where it was);
          read    the round's ONE read-back, the [B, k+6] block.
        The host never asks whether a draft exists, copies no done flag and no cache length to the device; it appends each live
        request's first token and emitted tokens, frees the slots the block reports as finished and admits again.  Its upper bound
        of the cache lengths (forward_append's max_len) is exact: the admitted lens plus every round's n_emit.  The logits buffer is
        read only in the iteration after an admission, by the freshly admitted slots.  A MoE model routes the B * (k+1) rows of a
        round - idle slots' rows included - with the eval capacity rule over the rows of that call, as `generate()`'s lookup loop
        does over its B * (k+1).  `assisted_force_accept` (measurement only, as in `_prompt_lookup_generate`) counts every drafted
        token as accepted."""
        from ...constants import IMAGE_TOKEN_INDEX
        from ...generation import BatchOutput, LookupSlotScheduler
        sched = LookupSlotScheduler(budgets, max_batch_size)
        if not requests:
            return BatchOutput([], None, sched, []) if return_dict_in_generate else []
        V = self.lm_head.weight.shape[0]
        B, dev, cfg = max_batch_size, self.model.embed_tokens.weight.device, self.config
        tower = self.get_image_tower()
        extra = tower.num_patches - 1 if tower is not None else 0
        n_ids = [int(rq["input_ids"].numel()) for rq in requests]
        spliced = [n + (int((rq["input_ids"] == IMAGE_TOKEN_INDEX).sum()) * extra if rq.get("images") is not None else 0)
                   for n, rq in zip(n_ids, requests)]
        i32 = dict(device=dev, dtype=torch.int32)
        st = SimpleNamespace(
            cache=KVCache(cfg.num_hidden_layers, B, max(s + m for s, m in zip(spliced, budgets)) + k + 1,
                          cfg.num_key_value_heads * cfg.head_dim, dev),
            hist=torch.zeros((B, -(-max(n + m for n, m in zip(n_ids, budgets)) // 4) * 4), **i32),
            n_prompt=torch.zeros(B, **i32), n_hist=torch.zeros(B, **i32), n_gen=torch.zeros(B, **i32),
            done=torch.ones(B, **i32), req_id=torch.full((B,), -1, **i32), budget=torch.ones(B, **i32),
            logits=torch.zeros((B, V), device=dev, dtype=BF16))
        st.tab = K.ptr_table(st.cache.tensors())
        stop = K.seq_table(stops, dev)
        pad = eos_token_id if pad_token_id is None else pad_token_id
        emb_w = self.model.embed_tokens.weight
        bufs = (torch.empty((B, k), **i32), torch.empty((B, k + 1), **i32), torch.empty(B, **i32))
        first, block = torch.empty(B, **i32), torch.empty((B, k + 6), **i32)
        force = getattr(self, "assisted_force_accept", False)
        lens_h = [0] * B                                         # the host's copy of the slot cache's lens: exact, never read back
        out, accepted = [[] for _ in requests], [0] * len(requests)
        was_training = self.training
        self.eval()
        try:
            while not sched.finished:
                admitted = sched.admit()
                for with_images in (False, True):
                    group = [(r, s) for r, s in admitted if (requests[r].get("images") is not None) == with_images]
                    if group:
                        for s, n in self._admit(requests, budgets, group, st, reserve=k + 1).items():
                            lens_h[s] = n
                if admitted:
                    meta = torch.tensor([[s for _, s in admitted], [budgets[r] for r, _ in admitted]], dtype=torch.int32).to(dev)
                    st.budget[meta[0]] = meta[1]                 # int32 indices: no cast launch
                K.batch_lookup_first_(K.row_argmax(st.logits), st.done, st.hist, st.n_hist, st.n_prompt, st.n_gen, st.budget,
                                      eos_token_id, stop, out=first)
                draft_t, chunk, _ = K.ngram_draft(st.hist, st.n_hist, st.done, k, max_ngram, V, out=bufs)
                if max(lens_h) + k + 1 > st.cache.smax:          # cannot happen with the reservation above; never let the pass regrow
                    st.cache.grow(max(lens_h) + k + 1)
                    st.tab = K.ptr_table(st.cache.tensors())
                hid = self.model.forward_append(K.gather_rows(emb_w, None, chunk.view(-1), emb_w.shape[1]), st.cache, k + 1,
                                                max_len=max(lens_h))
                target = K.row_argmax(ops.linear_fwd(hid, self.head())).view(B, k + 1)
                if force:                                        # measurement only; the -1 fill stays a mismatch
                    target[:, :k] = torch.where(draft_t >= 0, draft_t, target[:, :k])
                K.batch_lookup_round_(draft_t, target, first, st.done, st.hist, st.n_hist, st.n_prompt, st.n_gen, st.budget,
                                      st.cache.lens, eos_token_id, pad, stop, out=block)
                blk = block.cpu().tolist()                       # the round's one read-back
                emitted, ended = {}, []
                for s, r in sched.live.items():
                    row = blk[s]
                    ft, n_acc, ne = row[k + 5], row[k + 1], row[k + 2]
                    if ft >= 0:
                        out[r].append(ft)
                    out[r].extend(row[:ne])
                    accepted[r] += min(n_acc, ne)
                    emitted[s] = int(ft >= 0) + ne
                    lens_h[s] += ne
                    if row[k + 4]:
                        ended.append(s)
                sched.advance(emitted, ended)
        finally:
            self.train(was_training)
        n_out = [len(o) for o in out]
        seqs = list(torch.tensor([t for o in out for t in o], dtype=torch.int64).to(dev).split(n_out))
        return BatchOutput(seqs, None, sched, accepted) if return_dict_in_generate else seqs

    def _admit(self, requests, budgets, group, st, reserve=0):
        """Admission of generate_batch: prefill the requests of `group` ([(request, slot)]) together and move them into their slots
        of the state `st` (the slot cache, the generation state, the logits buffer).  reserve: cache positions a request needs beyond
        prompt + budget (the lookup rounds' k + 1).  Returns {slot: the admitted cache length}: the host's bound needs no read-back
        of its own."""
        dev = st.logits.device
        rs, slots = [r for r, _ in group], [s for _, s in group]
        ids_list = [requests[r]["input_ids"].reshape(-1).to(torch.int64).cpu() for r in rs]
        n = [int(t.numel()) for t in ids_list]
        R, S = len(rs), max(n)
        ids = torch.zeros((R, S), dtype=torch.int64)
        for j, t in enumerate(ids_list):
            ids[j, :n[j]] = t
        mask = torch.arange(S)[None, :] < torch.tensor(n)[:, None]
        images = None
        if requests[rs[0]].get("images") is not None:
            images = torch.cat([im if im.dim() == 4 else im[None] for im in (requests[r]["images"] for r in rs)])
        tcache, lg = self._start(ids, mask, images, 0, None)
        lens_h = tcache.lens.cpu().tolist()
        need = max(l + budgets[r] for l, r in zip(lens_h, rs)) + reserve
        if need > st.cache.smax:                                 # the splice made a prompt longer than predicted
            st.cache.grow(need)
            st.tab = K.ptr_table(st.cache.tensors())
        K.kv_admit_rows(st.cache.tensors(), tcache.tensors(), slots, tcache.lens, max(lens_h),
                        tables=(st.tab, K.ptr_table(tcache.tensors())))
        prompt = torch.zeros((R, -(-S // 4) * 4), dtype=torch.int32)
        prompt[:, :S] = ids.to(torch.int32)
        meta = torch.tensor([n, rs], dtype=torch.int32).to(dev)
        K.slot_admit_(slots, prompt.to(dev), meta[0].contiguous(), tcache.lens, meta[1].contiguous(), st.hist, st.n_prompt, st.n_hist,
                      st.n_gen, st.done, st.cache.lens, st.req_id)
        st.logits[torch.tensor(slots, device=dev)] = lg
        return dict(zip(slots, lens_h))

    @torch.no_grad()
    def _assisted_generate(self, input_ids, attention_mask, images, max_new_tokens, eos_token_id, pad_token_id, draft, k,
                           return_dict_in_generate, past=None):
        """Greedy assisted (speculative) decoding, HF `generate(assistant_model=draft)`: this model is the target, `draft` (same
        tokenizer; e.g. the distilled student) proposes k tokens per round.  Both models prefill the same prompt and images, each
        with its own tower and projector.  Per round: (1) the draft runs its decode steps, argmax on the device; (2) the target runs
        ONE forward_append over [next_token, d_1 .. d_k]; (3) lmod_row_argmax_bf16 over the k+1 logit rows; (4) lmod_spec_accept
        (longest matching prefix, the corrected token, EOS, both caches' lens — a rejected draft costs no copy); (5) the draft
        catches up through its own forward_append with 1 or 2 tokens per sample ([d_k,] next_token — ragged), whose last row also
        gives the next round's first draft token, so later rounds run k-1 draft decode steps.  The host reads one int block
        [B, k+5] back per round (stop test and output).  Both argmaxes run over min(V_draft, V_target) columns, so the draft can
        never hand the target an id it has no embedding for.  The result equals plain greedy of the target wherever the chunk and
        the decode path agree on the argmax (they differ in summation order: away from ties).  A MoE model as target routes the
        B * (k+1) rows of a verification pass with the eval capacity rule over the rows of that call, as a decode step does over
        its B rows.  Returns the new tokens [B, <= max_new_tokens]; with return_dict_in_generate an `AssistedOutput`."""
        from ...generation import AssistedBookkeeper, AssistedOutput
        if past is not None:
            raise ValueError("assistant_model cannot continue from past_key_values: the draft model has no cache of the earlier turns")
        modes = (self.training, draft.training)
        self.eval(), draft.eval()
        try:
            tcache, tlogits = self._start(input_ids, attention_mask, images, max_new_tokens + k + 1, None)
            dcache, _ = draft._start(input_ids, attention_mask, images, max_new_tokens + k + 1, None)
            B, dev = tlogits.shape[0], tlogits.device
            V = min(tlogits.shape[1], draft.lm_head.weight.shape[0])
            book = AssistedBookkeeper(B, k, max_new_tokens, eos_token_id, eos_token_id if pad_token_id is None else pad_token_id)
            nxt = K.row_argmax(tlogits[:, :V])
            done = book.first(nxt).to(device=dev, dtype=torch.int32).contiguous()
            lt_h, ld_h = tcache.lens.cpu().long(), dcache.lens.cpu().long()         # host copies of the caches' lens at round start
            emb_t, emb_d = self.model.embed_tokens.weight, draft.model.embed_tokens.weight
            d_first = None
            trace = getattr(self, "assisted_trace", None)          # measurement only: a list that receives 5 events per round
            mark = (lambda: None) if trace is None else (lambda: (ev.append(torch.cuda.Event(enable_timing=True)), ev[-1].record()))
            while not book.finished:
                ev = []
                mark()
                # the draft's decode steps append by an unchecked indexed copy: make room first (k steps, then a catch-up of <= 2)
                if int(ld_h.max()) + k + 2 > dcache.smax:
                    dcache.grow(int(ld_h.max()) + k + 2 + max_new_tokens)
                tok, drafts = (nxt, []) if d_first is None else (d_first, [d_first])
                while len(drafts) < k:
                    tok = K.row_argmax(draft._decode_step(tok, dcache)[:, :V])
                    drafts.append(tok)
                draft_t = torch.stack(drafts, 1).contiguous()
                mark()
                chunk = torch.cat([nxt[:, None], draft_t], 1).reshape(-1).contiguous()
                hid = self.model.forward_append(K.gather_rows(emb_t, None, chunk, emb_t.shape[1]), tcache, k + 1, max_len=int(lt_h.max()))
                target = K.row_argmax(ops.linear_fwd(hid, self.head())[:, :V]).view(B, k + 1)
                mark()
                if getattr(self, "assisted_force_accept", False):                   # measurement only: every draft counts as accepted
                    target[:, :k] = draft_t
                pad = book.pad
                block, nxt = K.spec_accept(draft_t, target, done, eos_token_id, pad, tcache.lens, dcache.lens)
                blk = block.cpu()                                                   # the round's one read-back
                book.update(blk)
                n_acc = blk[:, k + 1].long()
                mark()
                if book.finished:
                    break
                # a sample the host stopped (max_new_tokens) is done on the device too: it emits nothing and, like an EOS row,
                # advances one position per round while the others finish
                done.copy_(book.stopped.to(torch.int32))
                full = n_acc == k
                # everything the catch-up needs is known from the block: no second read-back
                idx = torch.tensor([2 * b + j for b in range(B) for j in ((0, 1) if bool(full[b]) else (1,))], dtype=torch.long)
                toks = torch.stack([draft_t[:, k - 1], nxt], 1).reshape(-1)[idx.to(dev)].contiguous()
                n_ch = 1 + full.to(torch.int32)
                hid = draft.model.forward_append(K.gather_rows(emb_d, None, toks, emb_d.shape[1]), dcache, n_ch.to(dev), T=2,
                                                 max_len=int((ld_h + torch.clamp(n_acc + 1, max=k)).max()))
                lt_h, ld_h = lt_h + n_acc + 1, ld_h + n_acc + 1
                last = (n_ch.cumsum(0) - 1).to(torch.int32).to(dev)
                hl = K.gather_rows(hid, None, last, hid.shape[1])
                d_first = K.row_argmax(ops.linear_fwd(hl, draft.head())[:, :V])
                mark()
                if trace is not None:
                    trace.append(ev)
        finally:
            self.train(modes[0]), draft.train(modes[1])
        seq = book.sequences().to(dev)
        if return_dict_in_generate:
            return AssistedOutput(seq, book.num_rounds, 1 + book.num_rounds, book.num_accepted.to(dev), tcache)
        return seq

    @torch.no_grad()
    def _prompt_lookup_generate(self, input_ids, attention_mask, images, max_new_tokens, eos_token_id, pad_token_id, k, max_ngram,
                                return_dict_in_generate, past=None):
        """Greedy prompt-lookup decoding, HF `generate(prompt_lookup_num_tokens=k, max_matching_ngram_size=max_ngram)`: the assisted
        loop whose draft is the row's own token history, so there is no second model, no draft cache and no catch-up.  The history
        [B, S + max_new_tokens + k + 1] lives on the device as `_processed_generate` builds it: this call's `input_ids`, live tokens
        only (right-padded; ids as given, an image placeholder is one negative id), then the first argmax and whatever is emitted.
        With `past` the earlier turns' tokens are NOT in it: only this turn can be looked up.  Per round, always the same launches:
        (1) lmod_ngram_draft (draft, verification chunk); (2) the chunk's embeddings; (3) ONE forward_append with T = k + 1 for every
        row, whether it has a draft or not; (4) the head; (5) lmod_row_argmax_bf16; (6) lmod_spec_accept (the -1 behind a short draft
        never matches, the repeated pending token behind it is rejected and rewound like any rejected draft; `lens_draft` is a
        scratch nothing reads); (7) lmod_hist_push_block; (8) the round's one read-back, the [B, k+5] block.  The host never asks
        whether a draft exists.  A sample the host stops at max_new_tokens is marked done on the device; after every round the
        cache's lens are set from the host's count to prompt + emitted tokens - 1 (the device's value wherever the round was not cut
        by EOS or max_new_tokens), so a finished row rewrites the same dead positions while the others go on and the returned cache
        holds, as plain greedy's does, the prompt and every returned token but each row's last.  The result equals plain greedy
        wherever the chunk and the decode path agree on the argmax (away from ties).  A MoE model routes the B * (k+1) rows of a
        round with the eval capacity rule over the rows of that call.  `assisted_trace` (measurement only) receives 4 events per
        round: start, after the draft, after the verification pass and its argmax, after accept / push / read-back;
        `assisted_force_accept` (measurement only) counts every drafted token as accepted.  Returns the new tokens
        [B, <= max_new_tokens]; with return_dict_in_generate an `AssistedOutput`."""
        from ...generation import AssistedBookkeeper, AssistedOutput
        was_training = self.training
        self.eval()
        try:
            cache, logits = self._start(input_ids, attention_mask, images, max_new_tokens + k + 1, past)
            B, dev = logits.shape[0], logits.device
            V = logits.shape[1]
            book = AssistedBookkeeper(B, k, max_new_tokens, eos_token_id, eos_token_id if pad_token_id is None else pad_token_id)
            nxt = K.row_argmax(logits)
            done = book.first(nxt).to(device=dev, dtype=torch.int32).contiguous()
            ids = input_ids.to(device=dev, dtype=torch.int32)
            S = ids.shape[1]
            n_prompt = (attention_mask.to(dev).to(torch.int32).sum(1) if attention_mask is not None
                        else torch.full((B,), S, device=dev, dtype=torch.int32))
            hist = torch.zeros((B, S + max_new_tokens + k + 1), device=dev, dtype=torch.int32)
            hist[:, :S] = ids
            hist.scatter_(1, n_prompt.long()[:, None], nxt[:, None])                   # the pending token ends the history
            n_hist = (n_prompt + 1).to(torch.int32).contiguous()
            len0 = cache.lens.cpu().long()                                              # cache positions before the first new token
            lt_h = len0.clone()
            emb_w = self.model.embed_tokens.weight
            bufs = (torch.empty((B, k), device=dev, dtype=torch.int32), torch.empty((B, k + 1), device=dev, dtype=torch.int32),
                    torch.empty(B, device=dev, dtype=torch.int32))
            lens_scratch = torch.zeros(B, device=dev, dtype=torch.int32)
            force = getattr(self, "assisted_force_accept", False)
            trace = getattr(self, "assisted_trace", None)
            mark = (lambda: None) if trace is None else (lambda: (ev.append(torch.cuda.Event(enable_timing=True)), ev[-1].record()))
            while not book.finished:
                ev = []
                mark()
                draft_t, chunk, _ = K.ngram_draft(hist, n_hist, done, k, max_ngram, V, out=bufs)
                mark()
                if int(lt_h.max()) + k + 1 > cache.smax:
                    cache.grow(int(lt_h.max()) + k + 1 + max_new_tokens)
                hid = self.model.forward_append(K.gather_rows(emb_w, None, chunk.view(-1), emb_w.shape[1]), cache, k + 1,
                                                max_len=int(lt_h.max()))
                target = K.row_argmax(ops.linear_fwd(hid, self.head())).view(B, k + 1)
                mark()
                if force:                                                               # measurement only; the -1 fill stays a mismatch
                    target[:, :k] = torch.where(draft_t >= 0, draft_t, target[:, :k])
                block, nxt = K.spec_accept(draft_t, target, done, eos_token_id, book.pad, cache.lens, lens_scratch)
                K.hist_push_block_(block, k, hist, n_hist)
                book.update(block.cpu())                                                # the round's one read-back
                mark()
                if trace is not None:
                    trace.append(ev)
                # host -> device only: rows the host stopped are done, and every row's cache length is what the host counts
                done.copy_(book.stopped.to(torch.int32))
                lt_h = len0 + book.n - 1
                cache.lens.copy_(lt_h.to(torch.int32))
        finally:
            self.train(was_training)
        seq = book.sequences().to(dev)
        if return_dict_in_generate:
            return AssistedOutput(seq, book.num_rounds, 1 + book.num_rounds, book.num_accepted.to(dev), cache)
        return seq

    @torch.no_grad()
    def _constraint_draft_generate(self, input_ids, attention_mask, images, max_new_tokens, eos_token_id, pad_token_id, constraint, k,
                                   return_dict_in_generate, past=None):
        """Greedy constrained decoding that drafts the tokens the automaton forces, `generate(constraint=c,
        constraint_draft_tokens=k)`: `_prompt_lookup_generate`'s round with the automaton carried through it, so there is no token
        history and no lmod_hist_push_block.  The constraint's tables go to the device once; every row carries one int32 state and
        one int32 count of emitted tokens.  The prefill logits are masked with the start state, then lmod_row_argmax_bf16 and
        lmod_constrain_advance_rows: the first token may already end a row through a terminal state, so the host reads `done` back
        once here.  Per round, always the same launches: (1) lmod_constrain_draft (the forced run behind the pending token, the
        verification chunk, the state of every verification row); (2) the chunk's embeddings; (3) ONE forward_append with
        T = k + 1 for every row, whether it has a draft or not; (4) the head; (5) ONE lmod_constrain_mask_rows_bf16 over the
        B * (k+1) rows with the draft's states (-1 behind a run: those rows are never accepted); (6) lmod_row_argmax_bf16;
        (7) lmod_constrain_accept (the longest matching prefix; every emitted token follows its edge and is cut at EOS, a token
        that leaves the automaton, a terminal state or max_new_tokens; done, state, count and the cache's lens are written there);
        (8) the round's one read-back, the [B, k+5] block.  Nothing goes from the host to the device inside the loop: the device
        cuts, so the cache holds, as plain greedy's does, the prompt and every returned token but each row's last.  The result
        equals generate(constraint=c) wherever the chunk and the decode path agree on the masked argmax (away from ties).  A MoE
        model routes the B * (k+1) rows of a round with the eval capacity rule over the rows of that call.  `assisted_trace`
        (measurement only) receives 4 events per round: start, after the draft, after the verification pass with its mask and
        argmax, after accept / read-back.  Returns the new tokens [B, <= max_new_tokens]; with return_dict_in_generate an
        `AssistedOutput` with `constraint_states`."""
        from ...generation import AssistedBookkeeper, AssistedOutput
        was_training = self.training
        self.eval()
        try:
            cache, logits = self._start(input_ids, attention_mask, images, max_new_tokens + k + 1, past)
            B, dev = logits.shape[0], logits.device
            V = logits.shape[1]
            ctab = K.constraint_table(constraint, dev)
            cstate = torch.full((B,), constraint.start, device=dev, dtype=torch.int32)
            book = AssistedBookkeeper(B, k, max_new_tokens, eos_token_id, eos_token_id if pad_token_id is None else pad_token_id)
            K.constrain_mask_(logits, cstate, ctab, eos_token_id)
            nxt = K.row_argmax(logits)
            done = book.first(nxt).to(device=dev, dtype=torch.int32).contiguous()
            K.constrain_advance_(nxt, done, cstate, ctab)
            book.stopped |= done.cpu() != 0                                           # a terminal state behind the first token
            done.copy_(book.stopped.to(torch.int32))                                  # ... and max_new_tokens == 1
            n_gen = torch.ones(B, device=dev, dtype=torch.int32)
            len0 = cache.lens.cpu().long()                                              # cache positions before the first new token
            lt_h = len0.clone()
            emb_w = self.model.embed_tokens.weight
            bufs = (torch.empty((B, k), device=dev, dtype=torch.int32), torch.empty((B, k + 1), device=dev, dtype=torch.int32),
                    torch.empty((B, k + 1), device=dev, dtype=torch.int32), torch.empty(B, device=dev, dtype=torch.int32))
            trace = getattr(self, "assisted_trace", None)
            mark = (lambda: None) if trace is None else (lambda: (ev.append(torch.cuda.Event(enable_timing=True)), ev[-1].record()))
            while not book.finished:
                ev = []
                mark()
                draft_t, chunk, vstate, _ = K.constrain_draft(nxt, cstate, done, ctab, k, eos_token_id, V, out=bufs)
                mark()
                if int(lt_h.max()) + k + 1 > cache.smax:
                    cache.grow(int(lt_h.max()) + k + 1 + max_new_tokens)
                hid = self.model.forward_append(K.gather_rows(emb_w, None, chunk.view(-1), emb_w.shape[1]), cache, k + 1,
                                                max_len=int(lt_h.max()))
                vlogits = K.constrain_mask_(ops.linear_fwd(hid, self.head()), vstate.view(-1), ctab, eos_token_id)
                target = K.row_argmax(vlogits).view(B, k + 1)
                mark()
                block, nxt = K.constrain_accept(draft_t, target, done, cstate, ctab, eos_token_id, book.pad, n_gen, max_new_tokens,
                                                cache.lens)
                book.update(block.cpu())                                                # the round's one read-back
                mark()
                if trace is not None:
                    trace.append(ev)
                lt_h = len0 + book.n - 1                                                # what lmod_constrain_accept left in cache.lens
        finally:
            self.train(was_training)
        seq = book.sequences().to(dev)
        if return_dict_in_generate:
            return AssistedOutput(seq, book.num_rounds, 1 + book.num_rounds, book.num_accepted.to(dev), cache, cstate)
        return seq

    @torch.no_grad()
    def _speculative_generate(self, input_ids, attention_mask, images, max_new_tokens, eos_token_id, pad_token_id, draft, k,
                              temperature, top_k, top_p, seed, return_dict_in_generate, past=None):
        """Speculative sampling, `generate(assistant_model=draft, speculative_sampling=True)`: `_assisted_generate`'s loop with draws
        in place of arg-maxes.  The first token is a plain lmod_sample_bf16 draw from the target's prefill logits.  Per round: (1) the
        draft runs its decode steps, each token drawn by lmod_sample_bf16 from the draft's own warped distribution, its logit row
        copied into a [B*k, ld] buffer; (2) the target runs ONE forward_append over [next_token, d_1 .. d_k]; (3)
        lmod_spec_sample_bf16 over the B*(k+1) target rows and the B*k draft rows: accept d_i with probability min(1, p_i(d_i) /
        q_i(d_i)), at the first rejection draw from norm(max(0, p - q)), after k acceptances draw the bonus token from p_k; EOS, done
        and both caches' lens as lmod_spec_accept; (4) the draft catches up as in the greedy mode, and its last row gives the next
        round's first draft.  One block read-back per round.  Both sides use min(V_draft, V_target) columns.  Every uniform is
        lmod_spec_uniform(seed; row, round, position, purpose): draft draws, accept tests and the residual / bonus draw never share
        one (round 0 is the first token).  `speculative_force_accept` (measurement only): the verification sees the target's rows as
        the draft's, u_acc = 0 and no top-k / top-p filter, so every draft is accepted (2 filter launches fewer than a filtered
        call).  Returns the new tokens [B, <= max_new_tokens]; with return_dict_in_generate an `AssistedOutput`."""
        from ...generation import AssistedBookkeeper, AssistedOutput
        if past is not None:
            raise ValueError("assistant_model cannot continue from past_key_values: the draft model has no cache of the earlier turns")
        modes = (self.training, draft.training)
        self.eval(), draft.eval()
        try:
            tcache, tlogits = self._start(input_ids, attention_mask, images, max_new_tokens + k + 1, None)
            dcache, _ = draft._start(input_ids, attention_mask, images, max_new_tokens + k + 1, None)
            B, dev = tlogits.shape[0], tlogits.device
            V = min(tlogits.shape[1], draft.lm_head.weight.shape[0])
            seed = int(seed) if seed is not None else int(torch.randint(0, 2 ** 31 - 1, (1,)).item())   # as generate(do_sample=True)
            warp = (temperature, top_k, top_p)
            book = AssistedBookkeeper(B, k, max_new_tokens, eos_token_id, eos_token_id if pad_token_id is None else pad_token_id)
            nxt = K.sample(tlogits[:, :V], K.spec_uniform(seed, B, 0, K.SPEC_DRAW, device=dev).view(B), *warp)
            done = book.first(nxt).to(device=dev, dtype=torch.int32).contiguous()
            lt_h, ld_h = tcache.lens.cpu().long(), dcache.lens.cpu().long()         # host copies of the caches' lens at round start
            emb_t, emb_d = self.model.embed_tokens.weight, draft.model.embed_tokens.weight
            ld_q = -(-V // 8) * 8
            qbuf = torch.empty((B, k, ld_q), device=dev, dtype=BF16)                # the draft's logit rows, row b*k + i
            u_d = torch.empty((B, k), device=dev, dtype=torch.float32)
            u_a, u_n = torch.empty_like(u_d), torch.empty(B, device=dev, dtype=torch.float32)
            force = getattr(self, "speculative_force_accept", False)
            have_first, rnd = False, 0
            d_first = None
            while not book.finished:
                rnd += 1
                if int(ld_h.max()) + k + 2 > dcache.smax:
                    dcache.grow(int(ld_h.max()) + k + 2 + max_new_tokens)
                if not have_first:
                    K.spec_uniform(seed, B, rnd, K.SPEC_DRAFT, k, out=u_d)
                K.spec_uniform(seed, B, rnd, K.SPEC_ACCEPT, k, out=u_a)
                K.spec_uniform(seed, B, rnd, K.SPEC_DRAW, 1, out=u_n)
                tok, drafts = (nxt, []) if not have_first else (d_first, [d_first])
                while len(drafts) < k:
                    i = len(drafts)
                    qbuf[:, i, :V].copy_(draft._decode_step(tok, dcache)[:, :V])
                    tok = K.sample(qbuf[:, i, :V], u_d[:, i].contiguous(), *warp)
                    drafts.append(tok)
                draft_t = torch.stack(drafts, 1).contiguous()
                chunk = torch.cat([nxt[:, None], draft_t], 1).reshape(-1).contiguous()
                hid = self.model.forward_append(K.gather_rows(emb_t, None, chunk, emb_t.shape[1]), tcache, k + 1, max_len=int(lt_h.max()))
                plog = ops.linear_fwd(hid, self.head())
                vwarp = warp
                if force:                   # measurement only: q := p, u_acc = 0, no filter in the verification: every draft accepted
                    qbuf[:, :, :V].copy_(plog.view(B, k + 1, -1)[:, :k, :V])
                    u_a.zero_()
                    vwarp = (temperature, None, None)
                block, nxt = K.spec_sample(plog[:, :V], qbuf.view(B * k, ld_q)[:, :V], draft_t, u_a, u_n, done, eos_token_id, book.pad,
                                           tcache.lens, dcache.lens, *vwarp)
                blk = block.cpu()                                                   # the round's one read-back
                book.update(blk)
                n_acc = blk[:, k + 1].long()
                if book.finished:
                    break
                done.copy_(book.stopped.to(torch.int32))
                full = n_acc == k
                idx = torch.tensor([2 * b + j for b in range(B) for j in ((0, 1) if bool(full[b]) else (1,))], dtype=torch.long)
                toks = torch.stack([draft_t[:, k - 1], nxt], 1).reshape(-1)[idx.to(dev)].contiguous()
                n_ch = 1 + full.to(torch.int32)
                hid = draft.model.forward_append(K.gather_rows(emb_d, None, toks, emb_d.shape[1]), dcache, n_ch.to(dev), T=2,
                                                 max_len=int((ld_h + torch.clamp(n_acc + 1, max=k)).max()))
                lt_h, ld_h = lt_h + n_acc + 1, ld_h + n_acc + 1
                last = (n_ch.cumsum(0) - 1).to(torch.int32).to(dev)
                hl = K.gather_rows(hid, None, last, hid.shape[1])
                # the next round's first draft: drawn from the catch-up's last row with that round's first draft uniform
                qbuf[:, 0, :V].copy_(ops.linear_fwd(hl, draft.head())[:, :V])
                K.spec_uniform(seed, B, rnd + 1, K.SPEC_DRAFT, k, out=u_d)
                d_first = K.sample(qbuf[:, 0, :V], u_d[:, 0].contiguous(), *warp)
                have_first = True
        finally:
            self.train(modes[0]), draft.train(modes[1])
        seq = book.sequences().to(dev)
        if return_dict_in_generate:
            return AssistedOutput(seq, book.num_rounds, 1 + book.num_rounds, book.num_accepted.to(dev), tcache)
        return seq

    @torch.no_grad()
    def _beam_generate(self, input_ids, attention_mask, images, max_new_tokens, eos_token_id, pad_token_id, do_sample, num_beams,
                       num_return_sequences, length_penalty, early_stopping, return_dict_in_generate, past=None):
        """Beam search (HF `_beam_search`, do_sample=False; the bookkeeping and where it follows transformers 5.x rather than
        4.37: llavamod/generation.py).  The prompt is prefilled once at B rows and its cache replicated into B*num_beams rows
        (smax = S + max_new_tokens); every step is lmod_beam_topk_bf16 (top 2*nb candidates per sample, on the device) -> one
        read-back of the candidate block -> scorer -> lmod_kv_gather_rows (the beams' parent rows into the second cache buffer)
        -> one decode step over B*nb tokens.  Returns the new tokens [B*num_return_sequences, L] (int64, best hypothesis first
        within each sample; an EOS that ended a hypothesis stays, later positions hold pad_token_id); with
        return_dict_in_generate an object with `sequences` and `sequences_scores` (fp32, length-normalised)."""
        from ...generation import BeamSearchOutput, BeamSearchScorer, check_beam_args, unpack_candidates
        check_beam_args(num_beams, num_return_sequences, do_sample, length_penalty, early_stopping)
        was_training = self.training
        self.eval()                            # the MoE student routes with eval_capacity_factor, as greedy / sampling do
        try:
            pcache, logits = self._start(input_ids, attention_mask, images, max_new_tokens, past)
            B, nb, dev = logits.shape[0], num_beams, logits.device
            cfg = self.config
            cache = KVCache(cfg.num_hidden_layers, B * nb, pcache.smax, cfg.num_key_value_heads * cfg.head_dim, dev)
            cache.lens.copy_(pcache.lens.repeat_interleave(nb))
            K.kv_gather_rows(cache.tensors(), pcache.tensors(),
                             torch.arange(B * nb, device=dev, dtype=torch.int32) // nb, cache.lens)
            del pcache
            logits = logits.repeat_interleave(nb, 0)
            scorer = BeamSearchScorer(B, nb, max_new_tokens, length_penalty, early_stopping, eos_token_id, pad_token_id)
            beam_scores = scorer.initial_beam_scores().to(dev)
            while True:
                cand = K.beam_topk(logits, beam_scores, nb).cpu()
                tok, src, bs = scorer.step(*unpack_candidates(cand))
                if scorer.is_done:
                    break
                nxt = torch.stack([tok.to(torch.int32), src.to(torch.int32), bs.view(torch.int32)]).to(dev)   # one copy
                cache.reorder(nxt[1])
                beam_scores = nxt[2].view(torch.float32)
                logits = self._decode_step(nxt[0], cache)
            seq, scores = scorer.finalize(num_return_sequences)
        finally:
            self.train(was_training)
        seq, scores = seq.to(dev), scores.to(dev)
        return BeamSearchOutput(seq, scores, cache) if return_dict_in_generate else seq

    # ---- checkpoints in the reference's layout -----------------------------------------------------------------------
    def save_config(self, save_directory):
        """`config.json` alone (the reference: `model.config.save_pretrained(output_dir)`, align_trainer.py:631)."""
        import json
        import os
        os.makedirs(save_directory, exist_ok=True)
        cfg = {}
        for k, v in vars(self.config).items():
            if k == "mm_image_tower" and not isinstance(v, (str, type(None))):
                cfg[k] = {"__clip_vision_config__": {a: b for a, b in vars(v).items()}}
            elif isinstance(v, (str, int, float, bool, type(None), list, dict)):
                cfg[k] = v
        cfg["model_type"] = getattr(self.config, "model_type", None)
        cfg["architectures"] = [type(self).__name__]
        tmp = os.path.join(save_directory, f"config.json.tmp{os.getpid()}")
        with open(tmp, "w") as f:                              # temp file + rename: a crash never leaves half a config
            json.dump(cfg, f, indent=1)
        os.replace(tmp, os.path.join(save_directory, "config.json"))

    def save_pretrained(self, save_directory, max_shard_bytes=5 << 30, writer_rank=0):
        """config.json + HF-layout safetensors shards (+ mm_projector.bin), loadable by `from_pretrained`.  One rank writes
        (`writer_rank`, a global rank; without torch.distributed the caller is rank 0); an expert-parallel model is saved
        collectively with its experts gathered under global indices (`checkpoint.save_checkpoint`)."""
        from ...checkpoint import _dist_rank_world, save_checkpoint
        files = save_checkpoint(self, save_directory, max_shard_bytes=max_shard_bytes, writer_rank=writer_rank)
        rank = _dist_rank_world()[0]
        if rank == writer_rank:
            self.save_config(save_directory)
        else:                                   # not an error (the collective save calls this on every rank), but never silent
            import logging
            logging.getLogger("llavamod").info("save_pretrained(%s): rank %d is not the writer (rank %d) and wrote nothing",
                                               save_directory, rank, writer_rank)
        return files

    def save_mm_adapter(self, output_dir, keys_to_match=("mm_projector",)):
        """Adapter-only save of the reference's trainers (train/align_trainer.py:616-636 `_save_checkpoint` with
        tune_mm_mlp_adapter; train/align_train.py:623-631 `safe_save_model_for_hf_trainer`): ONLY the parameters whose name
        contains one of `keys_to_match`, under their full names, torch-pickled as `mm_projector.bin` — the file
        `--pretrain_mm_mlp_adapter` reads back (llava_arch.py:122-128)."""
        import os
        os.makedirs(output_dir, exist_ok=True)
        sd = {k: v.detach().cpu().clone() for k, v in self.state_dict().items() if any(m in k for m in keys_to_match)}
        if not sd:
            raise ValueError(f"no parameter matches {keys_to_match}")
        path = os.path.join(output_dir, "mm_projector.bin")
        tmp = f"{path}.tmp{os.getpid()}"                      # per-process temp name: two writers never share a half-written file
        torch.save(sd, tmp)
        os.replace(tmp, path)
        return path

    @classmethod
    def from_pretrained(cls, pretrained_model_name_or_path, *model_args, attn_implementation=None, torch_dtype=None,
                        device="cuda", strict=True, config=None, cache_dir=None, **kwargs):
        """`X.from_pretrained(path, attn_implementation=...)` of the reference's entry scripts (train/align_train.py:133-139):
        read config.json, build the architecture, load the weights by name.  attn_implementation is recorded only (there is
        one attention implementation here: the HIP flash kernels); torch_dtype must be bf16 (the compute dtype).

        Image tower: a tower NAMED in the config (`mm_image_tower: "<dir or hub name>"`) takes its weights from that
        directory (also looked up relative to the checkpoint), as `CLIPVisionModel.from_pretrained` does in the reference
        (clip_encoder.py:24-33) — `model.image_tower.*` tensors of the main checkpoint are then ignored, as the reference
        ignores them (its tower is built with delay_load, llava_arch.py:31).  If the name is not a local directory (a hub
        name; no network here) the main checkpoint's own `model.image_tower.*` tensors are used; if it has none, this raises."""
        import json
        import os
        from ...checkpoint import load_checkpoint, read_state
        from ..multimodal_encoder.clip_encoder import KNOWN_GEOMETRY, CLIPVisionConfig
        if torch_dtype not in (None, torch.bfloat16):
            raise ValueError("this path computes in bf16: torch_dtype must be torch.bfloat16 (or None)")
        path = pretrained_model_name_or_path
        if config is None:
            raw = json.load(open(os.path.join(path, "config.json")))
            raw.update(kwargs)
            moe = raw.pop("moe", None)
            for drop in ("architectures", "model_type", "transformers_version", "torch_dtype", "dtype", "lora"):
                raw.pop(drop, None)
            tower = raw.get("mm_image_tower")
            if isinstance(tower, dict) and "__clip_vision_config__" in tower:
                raw["mm_image_tower"] = CLIPVisionConfig(**tower["__clip_vision_config__"])
            config = cls.config_class(**raw)
            if moe is not None:
                config.moe = moe
        config._attn_implementation = attn_implementation
        config._name_or_path = path
        model = cls(config, device=device)
        tower, src, ignore = model.get_image_tower(), None, ()
        if tower is not None and not tower.is_loaded:
            try:
                tower.load_model(search=(path,))
                ignore = ("model.image_tower.",)
            except FileNotFoundError as e:
                src = read_state(path)
                pre = "model.image_tower.image_tower."
                tsd = {k[len(pre):]: v for k, v in src.items() if k.startswith(pre)}
                if not tsd:
                    raise FileNotFoundError(f"{e}; and {path} holds no `{pre}*` tensors either") from None
                heads = KNOWN_GEOMETRY.get(tower.image_tower_name, {}).get("num_attention_heads")
                tower.load_from_state(tsd, source=f"{path} ({pre}*)", heads=heads)
        load_checkpoint(model, path, strict=strict, ignore_prefixes=ignore, state=src)
        return model

    def lm_loss_from_hidden(self, hidden, info):
        """Shifted CrossEntropyLoss() of the reference forward (mean over non-ignored), loss rows only."""
        plan = build_loss_plan(info.labels_np, info.lens_np, kd_rows=False, ce_rows=True, device=hidden.device)
        if getattr(info, "packed", None) is not None:
            from ..llava_arch import pack_loss_plan
            plan = pack_loss_plan(plan, info.packed)
        _, _, ce_sum, ce_cnt = ops.DistillHead.apply(hidden, self.head(), plan, None, *self._head_trainable())
        return ce_sum.sum() / ce_cnt.sum()

    def _head_trainable(self):
        return [self.lm_head.weight] if self.lm_head.weight.requires_grad else []

    def full_logits(self, hidden, B, S, packed=None):
        if packed is not None:                 # unpadded execution: back to the reference's padded [B, S', V] (zero rows on pads)
            hidden = ops.RowGather.apply(hidden, packed.to_packed, _inverse_map(packed))
        lg = ops.Linear.apply(hidden, self.head(), *self._head_trainable())
        return lg.view(B, S, -1).float()                        # `logits = logits.float()` (modeling_qwen2.py:1164)


class LlavaQwen2ForCausalLM(_CausalLMBase):
    config_class = LlavaQwen2Config

    def __init__(self, config, device="cuda"):
        super().__init__()
        self.config = config
        self.model = LlavaQwen2Model(config, device)
        self._setup_head(config, device)
        self._plan = None
        init_normal_(self, getattr(config, "initializer_range", 0.02), getattr(config, "init_seed", 0))   # post_init()

    def forward(self, input_ids=None, attention_mask=None, position_ids=None, past_key_values=None,
                inputs_embeds=None, labels=None, use_cache=None, output_attentions=None, output_hidden_states=None,
                images=None, return_dict=None):
        if use_cache or past_key_values is not None:
            return self._cached_forward(input_ids, attention_mask, images, past_key_values, CausalLMOutputWithPast)
        hidden, _, info = self.forward_hidden(input_ids, attention_mask, labels, images, inputs_embeds)
        logits = self.full_logits(hidden, info.B, info.S, getattr(info, "packed", None))
        loss = self.lm_loss_from_hidden(hidden, info) if info.labels is not None else None
        return CausalLMOutputWithPast(loss=loss, logits=logits, labels=info.labels)


LlavaQwen1_5Config = LlavaQwen2Config
LlavaQwen1_5ForCausalLM = LlavaQwen2ForCausalLM
