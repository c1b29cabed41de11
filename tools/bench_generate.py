"""ms per new token of generate() at the teacher's geometry (Qwen1.5-7B decoder + CLIP-ViT-L/14-336 tower, random bf16 weights):
greedy (num_beams 1) and beam search (num_beams 4), prompts of 576 image rows + text (~700 positions).  The decode rate is the
difference of two generate() calls of N1 and N2 new tokens (device events, after a warm-up of each), so the prefill cancels:
ms/token = (t(N2) - t(N1)) / (N2 - N1).  One JSON line per (B, num_beams).

--sample adds the sampling arms: B in {1, 8} x {temperature 0.2 + top_p 0.7, top_k 50}, each timed twice in the same process,
alternating call by call: sample_on_device=True (lmod_sample_bf16) and False (the torch `_sample`: the selection path before the
kernel existed, on the same decode kernels).  One JSON line per (B, filter) with both rates; the greedy line of the same B is the
floor either can reach.

    python tools/bench_generate.py                       # B in {1, 4, 8} x num_beams in {1, 4}
    python tools/bench_generate.py --only 1x4 --reps 1   # one configuration (for a rocprofv3 --kernel-trace --stats run)
    python tools/bench_generate.py --only 1x1,8x1 --sample          # greedy lines + the sampling A/B
    python tools/bench_generate.py --only none --sample --sample-only 1 --device-arm-only --reps 1   # B = 1 device arm (trace)

--append T (comma-separated list) times the multi-token cache extension against the decode path in the same process, the arms
alternating call by call, over a 700-position cache: (a) lmod_attn_append for T queries of one sample against T calls of
lmod_attn_decode at the same cache length — wrapper calls back to back over ONE cache that stays in L2 / Infinity Cache, launch
overhead included: a warm-cache call cost, not the kernel time inside generate() (profiles/sample_kernel_trace.md has that); (b) one chunk forward of T tokens at B 1 (Qwen2Model.forward_append + lm_head) against one
decode step at batch T.  --assistant k times greedy assisted generation: the teacher drafting for itself (every draft accepted: the
mechanics' cost), the random-weight student drafting (nearly nothing accepted: the worst-case overhead) and the student with
acceptance forced (the round's cost at full acceptance), against plain greedy; every round is also split into draft / verify /
accept / catch-up by events inside the loop (model.assisted_trace).

    python tools/bench_generate.py --only none --append 2,4,8 > profiles/append_attn.jsonl

--extend T (comma-separated list) times a second turn of T text tokens after one image-plus-text prefill, B in {1, 8}, two arms
alternating call by call in one process, best of --reps: the extend path (one pass of Qwen2Model.forward_extend, lmod_attn_extend)
and the piece loop (extend_min_tokens raised: ceil(T / 16) passes of forward_append, the only path before lmod_attn_extend existed).
Both return the last row's logits (`_append_chunk(..., "last")`).  One JSON line per (B, T).

    python tools/bench_generate.py --only none --extend 32,160,640 > profiles/extend_attention.jsonl
    rocprofv3 --kernel-trace --stats -- python tools/bench_generate.py --only none --extend 640 --extend-only 1 --extend-arm-only --reps 1
    python tools/bench_generate.py --only none --assistant 4 > profiles/assisted_generate.jsonl

--processors times greedy generate() with repetition_penalty=1.1, no_repeat_ngram_size=3 and one two-token stop sequence that never
fires, B in {1, 8}, three arms alternating call by call in one process, best of --reps: plain greedy (none of the arguments: the
loop without a history), the device kernels (lmod_logits_process_bf16 + lmod_gen_push_stop) and torch glue (the statements of
tests/_logits_ref.py on device tensors, through model.logits_glue).  One JSON line per B.

    python tools/bench_generate.py --only none --processors > profiles/logits_process_ab.jsonl
    python tools/bench_generate.py --only none --processors --processors-only 1 --device-arm-only --reps 1   # B = 1 device arm (trace)

--batched N serves one list of N requests (one image + text each, planted lengths: max_new_tokens drawn per request, one word to a
paragraph; random weights never emit an EOS) three ways in one process, arms alternating call by call, best of --reps:
generate_batch (continuous batching at --max-batch-size slots), generate() over consecutive static batches of that size (each runs
until its longest row ends: the behaviour before generate_batch) and a B = 1 loop.  It also measures one decode step at
max_batch_size rows and one prefill per admission size that occurs, and prints the prediction
num_decode_forwards x step + sum over prefill passes of prefill(size), step and prefill counts from generation.SlotScheduler,
beside the measured wall time.  One JSON line.

    python tools/bench_generate.py --only none --batched 24 > profiles/batched_generate.jsonl

--speculative k times generate(do_sample=True) against generate(assistant_model=student, speculative_sampling=True) at B in {1, 8}
(speculative_arms); --spec-kernel-only k runs lmod_spec_sample_bf16 alone at V = 151936 for a kernel trace.

    python tools/bench_generate.py --only none --speculative 5 > profiles/spec_sample_ab.jsonl
    rocprofv3 --kernel-trace --stats -- python tools/bench_generate.py --spec-kernel-only 5

--lookup k times generate(prompt_lookup_num_tokens=k) (prompt-lookup decoding: the draft is the call's own token history) against plain
greedy at B in {1, 8}, three arms alternating call by call in one process, best of --reps: greedy, lookup (random weights: what the
history happens to offer is all that is accepted) and lookup_forced (model.assisted_force_accept: every drafted token counts as
accepted; its tokens are not greedy's).  Every round is split into draft / verify / accept by events inside the loop
(model.assisted_trace).  One JSON line per B.

    python tools/bench_generate.py --only none --lookup 4 > profiles/prompt_lookup.jsonl

--batched N --lookup k times generate_batch(prompt_lookup_num_tokens=k) (prompt-lookup decoding under continuous batching) against
plain greedy generate_batch on the --batched request list at --max-batch-size slots, three arms alternating call by call in one
process, one warm-up each, best of --reps with every repetition kept: greedy, lookup (random weights: what the history happens to
offer is all that is accepted) and lookup_forced (model.assisted_force_accept).  Per arm: wall ms, ms per emitted token, rounds (or
decode steps), prefill passes, accepted drafts and the spread between repetitions.  One JSON line.

    python tools/bench_generate.py --only none --batched 24 --lookup 4 --max-batch-size 8 >> profiles/batched_lookup.jsonl

--constraint times greedy generate(constraint=...) against plain greedy at B in {1, 8}, three arms alternating call by call in one
process, one warm-up each, every repetition kept: plain (no constraint: the loop that ran before constraints existed), closed
(TokenConstraint.from_allowed_tokens of 4 tokens: every row sits in a closed state, so lmod_constrain_mask_rows_bf16 sweeps the
whole row every step) and open (a one-state open automaton that bans nothing: the two launches without a sweep).  ms per new token
as above, (t(N2) - t(N1)) / (N2 - N1).  One JSON line per B.

    python tools/bench_generate.py --only none --constraint > profiles/constrained_decoding.jsonl

--constraint-draft k times generate(constraint=c, constraint_draft_tokens=k) (every round drafts the tokens the automaton forces and
verifies them in one pass) against generate(constraint=c) at B in {1, 8}, two arms alternating call by call in one process, one
warm-up each, every repetition kept.  c is a from_choices trie over answers of 8 tokens with a forced tail of 0, 3 or 7 tokens
(constraint_draft_tries); every call runs until its rows reach a terminal state.  per arm: ms per answer (the whole call, prefill
included), passes over the weights per answer, and a one-token call (the prefill and the first token) to subtract; one more,
untimed call splits the rounds into draft / verify / accept by events inside the loop (model.assisted_trace).  One JSON line per B
and tail.

    python tools/bench_generate.py --only none --constraint-draft 7 > profiles/constraint_draft.jsonl
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "llava-mod_amd"))

import torch  # noqa: E402


def prompts(B, text_len, seed=0):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(0, 151643, (B, text_len), generator=g)
    ids[:, 14] = -200                                          # one image: 576 patch rows
    return dict(input_ids=ids, attention_mask=torch.ones(B, text_len, dtype=torch.bool),
                images=torch.randn(B, 3, 336, 336, generator=g).to(torch.bfloat16).cuda())


SAMPLE_ARMS = [dict(temperature=0.2, top_p=0.7), dict(top_k=50)]


def timed(model, pr, nb, n_new, sample=None):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    kw = dict(num_beams=nb) if nb > 1 else {}
    if sample is not None:
        kw = dict(do_sample=True, seed=0, **sample)
    e0.record()
    out = model.generate(**pr, max_new_tokens=n_new, **kw)
    e1.record()
    torch.cuda.synchronize()
    assert out.shape[1] == n_new, out.shape                    # no EOS: every call runs its full length
    return e0.elapsed_time(e1)


def _ms(fn, reps):
    """Device time of fn() per call: `reps` calls between two events."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def append_arms(model, Ts, text_len, reps):
    import math
    from llavamod import kernels as K
    from llavamod import ops
    cfg = model.config
    nh, nkv, hd = cfg.num_attention_heads, cfg.num_key_value_heads, cfg.head_dim
    scale, L = 1.0 / math.sqrt(hd), text_len - 1 + 576
    g = torch.Generator().manual_seed(0)
    for T in Ts:
        # (a) the attention kernels alone: one sample, L cached positions (the chunk's own keys included)
        q = torch.randn(T, nh * hd, generator=g).to(torch.bfloat16).cuda()
        kc = torch.randn(1, L + 8, nkv * hd, generator=g).to(torch.bfloat16).cuda()
        vc = torch.randn(1, L + 8, nkv * hd, generator=g).to(torch.bfloat16).cuda()
        lens = torch.full((1,), L, dtype=torch.int32, device="cuda")
        arms = {"append": lambda: K.attn_append(q, kc, vc, lens, nh, nkv, hd, scale, T),
                "decode_x_T": lambda: [K.attn_decode(q[t:t + 1], kc, vc, lens, nh, nkv, hd, scale) for t in range(T)]}
        res = {k: [] for k in arms}
        for rep in range(reps + 1):                               # rep 0 warms both arms
            for k, fn in arms.items():
                ms = _ms(fn, 50)
                if rep:
                    res[k].append(ms)
        print(json.dumps({"metric": "attn_append_vs_T_decode_calls_us", "T": T, "cache_positions": L, "nh": nh, "nkv": nkv, "hd": hd,
                          "nsplit": K.attn_append_nsplit(1, nkv, L + 8), "append_us": round(1e3 * min(res["append"]), 2),
                          "decode_x_T_us": round(1e3 * min(res["decode_x_T"]), 2),
                          "append_us_all": [round(1e3 * v, 2) for v in res["append"]],
                          "decode_x_T_us_all": [round(1e3 * v, 2) for v in res["decode_x_T"]]}), flush=True)
        # (b) the model: a chunk of T tokens at B 1 against one decode step at batch T, caches of L positions
        c1, _ = model._prefill(**{k: v[:1] for k, v in prompts(1, text_len).items()}, max_new_tokens=T + 1)
        cT, _ = model._prefill(**prompts(T, text_len), max_new_tokens=2)
        l1, lT = c1.lens.clone(), cT.lens.clone()
        tok = torch.randint(0, 151643, (T,), generator=g).to(torch.int32).cuda()
        emb_w = model.model.embed_tokens.weight

        def chunk():
            c1.lens.copy_(l1)
            emb = K.gather_rows(emb_w, None, tok, emb_w.shape[1])
            return ops.linear_fwd(model.model.forward_append(emb, c1, T, max_len=L), model.head())

        def decode():
            cT.lens.copy_(lT)
            return model._decode_step(tok, cT)

        arms = {"chunk_B1": chunk, "decode_batch_T": decode}
        res = {k: [] for k in arms}
        for rep in range(reps + 1):
            for k, fn in arms.items():
                ms = _ms(fn, 5)
                if rep:
                    res[k].append(ms)
        a, b = min(res["chunk_B1"]), min(res["decode_batch_T"])
        print(json.dumps({"metric": "chunk_forward_vs_decode_step_ms", "T": T, "cache_positions": L, "chunk_B1_ms": round(a, 3),
                          "decode_batch_T_ms": round(b, 3), "ratio": round(a / b, 3),
                          "chunk_B1_ms_all": [round(v, 3) for v in res["chunk_B1"]],
                          "decode_batch_T_ms_all": [round(v, 3) for v in res["decode_batch_T"]]}), flush=True)
        del c1, cT


def extend_arms(model, Ts, text_len, reps, Bs=(1, 8), extend_only=False):
    """ms per continuation chunk of T tokens over a cache of text_len - 1 + 576 positions: extend path against the piece loop."""
    g = torch.Generator().manual_seed(0)
    arms = ("extend",) if extend_only else ("extend", "pieces")
    for B in Bs:
        for T in Ts:
            cache, _ = model._prefill(**prompts(B, text_len), max_new_tokens=T + 1)
            lens0 = cache.lens.clone()
            ids = torch.randint(0, 151643, (B, T), generator=g)

            def run(arm):
                cache.lens.copy_(lens0)                             # the same turn again: the chunk overwrites its own positions
                model.extend_min_tokens = 17 if arm == "extend" else 1 << 30
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                model._append_chunk(ids, None, cache, "last")
                e1.record()
                torch.cuda.synchronize()
                return e0.elapsed_time(e1)

            res = {a: [] for a in arms}
            for rep in range(reps + 1):                             # rep 0 warms both arms
                for a in arms:
                    ms = run(a)
                    if rep:
                        res[a].append(ms)
            del model.extend_min_tokens
            rec = {"metric": "continuation_chunk_ms", "B": B, "T": T, "cache_positions": text_len - 1 + 576,
                   "passes_pieces": (T + 15) // 16}
            for a in arms:
                rec[f"{a}_ms"] = round(min(res[a]), 3)
                rec[f"{a}_ms_all"] = [round(v, 3) for v in res[a]]
            if not extend_only:
                rec["speedup"] = round(min(res["pieces"]) / min(res["extend"]), 2)
            print(json.dumps(rec), flush=True)
            del cache


def assisted_arms(model, k, text_len, reps, n_new=33):
    """ms per emitted token of plain greedy, of the teacher drafting for itself and of a random-weight student drafting, B 1."""
    from bench import moe_model_args, student_cfg
    from llavamod.model import LLaVAMoDQwen2ForCausalLM
    student = LLaVAMoDQwen2ForCausalLM(student_cfg(4), device="cuda")
    student.initialize_moe_modules(moe_model_args(4))
    student.eval()
    pr = prompts(1, text_len)

    def run(draft):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        kw = {} if draft is None else dict(assistant_model=draft, num_assistant_tokens=k, return_dict_in_generate=True)
        e0.record()
        out = model.generate(**pr, max_new_tokens=n_new, **kw)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), out

    # student_forced: the student drafts and every draft counts as accepted (model.assisted_force_accept, measurement only): the
    # cost of a round at full acceptance with the real draft's cost; its tokens are not the teacher's greedy tokens
    arms = {"greedy": (None, False), "self_draft": (model, False), "student_draft": (student, False), "student_forced": (student, True)}
    res, stats, phases = {a: [] for a in arms}, {}, {}
    for rep in range(reps + 1):
        for a, (d, forced) in arms.items():
            model.assisted_force_accept = forced
            model.assisted_trace = [] if d is not None else None
            ms, out = run(d)
            if rep:
                res[a].append(ms)
            if d is not None:
                stats[a] = dict(rounds=out.num_rounds, accepted=int(out.num_accepted.sum()), tokens=int(out.sequences.shape[1]))
                full = [ev for ev in model.assisted_trace if len(ev) == 5]        # the last round ends before the catch-up
                names = ("draft", "verify", "accept", "catchup")
                phases[a] = {n: round(sum(ev[i].elapsed_time(ev[i + 1]) for ev in full) / max(1, len(full)), 3)
                             for i, n in enumerate(names)}
    del model.assisted_force_accept, model.assisted_trace
    # the prefill(s) are inside the per-call figures; the per-round phases are device time between events recorded inside the loop
    # (accept includes the round's one read-back and the host bookkeeping)
    rec = {"metric": "assisted_generate_ms_per_call", "B": 1, "k": k, "new_tokens": n_new, "prompt_positions": text_len - 1 + 576}
    for a in arms:
        rec[f"{a}_ms"] = round(min(res[a]), 2)
        rec[f"{a}_ms_all"] = [round(v, 2) for v in res[a]]
    rec.update({f"{a}_{n}": v for a, st in stats.items() for n, v in st.items()})
    rec.update({f"{a}_round_ms": ph for a, ph in phases.items()})
    print(json.dumps(rec), flush=True)


def lookup_arms(model, k, text_len, reps, Bs=(1, 8), n_new=33, max_ngram=2):
    """ms per call and per emitted token of plain greedy and of the prompt-lookup loop, B 1 and 8 (see the module docstring)."""
    for B in Bs:
        pr = prompts(B, text_len)

        def run(lookup):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            kw = dict(prompt_lookup_num_tokens=k, max_matching_ngram_size=max_ngram, return_dict_in_generate=True) if lookup else {}
            e0.record()
            out = model.generate(**pr, max_new_tokens=n_new, **kw)
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1), out

        arms = {"greedy": (False, False), "lookup": (True, False), "lookup_forced": (True, True)}
        res, stats, phases = {a: [] for a in arms}, {}, {}
        for rep in range(reps + 1):                                # rep 0 warms every arm
            for a, (lookup, forced) in arms.items():
                model.assisted_force_accept = forced
                model.assisted_trace = [] if lookup else None
                ms, out = run(lookup)
                if rep:
                    res[a].append(ms)
                if lookup:
                    stats[a] = dict(rounds=out.num_rounds, accepted=int(out.num_accepted.sum()), tokens=int(out.sequences.shape[1]))
                    tr = model.assisted_trace
                    phases[a] = {n: round(sum(ev[i].elapsed_time(ev[i + 1]) for ev in tr) / max(1, len(tr)), 3)
                                 for i, n in enumerate(("draft", "verify", "accept"))}
        del model.assisted_force_accept, model.assisted_trace
        # the prefill is inside the per-call figures; the per-round phases are device time between events recorded inside the loop
        # (draft: lmod_ngram_draft; verify: embedding gather, forward_append, head, argmax; accept: lmod_spec_accept,
        # lmod_hist_push_block, the round's one read-back and the host bookkeeping)
        rec = {"metric": "prompt_lookup_ms_per_call", "B": B, "k": k, "max_ngram": max_ngram, "new_tokens": n_new,
               "prompt_positions": text_len - 1 + 576}
        for a in arms:
            rec[f"{a}_ms"] = round(min(res[a]), 2)
            rec[f"{a}_ms_all"] = [round(v, 2) for v in res[a]]
        rec.update({f"{a}_{n}": v for a, st in stats.items() for n, v in st.items()})
        rec.update({f"{a}_round_ms": ph for a, ph in phases.items()})
        print(json.dumps(rec), flush=True)


def speculative_arms(model, k, text_len, reps, Bs=(1, 8), n_new=33, sample=dict(temperature=1.0, top_p=0.9)):
    """ms per new token of plain generate(do_sample=True) (the baseline: the path before speculative sampling existed) against
    generate(assistant_model=student, speculative_sampling=True), arms alternating call by call in one process, best of `reps`.
    Random weights give a meaningless acceptance rate, so two arms bracket it: student_draft (lower bound: the random student's drafts
    are nearly always rejected) and student_forced (upper bound: model.speculative_force_accept replaces the draft's logit rows by the
    target's, every draft is accepted; measurement only).  One JSON line per B, with the measured acceptance and rounds."""
    from bench import moe_model_args, student_cfg
    from llavamod.model import LLaVAMoDQwen2ForCausalLM
    student = LLaVAMoDQwen2ForCausalLM(student_cfg(4), device="cuda")
    student.initialize_moe_modules(moe_model_args(4))
    student.eval()
    for B in Bs:
        pr = prompts(B, text_len)

        def run(arm):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            if arm == "plain":
                kw = dict(do_sample=True, seed=0, **sample)
            else:
                kw = dict(assistant_model=student, speculative_sampling=True, num_assistant_tokens=k, seed=0,
                          return_dict_in_generate=True, **sample)
                model.speculative_force_accept = arm == "student_forced"
            e0.record()
            out = model.generate(**pr, max_new_tokens=n_new, **kw)
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1), out

        arms = ("plain", "student_draft", "student_forced")
        res, stats = {a: [] for a in arms}, {}
        for rep in range(reps + 1):                                # rep 0 warms every arm
            for a in arms:
                ms, out = run(a)
                if rep:
                    res[a].append(ms)
                if a != "plain":
                    stats[a] = dict(rounds=out.num_rounds, accepted=int(out.num_accepted.sum()), tokens=int(out.sequences.shape[1]),
                                    acceptance=round(float(out.num_accepted.sum()) / (B * k * out.num_rounds), 4))
        del model.speculative_force_accept
        # the prefill(s) are inside every figure: ms per call / new tokens
        rec = {"metric": "speculative_sampling_ms_per_new_token", "B": B, "k": k, "new_tokens": n_new, **sample,
               "prompt_positions": text_len - 1 + 576}
        for a in arms:
            rec[f"{a}_ms_per_token"] = round(min(res[a]) / n_new, 3)
            rec[f"{a}_ms_per_token_all"] = [round(v / n_new, 3) for v in res[a]]
        rec.update({f"{a}_{n}": v for a, st in stats.items() for n, v in st.items()})
        print(json.dumps(rec), flush=True)


def spec_kernel_only(k, reps=20, V=151936):
    """lmod_spec_sample_bf16 alone at the vocabulary's size, B in {1, 8} (for a kernel trace): device ms per call by events."""
    from llavamod import kernels as K
    for B in (1, 8):
        g = torch.Generator(device="cuda").manual_seed(B)
        P = (3 * torch.randn(B * (k + 1), V, device="cuda", generator=g)).to(torch.bfloat16)
        Q = (P.view(B, k + 1, V)[:, :k].float() + 0.5 * torch.randn(B, k, V, device="cuda", generator=g)).to(torch.bfloat16).view(B * k, V)
        draft = K.sample(Q, torch.rand(B * k, device="cuda", generator=g), 1.0, None, 0.9).view(B, k).contiguous()
        ua, un = torch.rand(B, k, device="cuda", generator=g), torch.rand(B, device="cuda", generator=g)
        i32 = dict(device="cuda", dtype=torch.int32)

        def call(tk, tp):
            K.spec_sample(P, Q, draft, ua, un, torch.zeros(B, **i32), None, 0, torch.full((B,), 700, **i32), torch.full((B,), 700, **i32),
                          1.0, tk, tp)
        for name, (tk, tp) in (("none", (None, None)), ("top_p", (None, 0.9)), ("top_k_top_p", (50, 0.9))):
            call(tk, tp)
            print(json.dumps({"metric": "spec_sample_kernel_ms_per_call", "B": B, "k": k, "V": V, "filter": name,
                              "ms": round(_ms(lambda: call(tk, tp), reps), 4)}), flush=True)


PROCESSORS = dict(repetition_penalty=1.1, no_repeat_ngram_size=3, stop_sequences=[[151640, 151641]])


def processor_arms(model, Bs, text_len, reps, n1, n2, device_only=False):
    """ms per new token of greedy generate(): plain, with the processors on the device kernels, with the processors as torch glue."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import _logits_ref as LR

    def run(pr, arm, n_new):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        if arm == "glue":
            model.logits_glue = (LR.process_logits, LR.push_stop)
        try:
            e0.record()
            out = model.generate(**pr, max_new_tokens=n_new, **({} if arm == "plain" else PROCESSORS))
            e1.record()
            torch.cuda.synchronize()
        finally:
            if arm == "glue":
                del model.logits_glue
        assert out.shape[1] == n_new, out.shape                    # the stop sequence never fires: every call runs its full length
        return e0.elapsed_time(e1)

    arms = ("device",) if device_only else ("plain", "device", "glue")
    for B in Bs:
        pr = prompts(B, text_len)
        t1, t2 = {a: [] for a in arms}, {a: [] for a in arms}
        for rep in range(reps + 1):                                # rep 0 warms every arm at both lengths
            for a in arms:
                x, y = run(pr, a, n1), run(pr, a, n2)
                if rep:
                    t1[a].append(x)
                    t2[a].append(y)
        rec = {"metric": "generate_processors_ms_per_new_token", "B": B, **PROCESSORS, "prompt_positions": text_len - 1 + 576,
               "n1": n1, "n2": n2}
        for a in arms:
            per = [(y - x) / (n2 - n1) for x, y in zip(t1[a], t2[a])]
            rec[f"ms_per_token_{a}"] = round(min(per), 3)
            rec[f"ms_per_token_{a}_all"] = [round(v, 3) for v in per]
        print(json.dumps(rec), flush=True)


CONSTRAINT_ALLOWED = [32, 33, 34, 35]


def constraint_arms(model, Bs, text_len, reps, n1, n2):
    """ms per new token of greedy generate(): plain, under a closed allow-list of 4 tokens, under an open automaton that bans nothing."""
    from llavamod.generation import TokenConstraint
    cons = {"plain": None, "closed": TokenConstraint.from_allowed_tokens(CONSTRAINT_ALLOWED), "open": TokenConstraint(1, [], [], default=0)}

    def run(pr, arm, n_new):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        kw = {} if cons[arm] is None else dict(constraint=cons[arm])
        e0.record()
        out = model.generate(**pr, max_new_tokens=n_new, **kw)
        e1.record()
        torch.cuda.synchronize()
        assert out.shape[1] == n_new, out.shape                    # no EOS and no terminal state: every call runs its full length
        assert arm != "closed" or set(out.reshape(-1).tolist()) <= set(CONSTRAINT_ALLOWED)
        return e0.elapsed_time(e1)

    for B in Bs:
        pr = prompts(B, text_len)
        t1, t2 = {a: [] for a in cons}, {a: [] for a in cons}
        for rep in range(reps + 1):                                # rep 0 warms every arm at both lengths
            for a in cons:
                x, y = run(pr, a, n1), run(pr, a, n2)
                if rep:
                    t1[a].append(x)
                    t2[a].append(y)
        rec = {"metric": "generate_constraint_ms_per_new_token", "B": B, "V": model.lm_head.weight.shape[0],
               "closed_allowed_tokens": len(CONSTRAINT_ALLOWED), "prompt_positions": text_len - 1 + 576, "n1": n1, "n2": n2}
        for a in cons:
            per = [(y - x) / (n2 - n1) for x, y in zip(t1[a], t2[a])]
            rec[f"ms_per_token_{a}"] = round(min(per), 3)
            rec[f"ms_per_token_{a}_all"] = [round(v, 3) for v in per]
            rec[f"spread_{a}"] = round(max(per) / min(per) - 1, 4)
        print(json.dumps(rec), flush=True)


CONSTRAINT_DRAFT_LEN = 8


def constraint_draft_tries(tail):
    """from_choices over answers of CONSTRAINT_DRAFT_LEN tokens: each of the first 8 - tail tokens is a choice between two ids (the
    same two at every state of that depth), the last `tail` tokens are forced.  tail 0: every state branches, nothing can be drafted;
    tail 3: the last branch is the fifth token; tail 7: only the first token is chosen.  Whatever the random weights choose, an
    answer has the same shape."""
    from llavamod.generation import TokenConstraint
    n = CONSTRAINT_DRAFT_LEN
    heads = [[]]
    for d in range(n - tail):
        heads = [h + [1000 + 2 * d + j] for h in heads for j in (0, 1)]
    return TokenConstraint.from_choices([h + [2000 + d for d in range(tail)] for h in heads])


def constraint_draft_arms(model, k, Bs, text_len, reps):
    """ms and passes per answer: generate(constraint=c) against generate(constraint=c, constraint_draft_tokens=k)."""
    n = CONSTRAINT_DRAFT_LEN

    def run(pr, c, arm, n_new=n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        kw = dict(constraint_draft_tokens=k) if arm == "draft" else {}
        e0.record()
        out = model.generate(**pr, max_new_tokens=n_new, constraint=c, return_dict_in_generate=True, **kw)
        e1.record()
        torch.cuda.synchronize()
        assert out.sequences.shape[1] == n_new, out.sequences.shape             # every row runs into its terminal state at token 8
        passes = out.num_target_forwards if arm == "draft" else out.sequences.shape[1]
        return e0.elapsed_time(e1), passes, out.sequences

    for B in Bs:
        pr = prompts(B, text_len)
        for tail in (0, 3, 7):
            c = constraint_draft_tries(tail)
            ms, first, passes, same = {"plain": [], "draft": []}, {"plain": [], "draft": []}, {}, True
            for rep in range(reps + 1):                            # rep 0 warms both arms
                seqs = {}
                for arm in ("plain", "draft"):
                    t, passes[arm], seqs[arm] = run(pr, c, arm)
                    t1 = run(pr, c, arm, 1)[0]
                    if rep:
                        ms[arm].append(t)
                        first[arm].append(t1)
                same = same and bool(torch.equal(seqs["plain"], seqs["draft"]))
            rec = {"metric": "generate_constraint_draft_ms_per_answer", "B": B, "k": k, "answer_tokens": n, "forced_tail": tail,
                   "states": c.n_states, "prompt_positions": text_len - 1 + 576, "same_tokens": same}
            for arm in ("plain", "draft"):
                rec[f"passes_{arm}"] = passes[arm]
                rec[f"ms_per_answer_{arm}"] = round(min(ms[arm]), 2)
                rec[f"ms_per_answer_{arm}_all"] = [round(v, 2) for v in ms[arm]]
                rec[f"ms_first_token_call_{arm}_all"] = [round(v, 2) for v in first[arm]]
                rec[f"ms_behind_first_token_{arm}"] = round(min(ms[arm]) - min(first[arm]), 2)
            model.assisted_trace = []                              # one more, untimed call: the rounds' phases from events in the loop
            run(pr, c, "draft")
            ev, model.assisted_trace = model.assisted_trace, None
            del model.assisted_trace
            for i, name in enumerate(("draft", "verify", "accept")):
                rec[f"round_ms_{name}"] = round(sum(r[i].elapsed_time(r[i + 1]) for r in ev) / len(ev), 3)
            print(json.dumps(rec), flush=True)


def batched_arms(model, n_req, B, text_len, reps, n1, n2, seed=0):
    """Wall ms of serving one request list: generate_batch / static batches of generate() / a B = 1 loop, and the scheduler's prediction."""
    import random
    from llavamod.generation import SlotScheduler, static_batch_steps
    rng = random.Random(seed)
    lengths = [rng.choice((1, 2, 3, 4, 6, 8, 12, 16, 24, 32, 48, 64)) for _ in range(n_req)]     # one word to a paragraph
    pr = prompts(n_req, text_len, seed)
    reqs = [dict(input_ids=pr["input_ids"][i], images=pr["images"][i:i + 1], max_new_tokens=lengths[i]) for i in range(n_req)]
    cut = lambda i, j: {k: v[i:j] for k, v in pr.items()}

    def run(arm):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        if arm == "batched":
            out = model.generate_batch(reqs, max_batch_size=B, return_dict_in_generate=True)
            got = [len(x) for x in out.sequences]
        elif arm == "static":
            got = []
            for i in range(0, n_req, B):
                o = model.generate(**cut(i, i + B), max_new_tokens=max(lengths[i:i + B]))
                got += [min(o.shape[1], m) for m in lengths[i:i + B]]
        else:
            got = [model.generate(**cut(i, i + 1), max_new_tokens=lengths[i]).shape[1] for i in range(n_req)]
        e1.record()
        torch.cuda.synchronize()
        assert got == lengths, (arm, got, lengths)
        return e0.elapsed_time(e1), (out if arm == "batched" else None)

    arms, t, counters = ("batched", "static", "b1"), {}, None
    for rep in range(reps + 1):                                    # rep 0 warms every arm
        for a in arms:
            ms, out = run(a)
            if rep:
                t.setdefault(a, []).append(ms)
            counters = out or counters
    # the prediction's two unit costs, measured here: a decode step at B rows, a prefill at every admission size that occurs
    sched, sizes = SlotScheduler(lengths, B), []
    while not sched.finished:
        adm = sched.admit()
        if adm:
            sizes.append(len(adm))
        sched.step()
    prB = cut(0, B)
    timed(model, prB, 1, n1), timed(model, prB, 1, n2)
    step_ms = min((timed(model, prB, 1, n2) - timed(model, prB, 1, n1)) / (n2 - n1) for _ in range(reps))
    prefill_ms = {}
    for R in sorted(set(sizes)):
        timed(model, cut(0, R), 1, 1)
        prefill_ms[R] = min(timed(model, cut(0, R), 1, 1) for _ in range(reps))          # prefill + one token selection
    predicted = sched.num_decode_forwards * step_ms + sum(prefill_ms[R] for R in sizes)
    assert counters.num_decode_steps == sched.num_decode_steps and counters.num_prefills == len(sizes)
    best = {a: min(v) for a, v in t.items()}
    print(json.dumps({
        "metric": "generate_batched_wall_ms", "requests": n_req, "max_batch_size": B, "lengths": lengths,
        "prompt_positions": text_len - 1 + 576, "new_tokens": sum(lengths),
        "ms_batched": round(best["batched"], 1), "ms_static": round(best["static"], 1), "ms_b1": round(best["b1"], 1),
        "ms_all": {a: [round(x, 1) for x in v] for a, v in t.items()},
        "speedup_vs_static": round(best["static"] / best["batched"], 3), "speedup_vs_b1": round(best["b1"] / best["batched"], 3),
        "num_decode_steps": sched.num_decode_steps, "num_decode_forwards": sched.num_decode_forwards,
        "static_steps": static_batch_steps(lengths, B), "b1_steps": sum(lengths),
        "num_admissions": sched.num_admissions, "num_prefills": sched.num_prefills, "admission_sizes": sizes,
        "live_fraction": round(sched.live_fraction, 4),
        "live_fraction_static": round(sum(lengths) / (B * static_batch_steps(lengths, B)), 4),
        "step_ms": round(step_ms, 3), "prefill_ms": {str(k): round(v, 1) for k, v in prefill_ms.items()},
        "predicted_ms_batched": round(predicted, 1), "measured_over_predicted": round(best["batched"] / predicted, 3)}), flush=True)


def batched_lookup_arms(model, n_req, B, k, text_len, reps, seed=0, max_ngram=2):
    """Wall ms of serving the --batched request list: plain greedy generate_batch against generate_batch(prompt_lookup_num_tokens=k),
    as is and with every drafted token counted as accepted."""
    import random
    rng = random.Random(seed)
    lengths = [rng.choice((1, 2, 3, 4, 6, 8, 12, 16, 24, 32, 48, 64)) for _ in range(n_req)]     # batched_arms' list
    pr = prompts(n_req, text_len, seed)
    reqs = [dict(input_ids=pr["input_ids"][i], images=pr["images"][i:i + 1], max_new_tokens=lengths[i]) for i in range(n_req)]

    def run(arm):
        kw = {} if arm == "greedy" else dict(prompt_lookup_num_tokens=k, max_matching_ngram_size=max_ngram)
        model.assisted_force_accept = arm == "lookup_forced"
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = model.generate_batch(reqs, max_batch_size=B, return_dict_in_generate=True, **kw)
        e1.record()
        torch.cuda.synchronize()
        del model.assisted_force_accept
        assert [len(x) for x in out.sequences] == lengths, (arm, [len(x) for x in out.sequences], lengths)
        return e0.elapsed_time(e1), out

    arms, t, outs = ("greedy", "lookup", "lookup_forced"), {}, {}
    for rep in range(reps + 1):                                    # rep 0 warms every arm
        for a in arms:
            ms, outs[a] = run(a)
            if rep:
                t.setdefault(a, []).append(ms)
    # random weights leave near-ties, where the chunk path and the decode path may pick different tokens: reported, not asserted
    same = sum(bool(torch.equal(x, y)) for x, y in zip(outs["greedy"].sequences, outs["lookup"].sequences))
    n_tok = sum(lengths)
    rec = {"metric": "generate_batched_lookup_wall_ms", "requests": n_req, "max_batch_size": B, "k": k, "max_ngram": max_ngram,
           "lengths": lengths, "prompt_positions": text_len - 1 + 576, "new_tokens": n_tok, "requests_equal_to_greedy": same}
    for a in arms:
        o, best = outs[a], min(t[a])
        passes = o.num_decode_steps if a == "greedy" else o.num_rounds
        rec[a] = {"ms": round(best, 1), "ms_all": [round(x, 1) for x in t[a]], "spread": round(max(t[a]) / best - 1, 4),
                  "ms_per_token": round(best / n_tok, 3), "passes": passes, "ms_per_pass_incl_prefill": round(best / passes, 3),
                  "num_prefills": o.num_prefills, "live_fraction": round(o.live_fraction, 4)}
        if a != "greedy":
            rec[a]["accepted"] = sum(o.num_accepted)
            rec[a]["tokens_per_live_row_round"] = round(n_tok / o.live_row_steps, 3)
    rec["lookup_over_greedy"] = round(rec["lookup"]["ms"] / rec["greedy"]["ms"], 3)
    rec["forced_over_greedy"] = round(rec["lookup_forced"]["ms"] / rec["greedy"]["ms"], 3)
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--text-len", type=int, default=125, help="text tokens incl. the image placeholder (+575 -> prompt length)")
    ap.add_argument("--n1", type=int, default=4)
    ap.add_argument("--n2", type=int, default=36)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--only", default=None, help="comma-separated BxNB, e.g. 1x4,4x1")
    ap.add_argument("--sample", action="store_true", help="also time the sampling arms, device kernel against the torch path")
    ap.add_argument("--sample-only", default=None, help="comma-separated B of the sampling arms (default 1,8)")
    ap.add_argument("--device-arm-only", action="store_true", help="sampling: skip the torch arm (for a kernel trace)")
    ap.add_argument("--append", default=None, help="comma-separated chunk lengths T: chunk path against the decode path")
    ap.add_argument("--extend", default=None, help="comma-separated chunk lengths T: extend path against the piece loop, B 1 and 8")
    ap.add_argument("--extend-only", default=None, help="comma-separated B of the extend arms (default 1,8)")
    ap.add_argument("--extend-arm-only", action="store_true", help="extend: skip the piece-loop arm (for a kernel trace)")
    ap.add_argument("--assistant", type=int, default=None, help="k: assisted generation (self-draft, student draft) against greedy")
    ap.add_argument("--processors", action="store_true", help="greedy with logits processors: plain / device kernels / torch glue")
    ap.add_argument("--processors-only", default=None, help="comma-separated B of the processor arms (default 1,8)")
    ap.add_argument("--batched", type=int, default=None, help="N requests: generate_batch against static batches and a B = 1 loop")
    ap.add_argument("--max-batch-size", type=int, default=8, help="slots of the --batched arms")
    ap.add_argument("--speculative", type=int, default=None, help="k: speculative sampling (student draft / forced) against do_sample")
    ap.add_argument("--lookup", type=int, default=None, help="k: prompt-lookup decoding (as is / acceptance forced) against greedy; with --batched: the generate_batch arms")
    ap.add_argument("--constraint", action="store_true", help="greedy under a token automaton: plain / closed allow-list / open")
    ap.add_argument("--constraint-only", default=None, help="comma-separated B of the constraint arms (default 1,8)")
    ap.add_argument("--constraint-draft", type=int, default=None, help="k: generate(constraint=, constraint_draft_tokens=k) against generate(constraint=)")
    ap.add_argument("--spec-kernel-only", type=int, default=None, help="k: lmod_spec_sample_bf16 alone, no model (for a kernel trace)")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_generate.py measures on the GPU"
    if a.spec_kernel_only:
        return spec_kernel_only(a.spec_kernel_only)
    from bench import teacher_cfg
    from llavamod.model import LlavaQwen2ForCausalLM
    model = LlavaQwen2ForCausalLM(teacher_cfg(), device="cuda")
    model.eval()
    cfgs = [(1, 1), (1, 4), (4, 1), (8, 1), (8, 4)]
    if a.only:
        cfgs = [] if a.only == "none" else [tuple(int(x) for x in c.split("x")) for c in a.only.split(",")]
    for B, nb in cfgs:
        pr = prompts(B, a.text_len)
        timed(model, pr, nb, a.n1)                             # warm-up of both lengths
        timed(model, pr, nb, a.n2)
        t1 = [timed(model, pr, nb, a.n1) for _ in range(a.reps)]
        t2 = [timed(model, pr, nb, a.n2) for _ in range(a.reps)]
        per = [(y - x) / (a.n2 - a.n1) for x, y in zip(t1, t2)]
        print(json.dumps({"metric": "generate_ms_per_new_token", "B": B, "num_beams": nb, "rows": B * nb,
                          "prompt_positions": a.text_len - 1 + 576, "ms_per_token": round(min(per), 3),
                          "ms_per_token_all": [round(p, 3) for p in per], "ms_call_n1": [round(x, 1) for x in t1],
                          "ms_call_n2": [round(y, 1) for y in t2], "n1": a.n1, "n2": a.n2}), flush=True)
    if a.append:
        append_arms(model, [int(x) for x in a.append.split(",")], a.text_len, a.reps)
    if a.extend:
        extend_arms(model, [int(x) for x in a.extend.split(",")], a.text_len, a.reps,
                    [int(x) for x in a.extend_only.split(",")] if a.extend_only else (1, 8), a.extend_arm_only)
    if a.assistant:
        assisted_arms(model, a.assistant, a.text_len, a.reps)
    if a.lookup and a.batched:                                     # together: the lookup rounds under continuous batching
        batched_lookup_arms(model, a.batched, a.max_batch_size, a.lookup, a.text_len, a.reps)
    elif a.lookup:
        lookup_arms(model, a.lookup, a.text_len, a.reps)
    if a.speculative:
        speculative_arms(model, a.speculative, a.text_len, a.reps)
    if a.batched and not a.lookup:
        batched_arms(model, a.batched, a.max_batch_size, a.text_len, a.reps, a.n1, a.n2)
    if a.processors:
        processor_arms(model, [int(x) for x in a.processors_only.split(",")] if a.processors_only else [1, 8], a.text_len, a.reps,
                       a.n1, a.n2, a.device_arm_only)
    if a.constraint:
        constraint_arms(model, [int(x) for x in a.constraint_only.split(",")] if a.constraint_only else [1, 8], a.text_len, a.reps,
                        a.n1, a.n2)
    if a.constraint_draft:
        constraint_draft_arms(model, a.constraint_draft, [int(x) for x in a.constraint_only.split(",")] if a.constraint_only else [1, 8],
                              a.text_len, a.reps)
    if not a.sample:
        return
    arms = (True,) if a.device_arm_only else (True, False)
    for B in ([int(x) for x in a.sample_only.split(",")] if a.sample_only else [1, 8]):
        pr = prompts(B, a.text_len)
        for sm in SAMPLE_ARMS:
            t1, t2 = {d: [] for d in arms}, {d: [] for d in arms}
            for rep in range(a.reps + 1):                          # rep 0 warms both arms at both lengths
                for d in arms:
                    model.sample_on_device = d
                    x, y = timed(model, pr, 1, a.n1, sm), timed(model, pr, 1, a.n2, sm)
                    if rep:
                        t1[d].append(x)
                        t2[d].append(y)
            del model.sample_on_device
            rec = {"metric": "generate_sampling_ms_per_new_token", "B": B, **sm, "prompt_positions": a.text_len - 1 + 576,
                   "n1": a.n1, "n2": a.n2}
            for d in arms:
                per = [(y - x) / (a.n2 - a.n1) for x, y in zip(t1[d], t2[d])]
                name = "device" if d else "torch"
                rec[f"ms_per_token_{name}"] = round(min(per), 3)
                rec[f"ms_per_token_{name}_all"] = [round(v, 3) for v in per]
            print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
