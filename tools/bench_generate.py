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
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_generate.py measures on the GPU"
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
