"""ms per new token of generate() at the teacher's geometry (Qwen1.5-7B decoder + CLIP-ViT-L/14-336 tower, random bf16 weights):
greedy (num_beams 1) and beam search (num_beams 4), prompts of 576 image rows + text (~700 positions).  The decode rate is the
difference of two generate() calls of N1 and N2 new tokens (device events, after a warm-up of each), so the prefill cancels:
ms/token = (t(N2) - t(N1)) / (N2 - N1).  One JSON line per (B, num_beams).

    python tools/bench_generate.py                       # B in {1, 4, 8} x num_beams in {1, 4}
    python tools/bench_generate.py --only 1x4 --reps 1   # one configuration (for a rocprofv3 --kernel-trace --stats run)
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


def timed(model, pr, nb, n_new):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    kw = dict(num_beams=nb) if nb > 1 else {}
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
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_generate.py measures on the GPU"
    from bench import teacher_cfg
    from llavamod.model import LlavaQwen2ForCausalLM
    model = LlavaQwen2ForCausalLM(teacher_cfg(), device="cuda")
    model.eval()
    cfgs = [(1, 1), (1, 4), (4, 1), (8, 1), (8, 4)]
    if a.only:
        cfgs = [tuple(int(x) for x in c.split("x")) for c in a.only.split(",")]
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


if __name__ == "__main__":
    main()
