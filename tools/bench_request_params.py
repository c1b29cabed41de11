"""ms per decode step of generate_batch at the teacher's geometry, max_batch_size slots all live: the call-wide sampling arguments
(`call`: the per-call kernels, the path of a call without `params`) against the same arguments given per request
(`params`: generation.RequestParams on every request -> the per-row kernels).  A step's cost is the difference of two calls that
differ only in max_new_tokens, so the admission prefill cancels.  The arms are interleaved, every repeat is kept; one JSON line.
Runs on a checkout without RequestParams too (the `call` arm only), which is how the parent commit is measured.

    python tools/bench_request_params.py > profiles/request_params.jsonl
    rocprofv3 --kernel-trace --stats -- python tools/bench_request_params.py --arm params --reps 1       # kernel time per step
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "llava-mod_amd"))

import torch  # noqa: E402

SAMPLE = dict(temperature=0.2, top_p=0.7)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--max-batch-size", type=int, default=8)
    ap.add_argument("--text-len", type=int, default=125, help="text tokens incl. the image placeholder (+575 -> prompt length)")
    ap.add_argument("--n1", type=int, default=4)
    ap.add_argument("--n2", type=int, default=36)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--arm", default=None, help="call / params: that arm only")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_request_params.py measures on the GPU"
    from bench import teacher_cfg
    from llavamod import generation
    from llavamod.model import LlavaQwen2ForCausalLM
    from tools.bench_generate import prompts
    model = LlavaQwen2ForCausalLM(teacher_cfg(), device="cuda")
    model.eval()
    B = a.max_batch_size
    pr = prompts(B, a.text_len)
    arms = ["call"] + (["params"] if hasattr(generation, "RequestParams") else [])
    if a.arm:
        assert a.arm in arms, (a.arm, arms)
        arms = [a.arm]

    def run(arm, n_new):
        reqs = [dict(input_ids=pr["input_ids"][i], images=pr["images"][i:i + 1], max_new_tokens=n_new) for i in range(B)]
        kw = dict(do_sample=True, seed=0, **SAMPLE)
        if arm == "params":
            for rq in reqs:
                rq["params"] = generation.RequestParams(do_sample=True, **SAMPLE)
            kw = dict(seed=0)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = model.generate_batch(reqs, max_batch_size=B, **kw)
        e1.record()
        torch.cuda.synchronize()
        assert [len(s) for s in out] == [n_new] * B
        return e0.elapsed_time(e1)

    steps = {arm: [] for arm in arms}
    for rep in range(a.reps + 1):                                  # rep 0 warms every arm
        for arm in arms:
            t1, t2 = run(arm, a.n1), run(arm, a.n2)
            if rep:
                steps[arm].append((t2 - t1) / (a.n2 - a.n1))
    print(json.dumps({
        "metric": "generate_batch_ms_per_decode_step", "max_batch_size": B, "prompt_positions": a.text_len - 1 + 576,
        "sampling": SAMPLE, "n1": a.n1, "n2": a.n2,
        **{f"ms_{arm}_median": round(statistics.median(v), 4) for arm, v in steps.items() if v},
        **{f"ms_{arm}_all": [round(x, 4) for x in v] for arm, v in steps.items()}}), flush=True)


if __name__ == "__main__":
    main()
