"""Write tests/golden/append_prompt.safetensors: ragged, right-padded prompts with images on which the fp32 oracle's own greedy
continuation stays away from ties — every step's top-2 logit gap is at least MARGIN = 1.5 x 8 bf16 ulps (headroom for the bf16 path's own noise) of the top logit — so that token
equality across two kernel paths (tests/test_append_gpu.py, tests/test_assisted_gpu.py) is meaningful.  One prompt for the golden small
teacher (9 steps), one for the student (8 steps, drop-free capacity), and a text-only two-turn prompt for the teacher.  Uses the oracle only (CPU).   python tools/make_append_fixture.py"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _util as U  # noqa: E402
from _attn_ref import ulp_bf16  # noqa: E402
from test_step_parity_gpu import _oracle_pair_from, small_cfgs  # noqa: E402

STEPS, MARGIN, STUDENT_MARGIN, B, T = 9, 1.5, 1.5, 2, 12


def min_gap(oracle, ids, mask, images, n_img, steps, margin=MARGIN):
    """Greedy continuation with the oracle (full recomputation); the smallest top-2 gap over all steps in units of 8 bf16 ulps."""
    ids, mask = ids.clone(), mask.clone()
    plen = mask.sum(1)
    ids = torch.cat([ids, torch.zeros(B, steps, dtype=ids.dtype)], 1)
    mask = torch.cat([mask, torch.zeros(B, steps, dtype=torch.bool)], 1)
    worst = float("inf")
    for s in range(steps):
        with torch.no_grad():
            lg = oracle(input_ids=ids, attention_mask=mask, images=images).logits
        last = mask.sum(1) + n_img - 1
        row = lg[torch.arange(B), last].float()
        t2 = row.topk(2, -1).values
        worst = min(worst, float(((t2[:, 0] - t2[:, 1]) / (8 * ulp_bf16(t2[:, 0]))).min()))
        if worst < margin:
            return worst
        tok = row.argmax(-1)
        for b in range(B):
            ids[b, int(plen[b]) + s] = tok[b]
            mask[b, int(plen[b]) + s] = True
    return worst


def text_greedy(oracle, ids, steps):
    """Text-only greedy continuation of equal-length rows: (tokens [B, steps], smallest top-2 gap in units of 8 bf16 ulps)."""
    worst, out = float("inf"), []
    for _ in range(steps):
        with torch.no_grad():
            row = oracle(input_ids=ids).logits[:, -1].float()
        t2 = row.topk(2, -1).values
        worst = min(worst, float(((t2[:, 0] - t2[:, 1]) / (8 * ulp_bf16(t2[:, 0]))).min()))
        out.append(row.argmax(-1))
        ids = torch.cat([ids, out[-1][:, None]], 1)
    return torch.stack(out, 1), worst


def two_turn(o_teacher, vocab):
    """A text-only first prompt [2, 9] and second-turn text [2, 7] on which the teacher's 5 first-turn steps and the 8 steps after the
    second turn are all tie-free."""
    for seed in range(200000):
        g = torch.Generator().manual_seed(1000000 + seed)
        ids, turn2 = torch.randint(0, vocab - 8, (2, 9), generator=g), torch.randint(0, vocab - 8, (2, 7), generator=g)
        t1, g1 = text_greedy(o_teacher, ids, 5)
        if g1 < MARGIN:
            continue
        _, g2 = text_greedy(o_teacher, torch.cat([ids, t1, turn2], 1), 8)
        if g2 >= MARGIN:
            print(f"two-turn seed {seed}: {g1:.2f} / {g2:.2f} (x 8 bf16 ulps)")
            return ids, turn2
    raise SystemExit("no two-turn seed found")


def prompt(seed, vocab, img):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(0, vocab - 8, (B, T), generator=g)
    ids[:, 2] = -200
    mask = torch.ones(B, T, dtype=torch.bool)
    for b in range(1, B):
        mask[b, T - 2 * b:] = False
        ids[b, T - 2 * b:] = vocab - 1
    images = torch.randn(B, 3, img, img, generator=g).to(torch.bfloat16).float()
    return ids, mask, images


def search(oracle, name, vocab, img, n_img, steps, margin, seeds):
    """The first seed whose prompt keeps `oracle`'s greedy continuation at least margin x 8 bf16 ulps away from a tie for `steps` steps."""
    for seed in seeds:
        ids, mask, images = prompt(seed, vocab, img)
        gap = min_gap(oracle, ids, mask, images, n_img, steps, margin)
        if gap >= margin:
            print(f"{name}: seed {seed}, smallest top-2 gap {gap:.2f} x 8 bf16 ulps over {steps} steps")
            return seed, ids, mask, images
    raise SystemExit(f"no seed found for the {name}")


def main():
    from safetensors.torch import save_file
    vc, sc, tc = small_cfgs()
    sc.eval_capacity_factor = 64.0
    ssd, tsd = U.load_golden("gpusmall_student.safetensors"), U.load_golden("gpusmall_teacher.safetensors")
    o_student, o_teacher = _oracle_pair_from(ssd, tsd, sc, tc, vc)
    o_student.eval(), o_teacher.eval()
    o_student.set_gate_noise([None])
    n_img = (vc.image_size // vc.patch_size) ** 2 - 1
    # one prompt per model: each search stops at the first seed that meets its margin
    st, ids, mask, images = search(o_teacher, "teacher", tc.vocab_size, vc.image_size, n_img, STEPS, MARGIN, range(100000))
    ss, s_ids, s_mask, s_images = search(o_student, "student", sc.vocab_size, vc.image_size, n_img, 8, STUDENT_MARGIN, range(100000, 200000))
    tt_ids, tt_turn2 = two_turn(o_teacher, tc.vocab_size)
    save_file(dict(two_turn_ids=tt_ids, two_turn_next=tt_turn2, input_ids=ids, attention_mask=mask.to(torch.uint8),
                   images=images.to(torch.bfloat16), student_input_ids=s_ids, student_attention_mask=s_mask.to(torch.uint8),
                   student_images=s_images.to(torch.bfloat16)),
              os.path.join(U.GOLD, "append_prompt.safetensors"), metadata=dict(seed=str(st), student_seed=str(ss)))


if __name__ == "__main__":
    main()
