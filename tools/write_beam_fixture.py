"""Write tests/golden/ref_beam.safetensors: beam search (num_beams 4, 2 returned sequences) of the IMPORTED reference model on the
checkpoint it wrote (tests/golden/ref_ckpt).  Authoring machine only (CPU, needs the reference sources, which never reach the
GPU machine); the GPU test tests/test_beam_gpu.py::test_beam_reproduces_reference_fixture reads the file this writes.

The reference is imported the way oracle/validate_vs_reference.py does it (that module is imported, not edited).  Its own
forward runs cache-free on the growing right-padded batch of every running beam, as oracle/validate_vs_reference.py::ref_greedy
does for greedy decoding; llavamod.generation's scorer takes the candidates (fp32 log_softmax + beam score, stable descending
sort: ties by the smaller beam * V + token, the device kernel's order).  Among seeded ragged prompt batches it keeps those whose
best beam differs from the greedy continuation and picks the one whose beam decisions have the largest smallest margin:

  margin of a step (per sample) = min( score gap at the cut between rank nb and rank nb + 1 of the sorted candidates,
                                       for every EOS candidate admitted this step: the gap between its length-normalised score
                                       and its nearest neighbour in the merged finished list ).

    python tools/write_beam_fixture.py            # rewrites tests/golden/ref_beam.safetensors (byte-identical on rerun)
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from oracle import validate_vs_reference as VR  # noqa: E402  (its reference import owns the name `llavamod`)

CKPT = os.path.join(ROOT, "tests", "golden", "ref_ckpt")
OUT = os.path.join(ROOT, "tests", "golden", "ref_beam.safetensors")
NB, NRS, N_NEW, N_IMG = 4, 2, 6, 4          # 28 px / patch 14: 4 patch rows replace the one -200 placeholder


def _scorer_module():
    """llavamod/generation.py of THIS repository, loaded by path (the name `llavamod` belongs to the imported reference)."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("lmod_generation", os.path.join(ROOT, "llava-mod_amd", "llavamod", "generation.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def load_reference(R):
    """The reference's LlavaQwen2ForCausalLM with the weights it saved to tests/golden/ref_ckpt."""
    from types import SimpleNamespace
    from safetensors.torch import load_file
    _, _, tc = VR.small_gpu_cfgs()
    cwd = os.getcwd()
    os.chdir(CKPT)                                   # the tower is named relative to the checkpoint
    try:
        ref = R.lq.LlavaQwen2ForCausalLM(VR.ref_qwen2_config(R, tc, "eager"))
        margs = SimpleNamespace(image_tower="openai_clip_tiny", video_tower=None, mm_vision_select_layer=-2,
                                mm_vision_select_feature="patch", pretrain_mm_mlp_adapter=None, image_projector_type="mlp2x_gelu",
                                video_projector_type="linear", video_global_proj=False, video_temproal_proj=False,
                                video_spatial_proj=False)
        ref.get_model().initialize_vision_modules(margs, fsdp=None)
        res = ref.load_state_dict(load_file("model.safetensors"), strict=False)
    finally:
        os.chdir(cwd)
    assert not [m for m in res.missing_keys if "rotary" not in m and "position_ids" not in m], res.missing_keys
    assert not res.unexpected_keys, res.unexpected_keys
    return ref.eval()


def last_logits(ref, seqs, images):
    """fp32 logits at every sequence's last real position (right-padded batch, cache-free reference forward)."""
    T = max(len(q) for q in seqs)
    bi = torch.zeros(len(seqs), T, dtype=torch.long)
    bm = torch.zeros(len(seqs), T, dtype=torch.bool)
    for i, q in enumerate(seqs):
        bi[i, :len(q)] = q
        bm[i, :len(q)] = True
    with torch.no_grad():
        lg = ref(input_ids=bi, attention_mask=bm, images=list(images), return_dict=True).logits
    return torch.stack([lg[i, len(q) - 1 + N_IMG - 1].float() for i, q in enumerate(seqs)])


def ref_beam(G, ref, ids, mask, images, eos, pad):
    """Beam search of the reference forward through llavamod.generation: (tokens [B*NRS, L], scores [B*NRS], margins [B, steps],
    length of every sample's best hypothesis [B])."""
    B = ids.shape[0]
    sc = G.BeamSearchScorer(B, NB, N_NEW, eos_token_id=eos, pad_token_id=pad)
    prompts = [ids[i, :int(mask[i].sum())] for i in range(B)]
    seqs = [prompts[i // NB].clone() for i in range(B * NB)]
    ims = images.repeat_interleave(NB, 0)
    beam_scores = sc.initial_beam_scores()
    margins = []
    while True:
        lg = last_logits(ref, seqs, ims)
        V = lg.shape[-1]
        flat = (torch.log_softmax(lg, -1) + beam_scores[:, None]).reshape(B, NB * V)
        vals, idx = torch.sort(flat, dim=-1, descending=True, stable=True)
        vals, idx = vals[:, :2 * NB], idx[:, :2 * NB]
        old_scores, old_fin = sc.scores.clone(), sc.finished.clone()
        tok, src, beam_scores = sc.step(vals, idx // V, idx % V)
        mrow = []
        for b in range(B):
            m = float(vals[b, NB - 1] - vals[b, NB])
            for j in range(NB):
                if int(idx[b, j] % V) == eos:
                    s = float(vals[b, j]) / (sc.t ** sc.length_penalty)
                    others = [float(x) for x, f in zip(old_scores[b], old_fin[b]) if f]
                    others += [float(vals[b, k]) / (sc.t ** sc.length_penalty) for k in range(NB)
                               if k != j and int(idx[b, k] % V) == eos]
                    if others:
                        m = min(m, min(abs(s - o) for o in others))
            mrow.append(m)
        margins.append(mrow)
        if sc.is_done:
            break
        seqs = [torch.cat([seqs[int(s)], t.reshape(1)]) for s, t in zip(src, tok)]
    tokens, scores = sc.finalize(NRS)
    return tokens, scores, torch.tensor(margins).t().contiguous(), sc.lens[:, 0].clone()


def main(tries=1500, out=OUT):
    torch.set_num_threads(1)                       # fixed reduction order: the file is rewritten byte for byte
    G = _scorer_module()
    R = VR._import_reference()
    ref = load_reference(R)
    pad = 511
    best, kept = None, 0
    for seed in range(300, 300 + tries):
        b = VR.tiny_batch(seed=seed, B=2, T=12, ragged=True)
        im = b["images"].to(torch.bfloat16).float()
        greedy, _ = VR.ref_greedy(ref, b["input_ids"], b["attention_mask"], im, N_NEW)
        eos = int(greedy[0, 2])                    # a token the model emits early: beams end before max_new_tokens
        toks, scores, mg, best_len = ref_beam(G, ref, b["input_ids"], b["attention_mask"], im, eos, pad)
        if all(torch.equal(toks[i * NRS, :n], greedy[i, :n]) for i, n in enumerate(best_len.tolist())):
            continue
        kept += 1
        if best is None or float(mg.min()) > best[0]:
            best = (float(mg.min()), seed, b, im, eos, toks, scores, mg, greedy)
    assert best is not None, "no prompt whose best beam differs from the greedy continuation"
    mmin, seed, b, im, eos, toks, scores, mg, greedy = best
    print(f"beam fixture: {kept} of {tries} prompts differ from greedy; prompt seed {seed}, eos {eos}, smallest decision margin {mmin:.4f}\n  tokens {toks.tolist()}\n"
          f"  scores {scores.tolist()}\n  greedy {greedy.tolist()}")
    from safetensors.torch import save_file
    save_file({"input_ids": b["input_ids"], "attention_mask": b["attention_mask"].to(torch.int64), "images": im,
               "tokens": toks, "scores": scores, "margins": mg, "greedy": greedy,
               "params": torch.tensor([NB, NRS, N_NEW, eos, pad], dtype=torch.int64)}, out)
    print(f"wrote {out}")


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--tries", type=int, default=1500, help="seeded prompt batches searched")
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    main(a.tries, a.out)
