"""Beam search on the device: lmod_beam_topk_bf16 against torch (fp32 log_softmax + beam score, stable descending sort),
lmod_kv_gather_rows against index_select, generate(num_beams > 1) with the KV cache against the same scorer driven by cache-free
recomputation, and the reference model's own beam search (tests/golden/ref_beam.safetensors, written by
tools/write_beam_fixture.py from the imported reference) reproduced from the checkpoint it wrote."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "llava-mod_amd"))

from test_generate_gpu import _pair, _prompt  # noqa: E402

DEV = "cuda"
BF = torch.bfloat16
REF_CKPT = os.path.join(ROOT, "tests", "golden", "ref_ckpt")
REF_BEAM = os.path.join(ROOT, "tests", "golden", "ref_beam.safetensors")


def _torch_candidates(logits, beam_scores, nb):
    """Reference candidates: fp32 log_softmax + beam score, flattened per sample, stable descending sort, top 2*nb."""
    R, V = logits.shape
    lp = torch.log_softmax(logits.float(), -1) + beam_scores.float()[:, None]
    flat = lp.reshape(R // nb, nb * V)
    vals, idx = torch.sort(flat, dim=-1, descending=True, stable=True)
    return flat, vals[:, :2 * nb], idx[:, :2 * nb], torch.logsumexp(logits.float(), -1)


@pytest.mark.parametrize("V,ld", [(512, 512), (1000, 1000), (1001, 1001), (1003, 1008), (151936, 151936), (151936, 152064),
                                  (152064, 152064)])
@pytest.mark.parametrize("nb", [1, 2, 4, 8])
@pytest.mark.parametrize("B", [1, 3, 16])
def test_beam_topk_vs_torch(V, ld, nb, B):
    from llavamod import kernels as K
    from llavamod.generation import unpack_candidates
    if V > 2000 and B * nb > 32:
        B = max(1, 32 // nb)                          # keep the torch reference's sort within reason
    g = torch.Generator(device=DEV).manual_seed(V + 7 * nb + B)
    full = (3.0 * torch.randn(B * nb, ld, device=DEV, generator=g)).to(BF)
    logits = full[:, :V]
    for first in (True, False):
        if first:                                     # first step: [0, -1e9, ...] per sample
            bs = torch.full((B, nb), -1e9, device=DEV)
            bs[:, 0] = 0.0
            bs = bs.reshape(-1).contiguous()
        else:
            bs = -20.0 * torch.rand(B * nb, device=DEV, generator=g)
        s, b, t = unpack_candidates(K.beam_topk(logits, bs, nb))
        flat, rv, ri, lse = _torch_candidates(logits, bs, nb)
        tol = 2e-6 * lse.abs().max().item() + 1e-6
        assert torch.all(s[:, :-1] >= s[:, 1:]), "candidates not sorted"
        err = (s - rv).abs().max().item()
        assert err <= tol, (err, tol)
        got = b.long() * V + t.long()
        assert torch.all((b >= 0) & (b < nb) & (t >= 0) & (t < V))
        for i in range(B):
            kth = rv[i, -1].item()
            sg, sr = set(got[i].tolist()), set(ri[i].tolist())
            for f in sg ^ sr:                         # only near-ties at the cut may differ
                assert abs(flat[i, f].item() - kth) <= tol, (i, f, flat[i, f].item(), kth)
            exact = [f for f in got[i].tolist() if abs(flat[i, f].item() - kth) > tol]
            ref_exact = [f for f in ri[i].tolist() if abs(flat[i, f].item() - kth) > tol]
            assert exact == ref_exact, (i, exact, ref_exact)   # order too, ties by the smaller beam*V + token


@pytest.mark.parametrize("width", [128, 4096])
def test_kv_gather_rows_vs_index_select(width):
    from llavamod import kernels as K
    g = torch.Generator(device=DEV).manual_seed(width)
    n_layers, R_src, R, smax_src, smax_dst = 3, 3, 7, 40, 48
    src = [torch.randn(R_src, smax_src, width, device=DEV, generator=g).to(BF) for _ in range(2 * n_layers)]
    poison = torch.full((R, smax_dst, width), -7.0, device=DEV, dtype=BF)
    dst = [poison.clone() for _ in range(2 * n_layers)]
    src_row = torch.tensor([2, 0, 1, 1, 2, 0, 2], device=DEV, dtype=torch.int32)
    lens = torch.tensor([40, 0, 1, 17, 33, 39, 8], device=DEV, dtype=torch.int32)
    K.kv_gather_rows(dst, src, src_row, lens)
    for d, s in zip(dst, src):
        want = s.index_select(0, src_row.long())
        for r in range(R):
            n = int(lens[r])
            assert torch.equal(d[r, :n], want[r, :n]), r
            assert torch.equal(d[r, n:], poison[r, n:]), r


def _recompute_beam(model, pr, nb, max_new, eos, pad):
    """The scorer driven by the model's cache-free forward over every running beam (prompt + generated tokens), re-run each
    step.  Returns (scorer, smallest cut margin per step)."""
    from llavamod.generation import BeamSearchScorer
    ids, mask = pr["input_ids"], pr["attention_mask"]
    B = ids.shape[0]
    P = model.get_image_tower().num_patches
    sc = BeamSearchScorer(B, nb, max_new, eos_token_id=eos, pad_token_id=pad)
    seqs = [ids[i // nb, :int(mask[i // nb].sum())].clone() for i in range(B * nb)]
    images = pr["images"].repeat_interleave(nb, 0)
    beam_scores = sc.initial_beam_scores().to(DEV)
    margins = []
    while True:
        T = max(len(q) for q in seqs)
        bi = torch.zeros(len(seqs), T, dtype=ids.dtype)
        bm = torch.zeros(len(seqs), T, dtype=torch.bool)
        for i, q in enumerate(seqs):
            bi[i, :len(q)] = q
            bm[i, :len(q)] = True
        with torch.no_grad():
            lg = model(input_ids=bi, attention_mask=bm, images=images).logits
        last = torch.tensor([len(q) - 1 + P - 1 for q in seqs], device=DEV)
        rows = lg[torch.arange(len(seqs), device=DEV), last]
        _, vals, idx, _ = _torch_candidates(rows, beam_scores, nb)
        V = rows.shape[-1]
        margins.append((vals[:, nb - 1] - vals[:, nb]).min().item())
        tok, src, bs = sc.step(vals.cpu(), (idx // V).cpu(), (idx % V).cpu())
        if sc.is_done:
            return sc, margins
        beam_scores = bs.to(DEV)
        seqs = [torch.cat([seqs[int(s)], t.reshape(1)]) for s, t in zip(src, tok)]


@pytest.mark.parametrize("which", ["teacher", "student"])
def test_beam_generate_with_kv_cache_equals_recomputation(which):
    """generate(num_beams=4, num_return_sequences=2) on the cache (beam_topk + kv_gather_rows + decode steps) == the same scorer on
    candidates from the full forward without cache, re-run every step.  Right-padded ragged prompts.  (The MoE student with
    drop-free capacity, as in the greedy test: a decode step routes B*nb tokens, the recomputation routes them all.)"""
    student, teacher = _pair()
    model = teacher if which == "teacher" else student
    if which == "student":
        for m in model.moe_layers():
            m.eval_capacity_factor = 64.0
    model.eval()
    pr = _prompt()
    greedy = model.generate(**pr, max_new_tokens=6)
    eos, pad = int(greedy[0, 2]), 0
    out = model.generate(**pr, max_new_tokens=6, num_beams=4, num_return_sequences=2, eos_token_id=eos, pad_token_id=pad,
                         return_dict_in_generate=True)
    sc, margins = _recompute_beam(model, pr, 4, 6, eos, pad)
    want, want_scores = sc.finalize(2)
    print(f"{which}: beams {out.sequences.tolist()} scores {out.sequences_scores.tolist()}; smallest cut margin per step "
          f"{[round(m, 4) for m in margins]}")
    assert out.sequences.dtype == torch.int64 and out.sequences_scores.dtype == torch.float32
    assert torch.equal(out.sequences.cpu(), want), (out.sequences.cpu(), want)
    assert torch.allclose(out.sequences_scores.cpu(), want_scores, atol=3e-2, rtol=0), (out.sequences_scores, want_scores)
    # model state: generate restores training mode and never touches parameters
    assert not model.training
    model.train()
    model.generate(**pr, max_new_tokens=2, num_beams=2)
    assert model.training


def test_num_beams_one_is_greedy_and_beam_sampling_is_refused():
    _, teacher = _pair()
    pr = _prompt()
    greedy = teacher.generate(**pr, max_new_tokens=6)
    assert torch.equal(teacher.generate(**pr, max_new_tokens=6, num_beams=1), greedy)
    with pytest.raises(ValueError, match="beam sampling"):
        teacher.generate(**pr, max_new_tokens=2, num_beams=4, do_sample=True)
    with pytest.raises(ValueError, match="num_return_sequences"):
        teacher.generate(**pr, max_new_tokens=2, num_beams=2, num_return_sequences=3)


def _ref_model():
    from llavamod.model import LlavaQwen2ForCausalLM
    return LlavaQwen2ForCausalLM.from_pretrained(REF_CKPT, attn_implementation="flash_attention_2", torch_dtype=BF, device=DEV)


def _fixture():
    from safetensors.torch import load_file
    f = load_file(REF_BEAM)
    nb, nrs, n_new, eos, pad = f["params"].tolist()
    pr = dict(input_ids=f["input_ids"], attention_mask=f["attention_mask"].bool(), images=f["images"].to(DEV).to(BF))
    return f, pr, dict(num_beams=nb, num_return_sequences=nrs, max_new_tokens=n_new, eos_token_id=eos, pad_token_id=pad)


def test_beam_output_differs_from_greedy():
    """num_beams is honoured: on the fixture prompt the best beam is not the greedy continuation (an implementation that drops
    num_beams returns the greedy tokens, one row per sample)."""
    model = _ref_model()
    f, pr, kw = _fixture()
    greedy = model.generate(**pr, max_new_tokens=kw["max_new_tokens"])
    out = model.generate(**pr, **kw)
    B, nrs = pr["input_ids"].shape[0], kw["num_return_sequences"]
    assert out.shape[0] == B * nrs, out.shape
    best = out[::nrs]
    assert not torch.equal(best[:, :greedy.shape[1]].cpu(), greedy.cpu()[:, :best.shape[1]]) or best.shape[1] != greedy.shape[1]
    assert torch.equal(greedy.cpu(), f["greedy"]), (greedy.cpu(), f["greedy"])


def test_beam_reproduces_reference_fixture():
    """from_pretrained(ref_ckpt).generate(num_beams=4, num_return_sequences=2, eos) == the beam search the imported reference
    model's own forward produced (tools/write_beam_fixture.py), token for token; the decision margins travel with the tokens."""
    model = _ref_model()
    f, pr, kw = _fixture()
    out = model.generate(**pr, **kw, return_dict_in_generate=True)
    want, margins = f["tokens"], f["margins"]
    print(f"reference beams {want.tolist()} scores {f['scores'].tolist()}, smallest decision margin {margins.min().item():.4f}; "
          f"generate() -> {out.sequences.tolist()} {out.sequences_scores.tolist()}")
    assert out.sequences.shape == want.shape and out.sequences.dtype == torch.int64
    assert torch.equal(out.sequences.cpu(), want), (out.sequences.cpu(), want, margins)
    assert torch.allclose(out.sequences_scores.cpu(), f["scores"], atol=3e-2, rtol=0)
