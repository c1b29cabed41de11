"""Beam-search bookkeeping (llavamod.generation) against HF's own `generate(num_beams=...)` on the CPU: a tiny random
transformers.Qwen2ForCausalLM (fp32, text only) drives the scorer with candidates from torch log_softmax + topk over the
cache-free forward of the running beams, and must return HF's sequences and sequence scores."""
import itertools
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "llava-mod_amd"))

from llavamod.generation import BeamSearchScorer, check_beam_args  # noqa: E402

transformers = pytest.importorskip("transformers")

V, B, P, N_NEW, PAD = 96, 2, 5, 7, 3


@pytest.fixture(scope="module")
def tiny():
    cfg = transformers.Qwen2Config(vocab_size=V, hidden_size=32, intermediate_size=64, num_hidden_layers=2,
                                   num_attention_heads=4, num_key_value_heads=2, max_position_embeddings=64,
                                   tie_word_embeddings=False)
    torch.manual_seed(0)
    model = transformers.Qwen2ForCausalLM(cfg).eval()
    with torch.no_grad():
        for p in model.parameters():
            p.normal_(0.0, 0.5 if p.dim() > 1 else 0.1)            # peaked distributions: beams really diverge
    ids = torch.randint(10, V, (B, P), generator=torch.Generator().manual_seed(1))
    with torch.no_grad():
        greedy = model.generate(input_ids=ids, attention_mask=torch.ones_like(ids), max_new_tokens=4, do_sample=False,
                                num_beams=1, pad_token_id=PAD)[:, P:]
    eos = int(greedy[0, 2])                                          # a token the model emits early
    return model, ids, eos


def drive_scorer(model, ids, nb, max_new, eos, pad, **kw):
    """Our scorer on candidates from the model's cache-free forward over the running beams."""
    Bn = ids.shape[0]
    sc = BeamSearchScorer(Bn, nb, max_new, eos_token_id=eos, pad_token_id=pad, **kw)
    rows = ids.repeat_interleave(nb, 0)
    beam_scores = sc.initial_beam_scores()
    while True:
        with torch.no_grad():
            lg = model(input_ids=rows).logits[:, -1].float()
        lp = torch.log_softmax(lg, -1) + beam_scores[:, None]
        vals, idx = torch.topk(lp.reshape(Bn, nb * lg.shape[-1]), 2 * nb)
        tok, src, beam_scores = sc.step(vals, idx // lg.shape[-1], idx % lg.shape[-1])
        if sc.is_done:
            return sc
        rows = torch.cat([rows[src], tok[:, None]], 1)


MATRIX = [(nb, lp, es, nrs) for nb, lp, es in itertools.product((2, 4, 8), (0.0, 1.0, 2.0), (False, True))
          for nrs in sorted({1, nb})]


@pytest.mark.parametrize("nb,lp,es,nrs", MATRIX)
def test_scorer_matches_hf_beam_search(tiny, nb, lp, es, nrs):
    model, ids, eos = tiny
    with torch.no_grad():
        hf = model.generate(input_ids=ids, attention_mask=torch.ones_like(ids), max_new_tokens=N_NEW, do_sample=False,
                            num_beams=nb, length_penalty=lp, early_stopping=es, num_return_sequences=nrs, eos_token_id=eos,
                            pad_token_id=PAD, return_dict_in_generate=True, output_scores=True)
    sc = drive_scorer(model, ids, nb, N_NEW, eos, PAD, length_penalty=lp, early_stopping=es)
    seq, scores = sc.finalize(nrs)
    want = hf.sequences[:, P:]
    assert seq.shape == want.shape and seq.dtype == torch.int64, (seq.shape, want.shape)
    assert torch.equal(seq, want), (seq, want)
    assert scores.dtype == torch.float32
    assert torch.allclose(scores, hf.sequences_scores.float(), atol=1e-5, rtol=0), (scores, hf.sequences_scores)


def test_some_hypothesis_ends_early(tiny):
    """The fixture EOS really ends hypotheses before max_new_tokens (otherwise the matrix would not test EOS admission)."""
    model, ids, eos = tiny
    ended = 0
    for nb in (2, 4, 8):
        seq, _ = drive_scorer(model, ids, nb, N_NEW, eos, PAD).finalize(nb)
        for row in seq:
            hit = (row == eos).nonzero()
            ended += int(len(hit) > 0 and int(hit[0]) < N_NEW - 1)
    assert ended > 0


def test_argument_errors():
    with pytest.raises(ValueError, match="beam sampling"):
        check_beam_args(4, do_sample=True)
    for nb in (1, 9, 2.0):
        with pytest.raises(ValueError, match="num_beams"):
            check_beam_args(nb)
    for n in (0, 5):
        with pytest.raises(ValueError, match="num_return_sequences"):
            check_beam_args(4, num_return_sequences=n)
    with pytest.raises(ValueError, match="early_stopping"):
        check_beam_args(4, early_stopping="never")
    with pytest.raises(ValueError, match="max_new_tokens"):
        BeamSearchScorer(1, 2, 0)
    sc = BeamSearchScorer(1, 2, 3)
    with pytest.raises(ValueError, match="num_return_sequences"):
        sc.finalize(3)
