"""Beam-search bookkeeping of `generate(num_beams > 1)` and the argument checks / result object of sampling, in plain torch (no
kernels, importable without the HIP library).

The semantics are HF `GenerationMixin._beam_search` (do_sample=False) of transformers 5.x, the version this project can run:
  * running beam scores start as [0, -1e9, ...] per sample; a step's candidates are the top 2*nb of
    log_softmax(logits) + beam score over nb*V per sample, sorted by score (descending);
  * a candidate "hits" when its token is EOS, or on the last step (max_new_tokens) for every candidate;
  * the best nb candidates that do not hit continue (their un-normalised score is the new beam score);
  * a hitting candidate ranked below nb is dropped; one ranked within nb enters the sample's finished list (nb slots) with
    score sum_logprobs / n_generated ** length_penalty (n_generated counts the EOS), unless the sample is closed (its early-stop
    heuristic is satisfied, or early_stopping=True and all nb slots are full);
  * the heuristic closes a sample once every slot is full and the best running score / n_generated ** length_penalty
    cannot beat the worst finished score; the search ends when every sample is closed, when early_stopping=True and every
    slot of every sample is full, or at max_new_tokens.
Where transformers 4.37's BeamSearchScorer differs, this follows 5.x: at max_new_tokens 4.37 finalises the nb running beams
chosen after that step (the best non-EOS candidates, even below rank nb), 5.x admits the top nb candidates of the last step
themselves.  Length normalisation counts generated tokens only, so right padding of the prompt never changes a score.

Per step the caller hands over a candidate block [B, 2*nb] (score fp32, beam in 0..nb-1, token) and gets back the next tokens
[B*nb], the flat source rows [B*nb] (cache row b*nb + beam) and the new running beam scores [B*nb].
"""
import torch

NEG = -1.0e9


def check_beam_args(num_beams, num_return_sequences=1, do_sample=False, length_penalty=1.0, early_stopping=False):
    if do_sample:
        raise ValueError("beam sampling (do_sample=True with num_beams > 1) is not supported: use do_sample=False for beam "
                         "search or num_beams=1 for sampling")
    if not isinstance(num_beams, int) or not 2 <= num_beams <= 8:
        raise ValueError(f"num_beams must be an int in 2..8 for beam search, got {num_beams!r}")
    if not isinstance(num_return_sequences, int) or not 1 <= num_return_sequences <= num_beams:
        raise ValueError(f"num_return_sequences must be in 1..num_beams ({num_beams}), got {num_return_sequences!r}")
    if early_stopping not in (False, True):
        raise ValueError(f"early_stopping must be False or True, got {early_stopping!r}")
    float(length_penalty)


def check_sample_args(do_sample=False, temperature=1.0, top_k=None, top_p=None, num_return_sequences=1):
    """Arguments of `generate(num_beams=1)`: greedy returns one sequence per prompt (HF raises for more); sampling needs
    temperature > 0, top_k None or a positive int, top_p None or in (0, 1]."""
    n = num_return_sequences
    if isinstance(n, bool) or not isinstance(n, int) or n < 1:
        raise ValueError(f"num_return_sequences must be an int >= 1, got {n!r}")
    if not do_sample:
        if n != 1:
            raise ValueError(f"greedy decoding returns one sequence per prompt: num_return_sequences={n} needs do_sample=True "
                             "or num_beams > 1")
        return
    if isinstance(temperature, bool) or not isinstance(temperature, (int, float)) or not temperature > 0:
        raise ValueError(f"temperature must be a number > 0 when do_sample=True, got {temperature!r}")
    if top_k is not None and (isinstance(top_k, bool) or not isinstance(top_k, int) or top_k < 1):
        raise ValueError(f"top_k must be None or a positive int, got {top_k!r}")
    if top_p is not None and (isinstance(top_p, bool) or not isinstance(top_p, (int, float)) or not 0 < top_p <= 1):
        raise ValueError(f"top_p must be None or in (0, 1], got {top_p!r}")


class BeamSearchScorer:
    """Hypothesis lists, done flags and the early-stop test of a beam search over B samples x nb beams.  All state lives on
    `device` (the host by default: the candidate block is read back once per step)."""

    def __init__(self, batch_size, num_beams, max_new_tokens, length_penalty=1.0, early_stopping=False, eos_token_id=None,
                 pad_token_id=None, device="cpu"):
        check_beam_args(num_beams, 1, False, length_penalty, early_stopping)
        if max_new_tokens < 1:
            raise ValueError("max_new_tokens must be >= 1")
        B, nb = batch_size, num_beams
        self.B, self.nb, self.max_new = B, nb, int(max_new_tokens)
        self.length_penalty, self.early_stopping = float(length_penalty), early_stopping
        self.eos = eos_token_id
        pad = eos_token_id if pad_token_id is None else pad_token_id
        self.pad = 0 if pad is None else int(pad)
        self.device = device
        i64 = dict(dtype=torch.int64, device=device)
        self.running_seq = torch.full((B, nb, self.max_new), self.pad, **i64)
        self.running_scores = torch.zeros((B, nb), dtype=torch.float32, device=device)
        self.running_scores[:, 1:] = NEG
        self.seq = torch.full((B, nb, self.max_new), self.pad, **i64)          # finished hypotheses (nb slots, best first)
        self.scores = torch.full((B, nb), NEG, dtype=torch.float32, device=device)
        self.lens = torch.zeros((B, nb), **i64)
        self.finished = torch.zeros((B, nb), dtype=torch.bool, device=device)
        self.open = torch.ones((B, 1), dtype=torch.bool, device=device)          # early-stop heuristic not yet satisfied
        self.top_nb = torch.arange(2 * nb, device=device) < nb
        self.t = 0                                                              # tokens generated so far
        self.is_done = False

    def initial_beam_scores(self):
        """[B*nb] fp32: 0 for the first beam of every sample, -1e9 for the others (all beams start as the same prompt)."""
        return self.running_scores.reshape(-1).clone()

    @staticmethod
    def _gather(x, idx):
        return torch.gather(x, 1, idx.reshape(idx.shape + (1,) * (x.dim() - 2)).expand(idx.shape + x.shape[2:]))

    def step(self, scores, beams, tokens):
        """scores fp32 [B, 2nb] (log-prob sums, sorted descending per sample), beams / tokens int [B, 2nb].
        Returns (next_tokens int64 [B*nb], src_rows int64 [B*nb], beam_scores fp32 [B*nb])."""
        if self.is_done:
            raise RuntimeError("beam search already finished")
        B, nb, t = self.B, self.nb, self.t
        dev = self.device
        scores = scores.to(device=dev, dtype=torch.float32)
        beams, tokens = beams.to(device=dev, dtype=torch.int64), tokens.to(device=dev, dtype=torch.int64)
        assert scores.shape == (B, 2 * nb) and beams.shape == scores.shape and tokens.shape == scores.shape
        cand_seq = self._gather(self.running_seq, beams).clone()                   # [B, 2nb, max_new]
        cand_seq[:, :, t] = tokens
        hits = torch.zeros_like(tokens, dtype=torch.bool)
        if self.eos is not None:
            hits |= tokens == int(self.eos)
        if t + 1 >= self.max_new:
            hits[:] = True
        # running beams for the next step: the best nb candidates that do not hit
        run_scores = scores + hits.to(torch.float32) * NEG
        nxt = torch.topk(run_scores, k=nb)[1]
        self.running_seq = self._gather(cand_seq, nxt)
        self.running_scores = self._gather(run_scores, nxt)
        next_tokens = self._gather(tokens, nxt)
        src_rows = self._gather(beams, nxt) + torch.arange(B, device=dev)[:, None] * nb
        # finished hypotheses: candidates ranked within nb that hit, length-normalised, merged with the nb slots
        admitted = hits & self.top_nb[None, :]
        fin = scores / ((t + 1) ** self.length_penalty)
        full = torch.all(self.finished, dim=-1, keepdim=True) & (self.early_stopping is True)
        fin = fin + full.to(torch.float32) * NEG
        fin = fin + (~self.open).to(torch.float32) * NEG
        fin = fin + (~admitted) * NEG
        m_seq = torch.cat((self.seq, cand_seq), 1)
        m_scores = torch.cat((self.scores, fin), 1)
        m_lens = torch.cat((self.lens, torch.full_like(tokens, t + 1)), 1)
        m_fin = torch.cat((self.finished, admitted), 1)
        keep = torch.topk(m_scores, k=nb)[1]
        self.seq, self.scores = self._gather(m_seq, keep), self._gather(m_scores, keep)
        self.lens, self.finished = self._gather(m_lens, keep), self._gather(m_fin, keep)
        # early-stop heuristic and the end of the search
        self.t = t = t + 1
        best = self.running_scores[:, :1] / (t ** self.length_penalty)
        worst = torch.where(self.finished, torch.min(self.scores, dim=1, keepdim=True)[0], NEG)
        self.open = self.open & torch.any(best > worst, dim=-1, keepdim=True)
        improvement_possible = bool(torch.any(self.open))
        open_beam = not (bool(torch.all(self.finished)) and self.early_stopping is True)
        continuations = not bool(torch.all(hits))
        self.is_done = not (improvement_possible and open_beam and continuations)
        return next_tokens.reshape(-1), src_rows.reshape(-1), self.running_scores.reshape(-1).clone()

    def finalize(self, num_return_sequences=1):
        """Best `num_return_sequences` finished hypotheses per sample, best first: (tokens int64 [B*n, L], scores fp32 [B*n]),
        L = the longest returned hypothesis; positions after a hypothesis ends hold pad_token_id (an EOS that ended it stays)."""
        n = int(num_return_sequences)
        if not 1 <= n <= self.nb:
            raise ValueError(f"num_return_sequences must be in 1..{self.nb}")
        seq = self.seq[:, :n].reshape(self.B * n, -1)
        lens = self.lens[:, :n].reshape(-1)
        L = max(int(lens.max()), 1)
        return seq[:, :L].contiguous(), self.scores[:, :n].reshape(-1).clone()


def unpack_candidates(block):
    """The int32 block [3, B, 2nb] of kernels.beam_topk -> (scores fp32, beams, tokens), each [B, 2nb]."""
    return block[0].view(torch.float32), block[1], block[2]


class BeamSearchOutput:
    """`generate(num_beams > 1, return_dict_in_generate=True)`: sequences int64 [B*n, L] (new tokens only, best first per sample)
    and sequences_scores fp32 [B*n] (length-normalised sum of log-probabilities).  past_key_values: the cache of the B*num_beams
    RUNNING beams in their last step's order — NOT aligned with the rows of `sequences` (finalized hypotheses)."""

    def __init__(self, sequences, sequences_scores, past_key_values=None):
        self.sequences, self.sequences_scores, self.past_key_values = sequences, sequences_scores, past_key_values


class SampleOutput:
    """`generate(do_sample=True, return_dict_in_generate=True)`: sequences int64 [B*n, L] (new tokens only, sample b's n
    continuations in rows b*n .. b*n+n-1) and token_logprobs fp32 [B*n, L]: the log-probability of each drawn token under the
    warped (temperature / top-k / top-p) distribution it was drawn from, 0 at positions after a sequence's EOS.  With
    `generate(constraint=...)`: constraint_states int32 [B*n], every row's final automaton state (None otherwise), and the
    log-probabilities are under the masked, warped distribution."""

    def __init__(self, sequences, token_logprobs, past_key_values=None, constraint_states=None):
        self.sequences, self.token_logprobs, self.past_key_values = sequences, token_logprobs, past_key_values
        self.constraint_states = constraint_states


class GreedyOutput:
    """`generate(return_dict_in_generate=True)` without sampling or beams: sequences int64 [B, L] (new tokens only) and the KV cache.
    With `generate(constraint=...)`: constraint_states int32 [B], every row's final automaton state (None otherwise) - the caller
    checks `constraint.accept[state]` on it, for example when max_new_tokens cut an answer short."""

    def __init__(self, sequences, past_key_values=None, constraint_states=None):
        self.sequences, self.past_key_values, self.constraint_states = sequences, past_key_values, constraint_states


# ---------------------------------------------------------------------------------------------- assisted (speculative) decoding
class AssistedOutput:
    """`generate(assistant_model=..., return_dict_in_generate=True)`: sequences int64 [B, L] (new tokens only), num_rounds (draft /
    verify rounds), num_target_forwards (the prefill plus one verification pass per round), num_accepted int64 [B] (draft tokens that
    were emitted) and the target's KV cache (when max_new_tokens cut the last round short it holds accepted tokens behind the
    returned ones).  With `generate(constraint=..., constraint_draft_tokens=k)`: constraint_states int32 [B], every row's final automaton
    state (None otherwise), and the cache holds the prompt and every returned token but each row's last."""

    def __init__(self, sequences, num_rounds, num_target_forwards, num_accepted, past_key_values=None, constraint_states=None):
        self.sequences, self.num_rounds, self.num_target_forwards = sequences, num_rounds, num_target_forwards
        self.num_accepted, self.past_key_values, self.constraint_states = num_accepted, past_key_values, constraint_states


def check_assisted_args(do_sample, num_beams, num_assistant_tokens, t_max, num_return_sequences=1):
    if do_sample or num_beams != 1:
        raise ValueError("assistant_model supports greedy decoding only: do_sample=True and num_beams > 1 cannot be combined with it")
    if num_return_sequences != 1:
        raise ValueError("greedy assisted decoding returns one sequence per prompt")
    k = num_assistant_tokens
    if not isinstance(k, int) or not 1 <= k <= t_max - 1:
        raise ValueError(f"num_assistant_tokens must be an int in 1..{t_max - 1}, got {k!r}")


def spec_accept(draft, target, done, eos, pad, lens_target, lens_draft):
    """The acceptance rule of greedy assisted decoding in plain torch — what lmod_spec_accept computes on the device (the product path
    calls the kernel; this is the statement the tests hold both against).  draft [B, k], target [B, k+1], done [B] (bool / int), lens
    [B]; eos None: no stop token.  Returns (block [B, k+5] = emitted tokens (pad behind) | n_acc | n_emitted | next_token | done,
    next_token [B], done [B], lens_target [B], lens_draft [B]) without modifying its inputs."""
    k = draft.shape[1]
    match = (draft == target[:, :k]).long()
    n_acc = match.cumprod(1).sum(1)
    n_acc = torch.where(done.bool(), torch.zeros_like(n_acc), n_acc)
    return _assisted_block(draft, n_acc, target.gather(1, n_acc[:, None])[:, 0], done, eos, pad, lens_target, lens_draft)


def _assisted_block(draft, n_acc, corrected, done, eos, pad, lens_target, lens_draft):
    """The block of one assisted round from n_acc [B] (0 on done rows) and the token behind the accepted drafts, corrected [B]."""
    B, k = draft.shape
    done = done.bool()
    padv = 0 if pad is None else int(pad)
    idx = torch.arange(k + 1, device=draft.device)[None, :]
    corrected = corrected.to(draft.dtype)[:, None]
    tokens = torch.where(idx < n_acc[:, None], torch.cat([draft, draft[:, -1:]], 1), corrected.expand(B, k + 1))
    n_emit = torch.where(done, torch.zeros_like(n_acc), n_acc + 1)
    fin = done.clone()
    if eos is not None:
        is_eos = (tokens == int(eos)) & (idx < n_emit[:, None])
        first = torch.where(is_eos.any(1), is_eos.long().argmax(1), torch.full_like(n_acc, k + 1))
        n_emit = torch.minimum(n_emit, first + 1)
        fin = fin | is_eos.any(1)
    tokens = torch.where(idx < n_emit[:, None], tokens, torch.full_like(tokens, padv))
    nxt = torch.where(fin, torch.full_like(n_acc, padv), corrected[:, 0].long())
    block = torch.cat([tokens.long(), n_acc[:, None], n_emit[:, None], nxt[:, None], fin.long()[:, None]], 1)
    return (block, nxt, fin, lens_target.long() - k + n_acc, lens_draft.long() - k + torch.clamp(n_acc + 1, max=k))


def check_spec_sample_args(num_beams, num_assistant_tokens, t_max, num_return_sequences=1, temperature=1.0, top_k=None, top_p=None,
                           do_sample=False, **unsupported):
    """Arguments of `generate(assistant_model=..., speculative_sampling=True)`: one sequence per prompt, no beams, k in 1..t_max-1, the
    temperature / top_k / top_p rules of `check_sample_args`.  `unsupported`: the logits-processor and stop-sequence arguments as
    name=value; any that is not at its default raises ValueError (out of scope of this mode).  do_sample stays False: combined with
    assistant_model it keeps raising the greedy-only error of `check_assisted_args`."""
    defaults = {"repetition_penalty": 1.0, "no_repeat_ngram_size": 0, "min_new_tokens": 0}
    used = [n for n, v in unsupported.items() if v is not None and v != defaults.get(n)]
    if used:
        raise ValueError(f"{', '.join(used)}: logits processors and stop sequences are out of scope of speculative_sampling=True")
    if do_sample:
        raise ValueError("assistant_model supports greedy decoding only with do_sample=True: pass speculative_sampling=True and leave "
                         "do_sample False to sample with an assistant")
    if num_beams != 1:
        raise ValueError("speculative_sampling cannot be combined with num_beams > 1")
    if num_return_sequences != 1:
        raise ValueError("speculative sampling returns one sequence per prompt: num_return_sequences must be 1")
    k = num_assistant_tokens
    if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= t_max - 1:
        raise ValueError(f"num_assistant_tokens must be an int in 1..{t_max - 1}, got {k!r}")
    check_sample_args(True, temperature, top_k, top_p, 1)


def check_prompt_lookup_args(prompt_lookup_num_tokens, max_matching_ngram_size, t_max, ngram_max, do_sample=False, num_beams=1,
                             num_return_sequences=1, assistant_model=None, speculative_sampling=False, **unsupported):
    """Arguments of `generate(prompt_lookup_num_tokens=k, max_matching_ngram_size=n)`: greedy, one sequence per prompt, k in
    1..t_max-1 (the verification chunk holds k + 1 tokens), n in 1..ngram_max.  ValueError with do_sample, num_beams > 1,
    num_return_sequences > 1, assistant_model, speculative_sampling, and with any logits-processor or stop-sequence argument
    (`unsupported`, as name=value) that is not at its default: the loop verifies unprocessed logits, as the assisted loop does."""
    defaults = {"repetition_penalty": 1.0, "no_repeat_ngram_size": 0, "min_new_tokens": 0}
    used = [n for n, v in unsupported.items() if v is not None and v != defaults.get(n)]
    if used:
        raise ValueError(f"{', '.join(used)} cannot be combined with prompt_lookup_num_tokens: prompt-lookup decoding verifies "
                         "unprocessed logits")
    if assistant_model is not None or speculative_sampling:
        raise ValueError("prompt_lookup_num_tokens drafts from the token history: it cannot be combined with assistant_model or "
                         "speculative_sampling")
    if do_sample or num_beams != 1:
        raise ValueError("prompt_lookup_num_tokens supports greedy decoding only: do_sample=True and num_beams > 1 cannot be "
                         "combined with it")
    if num_return_sequences != 1:
        raise ValueError("prompt-lookup decoding returns one sequence per prompt")
    k, n = prompt_lookup_num_tokens, max_matching_ngram_size
    if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= t_max - 1:
        raise ValueError(f"prompt_lookup_num_tokens must be an int in 1..{t_max - 1}, got {k!r}")
    if isinstance(n, bool) or not isinstance(n, int) or not 1 <= n <= ngram_max:
        raise ValueError(f"max_matching_ngram_size must be an int in 1..{ngram_max}, got {n!r}")


def spec_sample_rule(p, q, draft, u_acc, u_draw, done, eos, pad, lens_target, lens_draft):
    """The speculative-sampling rule (Leviathan et al.; HF `_speculative_sampling`) in plain torch — what lmod_spec_sample_bf16 computes
    on the device from logits (the product path calls the kernel; this is the statement the tests hold it against).  p [B, k+1, V] and
    q [B, k, V]: the WARPED distributions of the target's and the draft's rows (any float dtype; rows sum to 1); draft [B, k];
    u_acc [B, k], u_draw [B] in [0, 1).  Position i is accepted iff u_acc * q_i(d_i) < p_i(d_i); n_acc = accepted positions before the
    first rejection (0 on a done row).  The next token is the inverse-CDF draw with u_draw in token-id order (the first token whose
    cumulative mass exceeds u_draw * total) from max(0, p_n - q_n), n = n_acc < k (from p_n when that is zero everywhere), or from
    p_k.  Returns spec_accept's tuple (block [B, k+5], next_token, done, lens_target, lens_draft) without modifying its inputs."""
    B, k = draft.shape
    V = p.shape[-1]
    d = draft.long().clamp(0, V - 1)[:, :, None]
    inside = (draft >= 0) & (draft < V)
    pd, qd = p[:, :k].gather(2, d)[:, :, 0], q.gather(2, d)[:, :, 0]
    ok = inside & (u_acc.to(p.dtype) * qd < pd)
    n_acc = ok.long().cumprod(1).sum(1)
    n_acc = torch.where(done.bool(), torch.zeros_like(n_acc), n_acc)
    pn = p.gather(1, n_acc[:, None, None].expand(B, 1, V))[:, 0]
    qn = torch.cat([q, torch.zeros_like(q[:, :1])], 1).gather(1, n_acc[:, None, None].expand(B, 1, V))[:, 0]
    r = (pn - qn).clamp_min(0)
    r = torch.where((r.sum(-1, keepdim=True) > 0) & (n_acc < k)[:, None], r, pn)
    cdf = r.cumsum(-1)
    tok = torch.searchsorted(cdf, (u_draw.to(p.dtype) * cdf[:, -1])[:, None].contiguous(), right=True)[:, 0]
    pos = torch.where(r > 0, torch.arange(V, device=p.device)[None, :], torch.full_like(r, -1, dtype=torch.long)).max(-1).values
    tok = torch.minimum(tok, pos.clamp_min(0))                                # rounding ran past the end: the last token with mass
    return _assisted_block(draft.long(), n_acc, tok, done, eos, pad, lens_target, lens_draft)


class AssistedBookkeeper:
    """Host-side bookkeeping of the assisted loop: the output buffer, how many tokens every sample holds, which samples have stopped
    (EOS or max_new_tokens, possibly in the middle of a round) and the statistics.  Fed with the first token (the target's prefill
    argmax) and then one int block [B, k+5] per round (spec_accept's layout), all on the host."""

    def __init__(self, B, k, max_new_tokens, eos, pad):
        self.B, self.k, self.max_new, self.eos = B, k, max_new_tokens, eos
        self.pad = 0 if pad is None else int(pad)
        self.seq = torch.full((B, max_new_tokens), self.pad, dtype=torch.int64)
        self.n = torch.zeros(B, dtype=torch.int64)
        self.stopped = torch.zeros(B, dtype=torch.bool)
        self.num_accepted = torch.zeros(B, dtype=torch.int64)
        self.num_rounds = 0

    def first(self, tokens):
        """tokens [B]: the target's first token.  Returns done [B] (bool) for the device-side flag."""
        tokens = tokens.long().cpu()
        self.seq[:, 0] = tokens
        self.n += 1
        done = (tokens == self.eos) if self.eos is not None else torch.zeros(self.B, dtype=torch.bool)
        self.stopped = done | (self.n >= self.max_new)
        return done

    def update(self, block):
        """One round's block [B, k+5]: append every sample's emitted tokens, cut at max_new_tokens."""
        k = self.k
        block = block.long().cpu()
        live = ~self.stopped
        n_emit = torch.where(live, block[:, k + 2], torch.zeros_like(self.n))
        take = torch.minimum(n_emit, self.max_new - self.n)
        idx = torch.arange(k + 1)[None, :]
        mask = idx < take[:, None]
        rows = torch.arange(self.B)[:, None].expand(self.B, k + 1)
        self.seq[rows[mask], (self.n[:, None] + idx)[mask]] = block[:, :k + 1][mask]
        self.num_accepted += torch.minimum(block[:, k + 1], take)
        self.n = self.n + take
        self.stopped = self.stopped | (block[:, k + 4] != 0) | (self.n >= self.max_new)
        self.num_rounds += 1

    @property
    def finished(self):
        return bool(self.stopped.all())

    def sequences(self):
        return self.seq[:, :int(self.n.max())]


# ---------------------------------------------------------------------------------------------- logits processors, stop sequences
class LogitsPlan:
    """What `check_logits_args` made of generate()'s processing arguments: penalty (float), ngram (int), bad (the combined table of
    bad_words_ids and suppress_tokens: a list of token lists), min_new (int, 0 without an eos_token_id), stops (stop_sequences
    followed by the keyword sequences of stopping_criteria).  `process`: a logits kernel has to run every step."""

    def __init__(self, penalty, ngram, bad, min_new, stops):
        self.penalty, self.ngram, self.bad, self.min_new, self.stops = penalty, ngram, bad, min_new, stops
        self.process = penalty != 1.0 or ngram > 0 or bool(bad) or min_new > 0


def _token_seqs(name, seqs, vocab_size):
    if isinstance(seqs, (str, bytes)) or not hasattr(seqs, "__iter__"):
        raise ValueError(f"{name} must be a list of token-id lists, got {seqs!r}")
    out = []
    for s in seqs:
        s = s.tolist() if hasattr(s, "tolist") else s
        if isinstance(s, (str, bytes)) or not hasattr(s, "__iter__"):
            raise ValueError(f"{name} must be a list of token-id lists, got the element {s!r}")
        s = list(s)
        if not s:
            raise ValueError(f"{name} holds an empty sequence")
        for t in s:
            if isinstance(t, bool) or not isinstance(t, int) or not 0 <= t < vocab_size:
                raise ValueError(f"{name}: token id {t!r} is not an int in [0, {vocab_size})")
        out.append(s)
    return out


def check_logits_args(repetition_penalty=1.0, no_repeat_ngram_size=0, bad_words_ids=None, suppress_tokens=None, min_new_tokens=0,
                      stop_sequences=None, stopping_criteria=None, eos_token_id=None, vocab_size=None, num_beams=1,
                      assistant_model=None):
    """The logits-processing and stop arguments of `generate()` (HF names and semantics).  Returns None when every one of them is at
    its default — the caller then runs exactly the path it ran before these arguments existed — and a `LogitsPlan` otherwise.
    Raises before anything is launched: ValueError for a value out of range, a table over the kernels' limits (kernels.LOGITS_MAX_SEQS
    sequences per table, kernels.LOGITS_MAX_SEQ_LEN tokens per sequence), a token id outside [0, vocab_size), or any of these
    arguments combined with num_beams > 1 or assistant_model (HF processes log-softmaxed scores there; not built); TypeError for a
    stopping criterion without `keyword_ids`.

    stopping_criteria: each element must expose `keyword_ids`, an iterable of 1-D int tensors or lists — what the reference's
    KeywordsStoppingCriteria (mm_utils.py:74-105) builds in its __init__; its sequences join stop_sequences.  Only that token-level
    test is reproduced: the class's string-level fallback (decode the tail, then search the keyword as a substring) is not, and
    neither is its `all(...)` over the batch — stopping is per row, like EOS."""
    from .kernels import LOGITS_MAX_SEQ_LEN, LOGITS_MAX_SEQS
    given = {"repetition_penalty": repetition_penalty != 1.0, "no_repeat_ngram_size": no_repeat_ngram_size != 0,
             "bad_words_ids": bad_words_ids is not None, "suppress_tokens": suppress_tokens is not None,
             "min_new_tokens": min_new_tokens != 0, "stop_sequences": stop_sequences is not None,
             "stopping_criteria": stopping_criteria is not None}
    used = [k for k, v in given.items() if v]
    if not used:
        return None
    if num_beams != 1:
        raise ValueError(f"{', '.join(used)} cannot be combined with num_beams > 1: beam search scores log-softmaxed logits, which "
                         "these processors do not reach yet")
    if assistant_model is not None:
        raise ValueError(f"{', '.join(used)} cannot be combined with assistant_model: assisted decoding verifies unprocessed logits")
    if vocab_size is None:
        raise ValueError("vocab_size is needed to check token ids")
    p = repetition_penalty
    if isinstance(p, bool) or not isinstance(p, (int, float)) or not p > 0:
        raise ValueError(f"repetition_penalty must be a number > 0, got {p!r}")
    for name, v in (("no_repeat_ngram_size", no_repeat_ngram_size), ("min_new_tokens", min_new_tokens)):
        if isinstance(v, bool) or not isinstance(v, int) or v < 0:
            raise ValueError(f"{name} must be an int >= 0, got {v!r}")
    bad = _token_seqs("bad_words_ids", bad_words_ids, vocab_size) if bad_words_ids is not None else []
    if eos_token_id is not None:
        bad = [s for s in bad if s != [int(eos_token_id)]]                 # HF's NoBadWordsLogitsProcessor drops it too
    if suppress_tokens is not None:
        bad += _token_seqs("suppress_tokens", [[t] for t in (suppress_tokens.tolist() if hasattr(suppress_tokens, "tolist")
                                                               else suppress_tokens)], vocab_size)
    stops = _token_seqs("stop_sequences", stop_sequences, vocab_size) if stop_sequences is not None else []
    if stopping_criteria is not None:
        for c in stopping_criteria:
            if not hasattr(c, "keyword_ids"):
                raise TypeError(f"stopping_criteria: only token-level keyword criteria are supported (an object with `keyword_ids`, "
                                f"as the reference's KeywordsStoppingCriteria), got {type(c).__name__}")
            stops += _token_seqs("stopping_criteria keyword_ids", c.keyword_ids, vocab_size)
    for name, table in (("bad_words_ids + suppress_tokens", bad), ("stop_sequences + stopping_criteria", stops)):
        if len(table) > LOGITS_MAX_SEQS:
            raise ValueError(f"{name}: {len(table)} sequences, at most {LOGITS_MAX_SEQS} are supported")
        longest = max((len(s) for s in table), default=0)
        if longest > LOGITS_MAX_SEQ_LEN:
            raise ValueError(f"{name}: a sequence of {longest} tokens, at most {LOGITS_MAX_SEQ_LEN} are supported")
    return LogitsPlan(float(p), int(no_repeat_ngram_size), bad, int(min_new_tokens) if eos_token_id is not None else 0, stops)


def gen_push_stop(tokens, done, hist, n_hist, n_prompt, n_gen, eos, pad, stops):
    """One generation step's bookkeeping in plain torch — what lmod_gen_push_stop computes on the device (the product path calls the
    kernel; this is the statement the tests hold both against).  tokens [R], done [R], hist [R, L], n_hist / n_prompt / n_gen [R];
    eos None: no stop token; stops: a list of token lists.  A done row's token becomes pad.  A live row's token is appended to its
    history; the row is done when the token is eos, or when its history now ends with a stop sequence that lies entirely behind the
    prompt (n_hist - len >= n_prompt).  Returns new (tokens, done, hist, n_hist, n_gen) without modifying its inputs."""
    was = done.bool()
    live = ~was
    tokens = torch.where(was, torch.full_like(tokens, 0 if pad is None else int(pad)), tokens)
    hist, R = hist.clone(), tokens.shape[0]
    rows = torch.arange(R, device=tokens.device)[live]
    hist[rows, n_hist.long()[live]] = tokens[live].to(hist.dtype)
    n_hist, n_gen = n_hist + live.to(n_hist.dtype), n_gen + live.to(n_gen.dtype)
    fin = was.clone()
    if eos is not None:
        fin |= live & (tokens == int(eos))
    for s in stops or ():
        k = len(s)
        fits = live & (n_hist.long() - k >= n_prompt.long())
        idx = (n_hist.long()[:, None] - k + torch.arange(k, device=tokens.device)[None, :]).clamp_min(0)
        tail = hist.gather(1, idx).long()
        fin |= fits & (tail == torch.tensor(s, device=tokens.device)[None, :]).all(1)
    return tokens, fin.to(done.dtype), hist, n_hist, n_gen


# ---------------------------------------------------------------------------------------------- continuous batching
class BatchOutput:
    """`generate_batch(return_dict_in_generate=True)`: sequences (a list, in request order, of 1-D int64 tensors: each request's new
    tokens, cut after its EOS / stop sequence, no padding), token_logprobs (when sampling: a list of fp32 tensors of the same lengths,
    the log-probability of each drawn token under the warped distribution; None otherwise; when a request carries `params`: a list
    for every request, a greedy token's entry being its log-softmax under the processed logits) and the scheduler's counters:
    num_decode_steps, num_decode_forwards, num_admissions, num_prefills, live_row_steps, total_row_steps, live_fraction.  A call with
    prompt_lookup_num_tokens (a `LookupSlotScheduler`) additionally carries num_rounds, num_target_forwards (one verification pass per
    round; admission prefills are counted by num_prefills, not here) and num_accepted (a list, in request order: the draft tokens that
    were emitted, min(n_acc, n_emitted) per round, `AssistedBookkeeper`'s count); its num_decode_steps and num_decode_forwards are 0
    and a row step is one slot in one round."""

    def __init__(self, sequences, token_logprobs, scheduler, num_accepted=None):
        self.sequences, self.token_logprobs = sequences, token_logprobs
        for k in ("num_decode_steps", "num_decode_forwards", "num_admissions", "num_prefills", "live_row_steps", "total_row_steps",
                  "live_fraction"):
            setattr(self, k, getattr(scheduler, k))
        if isinstance(scheduler, LookupSlotScheduler):
            self.num_rounds, self.num_target_forwards = scheduler.num_rounds, scheduler.num_target_forwards
            self.num_accepted = list(num_accepted) if num_accepted is not None else [0] * len(scheduler.budget)


def static_batch_steps(max_new_tokens, max_batch_size):
    """Steps that `generate()` over consecutive static batches of max_batch_size requests runs when every request emits its whole
    budget: a batch runs until its longest row ends."""
    m, B = list(max_new_tokens), int(max_batch_size)
    return sum(max(m[i:i + B]) for i in range(0, len(m), B))


class SlotScheduler:
    """Which request sits in which slot of `generate_batch`, in plain Python (no torch, no device).  A STEP selects one token for
    every slot (live or not: the batch always runs at max_batch_size rows) and is followed by one decode forward unless no slot is
    live afterwards.  Policy: before every step all free slots are filled from the queue in request order.

        sched = SlotScheduler(max_new_tokens, max_batch_size)
        while not sched.finished:
            for request, slot in sched.admit(): ...          # prefill `request` into `slot`
            ended = sched.step(stopped)                      # `stopped`: slots whose row hit EOS / a stop sequence in this step
            ...                                              # ended: [(request, slot)] freed by this step (stopped or budget reached)

    Counters: num_decode_steps (steps), num_decode_forwards (steps after which a slot was still live), num_admissions (requests
    admitted), num_prefills (admit() calls that admitted something: one prefill pass each), live_row_steps / total_row_steps
    (rows that emitted a real token / max_batch_size * steps) and their ratio live_fraction — what the feature exists to raise."""

    def __init__(self, max_new_tokens, max_batch_size):
        self.budget = [int(m) for m in max_new_tokens]
        B = max_batch_size
        if isinstance(B, bool) or not isinstance(B, int) or B < 1:
            raise ValueError(f"max_batch_size must be an int >= 1, got {B!r}")
        if any(m < 1 for m in self.budget):
            raise ValueError(f"every request needs max_new_tokens >= 1, got {self.budget}")
        self.B = B
        self.slot_request = [None] * B             # slot -> request index (None: free)
        self.n_gen = [0] * B                       # tokens the slot's request has emitted
        self.next_request = 0
        self.num_decode_steps = self.num_decode_forwards = self.num_admissions = self.num_prefills = 0
        self.live_row_steps = self.total_row_steps = 0

    @property
    def live(self):
        """{slot: request} of the occupied slots."""
        return {s: r for s, r in enumerate(self.slot_request) if r is not None}

    @property
    def finished(self):
        return self.next_request >= len(self.budget) and all(r is None for r in self.slot_request)

    @property
    def live_fraction(self):
        return self.live_row_steps / self.total_row_steps if self.total_row_steps else 0.0

    def admit(self):
        """Fill every free slot (ascending) from the queue (request order).  Returns [(request, slot)]."""
        out = []
        for s in range(self.B):
            if self.slot_request[s] is None and self.next_request < len(self.budget):
                self.slot_request[s], self.n_gen[s] = self.next_request, 0
                out.append((self.next_request, s))
                self.next_request += 1
        self.num_admissions += len(out)
        self.num_prefills += bool(out)
        return out

    def step(self, stopped=()):
        """One step: every occupied slot emits a token; a slot in `stopped` or at its request's budget is freed.  Returns the
        [(request, slot)] freed."""
        stopped = set(int(s) for s in stopped)
        live = self.live
        if not live:
            raise RuntimeError("step() without a live slot: call admit() first")
        if not stopped <= set(live):
            raise ValueError(f"slots {sorted(stopped - set(live))} reported as stopped hold no request")
        self.num_decode_steps += 1
        self.total_row_steps += self.B
        self.live_row_steps += len(live)
        ended = []
        for s, r in live.items():
            self.n_gen[s] += 1
            if s in stopped or self.n_gen[s] >= self.budget[r]:
                ended.append((r, s))
                self.slot_request[s] = None
        self.num_decode_forwards += any(r is not None for r in self.slot_request)
        return ended


class LookupSlotScheduler(SlotScheduler):
    """`SlotScheduler` for rounds that emit a variable number of tokens per slot (generate_batch with prompt_lookup_num_tokens): the
    same slots, queue, admission policy (all free slots are filled in request order before every round) and admission counters;
    `advance` replaces `step`, which stays as it is.

        while not sched.finished:
            for request, slot in sched.admit(): ...
            ended = sched.advance(emitted, ended_slots)      # emitted: {slot: tokens its request emitted in this round}

    Counters of its own: num_rounds, num_target_forwards (one verification pass per round), tokens_emitted.  A round adds
    max_batch_size to total_row_steps and the occupied slots to live_row_steps; num_decode_steps / num_decode_forwards stay 0."""

    def __init__(self, max_new_tokens, max_batch_size):
        super().__init__(max_new_tokens, max_batch_size)
        self.num_rounds = self.num_target_forwards = self.tokens_emitted = 0

    def advance(self, emitted, ended=()):
        """One round.  emitted: {slot: n} for every occupied slot, n >= 1 tokens (the first token of a freshly admitted slot
        included) and never past the request's budget; ended: the slots the device reported as finished (EOS, a stop sequence, the
        budget).  A slot in `ended` or at its budget is freed.  Returns the [(request, slot)] freed."""
        live = self.live
        if not live:
            raise RuntimeError("advance() without a live slot: call admit() first")
        emitted = {int(s): int(n) for s, n in dict(emitted).items()}
        ended = set(int(s) for s in ended)
        if set(emitted) != set(live):
            raise ValueError(f"emitted names slots {sorted(emitted)}, occupied are {sorted(live)}")
        if not ended <= set(live):
            raise ValueError(f"slots {sorted(ended - set(live))} reported as ended hold no request")
        for s, n in emitted.items():
            if n < 1 or self.n_gen[s] + n > self.budget[live[s]]:
                raise ValueError(f"slot {s}: {n} tokens emitted with {self.n_gen[s]} of {self.budget[live[s]]} already out")
        self.num_rounds += 1
        self.num_target_forwards += 1
        self.total_row_steps += self.B
        self.live_row_steps += len(live)
        freed = []
        for s, r in live.items():
            self.n_gen[s] += emitted[s]
            self.tokens_emitted += emitted[s]
            if s in ended or self.n_gen[s] >= self.budget[r]:
                freed.append((r, s))
                self.slot_request[s] = None
        return freed


def check_batch_lookup_args(requests, prompt_lookup_num_tokens, max_matching_ngram_size, t_max, ngram_max, do_sample=False,
                            **processors):
    """The arguments of `generate_batch(prompt_lookup_num_tokens=k, max_matching_ngram_size=n)` beyond `check_batch_args`: greedy only,
    unprocessed logits (the round verifies them, as `generate()`'s lookup loop does), no per-request `params`, k in 1..t_max-1 (the
    verification chunk holds k + 1 tokens), n in 1..ngram_max and GIVEN: n None raises, so a call with prompt_lookup_num_tokens alone
    keeps the refusal it always got (tests/test_prompt_lookup_gpu.py pins it).  `processors`: repetition_penalty, no_repeat_ngram_size, bad_words_ids,
    suppress_tokens, min_new_tokens as name=value; one that is not at its default raises.  Stop sequences, eos / pad, per-request
    max_new_tokens and images are supported and not checked here.  ValueError naming the argument, before any device work."""
    if do_sample:
        raise ValueError("do_sample=True cannot be combined with prompt_lookup_num_tokens in generate_batch: its rounds are greedy")
    defaults = {"repetition_penalty": 1.0, "no_repeat_ngram_size": 0, "min_new_tokens": 0}
    unknown = set(processors) - {"repetition_penalty", "no_repeat_ngram_size", "bad_words_ids", "suppress_tokens", "min_new_tokens"}
    if unknown:
        raise TypeError(f"check_batch_lookup_args: unexpected arguments {sorted(unknown)}")
    used = [n for n, v in processors.items() if v is not None and v != defaults.get(n)]
    if used:
        raise ValueError(f"{', '.join(used)} cannot be combined with prompt_lookup_num_tokens: prompt-lookup decoding verifies "
                         "unprocessed logits")
    for i, rq in enumerate(requests):
        if isinstance(rq, dict) and rq.get("params") is not None:
            raise ValueError(f"request {i}: params cannot be combined with prompt_lookup_num_tokens (per-request parameters are not "
                             "built for the lookup rounds)")
    k, n = prompt_lookup_num_tokens, max_matching_ngram_size
    if n is None:
        raise ValueError("generate_batch runs prompt_lookup_num_tokens only together with an explicit max_matching_ngram_size "
                         f"(1..{ngram_max}; HF's default is 2): prompt_lookup_num_tokens alone is refused as it was before the "
                         "lookup rounds existed")
    if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= t_max - 1:
        raise ValueError(f"prompt_lookup_num_tokens must be an int in 1..{t_max - 1}, got {k!r}")
    if isinstance(n, bool) or not isinstance(n, int) or not 1 <= n <= ngram_max:
        raise ValueError(f"max_matching_ngram_size must be an int in 1..{ngram_max}, got {n!r}")


def check_batch_args(requests, max_batch_size=8, max_new_tokens=16, num_beams=1, assistant_model=None, num_return_sequences=1,
                     past_key_values=None, prompt_lookup_num_tokens=None):
    """The arguments of `generate_batch` that `generate()` does not have, and the modes it leaves out.  Returns each request's
    max_new_tokens (a list).  ValueError: num_beams > 1, assistant_model, prompt_lookup_num_tokens, num_return_sequences > 1,
    past_key_values (out of scope of continuous batching), a bad max_batch_size, a request without `input_ids` or with a budget < 1, a request key other than
    `input_ids`, `images`, `max_new_tokens` and `params` (a `RequestParams`).  prompt_lookup_num_tokens is refused HERE whatever its
    value: `generate_batch` validates the lookup pair itself (`check_batch_lookup_args`) and calls this function without it."""
    if num_beams != 1:
        raise ValueError("generate_batch does not support num_beams > 1: beam search needs its beams in adjacent rows")
    if assistant_model is not None:
        raise ValueError("generate_batch does not support assistant_model")
    if prompt_lookup_num_tokens is not None:
        raise ValueError("generate_batch does not support prompt_lookup_num_tokens: its slots decode one token per step")
    if num_return_sequences != 1:
        raise ValueError("generate_batch returns one sequence per request: num_return_sequences > 1 is not supported "
                         "(list the request more than once)")
    if past_key_values is not None:
        raise ValueError("generate_batch does not support past_key_values: it owns its slot cache")
    B = max_batch_size
    if isinstance(B, bool) or not isinstance(B, int) or B < 1:
        raise ValueError(f"max_batch_size must be an int >= 1, got {B!r}")
    budgets = []
    for i, rq in enumerate(requests):
        if not isinstance(rq, dict) or rq.get("input_ids") is None:
            raise ValueError(f"request {i}: a dict with `input_ids` [S] is expected")
        unknown = set(rq) - {"input_ids", "images", "max_new_tokens", "params"}
        if unknown:
            raise ValueError(f"request {i}: unknown keys {sorted(unknown)} (a request's own sampling, processor and stop arguments "
                             "go into its `params`, a generation.RequestParams)")
        if rq.get("params") is not None and not isinstance(rq["params"], RequestParams):
            raise ValueError(f"request {i}: params must be a generation.RequestParams, got {type(rq['params']).__name__}")
        ids = rq["input_ids"]
        if getattr(ids, "dim", lambda: 0)() != 1 or ids.numel() < 1:
            raise ValueError(f"request {i}: input_ids must be a 1-D tensor of at least one token")
        m = rq.get("max_new_tokens", max_new_tokens)
        if isinstance(m, bool) or not isinstance(m, int) or m < 1:
            raise ValueError(f"request {i}: max_new_tokens must be an int >= 1, got {m!r}")
        budgets.append(m)
    return budgets


# ---------------------------------------------------------------------------------------------- per-request parameters
class RequestParams:
    """A request's own decoding arguments for `generate_batch` (the request dict's `params`).  Every field defaults to None = inherit
    the call's argument of the same name.  stop_sequences apply IN ADDITION to the call's.  seed: the request's k-th uniform is
    Philox4x32-10 with key = seed at counter (0, k, 0, 0) — the same draws wherever the request stands in the list and whichever call
    carries it; without one it keeps the call's stream, key = the call's seed at counter (request index, k, 0, 0).  bad_words_ids,
    suppress_tokens, eos_token_id and pad_token_id stay per call.  constraint: the request's own `TokenConstraint` instead of the
    call's (None inherits the call's; `NO_CONSTRAINT` turns the call's off for this request); it is not one of FIELDS: the slot's
    automaton state is an array of its own, not a column of the parameter table."""

    FIELDS = ("do_sample", "temperature", "top_k", "top_p", "seed", "repetition_penalty", "no_repeat_ngram_size", "min_new_tokens",
              "stop_sequences")

    def __init__(self, do_sample=None, temperature=None, top_k=None, top_p=None, seed=None, repetition_penalty=None,
                 no_repeat_ngram_size=None, min_new_tokens=None, stop_sequences=None, constraint=None):
        self.do_sample, self.temperature, self.top_k, self.top_p, self.seed = do_sample, temperature, top_k, top_p, seed
        self.repetition_penalty, self.no_repeat_ngram_size, self.min_new_tokens = repetition_penalty, no_repeat_ngram_size, min_new_tokens
        self.stop_sequences, self.constraint = stop_sequences, constraint

    def __repr__(self):
        return "RequestParams(" + ", ".join(f"{k}={getattr(self, k)!r}" for k in self.FIELDS + ("constraint",)
                                            if getattr(self, k) is not None) + ")"


class RequestRecord:
    """One request's effective parameters, as the device sees them: do_sample, temperature (1.0 when greedy), top_k (0: off), top_p
    (1.0: off), seed (its own, else the call's; None: the call gives none and generate_batch draws it), own_seed and ctr0 (the first
    counter word: 0 under an own seed, the request index otherwise), penalty, ngram, min_new (0 without an eos_token_id), and its own stop sequences
    as the range (stop_first, stop_count) of the plan's stop table."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


class RequestPlan:
    """What `check_request_params` made of a call.  per_request: some request carries `params` — False means generate_batch runs the
    loop and the kernels it ran before per-request parameters existed (`records` is then None).  Otherwise: records (a
    `RequestRecord` per request), stops (ONE stop table: the call's sequences first, then each request's own), n_call_stops, bad (the
    call's bad-word table), any_sample / any_process / any_penalty (some request samples / some processor or bad word is active /
    some repetition penalty differs from 1) and needs_call_seed (a sampled request without a seed of its own)."""

    # rows of the device table [len(TABLE_FIELDS) + 1, max_batch_size] int32 (floats bit-cast); `seed` takes two rows: the B 64-bit
    # keys as one contiguous u64 [B] array, so slot s's key is the int32 pair (2s, 2s + 1) of those rows
    TABLE_FIELDS = ("seed", "ctr0", "greedy", "temperature", "top_k", "top_p", "penalty", "ngram", "min_new", "stop_first",
                    "stop_count")
    TABLE_ROWS = len(TABLE_FIELDS) + 1

    def __init__(self, per_request, records=None, stops=(), n_call_stops=0, bad=(), any_sample=False, any_process=False,
                 any_penalty=False, needs_call_seed=False):
        self.per_request, self.records, self.stops, self.n_call_stops, self.bad = per_request, records, list(stops), n_call_stops, list(bad)
        self.any_sample, self.any_process, self.any_penalty, self.needs_call_seed = any_sample, any_process, any_penalty, needs_call_seed

    @staticmethod
    def _f32(x):
        import struct
        return struct.unpack("<i", struct.pack("<f", float(x)))[0]

    @classmethod
    def row_of(cls, field):
        """First row of `field` in the device table (seed: rows 0 and 1)."""
        i = cls.TABLE_FIELDS.index(field)
        return i if i == 0 else i + 1

    @classmethod
    def neutral_table(cls, B):
        """The table of B idle slots as a nested list [TABLE_ROWS][B] of int32 values: greedy, temperature 1, no filter, penalty 1, no
        n-gram, no minimum, no stops."""
        one = cls._f32(1.0)
        rows = {"greedy": 1, "temperature": one, "top_p": one, "penalty": one}
        return [[0] * B, [0] * B] + [[rows.get(f, 0)] * B for f in cls.TABLE_FIELDS[1:]]

    def columns(self, admitted, B, call_seed):
        """The table entries of the admitted [(request, slot)] as (flat indices into the table viewed as 1-D, int32 values), two
        equally long lists: one indexed copy writes them."""
        idx, val = [], []
        for r, s in admitted:
            rec = self.records[r]
            seed = (call_seed if rec.seed is None else rec.seed) or 0
            seed &= 0xFFFFFFFFFFFFFFFF
            words = {"ctr0": rec.ctr0, "greedy": int(not rec.do_sample), "temperature": self._f32(rec.temperature), "top_k": rec.top_k,
                     "top_p": self._f32(rec.top_p), "penalty": self._f32(rec.penalty), "ngram": rec.ngram, "min_new": rec.min_new,
                     "stop_first": rec.stop_first, "stop_count": rec.stop_count}
            for half, w in enumerate((seed & 0xFFFFFFFF, seed >> 32)):
                idx.append(2 * s + half)
                val.append(w - (1 << 32) if w >= 1 << 31 else w)
            for f, w in words.items():
                idx.append(self.row_of(f) * B + s)
                val.append(int(w))
        return idx, val


def check_request_params(requests, do_sample=False, temperature=1.0, top_k=None, top_p=None, seed=None, repetition_penalty=1.0,
                         no_repeat_ngram_size=0, bad_words_ids=None, suppress_tokens=None, min_new_tokens=0, stop_sequences=None,
                         stopping_criteria=None, eos_token_id=None, vocab_size=None):
    """Resolve every request's effective parameters (its `params` over the call's arguments) and check them with the rules of
    `check_sample_args` and `check_logits_args`; a ValueError names the request.  Host only, once per call.  Returns a `RequestPlan`;
    when no request carries `params` the plan says so (per_request False) and nothing else is built: the caller's existing checks
    and path apply unchanged."""
    if not any(isinstance(rq, dict) and rq.get("params") is not None for rq in requests):
        return RequestPlan(False)
    from .kernels import LOGITS_MAX_SEQS
    call_plan = check_logits_args(repetition_penalty, no_repeat_ngram_size, bad_words_ids, suppress_tokens, min_new_tokens,
                                  stop_sequences, stopping_criteria, eos_token_id, vocab_size)
    call_stops = list(call_plan.stops) if call_plan is not None else []
    bad = list(call_plan.bad) if call_plan is not None else []
    call = dict(do_sample=do_sample, temperature=temperature, top_k=top_k, top_p=top_p, seed=seed,
                repetition_penalty=repetition_penalty, no_repeat_ngram_size=no_repeat_ngram_size, min_new_tokens=min_new_tokens)
    records, stops = [], list(call_stops)
    for i, rq in enumerate(requests):
        prm = rq.get("params") or RequestParams()
        if not isinstance(prm, RequestParams):
            raise ValueError(f"request {i}: params must be a generation.RequestParams, got {type(prm).__name__}")
        e = {k: (call[k] if getattr(prm, k) is None else getattr(prm, k)) for k in call}
        try:
            if e["do_sample"] not in (False, True):
                raise ValueError(f"do_sample must be False or True, got {e['do_sample']!r}")
            sd = e["seed"]
            if sd is not None and (isinstance(sd, bool) or not isinstance(sd, int)):
                raise ValueError(f"seed must be None or an int, got {sd!r}")
            check_sample_args(bool(e["do_sample"]), e["temperature"], e["top_k"], e["top_p"], 1)
            own = check_logits_args(e["repetition_penalty"], e["no_repeat_ngram_size"], None, None, e["min_new_tokens"],
                                    prm.stop_sequences, None, eos_token_id, vocab_size)
            own_stops = own.stops if own is not None else []
            if len(call_stops) + len(own_stops) > LOGITS_MAX_SEQS:
                raise ValueError(f"stop_sequences: {len(call_stops)} of the call and {len(own_stops)} of the request, at most "
                                 f"{LOGITS_MAX_SEQS} are supported together")
        except ValueError as err:
            raise ValueError(f"request {i}: {err}") from None
        sample = bool(e["do_sample"])
        own_seed = prm.seed is not None
        records.append(RequestRecord(
            do_sample=sample, temperature=float(e["temperature"]) if sample else 1.0,
            top_k=(max(0, min(int(e["top_k"]), 2 ** 31 - 1)) if e["top_k"] is not None else 0) if sample else 0,
            top_p=(float(e["top_p"]) if e["top_p"] is not None else 1.0) if sample else 1.0,
            seed=(int(sd) & 0xFFFFFFFFFFFFFFFF) if sd is not None else None, own_seed=own_seed, ctr0=0 if own_seed else i,
            penalty=own.penalty if own is not None else 1.0, ngram=own.ngram if own is not None else 0,
            min_new=own.min_new if own is not None else 0, stop_first=len(stops) if own_stops else 0, stop_count=len(own_stops)))
        stops += own_stops
    return RequestPlan(True, records, stops, len(call_stops), bad,
                       any_sample=any(r.do_sample for r in records),
                       any_process=bool(bad) or any(r.penalty != 1.0 or r.ngram > 0 or r.min_new > 0 for r in records),
                       any_penalty=any(r.penalty != 1.0 for r in records),
                       needs_call_seed=any(r.do_sample and not r.own_seed for r in records))


# ---------------------------------------------------------------------------------------------- constrained decoding
class TokenConstraint:
    """A deterministic finite automaton over token ids: what a row of `generate(constraint=...)` MAY emit.  States are
    0 .. n_states-1; a row starts in `start`.  A state s is CLOSED (default_next[s] == -1: only tokens with a listed edge whose next is
    >= 0 are allowed) or OPEN (default_next[s] = d >= 0: every token is allowed, an unlisted one leads to d, a listed edge redirects
    its token and one with next == -1 bans it).  accept[s]: the row may end here, so EOS is allowed in this state; terminal[s]:
    accepting, closed and without an allowed edge - a row that enters it is finished by that token.

        TokenConstraint(n_states, edges, accepting, default=None, start=0)

    edges: an iterable of (state, token, next or -1); accepting: an iterable of states; default: None (every state closed), one int
    for every state, a sequence of n_states ints or a dict {state: d}.  ValueError for a duplicate (state, token), for a state, next,
    default or start out of range, and for a dead end (a closed, non-accepting state without an allowed edge).  Token ids are
    checked against a vocabulary by `check_constraint_args`.

    The device form (lmod_constrain_mask_rows_bf16 / lmod_constrain_advance_rows), plain int lists here: edge_off [n_states + 1],
    edge_tok / edge_next [E] (CSR, tokens strictly ascending inside a state), default_next [n_states], flags [n_states] (bit 0
    accept, bit 1 terminal)."""

    ACCEPT, TERMINAL = 1, 2

    def __init__(self, n_states, edges, accepting, default=None, start=0):
        n = n_states
        if isinstance(n, bool) or not isinstance(n, int) or n < 1:
            raise ValueError(f"n_states must be an int >= 1, got {n!r}")

        def _int(name, v, lo):
            if isinstance(v, bool) or not isinstance(v, int) or not lo <= v < n:
                raise ValueError(f"{name} must be an int in [{lo}, {n}), got {v!r}")
            return v

        if default is None:
            dn = [-1] * n
        elif isinstance(default, dict):
            dn = [-1] * n
            for st, d in default.items():
                dn[_int("a state of default", st, 0)] = d
        elif isinstance(default, int):
            dn = [default] * n
        else:
            dn = list(default)
            if len(dn) != n:
                raise ValueError(f"default lists {len(dn)} states, the automaton has {n}")
        self.default_next = [_int("default", d, -1) for d in dn]
        self.n_states, self.start = n, _int("start", start, 0)
        per = [{} for _ in range(n)]
        for e in edges:
            st, tok, nx = e
            _int("an edge's state", st, 0)
            if isinstance(tok, bool) or not isinstance(tok, int):
                raise ValueError(f"an edge's token must be an int, got {tok!r}")
            if tok in per[st]:
                raise ValueError(f"duplicate edge: state {st}, token {tok}")
            per[st][tok] = _int("an edge's next state", nx, -1)
        self.accept = [False] * n
        for st in accepting:
            self.accept[_int("an accepting state", st, 0)] = True
        self.edge_off, self.edge_tok, self.edge_next = [0], [], []
        for d in per:
            for tok in sorted(d):
                self.edge_tok.append(tok)
                self.edge_next.append(d[tok])
            self.edge_off.append(len(self.edge_tok))
        self.terminal = []
        for st in range(n):
            stuck = self.default_next[st] < 0 and not any(nx >= 0 for nx in per[st].values())
            if stuck and not self.accept[st]:
                raise ValueError(f"state {st} is a dead end: closed, not accepting and without an allowed edge")
            self.terminal.append(stuck)
        self.flags = [self.ACCEPT * a + self.TERMINAL * t for a, t in zip(self.accept, self.terminal)]

    @property
    def has_closed(self):
        """Some state is closed: lmod_constrain_mask_rows_bf16 then needs its V-bit bitmap."""
        return any(d < 0 for d in self.default_next)

    @property
    def has_terminal(self):
        return any(self.terminal)

    def edges(self):
        """The edges as a list of (state, token, next), state by state, tokens ascending."""
        return [(st, self.edge_tok[e], self.edge_next[e]) for st in range(self.n_states)
                for e in range(self.edge_off[st], self.edge_off[st + 1])]

    @classmethod
    def from_choices(cls, seqs):
        """Exactly one of these token sequences: a trie of closed states.  Duplicates are dropped; a choice that is a proper prefix of
        another ends in an accepting state that is not terminal (the row may stop there or go on).  ValueError for an empty choice
        or an empty list."""
        seqs = [list(s.tolist() if hasattr(s, "tolist") else s) for s in seqs]
        if not seqs:
            raise ValueError("from_choices needs at least one choice")
        children, accepting = [{}], set()
        for s in seqs:
            if not s:
                raise ValueError("from_choices: an empty choice")
            node = 0
            for tok in s:
                if isinstance(tok, bool) or not isinstance(tok, int):
                    raise ValueError(f"from_choices: token id {tok!r} is not an int")
                if tok not in children[node]:
                    children[node][tok] = len(children)
                    children.append({})
                node = children[node][tok]
            accepting.add(node)
        return cls(len(children), [(st, tok, nx) for st, d in enumerate(children) for tok, nx in d.items()], sorted(accepting))

    @classmethod
    def from_allowed_tokens(cls, tokens):
        """Only these tokens, any number of them: one closed, accepting state with a self-loop per token (the constant case of HF's
        prefix_allowed_tokens_fn)."""
        tokens = sorted(set(tokens.tolist() if hasattr(tokens, "tolist") else tokens))
        if not tokens:
            raise ValueError("from_allowed_tokens needs at least one token")
        return cls(1, [(0, tok, 0) for tok in tokens], [0])

    @classmethod
    def merge(cls, constraints):
        """The disjoint union of a list of constraints (None entries allowed) with state offsets, for a batch whose rows follow
        different automata through one set of tables.  Returns (merged, starts): starts[i] is constraint i's start state inside
        `merged`, -1 for None; merged is None when every entry is."""
        edges, accepting, default, starts, off = [], [], [], [], 0
        for c in constraints:
            if c is None:
                starts.append(-1)
                continue
            if not isinstance(c, cls):
                raise ValueError(f"merge: a TokenConstraint or None is expected, got {type(c).__name__}")
            edges += [(st + off, tok, nx + off if nx >= 0 else -1) for st, tok, nx in c.edges()]
            accepting += [st + off for st in range(c.n_states) if c.accept[st]]
            default += [d + off if d >= 0 else -1 for d in c.default_next]
            starts.append(c.start + off)
            off += c.n_states
        return (cls(off, edges, accepting, default) if off else None), starts

    def walk(self, tokens, state=None):
        """The transition rule in plain Python - what lmod_constrain_advance_rows does with one token at a time.  From `state` (the
        start state by default) follow `tokens`: a listed edge leads to its next state, an unlisted token to the state's default.
        Returns (state, ok): ok False at the first token that is not allowed (next -1); the state is then the one that refused it."""
        s = self.start if state is None else state
        for tok in tokens:
            lo, hi = self.edge_off[s], self.edge_off[s + 1]
            nx = self.default_next[s]
            for e in range(lo, hi):
                if self.edge_tok[e] == int(tok):
                    nx = self.edge_next[e]
                    break
            if nx < 0:
                return s, False
            s = nx
        return s, True

    def forced(self, state, eos=None, vocab_size=None):
        """The token `state` forces, as (token, next), or None - what lmod_constrain_draft drafts from it.  A state is FORCED when
        it is closed, not terminal, and the set the mask would allow in it - the edges with next >= 0 and 0 <= token < vocab_size
        (None: no upper bound), plus `eos` where the state accepts (None: no such token) - has exactly one element, and that element
        is a listed edge, not eos.  generate(constraint_draft_tokens=k) emits up to k consecutive forced tokens per pass."""
        if not 0 <= state < self.n_states or self.default_next[state] >= 0 or self.terminal[state]:
            return None
        inside = lambda tok: tok >= 0 and (vocab_size is None or tok < vocab_size)
        if self.accept[state] and eos is not None and inside(eos):
            return None
        allowed = [(self.edge_tok[e], self.edge_next[e]) for e in range(self.edge_off[state], self.edge_off[state + 1])
                   if self.edge_next[e] >= 0 and inside(self.edge_tok[e])]
        if len(allowed) != 1 or (eos is not None and allowed[0][0] == eos):
            return None
        return allowed[0]

    def __repr__(self):
        return f"TokenConstraint(n_states={self.n_states}, edges={len(self.edge_tok)}, start={self.start})"


class _NoConstraint:
    def __repr__(self):
        return "NO_CONSTRAINT"


NO_CONSTRAINT = _NoConstraint()           # RequestParams(constraint=NO_CONSTRAINT): this request ignores the call's constraint


def _constraint_vocab(constraint, vocab_size, who="constraint"):
    from .kernels import CONSTRAIN_MAX_V
    if not isinstance(constraint, TokenConstraint):
        raise ValueError(f"{who} must be a generation.TokenConstraint, got {type(constraint).__name__}")
    if vocab_size is None:
        raise ValueError("vocab_size is needed to check token ids")
    for tok in constraint.edge_tok:
        if not 0 <= tok < vocab_size:
            raise ValueError(f"{who}: token id {tok} is not in [0, {vocab_size})")
    if constraint.has_closed and vocab_size > CONSTRAIN_MAX_V:
        raise ValueError(f"{who}: a closed state needs a {vocab_size}-bit bitmap in LDS: a vocabulary above {CONSTRAIN_MAX_V} is not "
                         "supported")


def _banning(no_repeat_ngram_size=0, bad_words_ids=None, suppress_tokens=None, min_new_tokens=0):
    given = {"no_repeat_ngram_size": no_repeat_ngram_size not in (0, None), "bad_words_ids": bad_words_ids is not None,
             "suppress_tokens": suppress_tokens is not None, "min_new_tokens": min_new_tokens not in (0, None)}
    return [k for k, v in given.items() if v]


_BANNING_MSG = ("{used} cannot be combined with a constraint: a banning processor can empty a row's allowed set, and combining the "
                "two is not built yet (repetition_penalty and stop sequences are fine)")


def check_constraint_args(constraint, vocab_size, num_beams=1, assistant_model=None, prompt_lookup_num_tokens=None,
                          speculative_sampling=False, no_repeat_ngram_size=0, bad_words_ids=None, suppress_tokens=None,
                          min_new_tokens=0):
    """`generate(constraint=...)` beside its other arguments; nothing to check without a constraint.  ValueError, before anything is
    launched: a token id outside [0, vocab_size); num_beams > 1, assistant_model, prompt_lookup_num_tokens or speculative_sampling
    (those loops verify or score logits the mask does not reach); a banning processor (no_repeat_ngram_size, bad_words_ids,
    suppress_tokens, min_new_tokens: it can empty a row's allowed set - not built yet); a closed state with a vocabulary above
    kernels.CONSTRAIN_MAX_V.  repetition_penalty, stop_sequences and stopping_criteria combine freely."""
    if constraint is None:
        return
    _constraint_vocab(constraint, vocab_size)
    modes = {"num_beams > 1": num_beams != 1, "assistant_model": assistant_model is not None,
             "prompt_lookup_num_tokens": prompt_lookup_num_tokens is not None, "speculative_sampling": bool(speculative_sampling)}
    used = [k for k, v in modes.items() if v]
    if used:
        raise ValueError(f"constraint cannot be combined with {', '.join(used)}: that loop verifies or scores logits the "
                         "constraint's mask does not reach")
    used = _banning(no_repeat_ngram_size, bad_words_ids, suppress_tokens, min_new_tokens)
    if used:
        raise ValueError(_BANNING_MSG.format(used=", ".join(used)))


def check_constraint_draft_args(constraint_draft_tokens, constraint, t_max, do_sample=False, num_beams=1, num_return_sequences=1,
                                assistant_model=None, speculative_sampling=False, prompt_lookup_num_tokens=None,
                                repetition_penalty=1.0, stop_sequences=None, stopping_criteria=None):
    """`generate(constraint=c, constraint_draft_tokens=k)` beside its other arguments; nothing to check without the argument.
    ValueError, before any device work: no constraint; k not an int in 1..t_max-1 (the verification chunk holds k + 1 tokens);
    do_sample, num_beams > 1, num_return_sequences > 1 (greedy, one sequence per prompt); assistant_model, speculative_sampling,
    prompt_lookup_num_tokens (another drafter); repetition_penalty != 1, stop_sequences, stopping_criteria (the round verifies
    logits that only the constraint's mask has touched).  The banning processors are refused with any constraint
    (`check_constraint_args`)."""
    k = constraint_draft_tokens
    if k is None:
        return
    if constraint is None:
        raise ValueError("constraint_draft_tokens needs a constraint: it drafts the tokens the automaton forces")
    if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= t_max - 1:
        raise ValueError(f"constraint_draft_tokens must be an int in 1..{t_max - 1}, got {k!r}")
    if do_sample or num_beams != 1:
        raise ValueError("constraint_draft_tokens supports greedy decoding only: do_sample=True and num_beams > 1 cannot be combined "
                         "with it")
    if num_return_sequences != 1:
        raise ValueError("constraint_draft_tokens returns one sequence per prompt: num_return_sequences must be 1")
    modes = {"assistant_model": assistant_model is not None, "speculative_sampling": bool(speculative_sampling),
             "prompt_lookup_num_tokens": prompt_lookup_num_tokens is not None}
    used = [n for n, v in modes.items() if v]
    if used:
        raise ValueError(f"constraint_draft_tokens drafts from the automaton: it cannot be combined with {', '.join(used)}")
    given = {"repetition_penalty": repetition_penalty not in (1.0, None), "stop_sequences": stop_sequences is not None,
             "stopping_criteria": stopping_criteria is not None}
    used = [n for n, v in given.items() if v]
    if used:
        raise ValueError(f"{', '.join(used)} cannot be combined with constraint_draft_tokens: the round verifies logits that only the "
                         "constraint's mask has touched")


class ConstraintPlan:
    """What `check_batch_constraint_args` made of a generate_batch call: merged (ONE TokenConstraint: the disjoint union of the
    call's distinct constraints) and starts (per request: its start state inside `merged`, -1 for an unconstrained request)."""

    def __init__(self, merged, starts):
        self.merged, self.starts = merged, starts


def check_batch_constraint_args(requests, constraint, vocab_size, prompt_lookup_num_tokens=None, no_repeat_ngram_size=0,
                                bad_words_ids=None, suppress_tokens=None, min_new_tokens=0):
    """`generate_batch(constraint=...)` and every request's `params.constraint`: a request's own constraint overrides the call's,
    None inherits it, NO_CONSTRAINT turns it off.  Returns None when no request ends up constrained and the call gives none (the
    caller then allocates and launches nothing new), else a `ConstraintPlan`.  ValueError, naming the request, before any device
    work: the token and vocabulary rules of `check_constraint_args`; prompt_lookup_num_tokens; a banning processor (the request's
    effective no_repeat_ngram_size / min_new_tokens, the call's bad_words_ids / suppress_tokens) on a CONSTRAINED request -
    unconstrained requests of the same list may use them."""
    eff = []
    for i, rq in enumerate(requests):
        prm = rq.get("params") if isinstance(rq, dict) else None
        own = getattr(prm, "constraint", None)
        c = constraint if own is None else (None if own is NO_CONSTRAINT else own)
        eff.append(c)
    if constraint is None and all(c is None for c in eff):
        return None
    if constraint is not None:
        _constraint_vocab(constraint, vocab_size)
    if prompt_lookup_num_tokens is not None:
        raise ValueError("constraint cannot be combined with prompt_lookup_num_tokens: the lookup rounds verify logits the "
                         "constraint's mask does not reach")
    for i, (rq, c) in enumerate(zip(requests, eff)):
        if c is None:
            continue
        _constraint_vocab(c, vocab_size, f"request {i}: constraint")
        prm = rq.get("params")
        own = lambda name, call: call if getattr(prm, name, None) is None else getattr(prm, name)
        used = _banning(own("no_repeat_ngram_size", no_repeat_ngram_size), bad_words_ids, suppress_tokens,
                        own("min_new_tokens", min_new_tokens))
        if used:
            raise ValueError(f"request {i}: " + _BANNING_MSG.format(used=", ".join(used)))
    distinct = []
    for c in eff:
        if c is not None and not any(c is d for d in distinct):
            distinct.append(c)
    merged, first = TokenConstraint.merge(distinct)
    if merged is None:                                     # the call's constraint is turned off by every request
        return None
    starts = [-1 if c is None else first[next(j for j, d in enumerate(distinct) if d is c)] for c in eff]
    return ConstraintPlan(merged, starts)
