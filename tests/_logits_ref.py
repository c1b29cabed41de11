"""Plain-torch reference of the logits processors and the stop rule of generate() (the contract of lmod_logits_process_bf16 and
lmod_gen_push_stop, include/lmod_hip.h), written from HF's semantics (transformers 5.x) and not from the kernels: no bitmap, no
phases — one boolean ban mask per row and one `where`.  No HIP library; works on host and device tensors alike.

History: hist [R, L] int, of which the first n_hist[r] entries of row r are live (the row's prompt ids, then what it generated);
n_gen [R] counts the generated ones.  Ids are compared as plain integers; an id outside [0, V) is never penalised or banned.
  1. repetition penalty p: every distinct live token t gets x = x * p if x < 0 else x / p, once;
  2. no-repeat n-gram n (n_hist >= n): the last token of every live window of n tokens whose first n-1 tokens equal the row's last
     n-1 tokens is banned (n = 1: every live token);
  3. bad words: a one-token entry is banned always; a longer entry's last token when n_hist >= len(entry) and the history ends with
     the entry's other tokens (HF's SequenceBiasLogitsProcessor skips an entry longer than the context);
  4. min new tokens: eos is banned while n_gen < min_new.
The arithmetic is fp32 on the bf16 values; a ban is -inf; the result is rounded once to bf16.
"""
import torch

NEG_INF = float("-inf")


def process_logits(logits, hist, n_hist, n_gen, penalty=1.0, ngram=0, bad=None, min_new=0, eos=None, round_bf16=True):
    """logits [R, V] (bf16, or fp32 for the pin against transformers) -> processed copy (bf16 unless round_bf16=False)."""
    x = logits.float()
    R, V = x.shape
    dev = x.device
    hist, n_hist, n_gen = hist.long(), n_hist.long().reshape(R), n_gen.long().reshape(R)
    L = hist.shape[1]
    live = torch.arange(L, device=dev)[None, :] < n_hist[:, None]
    inside = live & (hist >= 0) & (hist < V)
    spare = torch.full_like(hist, V)                              # column V takes everything that must not count
    if penalty != 1.0:
        seen = torch.zeros((R, V + 1), dtype=torch.bool, device=dev).scatter_(1, torch.where(inside, hist, spare), True)[:, :V]
        p = torch.tensor(float(penalty), dtype=torch.float32, device=dev)
        x = torch.where(seen, torch.where(x < 0, x * p, x / p), x)
    ban = torch.zeros((R, V + 1), dtype=torch.bool, device=dev)
    if ngram > 0 and L >= ngram:
        n = int(ngram)
        win = hist.unfold(1, n, 1)                                # [R, L - n + 1, n]
        start = torch.arange(L - n + 1, device=dev)[None, :]
        ok = (start + n <= n_hist[:, None]) & (n_hist[:, None] >= n)
        if n > 1:
            idx = (n_hist[:, None] - (n - 1) + torch.arange(n - 1, device=dev)[None, :]).clamp(0, L - 1)
            suffix = hist.gather(1, idx)
            ok = ok & (win[..., :-1] == suffix[:, None, :]).all(-1)
        last = win[..., -1]
        ok = ok & (last >= 0) & (last < V)
        ban.scatter_(1, torch.where(ok, last, torch.full_like(last, V)), True)
    for entry in bad or ():
        k, t = len(entry), int(entry[-1])
        if not 0 <= t < V or k > max(L, 1):
            continue
        hit = torch.ones(R, dtype=torch.bool, device=dev)
        if k > 1:
            hit = n_hist >= k
            for q in range(k - 1):
                pos = (n_hist - (k - 1) + q).clamp(0, L - 1)
                hit = hit & (hist.gather(1, pos[:, None]).squeeze(1) == int(entry[q]))
        ban[:, t] |= hit
    if eos is not None and 0 <= int(eos) < V and min_new > 0:
        ban[:, int(eos)] |= n_gen < int(min_new)
    x = x.masked_fill(ban[:, :V], NEG_INF)
    return x.to(torch.bfloat16) if round_bf16 else x


def push_stop(tokens, done, hist, n_hist, n_prompt, n_gen, eos, pad, stops):
    """One step's bookkeeping: a done row's token becomes pad; a live row's token is appended to its history (n_hist, n_gen + 1) and
    the row is done when the token is eos (eos None: never) or when its last len tokens equal a stop sequence and all of them were
    generated (n_gen >= len).  Returns new (tokens, done, hist, n_hist, n_gen), dtypes kept, inputs untouched."""
    R, dev = tokens.shape[0], tokens.device
    was = done != 0
    tok = torch.where(was, torch.full_like(tokens, 0 if pad is None else int(pad)), tokens)
    new_hist = hist.clone()
    at = n_hist.long().clamp(0, hist.shape[1] - 1)
    new_hist.scatter_(1, at[:, None], torch.where(was, hist.gather(1, at[:, None]).squeeze(1), tok.to(hist.dtype))[:, None])
    step = (~was).to(n_hist.dtype)
    nh, ng = n_hist + step, n_gen + step.to(n_gen.dtype)
    fin = torch.zeros(R, dtype=torch.bool, device=dev)
    if eos is not None:
        fin = tok == int(eos)
    for s in stops or ():
        k = len(s)
        same = ng.long() >= k
        for q in range(k):
            pos = (nh.long() - k + q).clamp(0, hist.shape[1] - 1)
            same = same & (new_hist.gather(1, pos[:, None]).squeeze(1) == int(s[q]))
        fin = fin | same
    return tok, (was | (fin & ~was)).to(done.dtype), new_hist, nh, ng


def first_stop(row, stops, eos=None):
    """Index of the token of `row` (a list of generated tokens) at which the row is done — the end of the first stop sequence found
    among the generated tokens, or the first eos — or None."""
    row = [int(t) for t in row]
    for i in range(len(row)):
        if eos is not None and row[i] == int(eos):
            return i
        for s in stops:
            if i + 1 >= len(s) and row[i + 1 - len(s):i + 1] == [int(t) for t in s]:
                return i
    return None
