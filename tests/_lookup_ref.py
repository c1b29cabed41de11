"""Prompt-lookup decoding in plain Python: the drafting rule lmod_ngram_draft implements (HF PromptLookupCandidateGenerator plus the
stated cut at ids outside [0, V)) and a replay of the loop's rounds on plain greedy's own output.  No torch, no device."""


def ngram_draft(hist_row, k, max_ngram, V):
    """hist_row: the row's live history (a list of ints) whose last element is the pending next token.  For n = min(max_ngram, L-1)
    down to 1: the smallest window start i with hist[i:i+n] == hist[L-n:L] and i + n < L; the first n that has one wins.  The draft is
    hist[i+n : min(i+n+k, L)] cut before its first id outside [0, V) - an empty draft after the cut does NOT fall through to a shorter
    n.  Returns the draft (a list of 0..k ids)."""
    h = [int(t) for t in hist_row]
    L = len(h)
    for n in range(min(max_ngram, L - 1), 0, -1):
        tail = h[L - n:]
        for i in range(0, L - n):                      # i + n < L
            if h[i:i + n] == tail:
                out = []
                for t in h[i + n:min(i + n + k, L)]:
                    if not 0 <= t < V:
                        break
                    out.append(t)
                return out
    return []


def draft_arrays(hist_row, done, k, max_ngram, V):
    """What the kernel writes for one row: (draft [k]: the draft then -1, chunk [k+1]: pending token, draft, pending token again,
    n_draft).  A done row and a row of fewer than 2 tokens draft nothing; an empty row's pending token is 0."""
    h = [int(t) for t in hist_row]
    pending = h[-1] if h else 0
    d = [] if (done or len(h) < 2) else ngram_draft(h, k, max_ngram, V)
    return d + [-1] * (k - len(d)), [pending] + d + [pending] * (k - len(d)), len(d)


def push_block(block_row, k, hist_row, n_hist, ld_hist):
    """lmod_hist_push_block for one row: block_row is spec_accept's [k+5] row.  Returns the new (hist_row, n_hist)."""
    ne = int(block_row[k + 2])
    if ne < 1 or n_hist + ne > ld_hist:
        return list(hist_row), n_hist
    return list(hist_row[:n_hist]) + [int(t) for t in block_row[:ne]] + list(hist_row[n_hist + ne:]), n_hist + ne


def simulate(prompt_rows, greedy_tokens, k, max_ngram, V, eos=None):
    """Replays the prompt-lookup loop on plain greedy's output.  prompt_rows: per row the live prompt ids of the call; greedy_tokens:
    per row the N = max_new_tokens tokens plain greedy emits (anything behind a row's eos is not read).  A round drafts from the
    row's history (prompt + emitted, the pending token last), accepts the longest prefix of the draft that equals greedy's next
    tokens, emits it plus greedy's token behind it, cuts after an eos and at N.  The loop runs until every row has stopped, so
    the number of rounds is the slowest row's.  Returns (sequences: per row the emitted tokens, rounds, accepted: per row the number of
    emitted draft tokens) - `AssistedBookkeeper`'s counts."""
    seqs, rounds, accepted = [], 0, []
    for prompt, g in zip(prompt_rows, greedy_tokens):
        g = [int(t) for t in g]
        N = len(g)
        hist = [int(t) for t in prompt] + [g[0]]
        n, acc, r = 1, 0, 0
        stopped = (eos is not None and g[0] == eos) or n >= N
        while not stopped:
            r += 1
            draft = ngram_draft(hist, k, max_ngram, V)
            room = N - n                                 # greedy tokens still to emit: only these can be compared, and be taken
            n_acc = 0
            while n_acc < min(len(draft), room) and draft[n_acc] == g[n + n_acc]:
                n_acc += 1
            emitted = g[n:n + min(n_acc + 1, room)]      # accepted drafts equal greedy's tokens; then greedy's own next token
            if eos is not None and eos in emitted:
                emitted = emitted[:emitted.index(eos) + 1]
                stopped = True
            acc += min(n_acc, len(emitted))
            hist += emitted
            n += len(emitted)
            stopped = stopped or n >= N
        seqs.append(g[:n])
        accepted.append(acc)
        rounds = max(rounds, r)
    return seqs, rounds, accepted
