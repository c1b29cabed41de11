"""Prompt-lookup decoding under continuous batching in plain Python: the two bookkeeping kernels (lmod_batch_lookup_first,
lmod_batch_lookup_round; include/lmod_hip.h) restated row by row, a replay of a whole generate_batch(prompt_lookup_num_tokens=k)
call on plain greedy's own output, and the hand-built rows both test files share.  No torch, no device.  TEST INFRASTRUCTURE ONLY."""
import _lookup_ref as LR


def ends_with_stop(hist, n_prompt, stops):
    """Do the generated tokens hist[n_prompt:] end with one of `stops`?  A match that needs a prompt token does not count."""
    n = len(hist)
    for s in stops:
        s = [int(t) for t in s]
        if len(s) >= 1 and n - len(s) >= max(n_prompt, 0) and hist[n - len(s):] == s:
            return True
    return False


def _ends(token, hist, n_prompt, n_gen, budget, eos, stops):
    return (eos is not None and token == eos) or ends_with_stop(hist, n_prompt, stops) or n_gen >= budget


def first_row(token, done, hist, n_prompt, n_gen, budget, eos=None, stops=(), ld_hist=None):
    """lmod_batch_lookup_first for one slot.  hist: the live history (a list).  Returns (first_tok, done, hist, n_gen)."""
    hist = list(hist)
    if done or n_gen != 0:
        return -1, done, hist, n_gen
    if ld_hist is not None and len(hist) >= ld_hist:
        return -1, 1, hist, n_gen
    hist.append(int(token))
    return int(token), int(_ends(int(token), hist, n_prompt, 1, budget, eos, stops)), hist, 1


def round_row(draft, target, first_tok, k, done, hist, n_prompt, n_gen, budget, cache_len, eos=None, pad=0, stops=(), ld_hist=None):
    """lmod_batch_lookup_round for one slot.  cache_len: as the verification pass left it (L0 + k + 1).  Returns (block row [k+6],
    done, hist, n_gen, cache_len)."""
    hist = list(hist)
    L0 = cache_len - (k + 1)
    if done or L0 < 0:
        return [pad] * (k + 1) + [0, 0, pad, 1, first_tok], 1, hist, n_gen, (L0 if L0 >= 0 else cache_len)
    n_acc = 0
    while n_acc < k and draft[n_acc] == target[n_acc]:
        n_acc += 1
    emitted, fin = [], False
    for c in [int(t) for t in draft[:n_acc]] + [int(target[n_acc])]:
        if ld_hist is not None and len(hist) >= ld_hist:
            fin = True
            break
        hist.append(c)
        n_gen += 1
        emitted.append(c)
        if _ends(c, hist, n_prompt, n_gen, budget, eos, stops):
            fin = True
            break
    ne = len(emitted)
    nxt = pad if (fin or not emitted) else emitted[-1]
    return emitted + [pad] * (k + 1 - ne) + [n_acc, ne, nxt, int(fin), first_tok], int(fin), hist, n_gen, L0 + ne


def replay(prompts, greedy, k, max_ngram, V, budgets, max_batch_size, eos=None, stops=(), pad=0):
    """The whole call on plain greedy's output.  prompts: per request the prompt ids (text only: a prompt takes len(prompt) cache
    positions); greedy: per request at least budget tokens of plain greedy's continuation (not cut at eos or a stop sequence: the
    replay cuts).  The verification rows' argmax is greedy's next token as long as the chunk so far equals greedy's tokens; behind
    the first wrong draft token, and past the end of `greedy`, it is a value no draft holds (-2), which nothing reads.  Returns
    (tokens per request, admissions [(iteration, request, slot)], rounds, accepted per request, lens: per round the [B] cache
    lengths after it)."""
    R, B = len(prompts), max_batch_size
    slots = [dict(req=None, done=1, hist=[], n_prompt=0, n_gen=0, budget=1, lens=0) for _ in range(B)]
    tokens, accepted, admissions, lens_trace = [[] for _ in range(R)], [0] * R, [], []
    nxt, rounds = 0, 0
    while nxt < R or any(sl["req"] is not None for sl in slots):
        for s, sl in enumerate(slots):                              # all free slots, ascending, in request order
            if sl["req"] is None and nxt < R:
                sl.update(req=nxt, done=0, hist=[int(t) for t in prompts[nxt]], n_prompt=len(prompts[nxt]), n_gen=0,
                          budget=int(budgets[nxt]), lens=len(prompts[nxt]))
                admissions.append((rounds, nxt, s))
                nxt += 1
        for s, sl in enumerate(slots):
            r = sl["req"]
            g = [int(t) for t in greedy[r]] if r is not None else []
            ft, sl["done"], sl["hist"], sl["n_gen"] = first_row(g[0] if g else 0, sl["done"], sl["hist"], sl["n_prompt"], sl["n_gen"],
                                                                 sl["budget"], eos, stops)
            draft = LR.draft_arrays(sl["hist"], sl["done"], k, max_ngram, V)[0]
            target, ok = [], True
            for j in range(k + 1):
                i = sl["n_gen"] + j
                target.append(g[i] if ok and i < len(g) else -2)
                ok = ok and j < k and i < len(g) and draft[j] == g[i]
            row, sl["done"], sl["hist"], sl["n_gen"], sl["lens"] = round_row(
                draft, target, ft, k, sl["done"], sl["hist"], sl["n_prompt"], sl["n_gen"], sl["budget"], sl["lens"] + k + 1, eos, pad,
                stops)
            if r is None:
                continue
            if row[k + 5] >= 0:
                tokens[r].append(row[k + 5])
            tokens[r] += row[:row[k + 2]]
            accepted[r] += min(row[k + 1], row[k + 2])
            if row[k + 4]:
                sl["req"] = None
        rounds += 1
        lens_trace.append([sl["lens"] for sl in slots])
    return tokens, admissions, rounds, accepted, lens_trace


# ------------------------------------------------------------------------------------------------ the hand-built rows
EOS, PAD, STOPS, LD = 9, 0, [[41, 42, 43]], 64


def clause_rows(k):
    """Eight slots, one row kind each (some carry a second clause), for any k in 1..15.  d_j = 10 + j is the draft alphabet.  Returns a
    list of dicts: name, draft [k], target [k+1], first_tok, done, hist, n_prompt, n_gen, budget, cache_len (L0 + k + 1)."""
    D = [10 + j for j in range(k)]
    junk = [70 + j for j in range(k + 1)]
    nd = min(2, k - 1)                       # the partial run's accepted tokens
    m = min(1, k - 1)                        # where eos sits inside the accepted run
    a = k // 2                               # accepted tokens in front of an eos correction
    e = max(1, (k + 1) // 2)                 # tokens the budget leaves inside a fully accepted run (< k + 1)
    eos_run = D[:m] + [EOS] + D[m + 1:]
    rows = [
        dict(name="done slot, first_tok carried through", draft=[-1] * k, target=junk, first_tok=77, done=1, hist=[1, 2, 3, 77],
             n_prompt=3, n_gen=1, budget=1, L0=20),
        dict(name="n_acc 0; 41 42 | 43 would need the prompt's 41", draft=D, target=[43] + junk[1:], first_tok=-1, done=0,
             hist=[5, 41, 42], n_prompt=2, n_gen=1, budget=40, L0=2),
        dict(name="n_acc k", draft=D, target=D + [60], first_tok=-1, done=0, hist=[1, 2, 3, 4, 30], n_prompt=4, n_gen=1, budget=40,
             L0=4),
        dict(name="partial run, -1 tail, budget reached exactly by the last candidate", draft=D[:nd] + [-1] * (k - nd),
             target=D[:nd] + [61] + junk[nd + 1:], first_tok=-1, done=0, hist=[1, 2, 31, 32], n_prompt=2, n_gen=2, budget=2 + nd + 1,
             L0=3),
        dict(name="eos inside the accepted run", draft=eos_run, target=eos_run + [62], first_tok=-1, done=0, hist=[1, 2, 3, 33],
             n_prompt=3, n_gen=1, budget=40, L0=3),
        dict(name="eos as the correction token", draft=D, target=D[:a] + [EOS] + junk[a + 1:], first_tok=-1, done=0, hist=[1, 34],
             n_prompt=1, n_gen=1, budget=40, L0=1),
        dict(name="budget reached inside the run", draft=D, target=D + [63], first_tok=-1, done=0, hist=[1, 2, 35, 36, 37],
             n_prompt=2, n_gen=3, budget=3 + e, L0=4),
        dict(name="stop sequence: two tokens of earlier rounds plus one of this round", draft=[43] + D[1:],
             target=[43] + D[1:] + [64], first_tok=-1, done=0, hist=[1, 2, 38, 41, 42], n_prompt=2, n_gen=3, budget=40, L0=4),
    ]
    for r in rows:
        r["cache_len"] = r.pop("L0") + k + 1
    return rows


def run_rows(rows, k, eos=EOS, pad=PAD, stops=STOPS, ld_hist=LD):
    """round_row over `rows`: ([block rows], [done], [hist], [n_gen], [cache_len])."""
    out = [round_row(r["draft"], r["target"], r["first_tok"], k, r["done"], r["hist"], r["n_prompt"], r["n_gen"], r["budget"],
                     r["cache_len"], eos, pad, stops, ld_hist) for r in rows]
    return tuple(list(x) for x in zip(*out))
