"""Plain Python reference of drafting what a constraint forces (the contract of lmod_constrain_draft and lmod_constrain_accept,
include/lmod_hip.h) over the dict-of-dicts automaton of tests/_constrain_ref.py, written from the rule and not from the kernels or
the CSR packing, and a replay of the loop's rounds on plain constrained greedy's own output.  No HIP library, no torch."""
import _constrain_ref as CR


def automaton_of(c):
    """A generation.TokenConstraint as the dict-of-dicts automaton."""
    return CR.automaton(c.n_states, c.edges(), [s for s in range(c.n_states) if c.accept[s]], list(c.default_next))


def forced(aut, s, eos=None, V=None):
    """(token, next) when state s is FORCED, else None: closed, not terminal, and the set the mask would allow - the edges with
    next >= 0 and 0 <= token < V, plus eos where the state accepts and 0 <= eos < V - is exactly one listed edge, not eos."""
    if s not in aut:
        return None
    st = aut[s]
    if st["default"] >= 0 or CR.is_terminal(aut, s):
        return None
    inside = lambda t: t >= 0 and (V is None or t < V)
    ok = {t: n for t, n in st["edges"].items() if n >= 0 and inside(t)}
    if eos is not None and inside(eos) and st["accept"]:
        return None                                  # eos is in the set: beside an edge (two elements) or alone (not a listed edge)
    if len(ok) != 1:
        return None
    (t, n), = ok.items()
    return None if (eos is not None and t == eos) else (t, n)


def draft_row(aut, pending, s, done, k, eos=None, V=None):
    """One row of lmod_constrain_draft: (draft [k], chunk [k+1], vstate [k+1], n_draft)."""
    run, states = [], []
    if not done and s in aut:
        states.append(s)
        while len(run) < k:
            f = forced(aut, states[-1], eos, V)
            if f is None:
                break
            run.append(f[0])
            states.append(f[1])
        if CR.is_terminal(aut, states[-1]):
            states[-1] = -1
    n = len(run)
    return run + [-1] * (k - n), [pending] + run + [pending] * (k - n), states + [-1] * (k + 1 - len(states)), n


def draft(aut, pending, state, done, k, eos=None, V=None):
    """All rows: (draft [R][k], chunk [R][k+1], vstate [R][k+1], n_draft [R])."""
    rows = [draft_row(aut, int(p), int(s), bool(d), k, eos, V) for p, s, d in zip(pending, state, done)]
    return tuple([r[i] for r in rows] for i in range(4))


def accept_row(aut, dr, tg, done, s, n_gen, budget, lens, k, eos=None, pad=0):
    """One row of lmod_constrain_accept.  Returns (block [k+5], next, done, state, n_gen, lens_target)."""
    len0 = lens - (k + 1)
    if done:
        return [pad] * (k + 1) + [0, 0, pad, 1], pad, 1, s, n_gen, len0
    n_acc = 0
    while n_acc < k and dr[n_acc] == tg[n_acc]:
        n_acc += 1
    emitted, fin = [], 0
    for tok in list(dr[:n_acc]) + [tg[n_acc]]:
        emitted.append(tok)
        n_gen += 1
        if eos is not None and tok == eos:
            fin = 1
        elif s in aut:
            ns = CR.step(aut, s, tok)
            if ns < 0:
                fin = 1
            else:
                s = ns
                if CR.is_terminal(aut, ns):
                    fin = 1
        if n_gen >= budget:
            fin = 1
        if fin:
            break
    nxt = pad if fin else emitted[-1]
    block = emitted + [pad] * (k + 1 - len(emitted)) + [n_acc, len(emitted), nxt, fin]
    return block, nxt, fin, s, n_gen, len0 + len(emitted)


def accept(aut, drafts, targets, done, state, n_gen, budget, lens_target, k, eos=None, pad=0):
    """All rows: (block [R][k+5], next [R], done [R], state [R], n_gen [R], lens_target [R])."""
    rows = [accept_row(aut, [int(t) for t in d], [int(t) for t in g], bool(dn), int(s), int(n), budget, int(L), k, eos, pad)
            for d, g, dn, s, n, L in zip(drafts, targets, done, state, n_gen, lens_target)]
    return tuple([r[i] for r in rows] for i in range(6))


def simulate_row(aut, start, tokens, k, eos=None, max_new=None, V=None):
    """Replays the loop on ONE row's plain constrained-greedy tokens (anything behind the token that ends the row is not read).  The
    first token comes from the prefill; then every round drafts the forced run from the row's state, accepts the longest prefix that
    equals greedy's next tokens (behind max_new greedy has none: the budget cuts there whatever the target is) and emits through
    `accept_row`.  Returns (emitted tokens, rounds, accepted, final state)."""
    g = [int(t) for t in tokens]
    N = len(g) if max_new is None else max_new
    s, out = start, [g[0]]
    done = 0
    if eos is not None and g[0] == eos:
        done = 1
    else:
        ns = CR.step(aut, s, g[0])
        if ns < 0:
            done = 1
        else:
            s = ns
            done = int(CR.is_terminal(aut, ns))
    done = done or len(out) >= N
    rounds = acc = 0
    while not done:
        rounds += 1
        dr, _, _, _ = draft_row(aut, out[-1], s, False, k, eos, V)
        n = len(out)
        tg = [g[n + j] if n + j < len(g) else (dr[j] if j < k and dr[j] >= 0 else 0) for j in range(k + 1)]
        block, _, done, s, n_gen, _ = accept_row(aut, dr, tg, False, s, n, N, k + 1, k, eos, 0)
        ne = block[k + 2]
        out += block[:ne]
        acc += min(block[k + 1], ne)
        assert n_gen == len(out)
    return out, rounds, acc, s


def simulate(constraint, tokens, k, eos=None, max_new=None):
    """Every row of a batch (tokens: per row plain constrained greedy's tokens): (sequences, rounds of the loop = the slowest row's,
    accepted per row, final states) - `AssistedBookkeeper`'s counts and generate()'s `constraint_states`."""
    aut = automaton_of(constraint)
    rows = [simulate_row(aut, constraint.start, t, k, eos, max_new) for t in tokens]
    return [r[0] for r in rows], max(r[1] for r in rows), [r[2] for r in rows], [r[3] for r in rows]
