"""Plain Python / NumPy reference of constrained decoding (the contract of lmod_constrain_mask_rows_bf16 and
lmod_constrain_advance_rows, include/lmod_hip.h), written from the rule and not from the kernels or the CSR packing: the automaton is
a dict of dicts,

    aut[s] = {"edges": {token: next or -1}, "default": d or -1, "accept": bool}          for s in 0 .. n-1

A state is CLOSED when its default is -1 (only tokens with an edge whose next is >= 0 are allowed) and OPEN otherwise (every token is
allowed, an unlisted one leads to the default, an edge with next -1 bans its token).  EOS is allowed in accepting states only.  A
state is TERMINAL when it is accepting, closed and has no allowed edge.  No HIP library, no torch.
"""
import numpy as np

NEG_INF_BITS = np.uint16(0xFF80)                     # bf16 -inf


def automaton(n_states, edges, accepting, default=None):
    """The dict-of-dicts form from the general constructor's arguments (default: None, one int, a list or a dict)."""
    if default is None:
        dflt = {}
    elif isinstance(default, dict):
        dflt = dict(default)
    elif isinstance(default, int):
        dflt = {s: default for s in range(n_states)}
    else:
        dflt = dict(enumerate(default))
    aut = {s: {"edges": {}, "default": dflt.get(s, -1), "accept": s in set(accepting)} for s in range(n_states)}
    for s, tok, nxt in edges:
        aut[s]["edges"][tok] = nxt
    return aut


def is_terminal(aut, s):
    st = aut[s]
    return st["accept"] and st["default"] < 0 and not any(n >= 0 for n in st["edges"].values())


def allowed(aut, s, tok, eos=None):
    """May a row in state s emit tok?"""
    st = aut[s]
    if st["default"] >= 0:                           # open: a listed ban refuses it, and so does the EOS rule
        return st["edges"].get(tok, 0) >= 0 and not (eos is not None and tok == eos and not st["accept"])
    return st["edges"].get(tok, -1) >= 0 or (eos is not None and tok == eos and st["accept"])


def mask(aut, bits, state, eos=None):
    """bits: uint16 [R, V], the bf16 logits' bit patterns; state: ints [R].  Returns the masked copy: a row whose state is outside
    the automaton is unchanged; elsewhere every element that `allowed` refuses becomes bf16 -inf and the others keep their bits."""
    out = np.array(bits, dtype=np.uint16, copy=True)
    R, V = out.shape
    for r in range(R):
        s = int(state[r])
        if s not in aut:
            continue
        st = aut[s]
        if st["default"] >= 0:                       # open: only the listed bans and the EOS rule
            for tok, nxt in st["edges"].items():
                if nxt < 0 and 0 <= tok < V:
                    out[r, tok] = NEG_INF_BITS
            if eos is not None and 0 <= eos < V and not st["accept"]:
                out[r, eos] = NEG_INF_BITS
            continue
        keep = np.zeros(V, dtype=bool)
        for tok, nxt in st["edges"].items():
            if nxt >= 0 and 0 <= tok < V:
                keep[tok] = True
        if eos is not None and 0 <= eos < V and st["accept"]:
            keep[eos] = True
        out[r, ~keep] = NEG_INF_BITS
    return out


def step(aut, s, tok):
    """The state after tok, or -1 when tok leaves the automaton."""
    st = aut[s]
    return st["edges"].get(int(tok), st["default"])


def advance(aut, tokens, done, state):
    """One step's bookkeeping after the push: a row that is done (before, or by this step's push) or whose state is outside the
    automaton is left alone; otherwise it follows its token - leaving the automaton sets done and keeps the state, entering a
    terminal state sets done.  Returns new (done, state) as int32 arrays."""
    done, state = np.array(done, dtype=np.int32, copy=True), np.array(state, dtype=np.int32, copy=True)
    for r in range(len(state)):
        s = int(state[r])
        if done[r] or s not in aut:
            continue
        ns = step(aut, s, tokens[r])
        if ns < 0:
            done[r] = 1
            continue
        state[r] = ns
        if is_terminal(aut, ns):
            done[r] = 1
    return done, state


def walk(aut, tokens, s=0):
    """Follow tokens from s: (state, ok); ok False at the first token that leaves the automaton (the state is the one it left)."""
    for tok in tokens:
        ns = step(aut, s, tok)
        if ns < 0:
            return s, False
        s = ns
    return s, True


def random_automaton(rng, n_states, vocab, max_edges=6, p_open=0.3):
    """(n_states, edges, accepting, default) of a random automaton without dead ends (rng: numpy Generator)."""
    edges, accepting, default = [], [], []
    for s in range(n_states):
        is_open = rng.random() < p_open
        default.append(int(rng.integers(0, n_states)) if is_open else -1)
        toks = rng.choice(vocab, size=int(rng.integers(0, max_edges + 1)), replace=False)
        nexts = [int(rng.integers(-1, n_states)) for _ in toks]
        edges += [(s, int(t), n) for t, n in zip(toks, nexts)]
        if rng.random() < 0.4 or (not is_open and not any(n >= 0 for n in nexts)):
            accepting.append(s)
    return n_states, edges, accepting, default
