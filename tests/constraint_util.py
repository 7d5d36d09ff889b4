"""Shared pieces of the constrained-decoding tests (tests/test_constraint_host.py, tests/test_gpu_constraint.py, tests/test_gpu_constraint_cli.py): an independent NumPy
step 0 (a boolean mask from the edge list), delta as a dict lookup, the automata both files use, and the host loop of shape_util.host_loop with the automaton in front --
mask -> fh_shape -> fh_sample_state -> delta -- whose ids and states the armed _ex entry points must reproduce."""
import numpy as np

from fast_llama_amd import capi
from sample_util import host_sample
from shape_util import NINF, window_at

Dfa = capi.Dfa
SIZES = (2, 63, 64, 65, 1000, 4099, 32767, 32768, 32769, 65537)


def np_mask(logits, tokens):
    """step 0: -inf wherever the index has no edge"""
    S = np.array(logits, dtype=np.float32, copy=True)
    allowed = np.zeros(S.size, dtype=bool)
    allowed[np.asarray(tokens, dtype=np.int64)] = True
    S[~allowed] = NINF
    return S


def table(dfa):
    """{(state, token): next}"""
    return {(q, int(t)): int(n) for q in range(dfa.n_states) for t, n in zip(*dfa.edges(q))}


def delta(tab, q, t):
    return tab.get((int(q), int(t)), int(q))


def fold(tab, q, ids):
    for t in ids:
        q = delta(tab, q, t)
    return q


def edge_lists(n):
    """the allowed sets step 0 is checked on: only id 0, only id n - 1, both sides of 32768 (where the row reaches it), every second id, all ids"""
    out = {"first": [0], "last": [n - 1], "every2": list(range(0, n, 2)), "all": list(range(n))}
    if n > 32768:
        out["around32768"] = [32767, 32768]
    return out


def cycle3(V):
    """state i allows the ids = i (mod 3) and goes to (i + 1) % 3: ids[s] % 3 == (q0 + s) % 3 needs no reference"""
    return Dfa.from_edges(3, [(q, t, (q + 1) % 3) for q in range(3) for t in range(q, V, 3)])


def pairs(V, seed=5):
    """8 states, two allowed ids each, pseudo-random targets"""
    rng = np.random.default_rng(seed)
    tr = []
    for q in range(8):
        a, b = sorted(int(x) for x in rng.choice(V, 2, replace=False))
        tr += [(q, a, int(rng.integers(0, 8))), (q, b, int(rng.integers(0, 8)))]
    return Dfa.from_edges(8, tr)


def ends(V, stop):
    """three steps of cycle3, then a state whose only edge is the stop id onto itself"""
    tr = [(q, t, q + 1) for q in range(3) for t in range(q, V, 3)]
    return Dfa.from_edges(4, tr + [(3, int(stop), 3)])


def wide(V):
    """one state with all V ids: must change no bit"""
    return Dfa.from_edges(1, [(0, t, 0) for t in range(V)])


def host_loop(ctx, H, prompt, n_tokens, s, seed, dfa, q0, stop=-1):
    """-> (ids, the sampler state after them, the automaton state after them)"""
    tab = table(dfa)
    ctx.reset_kv()
    hist, ids, state, q = [int(x) for x in prompt], [], int(seed), int(q0)
    logits = ctx.forward(np.asarray(prompt, np.int32), 0)
    pos = len(hist)
    while True:
        row = capi.shape_host(np_mask(logits, dfa.edges(q)[0]), s, window_at(hist, s.penalty_last_n))
        tok, state = host_sample(H, row, s.temperature, s.topp, state)
        ids.append(tok); hist.append(tok)
        q = delta(tab, q, tok)
        if tok == stop or len(ids) >= n_tokens:
            return ids, state, q
        logits = ctx.forward(np.array([tok], np.int32), pos)
        pos += 1
