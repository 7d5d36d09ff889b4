"""Shared pieces of the entropy-sampler tests (locally typical sampling, Mirostat v2): a plain-Python restatement of the definition in include/flm_gpu.h (flm_entropy) --
float32 scalars, sequential loops, libm's expf through ctypes --, an exact-rational restatement of flm_logf, the hand-built rows, the rows on which the summation order
decides the kept set, and the host loop the device-resident loop is compared with."""
import ctypes as C
import fractions

import numpy as np

from fast_llama_amd import capi
from sample_util import host_sample, logits_case
from shape_util import window_at

F = np.float32
NINF = F(-np.inf)
LOG2E = F(1.44269504)
Entropy = capi.Entropy

_libm = C.CDLL("libm.so.6")
_libm.expf.restype = C.c_float; _libm.expf.argtypes = [C.c_float]
_libm.logf.restype = C.c_float; _libm.logf.argtypes = [C.c_float]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def libm_logf(x):
    return np.array([_libm.logf(float(v)) for v in np.asarray(x, np.float32).reshape(-1)], dtype=np.float32)


def _fma(a, b, c):
    """one IEEE double fma: exact rational arithmetic, one rounding (Fraction -> float rounds to nearest even)"""
    return float(fractions.Fraction(a) * fractions.Fraction(b) + fractions.Fraction(c))


def py_logf(x):
    """csrc/flm_logf.h operation by operation in Python doubles (+, -, *, / are IEEE double operations; fma through exact rationals)"""
    ix = int(np.float32(x).view(np.uint32))
    k = (ix >> 23) - 127
    m = float(np.uint32((ix & 0x007FFFFF) | 0x3F800000).view(np.float32))
    if m > float.fromhex("0x1.6a09e667f3bcdp+0"):
        m = m * 0.5; k += 1
    s = (m - 1.0) / (m + 1.0)
    z = s * s
    q = 1.0 / 19.0
    for c in (17.0, 15.0, 13.0, 11.0, 9.0, 7.0, 5.0, 3.0):
        q = _fma(q, z, 1.0 / c)
    w = _fma(q, z, 1.0)
    return np.float32(_fma(float(k), float.fromhex("0x1.62e42fefa39efp-1"), (2.0 * s) * w))


def row_stats(R, T):
    """-> (d[n], e[n], sum, first maximum): every value an np.float32, the sum sequential in index order"""
    R = np.asarray(R, np.float32)
    y = [F(v) / F(T) for v in R]
    mx, first = y[0], 0
    for i, v in enumerate(y):
        if v > mx:
            mx, first = v, i
    d = [F(v - mx) for v in y]
    e = [F(0) if v < F(-15) else F(_libm.expf(float(v))) for v in d]
    s = F(0)
    for v in e:
        s = F(s + v)
    return d, e, s, first


def py_entropy(R, T, ent, mu=None, sum_h=None, sum_c=None):
    """the definition's stages 5 / 6 on one row -> the masked row.  sum_h / sum_c (the order tests): H / the cumulative c at position j computed by that function of the
    terms so far instead of the sequential chain"""
    R = np.asarray(R, np.float32)
    S = R.copy()
    if T == 0 or ent.mode == 0:
        return S
    d, e, s, first = row_stats(R, T)
    ls = capi.logf_host([s])[0]
    n = len(R)
    if ent.mode == 2:
        m = F(ent.struct().mu if mu is None else mu)
        for i in range(n):
            if e[i] == 0 or i == first:
                continue
            a = F(ls - d[i])
            if not (F(a * LOG2E) <= m):
                S[i] = NINF
        return S
    inv = F(1.0 / float(s))
    p = [F(v * inv) for v in e]
    h = [F(0) if e[i] == 0 else F(p[i] * F(ls - d[i])) for i in range(n)]
    if sum_h is None:
        H = F(0)
        for v in h:
            H = F(H + v)
    else:
        H = sum_h(np.array(h, np.float32))
    live = [i for i in range(n) if e[i] != 0]
    key = {i: F(abs(F(F(ls - d[i]) - H))) for i in live}
    order = sorted(live, key=lambda i: (key[i], i))
    last = len(order)
    c = F(0)
    for j, i in enumerate(order):
        c = F(c + p[i]) if sum_c is None else sum_c(np.array([p[k] for k in order[:j + 1]], np.float32))
        if c > F(ent.typical_p):
            last = j
            break
    for i in order[last + 1:]:
        S[i] = NINF
    return S


def py_mirostat_update(S, T, t, ent, mu):
    """obs and mu' behind the draw of t from the masked row S"""
    d, e, s, _ = row_stats(S, T)
    obs = F(F(capi.logf_host([s])[0] - d[t]) * LOG2E)
    return obs, F(F(mu) - F(F(ent.eta) * F(obs - F(ent.tau))))


def tree_sum(a):
    a = np.asarray(a, np.float32)
    while a.size > 1:
        if a.size % 2:
            a = np.append(a, F(0))
        a = (a[0::2] + a[1::2]).astype(np.float32)
    return F(a[0]) if a.size else F(0)


def hand_rows():
    """the hand-built rows: {name: logits}"""
    rows = {}
    for n in (2, 64, 1000):
        rows[f"equal {n}"] = np.full(n, 1.25, np.float32)
        dom = np.full(n, -40.0, np.float32); dom[n // 3] = 7.0                       # one dominant entry: every other d < -15, sum == 1
        rows[f"dominant {n}"] = dom
        ties = logits_case("medium", n, seed=3)
        ties[[0, n // 2, n - 1]] = ties.max() + F(1.0)                               # ties at the maximum
        rows[f"ties at the maximum {n}"] = ties
        rows[f"neginf {n}"] = logits_case("neginf", n, seed=4)
        edge = np.linspace(-14.0, -1.0, n).astype(np.float32)
        edge[0] = 0.0; edge[-1] = -15.0                                                # d == -15 exactly: alive
        if n > 2:
            edge[1] = np.nextafter(F(-15.0), NINF)                                     # just below: dead
        rows[f"clip edge {n}"] = edge
    return rows


def typical_walk(R, T, sum_h=None):
    """the candidates of stage 5 in their order, their p, and H -> (order, p[n], H)"""
    d, e, s, _ = row_stats(R, T)
    ls = capi.logf_host([s])[0]
    inv = F(1.0 / float(s))
    n = len(d)
    p = [F(v * inv) for v in e]
    h = np.array([F(0) if e[i] == 0 else F(p[i] * F(ls - d[i])) for i in range(n)], np.float32)
    if sum_h is None:
        H = F(0)
        for v in h:
            H = F(H + v)
    else:
        H = sum_h(h)
    live = [i for i in range(n) if e[i] != 0]
    key = {i: F(abs(F(F(ls - d[i]) - H))) for i in live}
    return sorted(live, key=lambda i: (key[i], i)), p, H


def order_case_H():
    """a row (T = 1) and a typical_p on which H summed as a pairwise tree gives another kept set than the sequential chain: the two sums differ in the last place, two
    candidates on either side of H then swap places in the order, and typical_p puts the cut between them"""
    rng = np.random.default_rng(0)
    for trial in range(200):
        L = (rng.standard_normal(3000) * 0.7).astype(np.float32)
        o1, p, H1 = typical_walk(L, 1.0)
        o2, _, H2 = typical_walk(L, 1.0, tree_sum)
        if H1 == H2 or o1 == o2:
            continue
        j = next(k for k in range(len(o1)) if o1[k] != o2[k])
        if j == 0:
            continue
        c = F(0)
        for i in o1[:j]:
            c = F(c + p[i])
        if 0 < c < 1:
            return L, Entropy(typical_p=float(c))                                     # c_(j-1) <= typical_p < c_j: the kept set ends with position j
    raise AssertionError("no row found")


def order_case_c():
    """the same for the cumulative sum c of the walk: typical_p lies between the chain's value and the tree's at one position, so only one of them passes it there"""
    rng = np.random.default_rng(1)
    for trial in range(200):
        L = (rng.standard_normal(1500) * 0.7).astype(np.float32)
        order, p, _ = typical_walk(L, 1.0)
        c = F(0)
        for j, i in enumerate(order):
            c = F(c + p[i])
            t = tree_sum(np.array([p[k] for k in order[:j + 1]], np.float32))
            if t != c:
                tp = min(c, t)
                if 0 < tp < 1:
                    return L, Entropy(typical_p=float(tp))
                break
    raise AssertionError("no row found")


def host_loop(ctx, H, prompt, n_tokens, s, ent, seed, stop=-1, rules=None, dfa=None, q=-1):
    """the loop flm_generate_ex runs on the device while flm_entropy_set is on, step by step through the host: flm_forward's logits, the constraint's mask, fh_shape over the
    window, fh_entropy, fh_sample_state (Mirostat: at topp = 1), fh_mirostat_update.  -> (ids, the sampler state, mu, the constraint state, masked-entry counts per step)"""
    ctx.reset_kv()
    hist, ids, state = [int(x) for x in prompt], [], int(seed)
    mu = F(ent.struct().mu)
    logits = ctx.forward(np.asarray(prompt, np.int32), 0)
    pos = len(hist)
    dropped = []
    while True:
        row = logits
        if q >= 0:
            row = capi.constrain_host(row, dfa.edges(q)[0])
        row = capi.shape_host(row, s, window_at(hist, s.penalty_last_n))
        live = int(np.count_nonzero(row != NINF))
        masked = capi.entropy_host(row, s.temperature, ent, mu=mu)
        dropped.append((int(np.count_nonzero(masked != NINF)), live))
        miro = ent.mode == 2 and s.temperature != 0
        tok, state = host_sample(H, masked, s.temperature, 1.0 if miro else s.topp, state)
        if miro:
            _, _, mu = capi.entropy_host(row, s.temperature, ent, mu=mu, chosen=tok)
        if q >= 0:
            q = capi.dfa_next_host(dfa, q, tok)
        ids.append(tok); hist.append(tok)
        fired = rules is not None and capi.stop_match_host(rules, ids, stop)[0] < len(ids)
        if tok == stop or fired or len(ids) >= n_tokens:
            return ids, state, mu, q, dropped
        logits = ctx.forward(np.array([tok], np.int32), pos)
        pos += 1
