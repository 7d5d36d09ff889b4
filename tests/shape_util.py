"""Shared pieces of the logit-shaping tests (tests/test_shape_host.py, tests/test_gpu_shape.py): an independent NumPy formulation of the definition in include/flm_gpu.h
(flm_sampling), the grid of cases both files run, and the host loop -- flm_forward logits, fh_shape, fh_sample_state -- whose ids flm_generate_ex must reproduce."""
import collections
import ctypes as C
import ctypes.util

import numpy as np

from fast_llama_amd import capi
from sample_util import host_sample, logits_case

Sampling = capi.Sampling
NINF = np.float32(-np.inf)
SIZES = (2, 63, 64, 65, 1000, 4099)
KINDS = ("medium", "ties", "neginf")

_libm = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.logf.restype = C.c_float
_libm.logf.argtypes = [C.c_float]


def logf(x):
    return np.float32(_libm.logf(C.c_float(float(x))))


def np_shape(logits, s, window=()):
    """the five-step definition, steps 1 - 4, in NumPy fp32: bias, penalties per distinct id (a Counter), top-k by a stable argsort of the negated values, min-p against
    libm's logf.  A stage whose control is neutral writes nothing."""
    S = np.array(logits, dtype=np.float32, copy=True)
    n = S.size
    ids, vals = s.bias_arrays()
    for i, b in zip(ids, vals):
        S[i] = np.float32(S[i] + np.float32(b))
    rp, fp, pp = np.float32(s.repeat_penalty), np.float32(s.frequency_penalty), np.float32(s.presence_penalty)
    if len(window) and (rp != 1 or fp != 0 or pp != 0):
        for t, c in collections.Counter(int(x) for x in window).items():
            x = S[t]
            if rp != 1:
                x = np.float32(x / rp) if x > 0 else np.float32(x * rp)
            if fp != 0 or pp != 0:
                x = np.float32(x - np.float32(np.float32(np.float32(c) * fp) + pp))
            S[t] = x
    if 0 < s.top_k < n:
        order = np.argsort(-S, kind="stable")           # larger value first, equal values (-0.0 == +0.0) by lower index
        S[order[s.top_k:]] = NINF
    if s.min_p > 0 and s.temperature != 0:
        lt = logf(np.float32(s.min_p))
        keep = S != NINF
        if keep.any():
            y = (S / np.float32(s.temperature)).astype(np.float32)
            mx = y[keep].max()
            S[keep & ((y - mx).astype(np.float32) < lt)] = NINF
    return S


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def windows(n, seed=0):
    """empty, length 1, one id repeated 300 times, all ids distinct (as many as the row has, at most 1024), 1024 ids drawn from 3 values"""
    rng = np.random.default_rng(100 + seed)
    d = min(n, 1024)
    return {"empty": np.empty(0, np.int32), "one": np.array([n // 2], np.int32), "rep300": np.full(300, n - 1, np.int32),
            "distinct": rng.permutation(n)[:d].astype(np.int32), "three": rng.choice(np.array([0, n // 2, n - 1]), 1024).astype(np.int32)}


PENALTIES = ((1.1, 0.0, 0.0), (0.5, 0.0, 0.0), (1.0, 0.3, 0.0), (1.0, 0.0, 0.4), (1.3, 0.2, -0.1), (1.0, 0.0, 0.0))


def grid(n):
    """(name, logits, Sampling, window) for one row size: every top-k of the issue on every logit family; every window under every penalty setting on rows that hold
    positive, negative, zero (both signs) and -inf entries at penalised ids; biases (finite, a ban, on a penalised id) with top-k and min-p behind them; min-p alone"""
    out = []
    for kind in KINDS:
        L = logits_case(kind, n, seed=11)
        for k in sorted({1, 2, 40, n - 1, n, n + 5}):
            out.append((f"{kind} top_k={k}", L, Sampling(temperature=0.7, top_k=k), ()))
        for mp, t in ((0.05, 0.7), (0.5, 1.0), (0.05, 0.0)):
            out.append((f"{kind} min_p={mp} t={t}", L, Sampling(temperature=t, min_p=mp), ()))
    for kind in ("medium", "neginf"):
        L = logits_case(kind, n, seed=12).copy()
        for wname, w in windows(n).items():
            Lw = L.copy()
            if len(w):                                   # the penalised ids cover every class of value
                u = np.unique(w)
                for j, v in enumerate((2.5, -1.5, 0.0, -0.0, -np.inf)):
                    Lw[u[j::5]] = np.float32(v)
            for rp, fp, pp in PENALTIES:
                out.append((f"{kind} window={wname} rp={rp} fp={fp} pp={pp}", Lw, Sampling(temperature=1.0, repeat_penalty=rp, frequency_penalty=fp, presence_penalty=pp), w))
    L = logits_case("medium", n, seed=13)
    w = windows(n)["three"]
    out.append(("bias finite", L, Sampling(temperature=0.7, bias={0: 1.5, n - 1: -2.25}), ()))
    out.append(("bias ban", L, Sampling(temperature=0.7, bias={int(np.argmax(L)): -np.inf, (int(np.argmax(L)) + 1) % n: 0.5}), ()))
    out.append(("bias on a penalised id, top-k, min-p", L, Sampling(temperature=0.7, top_k=min(40, n - 1), min_p=0.05, repeat_penalty=1.3, frequency_penalty=0.1,
                                                                 bias={n // 2: 3.0, 0: -np.inf}), w))
    return out


def window_at(history, last_n):
    return np.array(history[len(history) - min(last_n, len(history)):] if last_n > 0 else [], dtype=np.int32)


def host_loop(ctx, H, prompt, n_tokens, s, seed, stop=-1, shaped=True):
    """the loop flm_generate_ex runs on the device, step by step through the host: flm_forward's logits, fh_shape over the window (the last penalty_last_n ids of the prompt
    and what was generated since), fh_sample_state.  -> (ids, the sampler state after them).  shaped=False: the plain sampler on the raw logits."""
    ctx.reset_kv()
    hist, ids, state = [int(x) for x in prompt], [], int(seed)
    logits = ctx.forward(np.asarray(prompt, np.int32), 0)
    pos = len(hist)
    while True:
        row = capi.shape_host(logits, s, window_at(hist, s.penalty_last_n)) if shaped else logits
        tok, state = host_sample(H, row, s.temperature, s.topp, state)
        ids.append(tok); hist.append(tok)
        if tok == stop or len(ids) >= n_tokens:
            return ids, state
        logits = ctx.forward(np.array([tok], np.int32), pos)
        pos += 1
