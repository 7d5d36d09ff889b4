"""Shared pieces of the log-probability tests (tests/test_logprob_host.py, tests/test_gpu_logprobs.py): the host restatement of a flm_logprob record (lib/libflm_host.so,
fh_logprob_row), an independent NumPy statement of the definition in include/flm_gpu.h, record comparison on the bit patterns, and the host loop -- flm_forward's logits,
the NumPy mask, fh_shape, fh_sample_state -- that keeps every step's raw and shaped row."""
import numpy as np

from fast_llama_amd import capi
from constraint_util import delta, np_mask, table
from sample_util import host_sample
from score_util import numpy_score
from shape_util import window_at

FIELDS = ("token", "logit", "max_logit", "sum", "n_top", "top_id", "top_logit", "pad_")
NMAX = capi.LOGPROBS_MAX


def host_logprob(logits, chosen, top_n):
    """fh_logprob_row on every row of logits[rows][n] -> capi.LOGPROB_DTYPE[rows]; chosen[rows]"""
    a = np.ascontiguousarray(logits, dtype=np.float32)
    a = a.reshape(1, -1) if a.ndim == 1 else a
    ch = np.asarray(chosen, np.int32).reshape(-1)
    return np.concatenate([capi.logprob_host(a[r], int(ch[r]), top_n) for r in range(a.shape[0])])


def order_key(x):
    """larger float <-> larger key, -0.0 and +0.0 share one"""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).copy()
    u[u == 0x80000000] = 0
    return np.where(u & 0x80000000, ~u, u | np.uint32(0x80000000)).astype(np.int64)


def numpy_logprob(x, chosen, top_n):
    """the definition once more, without the shim: the statistics from score_util.numpy_score, the order by np.lexsort on (index, -key)"""
    x = np.asarray(x, np.float32)
    sc = numpy_score(x, int(chosen))
    out = np.zeros(1, dtype=capi.LOGPROB_DTYPE)
    out["token"] = chosen; out["logit"] = x[chosen]; out["max_logit"] = sc["max_logit"]; out["sum"] = sc["sum"]
    k = min(int(top_n), x.size)
    order = np.lexsort((np.arange(x.size), -order_key(x)))[:k]
    out["n_top"] = k
    out["top_id"][0, :k] = order
    out["top_logit"][0, :k] = x[order]
    return out


def _bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same_records(a, b):
    """every field, bit for bit"""
    return a.shape == b.shape and all(np.array_equal(_bits(np.ascontiguousarray(a[f])), _bits(np.ascontiguousarray(b[f]))) for f in FIELDS)


def diff_records(a, b):
    if a.shape != b.shape:
        return {"shape": (a.shape, b.shape)}
    out = {}
    for f in FIELDS:
        x, y = _bits(np.ascontiguousarray(a[f])), _bits(np.ascontiguousarray(b[f]))
        if not np.array_equal(x, y):
            rows = np.nonzero((x != y).reshape(x.shape[0], -1).any(axis=1))[0][:4].tolist()
            out[f] = {r: (a[f][r].tolist(), b[f][r].tolist()) for r in rows}
    return out


def host_loop_rows(ctx, H, prompt, n_tokens, s, seed, dfa=None, q0=0, stop=-1):
    """shape_util.host_loop / constraint_util.host_loop, keeping the rows: -> (ids, the sampler state after them, raw rows L[len(ids)][V], shaped rows S[len(ids)][V])"""
    tab = table(dfa) if dfa is not None else None
    ctx.reset_kv()
    hist, ids, state, q = [int(x) for x in prompt], [], int(seed), int(q0)
    raw, shaped = [], []
    logits = ctx.forward(np.asarray(prompt, np.int32), 0)
    pos = len(hist)
    while True:
        L = logits.copy()
        masked = np_mask(L, dfa.edges(q)[0]) if dfa is not None else L
        S = capi.shape_host(masked, s, window_at(hist, s.penalty_last_n))
        tok, state = host_sample(H, S, s.temperature, s.topp, state)
        raw.append(L); shaped.append(S)
        ids.append(tok); hist.append(tok)
        if dfa is not None:
            q = delta(tab, q, tok)
        if tok == stop or len(ids) >= n_tokens:
            return ids, state, np.stack(raw), np.stack(shaped)
        logits = ctx.forward(np.array([tok], np.int32), pos)
        pos += 1


def expected_records(ids, raw, shaped, source, top_n):
    rows = raw if source == "raw" else shaped
    return host_logprob(rows, ids, top_n)
