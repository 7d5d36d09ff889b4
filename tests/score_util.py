"""Shared pieces of the scoring tests: the host restatement of a flm_score row (lib/libflm_host.so, fh_score_row: libm expf and a sequential loop) and an independent
NumPy / ctypes-libm evaluation of the same specification."""
import ctypes as C
import ctypes.util

import numpy as np

from fast_llama_amd import capi
from sample_util import host_lib

FIELDS = ("argmax", "target_logit", "max_logit", "sum", "prob")


def host_score(logits, targets=None):
    """fh_score_row on every row of logits[rows][n] -> capi.SCORE_DTYPE[rows]; targets[rows], -1 / None: no target"""
    H = host_lib()
    H.fh_score_row.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    H.fh_score_row.restype = None
    a = np.ascontiguousarray(logits, dtype=np.float32)
    a = a.reshape(1, -1) if a.ndim == 1 else a
    tg = np.full(a.shape[0], -1, np.int32) if targets is None else np.asarray(targets, np.int32).reshape(-1)
    out = np.zeros(a.shape[0], dtype=capi.SCORE_DTYPE)
    for r in range(a.shape[0]):
        H.fh_score_row(a[r].ctypes.data, int(a.shape[1]), int(tg[r]), out[r:r + 1].ctypes.data)
    return out


def next_targets(tokens):
    """the targets flm_score_tokens takes when none are given: the next token, none for the last row"""
    t = np.asarray(tokens, np.int32)
    return np.append(t[1:], np.int32(-1)).astype(np.int32)


def same_scores(a, b):
    """every field, bit for bit"""
    return all(np.array_equal(a[f].view(np.uint32) if a[f].dtype == np.float32 else a[f], b[f].view(np.uint32) if b[f].dtype == np.float32 else b[f]) for f in FIELDS)


def diff_scores(a, b):
    return {f: np.nonzero(a[f].view(np.uint32) != b[f].view(np.uint32))[0][:6].tolist() for f in FIELDS if not np.array_equal(a[f].view(np.uint32), b[f].view(np.uint32))}


_libm = None


def _expf():
    global _libm
    if _libm is None:
        _libm = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
        _libm.expf.argtypes = [C.c_float]; _libm.expf.restype = C.c_float
    return _libm.expf


def clipped_terms(x):
    """e_i = d < -15 ? 0 : expf(d), d = x - max, with the C library's expf"""
    x = np.asarray(x, np.float32)
    f = _expf()
    with np.errstate(invalid="ignore"):
        d = (x - x.max()).astype(np.float32)
    return np.array([0.0 if v < np.float32(-15) else f(float(v)) for v in d], np.float32)


def tree_sum(a):
    """pairwise fp32 sum: what a parallel reduction would compute"""
    a = np.asarray(a, np.float32)
    while a.size > 1:
        if a.size % 2:
            a = np.append(a, np.float32(0))
        a = (a[0::2] + a[1::2]).astype(np.float32)
    return a[0]


def teeth_row(trial, n=4096):
    """sample_util.teeth_logits' pattern of maxima and far-away entries, the maxima replaced by values around 0: the kept terms are inexact, so the ORDER of the sum shows"""
    from sample_util import logits_case, teeth_logits
    t = teeth_logits(trial, n)
    return np.where(t == 0.0, logits_case("flat", n, seed=trial), np.float32(-100.0)).astype(np.float32)


def numpy_score(x, target):
    """the specification once more, without the shim: fp32 NumPy scalars, expf from the C library through ctypes, a Python loop for the sum"""
    x = np.asarray(x, np.float32)
    arg = int(np.argmax(x))                          # NumPy's argmax returns the first maximum
    mx = x[arg]
    e = clipped_terms(x)
    s = np.float32(0)
    for v in e:
        s = np.float32(s + v)
    out = np.zeros(1, dtype=capi.SCORE_DTYPE)
    out["argmax"] = arg; out["max_logit"] = mx; out["sum"] = s
    if target >= 0:
        out["target_logit"] = x[target]
        out["prob"] = np.float32(e[target] * np.float32(1.0 / float(s)))
    return out
