"""Cache slots behind a shared prefix, without a GPU (include/flm_gpu.h: flm_batch_layout_prefix_for, flm_batch_open_prefix, flm_generate_batch_prefix,
flm_op_attention_slots_prefix / _segs_prefix): the symbols in the header, in capi.SYMBOLS and in the library; the layout against a Python statement of the rule; the
binding's argument checks."""
import ctypes as C
import os

import numpy as np
import pytest

import __graft_entry__ as graft
from fast_llama_amd import capi

SYMS = ("flm_batch_layout_prefix_for", "flm_batch_open_prefix", "flm_generate_batch_prefix", "flm_op_attention_slots_prefix", "flm_op_attention_segs_prefix")


def test_symbols_and_binding():
    hdr = open(os.path.join(graft.ROOT, "include", "flm_gpu.h")).read()
    lib = capi.lib()
    for sym in SYMS:
        assert sym + "(" in hdr and sym in capi.SYMBOLS and hasattr(lib, sym)
    assert '"batch_prefix"' in hdr
    assert callable(capi.op_attention_slots_prefix) and callable(capi.op_attention_segs_prefix)


def py_layout(S, rows, max_seq_len):
    """the rule as the header states it: None where the call refuses"""
    if S < 0 or not 1 <= len(rows) <= 16 or any(r < 1 for r in rows) or S + sum(rows) > max_seq_len:
        return None
    return [S + sum(rows[:s]) for s in range(len(rows))], list(rows)


def c_layout(S, rows, max_seq_len):
    out = capi.BatchLayout()
    out.n_slots = -7
    r = np.asarray(list(rows) + [1], dtype=np.int32)
    rc = capi.lib().flm_batch_layout_prefix_for(S, len(rows), r.ctypes.data_as(C.c_void_p), max_seq_len, C.byref(out))
    if rc != 0:
        assert rc == -1 and out.n_slots == -7, "a refused layout writes nothing"
        return None
    return [out.base[s] for s in range(len(rows))], [out.rows[s] for s in range(len(rows))]


@pytest.mark.parametrize("S", [0, 1, 64, 512, -1])
@pytest.mark.parametrize("rows", [[1], [9] * 16, [3, 70, 1, 200], [1] * 17, [5, 0, 3]], ids=["one", "sixteen", "ragged", "seventeen", "empty-slot"])
def test_layout_is_the_rule(S, rows):
    fit = max(S, 0) + sum(rows)
    for max_seq_len in (fit - 1, fit, fit + 1, 4096):                     # one row over, the exact fit, one to spare
        assert c_layout(S, rows, max_seq_len) == py_layout(S, rows, max_seq_len), (S, rows, max_seq_len)
    if S == 0 and py_layout(0, rows, 4096):                               # S = 0: flm_batch_layout_for's layout
        lay = capi.batch_layout(rows, 4096)
        assert c_layout(0, rows, 4096) == (list(lay.base[:len(rows)]), list(lay.rows[:len(rows)]))


def test_layout_edges_and_the_binding():
    assert c_layout(64, [8, 100, 20], 192) == ([64, 72, 172], [8, 100, 20]) and c_layout(2 ** 30, [2 ** 30] * 3, 2 ** 31 - 1) is None      # sums past 2^31 do not wrap
    lib, r = capi.lib(), np.array([200, 100], np.int32)
    assert lib.flm_batch_layout_prefix_for(4, 2, None, 512, C.byref(capi.BatchLayout())) == -1 and lib.flm_batch_layout_prefix_for(4, 2, r.ctypes.data_as(C.c_void_p), 512, None) == -1
    assert lib.flm_batch_layout_prefix_for(8, 2, r.ctypes.data_as(C.c_void_p), 307, C.byref(capi.BatchLayout())) == -1 and b"exceed max_seq_len" in lib.flm_last_error(None)
    assert lib.flm_batch_layout_prefix_for(-1, 2, r.ctypes.data_as(C.c_void_p), 512, C.byref(capi.BatchLayout())) == -1 and b"prefix rows" in lib.flm_last_error(None)
    lay = capi.batch_layout([5, 7, 3], 64, prefix_rows=10)
    assert (lay.n_slots, list(lay.base[:3]), list(lay.rows[:3])) == (3, [10, 15, 22], [5, 7, 3])
    for bad in ({"max_seq_len": 24, "prefix_rows": 10}, {"max_seq_len": 64, "prefix_rows": -2}):
        with pytest.raises(capi.FlmError, match="flm error -1"):
            capi.batch_layout([5, 7, 3], **bad)


def test_binding_argument_checks():
    class NoCtx(capi.Ctx):
        def __init__(self):
            self._h = C.c_void_p()
            self.desc = None
    ctx = NoCtx()
    R = capi.BatchReq
    with pytest.raises(ValueError):
        ctx.generate_batch([], prefix_rows=4)
    with pytest.raises(ValueError):
        ctx.generate_batch([R([1, 2], 0)], prefix_rows=4)
    kc = np.zeros((2, 16, 64), np.float32); x = np.zeros((2, 128), np.float32)
    with pytest.raises(ValueError):
        capi.op_attention_slots_prefix(kc, kc.copy(), x, x, x, 2, 64, 16, 4, [4, 8], [4], [4, 8])              # rows: one entry per row
    with pytest.raises(ValueError):
        capi.op_attention_segs_prefix(kc, kc.copy(), x, x, x[:1], 2, 64, 16, 4, [4], [8], [2], [4])            # q, k, v of one shape
    # a NULL context or NULL arrays: the library itself refuses, nothing is touched
    lib = capi.lib()
    lay = capi.batch_layout([8, 8], 64, prefix_rows=4)
    assert lib.flm_batch_open_prefix(None, C.byref(lay), 4) == -1
    assert lib.flm_generate_batch_prefix(None, 4, None, 1, None, None, None, 4, None, None) == -1
    assert lib.flm_op_attention_slots_prefix(None, None, None, None, None, None, 1, 64, 16, 4, 1, None, None, None) == -1
    assert lib.flm_op_attention_segs_prefix(None, None, None, None, None, None, 1, 64, 16, 4, 1, 1, 0, None, None, None, None) == -1
