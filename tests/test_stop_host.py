"""Stop rules without a GPU (include/flm_gpu.h: flm_stop_rules, flm_stop_validate, flm_stop_match; host/stop_rules.h): the host restatement equals the Python statement of
the definition (tests/stop_util.py) on the hand cases and on 2000 seeded streams; flm_stop_validate names every broken rule; the binding's surface."""
import ctypes as C
import os

import numpy as np
import pytest

import __graft_entry__ as graft
from fast_llama_amd import capi
from stop_util import ID, LENGTH, SEQ, TOKEN, py_stop_match, seeded_streams

A, B, X = 5, 6, 9


def both(ids, seqs, t, stop_token=-1):
    got = capi.stop_match_host(capi.StopRules(ids, seqs), t, stop_token)
    assert got == py_stop_match(ids, seqs, stop_token, t), (ids, seqs, stop_token, t, got)
    return got


def test_symbols_and_binding():
    hdr = open(os.path.join(graft.ROOT, "include", "flm_gpu.h")).read()
    lib = capi.lib()
    for sym in ("flm_stop_validate", "flm_stop_match", "flm_stop_set", "flm_op_stop_match"):
        assert sym + "(" in hdr and sym in capi.SYMBOLS and hasattr(lib, sym)
    for name, val in (("FLM_STOP_IDS_MAX", capi.STOP_IDS_MAX), ("FLM_STOP_SEQS_MAX", capi.STOP_SEQS_MAX), ("FLM_STOP_SEQ_LEN_MAX", capi.STOP_SEQ_LEN_MAX),
                      ("FLM_STOP_LENGTH", capi.STOP_LENGTH), ("FLM_STOP_TOKEN", capi.STOP_TOKEN), ("FLM_STOP_ID", capi.STOP_ID), ("FLM_STOP_SEQ", capi.STOP_SEQ),
                      ("FLM_STOP_CANCEL", capi.STOP_CANCEL)):
        assert f"#define {name} " in hdr and int(hdr.split(f"#define {name} ")[1].split()[0]) == val
    r = capi.StopRules(ids=[3, 4], seqs=[[1, 2], [7]])
    assert list(r.seq_ptr) == [0, 2, 3] and list(r.seq_tokens) == [1, 2, 7] and r.seqs == [[1, 2], [7]]
    assert list(capi.StopRules().seq_ptr) == [0] and capi.StopRules().n_seqs == 0


def test_hand_cases():
    # the overlap: a a b on a a a b fires at index 3 (a suffix comparison per index, not an automaton that loses the second a)
    assert both([], [[A, A, B]], [A, A, A, B]) == (3, SEQ, 0)
    # a sequence longer than the stream never fires
    assert both([], [[A, B, A, B]], [A, B, A]) == (3, LENGTH, 0)
    # a sequence equal to the whole stream fires at index L - 1
    assert both([], [[A, B, X]], [A, B, X]) == (2, SEQ, 0)
    # two sequences ending at one index: the lower s
    assert both([], [[X, B], [A, X, B], [B]], [A, X, B]) == (2, SEQ, 0)
    assert both([], [[A, X, B], [X, B]], [A, X, B]) == (2, SEQ, 0)
    # an id and a sequence at one index: the id
    assert both([X, B], [[A, B]], [A, B]) == (1, ID, 1)
    # the stop token at that index too: kind 1
    assert both([X, B], [[A, B]], [A, B], stop_token=B) == (1, TOKEN, 0)
    # nothing fires; no rules at all (NULL), with and without a stop token
    assert both([X], [[B, B]], [A, B, A]) == (3, LENGTH, 0)
    assert capi.stop_match_host(None, [A, B, A]) == (3, LENGTH, 0)
    assert capi.stop_match_host(None, [A, B, A], stop_token=B) == (1, TOKEN, 0)
    # a sequence of length 1 is an id in all but its kind
    assert both([], [[B]], [A, B]) == (1, SEQ, 0)
    # the largest sequence, 32 ids, at the end of a stream of 33
    q = list(range(100, 132))
    assert both([], [q], [99] + q) == (32, SEQ, 0)


def test_seeded_streams_equal_the_restatement():
    cases = seeded_streams()
    assert len(cases) == 2000
    fired = late_seq = 0
    for ids, seqs, stop_token, t in cases:
        assert max(t) < 4 and 1 <= len(t) <= 48
        first, kind, rule = both(ids, seqs, t, stop_token)
        if first < len(t):
            fired += 1
            if kind == SEQ and first >= len(seqs[rule]):
                late_seq += 1
    # the comparison is not vacuous: a good share of the streams fires, a good share does not, and many fire through a sequence well inside the stream
    assert 0.30 * len(cases) <= fired <= 0.90 * len(cases), fired
    assert late_seq >= 100, late_seq


def _raw(ids, ptr, toks):
    return capi.StopRules(raw=(ids, ptr, toks))


@pytest.mark.parametrize("what,make,words", [
    ("n_ids above the limit", lambda: (_raw(list(range(65)), [0], []), {}), "n_ids"),
    ("n_ids negative", lambda: (_raw([], [0], []), {"n_ids": -1}), "n_ids"),
    ("n_seqs above the limit", lambda: (_raw([], list(range(18)), list(range(17))), {}), "n_seqs"),
    ("n_seqs negative", lambda: (_raw([], [0], []), {"n_seqs": -1}), "n_seqs"),
    ("seq_ptr not starting at 0", lambda: (_raw([], [1, 3], [4, 5, 6]), {}), "start at 0"),
    ("seq_ptr decreasing", lambda: (_raw([], [0, 3, 2], [4, 5, 6]), {}), "decreasing"),
    ("a length of 0", lambda: (_raw([], [0, 2, 2], [4, 5]), {}), "length"),
    ("a length of 33", lambda: (_raw([], [0, 33], list(range(33))), {}), "length"),
    ("an id outside the vocabulary", lambda: (_raw([3, 320], [0], []), {}), "id outside"),
    ("a negative id", lambda: (_raw([-1], [0], []), {}), "id outside"),
    ("a sequence token outside the vocabulary", lambda: (_raw([], [0, 2], [4, 320]), {}), "sequence token outside"),
    ("a duplicate in ids", lambda: (_raw([3, 7, 3], [0], []), {}), "twice"),
])
def test_validate_names_the_broken_rule(what, make, words):
    rules, counts = make()
    st = rules.struct(**counts)
    assert capi.lib().flm_stop_validate(C.byref(st), 320) == -1, what
    assert words in capi.lib().flm_last_error(None).decode(), (what, capi.lib().flm_last_error(None))


def test_validate_accepts_the_limits():
    capi.StopRules(ids=list(range(64)), seqs=[list(range(32))] * 16).validate(320)
    capi.StopRules(ids=[319], seqs=[[0]]).validate(320)
    capi.StopRules().validate(320)
    with pytest.raises(capi.FlmError, match="stop: null struct"):
        capi._check(capi.lib().flm_stop_validate(None, 320))
