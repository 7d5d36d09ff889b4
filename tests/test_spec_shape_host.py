"""Draft-and-verify under the sampling controls, without a GPU: the per-row windows (capi.row_windows) are the windows the shaped token loop uses, and the scheme itself --
shape row r over its own window, draw it with coin r + 1, cut at the first draw that differs from its draft -- reproduces the shaped loop's ids and final state on a fake
model whose logits are a seeded function of the fed prefix.  The host restatements only: capi.shape_host (host/sampler.cpp shape_logits) and sample_util.host_sample.

Also: the new symbols are declared, listed, exported and bound, and the teeth case tests/test_gpu_spec_shape.py reuses -- controls under which shaping every row with row
0's window gives other ids than per-row windows -- is asserted here in NumPy first."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from fast_llama_amd import capi
from sample_util import advance_state, host_lib, host_sample
from shape_util import Sampling, bits, np_shape, window_at
from test_spec_sample_host import _binding_calls, _declared_params

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DECLARED = {"flm_verify_sample_ex": 11, "flm_generate_lookup_ex": 14, "flm_op_shape_rows": 9}
V = 97
# teeth: a negative presence penalty of 1e4 lifts every id of the window above anything a model's logits reach.  With per-row windows row r >= 1 sees the drafts in front
# of it and repeats row 0's id; with row 0's (empty) window on every row the rows are the model's raw first maxima
TEETH = dict(temperature=0.0, presence_penalty=-1.0e4, penalty_last_n=16)


def fake_logits(prefix, seed=5):
    """the fake model: logits of the next token, a seeded function of everything fed so far"""
    h = 1469598103934665603
    for t in [seed] + [int(x) for x in prefix]:
        h = ((h ^ (t + 1)) * 1099511628211) & ((1 << 64) - 1)
    return (np.random.default_rng(h).standard_normal(V) * 3).astype(np.float32)


def shaped_loop(prompt, n, s, seed, logits_of=fake_logits):
    """the plain shaped loop (what flm_generate_ex runs): -> (ids, state)"""
    H = host_lib()
    hist, ids, state = [int(x) for x in prompt], [], int(seed)
    for _ in range(n):
        row = capi.shape_host(logits_of(hist), s, window_at(hist, s.penalty_last_n))
        tok, state = host_sample(H, row, s.temperature, s.topp, state)
        ids.append(tok); hist.append(tok)
    return ids, state


def verify_rows(hist, drafts, s, state, logits_of=fake_logits, per_row=True):
    """one verify batch behind hist: the rows' draws a[0 .. k] (row r fed with hist ++ drafts[:r], shaped over its own window -- per_row False: over row 0's --, drawn with
    the (r + 1)-th coin of `state`) -> (a, the states after 1 .. k + 1 draws)"""
    H = host_lib()
    wins = capi.row_windows(window_at(hist, s.penalty_last_n), drafts, s.penalty_last_n)
    a, states = [], []
    for r in range(len(drafts) + 1):
        raw = logits_of(list(hist) + [int(x) for x in drafts[:r]])
        tok, state = host_sample(H, capi.shape_host(raw, s, wins[r if per_row else 0]), s.temperature, s.topp, state)
        a.append(tok); states.append(state)
    return a, states


def verify_loop(prompt, n, s, seed, drafts_of, k):
    """the verify-and-cut loop: token 0 as the plain loop draws it, then batches of k drafts from drafts_of(step, hist) -> (ids, state, [accepted per step])"""
    ids, state = shaped_loop(prompt, 1, s, seed)
    hist, acc, step = [int(x) for x in prompt] + ids, [], 0
    while len(ids) < n:
        d = drafts_of(step, hist)
        a, states = verify_rows(hist, d, s, state)
        m = 0
        while m < k and a[m] == d[m]:
            m += 1
        take = min(m + 1, n - len(ids))
        ids += a[:take]; hist += a[:take]; state = states[take - 1]
        acc.append(take - 1); step += 1
    return ids, state, acc


# ---- the windows -------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_prompt,last_n,k,s_at", [(0, 8, 7, 0), (5, 8, 7, 0), (3, 8, 15, 2), (1100, 1024, 15, 40), (12, 0, 4, 3), (6, 1, 4, 0), (2, 64, 15, 9)])
def test_row_windows_are_the_loops_windows(n_prompt, last_n, k, s_at):
    """drafts = the loop's own ids: row r's window is the loop's window at step s + r.  n_window 0; n_window + r crossing last_n mid-batch (5 + r against 8); last_n 1024
    with a full window; last_n 0 and 1"""
    rng = np.random.default_rng(n_prompt + last_n)
    prompt = [int(x) for x in rng.integers(0, V, n_prompt)]
    ids = [int(x) for x in rng.integers(0, 5, s_at + k + 1)]              # (five values: ids repeat inside a batch, the counts change from row to row)
    hist = prompt + ids[:s_at]
    base = window_at(hist, last_n)
    assert len(base) == min(last_n, len(hist))
    wins = capi.row_windows(base, ids[s_at:s_at + k], last_n)
    assert len(wins) == k + 1
    for r in range(k + 1):
        want = window_at(prompt + ids[:s_at + r], last_n)
        assert wins[r].dtype == np.int32 and np.array_equal(wins[r], want), (r, list(wins[r]), list(want))
    if last_n:
        assert len(wins[k]) == min(last_n, len(hist) + k)


def test_rows_shaped_over_their_windows_are_the_definition():
    """a draft id repeated within the batch (its count, and with it the frequency penalty, changes per row) and a draft id that also carries a bias: shape_host over
    row_windows equals the NumPy definition over the loop's windows, row by row, and the rows differ from one another where the counts do"""
    window = [7, 11, 30]
    drafts = [11, 50, 11, 11, 50, 2, 11]                                   # 11: biased AND repeated; the window slides from row 3 on
    raw = fake_logits([1, 2, 3])
    pen = dict(repeat_penalty=1.2, frequency_penalty=0.3, presence_penalty=0.1, penalty_last_n=6, bias={11: 1.5, 4: -np.inf})
    for s in (Sampling(temperature=0.8, **pen), Sampling(temperature=0.8, top_k=9, min_p=0.02, **pen)):
        wins = capi.row_windows(window, drafts, s.penalty_last_n)
        rows = [capi.shape_host(raw, s, w) for w in wins]
        for r, w in enumerate(wins):
            assert np.array_equal(w, window_at(window + drafts[:r], s.penalty_last_n))
            assert np.array_equal(bits(rows[r]), bits(np_shape(raw, s, w))), r
        if s.top_k == 0:
            assert len({float(rows[r][11]) for r in (0, 1, 3)}) == 3 and np.isneginf(rows[0][4])      # 11 occurs 1, 2, 3 times
            assert len({r.tobytes() for r in rows}) >= 5


# ---- the scheme --------------------------------------------------------------------------------------------------------------------------------------------------
CONTROLS = dict(top_k=5, min_p=0.05, repeat_penalty=1.3, penalty_last_n=8, bias={3: 2.0, 7: -np.inf})


@pytest.mark.parametrize("k", [4, 15])
@pytest.mark.parametrize("t,p,seed,ctl", [(1.0, 0.9, 1234, CONTROLS), (0.0, 0.9, 3, CONTROLS), (0.7, 1.0, 0, CONTROLS),
                                         (1.0, 0.9, 77, dict(repeat_penalty=1.5, frequency_penalty=0.4, presence_penalty=0.2, penalty_last_n=8))])
def test_verify_and_cut_reproduces_the_shaped_loop(k, t, p, seed, ctl):
    """drafts that are right, wrong at 0, wrong at 2 and wrong at k - 1, step after step: the ids and the final state of the plain shaped loop, and exactly the accepted
    counts the wrong draft fixes"""
    s = Sampling(temperature=t, topp=p, **ctl)
    prompt, n = [1, 9, 40, 9, 3], 70
    ref, sref = shaped_loop(prompt, n + k + 1, s, seed)
    assert sref == (advance_state(seed, n + k + 1) if t else seed)
    wrong_at = (None, 0, 2, k - 1)

    def drafts_of(step, hist):
        at = len(hist) - len(prompt)
        d = list(ref[at:at + k])
        w = wrong_at[step % 4]
        if w is not None:
            d[w] = (d[w] + 1) % V
        return d
    ids, state, acc = verify_loop(prompt, n, s, seed, drafts_of, k)
    assert ids == ref[:n] and state == (advance_state(seed, n) if t else seed)
    full = [k if wrong_at[i % 4] is None else wrong_at[i % 4] for i in range(len(acc))]
    assert acc[:-1] == full[:len(acc) - 1] and acc[-1] <= full[len(acc) - 1] and sum(acc) > 0


def teeth_case(logits_of, hist, k, s):
    """-> (drafts = the per-row ids' first k, the per-row ids a[0 .. k], the ids with row 0's window on every row).  Temperature 0: no coin"""
    d = []
    for _ in range(k):
        a, _ = verify_rows(hist, d + [0] * (k - len(d)), s, 0, logits_of)
        d.append(a[len(d)])
    per_row, _ = verify_rows(hist, d, s, 0, logits_of)
    shared, _ = verify_rows(hist, d, s, 0, logits_of, per_row=False)
    return d, per_row, shared


def test_teeth_row_zeros_window_on_every_row_gives_other_ids():
    s = Sampling(**TEETH)
    d, per_row, shared = teeth_case(fake_logits, [], 15, s)
    assert per_row[:15] == d and per_row != shared, (per_row, shared)
    assert per_row == [per_row[0]] * 16 and shared[0] == per_row[0]        # the lifted id repeats; row 0 (the same window either way) agrees
    # ... and the plain shaped loop draws the per-row ids
    hist, want = [], []
    for _ in range(16):
        want.append(int(np.argmax(capi.shape_host(fake_logits(hist), s, window_at(hist, s.penalty_last_n)))))
        hist.append(want[-1])
    assert want == per_row


# ---- the boundary ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(DECLARED))
def test_new_symbols_are_declared_listed_exported_and_bound(name):
    hdr = open(os.path.join(ROOT, "include", "flm_gpu.h")).read()
    params = _declared_params(hdr, name)
    assert len(params) == DECLARED[name], params
    assert name in capi.SYMBOLS and hasattr(capi.lib(), name)
    calls = _binding_calls(name)
    assert calls and all(len(c) == len(params) for c in calls), (name, calls)


def test_bindings_and_header():
    v = list(inspect.signature(capi.Ctx.verify_sample_ex).parameters)
    assert v == ["self", "first_token", "drafts", "pos", "sampling", "window", "rng_state"], v
    g = list(inspect.signature(capi.Ctx.generate_lookup_ex).parameters)
    assert g[:9] == ["self", "prompt", "pos", "max_tokens", "sampling", "rng_state", "stop_token", "draft_len", "ngram_max"], g
    assert list(inspect.signature(capi.op_shape_rows).parameters) == ["logits", "n", "sampling", "window", "drafts"]
    hdr = open(os.path.join(ROOT, "include", "flm_gpu.h")).read()
    assert "does not take the controls" not in hdr and "each row of a verify batch would need a window of its own" not in hdr


def test_null_and_out_of_range_arguments_are_rejected_without_a_gpu():
    lib = capi.lib()
    n = C.c_int(0); st = C.c_uint64(5)
    sp, keep = Sampling(temperature=1.0, top_k=5).struct()
    assert lib.flm_verify_sample_ex(None, 1, None, 4, 0, C.byref(sp), None, 0, C.byref(st), None, C.byref(n)) != 0
    assert lib.flm_generate_lookup_ex(None, None, 1, 0, 1, C.byref(sp), C.byref(st), -1, 7, 3, None, None, None, C.byref(n)) != 0
    lg = (C.c_float * 64)(); out = (C.c_float * 64)(); d = (C.c_int32 * 16)()
    for rows, ld, nn in ((0, 8, 8), (17, 4, 4), (1, 8, 1), (1, 7, 8)):
        assert lib.flm_op_shape_rows(lg, rows, ld, nn, C.byref(sp), None, 0, d, out) == -1, (rows, ld, nn)
    assert lib.flm_op_shape_rows(lg, 2, 8, 8, C.byref(sp), None, 0, None, out) == -1           # two rows need a draft
    assert lib.flm_op_shape_rows(lg, 1, 8, 8, None, None, 0, d, out) == -1
    d[0] = 8
    assert lib.flm_op_shape_rows(lg, 2, 8, 8, C.byref(sp), None, 0, d, out) == -1               # a draft outside [0, n)
    assert st.value == 5
