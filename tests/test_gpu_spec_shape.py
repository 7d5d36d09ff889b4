"""Draft-and-verify under the sampling controls: k_shape_rows (flm_op_shape_rows), flm_verify_sample_ex, flm_generate_lookup_ex and bin/main --draft / --lookup with the
control flags.  Everything is equality: ids with np.array_equal, sampler states as 64-bit integers, shaped rows and K/V rows on bit patterns.

References: the host restatement (capi.shape_host over capi.row_windows) and k_shape_logits row by row; a flm_forward_sample_ex loop / flm_generate_ex on a SECOND context
(the shaped token path); the loop's steps simulated on the reference ids with the drafter's host restatement.  Models, the looping prompt and the simulation are those of
tests/test_gpu_spec.py; the controls are CONTROLS of tests/test_gpu_shape.py and a penalties-only set whose window (8 ids) slides inside a batch; max_seq_len is 256."""
import ctypes
import dataclasses
import os
import re
import subprocess

import numpy as np
import pytest

import __graft_entry__ as graft
from fast_llama_amd import flmfile as ff
from sample_util import advance_state
from shape_util import Sampling, bits, grid
from test_gpu_shape import CONTROLS
from test_gpu_spec import MAX_SEQ, _caches, _ctx, _looping_prompt, _model, _model_7b, _prompt, _record, _simulate
from test_spec_shape_host import TEETH, teeth_case

pytestmark = pytest.mark.gpu

PEN_ONLY = dict(repeat_penalty=1.3, frequency_penalty=0.2, presence_penalty=0.1, penalty_last_n=8)
SETS = {"controls": CONTROLS, "penalties": PEN_ONLY}
SETTINGS = ((1.0, 0.9, 1234), (0.0, 0.9, 3), (1.0, 0.9, 0), (0.7, 0.5, 77))


def _after(s0, t, draws):
    return advance_state(s0, draws) if t != 0 else s0


# ---- k_shape_rows ------------------------------------------------------------------------------------------------------------------------------------------------
def _rows_case(L, s, w, n, seed):
    """16 rows that differ (row r = the case's row rotated by 7 r), a window length the batch slides over (penalty_last_n = len(w) + 3, at most 1024) and 15 drafts that
    repeat and hit the grid's bias ids (0, n // 2, n - 1)"""
    rng = np.random.default_rng(seed)
    rows = np.stack([np.roll(L, 7 * r) for r in range(16)]).astype(np.float32)
    pool = np.array([0, n // 2, n - 1, int(rng.integers(0, n)), int(rng.integers(0, n))])
    drafts = rng.choice(pool, 15).astype(np.int32)
    return rows, dataclasses.replace(s, penalty_last_n=min(1024, len(w) + 3)), drafts


@pytest.mark.parametrize("n", [2, 65, 4099])
def test_op_shape_rows_is_the_host_restatement_row_by_row(gpu, n):
    """the grid of the shaper's tests (every top-k, min-p, window and penalty setting, biases) on 1, 5 and 16 rows, rows n and n + 5 floats apart (the padding holds NaN);
    every row against shape_host over its own window, bit for bit -- a histogram, a window or a threshold shared between rows would show"""
    bad = []
    for ci, (name, L, s, w) in enumerate(grid(n)):
        rows, sl, drafts = _rows_case(L, s, w, n, 1000 + ci)
        wins = gpu.row_windows(w, drafts, sl.penalty_last_n)
        want = np.stack([gpu.shape_host(rows[r], s, wins[r]) for r in range(16)])
        padded = np.full((16, n + 5), np.nan, np.float32); padded[:, :n] = rows
        for nr in (1, 5, 16):
            for lg in (rows, padded):
                got = gpu.op_shape_rows(lg[:nr], n, sl, w, drafts[:nr - 1])
                if got.shape != (nr, n) or not np.array_equal(bits(got), bits(want[:nr])):
                    bad.append((name, nr, lg.shape[1]))
    assert not bad, bad[:8]


@pytest.mark.parametrize("n", [65, 4099])
def test_op_shape_rows_is_k_shape_logits_row_by_row(gpu, n):
    """against the token path's own kernel (flm_op_shape_logits with row r's window): one definition, two kernels"""
    for ci, (name, L, s, w) in enumerate(grid(n)[::3]):
        rows, sl, drafts = _rows_case(L, s, w, n, 2000 + ci)
        wins = gpu.row_windows(w, drafts, sl.penalty_last_n)
        got = gpu.op_shape_rows(rows, n, sl, w, drafts)
        for r in (0, 1, 4, 15):
            assert np.array_equal(bits(got[r]), bits(gpu.op_shape_logits(rows[r], s, wins[r]))), (name, r)


def test_op_shape_rows_has_no_vocabulary_bound(gpu):
    """n = 40000, above the sampler's LDS bound: 16 rows, top-k with penalties, min-p and a ban"""
    n = 40000
    L = (np.random.default_rng(8).standard_normal(n) * 3).astype(np.float32)
    s = Sampling(temperature=0.7, top_k=40, min_p=0.05, repeat_penalty=1.3, frequency_penalty=0.1, bias={n // 2: 3.0, 0: -np.inf})
    w = np.random.default_rng(9).integers(0, n, 1024).astype(np.int32)
    rows, sl, drafts = _rows_case(L, s, w, n, 3)
    wins = gpu.row_windows(w, drafts, sl.penalty_last_n)
    got = gpu.op_shape_rows(rows, n, sl, w, drafts)
    for r in range(16):
        assert np.array_equal(bits(got[r]), bits(gpu.shape_host(rows[r], s, wins[r]))), r


# ---- flm_verify_sample_ex ----------------------------------------------------------------------------------------------------------------------------------------
def _window_of(hist, last_n):
    return hist[len(hist) - min(last_n, len(hist)):] if last_n > 0 else []


def _ref_loop(ref, first, pos, n, s, window, s0):
    """the caller's loop the contract names: n successive flm_forward_sample_ex calls behind first at pos, the window slid over the ids drawn -> (ids, state)"""
    hist, ids, state, tok = [int(x) for x in window], [], s0, int(first)
    for i in range(n):
        tok, state = ref.forward_sample_ex(np.array([tok], np.int32), pos + i, s, _window_of(hist, s.penalty_last_n), rng_state=state)
        ids.append(tok); hist.append(tok)
    return np.array(ids, np.int32), state


def _verify_cases(gpu, cfg, tensors, gemms, positions, ks, s, s0):
    ref = _ctx(gpu, cfg, tensors)
    ctx = _ctx(gpu, cfg, tensors)
    V, t = cfg.vocab_size, s.temperature
    prompt = _prompt(V, 37)
    shaped0 = ctx.query("shaped_tokens")
    delivered = 0
    for pos in positions:
        def start(c):
            c.reset_kv()
            return c.forward_argmax(prompt, 0) if pos == 37 else 1
        # the caller's window in front of the batch: none at pos 0, the prompt's last penalty_last_n ids behind it, three ids elsewhere (n_window <= penalty_last_n)
        window = [] if pos == 0 else [int(x) for x in prompt[-s.penalty_last_n:]] if pos == 37 else [5, 9, 5]
        first = start(ref)
        n_ref = min(20, MAX_SEQ - pos)
        ids, s_ref = _ref_loop(ref, first, pos, n_ref, s, window, s0)
        assert s_ref == _after(s0, t, n_ref)
        kv_ref = _caches(ref, cfg)
        for k in ks:
            if pos + k + 1 > MAX_SEQ:
                continue
            for wrong in (None, 0, 2, k - 1):
                drafts = ids[:k].copy()
                if wrong is not None:
                    drafts[wrong] = (drafts[wrong] + 1) % V
                m = k if wrong is None else wrong
                for gemm in gemms:
                    ctx.set_option("spec_gemm", gemm)
                    assert start(ctx) == first
                    got, st = ctx.verify_sample_ex(first, drafts, pos, s, window, s0)
                    delivered += len(got)
                    assert len(got) == m + 1 and np.array_equal(got, ids[:m + 1]), (pos, k, wrong, gemm, list(got), list(ids[:m + 1]))
                    assert st == _after(s0, t, m + 1), (pos, k, wrong, gemm)
                    for a, b in zip(_caches(ctx, cfg), kv_ref):
                        assert np.array_equal(a[:, :pos + m + 1], b[:, :pos + m + 1]), (pos, k, wrong, gemm)
                    # the caller's loop continues from the returned position, state and window
                    tail = min(3, n_ref - (m + 1))
                    if tail > 0:
                        cont, s_cont = _ref_loop(ctx, got[-1], pos + m + 1, tail, s, window + [int(x) for x in got], st)
                        assert np.array_equal(cont, ids[m + 1:m + 1 + tail]) and s_cont == _after(s0, t, m + 1 + tail), (pos, k, wrong, gemm)
                        delivered += tail
    assert ctx.query("shaped_tokens") == shaped0 + delivered and ctx.query("fallback") == 0
    ref.close(); ctx.close()


@pytest.mark.parametrize("t,p,s0", SETTINGS)
@pytest.mark.parametrize("which", list(SETS))
def test_verify_sample_ex_is_the_callers_shaped_loop(gpu, which, t, p, s0):
    """drafts = the reference loop's ids with none / the first / draft 2 / draft k - 1 made wrong: n_out, the ids, the state after n_out draws, the K/V rows pos .. pos + m
    and the loop's continuation; k = 4 and 15; pos = 0, 37 (behind a batched prompt) and pos + k + 1 == max_seq_len; "spec_gemm" 0 and 1"""
    cfg, tensors = _model("tiny-int8")
    _verify_cases(gpu, cfg, tensors, (1, 0), (0, 37, MAX_SEQ - 16, MAX_SEQ - 5), (4, 15), Sampling(temperature=t, topp=p, **SETS[which]), s0)


def test_verify_sample_ex_int16_and_7b_width(gpu):
    cfg, tensors = _model("tiny-int16")
    _verify_cases(gpu, cfg, tensors, (0,), (0, 37), (4, 15), Sampling(temperature=1.0, topp=0.9, **CONTROLS), 1234)
    cfg, tensors = _model_7b()                                                 # 32000 entries: 16 rows shaped, then sorted, at once
    _verify_cases(gpu, cfg, tensors, (1, 0), (0,), (15,), Sampling(temperature=1.0, topp=0.9, **CONTROLS), 1234)
    _verify_cases(gpu, cfg, tensors, (1,), (0,), (15,), Sampling(temperature=0.0, **PEN_ONLY), 3)


def test_teeth_every_row_has_a_window_of_its_own(gpu):
    """the case of tests/test_spec_shape_host.py on the model's logits: asserted in NumPy first -- row 0's window on every row gives other ids --, then the device returns the
    per-row ids, which are the shaped loop's"""
    cfg, tensors = _model("tiny-int8")
    ref = _ctx(gpu, cfg, tensors)
    ctx = _ctx(gpu, cfg, tensors)
    s, k = Sampling(**TEETH), 7
    found = None
    for first in (1, 2, 3, 5, 8):
        def logits_of(prefix):
            ref.reset_kv()
            return ref.forward(np.array([first] + [int(x) for x in prefix], np.int32), 0)
        d, per_row, shared = teeth_case(logits_of, [], k, s)
        if per_row != shared:
            found = (first, d, per_row, shared)
            break
    assert found, "no start token at which a shared window changes the ids"
    first, d, per_row, shared = found
    assert per_row[:k] == d
    got, _ = ctx.verify_sample_ex(first, d, 0, s, (), None)
    assert [int(x) for x in got] == per_row and [int(x) for x in got] != shared
    ref.reset_kv()
    assert [int(x) for x in _ref_loop(ref, first, 0, k + 1, s, [], 0)[0]] == per_row
    ref.close(); ctx.close()


def test_verify_sample_ex_neutral_controls_are_verify_sample(gpu):
    cfg, tensors = _model("tiny-int8")
    ctx = _ctx(gpu, cfg, tensors)
    n0 = ctx.query("shaped_tokens")
    for t, p, s0 in ((1.0, 0.9, 1234), (0.0, 0.9, 3)):
        ctx.reset_kv()
        ids, _ = ctx.decode_sample(1, 0, 8, t, p, s0) if t else (ctx.decode_greedy(1, 0, 8), s0)
        drafts = ids[:7].copy(); drafts[4] = (drafts[4] + 1) % cfg.vocab_size
        ctx.reset_kv()
        want = ctx.verify_sample(1, drafts, 0, t, p, s0)
        for s, w in ((Sampling(temperature=t, topp=p), ()), (Sampling(temperature=t, topp=p, top_k=cfg.vocab_size, repeat_penalty=1.3, penalty_last_n=0), ()),
                     (Sampling(temperature=t, topp=p, penalty_last_n=4), [3, 4])):
            ctx.reset_kv()
            got = ctx.verify_sample_ex(1, drafts, 0, s, w, s0)
            assert np.array_equal(got[0], want[0]) and len(got[0]) == 5 and got[1] == want[1]
    assert ctx.query("shaped_tokens") == n0
    ctx.close()


# ---- flm_generate_lookup_ex --------------------------------------------------------------------------------------------------------------------------------------
LOOKUP = {
    "top_k 1": (1.0, 0.9, 1234, dict(top_k=1)),                                                       # the greedy cycle of the looping prompt, drawn at temperature 1
    "top_k 1, mild penalty": (1.0, 0.9, 1234, dict(top_k=1, repeat_penalty=1.05, penalty_last_n=8)),
    "controls": (1.0, 0.9, 1234, CONTROLS),
    "controls t 0": (0.0, 0.9, 3, CONTROLS),
    "penalties state 0": (1.0, 0.9, 0, PEN_ONLY),
}


@pytest.mark.parametrize("K", [4, 15])
@pytest.mark.parametrize("which", list(LOOKUP))
def test_generate_lookup_ex_is_generate_ex(gpu, which, K):
    """ids, n_out, the callback sequence with `last`, the final state and the K/V rows against flm_generate_ex on a second context; the step counters against the loop
    simulated on the reference ids.  top_k = 1 at temperature 1 reproduces the greedy cycle: the simulated loop accepts drafts there, asserted on the SIMULATED value"""
    t, p, s0, ctl = LOOKUP[which]
    s = Sampling(temperature=t, topp=p, **ctl)
    cfg, tensors = _model("tiny-int8")
    prompt, _ = _looping_prompt(gpu)
    ref = _ctx(gpu, cfg, tensors)
    ctx = _ctx(gpu, cfg, tensors)
    G, N = 3, 60
    a_seen, a_cb = _record(); b_seen, b_cb = _record()
    want, s_want = ref.generate_ex(prompt, 0, N, s, rng_state=s0, on_token=a_cb)
    n0, m0 = ctx.query("shaped_tokens"), ctx.query("sampled_tokens")
    got, s_got = ctx.generate_lookup_ex(prompt, 0, N, s, rng_state=s0, draft_len=K, ngram_max=G, on_token=b_cb)
    assert len(want) == N and s_want == _after(s0, t, N)
    assert np.array_equal(got, want) and s_got == s_want
    assert a_seen == b_seen and len(b_seen) == N and b_seen[-1][2]
    assert ctx.query("shaped_tokens") == n0 + N and ctx.query("sampled_tokens") == m0 + (N if t else 0)
    steps, accepted, _ = _simulate(gpu, prompt, want, K, G)
    print("shaped lookup", which, "K", K, "steps", ctx.query("spec_steps"), "accepted", ctx.query("spec_accepted"), "simulated", (steps, accepted))
    assert (ctx.query("spec_steps"), ctx.query("spec_accepted")) == (steps, accepted)
    if which == "top_k 1":
        assert accepted >= 1 and steps < N - 1
    for x, y in zip(_caches(ctx, cfg), _caches(ref, cfg)):
        assert np.array_equal(x[:, :len(prompt) + N - 1], y[:, :len(prompt) + N - 1])
    assert ctx.query("fallback") == 0
    ref.close(); ctx.close()


@pytest.mark.parametrize("K", [4, 15])
@pytest.mark.parametrize("which", ["top_k 1", "controls"])
def test_generate_lookup_ex_stop_cut_tail_and_cancel(gpu, which, K):
    t, p, s0, ctl = LOOKUP[which]
    s = Sampling(temperature=t, topp=p, **ctl)
    cfg, tensors = _model("tiny-int8")
    prompt, _ = _looping_prompt(gpu)
    ref = _ctx(gpu, cfg, tensors)
    ctx = _ctx(gpu, cfg, tensors)
    G, N = 3, 60
    want, _ = ref.generate_ex(prompt, 0, N, s, rng_state=s0)
    _, _, runs = _simulate(gpu, prompt, want, K, G)
    # a stop token hit mid-run: inside an accepted run where the loop has one, else at the first id not seen before index 5
    inside = [a + j for a, n in runs for j in range(1, n) if want[a + j] not in want[:a + j]]
    later = [i for i in range(5, N) if want[i] not in want[:i]]
    cut = inside[0] if inside else later[0]
    stop = int(want[cut])
    a_seen, a_cb = _record(); b_seen, b_cb = _record()
    ref.reset_kv(); ctx.reset_kv()
    want_s, sa = ref.generate_ex(prompt, 0, N, s, rng_state=s0, stop_token=stop, on_token=a_cb)
    got_s, sb = ctx.generate_lookup_ex(prompt, 0, N, s, rng_state=s0, stop_token=stop, draft_len=K, ngram_max=G, on_token=b_cb)
    assert len(want_s) == cut + 1 and want_s[-1] == stop
    assert np.array_equal(got_s, want_s) and a_seen == b_seen and b_seen[-1] == (cut, stop, True)
    assert sa == sb == _after(s0, t, cut + 1)
    assert (ctx.query("spec_steps"), ctx.query("spec_accepted")) == _simulate(gpu, prompt, want, K, G, stop=stop)[:2]
    # max_tokens cutting a run (1: no step at all; 2: a single-token step behind the prompt's id; 7: inside what K = 15 would accept)
    for n in (1, 2, 7):
        ref.reset_kv(); ctx.reset_kv()
        a_seen, a_cb = _record(); b_seen, b_cb = _record()
        w, sa = ref.generate_ex(prompt, 0, n, s, rng_state=s0, on_token=a_cb)
        g, sb = ctx.generate_lookup_ex(prompt, 0, n, s, rng_state=s0, draft_len=K, ngram_max=G, on_token=b_cb)
        assert np.array_equal(g, w) and len(g) == n and a_seen == b_seen and sa == sb == _after(s0, t, n), n
        assert (ctx.query("spec_steps"), ctx.query("spec_accepted")) == _simulate(gpu, prompt, want[:n], K, G)[:2], n
    # a call whose tail reaches max_seq_len: the last steps are single shaped tokens whose windows hold generated ids
    pos = MAX_SEQ - len(prompt) - 30 + 1
    a_seen, a_cb = _record(); b_seen, b_cb = _record()
    ref.reset_kv(); ctx.reset_kv()
    want_e, sa = ref.generate_ex(prompt, pos, 30, s, rng_state=s0, on_token=a_cb)
    got_e, sb = ctx.generate_lookup_ex(prompt, pos, 30, s, rng_state=s0, draft_len=K, ngram_max=G, on_token=b_cb)
    assert len(want_e) == 30 and np.array_equal(got_e, want_e) and a_seen == b_seen and sa == sb == _after(s0, t, 30)
    assert ctx.query("spec_steps") < 29
    for x, y in zip(_caches(ctx, cfg), _caches(ref, cfg)):
        assert np.array_equal(x[:, pos:pos + len(prompt) + 29], y[:, pos:pos + len(prompt) + 29])
    # a callback that cancels at index 5
    def cancelling(seen):
        return lambda i, tok, last: seen.append((i, tok, last)) or i == 5
    a_seen, b_seen = [], []
    ref.reset_kv(); ctx.reset_kv()
    want_c, _ = ref.generate_ex(prompt, 0, N, s, rng_state=s0, on_token=cancelling(a_seen))
    got_c, sb = ctx.generate_lookup_ex(prompt, 0, N, s, rng_state=s0, draft_len=K, ngram_max=G, on_token=cancelling(b_seen))
    assert a_seen == b_seen and len(b_seen) == 6
    assert 6 <= len(got_c) <= N and np.array_equal(got_c, want[:len(got_c)]) and np.array_equal(want_c, want[:len(want_c)])
    assert sb == _after(s0, t, len(got_c))
    assert ctx.query("fallback") == 0
    ref.close(); ctx.close()


def test_generate_lookup_ex_neutral_controls_are_generate_lookup_sample(gpu):
    cfg, tensors = _model("tiny-int8")
    prompt, _ = _looping_prompt(gpu)
    ctx = _ctx(gpu, cfg, tensors)
    n0 = ctx.query("shaped_tokens")
    for t, p, s0 in ((1.0, 0.9, 0), (0.0, 0.9, 3)):
        a_seen, a_cb = _record(); b_seen, b_cb = _record()
        ctx.reset_kv()
        want = ctx.generate_lookup_sample(prompt, 0, 40, t, p, s0, draft_len=7, on_token=a_cb)
        counters = (ctx.query("spec_steps"), ctx.query("spec_accepted"))
        ctx.reset_kv()
        got = ctx.generate_lookup_ex(prompt, 0, 40, Sampling(temperature=t, topp=p, top_k=cfg.vocab_size, penalty_last_n=16), rng_state=s0, draft_len=7, on_token=b_cb)
        assert np.array_equal(got[0], want[0]) and got[1] == want[1] and a_seen == b_seen
        assert (ctx.query("spec_steps"), ctx.query("spec_accepted")) == counters
    assert ctx.query("shaped_tokens") == n0
    ctx.close()


def test_generate_lookup_ex_other_models(gpu):
    for name, gemm in (("tiny-int16", 0), ("small-int8", 1)):
        cfg, tensors = _model(name)
        ref = _ctx(gpu, cfg, tensors)
        ctx = _ctx(gpu, cfg, tensors)
        ctx.set_option("spec_gemm", gemm)
        block = _prompt(cfg.vocab_size, 9, seed=6)
        prompt = np.concatenate([block, block, block]).astype(np.int32)
        s = Sampling(temperature=1.0, topp=0.9, **CONTROLS)
        want, sa = ref.generate_ex(prompt, 0, 50, s, rng_state=1234)
        got, sb = ctx.generate_lookup_ex(prompt, 0, 50, s, rng_state=1234, draft_len=7, ngram_max=4)
        assert np.array_equal(got, want) and sa == sb
        assert (ctx.query("spec_steps"), ctx.query("spec_accepted")) == _simulate(gpu, prompt, want, 7, 4)[:2]
        ref.close(); ctx.close()


def test_temperature_zero_has_no_vocabulary_bound(gpu):
    """vocab 40000: at temperature 0 both calls run and equal the token path; at temperature != 0 the sampler's refusal stays"""
    from fast_llama_amd import synth
    cfg = synth.make_config("tiny", ff.QT_INT8)
    cfg.vocab_size = 40000
    tensors = synth.make_tensors(cfg, seed=59)
    ref = _ctx(gpu, cfg, tensors)
    ctx = _ctx(gpu, cfg, tensors)
    prompt = _prompt(cfg.vocab_size, 12)
    s = Sampling(temperature=0.0, top_k=5, repeat_penalty=1.3, penalty_last_n=8, bias={3: 2.0})
    want, _ = ref.generate_ex(prompt, 0, 20, s)
    got, _ = ctx.generate_lookup_ex(prompt, 0, 20, s, draft_len=7)
    assert np.array_equal(got, want) and len(got) == 20
    ref.reset_kv(); ctx.reset_kv()                                           # (the verify passes of the call above left rows behind its last position)
    ids, _ = _ref_loop(ref, 1, 40, 8, s, [], 0)
    got, _ = ctx.verify_sample_ex(1, ids[:7], 40, s, (), None)
    assert np.array_equal(got, ids)
    hot = Sampling(temperature=1.0, top_k=5)
    with pytest.raises(gpu.FlmError, match="flm error -2"):
        ctx.generate_lookup_ex(prompt, 0, 8, hot, rng_state=1)
    with pytest.raises(gpu.FlmError, match="flm error -2"):
        ctx.verify_sample_ex(1, ids[:7], 40, hot, (), 1)
    ref.close(); ctx.close()


# ---- the contract around the calls -------------------------------------------------------------------------------------------------------------------------------
def test_a_retried_shaped_lookup_call_delivers_every_index_once(gpu):
    """after a timed-out cross-workgroup wait (injected) the step re-runs from the history, the state and the parameter block the host held at its start: the same ids and
    state as an undisturbed call, every index once.  The call ends at max_seq_len, so it includes single-token steps"""
    cfg, tensors = _model("tiny-int8")
    prompt, _ = _looping_prompt(gpu)
    pos, N = MAX_SEQ - len(prompt) - 12 + 1, 12
    for which in ("controls", "top_k 1", "controls t 0"):
        t, p, s0, ctl = LOOKUP[which]
        s = Sampling(temperature=t, topp=p, **ctl)
        ref = _ctx(gpu, cfg, tensors)
        ctx = _ctx(gpu, cfg, tensors)
        a_seen, a_cb = _record(); b_seen, b_cb = _record()
        want, sa = ref.generate_lookup_ex(prompt, pos, N, s, rng_state=s0, draft_len=7, on_token=a_cb)
        assert ref.query("spec_steps") < N - 1
        ref.reset_kv()
        assert np.array_equal(want, ref.generate_ex(prompt, pos, N, s, rng_state=s0)[0])
        ctx.set_option("inject_wait_failure", 1)
        got, sb = ctx.generate_lookup_ex(prompt, pos, N, s, rng_state=s0, draft_len=7, on_token=b_cb)
        assert np.array_equal(got, want) and sb == sa == _after(s0, t, N)
        assert b_seen == a_seen and [i for i, _, _ in b_seen] == list(range(N))
        assert ctx.query("fallback") == 1 and ref.query("fallback") == 0
        ref.close(); ctx.close()


def test_nothing_is_allocated_inside_the_shaped_calls(gpu):
    """the first flm_verify_sample_ex and flm_generate_lookup_ex of a fresh context (batch steps and, at the end, a single-token step), bracketed with hipMemGetInfo"""
    hip = ctypes.CDLL("libamdhip64.so")

    def free_bytes():
        f, t = ctypes.c_size_t(0), ctypes.c_size_t(0)
        assert hip.hipMemGetInfo(ctypes.byref(f), ctypes.byref(t)) == 0
        return f.value
    cfg, tensors = _model("tiny-int8")
    prompt, _ = _looping_prompt(gpu)
    ctx = _ctx(gpu, cfg, tensors)
    s = Sampling(temperature=1.0, topp=0.9, **CONTROLS)
    gpu.spec_draft_host([1, 2], 4, 1)                  # (the host library is loaded before the bracket)
    f0 = free_bytes()
    a, _ = ctx.verify_sample_ex(1, [2, 3, 4, 5, 6, 7, 8], 0, s, [9, 9], 1234)
    f1 = free_bytes()
    b, _ = ctx.generate_lookup_ex(prompt, 0, 40, s, rng_state=1234, draft_len=7)
    f2 = free_bytes()
    ctx.generate_lookup_ex(prompt, 0, 40, Sampling(temperature=0.0, **PEN_ONLY), draft_len=15)
    ctx.set_option("spec_gemm", 1 - ctx.query("spec_gemm"))
    c, _ = ctx.verify_sample_ex(1, [2, 3, 4, 5, 6, 7, 8], 0, s, [9, 9], 1234)
    f3 = free_bytes()
    assert f0 == f1 == f2 == f3, (f0, f1, f2, f3)
    assert np.array_equal(a, c) and len(b) == 40
    ctx.close()


def test_invalid_arguments_touch_nothing(gpu):
    cfg, tensors = _model("tiny-int8")
    ref = _ctx(gpu, cfg, tensors)
    ctx = _ctx(gpu, cfg, tensors)
    V = cfg.vocab_size
    prompt = _prompt(V, 12)
    s = Sampling(temperature=1.0, topp=0.9, **CONTROLS)
    got, st = ctx.generate_lookup_ex(prompt, 0, 20, s, rng_state=1234)
    want, s_ref = ref.generate_ex(prompt, 0, 20, s, rng_state=1234)
    assert np.array_equal(got, want) and st == s_ref
    before = _caches(ctx, cfg)
    counts = [ctx.query(k) for k in ("shaped_tokens", "sampled_tokens")]
    good = [2, 3, 4, 5]
    with pytest.raises(gpu.FlmError, match="flm error -1"):
        ctx.verify_sample_ex(1, good, 0, s, list(range(9)), 1)                 # n_window 9 > penalty_last_n 8
    with pytest.raises(gpu.FlmError, match="flm error -1"):
        ctx.verify_sample_ex(1, good, 0, Sampling(temperature=1.0, top_k=5), [3], 1)   # ... and > 0 where penalty_last_n is 0
    for first, drafts, pos, w in ((1, [2, 3, 4], 0, ()), (1, list(range(16)), 0, ()), (1, good, MAX_SEQ - 4, ()), (1, good, -1, ()), (V, good, 0, ()), (1, [2, 3, V, 5], 0, ()),
                                  (1, good, 0, [V]), (1, good, 0, [-1])):
        with pytest.raises(gpu.FlmError, match="flm error -1"):
            ctx.verify_sample_ex(first, drafts, pos, s, w, 1)
    with pytest.raises(gpu.FlmError, match="flm error -1"):
        ctx.verify_sample_ex(1, good, 0, s, (), None)                          # no state at temperature != 0
    nan, inf = float("nan"), float("inf")
    bad = [Sampling(top_k=-1), Sampling(min_p=1.0), Sampling(min_p=-0.5), Sampling(min_p=nan), Sampling(repeat_penalty=0.0), Sampling(repeat_penalty=nan),
           Sampling(frequency_penalty=nan), Sampling(presence_penalty=nan), Sampling(penalty_last_n=-1), Sampling(penalty_last_n=1025), Sampling(bias={V: 1.0}),
           Sampling(bias={-1: 1.0}), Sampling(bias=([3, 3], [1.0, 2.0])), Sampling(bias={3: nan}), Sampling(bias={3: inf}), Sampling(bias=(list(range(257)), [0.0] * 257)),
           Sampling(temperature=-1.0), Sampling(topp=nan)]
    for b in bad:
        if b.temperature == 0.0:
            b.temperature = 1.0
        with pytest.raises(gpu.FlmError, match="flm error -1"):
            ctx.generate_lookup_ex(prompt, 0, 8, b, rng_state=1)
        with pytest.raises(gpu.FlmError, match="flm error -1"):
            ctx.verify_sample_ex(1, good, 0, b, (), 1)
    for kw in (dict(max_tokens=0), dict(max_tokens=MAX_SEQ - len(prompt) + 2), dict(draft_len=3), dict(draft_len=16), dict(ngram_max=0), dict(ngram_max=9), dict(stop_token=V)):
        args = dict(max_tokens=8, draft_len=7, ngram_max=3, stop_token=-1); args.update(kw)
        with pytest.raises(gpu.FlmError, match="flm error -1"):
            ctx.generate_lookup_ex(prompt, 0, args["max_tokens"], s, rng_state=1, stop_token=args["stop_token"], draft_len=args["draft_len"], ngram_max=args["ngram_max"])
    wrong = prompt.copy(); wrong[4] = V
    with pytest.raises(gpu.FlmError, match="flm error -1"):
        ctx.generate_lookup_ex(wrong, 0, 8, s, rng_state=1)
    lib = gpu.lib()
    n_out = ctypes.c_int(0); st1 = ctypes.c_uint64(1)
    sp, keep = s.struct()
    pp = prompt.ctypes.data_as(ctypes.c_void_p)
    assert lib.flm_generate_lookup_ex(ctx._h, pp, len(prompt), 0, 8, None, ctypes.byref(st1), ctypes.c_int32(-1), 7, 3, None, None, None, ctypes.byref(n_out)) == -1
    assert lib.flm_generate_lookup_ex(ctx._h, pp, len(prompt), 0, 8, ctypes.byref(sp), None, ctypes.c_int32(-1), 7, 3, None, None, None, ctypes.byref(n_out)) == -1
    # nothing ran: the counters and the K/V rows stand, and the shaped loop continues bit-equal behind them
    assert [ctx.query(k) for k in ("shaped_tokens", "sampled_tokens")] == counts
    for x, y in zip(_caches(ctx, cfg), before):
        assert np.array_equal(x, y)
    at = len(prompt) + 19
    hist = [int(x) for x in prompt] + [int(x) for x in got]
    c_ids, c_s = _ref_loop(ctx, got[-1], at, 5, s, hist, st)
    r_ids, r_s = _ref_loop(ref, want[-1], at, 5, s, hist, s_ref)
    assert np.array_equal(c_ids, r_ids) and c_s == r_s
    for x, y in zip(_caches(ctx, cfg), _caches(ref, cfg)):
        assert np.array_equal(x[:, :at + 5], y[:, :at + 5])
    tp = gpu.Ctx(gpu.desc_from_config(cfg, max_seq_len=MAX_SEQ), rank=0, world=2)
    with pytest.raises(gpu.FlmError, match="flm error -2"):
        tp.generate_lookup_ex(prompt, 0, 4, Sampling(temperature=0.0, top_k=5))
    with pytest.raises(gpu.FlmError, match="flm error -2"):
        tp.verify_sample_ex(1, good, 0, Sampling(temperature=0.0, top_k=5), (), None)
    tp.close()
    ref.close(); ctx.close()


def test_other_entry_points_undisturbed(gpu):
    """forward, decode_greedy, generate, generate_ex, the unshaped spec calls and score give the same results on a context that ran the new calls as on a fresh one"""
    cfg, tensors = _model("tiny-int8")
    toks = _prompt(cfg.vocab_size, 50)
    s = Sampling(temperature=1.0, topp=0.9, **CONTROLS)

    def run(ctx):
        ctx.reset_kv()
        lg = ctx.forward(toks[:12], 0)
        ids = ctx.decode_greedy(int(np.argmax(lg)), 12, 10)
        ctx.reset_kv()
        gen, _ = ctx.generate(toks[:12], 0, 10)
        ctx.reset_kv()
        gex = ctx.generate_ex(toks[:12], 0, 10, s, rng_state=7)
        ctx.reset_kv()
        look = ctx.generate_lookup_sample(toks[:30], 0, 20, 1.0, 0.9, 7)
        ctx.reset_kv()
        ver = ctx.verify_sample(1, [2, 3, 4, 5, 6], 0, 1.0, 0.9, 7)
        ctx.reset_kv()
        sc = ctx.score(toks[:20], 0)
        return bits(lg).copy(), list(ids), list(gen), list(gex[0]), gex[1], list(look[0]), look[1], list(ver[0]), ver[1], sc.tobytes()
    fresh = _ctx(gpu, cfg, tensors)
    want = run(fresh)
    fresh.close()
    ctx = _ctx(gpu, cfg, tensors)
    for gemm in (1, 0):
        ctx.set_option("spec_gemm", gemm)
        ctx.reset_kv()
        ctx.generate_lookup_ex(toks[:30], MAX_SEQ - 30 - 20 + 1, 20, s, rng_state=3, draft_len=15)      # (ends at max_seq_len: the single-token steps re-write the block)
        ctx.verify_sample_ex(1, [2, 3, 4, 5, 6], 100, s, [4, 4], 9)
        got = run(ctx)
        assert np.array_equal(got[0], want[0]) and got[1:] == want[1:], gemm
    ctx.close()


# ---- bin/main ----------------------------------------------------------------------------------------------------------------------------------------------------
GOLD = os.path.join(os.path.dirname(__file__), "golden")
MAIN = os.path.join(graft.PKG_DIR, "bin", "main")
PROMPT = "Once upon a time there was a small village among the mountains. Once upon a time there was a small village among the mountains."
FLAGS = ("--top-k", "5", "--repeat-penalty", "1.3", "--repeat-last-n", "8")


def _main(*extra):
    r = subprocess.run([MAIN, "-c", os.path.join(GOLD, "hf_tiny_int8.flm"), "-j", "1", "-n", "48", "-i", PROMPT, *extra], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return r


def test_cli_draft_and_lookup_under_the_control_flags_print_the_same_text(gpu):
    if not os.path.exists(MAIN):
        graft.build()
    text = lambda out: out[out.index("output: "):out.index("num_threads:")]
    plain, draft = _main("-t", "0.8", "-p", "0.9", *FLAGS), _main("-t", "0.8", "-p", "0.9", *FLAGS, "--draft", "7,3")
    assert text(draft.stdout) == text(plain.stdout) and len(text(plain.stdout)) > len("output: ")
    m = re.search(r"draft:7,3\taccepted/steps:(?:\x1b\[\d+m)?(\d+)/(\d+)", draft.stdout)
    assert m and int(m.group(2)) >= 1, draft.stdout[-400:]                   # verify passes ran: the flag was not ignored
    assert "draft:" not in plain.stdout and "ignored" not in draft.stderr
    plain0, look0 = _main("-t", "0", *FLAGS), _main("-t", "0", *FLAGS, "--lookup", "7,3")
    assert text(look0.stdout) == text(plain0.stdout)
    m = re.search(r"lookup:7,3\taccepted/steps:(?:\x1b\[\d+m)?(\d+)/(\d+)", look0.stdout)
    assert m and int(m.group(2)) >= 1, look0.stdout[-400:]
    assert text(plain0.stdout) != text(_main("-t", "0").stdout)               # (the flags matter on this model, or equal text shows nothing)
