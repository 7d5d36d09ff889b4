"""Sampled draft-and-verify: k_sample_rows (flm_op_sample_rows), flm_verify_sample, flm_generate_lookup_sample and bin/main --draft.  Everything is equality: ids with
np.array_equal, sampler states as 64-bit integers, K/V rows on bit patterns.

References: the host sampler (sample_util.host_sample) and flm_op_sample called row after row with the state carried along; flm_decode_sample / flm_generate on a SECOND
context (the token path); the loop's steps simulated on the reference ids with the drafter's host restatement.  The models, the looping prompt and the simulation are
those of tests/test_gpu_spec.py; max_seq_len is 256 throughout."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import __graft_entry__ as graft
from fast_llama_amd import flmfile as ff
from sample_util import advance_state, chain_pick, host_lib, host_sample, logits_case, teeth_logits
from test_gpu_spec import MAX_SEQ, MODELS, _caches, _ctx, _looping_prompt, _model, _model_7b, _prompt, _record, _simulate

pytestmark = pytest.mark.gpu

KINDS = ("peaked", "medium", "flat", "ties", "clip", "neginf")
TP = ((1.0, 0.9), (0.7, 0.5), (1.0, 1.0), (0.0, 0.9))
SETTINGS = ((1.0, 0.9, 0), (1.0, 0.9, 1234), (0.3, 0.5, 77), (1.0, 1.0, 5), (0.0, 0.9, 3))


def _after(s0, t, draws):
    return advance_state(s0, draws) if t != 0 else s0


# ---- k_sample_rows -----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 67, 512, 32000])
def test_op_sample_rows_is_the_host_sampler_row_after_row(gpu, n):
    """row i of a batch = the host sampler's i-th draw from the same state, on the logit families of the sampler's grid (ties, values at d = -15, -inf); 1, 5 and 16 rows;
    rows n and n + 5 floats apart (the padding holds NaN: a read past n would poison the sum); the 16 rows differ, so rows that shared a sort slice or a coin would show
    (16 rows of 32000 entries under top-p is the case that sorts 16 x 8 B x 32000 at once)"""
    H = host_lib()
    bad = []
    for kind in KINDS:
        rows = np.stack([logits_case(kind, n, seed=100 + r) for r in range(16)])
        padded = np.full((16, n + 5), np.nan, np.float32); padded[:, :n] = rows
        for t, p in TP:
            for s0 in (0, 1234):
                want, s = [], s0
                for r in range(16):
                    tok, s = host_sample(H, rows[r], t, p, s)
                    want.append(tok)
                assert s == _after(s0, t, 16)
                for nr in (1, 5, 16):
                    for lg in (rows, padded):
                        got, got_s = gpu.op_sample_rows(lg[:nr], n, t, p, s0)
                        if list(got) != want[:nr] or got_s != _after(s0, t, nr):
                            bad.append((kind, t, p, s0, nr, lg.shape[1], list(got), want[:nr], got_s))
    assert not bad, bad[:6]


def test_op_sample_rows_is_op_sample_in_sequence(gpu):
    """against k_sample_advance itself (flm_op_sample, the state carried from call to call), with a row where the summation ORDER decides the token -- asserted with NumPy
    first -- placed in row 3: the row's chain and its coin (the 4th of the state) are the token path's"""
    s0, at = 1234, 3
    s_row = advance_state(s0, at)                                       # the state in front of row 3's draw
    teeth = None
    for trial in range(200):
        lg = teeth_logits(trial)
        _, seq_tok, tree_tok = chain_pick(lg, 1.0, s_row)
        if seq_tok != tree_tok:
            teeth = (lg, seq_tok)
            break
    assert teeth is not None, "no case where the summation order changes the token"
    n = teeth[0].size
    rows = np.stack([teeth[0] if r == at else logits_case("medium", n, seed=r) for r in range(6)])
    want, s = [], s0
    for r in range(6):
        tok, s = gpu.op_sample(rows[r], 1.0, 1.0, s)
        want.append(tok)
    assert want[at] == teeth[1]
    got, got_s = gpu.op_sample_rows(rows, n, 1.0, 1.0, s0)
    assert list(got) == want and got_s == s == advance_state(s0, 6)
    for t, p in ((1.0, 0.9), (0.7, 0.5)):
        want, s = [], s0
        for r in range(6):
            tok, s = gpu.op_sample(rows[r], t, p, s)
            want.append(tok)
        got, got_s = gpu.op_sample_rows(rows, n, t, p, s0)
        assert list(got) == want and got_s == s, (t, p)


# ---- flm_verify_sample -------------------------------------------------------------------------------------------------------------------------------------------
def _verify_cases(gpu, cfg, tensors, gemms, positions, ks, t=1.0, p=0.9, s0=1234):
    ref = _ctx(gpu, cfg, tensors)
    ctx = _ctx(gpu, cfg, tensors)
    V = cfg.vocab_size
    prompt = _prompt(V, 37)
    for pos in positions:
        def start(c):
            c.reset_kv()
            return c.forward_argmax(prompt, 0) if pos == 37 else 1
        first = start(ref)
        n_ref = 20
        ids, s_ref = ref.decode_sample(first, pos, n_ref, t, p, s0)          # the token path's ids, state and K/V rows
        assert s_ref == _after(s0, t, n_ref)
        kv_ref = _caches(ref, cfg)
        for k in ks:
            for wrong in (None, 0, 2, k - 1):
                drafts = ids[:k].copy()
                if wrong is not None:
                    drafts[wrong] = (drafts[wrong] + 1) % V
                m = k if wrong is None else wrong
                for gemm in gemms:
                    ctx.set_option("spec_gemm", gemm)
                    assert start(ctx) == first
                    got, s = ctx.verify_sample(first, drafts, pos, t, p, s0)
                    assert len(got) == m + 1 and np.array_equal(got, ids[:m + 1]), (pos, k, wrong, gemm, list(got), list(ids[:m + 1]))
                    assert s == _after(s0, t, m + 1), (pos, k, wrong, gemm)
                    for a, b in zip(_caches(ctx, cfg), kv_ref):
                        assert np.array_equal(a[:, :pos + m + 1], b[:, :pos + m + 1]), (pos, k, wrong, gemm)
                    # the sampled decode loop continues from the returned position and state
                    tail = min(3, n_ref - (m + 1))
                    if tail > 0:
                        cont, s_cont = ctx.decode_sample(int(got[-1]), pos + m + 1, tail, t, p, s)
                        assert np.array_equal(cont, ids[m + 1:m + 1 + tail]) and s_cont == _after(s0, t, m + 1 + tail), (pos, k, wrong, gemm)
    assert ctx.query("fallback") == 0
    ref.close(); ctx.close()


@pytest.mark.parametrize("name", list(MODELS))
def test_verify_sample_is_the_sampled_decode_loop(gpu, name):
    """drafts = flm_decode_sample's ids (a second context) with none / the first / draft 2 / draft k - 1 made wrong, which fixes m: n_out, the ids, the state after n_out
    draws, the K/V rows pos .. pos + m of every layer, and the loop's continuation; k = 4 and 15; pos = 0 and 37 (behind a batched prompt); "spec_gemm" 1 and 0 on int8"""
    cfg, tensors = _model(name)
    gemms = (1, 0) if MODELS[name][1] == ff.QT_INT8 else (0,)
    _verify_cases(gpu, cfg, tensors, gemms, (0, 37), (4, 15))


def test_verify_sample_other_parameters_and_temperature_zero(gpu):
    cfg, tensors = _model("tiny-int8")
    _verify_cases(gpu, cfg, tensors, (0,), (0,), (4,), t=0.7, p=0.5, s0=77)
    _verify_cases(gpu, cfg, tensors, (0,), (37,), (15,), t=1.0, p=1.0, s0=5)
    _verify_cases(gpu, cfg, tensors, (0,), (0,), (4,), t=1.0, p=0.9, s0=0)
    # temperature 0: flm_verify_greedy's result, the state untouched, a NULL state allowed
    ctx = _ctx(gpu, cfg, tensors)
    ids = ctx.decode_greedy(1, 0, 8)
    for drafts in (ids[:7], np.concatenate([ids[:3], [(ids[3] + 1) % cfg.vocab_size], ids[4:7]]).astype(np.int32)):
        ctx.reset_kv()
        want = ctx.verify_greedy(1, drafts, 0)
        ctx.reset_kv()
        got, s = ctx.verify_sample(1, drafts, 0, 0.0, 0.9, 99)
        assert np.array_equal(got, want) and s == 99
        ctx.reset_kv()
        got, s = ctx.verify_sample(1, drafts, 0, 0.0, 0.9, None)
        assert np.array_equal(got, want) and s is None
    # ... and flm_generate_lookup_sample is flm_generate_lookup: ids, step counters and callbacks; the state untouched, no token counted as sampled
    prompt, _ = _looping_prompt(gpu)
    sampled_before = ctx.query("sampled_tokens")
    for K in (4, 15):
        a_seen, a_cb = _record(); b_seen, b_cb = _record()
        ctx.reset_kv()
        want = ctx.generate_lookup(prompt, 0, 60, draft_len=K, on_token=a_cb)
        want_steps = (ctx.query("spec_steps"), ctx.query("spec_accepted"))
        ctx.reset_kv()
        got, s = ctx.generate_lookup_sample(prompt, 0, 60, 0.0, 0.9, 3, draft_len=K, on_token=b_cb)
        assert np.array_equal(got, want) and len(got) == 60 and s == 3, K
        assert (ctx.query("spec_steps"), ctx.query("spec_accepted")) == want_steps and want_steps[1] > 0, K
        assert a_seen == b_seen and len(b_seen) == 60, K
    assert ctx.query("sampled_tokens") == sampled_before
    ctx.close()


def test_verify_sample_at_7b_width(gpu):
    """the 2-layer 7B-width model: the real workgroup counts and a 32000-entry vocabulary (16 rows sorting at once)"""
    cfg, tensors = _model_7b()
    _verify_cases(gpu, cfg, tensors, (1, 0), (0,), (15,))


# ---- flm_generate_lookup_sample ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [4, 15])
@pytest.mark.parametrize("t,p,s0", SETTINGS)
def test_generate_lookup_sample_is_generate(gpu, K, t, p, s0):
    """ids, n_out, the callback sequence with `last`, the final state and the K/V rows against flm_generate on a second context; the queried step counters against the loop
    simulated on the reference ids.  State 0 keeps every coin at 0, the draw is then the lowest index among the maximal probabilities, and the looping prompt's continuation
    repeats: the simulated loop accepts drafts there, which is asserted on the SIMULATED value"""
    cfg, tensors = _model("tiny-int8")
    prompt, _ = _looping_prompt(gpu)
    ref = _ctx(gpu, cfg, tensors)
    ctx = _ctx(gpu, cfg, tensors)
    G, N = 3, 60
    a_seen, a_cb = _record(); b_seen, b_cb = _record()
    want, s_want = ref.generate(prompt, 0, N, t, p, s0, on_token=a_cb)
    got, s_got = ctx.generate_lookup_sample(prompt, 0, N, t, p, s0, draft_len=K, ngram_max=G, on_token=b_cb)
    assert len(want) == N and s_want == _after(s0, t, N)
    assert np.array_equal(got, want) and s_got == s_want
    assert a_seen == b_seen and len(b_seen) == N and b_seen[-1][2]
    steps, accepted, _ = _simulate(gpu, prompt, want, K, G)
    print("sampled lookup", (t, p, s0), "K", K, "steps", ctx.query("spec_steps"), "accepted", ctx.query("spec_accepted"), "simulated", (steps, accepted))
    assert (ctx.query("spec_steps"), ctx.query("spec_accepted")) == (steps, accepted)
    if (t, p, s0) == (1.0, 0.9, 0):
        assert accepted >= 1 and steps < N - 1
    for x, y in zip(_caches(ctx, cfg), _caches(ref, cfg)):
        assert np.array_equal(x[:, :len(prompt) + N - 1], y[:, :len(prompt) + N - 1])
    # the sampled decode loop continues from the returned position and state
    at = len(prompt) + N - 1
    c_ids, c_s = ctx.decode_sample(int(got[-1]), at, 4, t, p, s_got)
    r_ids, r_s = ref.decode_sample(int(want[-1]), at, 4, t, p, s_want)
    assert np.array_equal(c_ids, r_ids) and c_s == r_s == _after(s0, t, N + 4)
    assert ctx.query("fallback") == 0
    ref.close(); ctx.close()


@pytest.mark.parametrize("K", [4, 15])
@pytest.mark.parametrize("t,p,s0", [(1.0, 0.9, 0), (1.0, 0.9, 1234)])
def test_generate_lookup_sample_stop_cut_tail_and_cancel(gpu, K, t, p, s0):
    cfg, tensors = _model("tiny-int8")
    prompt, _ = _looping_prompt(gpu)
    ref = _ctx(gpu, cfg, tensors)
    ctx = _ctx(gpu, cfg, tensors)
    G, N = 3, 60
    want, _ = ref.generate(prompt, 0, N, t, p, s0)
    _, _, runs = _simulate(gpu, prompt, want, K, G)
    # a stop token hit mid-run: inside an accepted run where the loop has one, else at the first id not seen before index 5
    inside = [s + j for s, n in runs for j in range(1, n) if want[s + j] not in want[:s + j]]
    later = [i for i in range(5, N) if want[i] not in want[:i]]
    if s0 == 0:
        assert inside, "the test's precondition: an id first seen inside an accepted run"
    cut = inside[0] if inside else later[0]
    stop = int(want[cut])
    a_seen, a_cb = _record(); b_seen, b_cb = _record()
    ref.reset_kv(); ctx.reset_kv()
    want_s, sa = ref.generate(prompt, 0, N, t, p, s0, stop_token=stop, on_token=a_cb)
    got_s, sb = ctx.generate_lookup_sample(prompt, 0, N, t, p, s0, stop_token=stop, draft_len=K, ngram_max=G, on_token=b_cb)
    assert len(want_s) == cut + 1 and want_s[-1] == stop
    assert np.array_equal(got_s, want_s) and a_seen == b_seen and b_seen[-1] == (cut, stop, True)
    assert sa == sb == _after(s0, t, cut + 1)                              # the draws behind the cut are not counted
    assert (ctx.query("spec_steps"), ctx.query("spec_accepted")) == _simulate(gpu, prompt, want, K, G, stop=stop)[:2]
    # max_tokens cutting a run (1: no step at all; 2: one id behind the prompt's, a single-token step; 7: inside what K = 15 would accept)
    for n in (1, 2, 7):
        ref.reset_kv(); ctx.reset_kv()
        a_seen, a_cb = _record(); b_seen, b_cb = _record()
        w, sa = ref.generate(prompt, 0, n, t, p, s0, on_token=a_cb)
        g, sb = ctx.generate_lookup_sample(prompt, 0, n, t, p, s0, draft_len=K, ngram_max=G, on_token=b_cb)
        assert np.array_equal(g, w) and len(g) == n and a_seen == b_seen and sa == sb == _after(s0, t, n), n
        assert (ctx.query("spec_steps"), ctx.query("spec_accepted")) == _simulate(gpu, prompt, want[:n], K, G)[:2], n
    # a call whose tail reaches max_seq_len: the last steps are single sampled tokens
    pos = MAX_SEQ - len(prompt) - 30 + 1
    a_seen, a_cb = _record(); b_seen, b_cb = _record()
    ref.reset_kv(); ctx.reset_kv()
    want_e, sa = ref.generate(prompt, pos, 30, t, p, s0, on_token=a_cb)
    got_e, sb = ctx.generate_lookup_sample(prompt, pos, 30, t, p, s0, draft_len=K, ngram_max=G, on_token=b_cb)
    assert len(want_e) == 30 and np.array_equal(got_e, want_e) and a_seen == b_seen and sa == sb == _after(s0, t, 30)
    assert ctx.query("spec_steps") < 29                       # (at least the last K positions were single tokens)
    # a callback that cancels at index 5: the same sequence up to there, nothing behind it; *n_out covers what was delivered and the state counts *n_out draws
    def cancelling(seen):
        return lambda i, tok, last: seen.append((i, tok, last)) or i == 5
    a_seen, b_seen = [], []
    ref.reset_kv(); ctx.reset_kv()
    want_c, sa = ref.generate(prompt, 0, N, t, p, s0, on_token=cancelling(a_seen))
    got_c, sb = ctx.generate_lookup_sample(prompt, 0, N, t, p, s0, draft_len=K, ngram_max=G, on_token=cancelling(b_seen))
    assert a_seen == b_seen and len(b_seen) == 6
    assert 6 <= len(got_c) <= N and np.array_equal(got_c, want[:len(got_c)]) and np.array_equal(want_c, want[:len(want_c)])
    assert sb == _after(s0, t, len(got_c))
    c_ids, _ = ctx.decode_sample(int(got_c[-1]), len(prompt) + len(got_c) - 1, 3, t, p, sb)
    assert np.array_equal(c_ids, want[len(got_c):len(got_c) + 3])
    assert ctx.query("fallback") == 0
    ref.close(); ctx.close()


@pytest.mark.parametrize("name,gemm", [("tiny-int16", 0), ("tiny128-int8", 1), ("small-int8", 1), ("small-int8", 0)])
def test_generate_lookup_sample_other_models(gpu, name, gemm):
    cfg, tensors = _model(name)
    ref = _ctx(gpu, cfg, tensors)
    ctx = _ctx(gpu, cfg, tensors)
    ctx.set_option("spec_gemm", gemm)
    block = _prompt(cfg.vocab_size, 9, seed=6)
    prompt = np.concatenate([block, block, block]).astype(np.int32)
    for t, p, s0 in ((1.0, 0.9, 0), (1.0, 0.9, 1234)):
        ref.reset_kv(); ctx.reset_kv()
        a_seen, a_cb = _record(); b_seen, b_cb = _record()
        want, sa = ref.generate(prompt, 0, 50, t, p, s0, on_token=a_cb)
        got, sb = ctx.generate_lookup_sample(prompt, 0, 50, t, p, s0, draft_len=7, ngram_max=4, on_token=b_cb)
        assert np.array_equal(got, want) and a_seen == b_seen and sa == sb == _after(s0, t, 50)
        assert (ctx.query("spec_steps"), ctx.query("spec_accepted")) == _simulate(gpu, prompt, want, 7, 4)[:2]
    ref.close(); ctx.close()


# ---- the contract around the calls -------------------------------------------------------------------------------------------------------------------------------
def test_a_retried_sampled_lookup_call_draws_once_per_token(gpu):
    """after a timed-out cross-workgroup wait (injected: "inject_wait_failure") the step re-runs from the state the host held at its start: the same ids and state as an
    undisturbed call, every index delivered once.  The call ends at max_seq_len, so it includes single-token steps."""
    cfg, tensors = _model("tiny-int8")
    prompt, _ = _looping_prompt(gpu)
    pos, N = MAX_SEQ - len(prompt) - 12 + 1, 12
    for t, p, s0 in ((1.0, 0.9, 1234), (1.0, 0.9, 0), (0.0, 0.9, 3)):
        ref = _ctx(gpu, cfg, tensors)
        ctx = _ctx(gpu, cfg, tensors)
        a_seen, a_cb = _record(); b_seen, b_cb = _record()
        want, sa = ref.generate_lookup_sample(prompt, pos, N, t, p, s0, draft_len=7, on_token=a_cb)
        assert np.array_equal(want, ref.generate(prompt, pos, N, t, p, s0)[0])
        assert ref.query("spec_steps") < N - 1
        ctx.set_option("inject_wait_failure", 1)
        got, sb = ctx.generate_lookup_sample(prompt, pos, N, t, p, s0, draft_len=7, on_token=b_cb)
        assert np.array_equal(got, want) and sb == sa == _after(s0, t, N)
        assert b_seen == a_seen and [i for i, _, _ in b_seen] == list(range(N))
        assert ctx.query("fallback") == 1 and ref.query("fallback") == 0
        ref.close(); ctx.close()


def test_nothing_is_allocated_inside_the_sampled_calls(gpu):
    """the first flm_verify_sample and flm_generate_lookup_sample of a fresh context (batch steps and, at the end, a single-token step), bracketed with hipMemGetInfo"""
    hip = ctypes.CDLL("libamdhip64.so")

    def free_bytes():
        f, t = ctypes.c_size_t(0), ctypes.c_size_t(0)
        assert hip.hipMemGetInfo(ctypes.byref(f), ctypes.byref(t)) == 0
        return f.value
    cfg, tensors = _model("tiny-int8")
    prompt, _ = _looping_prompt(gpu)
    ctx = _ctx(gpu, cfg, tensors)
    gpu.spec_draft_host([1, 2], 4, 1)                  # (the host library is loaded before the bracket)
    f0 = free_bytes()
    a, _ = ctx.verify_sample(1, [2, 3, 4, 5, 6, 7, 8], 0, 1.0, 0.9, 1234)
    f1 = free_bytes()
    b, _ = ctx.generate_lookup_sample(prompt, 0, 40, 1.0, 0.9, 1234, draft_len=7)
    f2 = free_bytes()
    ctx.generate_lookup_sample(prompt, 0, 40, 0.3, 0.5, 0, draft_len=15)
    ctx.set_option("spec_gemm", 1 - ctx.query("spec_gemm"))
    c, _ = ctx.verify_sample(1, [2, 3, 4, 5, 6, 7, 8], 0, 1.0, 0.9, 1234)
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
    t, p, s0 = 1.0, 0.9, 1234
    got, s = ctx.generate_lookup_sample(prompt, 0, 20, t, p, s0)
    want, s_ref = ref.generate(prompt, 0, 20, t, p, s0)
    assert np.array_equal(got, want) and s == s_ref
    before = _caches(ctx, cfg)
    good = [2, 3, 4, 5]
    for first, drafts, pos in ((1, [2, 3, 4], 0), (1, list(range(16)), 0), (1, good, MAX_SEQ - 4), (1, good, -1), (V, good, 0), (-1, good, 0), (1, [2, 3, V, 5], 0), (1, [2, -1, 4, 5], 0)):
        with pytest.raises(gpu.FlmError, match="flm error -1"):
            ctx.verify_sample(first, drafts, pos, t, p, s0)
    for tt, pp, st in ((1.0, 0.9, None), (-1.0, 0.9, 5), (float("nan"), 0.9, 5), (1.0, float("nan"), 5)):
        with pytest.raises(gpu.FlmError, match="flm error -1"):
            ctx.verify_sample(1, good, 0, tt, pp, st)
    for kw in (dict(max_tokens=0), dict(max_tokens=MAX_SEQ - len(prompt) + 2), dict(draft_len=3), dict(draft_len=16), dict(ngram_max=0), dict(ngram_max=9), dict(stop_token=V),
               dict(temperature=-0.5)):
        args = dict(max_tokens=8, draft_len=7, ngram_max=3, stop_token=-1, temperature=t); args.update(kw)
        with pytest.raises(gpu.FlmError, match="flm error -1"):
            ctx.generate_lookup_sample(prompt, 0, args["max_tokens"], args["temperature"], p, s0, stop_token=args["stop_token"], draft_len=args["draft_len"], ngram_max=args["ngram_max"])
    bad = prompt.copy(); bad[4] = V
    with pytest.raises(gpu.FlmError, match="flm error -1"):
        ctx.generate_lookup_sample(bad, 0, 8, t, p, s0)
    n_out = ctypes.c_int(0)                                                     # a NULL state at temperature > 0 (the binding always passes one)
    assert gpu.lib().flm_generate_lookup_sample(ctx._h, prompt.ctypes.data_as(ctypes.c_void_p), len(prompt), 0, 8, ctypes.c_float(1.0), ctypes.c_float(0.9), None,
                                                ctypes.c_int32(-1), 7, 3, None, None, None, ctypes.byref(n_out)) == -1
    for x, y in zip(_caches(ctx, cfg), before):
        assert np.array_equal(x, y)
    # ... and the sampled decode loop continues bit-equal behind them
    at = len(prompt) + 19
    c_ids, c_s = ctx.decode_sample(int(got[-1]), at, 5, t, p, s)
    r_ids, r_s = ref.decode_sample(int(want[-1]), at, 5, t, p, s_ref)
    assert np.array_equal(c_ids, r_ids) and c_s == r_s
    for x, y in zip(_caches(ctx, cfg), _caches(ref, cfg)):
        assert np.array_equal(x[:, :at + 5], y[:, :at + 5])
    fresh = gpu.Ctx(gpu.desc_from_config(cfg, max_seq_len=MAX_SEQ))
    with pytest.raises(gpu.FlmError, match="flm error -5"):
        fresh.verify_sample(1, good, 0, t, p, s0)                              # the model is not complete
    with pytest.raises(gpu.FlmError, match="flm error -5"):
        fresh.generate_lookup_sample(prompt, 0, 8, t, p, s0)
    fresh.close()
    ref.close(); ctx.close()


# ---- bin/main --draft --------------------------------------------------------------------------------------------------------------------------------------------
GOLD = os.path.join(os.path.dirname(__file__), "golden")
MAIN = os.path.join(graft.PKG_DIR, "bin", "main")
PROMPT = "Once upon a time there was a small village among the mountains. Once upon a time there was a small village among the mountains."


def _main(*extra):
    r = subprocess.run([MAIN, "-c", os.path.join(GOLD, "hf_tiny_int8.flm"), "-j", "1", "-n", "48", "-i", PROMPT, *extra], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return r


def test_cli_draft_prints_the_same_text(gpu):
    if not os.path.exists(MAIN):
        graft.build()
    text = lambda out: out[out.index("output: "):out.index("num_threads:")]
    size = lambda out: re.search(r"output_size:\s*(\d+)", out).group(1)
    plain, draft = _main("-t", "0.8", "-p", "0.9"), _main("-t", "0.8", "-p", "0.9", "--draft", "7")
    assert text(draft.stdout) == text(plain.stdout) and len(text(plain.stdout)) > len("output: ")
    m = re.search(r"draft:7,3\taccepted/steps:(?:\x1b\[\d+m)?(\d+)/(\d+)", draft.stdout)
    assert m and int(m.group(2)) >= 1, draft.stdout[-400:]
    assert "draft:" not in plain.stdout and size(draft.stdout) == size(plain.stdout)
    # at temperature 0 the flag is --lookup's path
    look, draft0 = _main("-t", "0", "--lookup", "7"), _main("-t", "0", "--draft", "7,2")
    assert text(draft0.stdout) == text(look.stdout) and re.search(r"draft:7,2\taccepted/steps:", draft0.stdout) and "lookup:" not in draft0.stdout
