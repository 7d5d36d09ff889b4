"""Greedy draft-and-verify: flm_verify_greedy, flm_generate_lookup, the skinny int8 GEMM of the verify pass and the drafter kernel.  Everything is equality: ids with
np.array_equal, K/V rows and GEMM outputs on bit patterns.

References: flm_decode_greedy / flm_generate on a SECOND context (the token path), the CPU oracle's matmul, the drafter's host restatement (capi.spec_draft_host).  The
drafter kernel is reached through the op-level entry flm_op_spec_draft (capi.op_spec_draft), on the histories of tests/test_spec_host.py.  max_seq_len is 256 throughout."""
import ctypes
import os

import numpy as np
import pytest

import oracle_py as O
from fast_llama_amd import flmfile as ff, synth
from test_spec_host import histories

pytestmark = pytest.mark.gpu
MAX_SEQ = 256
MODELS = {
    "tiny-int8": ("tiny", ff.QT_INT8, 5),
    "tiny-int16": ("tiny", ff.QT_INT16, 5),
    "tiny128-int8": ("tiny128", ff.QT_INT8, 5),
    "small-int8": ("small", ff.QT_INT8, 7),
}
_made = {}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _model(name):
    if name not in _made:
        shape, qt, seed = MODELS[name]
        cfg = synth.make_config(shape, qt)
        _made[name] = (cfg, synth.make_tensors(cfg, seed=seed))
    return _made[name]


def _model_7b():
    if "7B" not in _made:
        cfg = synth.make_config("7B", ff.QT_INT8); cfg.n_layers = 2
        _made["7B"] = (cfg, synth.make_tensors(cfg, seed=53))
    return _made["7B"]


def _ctx(gpu, cfg, tensors):
    ctx = gpu.Ctx(gpu.desc_from_config(cfg, max_seq_len=MAX_SEQ)); ctx.upload_all(tensors)
    return ctx


def _caches(ctx, cfg):
    """[layer][k / v] -> uint32 [heads][MAX_SEQ][hs]"""
    hs = cfg.dim // cfg.n_heads
    n = cfg.n_heads * MAX_SEQ * hs
    return [ctx.debug_read(w, l, n).view(np.uint32).reshape(cfg.n_heads, MAX_SEQ, hs) for l in range(cfg.n_layers) for w in ("kcache", "vcache")]


def _prompt(V, n, seed=3):
    rng = np.random.default_rng(seed)
    return np.concatenate([[1], rng.integers(0, V, n - 1)]).astype(np.int32)


# ---- the skinny GEMM ---------------------------------------------------------------------------------------------------------------------------------------------
def _gemm_case(m, n, w, seed):
    rng = np.random.default_rng(seed)
    W = rng.integers(-127, 128, (m, n)).astype(np.int8)
    sW = (rng.random((m, n // 64)).astype(np.float32) * np.float32(0.02) + np.float32(1e-4)) * rng.choice(np.array([1, -1], np.float32), (m, n // 64))
    x = (rng.standard_normal((w, n)) * 3).astype(np.float32)
    q, s = O.quantize(x.reshape(-1), ff.QT_INT8)
    return W, sW.astype(np.float32), q.reshape(w, n), s.reshape(w, n // 64)


@pytest.mark.parametrize("nb", [0, 2], ids=["by-size", "two-fragments"])
@pytest.mark.parametrize("n", [64, 128, 704])
@pytest.mark.parametrize("m", [16, 48, 272])
def test_skinny_gemm_is_the_oracles_matmul(gpu, m, n, nb, monkeypatch):
    """w = 1, 2, 5, 15, 16 token rows; m = one fragment / not a multiple of a workgroup's rows / several workgroups; n = one group / one 128-byte stage / 11 groups.
    Bits equal to the CPU oracle; at w = 16 also to flm_op_matmul_q (the tile kernel).  Idle token columns and rows past the matrix store nothing (the op presets
    the output to NaN patterns and returns exactly [w][m])."""
    if nb:
        monkeypatch.setenv("FLM_OP_SKINNY_NB", str(nb))
    for w in (1, 2, 5, 15, 16):
        W, sW, X, sX = _gemm_case(m, n, w, seed=1000 * m + 10 * n + w)
        want = O.matmul_q(ff.QT_INT8, W, sW, X, sX)
        got = gpu.op_matmul_skinny(W, sW, X, sX)
        assert np.array_equal(bits(got), bits(want)), (m, n, w, np.argwhere(bits(got) != bits(want))[:4])
        if w == 16:
            tiles = gpu.op_matmul_q(ff.QT_INT8, W, sW, X, sX)
            assert np.array_equal(bits(got), bits(tiles)), (m, n)


def test_skinny_gemm_rejects_what_it_does_not_do(gpu):
    W, sW, X, sX = _gemm_case(16, 64, 16, seed=1)
    lib = gpu.lib()
    out = np.empty((17, 16), np.float32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    X17 = np.zeros((17, 64), np.int8); s17 = np.zeros((17, 1), np.float32)
    assert lib.flm_op_matmul_skinny(ff.QT_INT8, p(out), p(W), p(sW), p(X17), p(s17), 16, 64, 17, 64) == -1       # more than 16 rows
    assert lib.flm_op_matmul_skinny(ff.QT_INT16, p(out), p(W), p(sW), p(X), p(sX), 16, 64, 16, 64) == -2        # int16: the tiles


# ---- the drafter kernel ------------------------------------------------------------------------------------------------------------------------------------------
def test_drafter_kernel_is_the_host_drafter(gpu):
    """flm_op_spec_draft (k_spec_draft) == capi.spec_draft_host on every history of the host test; and on a long one (several strides of the kernel's 1024 threads)"""
    for h, g, k in histories():
        got, want = gpu.op_spec_draft(h, k, g), gpu.spec_draft_host(h, k, g)
        assert np.array_equal(got, want), (list(h), g, k, list(got), list(want))
    rng = np.random.default_rng(9)
    h = rng.integers(0, 3, 5000).astype(np.int32)
    for g in (1, 5, 8):
        assert np.array_equal(gpu.op_spec_draft(h, 15, g), gpu.spec_draft_host(h, 15, g)), g
    h = np.arange(3000, dtype=np.int32)                      # no match anywhere
    assert list(gpu.op_spec_draft(h, 4, 8)) == [2999] * 4


# ---- flm_verify_greedy -------------------------------------------------------------------------------------------------------------------------------------------
def _verify_cases(gpu, cfg, tensors, gemms, positions, ks):
    ref = _ctx(gpu, cfg, tensors)
    ctx = _ctx(gpu, cfg, tensors)
    V = cfg.vocab_size
    prompt = _prompt(V, 37)
    for pos in positions:
        def start(c):
            c.reset_kv()
            return c.forward_argmax(prompt, 0) if pos == 37 else 1
        first = start(ref)
        n_ref = min(20, MAX_SEQ - pos)
        ids = ref.decode_greedy(first, pos, n_ref)                     # the token path's ids and K/V rows
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
                    assert ctx.query("spec_gemm") == gemm
                    assert start(ctx) == first
                    got = ctx.verify_greedy(first, drafts, pos)
                    assert np.array_equal(got, ids[:m + 1]), (pos, k, wrong, gemm, list(got), list(ids[:m + 1]))
                    for a, b in zip(_caches(ctx, cfg), kv_ref):
                        assert np.array_equal(a[:, :pos + m + 1], b[:, :pos + m + 1]), (pos, k, wrong, gemm)
                    tail = min(3, n_ref - (m + 1))
                    if tail > 0:
                        cont = ctx.decode_greedy(int(got[-1]), pos + m + 1, tail)
                        assert np.array_equal(cont, ids[m + 1:m + 1 + tail]), (pos, k, wrong, gemm)
    assert ctx.query("fallback") == 0
    ref.close(); ctx.close()


@pytest.mark.parametrize("name", list(MODELS))
def test_verify_greedy_is_the_decode_loop(gpu, name):
    """drafts = the token path's ids (a second context) with none / the first / draft 2 / draft k - 1 made wrong: n_out and the ids, the K/V rows pos .. pos + m of every
    layer bit for bit, and the decode loop's continuation behind them; k = 4 and 15; pos = 0, 37 (behind a prompt) and pos + k + 1 == max_seq_len; "spec_gemm" 0 and 1
    (int16: only the tiles exist, both settings give the same)"""
    cfg, tensors = _model(name)
    _verify_cases(gpu, cfg, tensors, (1, 0), (0, 37, MAX_SEQ - 16, MAX_SEQ - 5), (4, 15))


def test_verify_greedy_at_7b_width(gpu):
    """the 2-layer 7B-width model: the real workgroup counts (Wo / W2: 256 one-fragment workgroups, QKV and the classifier two fragments per wave, [W1; W3] 688)"""
    cfg, tensors = _model_7b()
    _verify_cases(gpu, cfg, tensors, (1, 0), (0,), (15,))


# ---- flm_generate_lookup -----------------------------------------------------------------------------------------------------------------------------------------
def _simulate(gpu, prompt, ids, K, G, stop=-1):
    """the loop's steps on the host, given the ids the model produces: -> (steps, accepted, [(start, length) of every verified run])"""
    hist = list(prompt) + [int(ids[0])]
    total, steps, accepted, runs = 1, 0, 0, []
    at = len(prompt)                                                  # position the last id is fed at (pos = 0)
    while total < len(ids) and ids[total - 1] != stop:
        room = len(ids) - total
        if room >= 2 and at + K + 1 <= MAX_SEQ:
            d = gpu.spec_draft_host(np.array(hist, np.int32), K, G)
            m = 0
            while m < K and total + m < len(ids) and d[m] == ids[total + m]:
                m += 1
            n = min(m + 1, room)
            for i in range(n):
                if ids[total + i] == stop:
                    n = i + 1
                    break
            steps += 1; accepted += n - 1; runs.append((total, n))
        else:
            n = 1
        hist += [int(x) for x in ids[total:total + n]]
        total += n; at += n
    return steps, accepted, runs


def _record():
    seen = []
    return seen, (lambda i, t, last: seen.append((i, t, last)) and False)


_loop = {}


def _looping_prompt(gpu):
    """a prompt whose greedy continuation is known: seed prompt + the first 60 ids of its own continuation c (a second context's flm_generate); what follows is c[60:].
    Once c has run into a cycle the prompt holds repeated blocks of it, and the drafter reads the continuation off them."""
    if not _loop:
        cfg, tensors = _model("tiny-int8")
        ref = _ctx(gpu, cfg, tensors)
        seed = _prompt(cfg.vocab_size, 6, seed=4)
        c, _ = ref.generate(seed, 0, 140)
        ref.close()
        _loop["x"] = (np.concatenate([seed, c[:60]]).astype(np.int32), c[60:])
    return _loop["x"]


@pytest.mark.parametrize("K", [4, 15])
def test_generate_lookup_is_generate(gpu, K):
    cfg, tensors = _model("tiny-int8")
    prompt, cont = _looping_prompt(gpu)
    ref = _ctx(gpu, cfg, tensors)
    ctx = _ctx(gpu, cfg, tensors)
    G = 3
    # no stop token
    N = 60
    a_seen, a_cb = _record(); b_seen, b_cb = _record()
    want, _ = ref.generate(prompt, 0, N, on_token=a_cb)
    got = ctx.generate_lookup(prompt, 0, N, draft_len=K, ngram_max=G, on_token=b_cb)
    assert np.array_equal(want, cont[:N])
    assert np.array_equal(got, want) and a_seen == b_seen and len(b_seen) == N and b_seen[-1][2]
    steps, accepted, runs = _simulate(gpu, prompt, want, K, G)
    print("lookup K", K, "steps", ctx.query("spec_steps"), "accepted", ctx.query("spec_accepted"), "n_out", len(got))
    assert (ctx.query("spec_steps"), ctx.query("spec_accepted")) == (steps, accepted)
    assert ctx.query("spec_accepted") > 0 and ctx.query("spec_steps") < len(got)
    # the K/V rows behind the call are the token path's, and any entry point continues from them
    for x, y in zip(_caches(ctx, cfg), _caches(ref, cfg)):
        assert np.array_equal(x[:, :len(prompt) + N - 1], y[:, :len(prompt) + N - 1])
    assert np.array_equal(ctx.decode_greedy(int(got[-1]), len(prompt) + N - 1, 4), ref.decode_greedy(int(want[-1]), len(prompt) + N - 1, 4))
    # a stop token whose first occurrence lies INSIDE an accepted run
    inside = [s + j for s, n in runs for j in range(1, n) if want[s + j] not in want[:s + j]]
    assert inside, "the test's precondition: an id first seen inside an accepted run"
    stop = int(want[inside[0]])
    a_seen, a_cb = _record(); b_seen, b_cb = _record()
    ref.reset_kv(); ctx.reset_kv()
    want_s, _ = ref.generate(prompt, 0, N, stop_token=stop, on_token=a_cb)
    got_s = ctx.generate_lookup(prompt, 0, N, stop_token=stop, draft_len=K, ngram_max=G, on_token=b_cb)
    assert len(want_s) == inside[0] + 1 and want_s[-1] == stop
    assert np.array_equal(got_s, want_s) and a_seen == b_seen and b_seen[-1] == (inside[0], stop, True)
    assert (ctx.query("spec_steps"), ctx.query("spec_accepted")) == _simulate(gpu, prompt, want[:N], K, G, stop=stop)[:2]
    # a callback that cancels at index 5: the same sequence up to there, nothing behind it; *n_out covers what was delivered
    def cancelling(seen):
        return lambda i, t, last: seen.append((i, t, last)) or i == 5
    a_seen, b_seen = [], []
    ref.reset_kv(); ctx.reset_kv()
    want_c, _ = ref.generate(prompt, 0, N, on_token=cancelling(a_seen))
    got_c = ctx.generate_lookup(prompt, 0, N, draft_len=K, ngram_max=G, on_token=cancelling(b_seen))
    assert a_seen == b_seen and len(b_seen) == 6
    assert 6 <= len(got_c) <= N and np.array_equal(got_c, want[:len(got_c)]) and np.array_equal(want_c, want[:len(want_c)])
    # a call that runs into max_seq_len: the last steps are single tokens
    pos = MAX_SEQ - len(prompt) - 30 + 1
    a_seen, a_cb = _record(); b_seen, b_cb = _record()
    ref.reset_kv(); ctx.reset_kv()
    want_e, _ = ref.generate(prompt, pos, 30, on_token=a_cb)
    got_e = ctx.generate_lookup(prompt, pos, 30, draft_len=K, ngram_max=G, on_token=b_cb)
    assert len(want_e) == 30 and np.array_equal(got_e, want_e) and a_seen == b_seen
    assert ctx.query("spec_steps") < 29                       # (at least the last K positions were single tokens)
    # max_tokens 1 and 2: no batch at all / one id behind the prompt's
    for n in (1, 2):
        ref.reset_kv(); ctx.reset_kv()
        assert np.array_equal(ctx.generate_lookup(prompt, 0, n, draft_len=K), ref.generate(prompt, 0, n)[0])
    assert ctx.query("fallback") == 0
    ref.close(); ctx.close()


@pytest.mark.parametrize("name,gemm", [("tiny-int16", 1), ("small-int8", 1), ("small-int8", 0)])
def test_generate_lookup_other_models(gpu, name, gemm):
    cfg, tensors = _model(name)
    ref = _ctx(gpu, cfg, tensors)
    ctx = _ctx(gpu, cfg, tensors)
    ctx.set_option("spec_gemm", gemm)
    block = _prompt(cfg.vocab_size, 9, seed=6)
    prompt = np.concatenate([block, block, block]).astype(np.int32)
    a_seen, a_cb = _record(); b_seen, b_cb = _record()
    want, _ = ref.generate(prompt, 0, 80, on_token=a_cb)
    got = ctx.generate_lookup(prompt, 0, 80, draft_len=7, ngram_max=4, on_token=b_cb)
    assert np.array_equal(got, want) and a_seen == b_seen
    assert (ctx.query("spec_steps"), ctx.query("spec_accepted")) == _simulate(gpu, prompt, want, 7, 4)[:2]
    ref.close(); ctx.close()


# ---- the contract around the calls -------------------------------------------------------------------------------------------------------------------------------
def test_a_retried_greedy_lookup_call_delivers_once_per_token(gpu):
    """after a timed-out cross-workgroup wait (injected: "inject_wait_failure") the step re-runs from the history and counters the host held at its start: the same ids as
    an undisturbed call and as flm_generate, every index delivered once.  The call ends at max_seq_len, so it includes single-token steps."""
    cfg, tensors = _model("tiny-int8")
    prompt, _ = _looping_prompt(gpu)
    pos, N = MAX_SEQ - len(prompt) - 12 + 1, 12
    ref = _ctx(gpu, cfg, tensors)
    ctx = _ctx(gpu, cfg, tensors)
    a_seen, a_cb = _record(); b_seen, b_cb = _record()
    want = ref.generate_lookup(prompt, pos, N, draft_len=7, on_token=a_cb)
    assert ref.query("spec_steps") < N - 1
    ref.reset_kv()
    assert np.array_equal(want, ref.generate(prompt, pos, N)[0])
    ctx.set_option("inject_wait_failure", 1)
    got = ctx.generate_lookup(prompt, pos, N, draft_len=7, on_token=b_cb)
    assert np.array_equal(got, want) and len(got) == N
    assert b_seen == a_seen and [i for i, _, _ in b_seen] == list(range(N))
    assert ctx.query("fallback") == 1 and ref.query("fallback") == 0
    ref.close(); ctx.close()


def test_nothing_is_allocated_inside_the_new_calls(gpu):
    """the first flm_verify_greedy and flm_generate_lookup of a fresh context, bracketed with hipMemGetInfo: free memory unchanged"""
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
    a = ctx.verify_greedy(1, [2, 3, 4, 5, 6, 7, 8], 0)
    f1 = free_bytes()
    b = ctx.generate_lookup(prompt, 0, 40, draft_len=7)
    f2 = free_bytes()
    ctx.set_option("spec_gemm", 1 - ctx.query("spec_gemm"))        # (the other GEMM form: the option re-captures and allocates nothing)
    c = ctx.verify_greedy(1, [2, 3, 4, 5, 6, 7, 8], 0)
    f3 = free_bytes()
    assert f0 == f1 == f2 == f3, (f0, f1, f2, f3)
    assert np.array_equal(a, c) and len(b) == 40
    ctx.close()


def test_invalid_arguments_touch_nothing(gpu):
    cfg, tensors = _model("tiny-int8")
    ctx = _ctx(gpu, cfg, tensors)
    V = cfg.vocab_size
    prompt = _prompt(V, 12)
    ctx.generate_lookup(prompt, 0, 20)
    before = _caches(ctx, cfg)
    good = [2, 3, 4, 5]
    for first, drafts, pos in ((1, [2, 3, 4], 0), (1, list(range(16)), 0), (1, good, MAX_SEQ - 4), (1, good, -1), (V, good, 0), (-1, good, 0), (1, [2, 3, V, 5], 0), (1, [2, -1, 4, 5], 0)):
        with pytest.raises(gpu.FlmError, match="flm error -1"):
            ctx.verify_greedy(first, drafts, pos)
    for kw in (dict(max_tokens=0), dict(max_tokens=MAX_SEQ - len(prompt) + 2), dict(draft_len=3), dict(draft_len=16), dict(ngram_max=0), dict(ngram_max=9), dict(stop_token=V)):
        args = dict(max_tokens=8, draft_len=7, ngram_max=3, stop_token=-1); args.update(kw)
        with pytest.raises(gpu.FlmError, match="flm error -1"):
            ctx.generate_lookup(prompt, 0, args["max_tokens"], stop_token=args["stop_token"], draft_len=args["draft_len"], ngram_max=args["ngram_max"])
    bad = prompt.copy(); bad[4] = V
    with pytest.raises(gpu.FlmError, match="flm error -1"):
        ctx.generate_lookup(bad, 0, 8)
    for x, y in zip(_caches(ctx, cfg), before):
        assert np.array_equal(x, y)
    fresh = gpu.Ctx(gpu.desc_from_config(cfg, max_seq_len=MAX_SEQ))
    with pytest.raises(gpu.FlmError, match="flm error -5"):
        fresh.verify_greedy(1, good, 0)                                      # the model is not complete
    with pytest.raises(gpu.FlmError, match="flm error -5"):
        fresh.generate_lookup(prompt, 0, 8)
    fresh.close()
    ctx.close()


def test_other_entry_points_undisturbed(gpu):
    """forward, decode_greedy, generate and score give the same logits, ids and rows on a context that ran lookup and verify calls as on a fresh one"""
    cfg, tensors = _model("tiny-int8")
    toks = _prompt(cfg.vocab_size, 50)

    def run(ctx):
        ctx.reset_kv()
        lg = ctx.forward(toks[:12], 0)
        ids = ctx.decode_greedy(int(np.argmax(lg)), 12, 10)
        ctx.reset_kv()
        gen, _ = ctx.generate(toks[:12], 0, 10)
        ctx.reset_kv()
        sc = ctx.score(toks[:20], 0)
        return bits(lg).copy(), list(ids), list(gen), sc.tobytes()
    fresh = _ctx(gpu, cfg, tensors)
    want = run(fresh)
    fresh.close()
    ctx = _ctx(gpu, cfg, tensors)
    for gemm in (1, 0):
        ctx.set_option("spec_gemm", gemm)
        ctx.reset_kv()
        ctx.generate_lookup(toks[:30], 0, 40, draft_len=15)
        ctx.verify_greedy(1, [2, 3, 4, 5, 6], 100)
        got = run(ctx)
        assert np.array_equal(got[0], want[0]) and got[1:] == want[1:], gemm
    ctx.close()
