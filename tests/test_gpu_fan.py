"""Parallel sampling (include/flm_gpu.h: flm_generate_n, flm_fan_keep, flm_op_attention_fan; kernels: csrc/flm_fan.h).  Everything is equality: ids with np.array_equal,
sampler states as 64-bit integers, attention outputs and K/V rows on bit patterns.

Op level: flm_op_attention_fan (k_rope_kv_fan + k_attn_fan) against flm_op_attention on a CONTIGUOUS cache that holds the row's prefix followed by its tail.  Unused
cache rows hold NaN, so a read outside a row's two ranges poisons the result.
Model level: generate_n against n runs of generate on a SECOND context with the same states.  max_seq_len is 256 throughout."""
import ctypes

import numpy as np
import pytest

import oracle_py as O
from fast_llama_amd import capi, flmfile as ff, synth
from test_gpu_spec import MAX_SEQ, MODELS, _caches, _ctx, _model, _prompt, bits

pytestmark = pytest.mark.gpu
HEADS = 2


# ---- op level ------------------------------------------------------------------------------------------------------------------------------------------------------
def _fan_case(rng, hs, S, t, n, q_scale=1.0, max_seq=None):
    """the fan's caches (NaN wherever no row lives), the rows' q / k / v, the layout.  Row j's tail region has t + 1 rows: t fed earlier, one for this step"""
    R = t + 1
    base = [S + j * R for j in range(n)]
    max_seq = max_seq or S + n * R + 3                               # (the layout fits; three rows nobody owns behind it -- or a longer cache: fewer queries per workgroup)
    assert max_seq >= S + n * R
    kc = np.full((HEADS, max_seq, hs), np.nan, np.float32); vc = np.full_like(kc, np.nan)
    kc[:, :S] = rng.standard_normal((HEADS, S, hs)); vc[:, :S] = rng.standard_normal((HEADS, S, hs))
    for j in range(n):
        kc[:, base[j]:base[j] + t] = rng.standard_normal((HEADS, t, hs)); vc[:, base[j]:base[j] + t] = rng.standard_normal((HEADS, t, hs))
    q = (rng.standard_normal((n, HEADS * hs)) * q_scale).astype(np.float32)
    k = rng.standard_normal((n, HEADS * hs)).astype(np.float32); v = rng.standard_normal((n, HEADS * hs)).astype(np.float32)
    return kc, vc, q, k, v, base, max_seq


def _contiguous(kc, vc, S, t, b, max_seq):
    """row j's own cache: the prefix, then its tail, NaN behind"""
    kr = np.full_like(kc, np.nan); vr = np.full_like(vc, np.nan)
    kr[:, :S] = kc[:, :S]; vr[:, :S] = vc[:, :S]
    kr[:, S:S + t] = kc[:, b:b + t]; vr[:, S:S + t] = vc[:, b:b + t]
    return kr, vr


def _check_fan(gpu, hs, S, t, n, case, tag):
    kc, vc, q, k, v, base, max_seq = case
    kc0, vc0 = kc.copy(), vc.copy()
    out = gpu.op_attention_fan(kc, vc, q, k, v, HEADS, hs, max_seq, S, t, base)
    written = np.zeros(max_seq, bool)
    for j in range(n):
        kr, vr = _contiguous(kc0, vc0, S, t, base[j], max_seq)
        want = gpu.op_attention(kr, vr, q[j], k[j], v[j], HEADS, hs, max_seq, S + t)
        assert np.array_equal(bits(out[j]), bits(want)), (tag, hs, S, t, n, j)
        assert np.array_equal(bits(kc[:, base[j] + t]), bits(kr[:, S + t])) and np.array_equal(bits(vc[:, base[j] + t]), bits(vr[:, S + t])), (tag, "the step's K/V row", j)
        written[base[j] + t] = True
    assert np.array_equal(bits(kc[:, ~written]), bits(kc0[:, ~written])) and np.array_equal(bits(vc[:, ~written]), bits(vc0[:, ~written])), (tag, "a row nobody owns was written")


@pytest.mark.parametrize("n", [2, 3, 5, 9, 16])
@pytest.mark.parametrize("hs", [64, 128])
def test_attention_fan_is_the_contiguous_attention(gpu, hs, n):
    """every row against flm_op_attention on its own contiguous cache: prefix lengths around the 64-row tile, tails of 0 / 1 / 63 / 64 / 65 earlier rows (none, one
    partial tile, a tile less one, a whole tile, a tile and a row); n = 2 .. 16: groups of 8 queries that are full, partial, and a single query (n = 9)"""
    rng = np.random.default_rng(1000 * hs + n)
    for S in (1, 63, 64, 65, 130):
        for t in (0, 1, 63, 64, 65):
            _check_fan(gpu, hs, S, t, n, _fan_case(rng, hs, S, t, n), "grid")


@pytest.mark.parametrize("max_seq,n", [(3000, 3), (3000, 9), (6000, 3), (12000, 3)])
def test_attention_fan_with_fewer_queries_per_workgroup(gpu, max_seq, n):
    """head size 128: a context of 3000 rows leaves the LDS room for 4 queries per workgroup, 6000 for 2, 12000 for 1 (fan_group halves the group until a query's score
    rows fit beside the tiles).  n = 3 and 9: a partial group, and two full groups and a single query.  The tails lie at the END of the long cache"""
    hs, S, t = 128, 70, 66
    rng = np.random.default_rng(max_seq + n)
    kc0, vc0, q, k, v, base0, _ = _fan_case(rng, hs, S, t, n)
    kc = np.full((HEADS, max_seq, hs), np.nan, np.float32); vc = np.full_like(kc, np.nan)
    kc[:, :S] = kc0[:, :S]; vc[:, :S] = vc0[:, :S]
    base = [max_seq - (n - j) * (t + 1) for j in range(n)]
    for j in range(n):
        kc[:, base[j]:base[j] + t] = kc0[:, base0[j]:base0[j] + t]; vc[:, base[j]:base[j] + t] = vc0[:, base0[j]:base0[j] + t]
    _check_fan(gpu, hs, S, t, n, (kc, vc, q, k, v, base, max_seq), f"max_seq {max_seq}")


def _weights(kr, q, k, hs, pos):
    """per head: the fp32 scores' softmax weights of one row over its contiguous cache (NumPy; RoPE from the oracle), in float64"""
    ws = []
    for h in range(HEADS):
        qr = O.rope(q[h * hs:(h + 1) * hs], pos); kn = O.rope(k[h * hs:(h + 1) * hs], pos)
        K = np.concatenate([kr[h, :pos], kn[None]]).astype(np.float64)
        sc = (K @ qr.astype(np.float64)) / np.sqrt(hs)
        e = np.exp(sc - sc.max())
        ws.append(e / e.sum())
    return ws


def test_attention_fan_peaked_scores(gpu):
    """a peaked softmax: weights fall under the 1e-15 skip threshold inside BOTH segments (asserted in NumPy first), next to weights that count"""
    hs, S, t, n = 64, 70, 66, 3
    rng = np.random.default_rng(77)
    case = _fan_case(rng, hs, S, t, n, q_scale=30.0)
    kc, vc, q, k, v, base, max_seq = case
    for j in range(n):
        kr, _ = _contiguous(kc, vc, S, t, base[j], max_seq)
        for w in _weights(kr, q[j], k[j], hs, S + t):
            assert (w[1:S] < 1e-17).sum() > 5 and (w[S:] < 1e-17).sum() > 5 and (w > 1e-6).sum() >= 1, "the case is not peaked enough"
    _check_fan(gpu, hs, S, t, n, case, "peaked")


def _chain(x):
    s = np.float32(0)
    for e in x:
        s = np.float32(s + e)
    return s


def test_attention_fan_has_teeth(gpu):
    """the softmax sum is ONE chain over the logical order.  NumPy first shows that on this case summing the prefix and the tail separately and adding the two gives other
    bits than the sequential chain (for every row and head), so a kernel that reduces per segment cannot pass the comparison behind it"""
    hs, S, t, n = 64, 65, 69, 2                                      # (fits max_seq_len 256 with room)
    rng = np.random.default_rng(7)
    case = _fan_case(rng, hs, S, t, n, q_scale=2.0)
    kc, vc, q, k, v, base, max_seq = case
    differ = 0
    for j in range(n):
        kr, _ = _contiguous(kc, vc, S, t, base[j], max_seq)
        for w in _weights(kr, q[j], k[j], hs, S + t):
            e = (w / w.max()).astype(np.float32)                    # the exponentials exp(score - max), up to rounding
            whole, split = _chain(e), np.float32(_chain(e[:S]) + _chain(e[S:]))
            differ += int(whole.view(np.uint32) != split.view(np.uint32))
    assert differ == n * HEADS, f"summing per segment gives the chain's bits on {n * HEADS - differ} of {n * HEADS} rows: pick another case"
    _check_fan(gpu, hs, S, t, n, case, "teeth")


def test_attention_fan_rejects_what_it_does_not_do(gpu):
    rng = np.random.default_rng(3)
    kc, vc, q, k, v, base, max_seq = _fan_case(rng, 64, 8, 2, 2)
    lib = gpu.lib()
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    out = np.empty_like(q); b = np.array(base, np.int32)
    call = lambda hs, ms, n, S, t, bb: lib.flm_op_attention_fan(p(out), p(kc), p(vc), p(q), p(k), p(v), HEADS, hs, ms, n, S, t, p(bb))
    k0 = kc.copy()
    assert call(64, max_seq, 1, 8, 2, b) == -1 and call(64, max_seq, 17, 8, 2, b) == -1          # n outside 2 .. 16
    assert call(256, max_seq, 2, 8, 2, b) == -1                                                   # head sizes above 128
    assert call(64, max_seq, 2, 0, 2, b) == -1 and call(64, 10, 2, 8, 2, b) == -1                 # no shared row; S + t + 1 > max_seq
    assert call(64, max_seq, 2, 8, 2, np.array([8, max_seq - 2], np.int32)) == -1                 # a tail row outside the cache
    assert np.array_equal(bits(kc), bits(k0))


# ---- model level ---------------------------------------------------------------------------------------------------------------------------------------------------
SETTINGS = [(1.0, 0.9), (0.7, 0.5), (1.0, 1.0), (0.0, 0.9)]
_pairs = {}


@pytest.fixture(scope="module")
def pair(gpu):
    """(cfg, the context under test, the reference context) per model, made once"""
    def get(name):
        if name not in _pairs:
            cfg, tensors = _model(name)
            _pairs[name] = (cfg, _ctx(gpu, cfg, tensors), _ctx(gpu, cfg, tensors))
        return _pairs[name]
    yield get
    for _, a, b in _pairs.values():
        a.close(); b.close()
    _pairs.clear()


def _states(n, seed):
    """n sampler states; rows 0 and 1 share one"""
    st = [int(x) for x in np.random.default_rng(seed).integers(1, 2 ** 62, n)]
    st[1] = st[0]
    return st


def _reference(ref, prompt, pos, M, t, p, states, stop=-1):
    """n runs of flm_generate on the reference context, each from the same pos rows -> ids, states after"""
    ids, after = [], []
    for s in states:
        a, sa = ref.generate(prompt, pos, M, temperature=t, topp=p, rng_state=s, stop_token=stop)
        ids.append(a); after.append(sa if t != 0 else s)
    return ids, after


def _fill(ctxs, cfg, pos):
    """pos earlier rows in every context's cache (pos > 0: the call runs behind them)"""
    for c in ctxs:
        c.reset_kv()
        if pos:
            c.forward(_prompt(cfg.vocab_size, pos, seed=11), 0)


@pytest.mark.parametrize("n", [2, 3, 5, 16])
@pytest.mark.parametrize("name", list(MODELS))
def test_generate_n_is_n_generates(pair, name, n):
    """ids, n_out and states of every sequence equal flm_generate's with that state: prompts of 3 tokens (the token-by-token entry) and 40 (the batched entry), at pos 0
    and behind 9 earlier rows, sampled three ways and greedy; rows 0 and 1 are given the same state and produce the same ids; the prompt's rows stay flm_forward's"""
    cfg, ctx, ref = pair(name)
    M = 7
    for n_prompt, pos in ((3, 0), (40, 0), (3, 9), (40, 9)):
        prompt = _prompt(cfg.vocab_size, n_prompt, seed=n_prompt + pos)
        S = pos + n_prompt
        for si, (t, p) in enumerate(SETTINGS):
            if (n_prompt, pos) == (3, 9) and si not in (0, 3):          # (every setting at three of the four entries; two here)
                continue
            _fill((ctx, ref), cfg, pos)
            states = _states(n, 100 * n + si)
            want, after = _reference(ref, prompt, pos, M, t, p, states)
            got, st = ctx.generate_n(prompt, pos, M, states=states, temperature=t, topp=p)
            tag = (name, n, n_prompt, pos, t, p)
            assert len(got) == n and all(np.array_equal(g, w) for g, w in zip(got, want)), (tag, [list(g) for g in got], [list(w) for w in want])
            assert st == after, tag
            assert np.array_equal(got[0], got[1]), tag
            if t != 0:
                assert any(not np.array_equal(got[0], g) for g in got[2:]) or n == 2, (tag, "every state drew the same ids: the case shows nothing")
            for a, b in zip(_caches(ctx, cfg), _caches(ref, cfg)):
                assert np.array_equal(a[:, :S], b[:, :S]), (tag, "the shared rows")
    # temperature 0 with a NULL state array: the greedy run n times, nothing returned for the states
    _fill((ctx, ref), cfg, 0)
    prompt = _prompt(cfg.vocab_size, 12)
    want, _ = ref.generate(prompt, 0, M)
    got, st = ctx.generate_n(prompt, 0, M, n=n)
    assert st is None and all(np.array_equal(g, want) for g in got)


@pytest.mark.parametrize("name", ["tiny-int8", "small-int8"])
def test_generate_n_on_the_skinny_gemm(pair, name):
    """ "spec_gemm" 1: the step's int8 GEMMs run on k_gemm_q8_skinny (the plain-store form in front of k_rope_kv_fan): the same ids and states"""
    cfg, ctx, ref = pair(name)
    M = 7
    ctx.set_option("spec_gemm", 1)
    try:
        for n in (2, 5, 16):
            for n_prompt, pos, (t, p) in ((3, 0, SETTINGS[0]), (40, 9, SETTINGS[1]), (40, 0, SETTINGS[3])):
                prompt = _prompt(cfg.vocab_size, n_prompt, seed=n_prompt + pos)
                _fill((ctx, ref), cfg, pos)
                states = _states(n, 300 * n + pos)
                want, after = _reference(ref, prompt, pos, M, t, p, states)
                got, st = ctx.generate_n(prompt, pos, M, states=states, temperature=t, topp=p)
                assert all(np.array_equal(g, w) for g, w in zip(got, want)) and st == after, (name, n, n_prompt, pos, t, p)
        assert ctx.query("spec_gemm") == 1
    finally:
        ctx.set_option("spec_gemm", 0)


def _stop_case(ref, cfg, prompt, M, n, t, p):
    """a stop token and states under which, ON THE REFERENCE's ids, at least two rows end at different lengths, one of them early, and at least one runs to max_tokens"""
    tried = 0
    for seed in range(5):
        states = _states(n, 900 + seed)
        free, _ = _reference(ref, prompt, 0, M, t, p, states)
        cands = [int(x) for x in np.unique(np.concatenate([f[1:M - 1] for f in free]))]
        for stop in cands[:4]:
            tried += 1
            want, after = _reference(ref, prompt, 0, M, t, p, states, stop)
            lens = [len(w) for w in want]
            if len(set(lens)) >= 2 and max(lens) == M and all(w[-1] == stop for w in want if len(w) < M) and all(stop not in w[:-1] for w in want):
                return stop, states, want, after
            if tried == 20:
                break
    pytest.fail("none of 20 candidate (stop token, seed) pairs ends two rows at different lengths with one running to max_tokens")


@pytest.mark.parametrize("name", ["tiny-int8", "small-int8"])
def test_stop_token_ends_rows_one_by_one(pair, name):
    """the stop token is delivered, counted and not fed; a finished row's state stays behind its last draw while the others go on"""
    cfg, ctx, ref = pair(name)
    n, M, t, p = 5, 12, 1.0, 0.9
    prompt = _prompt(cfg.vocab_size, 9, seed=21)
    _fill((ctx, ref), cfg, 0)
    stop, states, want, after = _stop_case(ref, cfg, prompt, M, n, t, p)
    lens = [len(w) for w in want]
    assert len(set(lens)) >= 2 and max(lens) == M                          # (on the reference's ids, before anything is compared)
    seen = []
    got, st = ctx.generate_n(prompt, 0, M, states=states, temperature=t, topp=p, stop_token=stop, on_token=lambda j, i, tok, last: seen.append((j, i, tok, last)) and False)
    assert all(np.array_equal(g, w) for g, w in zip(got, want)), ([list(g) for g in got], [list(w) for w in want])
    assert st == after
    # the callback: every delivered id once, per step in sequence order, `last` on a row's final id only
    assert seen == [(j, i, int(want[j][i]), i + 1 == lens[j]) for i in range(M) for j in range(n) if i < lens[j]]
    assert ctx.query("stop_reason") == capi.STOP_LENGTH                  # (over the whole call: a sequence ran to max_tokens)
    # fan_keep of a row that ended EARLY on the stop token: its n_out - 1 fed rows move, whatever the finished rows went on writing behind them
    j = min(range(n), key=lambda r: lens[r])
    assert lens[j] < M
    _fill((ref,), cfg, 0)
    again, _ = ref.generate(prompt, 0, M, temperature=t, topp=p, rng_state=states[j], stop_token=stop)
    assert np.array_equal(again, want[j])
    ctx.fan_keep(j)
    rows = len(prompt) + lens[j] - 1
    for a, b in zip(_caches(ctx, cfg), _caches(ref, cfg)):
        assert np.array_equal(a[:, :rows], b[:, :rows]), (name, j)
    assert np.array_equal(ctx.decode_greedy(stop, rows, 8), ref.decode_greedy(stop, rows, 8))


@pytest.mark.parametrize("name", ["tiny-int8", "tiny128-int8"])
def test_fan_keep_leaves_that_sequences_cache(pair, name):
    """after fan_keep(j) the cache is bit for bit what sequence j's own flm_generate left, and greedy decoding continues from there: j = 0, a middle row, the last row"""
    cfg, ctx, ref = pair(name)
    n, M, t, p, pos = 5, 10, 1.0, 0.9, 4
    prompt = _prompt(cfg.vocab_size, 40, seed=31)
    S = pos + len(prompt)
    states = _states(n, 77)
    for j in (0, 2, n - 1):
        _fill((ctx, ref), cfg, pos)
        want, _ = ref.generate(prompt, pos, M, temperature=t, topp=p, rng_state=states[j])
        got, _ = ctx.generate_n(prompt, pos, M, states=states, temperature=t, topp=p)
        assert np.array_equal(got[j], want)
        ctx.fan_keep(j)
        rows = S + len(want) - 1
        for a, b in zip(_caches(ctx, cfg), _caches(ref, cfg)):
            assert np.array_equal(a[:, :rows], b[:, :rows]), (name, j)
        assert np.array_equal(ctx.decode_greedy(int(want[-1]), rows, 8), ref.decode_greedy(int(want[-1]), rows, 8)), (name, j)
        with pytest.raises(capi.FlmError, match="flm error -1"):
            ctx.fan_keep(j)                                              # once: the move has overwritten tail 0


def test_generate_n_leaves_nothing_behind(pair):
    """a plain generate on the same context after a generate_n equals the reference's, sampled and greedy; so does a second generate_n"""
    cfg, ctx, ref = pair("tiny-int8")
    prompt = _prompt(cfg.vocab_size, 40, seed=41)
    _fill((ctx, ref), cfg, 0)
    states = _states(4, 5)
    first, _ = ctx.generate_n(prompt, 0, 9, states=states, temperature=1.0, topp=0.9)
    other = _prompt(cfg.vocab_size, 17, seed=42)
    for t in (1.0, 0.0):
        want, sw = ref.generate(other, 0, 12, temperature=t, topp=0.9, rng_state=99)
        got, sg = ctx.generate(other, 0, 12, temperature=t, topp=0.9, rng_state=99)
        assert np.array_equal(got, want) and sg == sw
    _fill((ctx,), cfg, 0)
    again, _ = ctx.generate_n(prompt, 0, 9, states=states, temperature=1.0, topp=0.9)
    assert all(np.array_equal(a, b) for a, b in zip(first, again))


def test_cancel_ends_the_whole_call(pair):
    """a truthy return of the callback ends the call: it is not called again, and n_out covers what was delivered -- the step in flight is counted for every row"""
    cfg, ctx, ref = pair("tiny-int8")
    n, M = 4, 12
    prompt = _prompt(cfg.vocab_size, 9, seed=51)
    _fill((ctx, ref), cfg, 0)
    states = _states(n, 6)
    want, _ = _reference(ref, prompt, 0, M, 1.0, 0.9, states)
    seen = []

    def on_token(j, i, tok, last):
        seen.append((j, i))
        return (j, i) == (1, 2)
    got, st = ctx.generate_n(prompt, 0, M, states=states, temperature=1.0, topp=0.9, on_token=on_token)
    assert seen == [(j, i) for i in range(2) for j in range(n)] + [(0, 2), (1, 2)]
    assert all(len(g) == 3 and np.array_equal(g, w[:3]) for g, w in zip(got, want))
    # the states: after exactly n_out draws (the reference's state after 3 tokens)
    _fill((ref,), cfg, 0)
    assert st == _reference(ref, prompt, 0, 3, 1.0, 0.9, states)[1]
    assert ctx.query("stop_reason") == capi.STOP_CANCEL


def test_a_retried_call_delivers_every_id_once(gpu):
    """after a timed-out cross-workgroup wait (injected; the prompt's token launches can have one) the attempt re-runs from what the host holds: the same ids and states,
    every (sequence, index) once"""
    cfg, tensors = _model("tiny-int8")
    ref = _ctx(gpu, cfg, tensors); ctx = _ctx(gpu, cfg, tensors)
    n, M = 3, 8
    prompt = _prompt(cfg.vocab_size, 3, seed=61)
    states = _states(n, 8)
    want, after = _reference(ref, prompt, 0, M, 1.0, 0.9, states)
    seen = []
    ctx.set_option("inject_wait_failure", 1)
    got, st = ctx.generate_n(prompt, 0, M, states=states, temperature=1.0, topp=0.9, on_token=lambda j, i, tok, last: seen.append((j, i)) and False)
    assert all(np.array_equal(g, w) for g, w in zip(got, want)) and st == after
    assert seen == [(j, i) for i in range(M) for j in range(n)]
    assert ctx.query("fallback") == 1
    ref.close(); ctx.close()


def test_every_error_path_launches_nothing(pair, gpu):
    """each refused call returns its code and leaves the cache, the caller's arrays and the kept layout as they were"""
    cfg, ctx, ref = pair("tiny-int8")
    V = cfg.vocab_size
    prompt = _prompt(V, 12, seed=71)
    lib = gpu.lib()
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p) if a is not None else None
    out = np.full((16, 64), -5, np.int32); n_out = np.full(16, -5, np.int32); st = np.arange(1, 17, dtype=np.uint64)

    def call(pr=prompt, n_prompt=12, pos=0, M=6, n=4, t=1.0, states=st, stop=-1, o=out, no=n_out, h=ctx._h):
        return lib.flm_generate_n(h, p(pr), n_prompt, pos, M, n, ctypes.c_float(t), ctypes.c_float(0.9), p(states), ctypes.c_int32(stop), None, None, p(o), p(no))
    _fill((ctx,), cfg, 0)
    ctx.forward(prompt, 0)
    assert lib.flm_fan_keep(ctx._h, 0) == -1                                   # no flm_generate_n precedes
    ctx.generate_n(prompt, 0, 6, states=_states(4, 9), temperature=1.0, topp=0.9)
    before = [c.copy() for c in _caches(ctx, cfg)]
    assert call(n=1) == -1 and call(n=17) == -1                                # n outside 2 .. 16
    assert call(n=16, M=18) == -1                                              # 12 + 16 * 17 = 284 > 256: the capacity condition
    assert call(n=4, M=63) == -1                                               # 12 + 4 * 62 = 260: four rows over (M = 62 fits exactly: below)
    assert call(pr=None) == -1 and call(o=None) == -1 and call(no=None) == -1 and call(states=None) == -1      # null arguments (the states: at temperature != 0)
    bad = prompt.copy(); bad[5] = V
    assert call(pr=bad) == -1                                                  # ids outside [0, vocab)
    bad[5] = -1
    assert call(pr=bad) == -1
    assert call(stop=V) == -1 and call(t=-1.0) == -1 and call(t=float("nan")) == -1
    assert call(M=0) == -1 and call(pos=-1) == -1 and call(n_prompt=0) == -1
    assert call(h=None) == -1
    assert lib.flm_fan_keep(ctx._h, -1) == -1 and lib.flm_fan_keep(ctx._h, 4) == -1       # seq outside [0, n)
    assert (out == -5).all() and (n_out == -5).all() and list(st) == list(range(1, 17))
    for a, b in zip(_caches(ctx, cfg), before):
        assert np.array_equal(a, b)
    ctx.fan_keep(3)                                                            # the refused calls left the kept layout valid
    # the exact fit runs: 12 + 4 * 61 = 256
    assert call(M=62) == 0 and (n_out[:4] == 62).all()
    # a sharded context refuses (-2)
    tp = gpu.Ctx(gpu.desc_from_config(cfg, max_seq_len=MAX_SEQ), device=0, rank=0, world=1, comm_id=gpu.comm_unique_id())
    tp.upload_all(_model("tiny-int8")[1])
    tp.set_option("force_tp", 1)
    with pytest.raises(gpu.FlmError, match="flm error -2"):
        tp.generate_n(prompt, 0, 6, states=[1, 2, 3], temperature=1.0)
    tp.close()


def test_vocabulary_bound_holds_at_temperature_only(gpu):
    """vocab 40000 is beyond the device sampler: temperature 0 runs and equals flm_generate, temperature != 0 is refused as flm_decode_sample refuses it"""
    cfg = synth.make_config("tiny", ff.QT_INT8)
    cfg.vocab_size = 40000
    tensors = synth.make_tensors(cfg, seed=59)
    ref = _ctx(gpu, cfg, tensors); ctx = _ctx(gpu, cfg, tensors)
    prompt = _prompt(cfg.vocab_size, 12)
    want, _ = ref.generate(prompt, 0, 6)
    got, _ = ctx.generate_n(prompt, 0, 6, n=3)
    assert all(np.array_equal(g, want) for g in got)
    with pytest.raises(gpu.FlmError, match="flm error -2"):
        ctx.generate_n(prompt, 0, 6, states=[1, 2, 3], temperature=1.0)
    ref.close(); ctx.close()


def test_nothing_is_allocated_inside_the_call(gpu):
    """the first flm_generate_n and flm_fan_keep of a fresh context, bracketed with hipMemGetInfo"""
    hip = ctypes.CDLL("libamdhip64.so")

    def free_bytes():
        f, t = ctypes.c_size_t(0), ctypes.c_size_t(0)
        assert hip.hipMemGetInfo(ctypes.byref(f), ctypes.byref(t)) == 0
        return f.value
    cfg, tensors = _model("tiny-int8")
    ctx = _ctx(gpu, cfg, tensors)
    ctx.prepare()
    prompt = _prompt(cfg.vocab_size, 40)
    f0 = free_bytes()
    ids, _ = ctx.generate_n(prompt, 0, 8, states=[1, 2, 3, 4, 5], temperature=1.0, topp=0.9)
    ctx.fan_keep(2)
    assert free_bytes() == f0 and len(ids) == 5
    ctx.close()
