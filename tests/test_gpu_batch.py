"""Cache slots (include/flm_gpu.h: flm_batch_open / _join / _step / _state / _close, flm_generate_batch, flm_op_attention_slots; kernels: csrc/flm_batch.h).  Everything is
equality: ids with np.array_equal, sampler states as 64-bit integers, attention outputs and K/V rows on bit patterns.

Op level: flm_op_attention_slots (k_rope_kv_slots + k_attn_slots) against flm_op_attention on a CONTIGUOUS cache per row.  Every cache row no sequence owns holds NaN, so
a read outside a row's own range poisons the result.
Model level: every request against its own flm_generate on a SECOND context whose cache was reset.  max_seq_len is 256 throughout."""
import ctypes

import numpy as np
import pytest

import oracle_py as O
from fast_llama_amd import capi
from test_gpu_spec import MAX_SEQ, MODELS, _caches, _ctx, _model, _model_7b, _prompt, bits

pytestmark = pytest.mark.gpu
HEADS = 2
POSITIONS = (0, 1, 63, 64, 65, 130)
Req = capi.BatchReq


# ---- op level ------------------------------------------------------------------------------------------------------------------------------------------------------
def _slots_case(rng, hs, pos, live, q_scale=1.0):
    """len(pos) slots that ABUT (slot s has pos[s] + 1 rows: pos[s] fed earlier, one for this step), three rows nobody owns behind them; the batch's rows are the slots
    `live`.  NaN wherever no live row's earlier tokens lie -- the slots that are not in the batch included"""
    base = [int(x) for x in np.concatenate([[0], np.cumsum([p + 1 for p in pos])[:-1]])]
    max_seq = base[-1] + pos[-1] + 1 + 3
    kc = np.full((HEADS, max_seq, hs), np.nan, np.float32); vc = np.full_like(kc, np.nan)
    for s in live:
        kc[:, base[s]:base[s] + pos[s]] = rng.standard_normal((HEADS, pos[s], hs)); vc[:, base[s]:base[s] + pos[s]] = rng.standard_normal((HEADS, pos[s], hs))
    n = len(live)
    q = (rng.standard_normal((n, HEADS * hs)) * q_scale).astype(np.float32)
    k = rng.standard_normal((n, HEADS * hs)).astype(np.float32); v = rng.standard_normal((n, HEADS * hs)).astype(np.float32)
    return kc, vc, q, k, v, [base[s] for s in live], [pos[s] for s in live], max_seq


def _own_cache(kc, vc, b, p, hs):
    """row r's own cache: its p earlier rows at [0, p), NaN behind"""
    kr = np.full((HEADS, p + 3, hs), np.nan, np.float32); vr = np.full_like(kr, np.nan)
    kr[:, :p] = kc[:, b:b + p]; vr[:, :p] = vc[:, b:b + p]
    return kr, vr


def _check_slots(gpu, hs, case, tag):
    kc, vc, q, k, v, base, pos, max_seq = case
    kc0, vc0 = kc.copy(), vc.copy()
    out = gpu.op_attention_slots(kc, vc, q, k, v, HEADS, hs, max_seq, base, pos)
    written = np.zeros(max_seq, bool)
    for r, (b, p) in enumerate(zip(base, pos)):
        kr, vr = _own_cache(kc0, vc0, b, p, hs)
        want = gpu.op_attention(kr, vr, q[r], k[r], v[r], HEADS, hs, p + 3, p)
        assert np.array_equal(bits(out[r]), bits(want)), (tag, hs, r, b, p)
        assert np.array_equal(bits(kc[:, b + p]), bits(kr[:, p])) and np.array_equal(bits(vc[:, b + p]), bits(vr[:, p])), (tag, "the step's K/V row", r)
        written[b + p] = True
    assert np.array_equal(bits(kc[:, ~written]), bits(kc0[:, ~written])) and np.array_equal(bits(vc[:, ~written]), bits(vc0[:, ~written])), (tag, "a row nobody wrote has changed")


@pytest.mark.parametrize("B", [1, 2, 3, 9, 16])
@pytest.mark.parametrize("hs", [64, 128])
def test_attention_slots_is_the_contiguous_attention(gpu, hs, B):
    """every row against flm_op_attention on its own cache.  Positions mixed within one batch from 0 / 1 / 63 / 64 / 65 / 130 (T = 1: no earlier row at all; one row;
    a tile less one, a whole tile, a tile and a row; three tiles), rotated so that every position meets every batch size.  First all slots live and abutting --
    base[r + 1] == base[r] + pos[r] + 1: a read one row past a sequence's last lands in its neighbour --, then the live rows a non-contiguous subset of the slots"""
    rng = np.random.default_rng(1000 * hs + B)
    for rot in (0, 3):
        pos = [POSITIONS[(r + rot) % len(POSITIONS)] for r in range(B)]
        case = _slots_case(rng, hs, pos, list(range(B)))
        base = case[5]
        assert all(base[r + 1] == base[r] + pos[r] + 1 for r in range(B - 1))
        _check_slots(gpu, hs, case, ("abut", rot))
    n_slots = min(16, 2 * B + 1)
    pos = [POSITIONS[(s + 1) % len(POSITIONS)] for s in range(n_slots)]
    skipped = list(range(0, n_slots, 2))[:n_slots - B]                                   # slots 0, 2, 4, ... are not in the batch (B = 16: every slot is)
    live = [s for s in range(n_slots) if s not in skipped]
    assert len(live) == B and (B == 16 or live[0] > 0)
    _check_slots(gpu, hs, _slots_case(rng, hs, pos, live), "subset")


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


def test_attention_slots_peaked_scores(gpu):
    """a peaked softmax: weights fall under the 1e-15 skip threshold (asserted in NumPy first), next to weights that count"""
    hs, pos = 64, [130, 65, 130]
    rng = np.random.default_rng(77)
    case = _slots_case(rng, hs, pos, [0, 1, 2], q_scale=30.0)
    kc, vc, q, k, v, base, _, _ = case
    for r in range(3):
        kr, _ = _own_cache(kc, vc, base[r], pos[r], hs)
        for w in _weights(kr, q[r], k[r], hs, pos[r]):
            assert (w[1:] < 1e-17).sum() > 5 and (w > 1e-6).sum() >= 1, "the case is not peaked enough"
    _check_slots(gpu, hs, case, "peaked")


def test_attention_slots_rejects_what_it_does_not_do(gpu):
    rng = np.random.default_rng(3)
    kc, vc, q, k, v, base, pos, max_seq = _slots_case(rng, 64, [4, 2], [0, 1])
    lib = gpu.lib()
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    out = np.empty_like(q)
    call = lambda hs, ms, n, b, ps: lib.flm_op_attention_slots(p(out), p(kc), p(vc), p(q), p(k), p(v), HEADS, hs, ms, n, p(np.array(b, np.int32)), p(np.array(ps, np.int32)))
    k0 = kc.copy()
    assert call(64, max_seq, 0, base, pos) == -1 and call(64, max_seq, 17, base * 9, pos * 9) == -1      # n outside 1 .. 16
    assert call(60, max_seq, 2, base, pos) == -1                                                         # a head size that is no multiple of 8
    assert call(64, max_seq, 2, [0, max_seq - 2], [4, 2]) == -1                                           # a row outside the cache
    assert call(64, max_seq, 2, [0, -1], pos) == -1 and call(64, max_seq, 2, base, [4, -1]) == -1
    assert np.array_equal(bits(kc), bits(k0))


# ---- model level ---------------------------------------------------------------------------------------------------------------------------------------------------
SETTINGS = [(0.0, 0.9), (1.0, 0.9), (0.7, 0.5)]          # greedy and two sampled settings, mixed within one call
LENGTHS = {1: [[1], [2], [63]], 2: [[4, 65], [5, 64], [6, 1]], 5: [[65, 1, 64, 5, 63], [2, 4, 6, 1, 5]],
           16: [[1, 2, 4, 5, 6, 63, 1, 2, 4, 5, 6, 64, 1, 2, 4, 5]]}
_pairs = {}


@pytest.fixture(scope="module")
def pair(gpu):
    """(cfg, the context under test, the reference context) per model, made once"""
    def get(name):
        if name not in _pairs:
            cfg, tensors = _model_7b() if name == "7B" else _model(name)
            _pairs[name] = (cfg, _ctx(gpu, cfg, tensors), _ctx(gpu, cfg, tensors))
        return _pairs[name]
    yield get
    for _, a, b in _pairs.values():
        a.close(); b.close()
    _pairs.clear()


def _requests(V, lengths, seed, stop=-1, M=None):
    """one request per length: its own prompt, max_tokens 3 .. 8, the settings in turn; requests 0 and 1 share a sampler state"""
    st = [int(x) for x in np.random.default_rng(seed).integers(1, 2 ** 62, len(lengths))]
    if len(st) > 1:
        st[1] = st[0]
    return [Req(_prompt(V, L, seed=seed + 7 * j + L), M or 3 + (5 * j) % 6, *SETTINGS[(j + seed) % 3], rng_state=st[j], stop_token=stop) for j, L in enumerate(lengths)]


_ref_cache = {}


def _alone(ref, name, q, max_tokens=None):
    """the request by flm_generate on the reference context with an empty cache -> (ids, the state after)"""
    M = max_tokens or q.max_tokens
    key = (name, bytes(np.asarray(q.prompt, np.int32)), M, q.temperature, q.topp, q.rng_state, q.stop_token)
    if key not in _ref_cache:
        ref.reset_kv()
        ids, st = ref.generate(q.prompt, 0, M, temperature=q.temperature, topp=q.topp, rng_state=q.rng_state, stop_token=q.stop_token)
        _ref_cache[key] = (ids, st if q.temperature != 0 else q.rng_state)
    return _ref_cache[key]


def _check_batch(ctx, ref, name, reqs, tag):
    want = [_alone(ref, name, q) for q in reqs]
    got, st = ctx.generate_batch(reqs)
    assert len(got) == len(reqs)
    for j, (g, (w, sw)) in enumerate(zip(got, want)):
        assert np.array_equal(g, w), (tag, j, len(reqs[j].prompt), list(g), list(w))
        assert st[j] == sw, (tag, j, "the sampler state")
    return got


@pytest.mark.parametrize("n", [1, 2, 5, 16])
@pytest.mark.parametrize("name", list(MODELS))
def test_generate_batch_is_n_generates(pair, name, n):
    """ids, counts and states of every request equal its own flm_generate on a fresh context: prompt lengths 1 .. 6 (below the batched entry's threshold: the join still
    runs them as ONE batch) and 63 / 64 / 65 (around the tile) within one call, max_tokens 3 .. 8, greedy and two sampled settings mixed, two requests on one state"""
    cfg, ctx, ref = pair(name)
    for i, lengths in enumerate(LENGTHS[n]):
        reqs = _requests(cfg.vocab_size, lengths, 100 * n + i)
        assert sum(len(q.prompt) + q.max_tokens - 1 for q in reqs) <= MAX_SEQ
        got = _check_batch(ctx, ref, name, reqs, (name, n, i))
        assert [len(g) for g in got] == [q.max_tokens for q in reqs]
        assert ctx.query("stop_reason") == capi.STOP_LENGTH
    if n >= 5:
        sampled = [j for j, q in enumerate(reqs) if q.temperature != 0]
        assert len({tuple(got[j][:3]) for j in sampled}) > 1, "every sampled request drew the same ids: the case shows nothing"


@pytest.mark.parametrize("name", ["tiny-int8", "small-int8"])
def test_generate_batch_on_the_skinny_gemm(pair, name):
    """ "spec_gemm" 1: the steps' int8 GEMMs, and those of a join of up to 16 rows, run on k_gemm_q8_skinny: the same ids and states"""
    cfg, ctx, ref = pair(name)
    ctx.set_option("spec_gemm", 1)
    try:
        for n in (2, 5, 16):
            _check_batch(ctx, ref, name, _requests(cfg.vocab_size, LENGTHS[n][0], 300 + n), (name, n, "skinny"))
        assert ctx.query("spec_gemm") == 1
    finally:
        ctx.set_option("spec_gemm", 0)


def test_generate_batch_at_7b_width(pair):
    """the 2-layer model of 7B width (head size 128, 32 heads, the GEMMs' production shapes), 16 requests"""
    cfg, ctx, ref = pair("7B")
    _check_batch(ctx, ref, "7B", _requests(cfg.vocab_size, LENGTHS[16][0], 53), "7B")


@pytest.mark.parametrize("name", ["tiny-int8", "small-int8"])
def test_stop_token_ends_slots_one_by_one(pair, name):
    """the stop token, taken from the reference runs, is delivered, counted and not fed; a finished slot leaves the batch while the others go on"""
    cfg, ctx, ref = pair(name)
    M, lengths = 12, [5, 1, 64, 6, 2]
    found = None
    for seed in range(4):
        free = [_alone(ref, name, q)[0] for q in _requests(cfg.vocab_size, lengths, 900 + seed, M=M)]
        for stop in [int(x) for x in np.unique(np.concatenate([f[1:M - 1] for f in free]))][:5]:
            reqs = _requests(cfg.vocab_size, lengths, 900 + seed, stop=stop, M=M)
            want = [_alone(ref, name, q)[0] for q in reqs]
            lens = [len(w) for w in want]
            if len(set(lens)) >= 2 and max(lens) == M and min(lens) < M:
                found = (reqs, want, lens, stop)
                break
        if found:
            break
    assert found, "none of the candidate (stop token, seed) pairs ends two rows at different lengths with one running to max_tokens"
    reqs, want, lens, stop = found
    assert len(set(lens)) >= 2 and max(lens) == M                       # (on the reference's ids, before anything is compared)
    seen = []
    got, _ = ctx.generate_batch(reqs, on_token=lambda j, i, tok, last: seen.append((j, i, tok, last)) and False)
    assert all(np.array_equal(g, w) for g, w in zip(got, want)), ([list(g) for g in got], [list(w) for w in want])
    assert all(g[-1] == stop for g, L in zip(got, lens) if L < M)
    # the callback: every delivered id once, in (step, slot) order, `last` on a request's final id only
    assert seen == [(j, i, int(want[j][i]), i + 1 == lens[j]) for i in range(M) for j in range(len(reqs)) if i < lens[j]]
    assert ctx.query("stop_reason") == capi.STOP_LENGTH                # (over the whole call: a request ran to max_tokens)
    _check_batch(ctx, ref, name, reqs, "again")                        # (states included)


def _history(ref, name, q):
    """[(ids[:k], the state after k draws) for k = 0 .. n_out] of the request alone"""
    full, _ = _alone(ref, name, q)
    return [(full[:0], q.rng_state)] + [(full[:k], _alone(ref, name, q, k)[1]) for k in range(1, len(full) + 1)]


def test_continuous_batching(pair):
    """four slots; A and B join, three steps, C joins, B finishes, D (another prompt length) joins B's slot, steps until nobody is live: A, B, C and D each equal their own
    flm_generate, and batch_state equals the reference's count and state at every step boundary.  Slot 3 is never used: the live rows are a non-contiguous subset"""
    name = "tiny-int8"
    cfg, ctx, ref = pair(name)
    V = cfg.vocab_size
    reqs = {"A": Req(_prompt(V, 5, seed=1), 12, 1.0, 0.9, rng_state=11), "B": Req(_prompt(V, 6, seed=2), 5, 0.7, 0.5, rng_state=12),
            "C": Req(_prompt(V, 63, seed=3), 10, 0.0, 0.9, rng_state=13), "D": Req(_prompt(V, 2, seed=4), 8, 1.0, 0.9, rng_state=14)}
    hist = {k: _history(ref, name, q) for k, q in reqs.items()}
    assert all(len(hist[k]) - 1 == q.max_tokens for k, q in reqs.items())
    ctx.reset_kv()
    ctx.batch_open(capi.batch_layout([40, 30, 90, 30], MAX_SEQ))
    where, live = {}, set()                                              # slot -> the request in it; the slots that run
    ids = {k: [] for k in reqs}
    mask = lambda slots: sum(1 << s for s in slots)

    def check_states():
        for slot, k in where.items():
            st, n, why = ctx.batch_state(slot)
            want_ids, want_st = hist[k][len(ids[k])]
            assert n == len(ids[k]) and st == want_st and np.array_equal(ids[k], want_ids), (k, slot, n)
            assert why == 0                                              # (running, or FLM_STOP_LENGTH: no stop token in this test)

    def join(slot, k):
        tok, is_live = ctx.batch_join(slot, reqs[k])
        assert is_live
        where[slot] = k; ids[k] = [tok]; live.add(slot)
        check_states()

    def step():
        out, live_mask, fin = ctx.batch_step()
        for slot in range(16):
            if slot in live:
                assert out[slot] >= 0
                ids[where[slot]].append(int(out[slot]))
            else:
                assert out[slot] == -1, slot
        done = {s for s in live if len(ids[where[s]]) == reqs[where[s]].max_tokens}
        live.difference_update(done)
        assert fin == mask(done) and live_mask == mask(live), (fin, live_mask, done, live)
        check_states()
        return done

    join(0, "A"); join(1, "B")
    for _ in range(3):
        assert step() == set()
    join(2, "C")
    assert step() == {1} and len(ids["B"]) == 5                          # B's fifth id: its last
    with pytest.raises(capi.FlmError, match="flm error -1"):
        ctx.batch_join(0, reqs["D"])                                     # A is still running there
    b_ids = list(ids["B"])
    assert ctx.batch_state(1)[:2] == (hist["B"][5][1], 5)                # a finished slot's state stays readable ...
    join(1, "D")                                                         # ... until the next join into it: the slot is empty again
    steps = 0
    while live:
        step()
        steps += 1
    assert steps == 8                                                    # C: 10 ids = its join + 1 + 8 steps
    out, live_mask, fin = ctx.batch_step()                               # nobody is live: FLM_OK, nothing delivered
    assert live_mask == 0 and fin == 0 and (out == -1).all()
    ctx.batch_close()
    ids["B"] = b_ids
    for k in reqs:
        assert np.array_equal(ids[k], hist[k][-1][0]), k


@pytest.mark.parametrize("name", ["tiny-int8", "tiny128-int8", "tiny-int16"])
def test_slot_rows_are_the_sequences_own(pair, name):
    """every layer's K and V rows [base, base + n_prompt + n_out - 1) of every slot equal the reference context's rows [0, ...)"""
    cfg, ctx, ref = pair(name)
    reqs = _requests(cfg.vocab_size, LENGTHS[5][0], 41)
    got = _check_batch(ctx, ref, name, reqs, name)
    mine = _caches(ctx, cfg)
    lay = capi.batch_layout([len(q.prompt) + q.max_tokens - 1 for q in reqs], MAX_SEQ)
    for j, q in enumerate(reqs):
        ref.reset_kv()
        ref.generate(q.prompt, 0, q.max_tokens, temperature=q.temperature, topp=q.topp, rng_state=q.rng_state)
        rows, b = len(q.prompt) + len(got[j]) - 1, lay.base[j]
        for a, r in zip(mine, _caches(ref, cfg)):
            assert np.array_equal(a[:, b:b + rows], r[:, :rows]), (name, j)


@pytest.mark.parametrize("keep", [0, 1, 2, 3])
def test_close_keep_leaves_that_sequences_cache(pair, keep):
    """after batch_close(keep) the rows [0, len) are what the sequence's own flm_generate left, and flm_decode_sample continues from pos = len: the first slot (in
    place), slot 1 with base 8 < len (the overlapping move, in chunks of 8 rows), a middle and the last slot"""
    name = "tiny-int8"
    cfg, ctx, ref = pair(name)
    V = cfg.vocab_size
    rows = [8, 100, 20, 60]
    reqs = [Req(_prompt(V, 3, seed=1), 6, 1.0, 0.9, rng_state=5), Req(_prompt(V, 40, seed=2), 30, 1.0, 0.9, rng_state=6),
            Req(_prompt(V, 5, seed=3), 10, 0.0, 0.9, rng_state=7), Req(_prompt(V, 20, seed=4), 20, 0.7, 0.5, rng_state=8)]
    lay = capi.batch_layout(rows, MAX_SEQ)
    ctx.reset_kv()
    ctx.batch_open(lay)
    ids = []
    for s, q in enumerate(reqs):
        ids.append([ctx.batch_join(s, q)[0]])
    live = 0xF
    while live:
        out, live, _ = ctx.batch_step()
        for s in range(4):
            if out[s] >= 0:
                ids[s].append(int(out[s]))
    q = reqs[keep]
    want, st = _alone(ref, name, q)
    assert np.array_equal(ids[keep], want)
    n = len(q.prompt) + len(want) - 1
    assert keep != 1 or lay.base[1] < n                                   # (the overlapping move)
    ref.reset_kv()
    ref.generate(q.prompt, 0, q.max_tokens, temperature=q.temperature, topp=q.topp, rng_state=q.rng_state)
    ctx.batch_close(keep)
    for a, r in zip(_caches(ctx, cfg), _caches(ref, cfg)):
        assert np.array_equal(a[:, :n], r[:, :n]), (keep, "the kept rows")
    a, sa = ctx.decode_sample(int(want[-1]), n, 8, 1.0, 0.9, st)
    b, sb = ref.decode_sample(int(want[-1]), n, 8, 1.0, 0.9, st)
    assert np.array_equal(a, b) and sa == sb
    with pytest.raises(capi.FlmError, match="flm error -5"):
        ctx.batch_close(keep)                                            # the batch has ended


def test_refusals_leave_the_cache_untouched(pair, gpu):
    cfg, ctx, ref = pair("tiny-int8")
    V = cfg.vocab_size
    good = Req(_prompt(V, 6, seed=1), 5, 1.0, 0.9, rng_state=3)
    ctx.reset_kv()
    ctx.batch_open(capi.batch_layout([10, 10, 30], MAX_SEQ))
    ctx.batch_join(0, good)
    before = [c.copy() for c in _caches(ctx, cfg)]

    def refused(code, fn, *a):
        with pytest.raises(capi.FlmError, match=f"flm error {code}:"):
            fn(*a)
    refused(-1, ctx.batch_join, 0, good)                                  # a live slot
    refused(-1, ctx.batch_join, 3, good); refused(-1, ctx.batch_join, -1, good)      # a slot outside the layout
    refused(-1, ctx.batch_join, 1, Req(_prompt(V, 6), 6))                 # 6 + 6 - 1 = 11 rows into a slot of 10 (max_tokens 5 fits exactly: below)
    refused(-1, ctx.batch_join, 1, Req(_prompt(V, 11), 1))
    bad = _prompt(V, 6); bad[3] = V
    refused(-1, ctx.batch_join, 1, Req(bad, 3))                           # ids outside [0, vocab)
    bad[3] = -1
    refused(-1, ctx.batch_join, 1, Req(bad, 3))
    refused(-1, ctx.batch_join, 1, Req(_prompt(V, 6), 3, temperature=-1.0)); refused(-1, ctx.batch_join, 1, Req(_prompt(V, 6), 3, temperature=float("nan")))
    refused(-1, ctx.batch_join, 1, Req(_prompt(V, 6), 3, 1.0, float("nan"))); refused(-1, ctx.batch_join, 1, Req(_prompt(V, 6), 3, stop_token=V))
    refused(-1, ctx.batch_state, 3); refused(-1, ctx.batch_close, 3); refused(-1, ctx.batch_close, 1)      # outside the layout; a slot that never held a sequence
    lay = capi.batch_layout([10, 10], MAX_SEQ); lay.base[1] = 11
    refused(-1, ctx.batch_open, lay)                                      # not flm_batch_layout_for's layout
    big = capi.batch_layout([200, 100], 512)
    refused(-1, ctx.batch_open, big)                                      # ... or one for another max_seq_len
    for a, b in zip(_caches(ctx, cfg), before):
        assert np.array_equal(a, b)
    st, n, _ = ctx.batch_state(0)
    assert n == 1 and st == _alone(ref, "tiny-int8", good, 1)[1]          # the refused calls left the open batch as it was
    tok, live = ctx.batch_join(1, Req(_prompt(V, 6), 5))                  # the exact fit
    assert live
    # another entry point writes the cache: the batch has ended
    ctx.forward(_prompt(V, 4), 200)
    before = [c.copy() for c in _caches(ctx, cfg)]
    refused(-5, ctx.batch_join, 2, good); refused(-5, ctx.batch_step); refused(-5, ctx.batch_close, 0); refused(-5, ctx.batch_state, 0)
    ctx.batch_close()                                                     # (close(-1) of a batch that has ended: nothing to do)
    for a, b in zip(_caches(ctx, cfg), before):
        assert np.array_equal(a, b)
    # generate_batch: what does not fit is refused before anything runs
    refused(-1, ctx.generate_batch, [Req(_prompt(V, 100), 60), Req(_prompt(V, 90), 9)])     # 159 + 98 = 257 rows
    for a, b in zip(_caches(ctx, cfg), before):
        assert np.array_equal(a, b)
    got, _ = ctx.generate_batch([Req(_prompt(V, 100), 60), Req(_prompt(V, 90), 8)])         # 256: the exact fit
    assert [len(g) for g in got] == [60, 8]
    # a sharded context refuses (-2)
    tp = gpu.Ctx(gpu.desc_from_config(cfg, max_seq_len=MAX_SEQ), device=0, rank=0, world=1, comm_id=gpu.comm_unique_id())
    tp.upload_all(_model("tiny-int8")[1])
    tp.set_option("force_tp", 1)
    refused(-2, tp.generate_batch, [good]); refused(-2, tp.batch_open, capi.batch_layout([10], MAX_SEQ))
    tp.close()


def test_cancel_ends_the_call_behind_its_step(pair):
    """a truthy return of the callback: it is not called again, the step in flight is counted for every slot, the states are behind exactly the delivered ids"""
    name = "tiny-int8"
    cfg, ctx, ref = pair(name)
    reqs = _requests(cfg.vocab_size, [5, 2, 6, 1], 61, M=10)
    seen = []

    def on_token(j, i, tok, last):
        seen.append((j, i))
        return (j, i) == (1, 2)
    got, st = ctx.generate_batch(reqs, on_token=on_token)
    assert seen == [(j, i) for i in range(2) for j in range(4)] + [(0, 2), (1, 2)]
    for j, q in enumerate(reqs):
        w, sw = _alone(ref, name, q, 3)
        assert np.array_equal(got[j], w) and st[j] == sw, j
    assert ctx.query("stop_reason") == capi.STOP_CANCEL


def test_a_retried_step_delivers_every_id_once(gpu):
    """a cross-workgroup wait that gave up (injected) is noticed behind a step: the step re-runs from what the host holds -- the same ids and states, nothing twice"""
    name = "tiny-int8"
    cfg, tensors = _model(name)
    ref = _ctx(gpu, cfg, tensors); ctx = _ctx(gpu, cfg, tensors)
    reqs = _requests(cfg.vocab_size, [3, 6, 1], 8, M=8)
    want = [_alone(ref, name, q) for q in reqs]
    ctx.batch_open(capi.batch_layout([len(q.prompt) + 7 for q in reqs], MAX_SEQ))
    ids = [[ctx.batch_join(s, q)[0]] for s, q in enumerate(reqs)]
    for step in range(7):
        if step == 2:
            ctx.set_option("inject_wait_failure", 1)
        out, live, _ = ctx.batch_step()
        assert (out[:3] >= 0).all() and (out[3:] == -1).all()
        for s in range(3):
            ids[s].append(int(out[s]))
    assert live == 0 and ctx.query("fallback") == 1
    for s in range(3):
        assert np.array_equal(ids[s], want[s][0]) and ctx.batch_state(s)[:2] == (want[s][1], 8)
    ctx.batch_close()
    ref.close(); ctx.close()


def test_nothing_is_allocated_inside_the_calls(gpu):
    """the first open / join / step / close of a fresh context, bracketed with hipMemGetInfo"""
    hip = ctypes.CDLL("libamdhip64.so")

    def free_bytes():
        f, t = ctypes.c_size_t(0), ctypes.c_size_t(0)
        assert hip.hipMemGetInfo(ctypes.byref(f), ctypes.byref(t)) == 0
        return f.value
    cfg, tensors = _model("tiny-int8")
    ctx = _ctx(gpu, cfg, tensors)
    ctx.prepare()
    V = cfg.vocab_size
    lay = capi.batch_layout([20, 60, 70], MAX_SEQ)
    f0 = free_bytes()
    ctx.batch_open(lay)
    ctx.batch_join(0, Req(_prompt(V, 3), 6, 1.0, 0.9, rng_state=1))
    ctx.batch_join(2, Req(_prompt(V, 40), 6, 0.0, 0.9))
    for _ in range(3):
        ctx.batch_step()
    ctx.batch_join(1, Req(_prompt(V, 30), 6, 0.7, 0.5, rng_state=2))
    live = 1
    while live:
        _, live, _ = ctx.batch_step()
    ctx.batch_close(2)
    assert free_bytes() == f0
    ctx.close()
