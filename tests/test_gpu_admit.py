"""Ragged passes over the cache slots (include/flm_gpu.h: flm_batch_admit / flm_batch_pass, option "batch_rows", flm_op_attention_segs; kernels: csrc/flm_segs.h).
Everything is equality: ids with np.array_equal, sampler states as 64-bit integers, attention outputs and K/V rows on bit patterns.

Op level: every row of flm_op_attention_segs against flm_op_attention on that row's own CONTIGUOUS cache.  Every cache row no sequence owns holds NaN and the slots abut,
so a read one row past a sequence lands in its neighbour (the scheme of test_gpu_batch._check_slots).
Model level: every request against its own flm_generate on a SECOND context whose cache was reset.  max_seq_len is 256 throughout."""
import ctypes

import numpy as np
import pytest

from fast_llama_amd import capi
from test_gpu_batch import HEADS, LENGTHS, Req, _alone, _history, _requests, _weights, pair  # noqa: F401  (pair: the module's fixture)
from test_gpu_spec import MAX_SEQ, MODELS, _caches, _ctx, _model, _prompt, bits

pytestmark = pytest.mark.gpu
SEG_LENGTHS = (1, 2, 7, 8, 9, 17)          # a lone query, a group less one, a whole group, a group and one, three groups with a tail (groups of kMqQueries = 8)
SEG_POS0 = (0, 1, 56, 63, 64, 120)         # a first chunk; T = 1 + ...; a group of eight straddles the 64-position tile edge; later chunks read rows an earlier call wrote


# ---- op level ------------------------------------------------------------------------------------------------------------------------------------------------------
def _segs_case(rng, hs, ns, pos0, n_step=0, q_scale=1.0):
    """len(ns) slots that ABUT: slot s has pos0[s] + ns[s] rows -- pos0[s] fed earlier, ns[s] for this pass -- and three rows nobody owns lie behind the last one.  NaN
    wherever no segment's earlier rows lie"""
    rows = [p + n for p, n in zip(pos0, ns)]
    base = [int(x) for x in np.concatenate([[0], np.cumsum(rows)[:-1]])]
    max_seq = base[-1] + rows[-1] + 3
    kc = np.full((HEADS, max_seq, hs), np.nan, np.float32); vc = np.full_like(kc, np.nan)
    for b, p in zip(base, pos0):
        kc[:, b:b + p] = rng.standard_normal((HEADS, p, hs)); vc[:, b:b + p] = rng.standard_normal((HEADS, p, hs))
    B = sum(ns)
    q = (rng.standard_normal((B, HEADS * hs)) * q_scale).astype(np.float32)
    k = rng.standard_normal((B, HEADS * hs)).astype(np.float32); v = rng.standard_normal((B, HEADS * hs)).astype(np.float32)
    assert all(ns[s] == 1 for s in range(n_step))
    return kc, vc, q, k, v, base, rows, list(ns), list(pos0), max_seq, n_step


def _check_segs(gpu, hs, case, tag, one_query=False):
    kc, vc, q, k, v, base, rows, ns, pos0, max_seq, n_step = case
    assert all(base[s + 1] == base[s] + rows[s] for s in range(len(ns) - 1))          # the slots abut
    kc0, vc0 = kc.copy(), vc.copy()
    out = gpu.op_attention_segs(kc, vc, q, k, v, HEADS, hs, max_seq, base, rows, ns, pos0, n_step=n_step, one_query=one_query)
    written = np.zeros(max_seq, bool)
    row = 0
    for s, (b, n, p) in enumerate(zip(base, ns, pos0)):
        T = p + n + 3                                                                 # the sequence's own cache: its p earlier rows, NaN behind; row after row
        kr = np.full((HEADS, T, hs), np.nan, np.float32); vr = np.full_like(kr, np.nan)
        kr[:, :p] = kc0[:, b:b + p]; vr[:, :p] = vc0[:, b:b + p]
        for i in range(n):
            want = gpu.op_attention(kr, vr, q[row], k[row], v[row], HEADS, hs, T, p + i)
            assert np.array_equal(bits(out[row]), bits(want)), (tag, hs, "segment", s, "row", i, "pos0", p, "n", n)
            row += 1
        assert np.array_equal(bits(kc[:, b + p:b + p + n]), bits(kr[:, p:p + n])) and np.array_equal(bits(vc[:, b + p:b + p + n]), bits(vr[:, p:p + n])), (tag, "the segment's K/V rows", s)
        written[b + p:b + p + n] = True
    assert np.array_equal(bits(kc[:, ~written]), bits(kc0[:, ~written])) and np.array_equal(bits(vc[:, ~written]), bits(vc0[:, ~written])), (tag, "a row nobody wrote has changed")


FORMS = [(64, False), (128, False), (40, False), (136, False), (256, False), (64, True)]      # 64 / 40: NF = 1, 128: NF = 2 (multi-query); 136, 256 and the forced one: one query


@pytest.mark.parametrize("n_segs", [1, 2, 16])
@pytest.mark.parametrize("hs,one_query", FORMS, ids=[f"hs{h}{'-one-query' if o else ''}" for h, o in FORMS])
def test_attention_segs_is_the_contiguous_attention(gpu, hs, one_query, n_segs):
    """segment s has length SEG_LENGTHS[s % 6] and enters at SEG_POS0[(s + rot) % 6]; over the six rotations every length meets every pos0 (16 segments: within one
    call as well)"""
    rng = np.random.default_rng(1000 * hs + 10 * n_segs + one_query)
    met = set()
    for rot in range(6):
        first = rot if n_segs < 16 else 0                                             # (few segments: the rotation also moves through the lengths)
        ns = [SEG_LENGTHS[(first + s) % 6] for s in range(n_segs)]
        pos0 = [SEG_POS0[(first + s + rot) % 6] for s in range(n_segs)]
        met.update(zip(ns, pos0))
        _check_segs(gpu, hs, _segs_case(rng, hs, ns, pos0), (n_segs, rot), one_query)
    assert n_segs < 16 or len(met) == 36


@pytest.mark.parametrize("hs,one_query", [(64, False), (128, False), (136, False)])
def test_attention_segs_behind_step_rows(gpu, hs, one_query):
    """three step rows in front (k_rope_kv_slots + k_attn_slots), then two prompt segments"""
    rng = np.random.default_rng(hs)
    _check_segs(gpu, hs, _segs_case(rng, hs, [1, 1, 1, 9, 17], [64, 0, 130, 63, 1], n_step=3), "step rows", one_query)


def test_attention_segs_peaked_scores(gpu):
    """a peaked softmax: weights fall under the 1e-15 skip threshold (asserted in NumPy first, on every segment's first row), next to weights that count"""
    hs, ns, pos0 = 64, [9, 17, 8], [120, 56, 64]
    case = _segs_case(np.random.default_rng(77), hs, ns, pos0, q_scale=30.0)
    kc, vc, q, k, v, base = case[:6]
    row = 0
    for s in range(3):
        for w in _weights(kc[:, base[s]:base[s] + pos0[s]], q[row], k[row], hs, pos0[s]):
            assert (w[1:] < 1e-17).sum() > 5 and (w > 1e-6).sum() >= 1, "the case is not peaked enough"
        row += ns[s]
    _check_segs(gpu, hs, case, "peaked")
    _check_segs(gpu, hs, _segs_case(np.random.default_rng(77), hs, ns, pos0, q_scale=30.0), "peaked, one query", one_query=True)


def test_attention_segs_rejects_what_it_does_not_do(gpu):
    kc, vc, q, k, v, base, rows, ns, pos0, max_seq, _ = _segs_case(np.random.default_rng(3), 64, [4, 2], [3, 5])
    lib = gpu.lib()
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    i32 = lambda x: np.array(x, np.int32)
    out = np.empty_like(q)

    def call(B, n_segs, n_step, b, rw, n, ps, hs=64):
        keep = [i32(b), i32(rw), i32(n), i32(ps)]
        return lib.flm_op_attention_segs(p(out), p(kc), p(vc), p(q), p(k), p(v), HEADS, hs, max_seq, B, n_segs, n_step, *[p(a) for a in keep], 0)
    k0, v0 = kc.copy(), vc.copy()
    assert call(6, 2, 0, base, [rows[0] - 1, rows[1]], ns, pos0) == -1              # a segment outside its slot
    assert call(6, 2, 0, base, rows, ns, [3, -1]) == -1
    assert call(6, 2, 0, [base[0], max_seq - 2], rows, ns, pos0) == -1              # a slot outside the cache
    assert call(17, 17, 0, [0] * 17, [1] * 17, [1] * 17, [0] * 17) == -1            # more than 16 segments
    assert call(7, 2, 0, base, rows, ns, pos0) == -1 and call(5, 2, 0, base, rows, ns, pos0) == -1      # the rows given are not the segments' sum
    assert call(6, 2, 1, base, rows, ns, pos0) == -1                                # a step segment of four rows
    assert call(6, 2, 3, base, rows, ns, pos0) == -1 and call(6, 0, 0, base, rows, ns, pos0) == -1
    assert call(6, 2, 0, base, rows, ns, pos0, hs=60) == -1                         # a head size that is no multiple of 8
    assert np.array_equal(bits(kc), bits(k0)) and np.array_equal(bits(vc), bits(v0))
    assert call(6, 2, 0, base, rows, ns, pos0) == 0                                 # (the case itself is served)


# ---- model level ---------------------------------------------------------------------------------------------------------------------------------------------------
def _rows_of(reqs):
    return [len(q.prompt) + q.max_tokens - 1 for q in reqs]


def _serve(ctx, reqs, budget=0, rows=None, close=True):
    """open, admit every request, pass(budget) until nobody runs or fills -> (ids per slot, (state, n_out, reason) per slot, the number of passes)"""
    n = len(reqs)
    ctx.reset_kv()
    ctx.batch_open(capi.batch_layout(rows or _rows_of(reqs), MAX_SEQ))
    for s, q in enumerate(reqs):
        ctx.batch_admit(s, q)
    ids = [[] for _ in reqs]
    passes, busy = 0, 1
    while busy:
        out, live, fin, filling = ctx.batch_pass(budget)
        passes += 1
        assert passes <= 4 * MAX_SEQ and (out[n:] == -1).all() and not live & filling
        for s in range(n):
            if out[s] >= 0:
                ids[s].append(int(out[s]))
                assert bool((fin >> s) & 1) == (len(ids[s]) == reqs[s].max_tokens or out[s] == reqs[s].stop_token)
            else:
                assert not (fin >> s) & 1
        busy = live | filling
    states = [ctx.batch_state(s) for s in range(n)]
    if close:
        ctx.batch_close()
    return ids, states, passes


def _check_served(ctx, ref, name, reqs, tag, budget=0):
    want = [_alone(ref, name, q) for q in reqs]
    got, states, passes = _serve(ctx, reqs, budget)
    for j, (g, (w, sw)) in enumerate(zip(got, want)):
        assert np.array_equal(g, w), (tag, j, len(reqs[j].prompt), g, list(w))
        assert states[j][:2] == (sw, len(w)), (tag, j, "the sampler state and the count")
    return got, passes


@pytest.mark.parametrize("n", [1, 2, 5, 16])
@pytest.mark.parametrize("name", list(MODELS))
def test_admit_and_pass_is_n_generates(pair, name, n):
    """admit x n, then pass(0) until done: ids, counts and states of every request equal its own flm_generate on a fresh context -- prompt lengths 1 .. 6 and 63 / 64 / 65
    within one call, max_tokens 3 .. 8 and one request with max_tokens 1, greedy and two sampled settings mixed, two requests on one state.  Unbounded: every prompt
    completes in pass 0, so the call makes max(max_tokens) passes"""
    cfg, ctx, ref = pair(name)
    for i, lengths in enumerate(LENGTHS[n]):
        reqs = _requests(cfg.vocab_size, lengths, 100 * n + i)
        if n >= 2:
            reqs[-1].max_tokens = 1
        got, passes = _check_served(ctx, ref, name, reqs, (name, n, i))
        assert [len(g) for g in got] == [q.max_tokens for q in reqs] and passes == max(q.max_tokens for q in reqs)
    if n >= 5:
        sampled = [j for j, q in enumerate(reqs) if q.temperature != 0 and q.max_tokens >= 3]
        assert len({tuple(got[j][:3]) for j in sampled}) > 1, "every sampled request drew the same ids: the case shows nothing"


_ref_rows = {}


def _fresh_rows(ref, cfg, name, q):
    """the K / V rows flm_generate leaves for the request on a fresh context (made once per request)"""
    key = (name, bytes(np.asarray(q.prompt, np.int32)), q.max_tokens, q.temperature, q.topp, q.rng_state)
    if key not in _ref_rows:
        ref.reset_kv()
        ids, _ = ref.generate(q.prompt, 0, q.max_tokens, temperature=q.temperature, topp=q.topp, rng_state=q.rng_state)
        rows = len(q.prompt) + len(ids) - 1
        _ref_rows[key] = [c[:, :rows].copy() for c in _caches(ref, cfg)]
    return _ref_rows[key]


@pytest.mark.parametrize("budget", [1, 3, 8, 64])
@pytest.mark.parametrize("name", ["tiny-int8", "tiny128-int8"])
def test_chunked_prompts_leave_the_same_ids_and_rows(pair, name, budget):
    """a 65-token prompt beside two short ones, cut into chunks of at most `budget` rows per pass: the same ids, counts and states, and every slot's K / V rows equal the
    fresh context's rows bit for bit (a chunk at pos0 > 0 attends rows an earlier pass wrote; budget 8: chunks of whole groups; 3 and 1: the tile edge inside a prompt)"""
    cfg, ctx, ref = pair(name)
    V = cfg.vocab_size
    reqs = [Req(_prompt(V, 3, seed=21), 6, 1.0, 0.9, rng_state=31), Req(_prompt(V, 65, seed=22), 5, 0.7, 0.5, rng_state=32), Req(_prompt(V, 5, seed=23), 7, 0.0, 0.9)]
    want = [_alone(ref, name, q) for q in reqs]
    got, states, passes = _serve(ctx, reqs, budget, close=False)
    assert passes > max(q.max_tokens for q in reqs) or budget == 64                  # (the prompts did take several passes)
    mine = _caches(ctx, cfg)
    ctx.batch_close()
    lay = capi.batch_layout(_rows_of(reqs), MAX_SEQ)
    for j, q in enumerate(reqs):
        assert np.array_equal(got[j], want[j][0]) and states[j][:2] == (want[j][1], len(want[j][0])), (budget, j)
        theirs = _fresh_rows(ref, cfg, name, q)
        rows, b = theirs[0].shape[1], lay.base[j]
        assert rows == len(q.prompt) + len(got[j]) - 1
        for a, r in zip(mine, theirs):
            assert np.array_equal(a[:, b:b + rows], r), (name, budget, j)


def test_requests_enter_and_leave_mid_flight(pair):
    """four slots, a budget of 4 prompt rows per pass: A (5 tokens) and B (6) are admitted at pass 0, C (63) at pass 2, D at pass 5 into the slot of B, which has
    finished by then.  Every request equals its own flm_generate; batch_state equals the reference's count and state at every pass boundary, a filling slot's included"""
    name = "tiny-int8"
    cfg, ctx, ref = pair(name)
    V = cfg.vocab_size
    reqs = {"A": Req(_prompt(V, 5, seed=1), 12, 1.0, 0.9, rng_state=11), "B": Req(_prompt(V, 6, seed=2), 2, 0.7, 0.5, rng_state=12),
            "C": Req(_prompt(V, 63, seed=3), 6, 0.0, 0.9, rng_state=13), "D": Req(_prompt(V, 2, seed=4), 8, 1.0, 0.9, rng_state=14)}
    hist = {k: _history(ref, name, q) for k, q in reqs.items()}
    ctx.reset_kv()
    ctx.batch_open(capi.batch_layout([40, 30, 90, 30], MAX_SEQ))
    where, ids, fed = {}, {k: [] for k in reqs}, {k: 0 for k in reqs}
    done_ids = {}

    def admit(slot, k):
        if slot in where:
            done_ids[where[slot]] = ids[where[slot]]
        ctx.batch_admit(slot, reqs[k]); where[slot] = k

    def check_states(filling):
        for slot, k in where.items():
            st, n, why = ctx.batch_state(slot)
            want_ids, want_st = hist[k][len(ids[k])]
            assert n == len(ids[k]) and st == want_st and why == 0, (k, slot, n)
            assert bool((filling >> slot) & 1) == (fed[k] < len(reqs[k].prompt))
            if (filling >> slot) & 1:
                assert n == 0 and st == reqs[k].rng_state
    admit(0, "A"); admit(1, "B")
    check_states(0b11)
    busy, p = 1, 0
    while busy:
        if p == 2:
            admit(2, "C")
        if p == 5:
            assert len(ids["B"]) == 2                                               # B has delivered its last id ...
            with pytest.raises(capi.FlmError, match="flm error -1"):
                ctx.batch_admit(0, reqs["D"])                                        # (A is still running there)
            admit(1, "D")                                                            # ... its slot is empty again
        budget = 4
        for slot in sorted(where):                                                   # the host's own statement of the budget, in ascending slot order
            k = where[slot]
            take = min(len(reqs[k].prompt) - fed[k], budget)
            fed[k] += take; budget -= take
        out, live, fin, filling = ctx.batch_pass(4)
        for slot, k in where.items():
            if out[slot] >= 0:
                ids[k].append(int(out[slot]))
        check_states(filling)
        busy = live | filling
        p += 1
        assert p < 100
    assert p > 16                                                                    # (C's 63 rows at 4 per pass)
    with pytest.raises(capi.FlmError, match="flm error -1"):
        ctx.batch_pass(-1)                                                           # a negative budget
    out, live, fin, filling = ctx.batch_pass(4)                                      # nobody runs or fills: FLM_OK, nothing delivered
    assert (out == -1).all() and live == fin == filling == 0
    ctx.batch_close()
    ids.update(done_ids)
    for k in reqs:
        assert np.array_equal(ids[k], hist[k][-1][0]), k


def test_the_join_route_and_the_admit_route_agree_and_mix(pair):
    """the same requests through join / step and through admit / pass give the same ids; so does a batch in which slots 0 and 2 joined, 1 and 3 were admitted, and
    pass() serves all four; step() in between leaves the filling slots alone"""
    name = "small-int8"
    cfg, ctx, ref = pair(name)
    reqs = _requests(cfg.vocab_size, [5, 64, 2, 9], 77, M=6)
    by_join, st_join = ctx.generate_batch(reqs)
    by_pass, states, _ = _serve(ctx, reqs, 8)
    for j in range(4):
        assert np.array_equal(by_join[j], by_pass[j]) and st_join[j] == states[j][0] and np.array_equal(by_join[j], _alone(ref, name, reqs[j])[0])
    ctx.reset_kv()
    ctx.batch_open(capi.batch_layout(_rows_of(reqs), MAX_SEQ))
    ids = [[] for _ in reqs]
    for s in (0, 2):
        ids[s].append(ctx.batch_join(s, reqs[s])[0])
    ctx.batch_admit(1, reqs[1]); ctx.batch_admit(3, reqs[3])
    with pytest.raises(capi.FlmError, match="flm error -1"):
        ctx.batch_join(1, reqs[1])                                                   # a filling slot
    out, live, fin = ctx.batch_step()                                                # a step: the running slots only
    assert live == 0b0101 and (out[[1, 3]] == -1).all() and ctx.batch_state(1)[1] == 0
    for s in (0, 2):
        ids[s].append(int(out[s]))
    busy = 1
    while busy:
        out, live, fin, filling = ctx.batch_pass(16)
        for s in range(4):
            if out[s] >= 0:
                ids[s].append(int(out[s]))
        busy = live | filling
    ctx.batch_close()
    for j in range(4):
        assert np.array_equal(ids[j], by_join[j]), j


def test_a_stop_token_as_token_0(pair):
    """token 0 of a request, taken from the reference run, is its stop token: delivered, counted, finished in the pass that completes the prompt, never running"""
    name = "tiny-int8"
    cfg, ctx, ref = pair(name)
    free = _requests(cfg.vocab_size, [5, 9, 2], 500, M=6)
    stop = int(_alone(ref, name, free[1])[0][0])
    reqs = _requests(cfg.vocab_size, [5, 9, 2], 500, M=6)
    reqs[1].stop_token = stop
    assert list(_alone(ref, name, reqs[1])[0]) == [stop]
    ctx.reset_kv()
    ctx.batch_open(capi.batch_layout(_rows_of(reqs), MAX_SEQ))
    for s, q in enumerate(reqs):
        ctx.batch_admit(s, q)
    out, live, fin, filling = ctx.batch_pass(0)
    assert out[1] == stop and (fin >> 1) & 1 and not (live >> 1) & 1 and filling == 0 and live == 0b101
    assert ctx.batch_state(1)[1:] == (1, capi.STOP_TOKEN)
    ctx.batch_close()
    _check_served(ctx, ref, name, reqs, "stop as token 0", budget=3)


def test_close_keep_of_an_admitted_slot(pair):
    """close(keep) of a FILLING slot is refused; of a slot that was admitted and ran, it leaves the sequence's rows at [0, len) and flm_decode_sample continues there"""
    name = "tiny-int8"
    cfg, ctx, ref = pair(name)
    V = cfg.vocab_size
    reqs = [Req(_prompt(V, 3, seed=1), 6, 1.0, 0.9, rng_state=5), Req(_prompt(V, 40, seed=2), 9, 1.0, 0.9, rng_state=6)]
    ctx.reset_kv()
    ctx.batch_open(capi.batch_layout([8, 100], MAX_SEQ))
    ctx.batch_admit(0, reqs[0]); ctx.batch_admit(1, reqs[1])
    out, live, fin, filling = ctx.batch_pass(10)                                     # slot 0 completes, slot 1 has 7 of its 40 rows
    assert filling == 0b10 and out[0] >= 0 and out[1] == -1
    with pytest.raises(capi.FlmError, match="flm error -1"):
        ctx.batch_close(1)
    ids = [int(out[0])], []
    busy = 1
    while busy:
        out, live, fin, filling = ctx.batch_pass(10)
        for s in range(2):
            if out[s] >= 0:
                ids[s].append(int(out[s]))
        busy = live | filling
    q = reqs[1]
    want, st = _alone(ref, name, q)
    assert np.array_equal(ids[1], want) and np.array_equal(ids[0], _alone(ref, name, reqs[0])[0])
    n = len(q.prompt) + len(want) - 1
    ref.reset_kv()
    ref.generate(q.prompt, 0, q.max_tokens, temperature=q.temperature, topp=q.topp, rng_state=q.rng_state)
    ctx.batch_close(1)
    for a, r in zip(_caches(ctx, cfg), _caches(ref, cfg)):
        assert np.array_equal(a[:, :n], r[:, :n]), "the kept rows"
    a, sa = ctx.decode_sample(int(want[-1]), n, 8, 1.0, 0.9, st)
    b, sb = ref.decode_sample(int(want[-1]), n, 8, 1.0, 0.9, st)
    assert np.array_equal(a, b) and sa == sb


@pytest.mark.parametrize("name", ["tiny-int8", "small-int8"])
def test_passes_on_the_skinny_gemm(pair, name):
    """ "spec_gemm" 1: a pass of at most 16 rows runs its int8 GEMMs on k_gemm_q8_skinny (budget 4 beside up to 5 step rows; the unbounded first pass of 18 rows runs
    the tiles): the same ids and states"""
    cfg, ctx, ref = pair(name)
    ctx.set_option("spec_gemm", 1)
    try:
        reqs = _requests(cfg.vocab_size, LENGTHS[5][1], 305)
        assert sum(len(q.prompt) for q in reqs) == 18
        _check_served(ctx, ref, name, reqs, (name, "skinny", 4), budget=4)
        _check_served(ctx, ref, name, reqs, (name, "skinny", 0), budget=0)
    finally:
        ctx.set_option("spec_gemm", 0)


def test_admit_and_pass_at_7b_width(pair):
    """the 2-layer model of 7B width (head size 128, 32 heads, the GEMMs' production shapes), 16 requests, unbounded and with a budget of 8"""
    cfg, ctx, ref = pair("7B")
    reqs = _requests(cfg.vocab_size, LENGTHS[16][0], 53)
    _check_served(ctx, ref, "7B", reqs, "7B")
    _check_served(ctx, ref, "7B", reqs, "7B, 8 rows", budget=8)


def test_generate_batch_under_batch_rows(pair):
    """option "batch_rows" 0 and 8: flm_generate_batch's results equal the default's; 16 requests of 13-token prompts and 4 tokens each (the cache's 256 rows) make 4
    weight passes under "batch_rows" 0 (every prompt row and every token 0 in the first), against 16 joins + 3 steps by default"""
    name = "tiny-int8"
    cfg, ctx, ref = pair(name)
    V = cfg.vocab_size
    assert ctx.query("batch_rows") == -1
    mixed = _requests(V, LENGTHS[5][0], 41)
    same = [Req(_prompt(V, 13, seed=60 + j), 4, *[(0.0, 0.9), (1.0, 0.9)][j % 2], rng_state=70 + j) for j in range(16)]
    assert sum(_rows_of(same)) == MAX_SEQ
    default = {}
    for tag, reqs in (("mixed", mixed), ("same", same)):
        default[tag] = ctx.generate_batch(reqs)
        for j, q in enumerate(reqs):
            assert np.array_equal(default[tag][0][j], _alone(ref, name, q)[0])
    try:
        for rows in (0, 8):
            ctx.set_option("batch_rows", rows)
            assert ctx.query("batch_rows") == rows
            for tag, reqs in (("mixed", mixed), ("same", same)):
                seen = []
                got, st = ctx.generate_batch(reqs, on_token=lambda j, i, tok, last: seen.append((j, i, tok, last)) and False)
                assert all(np.array_equal(g, w) for g, w in zip(got, default[tag][0])) and st == default[tag][1], (rows, tag)
                assert sorted(seen) == sorted((j, i, int(t), i + 1 == len(g)) for j, g in enumerate(got) for i, t in enumerate(g))      # every id once; (pass, slot) order
                assert all(a[1] < b[1] for a, b in zip(seen, seen[1:]) if a[0] == b[0]) and ctx.query("stop_reason") == capi.STOP_LENGTH
            if rows == 0:
                assert ctx.query("batch_passes") == 4
        ctx.set_option("batch_rows", -1)
        ctx.generate_batch(same)
        assert ctx.query("batch_passes") == 19
    finally:
        ctx.set_option("batch_rows", -1)


def test_batch_passes_counts_the_ragged_path(gpu):
    """16 requests of 16-token prompts, 4 tokens each (16 x 19 rows: this one context has max_seq_len 512): 4 weight passes under "batch_rows" 0, 19 by default"""
    cfg, tensors = _model("tiny-int8")
    ctx = gpu.Ctx(gpu.desc_from_config(cfg, max_seq_len=512)); ctx.upload_all(tensors)
    reqs = [Req(_prompt(cfg.vocab_size, 16, seed=80 + j), 4, 0.0, 0.9) for j in range(16)]
    want, _ = ctx.generate_batch(reqs)
    assert ctx.query("batch_passes") == 19
    ctx.set_option("batch_rows", 0)
    got, _ = ctx.generate_batch(reqs)
    assert ctx.query("batch_passes") == 4 and all(np.array_equal(g, w) for g, w in zip(got, want))
    ctx.close()


def test_refusals_leave_the_cache_untouched(pair, gpu):
    cfg, ctx, ref = pair("tiny-int8")
    V = cfg.vocab_size
    good = Req(_prompt(V, 6, seed=1), 5, 1.0, 0.9, rng_state=3)

    def refused(code, fn, *a):
        with pytest.raises(capi.FlmError, match=f"flm error {code}:"):
            fn(*a)
    ctx.reset_kv()
    ctx.batch_close()
    refused(-5, ctx.batch_admit, 0, good); refused(-5, ctx.batch_pass, 0)             # no open batch
    ctx.batch_open(capi.batch_layout([10, 10, 30], MAX_SEQ))
    ctx.batch_join(0, good)
    ctx.batch_admit(2, good)
    before = [c.copy() for c in _caches(ctx, cfg)]
    refused(-1, ctx.batch_admit, 0, good); refused(-1, ctx.batch_admit, 2, good); refused(-1, ctx.batch_join, 2, good)      # a running slot, a filling slot
    refused(-1, ctx.batch_admit, 3, good); refused(-1, ctx.batch_admit, -1, good)     # a slot outside the layout
    refused(-1, ctx.batch_admit, 1, Req(_prompt(V, 6), 6)); refused(-1, ctx.batch_admit, 1, Req(_prompt(V, 11), 1))      # 11 rows into a slot of 10
    bad = _prompt(V, 6); bad[3] = V
    refused(-1, ctx.batch_admit, 1, Req(bad, 3))                                      # ids outside [0, vocab)
    bad[3] = -1
    refused(-1, ctx.batch_admit, 1, Req(bad, 3))
    refused(-1, ctx.batch_admit, 1, Req(_prompt(V, 6), 3, temperature=-1.0)); refused(-1, ctx.batch_admit, 1, Req(_prompt(V, 6), 3, temperature=float("nan")))
    refused(-1, ctx.batch_admit, 1, Req(_prompt(V, 6), 3, 1.0, float("nan"))); refused(-1, ctx.batch_admit, 1, Req(_prompt(V, 6), 3, stop_token=V))
    refused(-1, ctx.batch_pass, -1); refused(-1, ctx.batch_close, 2)                  # a negative budget; close(keep) of a filling slot
    for a, b in zip(_caches(ctx, cfg), before):
        assert np.array_equal(a, b)
    assert ctx.batch_state(2)[1:] == (0, 0) and ctx.batch_state(0)[1] == 1           # the refused calls left the open batch as it was
    ctx.batch_admit(1, Req(_prompt(V, 6), 5))                                         # the exact fit
    out, live, fin, filling = ctx.batch_pass(0)
    assert (out[:3] >= 0).all() and live == 0b111 and filling == 0
    ctx.forward(_prompt(V, 4), 200)                                                   # another entry point writes the cache: the batch has ended
    before = [c.copy() for c in _caches(ctx, cfg)]
    refused(-5, ctx.batch_admit, 2, good); refused(-5, ctx.batch_pass, 0)
    for a, b in zip(_caches(ctx, cfg), before):
        assert np.array_equal(a, b)
    tp = gpu.Ctx(gpu.desc_from_config(cfg, max_seq_len=MAX_SEQ), device=0, rank=0, world=1, comm_id=gpu.comm_unique_id())      # a sharded context refuses (-2)
    tp.upload_all(_model("tiny-int8")[1])
    tp.set_option("force_tp", 1)
    refused(-2, tp.batch_admit, 0, good); refused(-2, tp.batch_pass, 0)
    tp.close()


def test_cancel_ends_the_call_behind_its_pass(pair):
    """ "batch_rows" 0, a truthy return of the callback: it is not called again, the pass in flight counts for every slot, the states are behind the delivered ids"""
    name = "tiny-int8"
    cfg, ctx, ref = pair(name)
    reqs = _requests(cfg.vocab_size, [5, 2, 6, 1], 61, M=10)
    seen = []

    def on_token(j, i, tok, last):
        seen.append((j, i))
        return (j, i) == (1, 2)
    ctx.set_option("batch_rows", 0)
    try:
        got, st = ctx.generate_batch(reqs, on_token=on_token)
    finally:
        ctx.set_option("batch_rows", -1)
    assert seen == [(j, i) for i in range(2) for j in range(4)] + [(0, 2), (1, 2)]
    for j, q in enumerate(reqs):
        w, sw = _alone(ref, name, q, 3)
        assert np.array_equal(got[j], w) and st[j] == sw, j
    assert ctx.query("stop_reason") == capi.STOP_CANCEL


def test_a_retried_pass_delivers_every_id_once(gpu):
    """a cross-workgroup wait that gave up (injected) is noticed behind a pass: the pass re-runs from what the host holds -- the chunk's ids uploaded again, the same
    ids and states, nothing twice.  Injected in front of a pass that carries a step row, a chunk that completes its prompt and another prompt's first row"""
    name = "tiny-int8"
    cfg, tensors = _model(name)
    ref = _ctx(gpu, cfg, tensors); ctx = _ctx(gpu, cfg, tensors)
    reqs = _requests(cfg.vocab_size, [3, 20, 9], 8, M=8)
    want = [_alone(ref, name, q) for q in reqs]
    ctx.batch_open(capi.batch_layout(_rows_of(reqs), MAX_SEQ))
    for s, q in enumerate(reqs):
        ctx.batch_admit(s, q)
    ids = [[] for _ in reqs]
    busy, p = 1, 0
    while busy:
        if p == 1:
            ctx.set_option("inject_wait_failure", 1)
        out, live, fin, filling = ctx.batch_pass(12)
        for s in range(3):
            if out[s] >= 0:
                ids[s].append(int(out[s]))
        busy = live | filling
        p += 1
    assert ctx.query("fallback") == 1
    for s in range(3):
        assert np.array_equal(ids[s], want[s][0]) and ctx.batch_state(s)[:2] == (want[s][1], 8)
    ctx.batch_close()
    ref.close(); ctx.close()


def test_nothing_is_allocated_inside_the_calls(gpu):
    """the first open / admit / pass / close of a fresh context, bracketed with hipMemGetInfo"""
    hip = ctypes.CDLL("libamdhip64.so")

    def free_bytes():
        f, t = ctypes.c_size_t(0), ctypes.c_size_t(0)
        assert hip.hipMemGetInfo(ctypes.byref(f), ctypes.byref(t)) == 0
        return f.value
    cfg, tensors = _model("tiny-int8")
    ctx = _ctx(gpu, cfg, tensors)
    ctx.prepare()
    V = cfg.vocab_size
    f0 = free_bytes()
    ctx.batch_open(capi.batch_layout([20, 60, 70], MAX_SEQ))
    ctx.batch_admit(0, Req(_prompt(V, 3), 6, 1.0, 0.9, rng_state=1))
    ctx.batch_admit(2, Req(_prompt(V, 40), 6, 0.0, 0.9))
    for _ in range(3):
        ctx.batch_pass(16)
    ctx.batch_admit(1, Req(_prompt(V, 30), 6, 0.7, 0.5, rng_state=2))
    busy = 1
    while busy:
        _, live, _, filling = ctx.batch_pass(0)
        busy = live | filling
    ctx.batch_close(2)
    assert free_bytes() == f0
    ctx.close()
