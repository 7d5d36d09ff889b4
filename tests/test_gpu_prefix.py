"""Cache slots behind a shared prefix (include/flm_gpu.h: flm_batch_open_prefix, flm_generate_batch_prefix, flm_op_attention_slots_prefix / _segs_prefix; kernels:
csrc/flm_prefix.h).  Everything is equality: ids with np.array_equal, sampler states as 64-bit integers, attention outputs and K/V rows on bit patterns.
Op level: every row against flm_op_attention on a CONTIGUOUS cache of its own -- the prefix rows followed by that row's own rows.  Every cache row that neither the prefix
nor that sequence owns holds NaN and the slots abut, so a read one row past a range lands in a neighbour.
Model level: every request against flm_generate(..., pos=S) on a SECOND context that was fed the same prefix.  max_seq_len is 256 throughout."""
import ctypes

import numpy as np
import pytest

import head_sizes
from fast_llama_amd import capi, flmfile as ff
from test_gpu_batch import HEADS, LENGTHS, Req, _alone, _requests, _weights, pair  # noqa: F401  (pair: the module's fixture)
from test_gpu_spec import MAX_SEQ, _caches, _ctx, _model, _prompt, bits

pytestmark = pytest.mark.gpu
EDGES = (1, 63, 64, 65, 130)               # S around the 64-row tile: one row, a tile less one, a whole tile, a tile and a row, three tiles
OWN = (0, 1, 63, 64)                       # a row's earlier own rows: its tail has 1, 2, 64, 65 rows -- some queries of a group have a second own tile, their neighbours none
SEG_N = (1, 7, 8, 9, 17)                   # a prompt segment's rows around the group of 8
SHAPES = [(1, 0), (8, 0), (9, 0), (16, 0), (1, 1), (2, 2), (0, 16)]      # (step rows, prompt segments behind them)


def _case(rng, hs, S, own, ns, n_step, live=None, q_scale=1.0):
    """the prefix in rows [0, S); behind it len(own) slots that ABUT, slot s with own[s] earlier rows and ns[s] rows for this pass; three rows nobody owns at the end.
    The pass's segments are the slots `live` (all by default); NaN in every row that is neither the prefix's nor a live slot's earlier row"""
    rows = [p + n for p, n in zip(own, ns)]
    base = [S + int(x) for x in np.concatenate([[0], np.cumsum(rows)[:-1]])]
    max_seq = base[-1] + rows[-1] + 3
    kc = np.full((HEADS, max_seq, hs), np.nan, np.float32); vc = np.full_like(kc, np.nan)
    live = list(range(len(own))) if live is None else live
    for b, p in [(0, S)] + [(base[s], own[s]) for s in live]:
        kc[:, b:b + p] = rng.standard_normal((HEADS, p, hs)); vc[:, b:b + p] = rng.standard_normal((HEADS, p, hs))
    B = sum(ns[s] for s in live)
    q = (rng.standard_normal((B, HEADS * hs)) * q_scale).astype(np.float32)
    k = rng.standard_normal((B, HEADS * hs)).astype(np.float32); v = rng.standard_normal((B, HEADS * hs)).astype(np.float32)
    pick = lambda a: [a[s] for s in live]
    return kc, vc, q, k, v, S, pick(base), pick(rows), pick(ns), pick(own), max_seq, n_step


def _check(gpu, hs, case, tag):
    kc, vc, q, k, v, S, base, rows, ns, own, max_seq, n_step = case
    kc0, vc0 = kc.copy(), vc.copy()
    pos0 = [S + p for p in own]
    if n_step == len(ns):
        out = gpu.op_attention_slots_prefix(kc, vc, q, k, v, HEADS, hs, max_seq, S, base, rows, pos0)
    else:
        out = gpu.op_attention_segs_prefix(kc, vc, q, k, v, HEADS, hs, max_seq, S, base, rows, ns, pos0, n_step=n_step)
    written = np.zeros(max_seq, bool)
    row = 0
    for s, (b, n, p) in enumerate(zip(base, ns, own)):
        T = S + p + n + 3                                                             # the sequence's own cache: the prefix, its p earlier rows, NaN behind
        kr = np.full((HEADS, T, hs), np.nan, np.float32); vr = np.full_like(kr, np.nan)
        kr[:, :S] = kc0[:, :S]; vr[:, :S] = vc0[:, :S]
        kr[:, S:S + p] = kc0[:, b:b + p]; vr[:, S:S + p] = vc0[:, b:b + p]
        for i in range(n):
            want = gpu.op_attention(kr, vr, q[row], k[row], v[row], HEADS, hs, T, S + p + i)
            assert np.array_equal(bits(out[row]), bits(want)), (tag, hs, "S", S, "segment", s, "row", i, "own", p, "n", n)
            row += 1
        assert np.array_equal(bits(kc[:, b + p:b + p + n]), bits(kr[:, S + p:S + p + n])) and np.array_equal(bits(vc[:, b + p:b + p + n]), bits(vr[:, S + p:S + p + n])), (tag, "K/V rows", s)
        written[b + p:b + p + n] = True
    assert np.array_equal(bits(kc[:, ~written]), bits(kc0[:, ~written])) and np.array_equal(bits(vc[:, ~written]), bits(vc0[:, ~written])), (tag, "a row nobody wrote has changed")


@pytest.mark.parametrize("n_step,n_segs", SHAPES)
@pytest.mark.parametrize("S", EDGES)
@pytest.mark.parametrize("hs", [64, 128, 40])
def test_every_row_is_the_contiguous_attention(gpu, hs, S, n_step, n_segs):
    """step rows alone (n = 1, 8, 9, 16: the edges of a group) with tails of 1 / 2 / 64 / 65 rows mixed within every group; 1, 2 and 16 prompt segments behind step rows,
    segment s with SEG_N[s % 5] rows behind OWN[(s + rot) % 4] rows of its own: over the rotations every length meets every offset"""
    rng = np.random.default_rng(1000 * hs + 10 * S + n_step + n_segs)
    for rot in range(2 if n_segs in (0, 16) else 4):
        first = rot if n_segs < 16 else 0
        ns = [1] * n_step + [SEG_N[(first + s) % 5] for s in range(n_segs)]
        own = [OWN[(s + rot) % 4] for s in range(n_step)] + [OWN[(first + s + rot) % 4] for s in range(n_segs)]
        _check(gpu, hs, _case(rng, hs, S, own, ns, n_step), (n_step, n_segs, rot))


@pytest.mark.parametrize("hs", [64, 128])
def test_step_rows_peaked_and_a_subset_of_the_slots(gpu, hs):
    """a peaked softmax -- weights under the 1e-15 skip threshold next to weights that count, asserted in NumPy first -- and the live rows a non-contiguous subset of the
    slots: the slots between them hold NaN"""
    S, own, live = 65, [64, 1, 63, 0, 64, 64, 1, 63, 64, 0, 64], [1, 2, 4, 5, 7, 8, 10]
    case = _case(np.random.default_rng(77 + hs), hs, S, own, [1] * len(own), len(live), live=live, q_scale=30.0)
    kc, vc, q, k, v, _, base = case[:7]
    for r in (1, 2):                                                                  # (own 63 and 64: a long enough row)
        kr = np.concatenate([kc[:, :S], kc[:, base[r]:base[r] + case[9][r]]], axis=1)
        for w in _weights(kr, q[r], k[r], hs, kr.shape[1]):
            assert (w[1:] < 1e-17).sum() > 5 and (w > 1e-6).sum() >= 1, "the case is not peaked enough"
    _check(gpu, hs, case, "peaked subset")


def test_ops_refuse_what_they_do_not_do(gpu):
    kc, vc, q, k, v, S, base, rows, ns, own, max_seq, _ = _case(np.random.default_rng(3), 64, 5, [3, 5], [4, 2], 0)
    p = lambda a: np.ascontiguousarray(a, np.int32 if not isinstance(a, np.ndarray) else a.dtype).ctypes.data_as(ctypes.c_void_p)
    out, pos0, k0, v0 = np.empty_like(q), [S + x for x in own], kc.copy(), vc.copy()
    segs = lambda S, B, b, rw, n, ps, hs=64, n_step=0: gpu.lib().flm_op_attention_segs_prefix(p(out), p(kc), p(vc), p(q), p(k), p(v), HEADS, hs, max_seq, S, B, len(b), n_step, p(b), p(rw), p(n), p(ps))
    slots = lambda S, b, rw, ps, hs=64: gpu.lib().flm_op_attention_slots_prefix(p(out), p(kc), p(vc), p(q), p(k), p(v), HEADS, hs, max_seq, S, len(b), p(b), p(rw), p(ps))
    for hs in (256, 136):
        assert segs(S, 6, base, rows, ns, pos0, hs=hs) == -2 and slots(S, base, rows, pos0, hs=hs) == -2      # head sizes above 128
    assert segs(0, 6, base, rows, ns, pos0) == -1 and slots(-1, base, rows, pos0) == -1                      # no shared row
    assert segs(S, 6, [S - 1, base[1]], rows, ns, pos0) == -1 and slots(S, [S - 1, base[1]], rows, pos0) == -1      # a slot that begins inside the prefix
    assert segs(S, 6, base, rows, ns, [S - 1, pos0[1]]) == -1 and slots(S, base, rows, [S - 1, pos0[1]]) == -1      # a position in front of S
    assert segs(S, 6, base, [rows[0] - 1, rows[1]], ns, pos0) == -1 and slots(S, base, [own[0], rows[1]], pos0) == -1      # a row outside its slot
    assert segs(S, 6, [base[0], max_seq - 2], rows, ns, pos0) == -1 and segs(S, 7, base, rows, ns, pos0) == -1      # a slot outside the cache; rows that are not the segments' sum
    assert np.array_equal(bits(kc), bits(k0)) and np.array_equal(bits(vc), bits(v0))
    assert segs(S, 6, base, rows, ns, pos0) == 0                                                             # (the case itself is served)


# ---- model level ---------------------------------------------------------------------------------------------------------------------------------------------------
_fed, _ref = {}, {}


def _feed(c, S, V):
    """the shared rows: S tokens through the ordinary prompt path, at position 0 of an emptied cache"""
    c.reset_kv()
    c.forward(_prompt(V, S, seed=1000 + S), 0)
    _fed[id(c)] = S


def _behind(ref, cfg, name, S, q):
    """the request by flm_generate at pos = S on the reference context, whose rows [0, S) hold the prefix -> (ids, the state after, the K/V rows [S, ...) it left)"""
    key = (name, S, bytes(np.asarray(q.prompt, np.int32)), q.max_tokens, q.temperature, q.topp, q.rng_state, q.stop_token)
    if key not in _ref:
        if _fed.get(id(ref)) != S:
            _feed(ref, S, cfg.vocab_size)
        ids, st = ref.generate(q.prompt, S, q.max_tokens, temperature=q.temperature, topp=q.topp, rng_state=q.rng_state, stop_token=q.stop_token)
        _ref[key] = (ids, st if q.temperature != 0 else q.rng_state, [c[:, S:S + len(q.prompt) + len(ids) - 1].copy() for c in _caches(ref, cfg)])
    return _ref[key]


def _same(cfg, ref, name, S, reqs, got, states, tag, caches=None):
    """ids, states and (given the caches) every slot's K / V rows against the reference's rows [S, ...)"""
    lay = capi.batch_layout([len(q.prompt) + q.max_tokens - 1 for q in reqs], MAX_SEQ, prefix_rows=S)
    for j, q in enumerate(reqs):
        w, sw, theirs = _behind(ref, cfg, name, S, q)
        assert np.array_equal(got[j], w) and states[j] == sw, (tag, j, len(q.prompt), list(got[j]), list(w))
        for a, r in zip(caches or [], theirs):
            assert np.array_equal(a[:, lay.base[j]:lay.base[j] + r.shape[1]], r), (tag, j, "the slot's K/V rows")
    return lay


CALLS = [(5, [65]), (5, [65, 1, 64, 5, 63]), (70, [63, 2, 65, 4, 6]), (5, LENGTHS[16][0]), (70, [1, 2, 3, 4, 5, 6, 63, 1, 2, 3, 4, 5, 6, 1, 2, 3])]
ROUTES = ["stop", "skinny", "join+step", "pass-1", "pass-8", "pass-0", "rows-0", "rows-8"]
# the loop on three models at every call; the other routes on one model at n = 5, S = 5 and 70
CELLS = [(m, S, L, "loop") for m in ("tiny-int8", "tiny128-int8", "tiny-int16") for S, L in CALLS] + [("tiny-int8", S, L, r) for S, L in CALLS[1:3] for r in ROUTES]


@pytest.mark.parametrize("name,S,lengths,route", CELLS, ids=[f"{m}-S{S}-n{len(L)}-{r}" for m, S, L, r in CELLS])
def test_every_request_is_its_generate_at_pos_S(pair, name, S, lengths, route):
    """own prompts of 1 .. 6 and 63 .. 65 tokens within one call, greedy and two sampled settings mixed, differing max_tokens, two requests on one state.  Routes: the
    loop ("batch_rows" -1), with a stop token taken from the reference runs, and on the skinny GEMM; join + step; admit + pass at budgets 1, 8 and 0, the last request
    entering mid-flight behind two passes; the loop under "batch_rows" 0 and 8.  Ids, states, the slots' K / V rows, and the shared rows before and after"""
    cfg, ctx, ref = pair(name)
    n = len(lengths)
    reqs = _requests(cfg.vocab_size, lengths, 100 * n + S, M=3 if S + sum(lengths) + 6 * n > MAX_SEQ else None)
    if route == "stop":
        stop = int(_behind(ref, cfg, name, S, reqs[0])[0][1])                         # request 0 stops at its second id at the latest
        reqs = [Req(q.prompt, q.max_tokens, q.temperature, q.topp, q.rng_state, stop) for q in reqs]
    _feed(ctx, S, cfg.vocab_size)
    shared = [c[:, :S].copy() for c in _caches(ctx, cfg)]
    kind, _, arg = route.partition("-")
    if kind in ("loop", "stop", "skinny", "rows"):
        ctx.set_option("batch_rows", int(arg) if kind == "rows" else -1); ctx.set_option("spec_gemm", int(kind == "skinny"))
        try:
            got, st = ctx.generate_batch(reqs, prefix_rows=S)
        finally:
            ctx.set_option("batch_rows", -1); ctx.set_option("spec_gemm", 0)
    else:
        ctx.batch_open(capi.batch_layout([len(q.prompt) + q.max_tokens - 1 for q in reqs], MAX_SEQ, prefix_rows=S), prefix_rows=S)
        assert ctx.query("batch_prefix") == S
        got = [[ctx.batch_join(s, q)[0]] if kind == "join+step" else [] for s, q in enumerate(reqs)]
        for s in range(n - 1 if kind == "pass" else 0):
            ctx.batch_admit(s, reqs[s])
        passes, busy = 0, 1
        while busy:
            if kind == "pass" and passes == 2:
                ctx.batch_admit(n - 1, reqs[n - 1])                                   # enters mid-flight
            out, live, *rest = ctx.batch_pass(int(arg)) if kind == "pass" else ctx.batch_step()
            passes += 1
            for s in range(n):
                if out[s] >= 0:
                    got[s].append(int(out[s]))
            busy = live | (rest[1] if kind == "pass" else 0) | (kind == "pass" and passes < 3)
        st = [ctx.batch_state(s)[0] for s in range(n)]
    mine = _caches(ctx, cfg)
    ctx.batch_close()
    _same(cfg, ref, name, S, reqs, got, st, (name, S, route), mine)
    for a, b in zip(mine, shared):
        assert np.array_equal(a[:, :S], b), "the shared rows were written"


@pytest.mark.parametrize("keep", [0, 1, 2])
def test_close_keep_moves_the_slot_behind_the_prefix(pair, keep):
    """close(keep) for the first slot (in place), slot 1 with base - S = 8 < len (the overlapping move) and the last slot: rows [S, S + len) are the reference's, and one
    generate continues from S + len on both contexts"""
    name, S = "tiny-int8", 70
    cfg, ctx, ref = pair(name)
    V = cfg.vocab_size
    reqs = [Req(_prompt(V, 3, seed=1), 6, 1.0, 0.9, rng_state=5), Req(_prompt(V, 40, seed=2), 30, 1.0, 0.9, rng_state=6), Req(_prompt(V, 5, seed=3), 10, 0.0, 0.9, rng_state=7)]
    _feed(ctx, S, V)
    ctx.batch_open(capi.batch_layout([8, 100, 20], MAX_SEQ, prefix_rows=S), prefix_rows=S)
    ids = [[ctx.batch_join(s, q)[0]] for s, q in enumerate(reqs)]
    live = 7
    while live:
        out, live, _ = ctx.batch_step()
        for s in range(3):
            ids[s] += [int(out[s])] if out[s] >= 0 else []
    _fed.clear(); _ref.clear()                                                        # (the continuation below writes the reference's cache: feed and generate afresh)
    want, st, theirs = _behind(ref, cfg, name, S, reqs[keep])
    n = len(reqs[keep].prompt) + len(want) - 1
    assert np.array_equal(ids[keep], want) and (keep != 1 or 8 < n)
    ctx.batch_close(keep)
    for a, r in zip(_caches(ctx, cfg), theirs):
        assert np.array_equal(a[:, S:S + n], r[:, :n]), (keep, "the kept rows")
    nxt = np.array([int(want[-1])], np.int32)
    assert all(np.array_equal(a, b) for a, b in zip(ctx.generate(nxt, S + n, 8, temperature=1.0, topp=0.9, rng_state=st), ref.generate(nxt, S + n, 8, temperature=1.0, topp=0.9, rng_state=st)))
    _fed.clear(); _ref.clear()


def test_no_prefix_through_the_new_entry_points_is_the_plain_batch(pair):
    """S = 0: flm_generate_batch_prefix / flm_batch_open_prefix give what the plain calls give -- every request its own flm_generate on a fresh context"""
    name = "tiny-int8"
    cfg, ctx, ref = pair(name)
    reqs = _requests(cfg.vocab_size, LENGTHS[5][0], 41)
    want = [_alone(ref, name, q) for q in reqs]
    _fed.clear()                                                                      # (_alone empties the reference's cache)
    n, lib, vp = len(reqs), capi.lib(), lambda a: a.ctypes.data_as(ctypes.c_void_p)
    structs = [q.struct() for q in reqs]
    arr = (capi.BatchReqStruct * n)(*[s[0] for s in structs])
    out = np.full((n, 8), -1, np.int32); n_out = np.zeros(n, np.int32); st = np.zeros(n, np.uint64)
    ctx.reset_kv()
    assert lib.flm_generate_batch_prefix(ctx._h, 0, arr, n, None, None, vp(out), 8, vp(n_out), vp(st)) == 0
    assert all(np.array_equal(out[j, :n_out[j]], w) and int(st[j]) == sw for j, (w, sw) in enumerate(want))
    lay = capi.batch_layout([len(q.prompt) + q.max_tokens - 1 for q in reqs], MAX_SEQ)
    assert lib.flm_batch_open_prefix(ctx._h, ctypes.byref(lay), 0) == 0 and ctx.query("batch_prefix") == 0 and ctx.batch_join(0, reqs[0])[0] == want[0][0][0]
    ctx.batch_close()


def test_refusals_leave_the_cache_untouched(pair, gpu):
    name, S = "tiny-int8", 5
    cfg, ctx, ref = pair(name)
    V = cfg.vocab_size
    lay = lambda: capi.batch_layout([10, 10], MAX_SEQ, prefix_rows=S)
    _feed(ctx, S, V)
    ctx.batch_open(lay(), prefix_rows=S)
    ctx.batch_join(0, Req(_prompt(V, 6, seed=1), 5, 1.0, 0.9, rng_state=3))
    before = [c.copy() for c in _caches(ctx, cfg)]

    def refused(code, fn, *a, **kw):
        with pytest.raises(capi.FlmError, match=f"flm error {code}:"):
            fn(*a, **kw)
    refused(-1, ctx.batch_open, capi.batch_layout([10, 10], MAX_SEQ), prefix_rows=S); refused(-1, ctx.batch_open, lay(), prefix_rows=S + 1)      # base[0] != S
    refused(-1, ctx.batch_open, lay(), prefix_rows=-1)                                            # S < 0
    refused(-1, ctx.batch_open, capi.batch_layout([200, 100], 512, prefix_rows=S), prefix_rows=S)      # does not fit behind S
    refused(-1, ctx.generate_batch, [Req(_prompt(V, 100), 60), Req(_prompt(V, 90), 4)], prefix_rows=S)      # 5 + 159 + 93 = 257 rows
    refused(-1, ctx.batch_join, 1, Req(_prompt(V, 6), 6))                                         # 11 rows into a slot of 10
    assert all(np.array_equal(a, b) for a, b in zip(_caches(ctx, cfg), before))
    assert ctx.query("batch_prefix") == S and ctx.batch_state(0)[1] == 1 and ctx.batch_join(1, Req(_prompt(V, 6), 5))[1]      # the open batch is as it was; the exact fit
    ctx.batch_close()
    got, _ = ctx.generate_batch([Req(_prompt(V, 100), 60), Req(_prompt(V, 90), 3)], prefix_rows=S)      # 256: the exact fit
    assert [len(g) for g in got] == [60, 3]
    # head sizes above 128 and a sharded context: -2, with nothing touched
    cfg2, tensors2 = head_sizes.model(256, ff.QT_INT8)
    wide = _ctx(gpu, cfg2, tensors2)
    wide.forward(_prompt(cfg2.vocab_size, S), 0)
    before = [c.copy() for c in _caches(wide, cfg2)]
    refused(-2, wide.batch_open, lay(), prefix_rows=S); refused(-2, wide.generate_batch, [Req(_prompt(cfg2.vocab_size, 6), 5)], prefix_rows=S)
    assert all(np.array_equal(a, b) for a, b in zip(_caches(wide, cfg2), before))
    wide.close()
    tp = gpu.Ctx(gpu.desc_from_config(cfg, max_seq_len=MAX_SEQ), device=0, rank=0, world=1, comm_id=gpu.comm_unique_id())
    tp.upload_all(_model(name)[1])
    tp.set_option("force_tp", 1)
    refused(-2, tp.generate_batch, [Req(_prompt(V, 6), 5)], prefix_rows=S); refused(-2, tp.batch_open, lay(), prefix_rows=S)
    tp.close()


def test_nothing_is_allocated_inside_the_calls(gpu):
    """the first open / join / admit / pass / step / close of a fresh context behind a prefix, bracketed with hipMemGetInfo"""
    hip = ctypes.CDLL("libamdhip64.so")

    def free_bytes():
        f, t = ctypes.c_size_t(0), ctypes.c_size_t(0)
        assert hip.hipMemGetInfo(ctypes.byref(f), ctypes.byref(t)) == 0
        return f.value
    cfg, tensors = _model("tiny-int8")
    ctx = _ctx(gpu, cfg, tensors)
    ctx.prepare()
    V, S = cfg.vocab_size, 70
    ctx.forward(_prompt(V, S), 0)
    f0 = free_bytes()
    ctx.batch_open(capi.batch_layout([20, 60, 70], MAX_SEQ, prefix_rows=S), prefix_rows=S)
    ctx.batch_join(0, Req(_prompt(V, 3), 6, 1.0, 0.9, rng_state=1))
    ctx.batch_admit(2, Req(_prompt(V, 40), 6, 0.0, 0.9))
    for _ in range(3):
        ctx.batch_pass(16)
    ctx.batch_join(1, Req(_prompt(V, 30), 6, 0.7, 0.5, rng_state=2))
    live = 1
    while live:
        _, live, _ = ctx.batch_step()
    ctx.batch_close(2)
    assert free_bytes() == f0
    ctx.close()
