"""Per-token log-probabilities from the device loop (include/flm_gpu.h: flm_logprobs_arm, flm_last_logprobs, flm_op_logprob_rows; the stage: csrc/flm_logprob.h).

Op level: k_logprob_rows equals fh_logprob_row on the bit patterns.  Model level ("tiny" int8 / int16, MAX_SEQ 256; one case on the 2-layer 7B shape): an armed
flm_generate_ex changes no result and its records equal fh_logprob_row on the rows of the host loop (flm_forward's logits, the NumPy mask, fh_shape, fh_sample_state);
flm_forward_sample_ex, flm_verify_sample_ex and flm_generate_lookup_ex leave the same records.  Every comparison is exact: bit patterns for floats, no tolerance."""
import ctypes as C

import numpy as np
import pytest

from constraint_util import Dfa, cycle3, pairs
from logprob_util import diff_records, expected_records, host_logprob, host_loop_rows, same_records
from sample_util import host_lib, logits_case
from score_util import teeth_row
from shape_util import KINDS, Sampling
from test_gpu_constraint import MAX_SEQ, SETTINGS, _ctx, _prompt
from test_gpu_shape import CONTROLS

pytestmark = pytest.mark.gpu
SIZES = (2, 63, 64, 65, 1000, 4099, 32000, 32768)
TOPS = (0, 1, 5, 20)
SOURCES = ("raw", "shaped")


@pytest.fixture(scope="module")
def ctxs(gpu):
    made = {}

    def get(name):
        if name not in made:
            made[name] = _ctx(gpu, name)
        return made[name]
    yield get
    for _, c in made.values():
        c.close()


def _same(got, want, what=""):
    assert same_records(got, want), (what, diff_records(got, want))


# ---- op level ----------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_op_logprob_rows_equals_the_host(gpu, n):
    rng = np.random.default_rng(n)
    ld = n + 5
    L = np.full((16, ld), np.nan, np.float32)                       # NaN poison in the padding: it changes nothing
    for r in range(16):
        L[r, :n] = logits_case(KINDS[r % len(KINDS)], n, seed=100 * n + r)
    chosen = rng.integers(0, n, 16).astype(np.int32)
    for top_n in TOPS:
        got = gpu.op_logprob_rows(L, n, chosen, top_n)
        _same(got, host_logprob(L[:, :n], chosen, top_n), (n, top_n))
    one = gpu.op_logprob_rows(L[3:4], n, chosen[3:4], 5)             # rows = 1
    _same(one, host_logprob(L[3:4, :n], chosen[3:4], 5), (n, "one row"))


def test_op_teeth_a_tree_ordered_sum_would_show(gpu):
    L = np.stack([teeth_row(t) for t in range(8)])
    chosen = np.arange(8, dtype=np.int32) * 17
    _same(gpu.op_logprob_rows(L, L.shape[1], chosen, 5), host_logprob(L, chosen, 5))


def test_op_fewer_finite_entries_than_top_n(gpu):
    for n, top_n in ((4099, 5), (1000, 20), (70, 20)):
        x = np.full(n, -np.inf, np.float32)
        fin = np.random.default_rng(n).permutation(n)[:top_n - 1]
        x[fin] = np.random.default_rng(n + 1).standard_normal(top_n - 1).astype(np.float32)
        got = gpu.op_logprob_rows(x, n, [int(fin[0])], top_n)
        _same(got, host_logprob(x, [int(fin[0])], top_n), (n, top_n))
        assert sorted(got["top_id"][0, :top_n - 1].tolist()) == sorted(fin.tolist()) and np.isneginf(got["top_logit"][0, top_n - 1])
        assert int(got["top_id"][0, top_n - 1]) == min(set(range(n)) - set(fin.tolist()))      # the -inf entries by index


def test_op_threshold_ties_straddle_a_wave_boundary(gpu):
    n = 4099
    for idxs, top_n in (((63, 64, 65), 2), ((63, 64, 65), 3), ((1023, 1024), 1), ((1023, 1024), 2), ((63, 64, 65, 1023, 1024), 4), ((63, 64, 65, 1023, 1024), 20)):
        x = (np.random.default_rng(5).standard_normal(n) - 10).astype(np.float32)
        x[list(idxs)] = np.float32(3.5)
        x[2000] = np.float32(9.0)                                   # one entry above the tie, except where top_n is 1
        if top_n == 1:
            x[2000] = np.float32(-20.0)
        got = gpu.op_logprob_rows(x, n, [7], top_n)
        _same(got, host_logprob(x, [7], top_n), (idxs, top_n))
        head = [2000] if top_n > 1 else []
        k = min(top_n, len(head) + len(idxs))
        assert got["top_id"][0, :k].tolist() == (head + list(idxs))[:k]


def test_teeth_chosen_is_not_the_argmax_and_index_0_ties_for_second(gpu):
    n = 1000
    L = np.stack([logits_case("medium", n, seed=r) for r in range(16)])
    chosen = np.array([(int(np.argmax(L[r])) + 1 + r) % n for r in range(16)], np.int32)
    got = gpu.op_logprob_rows(L, n, chosen, 5)
    _same(got, host_logprob(L, chosen, 5))
    assert (got["token"] == chosen).all() and (got["top_id"][:, 0] != chosen).all()
    assert all(got["logit"][r] == L[r, chosen[r]] and got["logit"][r] < got["max_logit"][r] for r in range(16))
    x = np.full(n, -5.0, np.float32)
    x[[0, 400, 700]] = [2.0, 6.0, 2.0]                              # index 0 ties for second: the first place is not index 0
    got = gpu.op_logprob_rows(x, n, [700], 3)
    _same(got, host_logprob(x, [700], 3))
    assert got["top_id"][0, :3].tolist() == [400, 0, 700]


def test_op_errors(gpu):
    x = np.zeros((2, 8), np.float32)
    for args in ((x, 8, [0, 8], 5), (x, 8, [0, 1], 21), (x, 8, [0, 1], -1), (x, 9, [0, 1], 5), (x[:, :1], 1, [0, 0], 1)):
        with pytest.raises(gpu.FlmError, match="flm error -1"):
            gpu.op_logprob_rows(*args)


# ---- the token form ------------------------------------------------------------------------------------------------------------------------------------------------
_loops = {}


def _loop(ctx, name, prompt, n, s, seed, dfa=None, q0=0, stop=-1, tag=""):
    """the host loop's (ids, sampler state, raw rows, shaped rows), computed once per case and left unchanged"""
    key = (name, len(prompt), n, repr(s), seed, tag, q0, stop)
    if key not in _loops:
        _loops[key] = host_loop_rows(ctx, host_lib(), prompt, n, s, seed, dfa, q0, stop=stop)
    return _loops[key]


@pytest.mark.parametrize("source", SOURCES)
@pytest.mark.parametrize("which", list(SETTINGS))
@pytest.mark.parametrize("name", ["tiny", "tiny16"])
def test_generate_ex_armed_equals_the_host_loop(gpu, ctxs, name, which, source):
    cfg, ctx = ctxs(name)
    t, p, ctl = SETTINGS[which]
    s = Sampling(temperature=t, topp=p, **ctl)
    prompt, seed, N = _prompt(cfg.vocab_size, 12), 77, 24
    ids, sref, raw, shaped = _loop(ctx, name, prompt, N, s, seed)
    ctx.constraint_set(None)
    ctx.logprobs_arm(-1)
    ctx.reset_kv(); base, sbase = ctx.generate_ex(prompt, 0, N, s, rng_state=seed)
    kv = ctx.debug_read("kcache", 0, 4096)
    ctx.logprobs_arm(5, source)
    assert ctx.query("logprobs_top_n") == 5
    n0 = ctx.query("shaped_tokens")
    seen = []
    ctx.reset_kv(); got, st = ctx.generate_ex(prompt, 0, N, s, rng_state=seed, on_token=lambda i, tok, last: seen.append((i, tok, last)) and None)
    assert list(got) == list(base) == ids and st == sbase == sref and len(got) == N
    assert seen == [(i, ids[i], i == N - 1) for i in range(N)]
    assert np.array_equal(ctx.debug_read("kcache", 0, 4096).view(np.uint32), kv.view(np.uint32))
    assert ctx.query("shaped_tokens") == n0 + N and ctx.query("fallback") == 0      # an armed context counts as a control that is set
    _same(ctx.last_logprobs(), expected_records(ids, raw, shaped, source, 5), (name, which, source))
    _same(ctx.last_logprobs(3, 4), expected_records(ids, raw, shaped, source, 5)[3:7])
    if not ctl:
        assert np.array_equal(raw.view(np.uint32), shaped.view(np.uint32))          # neutral controls: S is L bit for bit
    ctx.logprobs_arm(-1)


def test_records_agree_with_the_merged_scorer(gpu, ctxs):
    cfg, ctx = ctxs("tiny")
    prompt, N = _prompt(cfg.vocab_size, 12), 16
    for t, seed in ((0.0, 0), (1.0, 9)):
        ctx.logprobs_arm(3, "raw")
        ctx.reset_kv(); ids, _ = ctx.generate_ex(prompt, 0, N, Sampling(temperature=t, topp=0.9), rng_state=seed)
        rec = ctx.last_logprobs()
        ctx.reset_kv()
        seq = np.concatenate([prompt, ids]).astype(np.int32)
        sc = ctx.score(seq, 0)
        rows = sc[len(prompt) - 1:len(prompt) - 1 + N]
        for a, b in (("max_logit", "max_logit"), ("sum", "sum"), ("logit", "target_logit")):
            assert np.array_equal(rec[a].view(np.uint32), rows[b].view(np.uint32)), (t, a)
        assert np.array_equal(rec["top_id"][:, 0], rows["argmax"])
    ctx.logprobs_arm(-1)


def test_constraint_armed(gpu, ctxs):
    cfg, ctx = ctxs("tiny")
    V = cfg.vocab_size
    prompt = _prompt(V, 12)
    ctx.constraint_set(None); ctx.logprobs_arm(-1)
    ctx.reset_kv(); plain, _ = ctx.generate_ex(prompt, 0, 16, Sampling(temperature=0.0))
    q0 = (int(plain[0]) + 1) % 3                                       # cycle3 state q0 bans plain[0]
    dfa = cycle3(V)
    s = Sampling(temperature=1.0, topp=0.9, **CONTROLS)
    ids, sref, raw, shaped = _loop(ctx, "tiny", prompt, 16, s, 5, dfa, q0, tag="cycle3")
    for source in SOURCES:
        ctx.constraint_set(dfa); ctx.constraint_arm(q0)
        ctx.logprobs_arm(20, source)
        ctx.reset_kv(); got, st = ctx.generate_ex(prompt, 0, 16, s, rng_state=5)
        assert list(got) == ids and st == sref and ctx.query("constraint_state") == (q0 + 16) % 3
        rec = ctx.last_logprobs()
        _same(rec, expected_records(ids, raw, shaped, source, 20), source)
        if source == "shaped":
            for i in range(16):
                fin = np.isfinite(rec["top_logit"][i, :rec["n_top"][i]])
                assert fin.any() and all(int(x) % 3 == (q0 + i) % 3 for x in rec["top_id"][i, :rec["n_top"][i]][fin])     # an edge in the token's state
        else:
            assert int(rec["top_id"][0, 0]) == int(plain[0]) != int(rec["token"][0])      # the unconstrained argmax, which the automaton bans
    ctx.constraint_set(None); ctx.logprobs_arm(-1)


def test_stop_and_cancel(gpu, ctxs):
    cfg, ctx = ctxs("tiny")
    V, stop = cfg.vocab_size, 2
    prompt = _prompt(V, 12)
    s = Sampling(temperature=1.0, topp=0.9)
    ctx.constraint_set(None)
    ctx.logprobs_arm(5, "shaped")
    # a longer earlier call fills the slots
    ctx.reset_kv(); ctx.generate_ex(prompt, 0, 12, s, rng_state=3)
    earlier = ctx.logprob_records_raw(12).copy()
    _same(earlier, ctx.last_logprobs())
    # the `ends` automaton shifted by one free step: the stop id is delivered at index 4
    tr = [(0, t, 1) for t in range(V)] + [(q + 1, t, q + 2) for q in range(3) for t in range(q, V, 3)] + [(4, stop, 4)]
    dfa = Dfa.from_edges(5, tr)
    ids, sref, raw, shaped = _loop(ctx, "tiny", prompt, 12, s, 5, dfa, 0, stop=stop, tag="ends+1")
    assert len(ids) == 5 and ids[4] == stop
    ctx.constraint_set(dfa); ctx.constraint_arm(0)
    ctx.reset_kv(); got, st = ctx.generate_ex(prompt, 0, 12, s, rng_state=5, stop_token=stop)
    assert list(got) == ids and st == sref and len(got) == 5
    want = expected_records(ids, raw, shaped, "shaped", 5)
    _same(ctx.last_logprobs(), want)
    _same(ctx.last_logprobs(4, 1), want[4:5])                         # the stop token's own record
    with pytest.raises(gpu.FlmError, match="flm error -1"):
        ctx.last_logprobs(5, 1)
    with pytest.raises(gpu.FlmError, match="flm error -1"):
        ctx.last_logprobs(0, 6)
    now = ctx.logprob_records_raw(12)
    _same(now[:5], want)
    assert now[5:].tobytes() == earlier[5:].tobytes()                 # the launches queued behind the stop wrote nothing
    ctx.constraint_set(None)
    # a callback that cancels at index 3: the records [0, n_out) are the host loop's
    ids, _, raw, shaped = _loop(ctx, "tiny", prompt, 24, s, 11)
    ctx.reset_kv(); got, _ = ctx.generate_ex(prompt, 0, 24, s, rng_state=11, on_token=lambda i, tok, last: i == 3)
    n = len(got)
    assert 4 <= n <= 24 and list(got) == ids[:n]
    _same(ctx.last_logprobs(), expected_records(ids[:n], raw[:n], shaped[:n], "shaped", 5))
    ctx.logprobs_arm(-1)


# ---- the other entry points ----------------------------------------------------------------------------------------------------------------------------------------
def _fs_loop(ctx, first, pos, n, s, window, s0):
    """a caller's own loop of flm_forward_sample_ex calls behind `first` at pos, the window slid over the ids -> (ids, the record each call left)"""
    hist, ids, state, tok, recs = [int(x) for x in window], [], s0, int(first), []
    for i in range(n):
        w = hist[len(hist) - min(s.penalty_last_n, len(hist)):] if s.penalty_last_n > 0 else []
        tok, state = ctx.forward_sample_ex(np.array([tok], np.int32), pos + i, s, w, rng_state=state)
        ids.append(tok); hist.append(tok); recs.append(ctx.last_logprobs())
        assert recs[-1].shape == (1,)
    return ids, np.concatenate(recs)


@pytest.mark.parametrize("source", SOURCES)
def test_forward_sample_ex_in_a_callers_loop(gpu, ctxs, source):
    cfg, ctx = ctxs("tiny")
    s = Sampling(temperature=1.0, topp=0.9, **CONTROLS)
    prompt = _prompt(cfg.vocab_size, 12)
    ids, sref, raw, shaped = _loop(ctx, "tiny", prompt, 24, s, 77)
    ctx.constraint_set(None)
    ctx.logprobs_arm(5, source)
    ctx.reset_kv()
    hist, state, got, recs = [int(x) for x in prompt], 77, [], []
    feed, pos = prompt, 0
    for i in range(8):
        w = hist[len(hist) - min(s.penalty_last_n, len(hist)):]
        tok, state = ctx.forward_sample_ex(feed, pos, s, w, rng_state=state)
        got.append(tok); hist.append(tok); recs.append(ctx.last_logprobs())
        pos += len(feed); feed = np.array([tok], np.int32)
    assert got == ids[:8]
    _same(np.concatenate(recs), expected_records(ids[:8], raw[:8], shaped[:8], source, 5))
    ctx.logprobs_arm(-1)


@pytest.mark.parametrize("source", SOURCES)
@pytest.mark.parametrize("k", [4, 15])
@pytest.mark.parametrize("which", ["t0", "t1 controls"])
def test_verify_sample_ex_leaves_the_callers_loops_records(gpu, ctxs, which, k, source):
    cfg, ctx = ctxs("tiny")
    V = cfg.vocab_size
    t, p, ctl = SETTINGS[which]
    s = Sampling(temperature=t, topp=p, **ctl)
    s0, pos = 4321, 7
    prompt = _prompt(V, pos)
    window = [int(x) for x in prompt[-min(s.penalty_last_n, pos):]] if s.penalty_last_n else []
    ctx.constraint_set(None)
    ctx.logprobs_arm(5, source)
    ctx.reset_kv(); ctx.forward(prompt, 0)
    ids, recs = _fs_loop(ctx, 5, pos, k + 1, s, window, s0)
    for wrong in (None, 0, k // 2, k - 1):                             # every draft right; a cut at the first row, inside the batch, at the last row
        drafts = np.array(ids[:k], np.int32)
        if wrong is not None:
            drafts[wrong] = (ids[wrong] + 3) % V
        m = k if wrong is None else wrong
        ctx.reset_kv(); ctx.forward(prompt, 0)
        got, _ = ctx.verify_sample_ex(5, drafts, pos, s, window, s0)
        assert [int(x) for x in got] == ids[:m + 1]
        _same(ctx.last_logprobs(), recs[:m + 1], (which, k, source, wrong))
        with pytest.raises(gpu.FlmError, match="flm error -1"):
            ctx.last_logprobs(m + 1, 1)
    ctx.logprobs_arm(-1)


@pytest.mark.parametrize("source", SOURCES)
@pytest.mark.parametrize("K", [4, 15])
@pytest.mark.parametrize("which", ["t0", "t1 controls"])
def test_generate_lookup_ex_leaves_generate_exs_records(gpu, ctxs, which, K, source):
    cfg, ctx = ctxs("tiny")
    V = cfg.vocab_size
    t, p, ctl = SETTINGS[which]
    s = Sampling(temperature=t, topp=p, **ctl)
    periodic = np.array([1] + [int(x) for x in ((np.arange(1, 25) % 6) * 7919 + 11) % V], np.int32)      # a period of 6: steps accept more than one id
    ctx.logprobs_arm(5, source)
    for dfa, q0, prompt, N, pos in ((pairs(V), 0, _prompt(V, 12), 40, 0),            # two ids per state: long accepted runs, cuts inside a batch
                                    (None, 0, periodic, 32, 0),
                                    (pairs(V), 0, _prompt(V, 12), 30, MAX_SEQ - 12 - 30 + 1)):     # the tail reaches max_seq_len: single-token steps
        def arm():
            ctx.reset_kv(); ctx.constraint_set(dfa)
            if dfa is not None:
                ctx.constraint_arm(q0)
        arm()
        want, sa = ctx.generate_ex(prompt, pos, N, s, rng_state=99)
        want_rec = ctx.last_logprobs().copy()
        arm()
        got, sb = ctx.generate_lookup_ex(prompt, pos, N, s, rng_state=99, draft_len=K, ngram_max=3)
        assert np.array_equal(got, want) and sa == sb and len(got) == N
        _same(ctx.last_logprobs(), want_rec, (which, K, source, pos))
        if dfa is not None and pos == 0:
            assert ctx.query("spec_accepted") > 0                     # some step delivered more than one id
    ctx.constraint_set(None); ctx.logprobs_arm(-1)


# ---- the call surface ------------------------------------------------------------------------------------------------------------------------------------------------
def test_disarmed_and_plain_calls_are_todays(gpu, ctxs):
    cfg, ctx = ctxs("tiny")
    prompt = _prompt(cfg.vocab_size, 12)
    neutral = Sampling(temperature=1.0, topp=0.9)
    ctx.constraint_set(None); ctx.logprobs_arm(-1)
    assert ctx.query("logprobs_top_n") == -1
    ctx.reset_kv(); base = ctx.generate(prompt, 0, 24, temperature=1.0, topp=0.9, rng_state=7)
    n0 = ctx.query("shaped_tokens")
    ctx.reset_kv(); got = ctx.generate_ex(prompt, 0, 24, neutral, rng_state=7)
    assert list(got[0]) == list(base[0]) and got[1] == base[1] and ctx.query("shaped_tokens") == n0       # disarmed, neutral: the plain form
    with pytest.raises(gpu.FlmError, match="flm error -5"):
        ctx.last_logprobs(0, 1)
    # armed: the plain entry points ignore it, the _ex one counts as shaped and draws the same ids
    ctx.logprobs_arm(0)
    ctx.reset_kv(); got = ctx.generate(prompt, 0, 24, temperature=1.0, topp=0.9, rng_state=7)
    assert list(got[0]) == list(base[0]) and got[1] == base[1] and ctx.query("shaped_tokens") == n0
    with pytest.raises(gpu.FlmError, match="flm error -5"):
        ctx.last_logprobs(0, 1)
    ctx.reset_kv(); got = ctx.generate_ex(prompt, 0, 24, neutral, rng_state=7)
    assert list(got[0]) == list(base[0]) and got[1] == base[1] and ctx.query("shaped_tokens") == n0 + 24
    rec = ctx.last_logprobs()
    assert rec.shape == (24,) and (rec["n_top"] == 0).all() and not rec["top_id"].any() and list(rec["token"]) == list(base[0])
    # disarmed again: a call that ran disarmed leaves no records to read
    ctx.logprobs_arm(-1)
    ctx.reset_kv(); ctx.generate_ex(prompt, 0, 8, neutral, rng_state=7)
    with pytest.raises(gpu.FlmError, match="flm error -5"):
        ctx.last_logprobs(0, 1)


def test_errors_launch_nothing(gpu, ctxs):
    cfg, ctx = ctxs("tiny")
    prompt = _prompt(cfg.vocab_size, 12)
    ctx.constraint_set(None)
    ctx.logprobs_arm(5, "raw")
    for top_n, source in ((21, 0), (-2, 0), (5, 2), (5, -1)):
        with pytest.raises(gpu.FlmError, match="flm error -1"):
            ctx.logprobs_arm(top_n, source)
    assert ctx.query("logprobs_top_n") == 5
    ctx.reset_kv(); ctx.generate_ex(prompt, 0, 6, Sampling(temperature=0.0))
    before = ctx.logprob_records_raw(8).copy()
    n0 = ctx.query("shaped_tokens")
    with pytest.raises(gpu.FlmError, match="flm error -1"):
        ctx.generate_ex(_prompt(cfg.vocab_size, 5), 0, MAX_SEQ, Sampling(temperature=0.0))      # past max_seq_len
    with pytest.raises(gpu.FlmError, match="flm error -5"):
        ctx.last_logprobs(0, 1)                                        # the last _ex call failed
    assert ctx.logprob_records_raw(8).tobytes() == before.tobytes() and ctx.query("shaped_tokens") == n0
    ctx.logprobs_arm(-1)
    fresh = gpu.Ctx(gpu.desc_from_config(cfg, max_seq_len=MAX_SEQ))
    with pytest.raises(gpu.FlmError, match="flm error -5"):
        fresh.logprobs_arm(5)                                          # before the model is complete
    fresh.close()
    tp = gpu.Ctx(gpu.desc_from_config(cfg, max_seq_len=MAX_SEQ), device=0, rank=0, world=1, comm_id=gpu.comm_unique_id())
    tp.set_option("force_tp", 1)
    with pytest.raises(gpu.FlmError, match="flm error -2"):
        tp.logprobs_arm(5)                                             # a sharded context
    tp.close()


def test_rearming_needs_no_prepare_and_prepare_keeps_the_setting(gpu, ctxs):
    cfg, ctx = ctxs("tiny")
    s = Sampling(temperature=1.0, topp=0.9, **CONTROLS)
    prompt = _prompt(cfg.vocab_size, 12)
    ids, _, raw, shaped = _loop(ctx, "tiny", prompt, 24, s, 77)
    ctx.constraint_set(None)
    for top_n, source in ((1, "raw"), (20, "shaped"), (0, "raw"), (7, "shaped")):
        ctx.logprobs_arm(top_n, source)
        ctx.reset_kv(); got, _ = ctx.generate_ex(prompt, 0, 10, s, rng_state=77)
        assert list(got) == ids[:10]
        _same(ctx.last_logprobs(), expected_records(ids[:10], raw[:10], shaped[:10], source, top_n), (top_n, source))
    ctx.set_option("graph_chunks", 0); ctx.prepare()
    assert ctx.query("logprobs_top_n") == 7
    ctx.reset_kv(); got, _ = ctx.generate_ex(prompt, 0, 10, s, rng_state=77)
    assert list(got) == ids[:10]
    _same(ctx.last_logprobs(), expected_records(ids[:10], raw[:10], shaped[:10], "shaped", 7))
    ctx.set_option("graph_chunks", 1); ctx.prepare()
    ctx.logprobs_arm(-1)


def test_nothing_is_allocated_in_the_steady_path(gpu, ctxs):
    """one warm armed flm_generate_ex, then arming, a second call and the read-back bracketed with hipMemGetInfo, in process"""
    cfg, ctx = ctxs("tiny")
    hip = C.CDLL("libamdhip64.so")

    def free_bytes():
        f, t = C.c_size_t(0), C.c_size_t(0)
        assert hip.hipMemGetInfo(C.byref(f), C.byref(t)) == 0
        return f.value
    prompt = _prompt(cfg.vocab_size, 12)
    s = Sampling(temperature=1.0, topp=0.9, **CONTROLS)
    ctx.constraint_set(None)
    ctx.logprobs_arm(5, "raw")
    ctx.reset_kv(); warm, _ = ctx.generate_ex(prompt, 0, 32, s, rng_state=3)
    warm_rec = ctx.last_logprobs()
    ctx.reset_kv()
    f0 = free_bytes()
    ctx.logprobs_arm(20, "shaped"); ctx.logprobs_arm(5, "raw")
    ids, _ = ctx.generate_ex(prompt, 0, 32, s, rng_state=3)
    rec = ctx.last_logprobs()
    f1 = free_bytes()
    assert list(ids) == list(warm) and f0 - f1 <= 0, f"{f0 - f1} bytes less free device memory after an armed flm_generate_ex"
    _same(rec, warm_rec)
    ctx.logprobs_arm(-1)


@pytest.mark.parametrize("source", SOURCES)
def test_the_7b_shape_with_its_vocabulary_and_a_retried_call(gpu, source):
    """the 2-layer 7B-width model, vocabulary 32000, top_n 20; then the injected wait failure: the first attempt runs through on garbage, the call re-runs and rewrites
    its records"""
    cfg, ctx = _ctx(gpu, "7B-int8")
    prompt = _prompt(cfg.vocab_size, 5)
    s = Sampling(temperature=1.0, topp=0.9, **CONTROLS)
    ids, sref, raw, shaped = host_loop_rows(ctx, host_lib(), prompt, 8, s, 1234)
    want = expected_records(ids, raw, shaped, source, 20)
    ctx.logprobs_arm(20, source)
    ctx.reset_kv(); got, st = ctx.generate_ex(prompt, 0, 8, s, rng_state=1234)
    assert list(got) == ids and st == sref
    _same(ctx.last_logprobs(), want, "first")
    ctx.reset_kv()
    ctx.set_option("inject_wait_failure", 1)
    assert ctx.query("logprobs_top_n") == 20                           # (an option drops the graphs, not the setting)
    seen = []
    got, st = ctx.generate_ex(prompt, 0, 8, s, rng_state=1234, on_token=lambda i, tok, last: seen.append((i, tok, last)) and None)
    assert list(got) == ids and st == sref and seen == [(i, ids[i], i == 7) for i in range(8)] and ctx.query("fallback") == 1
    _same(ctx.last_logprobs(), want, "retried")
    ctx.close()


def test_the_timing_tap_rewrites_the_last_record_with_the_same_bytes(gpu, ctxs):
    cfg, ctx = ctxs("tiny")
    prompt = _prompt(cfg.vocab_size, 12)
    ctx.constraint_set(None)
    ctx.logprobs_arm(-1)
    with pytest.raises(gpu.FlmError, match="flm error -5"):
        ctx.logprob_stage_time(3)                                      # disarmed
    ctx.logprobs_arm(20, "raw")
    ctx.reset_kv(); ctx.generate_ex(prompt, 0, 10, Sampling(temperature=1.0, topp=0.9, **CONTROLS), rng_state=5)
    before = ctx.logprob_records_raw(12).copy()
    assert ctx.logprob_stage_time(3) > 0.0
    assert ctx.logprob_records_raw(12).tobytes() == before.tobytes()
    ctx.logprobs_arm(-1)
