"""Constrained decoding on the device (include/flm_gpu.h: flm_dfa, flm_constraint_set / _arm, flm_op_constrain_rows; the mask: csrc/flm_shape.h step 0).

Op level: k_shape_rows with the automaton equals mask + fh_shape per row on the bit patterns and hands back the folded states.  Model level ("tiny" int8 / int16, MAX_SEQ
256): an armed flm_generate_ex equals the host loop of tests/constraint_util.py -- flm_forward's logits, the NumPy mask, fh_shape, fh_sample_state, delta -- in ids, sampler
state and "constraint_state"; flm_forward_sample_ex, flm_verify_sample_ex and flm_generate_lookup_ex equal it in turn.  Every comparison is array_equal: no tolerance."""
import ctypes as C

import numpy as np
import pytest

from fast_llama_amd import flmfile as ff, synth
from constraint_util import SIZES, Dfa, cycle3, delta, edge_lists, ends, fold, host_loop, np_mask, pairs, table, wide
from sample_util import advance_state, host_lib
from shape_util import NINF, Sampling, bits
from test_gpu_shape import CONTROLS

pytestmark = pytest.mark.gpu
MAX_SEQ = 256
MODELS = {"tiny": ("tiny", ff.QT_INT8, None, 59), "tiny16": ("tiny", ff.QT_INT16, None, 59), "7B-int8": ("7B", ff.QT_INT8, 2, 53)}
_tensors = {}


def _prompt(V, n):
    return np.array([1] + [int(x) for x in (np.arange(1, n) * 7919) % V], dtype=np.int32)


def _model(name):
    if name not in _tensors:
        shape, qt, layers, seed = MODELS[name]
        cfg = synth.make_config(shape, qt)
        if layers:
            cfg.n_layers = layers
        _tensors[name] = (cfg, synth.make_tensors(cfg, seed=seed))
    return _tensors[name]


def _ctx(gpu, name):
    cfg, tensors = _model(name)
    ctx = gpu.Ctx(gpu.desc_from_config(cfg, max_seq_len=MAX_SEQ)); ctx.upload_all(tensors)
    return cfg, ctx


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


AUTOMATA = {"cycle3": cycle3, "pairs": pairs}
SETTINGS = {"t0": (0.0, 0.9, {}), "t1": (1.0, 0.9, {}), "t1 controls": (1.0, 0.9, CONTROLS)}
_refs = {}


def _ref(ctx, name, aname, dfa, q0, prompt, n, s, seed, stop=-1):
    """the host loop's (ids, sampler state, automaton state), computed once per case"""
    key = (name, aname, q0, len(prompt), n, repr(s), seed, stop)
    if key not in _refs:
        _refs[key] = host_loop(ctx, host_lib(), prompt, n, s, seed, dfa, q0, stop=stop)
    return _refs[key]


def _arm(ctx, dfa, q):
    ctx.constraint_set(dfa)
    assert ctx.query("constraint_state") == -1                         # installing disarms
    ctx.constraint_arm(q)
    assert ctx.query("constraint_state") == q


# ---- op level ----------------------------------------------------------------------------------------------------------------------------------------------------
def _one_state(n, toks):
    return Dfa.from_edges(1, [(0, t, 0) for t in toks])


@pytest.mark.parametrize("n", SIZES + (70000,))
def test_op_constrain_rows_equals_mask_then_shape(gpu, n):
    rng = np.random.default_rng(n)
    lists = dict(edge_lists(n))
    if n > 5000:
        lists["5000 edges"] = sorted(int(x) for x in rng.choice(n, 5000, replace=False))
    ctl = dict(CONTROLS) if n > 7 else dict(top_k=1)
    for s in (Sampling(temperature=0.7, **ctl), Sampling(temperature=0.7)):
        for name, toks in lists.items():
            rows = {"first": 1, "last": 5}.get(name, 16 if n <= 4099 else 2)
            ld = n + 3
            L = (rng.standard_normal((rows, ld)) * 4).astype(np.float32)
            L[:, ::11] = np.float32(-0.0)
            drafts = [int(x) for x in rng.integers(0, n, rows - 1)]
            window = [int(x) for x in rng.integers(0, n, 3)]
            d = _one_state(n, toks)
            got, states = gpu.op_constrain_rows(L, n, s, d, 0, window, drafts)
            assert list(states) == [0] * rows
            wins = gpu.row_windows(window, drafts, s.penalty_last_n)
            for r in range(rows):
                want = gpu.shape_host(np_mask(L[r, :n], toks), s, wins[r])
                assert np.array_equal(bits(got[r]), bits(want)), (n, name, r, repr(s))


def test_op_states_out_is_the_folded_delta(gpu):
    V = 1000
    for d in (cycle3(V), pairs(V), ends(V, 2)):
        tab = table(d)
        rng = np.random.default_rng(3)
        q0 = d.n_states - 2
        drafts, q = [], q0
        for i in range(15):                       # ids with an edge and, every third, one without: the state stays there
            toks = d.edges(q)[0]
            t = int(toks[int(rng.integers(0, len(toks)))])
            if i % 3 == 2:
                t = next(x for x in range(V) if (q, x) not in tab) if len(toks) < V else t
            drafts.append(t); q = delta(tab, q, t)
        L = (rng.standard_normal((16, V)) * 3).astype(np.float32)
        got, states = gpu.op_constrain_rows(L, V, Sampling(temperature=1.0), d, q0, (), drafts)
        want_states = [fold(tab, q0, drafts[:r]) for r in range(16)]
        assert list(states) == want_states
        for r in range(16):
            assert np.array_equal(bits(got[r]), bits(np_mask(L[r], d.edges(want_states[r])[0]))), r


def test_op_wide_changes_no_bit(gpu):
    for n in (65, 4099, 40000):
        L = (np.random.default_rng(n).standard_normal((5, n)) * 3).astype(np.float32)
        L[:, 1] = np.float32(-0.0); L[:, 2] = -np.inf
        got, _ = gpu.op_constrain_rows(L, n, Sampling(temperature=1.0), wide(n), 0, (), [0, 1, 2, 3])
        assert np.array_equal(bits(got), bits(L))


def test_op_the_mask_runs_before_top_k(gpu):
    n = 4099
    L = np.random.default_rng(9).standard_normal(n).astype(np.float32)
    best = int(np.argmax(L))
    toks = [t for t in range(0, n, 3) if t != best]
    got, _ = gpu.op_constrain_rows(L, n, Sampling(temperature=1.0, top_k=1), _one_state(n, toks), 0)
    allowed_best = toks[int(np.argmax(L[toks]))]
    assert list(np.nonzero(got[0] != NINF)[0]) == [allowed_best] and allowed_best != best


# ---- model level -------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", list(SETTINGS))
@pytest.mark.parametrize("aname", list(AUTOMATA))
@pytest.mark.parametrize("name", ["tiny", "tiny16"])
def test_generate_ex_armed_equals_the_host_loop(gpu, ctxs, name, aname, which):
    cfg, ctx = ctxs(name)
    V = cfg.vocab_size
    t, p, ctl = SETTINGS[which]
    s = Sampling(temperature=t, topp=p, **ctl)
    dfa, q0, seed = AUTOMATA[aname](V), 1, 77
    prompt = _prompt(V, 12)
    ref, sref, qref = _ref(ctx, name, aname, dfa, q0, prompt, 48, s, seed)
    _arm(ctx, dfa, q0)
    n0 = ctx.query("shaped_tokens")
    ctx.reset_kv()
    seen = []
    ids, st = ctx.generate_ex(prompt, 0, 48, s, rng_state=seed, on_token=lambda i, tok, last: seen.append((i, tok, last)) and None)
    assert [int(x) for x in ids] == ref and st == sref and ctx.query("constraint_state") == qref
    assert seen == [(i, ref[i], i == 47) for i in range(48)]
    assert ctx.query("shaped_tokens") == n0 + 48 and ctx.query("fallback") == 0
    if aname == "cycle3":
        assert [x % 3 for x in ref] == [(q0 + i) % 3 for i in range(48)] and qref == (q0 + 48) % 3
    ctx.constraint_set(None)


def test_teeth_the_unconstrained_first_id_is_banned(gpu, ctxs):
    cfg, ctx = ctxs("tiny")
    V = cfg.vocab_size
    prompt = _prompt(V, 12)
    ctx.constraint_set(None)
    ctx.reset_kv()
    plain, _ = ctx.generate_ex(prompt, 0, 16, Sampling(temperature=0.0))
    q0 = (int(plain[0]) + 1) % 3                                       # cycle3 state q0 bans plain[0]
    dfa = cycle3(V)
    _arm(ctx, dfa, q0)
    ctx.reset_kv()
    ids, _ = ctx.generate_ex(prompt, 0, 16, Sampling(temperature=0.0))
    assert int(ids[0]) != int(plain[0]) and list(ids) != list(plain)
    assert [int(x) % 3 for x in ids] == [(q0 + i) % 3 for i in range(16)]
    ctx.constraint_set(None)


def test_ends_stops_on_the_stop_id_after_four(gpu, ctxs):
    cfg, ctx = ctxs("tiny")
    V, stop = cfg.vocab_size, 2
    prompt = _prompt(V, 12)
    dfa = ends(V, stop)
    for t, seed in ((0.0, 0), (1.0, 5)):
        s = Sampling(temperature=t, topp=0.9)
        ref, sref, qref = host_loop(ctx, host_lib(), prompt, 30, s, seed, dfa, 0, stop=stop)
        _arm(ctx, dfa, 0)
        ctx.reset_kv()
        seen = []
        ids, st = ctx.generate_ex(prompt, 0, 30, s, rng_state=seed, stop_token=stop, on_token=lambda i, tok, last: seen.append((i, tok, last)) and None)
        assert [int(x) for x in ids] == ref and st == sref and ctx.query("constraint_state") == qref
        assert len(ids) == 4 and int(ids[3]) == stop and [int(x) % 3 for x in ids[:3]] == [0, 1, 2]
        assert seen == [(i, ref[i], i == 3) for i in range(4)]
        assert qref == 3
    ctx.constraint_set(None)


def _fs_loop(ctx, first, pos, n, s, window, s0):
    """a caller's own loop: n flm_forward_sample_ex calls behind `first` at pos, the window slid over the ids -> (ids, sampler state, constraint state after each call)"""
    hist, ids, state, tok, qs = [int(x) for x in window], [], s0, int(first), []
    for i in range(n):
        w = hist[len(hist) - min(s.penalty_last_n, len(hist)):] if s.penalty_last_n > 0 else []
        tok, state = ctx.forward_sample_ex(np.array([tok], np.int32), pos + i, s, w, rng_state=state)
        ids.append(tok); hist.append(tok); qs.append(ctx.query("constraint_state"))
    return ids, state, qs


@pytest.mark.parametrize("which", ["t0", "t1 controls"])
def test_forward_sample_ex_in_a_callers_loop(gpu, ctxs, which):
    cfg, ctx = ctxs("tiny")
    V = cfg.vocab_size
    t, p, ctl = SETTINGS[which]
    s = Sampling(temperature=t, topp=p, **ctl)
    dfa, q0 = pairs(V), 3
    tab = table(dfa)
    prompt = _prompt(V, 12)
    ref, sref, qref = _ref(ctx, "tiny", "pairs", dfa, q0, prompt, 12, s, 31)
    _arm(ctx, dfa, q0)
    ctx.reset_kv()
    hist, state, ids = [int(x) for x in prompt], 31, []
    feed, pos = prompt, 0
    for i in range(12):
        w = hist[len(hist) - min(s.penalty_last_n, len(hist)):] if s.penalty_last_n > 0 else []
        tok, state = ctx.forward_sample_ex(feed, pos, s, w, rng_state=state)
        ids.append(tok); hist.append(tok)
        assert ctx.query("constraint_state") == fold(tab, q0, ids)     # moves each call
        pos += len(feed); feed = np.array([tok], np.int32)
    assert ids == ref[:12] and state == sref and ctx.query("constraint_state") == qref
    ctx.constraint_set(None)


@pytest.mark.parametrize("k", [4, 15])
@pytest.mark.parametrize("which", ["t0", "t1 controls"])
def test_verify_sample_ex_equals_the_callers_loop(gpu, ctxs, which, k):
    cfg, ctx = ctxs("tiny")
    _, ref = _second(gpu, ctxs)
    V = cfg.vocab_size
    t, p, ctl = SETTINGS[which]
    s = Sampling(temperature=t, topp=p, **ctl)
    dfa, q0, s0, pos = cycle3(V), 2, 4321, 7
    tab = table(dfa)
    prompt = _prompt(V, pos)
    window = [int(x) for x in prompt[-min(s.penalty_last_n, pos):]] if s.penalty_last_n else []

    def start(c):
        c.reset_kv(); c.forward(prompt, 0)
        c.constraint_set(dfa); c.constraint_arm(q0)
    start(ref)
    ids, _, qs = _fs_loop(ref, 5, pos, k + 1, s, window, s0)
    no_edge = next(x for x in range(V) if x % 3 != (q0 + 1) % 3 and x != ids[1])      # row 1's state is q0 + 1: an id without an edge there
    cases = [(None, None), (0, (ids[0] + 3) % V), (k // 2, (ids[k // 2] + 3) % V), (k - 1, (ids[k - 1] + 3) % V), (1, no_edge)]
    for wrong, val in cases:
        drafts = np.array(ids[:k], np.int32)
        if wrong is not None:
            drafts[wrong] = val
        m = k if wrong is None else wrong
        start(ctx)
        n0 = ctx.query("shaped_tokens")
        got, st = ctx.verify_sample_ex(5, drafts, pos, s, window, s0)
        assert [int(x) for x in got] == ids[:m + 1], (wrong, list(got), ids[:m + 1])
        assert st == (s0 if t == 0 else advance_state(s0, m + 1))
        assert ctx.query("constraint_state") == qs[m] == fold(tab, q0, ids[:m + 1])
        assert ctx.query("shaped_tokens") == n0 + m + 1
    ctx.constraint_set(None); ref.constraint_set(None)


_second_ctx = {}


def _second(gpu, ctxs):
    """a second context on the tiny int8 model (the reference side of the verify / lookup comparisons), made once"""
    if "c" not in _second_ctx:
        _second_ctx["c"] = _ctx(gpu, "tiny")
    return _second_ctx["c"]


@pytest.fixture(scope="module", autouse=True)
def _close_second():
    yield
    if "c" in _second_ctx:
        _second_ctx.pop("c")[1].close()


@pytest.mark.parametrize("K", [4, 15])
@pytest.mark.parametrize("which", ["t0", "t1 controls"])
def test_generate_lookup_ex_equals_generate_ex(gpu, ctxs, which, K):
    cfg, ctx = ctxs("tiny")
    _, ref = _second(gpu, ctxs)
    V = cfg.vocab_size
    t, p, ctl = SETTINGS[which]
    s = Sampling(temperature=t, topp=p, **ctl)
    prompt = _prompt(V, 12)
    s0 = 99
    for dfa, q0, N, stop, pos in ((pairs(V), 0, 40, -1, 0),                     # two ids per state: the drafter finds repeats
                                  (cycle3(V), 1, 40, -1, 0),
                                  (pairs(V), 0, 30, -1, MAX_SEQ - 12 - 30 + 1)):  # the tail reaches max_seq_len: single-token steps
        for c in (ref, ctx):
            c.reset_kv(); c.constraint_set(dfa); c.constraint_arm(q0)
        a_seen, b_seen = [], []
        want, sa = ref.generate_ex(prompt, pos, N, s, rng_state=s0, stop_token=stop, on_token=lambda i, tok, last: a_seen.append((i, tok, last)) and None)
        got, sb = ctx.generate_lookup_ex(prompt, pos, N, s, rng_state=s0, stop_token=stop, draft_len=K, ngram_max=3, on_token=lambda i, tok, last: b_seen.append((i, tok, last)) and None)
        assert np.array_equal(got, want) and len(got) == len(want) == N and sa == sb
        assert a_seen == b_seen
        assert ctx.query("constraint_state") == ref.query("constraint_state") == fold(table(dfa), q0, want)
        assert ctx.query("spec_steps") > 0 and ctx.query("fallback") == 0
    # a stop token inside a batch: pairs makes long accepted runs; stop at the first id not seen before index 6
    dfa, q0 = pairs(V), 0
    for c in (ref, ctx):
        c.reset_kv(); c.constraint_set(dfa); c.constraint_arm(q0)
    full, _ = ref.generate_ex(prompt, 0, 40, s, rng_state=s0)
    later = [i for i in range(3, 40) if full[i] not in full[:i]]
    if later:
        cut = later[0]; stop = int(full[cut])
        for c in (ref, ctx):
            c.reset_kv(); c.constraint_arm(q0)
        want, sa = ref.generate_ex(prompt, 0, 40, s, rng_state=s0, stop_token=stop)
        got, sb = ctx.generate_lookup_ex(prompt, 0, 40, s, rng_state=s0, stop_token=stop, draft_len=K, ngram_max=3)
        assert len(want) == cut + 1 and np.array_equal(got, want) and sa == sb
        assert ctx.query("constraint_state") == ref.query("constraint_state") == fold(table(dfa), q0, want)
    ctx.constraint_set(None); ref.constraint_set(None)


def test_disarmed_and_plain_calls_are_todays(gpu, ctxs):
    cfg, ctx = ctxs("tiny")
    V = cfg.vocab_size
    prompt = _prompt(V, 12)
    s = Sampling(temperature=1.0, topp=0.9, **CONTROLS)
    neutral = Sampling(temperature=1.0, topp=0.9)
    ctx.constraint_set(None)
    ctx.reset_kv(); base_ctl = ctx.generate_ex(prompt, 0, 24, s, rng_state=7)
    ctx.reset_kv(); base_plain = ctx.generate(prompt, 0, 24, temperature=1.0, topp=0.9, rng_state=7)
    # an automaton installed but disarmed changes nothing; neutral controls run the plain form ("shaped_tokens" stands)
    ctx.constraint_set(cycle3(V))
    n0 = ctx.query("shaped_tokens")
    ctx.reset_kv(); got = ctx.generate_ex(prompt, 0, 24, neutral, rng_state=7)
    assert list(got[0]) == list(base_plain[0]) and got[1] == base_plain[1] and ctx.query("shaped_tokens") == n0
    ctx.reset_kv(); got = ctx.generate_ex(prompt, 0, 24, s, rng_state=7)
    assert list(got[0]) == list(base_ctl[0]) and got[1] == base_ctl[1] and ctx.query("shaped_tokens") == n0 + 24
    # armed: the plain generate ignores the automaton and leaves the state alone
    ctx.constraint_arm(2)
    ctx.reset_kv(); got = ctx.generate(prompt, 0, 24, temperature=1.0, topp=0.9, rng_state=7)
    assert list(got[0]) == list(base_plain[0]) and ctx.query("constraint_state") == 2 and ctx.query("shaped_tokens") == n0 + 24
    # armed with neutral controls: the shaped form runs, masking only
    ctx.reset_kv(); ids, _ = ctx.generate_ex(prompt, 0, 9, neutral, rng_state=7)
    assert [int(x) % 3 for x in ids] == [(2 + i) % 3 for i in range(9)] and ctx.query("shaped_tokens") == n0 + 33 and ctx.query("constraint_state") == (2 + 9) % 3
    # disarm: today's results again
    ctx.constraint_arm(-1)
    ctx.reset_kv(); got = ctx.generate_ex(prompt, 0, 24, s, rng_state=7)
    assert list(got[0]) == list(base_ctl[0]) and ctx.query("constraint_state") == -1
    # wide changes no id
    _arm(ctx, wide(V), 0)
    ctx.reset_kv(); got = ctx.generate_ex(prompt, 0, 24, s, rng_state=7)
    assert list(got[0]) == list(base_ctl[0]) and got[1] == base_ctl[1] and ctx.query("constraint_state") == 0
    ctx.constraint_set(None)


def test_replacing_the_automaton_needs_no_prepare(gpu, ctxs):
    cfg, ctx = ctxs("tiny")
    V = cfg.vocab_size
    prompt = _prompt(V, 12)
    s = Sampling(temperature=0.0)
    _arm(ctx, cycle3(V), 0)
    ctx.reset_kv(); a, _ = ctx.generate_ex(prompt, 0, 6, s)
    two = Dfa.from_edges(2, [(0, t, 1) for t in range(0, V, 5)] + [(1, t, 0) for t in range(1, V, 5)])
    _arm(ctx, two, 0)
    ctx.reset_kv(); b, _ = ctx.generate_ex(prompt, 0, 6, s)
    assert [int(x) % 3 for x in a] == [0, 1, 2, 0, 1, 2] and [int(x) % 5 for x in b] == [0, 1, 0, 1, 0, 1]
    ctx.constraint_set(None)


def test_errors_launch_nothing(gpu, ctxs):
    cfg, ctx = ctxs("tiny")
    V = cfg.vocab_size
    ctx.constraint_set(None)
    with pytest.raises(gpu.FlmError, match="flm error -1"):
        ctx.constraint_arm(0)                                          # no automaton installed
    ctx.constraint_set(cycle3(V))
    for q in (3, -2, 1 << 20):
        with pytest.raises(gpu.FlmError, match="flm error -1"):
            ctx.constraint_arm(q)
    assert ctx.query("constraint_state") == -1
    with pytest.raises(gpu.FlmError, match="flm error -1"):
        ctx.constraint_set(cycle3(V + 1))                              # an id equal to the vocabulary
    ctx.constraint_arm(1)
    n0 = ctx.query("shaped_tokens")
    with pytest.raises(gpu.FlmError, match="flm error -1"):
        ctx.generate_ex(_prompt(V, 5), 0, MAX_SEQ, Sampling(temperature=0.0))      # past max_seq_len: the state does not move
    with pytest.raises(gpu.FlmError, match="flm error -1"):
        ctx.generate_ex(_prompt(V, 5), 0, 8, Sampling(temperature=0.0, top_k=-1))
    assert ctx.query("constraint_state") == 1 and ctx.query("shaped_tokens") == n0
    ctx.constraint_set(None)
    fresh = gpu.Ctx(gpu.desc_from_config(cfg, max_seq_len=MAX_SEQ))
    with pytest.raises(gpu.FlmError, match="flm error -5"):
        fresh.constraint_set(cycle3(V))                                # before the model is complete
    fresh.close()
    tp = gpu.Ctx(gpu.desc_from_config(cfg, max_seq_len=MAX_SEQ), rank=0, world=2)
    with pytest.raises(gpu.FlmError, match="flm error -2"):
        tp.constraint_set(cycle3(V))
    tp.close()


def test_a_retried_constrained_call_delivers_every_index_once(gpu):
    """the injected wait failure on the 2-layer 7B-width model: the first attempt runs through on garbage, the call re-runs from the state it was armed at"""
    cfg, ctx = _ctx(gpu, "7B-int8")
    V = cfg.vocab_size
    prompt = _prompt(V, 5)
    s = Sampling(temperature=1.0, topp=0.9, **CONTROLS)
    dfa, q0 = cycle3(V), 1
    ref, sref, qref = host_loop(ctx, host_lib(), prompt, 24, s, 1234, dfa, q0)
    _arm(ctx, dfa, q0)
    ctx.reset_kv()
    ctx.set_option("inject_wait_failure", 1)
    assert ctx.query("constraint_state") == q0                        # (an option drops the graphs, not the constraint)
    seen = []
    ids, st = ctx.generate_ex(prompt, 0, 24, s, rng_state=1234, on_token=lambda i, tok, last: seen.append((i, tok, last)) and None)
    assert [int(x) for x in ids] == ref and st == sref and ctx.query("constraint_state") == qref
    assert seen == [(i, ref[i], i == 23) for i in range(24)]
    assert ctx.query("fallback") == 1
    ctx.close()


def test_nothing_is_allocated_in_the_steady_path(gpu, ctxs):
    """one warm constrained flm_generate_ex, then a second one bracketed with hipMemGetInfo, in process"""
    cfg, ctx = ctxs("tiny")
    V = cfg.vocab_size
    hip = C.CDLL("libamdhip64.so")

    def free_bytes():
        f, t = C.c_size_t(0), C.c_size_t(0)
        assert hip.hipMemGetInfo(C.byref(f), C.byref(t)) == 0
        return f.value
    prompt = _prompt(V, 12)
    s = Sampling(temperature=1.0, topp=0.9, **CONTROLS)
    _arm(ctx, cycle3(V), 0)
    ctx.reset_kv(); warm, _ = ctx.generate_ex(prompt, 0, 32, s, rng_state=3)
    ctx.constraint_arm(0)
    ctx.reset_kv()
    f0 = free_bytes()
    ids, _ = ctx.generate_ex(prompt, 0, 32, s, rng_state=3)
    ctx.constraint_arm(1)
    f1 = free_bytes()
    assert list(ids) == list(warm) and f0 - f1 <= 0, f"{f0 - f1} bytes less free device memory after a constrained flm_generate_ex"
    ctx.constraint_set(None)
