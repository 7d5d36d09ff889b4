"""The entropy-driven samplers on the device (include/flm_gpu.h: flm_entropy, flm_entropy_set, flm_entropy_mu, flm_op_entropy_rows, flm_op_logf).

Op level: flm_logf on the device equals the host's compilation of the same header; k_entropy_rows equals the host restatement (fh_entropy / fh_mirostat_update, themselves
pinned against plain Python in tests/test_entropy_host.py) on the bit patterns -- the masked rows, the observed surprise, the updated mu.  Model level: flm_generate_ex and a
caller's flm_forward_sample_ex loop under the setting give the ids, the sampler state, the constraint state, the finish reason and the bits of mu of a host loop
(flm_forward's logits, fh_constrain, fh_shape, fh_entropy, fh_sample_state, fh_mirostat_update: tests/entropy_util.py host_loop); typical sampling through the
draft-and-verify entry points gives flm_generate_ex's ids.  Models: "tiny" int8 / int16 (model seed 59, as tests/test_gpu_shape.py) and, for the retry path, the 2-layer
7B-width model whose fused launches wait across workgroups.  Every comparison is np.array_equal / == on bit patterns."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import __graft_entry__ as graft
from fast_llama_amd import flmfile as ff, synth
from constraint_util import cycle3
from entropy_util import Entropy, F, NINF, bits, hand_rows, host_loop, order_case_H, order_case_c
from sample_util import advance_state, host_lib, logits_case
from shape_util import Sampling, host_loop as shaped_host_loop

pytestmark = pytest.mark.gpu
ROOT = graft.ROOT
MAX_SEQ = 256
MODELS = {"tiny": ("tiny", ff.QT_INT8, 59), "tiny16": ("tiny", ff.QT_INT16, 59)}
N_PROMPT, N_TOKENS, SEED = 9, 40, 1234
KINDS = ("peaked", "medium", "flat", "ties", "clip", "neginf")
TEMPS = (0.7, 1.0, 1.5)
TYPICALS = (0.2, 0.5, 0.95)
MUS = (0.5, 3.0, 10.0, 40.0)
CONTROLS = dict(top_k=40, repeat_penalty=1.3, penalty_last_n=16)


def prompt_of(V, n):
    return np.array([1] + [int(x) for x in (np.arange(1, n) * 7919) % V], dtype=np.int32)


def plain_cases():
    """the settings that run alone (tests/test_entropy_host.py checks on the CPU oracle that they mask something in most steps)"""
    return {"typical": (Sampling(temperature=1.0, topp=0.9), Entropy(typical_p=0.5)),
            "mirostat": (Sampling(temperature=1.0, topp=0.9), Entropy(mirostat=2, tau=3.0, eta=0.2))}


def all_cases():
    out = dict(plain_cases())
    out["typical + top-k + repeat"] = (Sampling(temperature=0.8, topp=0.95, **CONTROLS), Entropy(typical_p=0.7))
    out["mirostat + top-k + repeat"] = (Sampling(temperature=0.8, topp=0.95, **CONTROLS), Entropy(mirostat=2, tau=2.0, eta=0.3))
    return out


_tensors = {}


def _model(name):
    if name not in _tensors:
        shape, qt, seed = MODELS[name]
        cfg = synth.make_config(shape, qt)
        _tensors[name] = (cfg, synth.make_tensors(cfg, seed=seed))
    return _tensors[name]


@pytest.fixture(scope="module")
def ctxs(gpu):
    made = {}

    def get(name):
        if name not in made:
            cfg, tensors = _model(name)
            ctx = gpu.Ctx(gpu.desc_from_config(cfg, max_seq_len=MAX_SEQ)); ctx.upload_all(tensors)
            made[name] = (cfg, ctx)
        return made[name]
    yield get
    for _, c in made.values():
        c.close()


_refs = {}


def _ref(ctx, name, label, prompt, n, s, ent, seed, **kw):
    """the host loop's result, computed once per (model, case)"""
    key = (name, label, n, seed)
    if key not in _refs:
        _refs[key] = host_loop(ctx, host_lib(), prompt, n, s, ent, seed, **kw)
    return _refs[key]


def _mu_bits(ctx):
    return int(bits([ctx.entropy_mu()])[0])


# ---- op level ----------------------------------------------------------------------------------------------------------------------------------------------------
def test_op_logf_equals_the_host(gpu):
    from test_entropy_host import logf_inputs
    rng = np.random.default_rng(7)
    x = np.concatenate([logf_inputs(), np.exp(rng.uniform(0, 17, 100000)).astype(np.float32), rng.uniform(1, 40000, 100000).astype(np.float32)])
    assert np.array_equal(bits(gpu.op_logf(x)), bits(gpu.logf_host(x)))
    assert bits(gpu.op_logf([1.0]))[0] == 0


def _padded(rows, ld):
    a = np.full((len(rows), ld), 123.0, np.float32)                                 # (what lies behind n must not matter)
    for r, row in enumerate(rows):
        a[r, :row.size] = row
    return a


def _rows16(n):
    """16 rows: every family at least twice, each with a seed of its own"""
    return [logits_case(KINDS[r % len(KINDS)], n, seed=11 if r < len(KINDS) else 20 + r) for r in range(16)]


@pytest.mark.parametrize("T", TEMPS)
@pytest.mark.parametrize("n", (2, 64, 320, 32000, 32003))
def test_op_rows_equal_the_host_restatement(gpu, n, T):
    """vocab x the six families x T x typical_p or mu x 1 row and 16 rows, ld > n: for every typical_p and every mu a 16-row launch that holds every family (one mu for
    all its rows, so every family meets every mu) and a 1-row launch per family.  32003 is no multiple of 64 (a ragged last lane)"""
    rows16 = _rows16(n)
    launches = [rows16] + [[rows16[f]] for f in range(len(KINDS))]
    for tp in TYPICALS:
        ent = Entropy(typical_p=tp)
        want16 = [gpu.entropy_host(row, T, ent) for row in rows16]                 # (the 1-row launches' rows are the first six of these)
        for k, rows in enumerate(launches):
            got = gpu.op_entropy_rows(_padded(rows, n + 5), n, T, ent)
            for r in range(len(rows)):
                want = want16[r] if k == 0 else want16[k - 1]
                assert np.array_equal(bits(got[r]), bits(want)), (n, T, tp, len(rows), r, np.nonzero(bits(got[r]) != bits(want))[0][:8])
    ent = Entropy(mirostat=2, tau=3.0, eta=0.25)
    for mu in MUS:
        masked = [gpu.entropy_host(row, T, ent, mu=mu) for row in rows16]
        chosen16 = [int(np.nonzero(m != NINF)[0][(3 * r) % np.count_nonzero(m != NINF)]) for r, m in enumerate(masked)]       # a kept id
        want16 = [gpu.entropy_host(row, T, ent, mu=mu, chosen=chosen16[r]) for r, row in enumerate(rows16)]
        for k, rows in enumerate(launches):
            idx = list(range(16)) if k == 0 else [k - 1]
            got, obs, mu2 = gpu.op_entropy_rows(_padded(rows, n + 5), n, T, ent, mu=np.full(len(rows), mu, np.float32), chosen=[chosen16[i] for i in idx])
            for r, i in enumerate(idx):
                want, wobs, wmu = want16[i]
                assert np.array_equal(bits(got[r]), bits(want)), (n, T, mu, len(rows), r, np.nonzero(bits(got[r]) != bits(want))[0][:8])
                assert bits([obs[r]])[0] == bits([wobs])[0] and bits([mu2[r]])[0] == bits([wmu])[0], (n, T, mu, len(rows), r, obs[r], wobs, mu2[r], wmu)
    # per-row states in ONE launch: row r at mu MUS[r % 4]
    mus = np.array([MUS[r % 4] for r in range(16)], np.float32)
    got = gpu.op_entropy_rows(_padded(rows16, n + 5), n, T, ent, mu=mus)
    for r, row in enumerate(rows16):
        assert np.array_equal(bits(got[r]), bits(gpu.entropy_host(row, T, ent, mu=mus[r]))), (n, T, r)


def test_op_rows_on_the_hand_built_rows(gpu):
    cases = [(name, L, ent) for name, L in hand_rows().items()
             for ent in (Entropy(typical_p=1e-9), Entropy(typical_p=0.5), Entropy(typical_p=0.999), Entropy(mirostat=2, mu=-1.0), Entropy(mirostat=2, mu=3.0), Entropy(mirostat=2, mu=1e30))]
    for L, ent in (order_case_H(), order_case_c()):
        cases.append(("order", L, ent))
    for name, L, ent in cases:
        for T in (1.0, 0.7):
            mu = ent.struct().mu
            got = gpu.op_entropy_rows(L.reshape(1, -1), L.size, T, ent, mu=mu if ent.mode == 2 else None)
            want = gpu.entropy_host(L, T, ent)
            assert np.array_equal(bits(got[0]), bits(want)), (name, ent, T, np.nonzero(bits(got[0]) != bits(want))[0][:8])
    # off, or temperature 0: the rows as they are
    L = logits_case("medium", 320, seed=1).reshape(1, -1)
    for ent, T, mu in ((Entropy(), 1.0, None), (Entropy(typical_p=0.5), 0.0, None), (Entropy(mirostat=2), 0.0, 1.0)):
        assert np.array_equal(bits(gpu.op_entropy_rows(L, 320, T, ent, mu=mu)), bits(L))
    with pytest.raises(gpu.FlmError, match="flm error -2"):
        gpu.op_entropy_rows(np.zeros((1, 40000), np.float32), 40000, 1.0, Entropy(typical_p=0.5))       # beyond the sampler's LDS strip


# ---- model level -------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("label", list(all_cases()))
@pytest.mark.parametrize("name", list(MODELS))
def test_generate_ex_equals_the_host_loop(gpu, ctxs, name, label):
    cfg, ctx = ctxs(name)
    s, ent = all_cases()[label]
    prompt = prompt_of(cfg.vocab_size, N_PROMPT)
    ids, st, mu, _, counts = _ref(ctx, name, label, prompt, N_TOKENS, s, ent, SEED)
    masked = [live - kept for kept, live in counts]
    assert sum(1 for m in masked if m >= 1) * 2 >= len(masked), masked          # (the stage does something in most steps)
    ctx.reset_kv()
    ctx.entropy_set(ent)
    try:
        assert ctx.query("entropy") == ent.mode
        shaped0 = ctx.query("shaped_tokens")
        got, gst = ctx.generate_ex(prompt, 0, N_TOKENS, s, rng_state=SEED)
        assert [int(x) for x in got] == ids and gst == st == advance_state(SEED, N_TOKENS)
        assert ctx.query("shaped_tokens") == shaped0 + N_TOKENS
        if ent.mode == 2:
            assert _mu_bits(ctx) == int(bits([mu])[0]) and mu != F(ent.struct().mu)
            # the setting again: mu starts over, and the same call gives the same ids and the same mu
            ctx.entropy_set(ent); ctx.reset_kv()
            assert ctx.entropy_mu() == F(ent.struct().mu)
            got2, _ = ctx.generate_ex(prompt, 0, N_TOKENS, s, rng_state=SEED)
            assert [int(x) for x in got2] == ids and _mu_bits(ctx) == int(bits([mu])[0])
    finally:
        ctx.entropy_set(None)
    assert ctx.query("entropy") == 0


@pytest.mark.parametrize("label", list(plain_cases()))
@pytest.mark.parametrize("name", list(MODELS))
def test_generate_ex_under_an_armed_constraint(gpu, ctxs, name, label):
    cfg, ctx = ctxs(name)
    s, ent = plain_cases()[label]
    prompt = prompt_of(cfg.vocab_size, N_PROMPT)
    dfa = cycle3(cfg.vocab_size)
    ids, st, mu, q, _ = host_loop(ctx, host_lib(), prompt, N_TOKENS, s, ent, SEED, dfa=dfa, q=1)
    assert all(t % 3 == (1 + i) % 3 for i, t in enumerate(ids))
    ctx.reset_kv()
    ctx.constraint_set(dfa); ctx.constraint_arm(1); ctx.entropy_set(ent)
    try:
        got, gst = ctx.generate_ex(prompt, 0, N_TOKENS, s, rng_state=SEED)
        assert [int(x) for x in got] == ids and gst == st and ctx.query("constraint_state") == q
        if ent.mode == 2:
            assert _mu_bits(ctx) == int(bits([mu])[0])
    finally:
        ctx.entropy_set(None); ctx.constraint_set(None)


@pytest.mark.parametrize("label", list(plain_cases()))
@pytest.mark.parametrize("name", list(MODELS))
def test_a_stop_sequence_ends_the_run_and_mu_stops_with_it(gpu, ctxs, name, label):
    cfg, ctx = ctxs(name)
    s, ent = plain_cases()[label]
    prompt = prompt_of(cfg.vocab_size, N_PROMPT)
    free = _ref(ctx, name, label, prompt, N_TOKENS, s, ent, SEED)[0]
    rules = gpu.StopRules(seqs=[free[17:19]])
    ids, st, mu, _, _ = host_loop(ctx, host_lib(), prompt, N_TOKENS, s, ent, SEED, rules=rules)
    assert 2 <= len(ids) <= 19 and ids == free[:len(ids)]
    ctx.reset_kv()
    ctx.stop_set(rules); ctx.entropy_set(ent)
    try:
        got, gst = ctx.generate_ex(prompt, 0, N_TOKENS, s, rng_state=SEED)
        assert [int(x) for x in got] == ids and gst == st == advance_state(SEED, len(ids))
        assert ctx.stop_reason() == gpu.stop_match_host(rules, ids)[1:] and ctx.stop_reason()[0] == 3
        if ent.mode == 2:
            assert _mu_bits(ctx) == int(bits([mu])[0])                             # the stop token's update, and no further
    finally:
        ctx.entropy_set(None); ctx.stop_set(None)


@pytest.mark.parametrize("label", list(all_cases()))
def test_forward_sample_ex_as_a_callers_own_loop(gpu, ctxs, label):
    cfg, ctx = ctxs("tiny")
    s, ent = all_cases()[label]
    prompt = prompt_of(cfg.vocab_size, N_PROMPT)
    n = 12
    ids, st, mu, _, _ = _ref(ctx, "tiny", label + " x12", prompt, n, s, ent, SEED)
    ctx.reset_kv(); ctx.entropy_set(ent)
    try:
        hist, state, got = [int(x) for x in prompt], SEED, []
        feed, pos = prompt, 0
        for _ in range(n):
            w = hist[len(hist) - min(s.penalty_last_n, len(hist)):] if s.penalty_last_n > 0 else []
            tok, state = ctx.forward_sample_ex(feed, pos, s, w, rng_state=state)
            got.append(tok); hist.append(tok)
            pos += len(feed); feed = np.array([tok], np.int32)
        assert got == ids and state == st == advance_state(SEED, n)
        if ent.mode == 2:
            assert _mu_bits(ctx) == int(bits([mu])[0])
    finally:
        ctx.entropy_set(None)


def test_a_retried_call_delivers_every_index_once_and_leaves_the_same_mu(gpu):
    """the injected wait failure: the first attempt runs through on garbage, the call re-runs from the caller's state and the host's mu"""
    cfg = synth.make_config("7B", ff.QT_INT8); cfg.n_layers = 2
    ctx = gpu.Ctx(gpu.desc_from_config(cfg, max_seq_len=MAX_SEQ)); ctx.upload_all(synth.make_tensors(cfg, seed=53))
    s, ent = plain_cases()["mirostat"]
    prompt = prompt_of(cfg.vocab_size, 5)
    n = 16
    ids, st, mu, _, _ = host_loop(ctx, host_lib(), prompt, n, s, ent, SEED)
    ctx.reset_kv(); ctx.entropy_set(ent)
    ctx.set_option("inject_wait_failure", 1)
    seen = []
    got, gst = ctx.generate_ex(prompt, 0, n, s, rng_state=SEED, on_token=lambda i, tok, last: seen.append((i, tok, last)) and None)
    assert [int(x) for x in got] == ids and gst == st
    assert seen == [(i, ids[i], i == n - 1) for i in range(n)]
    assert ctx.query("fallback") == 1
    assert _mu_bits(ctx) == int(bits([mu])[0])
    ctx.close()


@pytest.mark.parametrize("K", (4, 15))
def test_typical_through_draft_and_verify_gives_generate_ex_s_ids(gpu, ctxs, K):
    cfg, ctx = ctxs("tiny")
    label = "typical + top-k + repeat"
    s, ent = all_cases()[label]
    prompt = prompt_of(cfg.vocab_size, N_PROMPT)
    ids, st, _, _, _ = _ref(ctx, "tiny", label, prompt, N_TOKENS, s, ent, SEED)
    ctx.entropy_set(ent)
    try:
        ctx.reset_kv()
        got, gst = ctx.generate_lookup_ex(prompt, 0, N_TOKENS, s, rng_state=SEED, draft_len=K, ngram_max=3)
        assert [int(x) for x in got] == ids and gst == st
        # one verify pass behind the prompt's token: every draft right, then one wrong in the middle
        s2 = Sampling(temperature=s.temperature, topp=s.topp, top_k=s.top_k)          # (no window to slide: the rows depend on the row alone)
        ref2 = host_loop(ctx, host_lib(), prompt, K + 2, s2, ent, SEED)[0]
        for wrong in (None, K // 2):
            ctx.reset_kv()
            t0, st0 = ctx.forward_sample_ex(prompt, 0, s2, (), rng_state=SEED)
            assert t0 == ref2[0]
            drafts = list(ref2[1:K + 1])
            if wrong is not None:
                drafts[wrong] = (drafts[wrong] + 1) % cfg.vocab_size
            out, st1 = ctx.verify_sample_ex(t0, drafts, N_PROMPT, s2, (), rng_state=st0)
            m = K + 1 if wrong is None else wrong + 1
            assert [int(x) for x in out] == ref2[1:1 + m] and st1 == advance_state(SEED, 1 + m)
    finally:
        ctx.entropy_set(None)


def test_what_is_not_built_is_refused_with_nothing_launched(gpu, ctxs):
    cfg, ctx = ctxs("tiny")
    prompt = prompt_of(cfg.vocab_size, N_PROMPT)
    s = Sampling(temperature=1.0, topp=0.9)
    ctx.reset_kv()
    logits = ctx.forward(prompt, 0)
    keys = ("shaped_tokens", "sampled_tokens", "gen_tokens", "spec_steps")
    counts = [ctx.query(k) for k in keys]
    miro, typ = Entropy(mirostat=2), Entropy(typical_p=0.5)
    try:
        ctx.entropy_set(miro)
        for call in (lambda: ctx.generate_lookup_ex(prompt, 0, 8, s, rng_state=1, draft_len=4), lambda: ctx.verify_sample_ex(5, [1, 2, 3, 4], N_PROMPT, s, (), rng_state=1)):
            with pytest.raises(gpu.FlmError, match="flm error -2"):
                call()
        assert ctx.entropy_mu() == F(10.0)
        for ent in (miro, typ):
            ctx.entropy_set(ent); ctx.logprobs_arm(3)
            for call in (lambda: ctx.generate_ex(prompt, 0, 8, s, rng_state=1), lambda: ctx.forward_sample_ex(prompt, 0, s, (), rng_state=1),
                         lambda: ctx.generate_lookup_ex(prompt, 0, 8, s, rng_state=1, draft_len=4)):
                with pytest.raises(gpu.FlmError, match="flm error -2"):
                    call()
            ctx.logprobs_arm(-1)
        for bad in (Entropy(typical_p=float("nan")), Entropy(mirostat=1), Entropy(mirostat=2, tau=float("inf")), Entropy(typical_p=0.5, mirostat=2)):
            with pytest.raises(gpu.FlmError, match="flm error -1"):
                ctx.entropy_set(bad)
        assert ctx.query("entropy") == 1                                              # (a refused setting leaves the one that stands)
    finally:
        ctx.logprobs_arm(-1); ctx.entropy_set(None)
    with pytest.raises(gpu.FlmError, match="flm error -5"):
        ctx.entropy_mu()                                                              # Mirostat is not set
    assert [ctx.query(k) for k in keys] == counts
    ctx.reset_kv()
    assert np.array_equal(bits(ctx.forward(prompt, 0)), bits(logits))
    tp = gpu.Ctx(gpu.desc_from_config(cfg, max_seq_len=MAX_SEQ), rank=0, world=2)
    with pytest.raises(gpu.FlmError, match="flm error -2"):
        tp.entropy_set(typ)
    tp.close()


def test_a_context_that_never_had_the_setting_draws_nothing_through_the_new_form(gpu):
    """a fresh context, flm_entropy_set never called: flm_generate_ex under controls is the shaped form's host loop and counts in "shaped_tokens"; with every control
    neutral it is flm_generate, the plain sampled form ("sampled_tokens" alone moves)"""
    cfg, tensors = _model("tiny")
    ctx = gpu.Ctx(gpu.desc_from_config(cfg, max_seq_len=MAX_SEQ)); ctx.upload_all(tensors)
    try:
        prompt = prompt_of(cfg.vocab_size, N_PROMPT)
        s = Sampling(temperature=0.8, topp=0.95, **CONTROLS)
        want, wst = shaped_host_loop(ctx, host_lib(), prompt, 24, s, SEED)
        assert ctx.query("entropy") == 0 and (ctx.query("shaped_tokens"), ctx.query("sampled_tokens")) == (0, 0)
        ctx.reset_kv()
        got, gst = ctx.generate_ex(prompt, 0, 24, s, rng_state=SEED)
        assert [int(x) for x in got] == want and gst == wst
        assert (ctx.query("shaped_tokens"), ctx.query("sampled_tokens")) == (24, 24)
        ctx.reset_kv()
        plain, pst = ctx.generate(prompt, 0, 24, temperature=1.0, topp=0.9, rng_state=SEED)
        ctx.reset_kv()
        got, gst = ctx.generate_ex(prompt, 0, 24, Sampling(temperature=1.0, topp=0.9), rng_state=SEED)
        assert np.array_equal(got, plain) and gst == pst
        assert (ctx.query("shaped_tokens"), ctx.query("sampled_tokens")) == (24, 72) and ctx.query("entropy") == 0
    finally:
        ctx.close()


def test_with_the_setting_off_nothing_changes(gpu, ctxs):
    """flm_generate_ex gives the ids it gave before; with every control neutral it is flm_generate (the sampled form: nothing is drawn through a shaped one); the plain entry
    points ignore the setting"""
    cfg, ctx = ctxs("tiny16")
    prompt = prompt_of(cfg.vocab_size, N_PROMPT)
    s = Sampling(temperature=0.8, topp=0.95, **CONTROLS)
    want, wst = shaped_host_loop(ctx, host_lib(), prompt, 24, s, SEED)
    ctx.entropy_set(Entropy(typical_p=0.3)); ctx.entropy_set(None)
    ctx.reset_kv()
    got, gst = ctx.generate_ex(prompt, 0, 24, s, rng_state=SEED)
    assert [int(x) for x in got] == want and gst == wst
    neutral = Sampling(temperature=1.0, topp=0.9)
    ctx.reset_kv()
    plain, pst = ctx.generate(prompt, 0, 24, temperature=1.0, topp=0.9, rng_state=SEED)
    shaped0, sampled0 = ctx.query("shaped_tokens"), ctx.query("sampled_tokens")
    ctx.reset_kv()
    got, gst = ctx.generate_ex(prompt, 0, 24, neutral, rng_state=SEED)
    assert np.array_equal(got, plain) and gst == pst
    assert (ctx.query("shaped_tokens"), ctx.query("sampled_tokens")) == (shaped0, sampled0 + 24)
    ctx.entropy_set(Entropy(typical_p=0.05))
    try:
        ctx.reset_kv()
        again, ast = ctx.generate(prompt, 0, 24, temperature=1.0, topp=0.9, rng_state=SEED)      # a plain entry point: the setting is ignored
        assert np.array_equal(again, plain) and ast == pst and ctx.query("shaped_tokens") == shaped0
    finally:
        ctx.entropy_set(None)


_ALLOC_CHILD = r"""
import ctypes, json, os, sys
import numpy as np
sys.path.insert(0, os.environ["FLM_ROOT"])
import __graft_entry__ as graft
graft.load_package()
from fast_llama_amd import capi, synth, flmfile as ff
cnt = ctypes.CDLL(None)                      # the LD_PRELOADed interposer (tests/helpers/hipcount.c)
cnt.hipcount_allocs.restype = ctypes.c_long
hip = ctypes.CDLL("libamdhip64.so")
def free_bytes():
    f, t = ctypes.c_size_t(0), ctypes.c_size_t(0)
    assert hip.hipMemGetInfo(ctypes.byref(f), ctypes.byref(t)) == 0
    return f.value
cfg = synth.make_config("tiny", ff.QT_INT8)
ctx = capi.Ctx(capi.desc_from_config(cfg, max_seq_len=256)); ctx.upload_all(synth.make_tensors(cfg, seed=3))
ctx.prepare()
prompt = np.array([1] + [int(x) for x in (np.arange(1, 9) * 7919) % cfg.vocab_size], np.int32)
s = capi.Sampling(temperature=1.0, topp=0.9, top_k=40)
out = {}
# this process has never called flm_entropy_set: the shaped form and the plain sampled form count as they always did
ctx.generate_ex(prompt, 0, 40, s, rng_state=1234); ctx.reset_kv()
ctx.generate_ex(prompt, 0, 40, capi.Sampling(temperature=1.0, topp=0.9), rng_state=1234); ctx.reset_kv()
before = [ctx.query("entropy"), ctx.query("shaped_tokens"), ctx.query("sampled_tokens")]
a0, f0 = cnt.hipcount_allocs(), free_bytes()
n = 0
for ent in (capi.Entropy(typical_p=0.5), capi.Entropy(mirostat=2, tau=3.0)):
    ctx.entropy_set(ent)                                                              # arm -> generate (the form's FIRST call) -> disarm
    ids, _ = ctx.generate_ex(prompt, 0, 40, s, rng_state=1234)
    n += len(ids)
    ctx.reset_kv()
    ids, _ = ctx.generate_lookup_ex(prompt, 0, 40, s, rng_state=1234, draft_len=4) if ent.mode == 1 else (ids, 0)
    ctx.entropy_set(None)
    ctx.reset_kv()
a1, f1 = cnt.hipcount_allocs(), free_bytes()
print("ALLOC " + json.dumps({"allocs": a1 - a0, "free_delta": f0 - f1, "n": n, "counted_before": a0, "shaped": ctx.query("shaped_tokens"), "before": before}))
ctx.close()
"""


def test_nothing_is_allocated_across_set_generate_unset(gpu):
    so = os.path.join(ROOT, "tests", "helpers", "libhipcount.so")
    assert os.path.exists(so), "tests/helpers/libhipcount.so missing: run __graft_entry__.build()"
    preload = os.pathsep.join(x for x in (so, os.environ.get("LD_PRELOAD", "")) if x)
    r = subprocess.run([sys.executable, "-c", _ALLOC_CHILD], capture_output=True, text=True, timeout=600, env=dict(os.environ, LD_PRELOAD=preload, FLM_ROOT=ROOT), cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    v = json.loads([l for l in r.stdout.splitlines() if l.startswith("ALLOC ")][-1][6:])
    assert v["counted_before"] > 20, "the interposer saw no allocation at create / upload -- it is not interposing"
    assert v["before"] == [0, 40, 80], v["before"]                                    # never set: 40 ids through the shaped form, 40 more through the sampled one
    assert v["n"] == 80 and v["shaped"] >= 40 + 80
    assert v["allocs"] == 0, f"{v['allocs']} allocation calls across flm_entropy_set -> flm_generate_ex -> flm_entropy_set(NULL)"
    assert v["free_delta"] <= 0, f"{v['free_delta']} bytes less free device memory"
