"""Stop rules on the device (include/flm_gpu.h: flm_stop_rules, flm_stop_set, flm_op_stop_match; the matcher: csrc/flm_stop.h).

Op level: the device's matcher equals the host restatement (flm_stop_match, pinned against tests/stop_util.py without a GPU) index for index.
Model level, on test_gpu_generate.py's "tiny" and 2-layer "7B-int8" with its seeds, MAX_SEQ, the 5-token prompt and max_tokens 40: `ref` is generate_ex with no rules
installed -- the parent's path, pinned by the existing suites -- at temperature 0 and at temperature 1 / top-p 0.9 / seed 1234; every rule set is built from it, and a call
under rules must be ref cut behind the firing index in every respect: ids, callbacks, counters, the sampler's state, the cache rows, the continuation, the finish reason.
The seeds' greedy and sampled ids were looked at on the CPU oracle (tests/oracle_py.py with host/sampler.cpp's sampler): every index the rule sets want exists -- the tests
assert that, they do not skip -- and tiny's greedy ids repeat the pair ref[6:8] at 25, which gives the draft-and-verify case an accepted draft to stop behind."""
import ctypes as C

import numpy as np
import pytest

from fast_llama_amd.capi import Dfa, Sampling, StopRules
from sample_util import advance_state
from stop_util import CANCEL, ID, LENGTH, SEQ, TOKEN, py_stop_match, seeded_streams
from test_gpu_generate import MAX_SEQ, _caches, _model, _prompt

pytestmark = pytest.mark.gpu
NAMES = ("tiny", "7B-int8")
SEED, N_MAX, N_P = 1234, 40, 5
MODES = {"greedy": Sampling(temperature=0.0, topp=0.9), "sampled": Sampling(temperature=1.0, topp=0.9)}


# ---- op level ------------------------------------------------------------------------------------------------------------------------------------------------------
def test_op_equals_the_host_restatement_on_seeded_streams(gpu):
    fired = 0
    for ids, seqs, stop_token, t in seeded_streams()[:300]:
        r = StopRules(ids, seqs)
        want = gpu.stop_match_host(r, t, stop_token)
        assert want == py_stop_match(ids, seqs, stop_token, t)
        assert gpu.op_stop_match(r, t, stop_token) == want, (ids, seqs, stop_token, t)
        fired += want[0] < len(t)
    assert fired >= 60, fired


def test_op_largest_rule_set_and_length_edges(gpu):
    rng = np.random.default_rng(5)
    # 64 ids and 16 sequences of 32: every thread of the matcher's nine waves owns an entry
    seqs = [[int(x) for x in rng.integers(0, 3, 32)] for _ in range(16)]
    ids = list(range(100, 164))
    big = StopRules(ids, seqs)
    for s in (0, 7, 15):                       # a stream that ends in sequence s behind a prefix no sequence matches (symbol 3 is in none); the lowest equal sequence wins
        t = [3] * 5 + seqs[s]
        want = gpu.stop_match_host(big, t)
        assert want == (len(t) - 1, SEQ, min(k for k in range(16) if seqs[k] == seqs[s]))
        assert gpu.op_stop_match(big, t) == want
    for p in (0, 31, 63):                      # id at position p, in front of a stream that would otherwise run into sequence 3
        t = [3, 3, ids[p]] + seqs[3]
        assert gpu.op_stop_match(big, t) == gpu.stop_match_host(big, t) == (2, ID, p)
    t = [int(x) for x in rng.integers(0, 3, 200)]
    assert gpu.op_stop_match(big, t) == gpu.stop_match_host(big, t)
    # n = 1, L - 1, L, L + 1 for L = 1, 2, 32, the sequence at the stream's end and one index earlier
    for L in (1, 2, 32):
        q = [int(x) for x in rng.integers(0, 4, L)]
        r = StopRules([], [q])
        for n in sorted({1, max(L - 1, 1), L, L + 1}):
            for t in ((q * 2)[:n], ([7] * n + q)[-n:], ([7] * n + q + [7])[-n:]):
                assert gpu.op_stop_match(r, t) == gpu.stop_match_host(r, t) == py_stop_match([], [q], -1, t), (L, n, t)
    # the stop token wins over an id and a sequence at one index
    r = StopRules([5], [[4, 5]])
    assert gpu.op_stop_match(r, [4, 5], 5) == (1, TOKEN, 0) and gpu.op_stop_match(r, [4, 5]) == (1, ID, 0)


# ---- model level ---------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def models(gpu):
    """per model: the context and, per mode, ref = the rule-free generate_ex's ids with the caches it leaves (computed once, never changed)"""
    made = {}

    def get(name):
        if name not in made:
            cfg, tensors = _model(name)
            ctx = gpu.Ctx(gpu.desc_from_config(cfg, max_seq_len=MAX_SEQ)); ctx.upload_all(tensors)
            prompt = _prompt(cfg.vocab_size, N_P)
            refs = {}
            for mode, sp in MODES.items():
                ctx.reset_kv()
                ids, s = ctx.generate_ex(prompt, 0, N_MAX, sp, rng_state=SEED)
                assert len(ids) == N_MAX and ctx.stop_reason() == (LENGTH, 0) and ctx.query("stop_rules") == 0
                assert s == (advance_state(SEED, N_MAX) if mode == "sampled" else SEED)
                refs[mode] = ([int(x) for x in ids], _caches(ctx, cfg))
            made[name] = (cfg, ctx, prompt, refs)
        return made[name]
    yield get
    for _, c, _, _ in made.values():
        c.close()


def _first_occurrence(ref, lo=3, hi=20):
    js = [j for j in range(lo, hi) if ref[j] not in ref[:j]]
    assert js, f"the model seed must give a first-occurrence id in ref[{lo}:{hi}]: {ref}"
    return js[0]


def _never(ref, V, k):
    out = [t for t in range(V - 1, 0, -1) if t not in ref][:k]
    assert len(out) == k
    return out


def rule_sets(gpu, ref, V):
    """(label, rules, (index, kind, rule)) for the six choices; every expectation is the host matcher's on ref, and lies below max_tokens - 1"""
    j = _first_occurrence(ref)
    nv = _never(ref, V, 4)
    sets = [
        ("a: an id set", StopRules([nv[0], ref[j], nv[1], nv[2]]), (j, ID, 1)),
        ("b: a 3-id sequence", StopRules([], [ref[j - 2:j + 1]]), (j, SEQ, 0)),
        ("c: the first three ids", StopRules([], [ref[0:3]]), (2, SEQ, 0)),
        ("d: a decoy in front", StopRules([], [[ref[j - 2], ref[j - 1], nv[3]], ref[j - 2:j + 1]]), (j, SEQ, 1)),
        ("e: the first id", StopRules([ref[0]]), (0, ID, 0)),
        ("f: across indices 15 | 16", StopRules([nv[0]], [ref[14:17]]), (16, SEQ, 0)),
    ]
    for label, rules, want in sets:
        assert gpu.stop_match_host(rules, ref) == want, (label, ref)
        assert want[0] < N_MAX - 1
    return sets


def _check(gpu, model, mode, label, rules, want, call="generate_ex", **kw):
    cfg, ctx, prompt, refs = model
    ref, ref_caches = refs[mode]
    sp = MODES[mode]
    j, kind, rule = want
    what = (mode, label, call, kw)
    ctx.stop_set(rules)
    try:
        assert ctx.query("stop_rules") == 1
        ctx.reset_kv()
        n_shaped = ctx.query("shaped_tokens")
        seen = []
        ids, s = getattr(ctx, call)(prompt, 0, N_MAX, sp, rng_state=SEED, on_token=lambda i, t, last: seen.append((i, t, last)) and None, **kw)
        assert [int(x) for x in ids] == ref[:j + 1], (what, list(ids), ref[:j + 1])
        assert seen == [(i, ref[i], i == j) for i in range(j + 1)], (what, seen)
        if call == "generate_ex":
            assert ctx.query("gen_tokens") == j + 1, what
        assert ctx.query("shaped_tokens") == n_shaped + j + 1, what                       # (installed rules count as a control that is set)
        assert s == (advance_state(SEED, j + 1) if mode == "sampled" else SEED), what
        assert ctx.stop_reason() == (kind, rule), (what, ctx.stop_reason())
        for got, exp in zip(_caches(ctx, cfg), ref_caches):
            if call == "generate_ex":               # (a verify batch writes the rows of its rejected drafts too: stale, and rewritten before they are read)
                assert not got[:, N_P + j:, :].any(), (what, "rows at or behind n_prompt + j were written")
            assert np.array_equal(got[:, :N_P + j, :], exp[:, :N_P + j, :]), what
        if mode == "greedy":
            assert [int(x) for x in ctx.decode_greedy(ref[j], N_P + j, 6)] == ref[j + 1:j + 7], what
        else:
            assert [int(x) for x in ctx.decode_sample(ref[j], N_P + j, 6, sp.temperature, sp.topp, s)[0]] == ref[j + 1:j + 7], what
        assert ctx.query("fallback") == 0, what
    finally:
        ctx.stop_set(None)
    assert ctx.query("stop_rules") == 0


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", NAMES)
def test_generate_ex_ends_at_the_firing_index(gpu, models, name, mode):
    model = models(name)
    for label, rules, want in rule_sets(gpu, model[3][mode][0], model[0].vocab_size):
        _check(gpu, model, mode, label, rules, want)


@pytest.mark.parametrize("name", NAMES)
def test_rules_that_never_fire_and_cancel(gpu, models, name):
    cfg, ctx, prompt, refs = models(name)
    ref, _ = refs["sampled"]
    nv = _never(ref, cfg.vocab_size, 4)
    rules = StopRules(nv[:2], [[ref[3], nv[2]], [nv[3]] * 32])
    assert gpu.stop_match_host(rules, ref) == (N_MAX, LENGTH, 0)
    ctx.stop_set(rules)
    try:
        ctx.reset_kv()
        ids, s = ctx.generate_ex(prompt, 0, N_MAX, MODES["sampled"], rng_state=SEED)
        assert [int(x) for x in ids] == ref and s == advance_state(SEED, N_MAX)
        assert ctx.stop_reason() == (LENGTH, 0) and ctx.query("gen_tokens") == N_MAX
        # the entry point's own stop token under installed rules: kind 1
        j = _first_occurrence(ref)
        ctx.reset_kv()
        ids, _ = ctx.generate_ex(prompt, 0, N_MAX, MODES["sampled"], rng_state=SEED, stop_token=ref[j])
        assert [int(x) for x in ids] == ref[:j + 1] and ctx.stop_reason() == (TOKEN, 0)
        # a cancelling callback: the call ends behind it, on no rule, short of max_tokens
        ctx.reset_kv()
        n_max = MAX_SEQ - N_P
        ids, _ = ctx.generate_ex(prompt, 0, n_max, MODES["greedy"], on_token=lambda i, t, last: i == 3)
        print(f"cancel at index 3 of {n_max} under rules: n_out = {len(ids)}")
        assert 4 <= len(ids) < n_max, "the device ran to max_tokens before the cancel landed"
        assert ctx.stop_reason() == (CANCEL, 0)
        assert ctx.query("fallback") == 0
    finally:
        ctx.stop_set(None)
    # the plain form's reasons: 0, 1 (and 4) without any rules
    ctx.reset_kv()
    g = refs["greedy"][0]
    ctx.generate(prompt, 0, 12)
    assert ctx.stop_reason() == (LENGTH, 0)
    ctx.reset_kv()
    jg = _first_occurrence(g)
    ctx.generate(prompt, 0, N_MAX, stop_token=g[jg])
    assert ctx.stop_reason() == (TOKEN, 0)


def test_rules_with_a_constraint_logprobs_and_top_k(gpu, models):
    model = models("tiny")
    cfg, ctx, prompt, refs = model
    V = cfg.vocab_size
    ref, _ = refs["sampled"]
    sets = {label[0]: (label, rules, want) for label, rules, want in rule_sets(gpu, ref, V)}
    # an armed constraint that allows every id (its state: the parity of the last id): the state is folded over the delivered ids, the final one included
    ctx.constraint_set(Dfa.from_edges(2, [(q, t, t % 2) for q in (0, 1) for t in range(V)]))
    try:
        for key in ("b", "e"):
            label, rules, want = sets[key]
            ctx.constraint_arm(0)
            _check(gpu, model, "sampled", label + " + constraint", rules, want)
            assert ctx.query("constraint_state") == ref[want[0]] % 2
    finally:
        ctx.constraint_set(None)
    # armed log-probabilities: exactly *n_out records, the rule-free run's first *n_out
    ctx.logprobs_arm(3, "raw")
    try:
        ctx.reset_kv()
        ids, _ = ctx.generate_ex(prompt, 0, N_MAX, MODES["sampled"], rng_state=SEED)
        assert [int(x) for x in ids] == ref
        all_recs = ctx.last_logprobs()
        assert len(all_recs) == N_MAX
        label, rules, want = sets["f"]
        _check(gpu, model, "sampled", label + " + logprobs", rules, want)
        ctx.stop_set(rules)
        ctx.reset_kv()
        ids, _ = ctx.generate_ex(prompt, 0, N_MAX, MODES["sampled"], rng_state=SEED)
        recs = ctx.last_logprobs()
        assert len(ids) == len(recs) == want[0] + 1 and recs.tobytes() == all_recs[:want[0] + 1].tobytes()
        with pytest.raises(gpu.FlmError, match="flm error -1"):
            ctx.last_logprobs(0, want[0] + 2)
    finally:
        ctx.stop_set(None)
        ctx.logprobs_arm(-1)
    # top_k = 5: a control of flm_sampling next to the rules; the reference is that control's own rule-free run
    sp = Sampling(temperature=1.0, topp=0.9, top_k=5)
    ctx.reset_kv()
    ref_k = [int(x) for x in ctx.generate_ex(prompt, 0, N_MAX, sp, rng_state=SEED)[0]]
    assert len(ref_k) == N_MAX and ref_k != ref
    j = _first_occurrence(ref_k)
    rules = StopRules([], [ref_k[j - 1:j + 1]])
    assert gpu.stop_match_host(rules, ref_k) == (j, SEQ, 0)
    ctx.stop_set(rules)
    try:
        ctx.reset_kv()
        ids, s = ctx.generate_ex(prompt, 0, N_MAX, sp, rng_state=SEED)
        assert [int(x) for x in ids] == ref_k[:j + 1] and s == advance_state(SEED, j + 1) and ctx.stop_reason() == (SEQ, 0)
    finally:
        ctx.stop_set(None)


def _lookup_rows(gpu, prompt, ref, draft_len, ngram_max):
    """the batch row every index of ref is delivered from when flm_generate_lookup_ex runs without rules: the host drafter (host/spec_draft.h) over the history, the
    accept rule, single-token steps where fewer than 2 ids are wanted (None: token 0 and single-token steps)"""
    rows, total = {0: None}, 1
    while total < len(ref):
        room = len(ref) - total
        if room >= 2 and N_P + total - 1 + draft_len + 1 <= MAX_SEQ:
            d = gpu.spec_draft_host(list(prompt) + ref[:total], draft_len, ngram_max)
            m = 0
            while m < draft_len and total + m < len(ref) and ref[total + m] == int(d[m]):
                m += 1
            n = min(m + 1, room)
            for r in range(n):
                rows[total + r] = r
        else:
            n = 1
            rows[total] = None
        total += n
    return rows


@pytest.mark.parametrize("draft_len", [4, 15])
@pytest.mark.parametrize("name", NAMES)
def test_generate_lookup_ex_under_rules(gpu, models, name, draft_len):
    model = models(name)
    cfg, ctx, prompt, refs = model
    for mode in MODES:
        ref = refs[mode][0]
        for label, rules, want in rule_sets(gpu, ref, cfg.vocab_size):      # all six: (a) and (d) fire in the accept step by id / behind a decoy, (e) in k_spec_begin
            _check(gpu, model, mode, label, rules, want, call="generate_lookup_ex", draft_len=draft_len, ngram_max=3)
    if name != "tiny":
        return
    # a rule that fires INSIDE an accepted run, at a row greater than 0: tiny's greedy ids repeat a pair, so the prompt-lookup drafter has a draft accepted there
    ref = refs["greedy"][0]
    rows = _lookup_rows(gpu, prompt, ref, draft_len, 3)
    js = [j for j in range(2, N_MAX - 1) if rows[j] and gpu.stop_match_host(StopRules([], [ref[j - 1:j + 1]]), ref)[0] == j]
    assert js, ("the model seed must give an accepted draft with a first-occurrence pair behind it (picked on the CPU oracle)", ref, rows)
    j = js[0]
    assert rows[j] > 0
    _check(gpu, model, "greedy", f"a pair ending at row {rows[j]} of its batch", StopRules([], [ref[j - 1:j + 1]]), (j, SEQ, 0), call="generate_lookup_ex", draft_len=draft_len, ngram_max=3)
    ctx.stop_set(StopRules([], [ref[j - 1:j + 1]]))
    try:
        ctx.reset_kv()
        ids = ctx.generate_lookup_ex(prompt, 0, N_MAX, MODES["greedy"], draft_len=draft_len, ngram_max=3)[0]
        assert len(ids) == j + 1 and ctx.query("spec_accepted") > 0 and ctx.query("spec_steps") > 0
    finally:
        ctx.stop_set(None)


def test_plain_entry_points_ignore_the_rules(gpu, models):
    cfg, ctx, prompt, refs = models("tiny")
    ref = refs["greedy"][0]
    ref_s = refs["sampled"][0]
    sp = Sampling(temperature=1.0, topp=0.9, top_k=5)

    def plain():
        ctx.reset_kv()
        out = [[int(x) for x in ctx.generate(prompt, 0, N_MAX)[0]]]
        ctx.reset_kv()
        out.append([int(x) for x in ctx.generate(prompt, 0, N_MAX, temperature=1.0, topp=0.9, rng_state=SEED)[0]])
        ctx.reset_kv()
        out.append([int(x) for x in ctx.generate_lookup(prompt, 0, N_MAX, draft_len=4)])
        ctx.reset_kv()
        first, s = ctx.forward_sample_ex(prompt, 0, sp, rng_state=SEED)
        out.append((first, s))
        v, s2 = ctx.verify_sample_ex(first, ref_s[1:6], N_P, sp, rng_state=s)
        out.append(([int(x) for x in v], s2))
        v, s2 = ctx.verify_sample_ex(ref[0], ref[1:6], N_P, MODES["greedy"], rng_state=None)
        out.append(([int(x) for x in v], s2))
        return out
    without = plain()
    assert without[0] == ref and without[1] == ref_s and without[2] == ref and len(without[5][0]) == 6
    # rules that would end every one of these at once: the first ids of both refs, and the greedy run's second id
    ctx.stop_set(StopRules([ref[0], ref_s[0], ref[1]], [[ref[1]], ref[0:2]]))
    try:
        assert plain() == without
        assert ctx.stop_reason() == (LENGTH, 0)                    # (the last generate-family call above: generate_lookup, all of max_tokens)
    finally:
        ctx.stop_set(None)
    assert ctx.query("fallback") == 0


def test_errors_launch_nothing(gpu, models):
    cfg, ctx, prompt, refs = models("tiny")
    V = cfg.vocab_size
    good = StopRules([7], [[8, 9]])
    ctx.stop_set(good)
    try:
        ctx.reset_kv()
        ctx.generate_ex(prompt, 0, 6, MODES["greedy"])
        before = ctx.query("gen_tokens")
        assert before == 6
        for bad in (StopRules([V]), StopRules([3, 3]), StopRules([], [[1] * 33]), StopRules(raw=([], [0, 2, 1], [4, 5])), StopRules([], [[V]])):
            with pytest.raises(gpu.FlmError, match="flm error -1: stop:"):
                ctx.stop_set(bad)
            assert ctx.query("gen_tokens") == before and ctx.query("stop_rules") == 1
        # the installed rules stayed as they were: they still fire
        ref = refs["greedy"][0]
        ctx.stop_set(StopRules([ref[2]]))
        with pytest.raises(gpu.FlmError):
            ctx.stop_set(StopRules([-5]))
        ctx.reset_kv()
        ids, _ = ctx.generate_ex(prompt, 0, N_MAX, MODES["greedy"])
        assert [int(x) for x in ids] == ref[:ref.index(ref[2]) + 1] and ctx.stop_reason()[0] == ID
    finally:
        ctx.stop_set(None)
    # a sharded context; a context whose model is not complete
    tp = gpu.Ctx(gpu.desc_from_config(cfg, max_seq_len=MAX_SEQ), rank=0, world=2)
    with pytest.raises(gpu.FlmError, match="flm error -2"):
        tp.stop_set(good)
    assert tp.query("stop_rules") == 0 and tp.query("gen_tokens") == 0
    tp.close()
    empty = gpu.Ctx(gpu.desc_from_config(cfg, max_seq_len=MAX_SEQ))
    with pytest.raises(gpu.FlmError, match="flm error -5"):
        empty.stop_set(good)
    assert empty.query("stop_rules") == 0 and empty.query("gen_tokens") == 0
    empty.close()


def test_nothing_is_allocated_by_stop_set_or_an_armed_call(gpu, models):
    """hipMemGetInfo around flm_stop_set and around generate_ex under rules, on a context that has run before: the rule block exists since flm_ctx_create, the shaped
    graphs since flm_prepare"""
    cfg, ctx, prompt, refs = models("7B-int8")
    ref = refs["greedy"][0]
    hip = C.CDLL("libamdhip64.so")

    def free_bytes():
        f, t = C.c_size_t(0), C.c_size_t(0)
        assert hip.hipMemGetInfo(C.byref(f), C.byref(t)) == 0
        return f.value
    big = StopRules(_never(ref, cfg.vocab_size, 63) + [ref[9]], [[ref[20]] * 32] * 16)
    f0 = free_bytes()
    ctx.stop_set(big)
    f1 = free_bytes()
    try:
        ctx.reset_kv()
        ids, _ = ctx.generate_ex(prompt, 0, N_MAX, MODES["greedy"])
        f2 = free_bytes()
        assert [int(x) for x in ids] == ref[:ref.index(ref[9]) + 1] and ctx.stop_reason() == (ID, 63)
    finally:
        ctx.stop_set(None)
    f3 = free_bytes()
    assert f0 - f1 <= 0 and f1 - f2 <= 0 and f2 - f3 <= 0, (f0, f1, f2, f3)
