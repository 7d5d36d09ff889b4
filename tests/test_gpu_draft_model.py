"""Draft-and-verify with a draft MODEL as the drafter: flm_draft_set / flm_generate_draft.  Everything is equality: ids with np.array_equal, sampler states as 64-bit
integers, K/V rows on bit patterns, log-probability records byte for byte.

The oracle everywhere is Ctx.generate_ex on a target context that never had a draft attached: the verify contract is equality with the plain loop, so the ids cannot depend on
the drafter.  Target: synth "tiny" (seed 1234, int8; once int16, once "tiny128" = head size 128).  Drafts: "self" = the same tensors in a second context (accepts
everything: the teeth of the drafting itself, and at temperature 1 of the coin coupling), "other" = the same shape with ONE layer and another seed (accepts less, must not
change an id).  max_seq_len is 256, 64 in the context-end test.  CONTROLS is the set of tests/test_gpu_shape.py, the automaton cycle3 of tests/constraint_util.py."""
import ctypes

import numpy as np
import pytest

from constraint_util import cycle3
from fast_llama_amd import flmfile as ff, synth
from sample_util import advance_state
from shape_util import Sampling
from test_gpu_shape import CONTROLS
from test_gpu_spec import MAX_SEQ, _caches, _prompt, _record

pytestmark = pytest.mark.gpu

TARGETS = {"tiny-int8": ("tiny", ff.QT_INT8), "tiny-int16": ("tiny", ff.QT_INT16), "tiny128-int8": ("tiny128", ff.QT_INT8)}
SETTINGS = {"t0": (0.0, 0.9, 0), "t1-state1234": (1.0, 0.9, 1234), "t1-state0": (1.0, 0.9, 0)}
_made = {}


def _models(name):
    """-> (target cfg, target tensors, other-draft cfg, other-draft tensors)"""
    if name not in _made:
        shape, qt = TARGETS[name]
        cfg = synth.make_config(shape, qt)
        ocfg = synth.make_config(shape, qt, n_layers=1)
        _made[name] = (cfg, synth.make_tensors(cfg, seed=1234), ocfg, synth.make_tensors(ocfg, seed=77))
    return _made[name]


def _ctx(gpu, cfg, tensors, max_seq=MAX_SEQ):
    ctx = gpu.Ctx(gpu.desc_from_config(cfg, max_seq_len=max_seq)); ctx.upload_all(tensors)
    return ctx


class Rig:
    """one model's contexts: ref (never paired: the oracle), ctx (the target), and the two drafts"""

    def __init__(self, gpu, name, max_seq=MAX_SEQ):
        self.cfg, self.tensors, self.ocfg, self.otensors = _models(name)
        self.ref = _ctx(gpu, self.cfg, self.tensors, max_seq)
        self.ctx = _ctx(gpu, self.cfg, self.tensors, max_seq)
        self.drafts = {"self": _ctx(gpu, self.cfg, self.tensors, max_seq), "other": _ctx(gpu, self.ocfg, self.otensors, max_seq)}
        self.dmodel = {"self": (self.cfg, self.tensors), "other": (self.ocfg, self.otensors)}

    def attach(self, which):
        self.ctx.draft_set(self.drafts[which])
        return self.drafts[which]

    def reset(self):
        for c in (self.ref, self.ctx, *self.drafts.values()):
            c.reset_kv()

    def close(self):
        self.ctx.draft_set(None)                              # (the target does not own the draft: detach before destroying either)
        for c in (self.ref, self.ctx, *self.drafts.values()):
            c.close()


@pytest.fixture(scope="module")
def rigs(gpu):
    made = {}

    def get(name):
        if name not in made:
            made[name] = Rig(gpu, name)
        return made[name]
    yield get
    for r in made.values():
        r.close()


def _after(s0, t, draws):
    return advance_state(s0, draws) if t != 0 else s0


def _steps(pos, n_prompt, n_out, K, max_seq=MAX_SEQ):
    """a loop whose drafts are ALL accepted and that no stop ends: every batch step delivers min(K + 1, room) ids -> (steps, accepted, ids delivered in batch steps)"""
    total, at, steps, accepted, in_batches = 1, pos + n_prompt, 0, 0, 0
    while total < n_out:
        room = n_out - total
        if room >= 2 and at + K + 1 <= max_seq:
            n = min(K + 1, room)
            steps += 1; accepted += n - 1; in_batches += n
        else:
            n = 1
        total += n; at += n
    return steps, accepted, in_batches


# ---- 1: generate_draft is generate_ex ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [4, 15])
@pytest.mark.parametrize("which", ["self", "other"])
def test_generate_draft_is_generate_ex(gpu, rigs, which, K):
    """ids, n_out, the final state and the callback triples, at temperature 0 and at temperature 1 / top-p 0.9 from two states; prompt lengths 1 (the token path) and 7 (the
    batched prompt); max_tokens 1 (no step), 2 (one single-token step), K + 1 (one batch cut by the room) and 60"""
    rig = rigs("tiny-int8")
    rig.attach(which)
    V = rig.cfg.vocab_size
    for label, (t, p, s0) in SETTINGS.items():
        s = Sampling(temperature=t, topp=p)
        for n_prompt in (1, 7):
            prompt = _prompt(V, n_prompt, seed=11)
            for N in (1, 2, K + 1, 60):
                rig.reset()
                a_seen, a_cb = _record(); b_seen, b_cb = _record()
                want, s_want = rig.ref.generate_ex(prompt, 0, N, s, rng_state=s0, on_token=a_cb)
                got, s_got = rig.ctx.generate_draft(prompt, 0, N, s, rng_state=s0, draft_len=K, on_token=b_cb)
                case = (label, n_prompt, N)
                assert len(want) == N and s_want == _after(s0, t, N), case
                assert np.array_equal(got, want) and s_got == s_want, (case, list(got), list(want))
                assert a_seen == b_seen and len(b_seen) == N and b_seen[-1][2], case
                assert rig.ctx.query("draft_tokens") >= n_prompt, case
    assert rig.ctx.query("fallback") == 0 and rig.drafts[which].query("fallback") == 0


def test_generate_draft_null_sampling_is_the_greedy_loop(gpu, rigs):
    rig = rigs("tiny-int8")
    rig.attach("self")
    prompt = _prompt(rig.cfg.vocab_size, 7, seed=11)
    rig.reset()
    want, _ = rig.ref.generate_ex(prompt, 0, 30, Sampling(temperature=0.0))
    got, _ = rig.ctx.generate_draft(prompt, 0, 30, None, draft_len=7)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("name", ["tiny-int16", "tiny128-int8"])
def test_generate_draft_other_models(gpu, name):
    """the sampled case on int16 and on head size 128, both drafts"""
    rig = Rig(gpu, name)
    try:
        prompt = _prompt(rig.cfg.vocab_size, 7, seed=11)
        s = Sampling(temperature=1.0, topp=0.9)
        want, s_want = rig.ref.generate_ex(prompt, 0, 40, s, rng_state=1234)
        for which in ("self", "other"):
            rig.attach(which)
            rig.ctx.reset_kv(); rig.drafts[which].reset_kv()
            got, s_got = rig.ctx.generate_draft(prompt, 0, 40, s, rng_state=1234, draft_len=7)
            assert np.array_equal(got, want) and s_got == s_want, which
            if which == "self":
                assert (rig.ctx.query("spec_steps"), rig.ctx.query("spec_accepted")) == _steps(0, 7, 40, 7)[:2]
    finally:
        rig.close()


# ---- 2: teeth ---------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [4, 15])
@pytest.mark.parametrize("setting", ["t0", "t1-state1234"])
def test_self_draft_accepts_everything_and_another_model_accepts_less(gpu, rigs, setting, K):
    """the drafts come from the model: the same tensors as the draft, neutral controls, accept every draft -- at temperature 0, and at temperature 1 because draft i is drawn
    with the coin of row i.  Every batch step then delivers min(K + 1, room) ids.  The one-layer model of another seed accepts strictly less on the same call; same ids"""
    t, p, s0 = SETTINGS[setting]
    rig = rigs("tiny-int8")
    s = Sampling(temperature=t, topp=p)
    prompt = _prompt(rig.cfg.vocab_size, 7, seed=11)
    N = 60
    rig.reset()
    want, s_want = rig.ref.generate_ex(prompt, 0, N, s, rng_state=s0)
    steps, accepted, in_batches = _steps(0, len(prompt), N, K)
    rig.attach("self")
    got, s_got = rig.ctx.generate_draft(prompt, 0, N, s, rng_state=s0, draft_len=K)
    assert np.array_equal(got, want) and s_got == s_want
    mine = (rig.ctx.query("spec_steps"), rig.ctx.query("spec_accepted"))
    print("self-draft", setting, "K", K, "steps / accepted", mine, "expected", (steps, accepted), "draft_tokens", rig.ctx.query("draft_tokens"))
    assert mine == (steps, accepted) and accepted == in_batches - steps
    rig.attach("other")
    rig.ctx.reset_kv()
    got, s_got = rig.ctx.generate_draft(prompt, 0, N, s, rng_state=s0, draft_len=K)
    assert np.array_equal(got, want) and s_got == s_want
    print("other draft", setting, "K", K, "steps / accepted", (rig.ctx.query("spec_steps"), rig.ctx.query("spec_accepted")))
    assert rig.ctx.query("spec_accepted") < accepted


# ---- 3: everything armed ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["self", "other"])
@pytest.mark.parametrize("setting", ["t0", "t1-state1234"])
def test_everything_armed(gpu, rigs, which, setting):
    """CONTROLS, an armed automaton, log-probabilities and stop rules at once: ids, state, "constraint_state", the records and the finish reason are generate_ex's.  The
    rules (an id, then a 3-token sequence) are taken from the rule-free run of the oracle itself, behind index 9: inside the loop's batches"""
    t, p, s0 = SETTINGS[setting]
    rig = rigs("tiny-int8")
    rig.attach(which)
    V = rig.cfg.vocab_size
    s = Sampling(temperature=t, topp=p, **CONTROLS)
    prompt = _prompt(V, 7, seed=11)
    N = 40
    dfa = cycle3(V)
    try:
        for c in (rig.ref, rig.ctx):
            c.constraint_set(dfa); c.logprobs_arm(3, "raw")

        def both(rules):
            out = []
            for c, call in ((rig.ref, lambda c: c.generate_ex(prompt, 0, N, s, rng_state=s0)), (rig.ctx, lambda c: c.generate_draft(prompt, 0, N, s, rng_state=s0, draft_len=7))):
                c.reset_kv(); c.stop_set(rules); c.constraint_arm(1)
                ids, st = call(c)
                out.append((list(ids), st, c.query("constraint_state"), c.last_logprobs().tobytes(), c.stop_reason()))
            rig.drafts[which].reset_kv()
            return out
        free, got = both(None)
        assert got == free and len(free[0]) == N and all(int(x) % 3 == (1 + i) % 3 for i, x in enumerate(free[0]))
        ids = free[0]
        j = [i for i in range(2, N - 1) if ids[i] not in ids[:i]][-1]               # the latest first occurrence of an id
        want, got = both(gpu.StopRules([ids[j]], []))
        assert j >= 3 and got == want and len(want[0]) == j + 1 and want[4][0] == gpu.STOP_ID
        k = [i for i in range(2, N - 1) if gpu.stop_match_host(gpu.StopRules([], [ids[i - 2:i + 1]]), ids)[0] == i][-1]      # ... of a 3-token sequence
        want, got = both(gpu.StopRules([], [ids[k - 2:k + 1]]))
        assert k >= 3 and got == want and len(want[0]) == k + 1 and want[4][0] == gpu.STOP_SEQ
        assert rig.ctx.query("spec_steps") > 0
    finally:
        for c in (rig.ref, rig.ctx):
            c.stop_set(None); c.logprobs_arm(-1); c.constraint_set(None)


# ---- 4: stop token, max_tokens inside a batch, cancel -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [4, 15])
@pytest.mark.parametrize("setting", ["t0", "t1-state1234"])
def test_stop_cut_and_cancel(gpu, rigs, setting, K):
    t, p, s0 = SETTINGS[setting]
    rig = rigs("tiny-int8")
    rig.attach("self")
    s = Sampling(temperature=t, topp=p)
    prompt = _prompt(rig.cfg.vocab_size, 7, seed=11)
    N = 60
    rig.reset()
    want, _ = rig.ref.generate_ex(prompt, 0, N, s, rng_state=s0)
    # a stop token inside a batch (self-draft: the batches deliver indices 1 .. K + 1, K + 2 .. 2 K + 2, ...): the first id not seen before, off a batch's last row
    cut = next(i for i in range(3, N) if want[i] not in want[:i] and i % (K + 1) != 0)
    stop = int(want[cut])
    a_seen, a_cb = _record(); b_seen, b_cb = _record()
    rig.reset()
    want_s, sa = rig.ref.generate_ex(prompt, 0, N, s, rng_state=s0, stop_token=stop, on_token=a_cb)
    got_s, sb = rig.ctx.generate_draft(prompt, 0, N, s, rng_state=s0, stop_token=stop, draft_len=K, on_token=b_cb)
    assert len(want_s) == cut + 1 and want_s[-1] == stop
    assert np.array_equal(got_s, want_s) and a_seen == b_seen and b_seen[-1] == (cut, stop, True)
    assert sa == sb == _after(s0, t, cut + 1)
    assert rig.ctx.stop_reason() == rig.ref.stop_reason() == (gpu.STOP_TOKEN, 0)
    # max_tokens cutting a batch
    for n in (3, K, K + 3):
        rig.reset()
        a_seen, a_cb = _record(); b_seen, b_cb = _record()
        w, sa = rig.ref.generate_ex(prompt, 0, n, s, rng_state=s0, on_token=a_cb)
        g, sb = rig.ctx.generate_draft(prompt, 0, n, s, rng_state=s0, draft_len=K, on_token=b_cb)
        assert np.array_equal(g, w) and len(g) == n and a_seen == b_seen and sa == sb == _after(s0, t, n), n
        assert (rig.ctx.query("spec_steps"), rig.ctx.query("spec_accepted")) == _steps(0, len(prompt), n, K)[:2], n
    # a callback that cancels at index 5: the call ends behind the step that delivered it
    def cancelling(seen):
        return lambda i, tok, last: seen.append((i, tok, last)) or i == 5
    a_seen, b_seen = [], []
    rig.reset()
    want_c, _ = rig.ref.generate_ex(prompt, 0, N, s, rng_state=s0, on_token=cancelling(a_seen))
    got_c, sb = rig.ctx.generate_draft(prompt, 0, N, s, rng_state=s0, draft_len=K, on_token=cancelling(b_seen))
    assert a_seen == b_seen and len(b_seen) == 6
    assert 6 <= len(got_c) <= N and np.array_equal(got_c, want[:len(got_c)]) and np.array_equal(want_c, want[:len(want_c)])
    assert sb == _after(s0, t, len(got_c)) and rig.ctx.stop_reason()[0] == gpu.STOP_CANCEL
    # ... and the draft is caught up behind a cancelled call too: the continuation is the oracle's
    at = len(prompt) + len(got_c) - 1
    rig.ref.reset_kv(); rig.ref.forward(np.concatenate([prompt, got_c[:-1]]), 0)
    w2, _ = rig.ref.generate_ex(got_c[-1:], at, 12, s, rng_state=7)
    g2, _ = rig.ctx.generate_draft(got_c[-1:], at, 12, s, rng_state=7, draft_len=K)
    assert np.array_equal(g2, w2)
    assert (rig.ctx.query("spec_steps"), rig.ctx.query("spec_accepted")) == _steps(at, 1, 12, K)[:2]
    assert rig.ctx.query("fallback") == 0


# ---- 5: the end of the context ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["self", "other"])
def test_context_end(gpu, which):
    """max_seq_len 64 on both contexts and pos + n_prompt + max_tokens - 1 == 64: the last steps are single-token steps on the target, the draft catches up at the end"""
    M = 64
    rig = Rig(gpu, "tiny-int8", max_seq=M)
    try:
        draft = rig.attach(which)
        V = rig.cfg.vocab_size
        head, prompt = _prompt(V, 9, seed=5), _prompt(V, 7, seed=11)
        pos, N = len(head), M - len(head) - 7 + 1
        for t, p, s0 in SETTINGS.values():
            s = Sampling(temperature=t, topp=p)
            for c in (rig.ref, rig.ctx, draft):
                c.reset_kv(); c.forward(head, 0)
            a_seen, a_cb = _record(); b_seen, b_cb = _record()
            want, sa = rig.ref.generate_ex(prompt, pos, N, s, rng_state=s0, on_token=a_cb)
            got, sb = rig.ctx.generate_draft(prompt, pos, N, s, rng_state=s0, draft_len=7, on_token=b_cb)
            assert len(want) == N and np.array_equal(got, want) and sa == sb and a_seen == b_seen
            assert 0 < rig.ctx.query("spec_steps") < N - 1            # (batch steps ran, and at least the last positions were single tokens)
            if which == "self":
                assert (rig.ctx.query("spec_steps"), rig.ctx.query("spec_accepted")) == _steps(pos, 7, N, 7, M)[:2]
        with pytest.raises(gpu.FlmError, match="flm error -1"):
            rig.ctx.generate_draft(prompt, pos, N + 1, Sampling(temperature=0.0), draft_len=7)
    finally:
        rig.close()


# ---- 6: both caches afterwards ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["self", "other"])
def test_both_caches_hold_the_sequence_and_the_loop_continues(gpu, rigs, which):
    """rows [0, n_prompt + n_out - 1) of every layer, target and draft, against plain contexts of the two models fed the same tokens with forward; then a second call at that
    position equals generate_ex continuing -- with the self-draft it still accepts everything, so the draft's rows are not just present but right"""
    rig = rigs("tiny-int8")
    draft = rig.attach(which)
    dcfg, dtensors = rig.dmodel[which]
    V = rig.cfg.vocab_size
    prompt = _prompt(V, 7, seed=11)
    for (t, p, s0), N, K in ((SETTINGS["t1-state1234"], 23, 7), (SETTINGS["t0"], 17, 4), (SETTINGS["t0"], 9, 15)):
        s = Sampling(temperature=t, topp=p)
        rig.reset()
        want, s1 = rig.ref.generate_ex(prompt, 0, N, s, rng_state=s0)
        got, s1g = rig.ctx.generate_draft(prompt, 0, N, s, rng_state=s0, draft_len=K)
        assert np.array_equal(got, want) and s1 == s1g
        rows = len(prompt) + N - 1
        seq = np.concatenate([prompt, want[:-1]]).astype(np.int32)
        for held, (cfg, tensors) in ((rig.ctx, (rig.cfg, rig.tensors)), (draft, (dcfg, dtensors))):
            plain = _ctx(gpu, cfg, tensors)
            plain.forward(seq, 0)
            for x, y in zip(_caches(held, cfg), _caches(plain, cfg)):
                assert np.array_equal(x[:, :rows], y[:, :rows]), (which, N, K, held is draft)
            plain.close()
        w2, s2 = rig.ref.generate_ex(want[-1:], rows, 20, s, rng_state=s1)
        g2, s2g = rig.ctx.generate_draft(got[-1:], rows, 20, s, rng_state=s1, draft_len=K)
        assert np.array_equal(g2, w2) and s2 == s2g
        if which == "self":
            assert (rig.ctx.query("spec_steps"), rig.ctx.query("spec_accepted")) == _steps(rows, 1, 20, K)[:2]


# ---- 7: re-run --------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["target", "draft", "both"])
def test_a_rerun_step_delivers_every_index_once(gpu, where):
    """a timed-out cross-workgroup wait (injected, the dial tests/test_gpu_spec.py uses) in the target, in the draft, in both: the whole attempt re-runs from what the host
    holds; the same ids and state, every index once"""
    rig = Rig(gpu, "tiny-int8")
    try:
        draft = rig.attach("self")
        prompt = _prompt(rig.cfg.vocab_size, 7, seed=11)
        t, p, s0 = SETTINGS["t1-state1234"]
        s = Sampling(temperature=t, topp=p)
        N = 30
        a_seen, a_cb = _record(); b_seen, b_cb = _record()
        want, sa = rig.ref.generate_ex(prompt, 0, N, s, rng_state=s0, on_token=a_cb)
        if where in ("target", "both"):
            rig.ctx.set_option("inject_wait_failure", 1)
        if where in ("draft", "both"):
            draft.set_option("inject_wait_failure", 1)
        got, sb = rig.ctx.generate_draft(prompt, 0, N, s, rng_state=s0, draft_len=7, on_token=b_cb)
        assert np.array_equal(got, want) and sb == sa == _after(s0, t, N)
        assert b_seen == a_seen and [i for i, _, _ in b_seen] == list(range(N))
        assert rig.ctx.query("fallback") == (1 if where in ("target", "both") else 0)
        assert draft.query("fallback") == (1 if where in ("draft", "both") else 0)
        assert (rig.ctx.query("spec_steps"), rig.ctx.query("spec_accepted")) == _steps(0, len(prompt), N, 7)[:2]
    finally:
        rig.close()


# ---- 8: nothing allocated ---------------------------------------------------------------------------------------------------------------------------------------
def test_nothing_is_allocated_inside_generate_draft(gpu):
    """the first flm_generate_draft of a fresh pair (sampled under the controls; then greedy with K = 15, ending in a single-token step), bracketed with hipMemGetInfo:
    everything the pairing needs was created by flm_draft_set"""
    hip = ctypes.CDLL("libamdhip64.so")

    def free_bytes():
        f, t = ctypes.c_size_t(0), ctypes.c_size_t(0)
        assert hip.hipMemGetInfo(ctypes.byref(f), ctypes.byref(t)) == 0
        return f.value
    rig = Rig(gpu, "tiny-int8")
    try:
        rig.attach("other")
        prompt = _prompt(rig.cfg.vocab_size, 7, seed=11)
        f0 = free_bytes()
        a, _ = rig.ctx.generate_draft(prompt, 0, 40, Sampling(temperature=1.0, topp=0.9, **CONTROLS), rng_state=1234, draft_len=7)
        f1 = free_bytes()
        rig.ctx.reset_kv(); rig.drafts["other"].reset_kv()
        b, _ = rig.ctx.generate_draft(prompt, 0, 34, Sampling(temperature=0.0), draft_len=15)
        f2 = free_bytes()
        rig.attach("self"); rig.ctx.draft_set(None); rig.attach("other")          # re-attaching and detaching allocate nothing that stays
        f3 = free_bytes()
        assert f0 == f1 == f2 == f3, (f0, f1, f2, f3)
        assert len(a) == 40 and len(b) == 34
    finally:
        rig.close()


# ---- 9: invalid arguments ---------------------------------------------------------------------------------------------------------------------------------------
def test_invalid_arguments_touch_nothing(gpu):
    M = 64
    rig = Rig(gpu, "tiny-int8", max_seq=M)
    short = _ctx(gpu, rig.cfg, rig.tensors, max_seq=32)                   # a draft with a shorter context
    vcfg = synth.make_config("tiny", ff.QT_INT8, vocab_size=384)
    vctx = _ctx(gpu, vcfg, synth.make_tensors(vcfg, seed=3), max_seq=M)   # another vocabulary
    empty = gpu.Ctx(gpu.desc_from_config(rig.cfg, max_seq_len=M))         # no tensors
    tp = gpu.Ctx(gpu.desc_from_config(rig.cfg, max_seq_len=M), rank=0, world=2)
    try:
        ctx, draft = rig.ctx, rig.drafts["self"]
        V = rig.cfg.vocab_size
        prompt = _prompt(V, 7, seed=11)
        s = Sampling(temperature=1.0, topp=0.9)
        for c in (ctx, draft, rig.ref):
            c.forward(prompt, 0)
        before = [_caches_m(c, rig.cfg, M) for c in (ctx, draft)]
        with pytest.raises(gpu.FlmError, match="flm error -5"):
            ctx.generate_draft(prompt, 0, 8, s, rng_state=1)                 # no draft attached
        with pytest.raises(gpu.FlmError, match="flm error -1"):
            ctx.draft_set(ctx)
        with pytest.raises(gpu.FlmError, match="flm error -1"):
            ctx.draft_set(vctx)
        with pytest.raises(gpu.FlmError, match="flm error -5"):
            ctx.draft_set(empty)
        with pytest.raises(gpu.FlmError, match="flm error -2"):
            ctx.draft_set(tp)
        with pytest.raises(gpu.FlmError, match="flm error -5"):
            ctx.generate_draft(prompt, 0, 8, s, rng_state=1)                 # a refused pairing attaches nothing
        rig.attach("self")
        lp0 = ctx.query("sampled_tokens")
        for kw in (dict(draft_len=3), dict(draft_len=16), dict(max_tokens=0), dict(max_tokens=M - len(prompt) + 2), dict(stop_token=V), dict(pos=-1)):
            args = dict(pos=0, max_tokens=8, draft_len=7, stop_token=-1); args.update(kw)
            with pytest.raises(gpu.FlmError, match="flm error -1"):
                ctx.generate_draft(prompt, args["pos"], args["max_tokens"], s, rng_state=1, stop_token=args["stop_token"], draft_len=args["draft_len"])
        for bad in (Sampling(temperature=-1.0), Sampling(temperature=1.0, top_k=-1), Sampling(temperature=1.0, min_p=1.0), Sampling(temperature=1.0, bias={V: 1.0})):
            with pytest.raises(gpu.FlmError, match="flm error -1"):
                ctx.generate_draft(prompt, 0, 8, bad, rng_state=1)
        wrong = prompt.copy(); wrong[3] = V
        with pytest.raises(gpu.FlmError, match="flm error -1"):
            ctx.generate_draft(wrong, 0, 8, s, rng_state=1)
        lib = gpu.lib()
        n_out = ctypes.c_int(0)
        sp, keep = s.struct()
        pp = prompt.ctypes.data_as(ctypes.c_void_p)
        assert lib.flm_generate_draft(ctx._h, pp, len(prompt), 0, 8, ctypes.byref(sp), None, ctypes.c_int32(-1), 7, None, None, None, ctypes.byref(n_out)) == -1   # no state at temperature != 0
        # the draft's max_seq_len: 7 + 26 - 1 = 32 fits it, one more does not (the target's 64 would hold both)
        ctx.draft_set(short)
        short.forward(prompt, 0)
        with pytest.raises(gpu.FlmError, match="flm error -1"):
            ctx.generate_draft(prompt, 0, 27, s, rng_state=1)
        rig.attach("self")
        assert ctx.query("sampled_tokens") == lp0
        for c, b in zip((ctx, draft), before):
            for x, y in zip(_caches_m(c, rig.cfg, M), b):
                assert np.array_equal(x, y)
        # nothing ran: the loop continues behind the prompt's rows on both, and equals the oracle
        first = int(np.argmax(rig.ref.forward(prompt, 0)))
        want, sa = rig.ref.generate_ex(np.array([first], np.int32), len(prompt), 20, s, rng_state=5)
        got, sb = ctx.generate_draft(np.array([first], np.int32), len(prompt), 20, s, rng_state=5, draft_len=7)
        assert np.array_equal(got, want) and sa == sb
        assert (ctx.query("spec_steps"), ctx.query("spec_accepted")) == _steps(len(prompt), 1, 20, 7, M)[:2]
        ctx.draft_set(short)
        short.reset_kv()
        ctx.reset_kv()
        got, _ = ctx.generate_draft(prompt, 0, 26, Sampling(temperature=0.0), draft_len=7)      # exactly the draft's context: single-token steps where the DRAFT would pass its end
        rig.ref.reset_kv()
        assert np.array_equal(got, rig.ref.generate_ex(prompt, 0, 26, Sampling(temperature=0.0))[0])
    finally:
        rig.close()
        for c in (short, vctx, empty, tp):
            c.close()


def _caches_m(ctx, cfg, max_seq):
    hs = cfg.dim // cfg.n_heads
    n = cfg.n_heads * max_seq * hs
    return [ctx.debug_read(w, l, n).view(np.uint32).copy() for l in range(cfg.n_layers) for w in ("kcache", "vcache")]


# ---- 10: the other entry points -----------------------------------------------------------------------------------------------------------------------------------
def test_other_entry_points_undisturbed(gpu):
    """with a draft attached (and after generate_draft calls) generate_lookup_ex, generate_ex, decode_greedy and verify_sample_ex on the target and decode_greedy on the
    draft give what they give on contexts that were never paired; after draft_set(None) generate_draft fails with FLM_ERR_STATE"""
    rig = Rig(gpu, "tiny-int8")
    try:
        cfg, V = rig.cfg, rig.cfg.vocab_size
        toks = _prompt(V, 50)
        s = Sampling(temperature=1.0, topp=0.9, **CONTROLS)

        def run(ctx):
            ctx.reset_kv()
            look = ctx.generate_lookup_ex(toks[:30], 0, 20, s, rng_state=7, draft_len=7)
            steps = (ctx.query("spec_steps"), ctx.query("spec_accepted"))
            ctx.reset_kv()
            gex = ctx.generate_ex(toks[:12], 0, 10, s, rng_state=7)
            ctx.reset_kv()
            ids = ctx.decode_greedy(1, 0, 20)
            ctx.reset_kv()
            ver = ctx.verify_sample_ex(1, [2, 3, 4, 5, 6], 0, s, [4, 4], 9)
            return list(look[0]), look[1], steps, list(gex[0]), gex[1], list(ids), list(ver[0]), ver[1]
        want = run(rig.ref)
        d_want = list(rig.drafts["other"].decode_greedy(1, 0, 20))
        draft = rig.attach("other")
        assert run(rig.ctx) == want and list(draft.decode_greedy(1, 0, 20)) == d_want
        rig.ctx.reset_kv(); draft.reset_kv()
        rig.ctx.generate_draft(toks[:12], 0, 30, s, rng_state=3, draft_len=15)
        assert run(rig.ctx) == want
        draft.reset_kv()
        assert list(draft.decode_greedy(1, 0, 20)) == d_want
        rig.ctx.draft_set(None)
        with pytest.raises(gpu.FlmError, match="flm error -5"):
            rig.ctx.generate_draft(toks[:12], 0, 8, s, rng_state=3)
        assert run(rig.ctx) == want
    finally:
        rig.close()
