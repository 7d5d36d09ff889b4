"""The model-level entry points interleaved on ONE long-lived context (the call scripts of tests/test_gpu_longlived.py draw only forward / decode).

Context A runs a seeded script of 24 calls drawn from forward_argmax, forward_sample, decode_sample, generate, generate_ex, forward_sample_ex, verify_sample_ex,
generate_lookup_sample, generate_lookup_ex, score, constraint_arm and logprobs_arm.  For every call a second context B is first put into a clean state -- flm_reset_kv,
the constraint and the log-probabilities armed to what the script says is armed at that point -- and then runs that one call alone.  Every call starts at pos 0 with its
own 12-token prompt, so what A carries from call to call is what the host side of the library keeps between calls: the device blocks (shape, sample, DFA,
log-probability), the host fields behind the counters, and the graph cache.  One call of A per script, an _ex call, runs behind an injected wait failure and is retried.

After every call: A's result (ids, returned state, n_out, callback sequence) equals B's, the increments of "sampled_tokens" / "shaped_tokens" are equal and
"constraint_state" is equal -- and equal to the script's own fold of cycle3 over the ids.  After every _ex call flm_last_logprobs agrees: armed, the records compare equal
bit for bit; disarmed, both contexts refuse with the same error.  (Only after an _ex call: a plain call leaves the records of the context's previous _ex call where they
are, and B's previous _ex call is not A's.)  Every comparison is equality: no tolerance."""
import numpy as np
import pytest

from constraint_util import cycle3, fold, table
from logprob_util import diff_records, same_records
from shape_util import Sampling
from test_gpu_constraint import MAX_SEQ, _ctx, _prompt
from test_gpu_shape import CONTROLS

pytestmark = pytest.mark.gpu
N_CALLS, N_PROMPT, N_GEN, N_DECODE, K = 24, 12, 24, 17, 7        # N_GEN: one 16-token chunk graph, then an 8
EX_OPS = ("generate_ex", "forward_sample_ex", "verify_sample_ex", "generate_lookup_ex")
PLAIN_OPS = ("forward_argmax", "forward_sample", "decode_sample", "generate", "generate_lookup_sample", "score")
ARM_OPS = ("constraint_arm", "logprobs_arm")


def make_script(seed, V):
    """24 calls: about half of them _ex calls, a quarter plain ones, a quarter re-armings; one _ex call is marked for the injected wait failure"""
    rng = np.random.default_rng(seed)
    script = []
    for i in range(N_CALLS):
        u = rng.random()
        op = str(rng.choice(EX_OPS if u < 0.5 else PLAIN_OPS if u < 0.8 else ARM_OPS))
        call = {"op": op, "prompt": (_prompt(V, N_PROMPT) + int(rng.integers(0, V))) % V, "t": float(rng.choice([0.0, 1.0])), "controls": bool(rng.integers(0, 2)),
                "rng": int(rng.integers(1, 1 << 62)), "drafts": rng.integers(0, V, K).astype(np.int32), "inject": False}
        if op == "constraint_arm":
            call["q"] = int(rng.choice([0, -1]))
        if op == "logprobs_arm":
            call["lp"] = [(5, "raw"), (5, "shaped"), (-1, "raw")][int(rng.integers(0, 3))]
        script.append(call)
    # the two arms early, so that every script runs armed calls; then the injection in front of one of the _ex calls
    script[1].update(op="constraint_arm", q=0)
    script[3].update(op="logprobs_arm", lp=(5, "shaped" if seed % 2 else "raw"))
    ex = [i for i, c in enumerate(script) if c["op"] in EX_OPS and i > 3]
    assert ex, "the script has no _ex call to retry"
    script[ex[int(rng.integers(0, len(ex)))]]["inject"] = True
    return script


def run_call(ctx, call):
    """-> what the call returned, as plain Python values (callback sequence included)"""
    op, prompt, t, seed = call["op"], call["prompt"], call["t"], call["rng"]
    s = Sampling(temperature=t, topp=0.9, **(CONTROLS if call["controls"] else {}))
    window = prompt[-s.penalty_last_n:] if s.penalty_last_n else ()
    seen = []

    def on_token(i, tok, last):
        seen.append((i, tok, last))

    def streamed(res):
        ids, st = res
        return [int(x) for x in ids], st, len(ids), seen
    if op == "forward_argmax":
        return ctx.forward_argmax(prompt, 0)
    if op == "forward_sample":
        return ctx.forward_sample(prompt, 0, t, 0.9, seed)
    if op == "decode_sample":
        ids, st = ctx.decode_sample(int(prompt[0]), 0, N_DECODE, t, 0.9, seed)
        return [int(x) for x in ids], st
    if op == "generate":
        return streamed(ctx.generate(prompt, 0, N_GEN, t, 0.9, seed, on_token=on_token))
    if op == "generate_ex":
        return streamed(ctx.generate_ex(prompt, 0, N_GEN, s, rng_state=seed, on_token=on_token))
    if op == "forward_sample_ex":
        return ctx.forward_sample_ex(prompt, 0, s, window, seed)
    if op == "verify_sample_ex":
        ids, st = ctx.verify_sample_ex(int(prompt[0]), call["drafts"], 0, s, window, seed)
        return [int(x) for x in ids], st, len(ids)
    if op == "generate_lookup_sample":
        return streamed(ctx.generate_lookup_sample(prompt, 0, N_GEN, t, 0.9, seed, draft_len=K, on_token=on_token))
    if op == "generate_lookup_ex":
        return streamed(ctx.generate_lookup_ex(prompt, 0, N_GEN, s, rng_state=seed, draft_len=K, on_token=on_token))
    if op == "score":
        return ctx.score(prompt, 0).tobytes()
    if op == "constraint_arm":
        return ctx.constraint_arm(call["q"])
    if op == "logprobs_arm":
        return ctx.logprobs_arm(*call["lp"])
    raise AssertionError(op)


def delivered_ids(op, res):
    """the ids an _ex call delivered (what the constraint's state is folded over)"""
    return [res[0]] if op == "forward_sample_ex" else res[0]


def counters(ctx):
    return ctx.query("sampled_tokens"), ctx.query("shaped_tokens")


def logprobs_or_error(gpu, ctx):
    try:
        return ctx.last_logprobs(), None
    except gpu.FlmError as e:
        return None, str(e)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_interleaved_calls_equal_each_call_alone(gpu, seed):
    cfg, A = _ctx(gpu, "tiny")
    _, B = _ctx(gpu, "tiny")
    V = cfg.vocab_size
    dfa = cycle3(V)
    tab = table(dfa)
    A.constraint_set(dfa); B.constraint_set(dfa)
    q, lp = -1, (-1, "raw")                                  # what the script says is armed
    fb = 0
    try:
        for i, call in enumerate(make_script(seed, V)):
            op = call["op"]
            what = f"seed {seed} call {i} {op} t={call['t']} controls={call['controls']} q={q} lp={lp} inject={call['inject']}"
            B.reset_kv(); B.constraint_arm(q); B.logprobs_arm(*lp)
            b0 = counters(B)
            want = run_call(B, call)
            a0 = counters(A)
            if call["inject"]:
                A.set_option("inject_wait_failure", 1); fb += 1
            got = run_call(A, call)
            assert got == want, what
            assert A.query("fallback") == fb, what              # (the injected failure was seen by that call, and by no other)
            a1, b1 = counters(A), counters(B)
            assert (a1[0] - a0[0], a1[1] - a0[1]) == (b1[0] - b0[0], b1[1] - b0[1]), what
            if op == "constraint_arm":
                q = call["q"]
            elif op == "logprobs_arm":
                lp = call["lp"]
            elif op in EX_OPS and q >= 0:
                q = fold(tab, q, delivered_ids(op, want))
            assert A.query("constraint_state") == B.query("constraint_state") == q, what
            assert A.query("logprobs_top_n") == B.query("logprobs_top_n") == lp[0], what
            if op in EX_OPS:
                ra, ea = logprobs_or_error(gpu, A)
                rb, eb = logprobs_or_error(gpu, B)
                if lp[0] >= 0:
                    assert ea is None and eb is None and len(ra) == len(delivered_ids(op, want)), (what, ea, eb)
                    assert same_records(ra, rb), (what, diff_records(ra, rb))
                else:
                    assert ea is not None and ea == eb, (what, ea, eb)
    finally:
        A.close(); B.close()
