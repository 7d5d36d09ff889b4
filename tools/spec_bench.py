"""Greedy draft-and-verify on the 32-layer 7B-shaped int8 synthetic model: what a verify pass costs against a decode token, and what the loop delivers.
   (a) flm_decode_greedy: tokens/s for N tokens behind a prompt (wall time; the ids are the reference for everything below)
   (b) flm_verify_greedy fed the TRUE continuation as drafts, k = 4, 7 and 15 (batches of B = 5, 8, 16 rows: every draft is accepted, the call is one pass): the pass time
       t_B alone, median of `reps` calls, for "spec_gemm" 1 (the skinny kernel) and 0 (the 64 x 64 tiles; measured twice, in front of and behind the skinny runs: the spread
       is printed beside it); t_B / t_1 is the break-even number of ids per step
   (c) flm_generate_lookup on a prompt that repeats a block of its own continuation: tokens/s, accepted / steps
With --temperature T (> 0) and --topp P the same three for the SAMPLED path, state 1234, after the greedy ones and in the same JSON line under "sampled":
   (a') flm_decode_sample: t_1 sampled, beside the greedy t_1 (the difference is k_sample_advance against the argmax tail)
   (b') flm_verify_sample fed flm_decode_sample's ids as drafts, B = 5, 8, 16, with the "spec_gemm" form (c) chose; beside it flm_verify_greedy's pass at the same B in the
        same run (the difference is k_sample_rows over B rows against k_argmax_rows)
   (c') flm_generate_lookup_sample on the same kind of prompt, at state 1234 and at state 0 (the CLI's default seed: every coin 0): tokens/s, accepted / steps
With --shape the same for the path under the sampling controls (the controls of tests/test_gpu_shape.py: CONTROLS), at --temperature (default 1.0 there), state 1234, in the
same JSON line under "shaped":
   (b") flm_verify_sample_ex fed flm_generate_ex's ids as drafts, B = 5, 8, 16; beside it the unshaped flm_verify_sample pass at the same B in the same run (the
        difference is the parameter block's upload and k_shape_rows over B rows)
   (c") flm_generate_lookup_ex on a prompt that repeats a block of its own shaped continuation: tokens/s, accepted / steps, beside flm_generate_ex's tokens/s
With --stop (behind (a), nothing else): the accept step with and without stop rules -- flm_generate_lookup_ex at temperature 1, state 1234, a bias of +0, on a prompt that
repeats a block of its own continuation, with no rules installed (k_spec_accept_sample, one thread) and with the largest rule set that never fires (64 ids, 16 sequences of
32: k_spec_accept_rules, the workgroup matcher over every id of the run), alternating; the difference per verify step in microseconds, under "stop".
With --draft-model SHAPE (behind (a), nothing else; SHAPE a synthetic shape of the target's vocabulary such as 110M, or `self` = the target's own tensors in a second
context: every draft accepted, the upper bound; --target SHAPE picks the target, default 7B): draft-and-verify with a draft MODEL as the drafter (flm_generate_draft), in
one run on one box: t_1 of the target, the draft's time per token, the target's verify pass t_B for B = 5, 8, 16, and the loop's tokens/s with accepted / steps beside
flm_generate_ex on the target alone in the same process -- at temperature 0 and, with --temperature T, sampled at state 1234; under "draft_model".
Exits non-zero unless the ids of (a), (b) and (c) agree -- and, sampled, unless ids and final states agree with flm_generate; shaped, with flm_generate_ex.  Prints one
JSON line.
python tools/spec_bench.py [--temperature T] [--topp P] [--shape] [--stop] [--target SHAPE] [--draft-model SHAPE|self] [N] [reps] [layers]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.getcwd())
import numpy as np
import __graft_entry__ as g; g.load_package()
from fast_llama_amd import capi, synth, flmfile as ff

ap = argparse.ArgumentParser()
ap.add_argument("--temperature", "-t", type=float, default=0.0)
ap.add_argument("--topp", "-p", type=float, default=0.9)
ap.add_argument("--shape", action="store_true")
ap.add_argument("--stop", action="store_true")
ap.add_argument("--target", default="7B")
ap.add_argument("--draft-model", dest="draft_model", default=None)
ap.add_argument("N", nargs="?", type=int, default=128)
ap.add_argument("reps", nargs="?", type=int, default=9)
ap.add_argument("layers", nargs="?", type=int, default=None)
opt = ap.parse_args()
N, reps = opt.N, opt.reps
cfg = synth.make_config(opt.target, ff.QT_INT8)
if opt.layers is not None:
    cfg.n_layers = opt.layers
ctx = capi.Ctx(capi.desc_from_config(cfg, max_seq_len=1024))
tensors = synth.make_tensors(cfg, seed=7, share_layers=True)
ctx.upload_all(tensors)
seed = np.concatenate([[1], np.random.default_rng(1).integers(0, cfg.vocab_size, 15)]).astype(np.int32)
ok = True

# (a) the decode loop
first = ctx.forward_argmax(seed, 0)
ctx.decode_greedy(first, len(seed), 8)                    # warm
t0 = time.perf_counter(); ids = ctx.decode_greedy(first, len(seed), N); dt_a = time.perf_counter() - t0
t1_ms = dt_a * 1e3 / N
res = {"layers": cfg.n_layers, "N": N, "decode_tok_s": round(N / dt_a, 1), "t1_ms": round(t1_ms, 4)}

if opt.stop:
    noop = capi.Sampling(temperature=1.0, topp=0.9, bias={11: 0.0})
    ctx.reset_kv()
    xref, _ = ctx.generate_ex(seed, 0, 32, noop, rng_state=1234)
    xblock = np.concatenate([seed, xref]).astype(np.int32)
    xprompt = np.concatenate([xblock, xblock]).astype(np.int32)
    ctx.reset_kv()
    want, sw = ctx.generate_ex(xprompt, 0, N, noop, rng_state=1234)
    seen = set(int(x) for x in want)
    never = [t for t in range(cfg.vocab_size - 1, 0, -1) if t not in seen][:65]
    big = capi.StopRules(never[:64], [[int(want[(q + j) % N]) for j in range(31)] + [never[64]] for q in range(16)])
    ts = {"no_rules": [], "largest_rules": []}
    steps = {}
    for r in range(reps + 1):
        for name in ts:                                   # alternating: both forms see the same machine
            ctx.stop_set(big if name == "largest_rules" else None)
            ctx.reset_kv()
            t0 = time.perf_counter(); got, sg = ctx.generate_lookup_ex(xprompt, 0, N, noop, rng_state=1234, draft_len=7, ngram_max=3); dt = time.perf_counter() - t0
            ok = ok and np.array_equal(got, want) and sg == sw
            steps[name] = ctx.query("spec_steps")
            if r:
                ts[name].append(dt)
    ctx.stop_set(None)
    med = {k: float(np.median(v)) for k, v in ts.items()}
    res["stop"] = {"lookup_ex_ms": {k: round(v * 1e3, 3) for k, v in med.items()}, "runs_ms": {k: [round(x * 1e3, 3) for x in v] for k, v in ts.items()}, "steps": steps,
                   "rules_extra_us_per_step": round((med["largest_rules"] - med["no_rules"]) / max(steps["largest_rules"], 1) * 1e6, 2),
                   "accepted": ctx.query("spec_accepted"), "ids_and_state_agree": bool(ok), "fallback": ctx.query("fallback")}
    print(json.dumps(res), flush=True)
    ctx.close()
    sys.exit(0 if ok else 1)

if opt.draft_model:
    same = opt.draft_model == "self"
    dcfg = cfg if same else synth.make_config(opt.draft_model, ff.QT_INT8)
    draft = capi.Ctx(capi.desc_from_config(dcfg, max_seq_len=1024))
    draft.upload_all(tensors if same else synth.make_tensors(dcfg, seed=8, share_layers=True))
    dm = {"target": opt.target, "draft": opt.draft_model, "draft_layers": dcfg.n_layers, "t1_ms": round(t1_ms, 4)}
    # the draft's time per token: its own decode loop behind the same prompt
    dfirst = draft.forward_argmax(seed, 0)
    draft.decode_greedy(dfirst, len(seed), 8)                 # warm
    t0 = time.perf_counter(); draft.decode_greedy(dfirst, len(seed), N); dm["draft_t1_ms"] = round((time.perf_counter() - t0) * 1e3 / N, 4)
    # the target's verify pass with every draft right, B = 5, 8, 16
    for k in (4, 7, 15):
        ts = []
        for _ in range(reps + 1):
            t0 = time.perf_counter(); got = ctx.verify_greedy(first, ids[:k], len(seed)); ts.append((time.perf_counter() - t0) * 1e3)
            ok = ok and np.array_equal(got, ids[:k + 1])
        dm[f"t{k + 1}_ms"] = round(float(np.median(ts[1:])), 3)
    ctx.draft_set(draft)
    settings = [("greedy", capi.Sampling(temperature=0.0), 0)] + ([("sampled", capi.Sampling(temperature=opt.temperature, topp=opt.topp), 1234)] if opt.temperature > 0 else [])
    for name, sp, S in settings:
        for K in (4, 7, 15):
            ctx.reset_kv(); draft.reset_kv()
            ctx.generate_ex(seed, 0, 8, sp, rng_state=S)          # warm
            ctx.reset_kv()
            t0 = time.perf_counter(); want, sw = ctx.generate_ex(seed, 0, N, sp, rng_state=S); dt_g = time.perf_counter() - t0
            ctx.reset_kv()
            ctx.generate_draft(seed, 0, 8, sp, rng_state=S, draft_len=K)          # warm
            ctx.reset_kv(); draft.reset_kv()
            t0 = time.perf_counter(); got, sg = ctx.generate_draft(seed, 0, N, sp, rng_state=S, draft_len=K); dt_d = time.perf_counter() - t0
            agree = bool(np.array_equal(got, want) and sg == sw)
            ok = ok and agree
            dm[f"{name}_K{K}"] = {"generate_ex_tok_s": round(N / dt_g, 1), "generate_draft_tok_s": round(N / dt_d, 1), "steps": ctx.query("spec_steps"), "accepted": ctx.query("spec_accepted"),
                                  "draft_tokens": ctx.query("draft_tokens"), "ids_and_state_agree": agree}
            print(f"{name} K = {K}: flm_generate_draft {dm[f'{name}_K{K}']['generate_draft_tok_s']} tokens/s, accepted / steps {ctx.query('spec_accepted')} / {ctx.query('spec_steps')} "
                  f"(flm_generate_ex on the target alone: {dm[f'{name}_K{K}']['generate_ex_tok_s']} tokens/s)")
    print(f"t_1 target {dm['t1_ms']} ms, draft {dm['draft_t1_ms']} ms per token; t_5 {dm['t5_ms']} ms, t_8 {dm['t8_ms']} ms, t_16 {dm['t16_ms']} ms")
    dm["fallback"] = [ctx.query("fallback"), draft.query("fallback")]
    res["draft_model"] = dm
    res["ids_agree"] = bool(ok)
    print(json.dumps(res), flush=True)
    ctx.draft_set(None)
    draft.close(); ctx.close()
    sys.exit(0 if ok else 1)

# (b) one verify pass with every draft right
def pass_ms(k, gemm):
    global ok
    ctx.set_option("spec_gemm", gemm)
    ts = []
    for _ in range(reps + 1):
        t0 = time.perf_counter(); got = ctx.verify_greedy(first, ids[:k], len(seed)); ts.append((time.perf_counter() - t0) * 1e3)
        ok = ok and np.array_equal(got, ids[:k + 1])
    return float(np.median(ts[1:]))
for k in (4, 7, 15):
    tiles_a = pass_ms(k, 0); skinny = pass_ms(k, 1); tiles_b = pass_ms(k, 0)
    tiles = 0.5 * (tiles_a + tiles_b)
    res[f"B{k + 1}"] = {"skinny_ms": round(skinny, 3), "tiles_ms": round(tiles, 3), "tiles_spread_ms": round(abs(tiles_a - tiles_b), 3),
                        "skinny_over_t1": round(skinny / t1_ms, 2), "tiles_over_t1": round(tiles / t1_ms, 2)}
res["skinny_faster_at_all_B"] = all(res[f"B{k + 1}"]["skinny_ms"] < res[f"B{k + 1}"]["tiles_ms"] for k in (4, 7, 15))

# (c) the loop, on a prompt that holds a block of its own continuation twice
ctx.set_option("spec_gemm", 1 if res["skinny_faster_at_all_B"] else 0)
block = np.concatenate([seed, [first], ids[:31]]).astype(np.int32)
prompt = np.concatenate([block, block]).astype(np.int32)
ctx.reset_kv()
ref, _ = ctx.generate(prompt, 0, N)
ctx.reset_kv()
ctx.generate_lookup(prompt, 0, 8, draft_len=7)            # warm
ctx.reset_kv()
t0 = time.perf_counter(); got = ctx.generate_lookup(prompt, 0, N, draft_len=7, ngram_max=3); dt_c = time.perf_counter() - t0
ok = ok and np.array_equal(got, ref)
res.update({"lookup_tok_s": round(N / dt_c, 1), "lookup_steps": ctx.query("spec_steps"), "lookup_accepted": ctx.query("spec_accepted"),
            "lookup_gemm": ctx.query("spec_gemm"), "ids_agree": bool(ok), "fallback": ctx.query("fallback")})

# the sampled path
if opt.temperature > 0:
    T, P, S0 = opt.temperature, opt.topp, 1234
    gemm = ctx.query("spec_gemm")
    sm = {"temperature": T, "topp": P, "gemm": gemm}
    ctx.reset_kv()
    sfirst, s1 = ctx.forward_sample(seed, 0, T, P, S0)
    ctx.decode_sample(sfirst, len(seed), 8, T, P, s1)        # warm
    t0 = time.perf_counter(); sids, s_end = ctx.decode_sample(sfirst, len(seed), N, T, P, s1); dt = time.perf_counter() - t0
    sm.update({"decode_tok_s": round(N / dt, 1), "t1_ms": round(dt * 1e3 / N, 4), "t1_minus_greedy_t1_ms": round(dt * 1e3 / N - t1_ms, 4)})

    def spass_ms(k, sampled):
        global ok
        ts = []
        for _ in range(reps + 1):
            t0 = time.perf_counter()
            if sampled:
                got, s = ctx.verify_sample(sfirst, sids[:k], len(seed), T, P, s1)
            else:
                got = ctx.verify_greedy(first, ids[:k], len(seed))
            ts.append((time.perf_counter() - t0) * 1e3)
            if sampled:
                want, sw = ctx.decode_sample(sfirst, len(seed), k + 1, T, P, s1)
                ok = ok and np.array_equal(got, want) and s == sw
        return float(np.median(ts[1:]))
    for k in (4, 7, 15):
        sa = spass_ms(k, True); gr = spass_ms(k, False)
        sm[f"B{k + 1}"] = {"sample_ms": round(sa, 3), "greedy_ms": round(gr, 3), "sample_minus_greedy_ms": round(sa - gr, 3), "sample_over_t1": round(sa / sm["t1_ms"], 2)}
    for S in (S0, 0):
        ctx.reset_kv()
        sref, s_ref = ctx.generate(seed, 0, 32, T, P, S)
        sblock = np.concatenate([seed, sref]).astype(np.int32)
        sprompt = np.concatenate([sblock, sblock]).astype(np.int32)
        ctx.reset_kv()
        t0 = time.perf_counter(); want, sw = ctx.generate(sprompt, 0, N, T, P, S); dt_g = time.perf_counter() - t0
        ctx.reset_kv()
        ctx.generate_lookup_sample(sprompt, 0, 8, T, P, S, draft_len=7)            # warm
        ctx.reset_kv()
        t0 = time.perf_counter(); got, sg = ctx.generate_lookup_sample(sprompt, 0, N, T, P, S, draft_len=7, ngram_max=3); dt_l = time.perf_counter() - t0
        agree = bool(np.array_equal(got, want) and sg == sw)
        ok = ok and agree
        sm[f"state{S}"] = {"generate_tok_s": round(N / dt_g, 1), "lookup_tok_s": round(N / dt_l, 1), "lookup_steps": ctx.query("spec_steps"), "lookup_accepted": ctx.query("spec_accepted"),
                           "ids_and_state_agree": agree}
    sm["fallback"] = ctx.query("fallback")
    res["sampled"] = sm
    res["ids_agree"] = bool(ok)
# the path under the sampling controls
if opt.shape:
    T, P, S0 = (opt.temperature if opt.temperature > 0 else 1.0), opt.topp, 1234
    controls = dict(top_k=5, min_p=0.05, repeat_penalty=1.3, penalty_last_n=8, bias={3: 2.0, 7: -np.inf})     # tests/test_gpu_shape.py: CONTROLS
    sc = capi.Sampling(temperature=T, topp=P, **controls)
    sh = {"temperature": T, "topp": P, "gemm": ctx.query("spec_gemm")}
    ctx.reset_kv()
    gids, _ = ctx.generate_ex(seed, 0, 17, sc, rng_state=S0)          # token 0 behind the seed prompt, then the 16 ids a verify pass at len(seed) must return
    window = np.concatenate([seed, gids[:1]])[-controls["penalty_last_n"]:]
    ctx.reset_kv()
    ufirst, u1 = ctx.forward_sample(seed, 0, T, P, S0)
    uids, _ = ctx.decode_sample(ufirst, len(seed), 16, T, P, u1)

    def xpass_ms(k, shaped):
        global ok
        ts = []
        for _ in range(reps + 1):
            t0 = time.perf_counter()
            if shaped:
                got, _ = ctx.verify_sample_ex(int(gids[0]), gids[1:k + 1], len(seed), sc, window, advance(S0, 1))
            else:
                got, _ = ctx.verify_sample(ufirst, uids[:k], len(seed), T, P, u1)
            ts.append((time.perf_counter() - t0) * 1e3)
            ok = ok and np.array_equal(got, gids[1:k + 2] if shaped else uids[:k + 1])
        return float(np.median(ts[1:]))

    def advance(s, n):
        for _ in range(n):
            s ^= s >> 12; s ^= (s << 25) & ((1 << 64) - 1); s ^= s >> 27
        return s
    for k in (4, 7, 15):
        a = xpass_ms(k, True); b = xpass_ms(k, False)
        sh[f"B{k + 1}"] = {"shaped_ms": round(a, 3), "unshaped_ms": round(b, 3), "shaped_minus_unshaped_ms": round(a - b, 3)}
    ctx.reset_kv()
    xref, _ = ctx.generate_ex(seed, 0, 32, sc, rng_state=S0)
    xblock = np.concatenate([seed, xref]).astype(np.int32)
    xprompt = np.concatenate([xblock, xblock]).astype(np.int32)
    ctx.reset_kv()
    t0 = time.perf_counter(); want, sw = ctx.generate_ex(xprompt, 0, N, sc, rng_state=S0); dt_g = time.perf_counter() - t0
    ctx.reset_kv()
    ctx.generate_lookup_ex(xprompt, 0, 8, sc, rng_state=S0, draft_len=7)          # warm
    ctx.reset_kv()
    t0 = time.perf_counter(); got, sg = ctx.generate_lookup_ex(xprompt, 0, N, sc, rng_state=S0, draft_len=7, ngram_max=3); dt_l = time.perf_counter() - t0
    agree = bool(np.array_equal(got, want) and sg == sw)
    ok = ok and agree
    sh.update({"generate_ex_tok_s": round(N / dt_g, 1), "lookup_ex_tok_s": round(N / dt_l, 1), "lookup_steps": ctx.query("spec_steps"), "lookup_accepted": ctx.query("spec_accepted"),
               "ids_and_state_agree": agree, "fallback": ctx.query("fallback")})
    for k in (4, 7, 15):
        print(f"t_{k + 1}: shaped {sh[f'B{k + 1}']['shaped_ms']} ms, unshaped {sh[f'B{k + 1}']['unshaped_ms']} ms")
    print(f"flm_generate_lookup_ex: {sh['lookup_ex_tok_s']} tokens/s, accepted / steps {sh['lookup_accepted']} / {sh['lookup_steps']} (flm_generate_ex: {sh['generate_ex_tok_s']} tokens/s)")
    res["shaped"] = sh
    res["ids_agree"] = bool(ok)
print(json.dumps(res), flush=True)
ctx.close()
sys.exit(0 if ok else 1)
