"""Cache slots on the 32-layer 7B-shaped int8 synthetic model: aggregate tokens/s of flm_generate_batch (n DISTINCT prompts, one batch per pass over the weights) against
n SEQUENTIAL flm_generate calls timed in the same run -- the path a caller had before -- and, as a second line, flm_generate_n at the same n and prompt length (n
completions of the first prompt: the fan's step is the yardstick for the batch's step).  Prompts of 16 and of 512 tokens, 64 new tokens per sequence, n = 4, 8, 16,
temperature 1.0 / top-p 0.9, sequence j at state 1234 + j.  All forms are warmed once and timed `reps` times, alternating; medians and the spread (max - min) of the
repetitions are reported; the batch runs through the step API so that its joins and its steps are timed apart.  A cell whose slots do not fit max_seq_len (n * (prompt + new - 1) rows) is reported as such and not run.
Exits non-zero unless every sequence's ids and final state equal flm_generate's.  Prints the table and one JSON line.
--admit: the ragged passes instead (flm_batch_admit / flm_batch_pass, option "batch_rows") against the serial joins timed in the same run, per cell: the time until every
request has its token 0 -- n flm_batch_joins | one flm_batch_pass(0) | flm_batch_pass(256) until nobody fills -- and flm_generate_batch's whole-call tokens/s under
"batch_rows" -1, 0 and 256; ids and final states must be equal in every form (exit non-zero otherwise).
python tools/batch_bench.py [--admit] [--new M] [--temperature T] [--topp P] [--max-seq S] [--gemm 0|1] [--only PROMPT,N] [reps] [layers]"""
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
ap.add_argument("--new", type=int, default=64)
ap.add_argument("--temperature", "-t", type=float, default=1.0)
ap.add_argument("--topp", "-p", type=float, default=0.9)
ap.add_argument("--target", default="7B")
ap.add_argument("--max-seq", type=int, default=2048)
ap.add_argument("--gemm", type=int, default=0, help='"spec_gemm" for the batch and the fan: 0 the 64 x 64 tiles (default), 1 the skinny kernel')
ap.add_argument("--admit", action="store_true", help="time the ragged passes (admit / pass, \"batch_rows\") against the serial joins")
ap.add_argument("--only", default=None, help="PROMPT,N: that one cell alone (a profiler's run)")
ap.add_argument("reps", nargs="?", type=int, default=3)
ap.add_argument("layers", nargs="?", type=int, default=None)
opt = ap.parse_args()
M, T, P, reps, max_seq = opt.new, opt.temperature, opt.topp, opt.reps, opt.max_seq
NS, PROMPTS = (4, 8, 16), (16, 512)
if opt.only:
    PROMPTS, NS = ((int(opt.only.split(",")[0]),), (int(opt.only.split(",")[1]),))
cfg = synth.make_config(opt.target, ff.QT_INT8)
if opt.layers is not None:
    cfg.n_layers = opt.layers
ctx = capi.Ctx(capi.desc_from_config(cfg, max_seq_len=max_seq))
ctx.upload_all(synth.make_tensors(cfg, seed=7, share_layers=True))
ok = True
res = {"layers": cfg.n_layers, "new_tokens": M, "temperature": T, "topp": P, "max_seq_len": max_seq, "reps": reps, "spec_gemm": opt.gemm, "rows": []}


def sequential(prompts, states):
    ids, after = [], []
    t0 = time.perf_counter()
    for p, s in zip(prompts, states):
        a, sa = ctx.generate(p, 0, M, temperature=T, topp=P, rng_state=s)
        ids.append(a); after.append(sa)
    return time.perf_counter() - t0, ids, after


def batch(prompts, states):
    """flm_generate_batch's loop through the step API, so that the joins and the steps are timed apart -> (whole, the steps alone, ids, states)"""
    reqs = [capi.BatchReq(p, M, T, P, rng_state=s) for p, s in zip(prompts, states)]
    lay = capi.batch_layout([len(p) + M - 1 for p in prompts], max_seq)
    t0 = time.perf_counter()
    ctx.batch_open(lay)
    ids = [[ctx.batch_join(j, q)[0]] for j, q in enumerate(reqs)]
    t1 = time.perf_counter()
    live = 1
    while live:
        out, live, _ = ctx.batch_step()
        for j in range(len(reqs)):
            if out[j] >= 0:
                ids[j].append(int(out[j]))
    t2 = time.perf_counter()
    after = [ctx.batch_state(j)[0] for j in range(len(reqs))]
    ctx.batch_close()
    return time.perf_counter() - t0, t2 - t1, [np.array(x, np.int32) for x in ids], after


def fan(prompt, states):
    t0 = time.perf_counter()
    ids, after = ctx.generate_n(prompt, 0, M, states=states, temperature=T, topp=P)
    return time.perf_counter() - t0, ids, after


def first_tokens(prompts, states, budget):
    """the time until every request has its token 0: budget None = n serial joins, else admit x n and pass(budget) until nobody fills -> (seconds, passes, token 0s)"""
    reqs = [capi.BatchReq(p, M, T, P, rng_state=s) for p, s in zip(prompts, states)]
    lay = capi.batch_layout([len(p) + M - 1 for p in prompts], max_seq)
    first = [-1] * len(reqs)
    passes = 0
    t0 = time.perf_counter()
    ctx.batch_open(lay)
    if budget is None:
        first = [ctx.batch_join(j, q)[0] for j, q in enumerate(reqs)]
        passes = len(reqs)
    else:
        for j, q in enumerate(reqs):
            ctx.batch_admit(j, q)
        filling = 1
        while filling:
            out, _, _, filling = ctx.batch_pass(budget)
            passes += 1
            for j in range(len(reqs)):
                if first[j] < 0 and out[j] >= 0:
                    first[j] = int(out[j])
    dt = time.perf_counter() - t0
    ctx.batch_close()
    return dt, passes, first


def whole_call(prompts, states, rows):
    reqs = [capi.BatchReq(p, M, T, P, rng_state=s) for p, s in zip(prompts, states)]
    ctx.set_option("batch_rows", rows)
    t0 = time.perf_counter()
    ids, after = ctx.generate_batch(reqs)
    dt = time.perf_counter() - t0
    ctx.set_option("batch_rows", -1)
    return dt, ids, after, ctx.query("batch_passes")


if opt.admit:
    FORMS = (("joins", None), ("pass0", 0), ("pass256", 256))
    ROWS = (-1, 0, 256)
    ctx.set_option("spec_gemm", opt.gemm)
    for n_prompt in PROMPTS:
        for n in NS:
            rows = n * (n_prompt + M - 1)
            if rows > max_seq:
                res["rows"].append({"prompt": n_prompt, "n": n, "fits": False, "rows_needed": rows})
                print(f"prompt {n_prompt:4d}  n {n:2d}  not run: the slots need {rows} rows, max_seq_len is {max_seq}", flush=True)
                continue
            prompts = [np.concatenate([[1], np.random.default_rng(1000 * n_prompt + j).integers(0, cfg.vocab_size, n_prompt - 1)]).astype(np.int32) for j in range(n)]
            states = [1234 + j for j in range(n)]
            t0s = {k: [] for k, _ in FORMS}; calls = {r: [] for r in ROWS}; npass = {}; cpass = {}
            want = None
            for r in range(reps + 1):                      # (round 0 warms every form)
                for k, budget in FORMS:
                    dt, npass[k], first = first_tokens(prompts, states, budget)
                    if r:
                        t0s[k].append(dt)
                    want0 = first if k == "joins" else want0
                    ok = ok and first == want0
                for rw in ROWS:
                    dt, ids, after, cpass[rw] = whole_call(prompts, states, rw)
                    if r:
                        calls[rw].append(dt)
                    if want is None:
                        want = (ids, after)
                    ok = ok and all(np.array_equal(a, b) for a, b in zip(ids, want[0])) and after == want[1] and [int(a[0]) for a in ids] == want0
            tokens = sum(len(w) for w in want[0])
            med = lambda v: float(np.median(v)); spread = lambda v: float(max(v) - min(v))
            row = {"prompt": n_prompt, "n": n, "fits": True, "tokens": tokens}
            for k, _ in FORMS:
                row.update({f"token0_{k}_ms": round(med(t0s[k]) * 1e3, 2), f"token0_{k}_spread_ms": round(spread(t0s[k]) * 1e3, 2), f"token0_{k}_passes": npass[k]})
            for rw in ROWS:
                tag = {-1: "default", 0: "rows0", 256: "rows256"}[rw]
                row.update({f"call_{tag}_tok_s": round(tokens / med(calls[rw]), 1), f"call_{tag}_ms": round(med(calls[rw]) * 1e3, 2), f"call_{tag}_spread_ms": round(spread(calls[rw]) * 1e3, 2), f"call_{tag}_passes": cpass[rw]})
            res["rows"].append(row)
            print(f"prompt {n_prompt:4d}  n {n:2d}  token 0 for all: {n} joins {row['token0_joins_ms']:8.2f} ms (spread {row['token0_joins_spread_ms']})  pass(0) {row['token0_pass0_ms']:8.2f} ms (spread {row['token0_pass0_spread_ms']}, "
                  f"{npass['pass0']} pass)  pass(256) {row['token0_pass256_ms']:8.2f} ms (spread {row['token0_pass256_spread_ms']}, {npass['pass256']} passes)   whole call: batch_rows -1 {row['call_default_tok_s']:8.1f} tok/s ({cpass[-1]} passes)  "
                  f"0 {row['call_rows0_tok_s']:8.1f} tok/s ({cpass[0]})  256 {row['call_rows256_tok_s']:8.1f} tok/s ({cpass[256]})  (spreads {row['call_default_spread_ms']} / {row['call_rows0_spread_ms']} / {row['call_rows256_spread_ms']} ms)", flush=True)
    res["admit"] = True
    res["ids_and_states_agree"] = bool(ok)
    res["fallback"] = ctx.query("fallback")
    print(json.dumps(res), flush=True)
    ctx.close()
    sys.exit(0 if ok else 1)

for n_prompt in PROMPTS:
    for n in NS:
        rows = n * (n_prompt + M - 1)
        if rows > max_seq:
            res["rows"].append({"prompt": n_prompt, "n": n, "fits": False, "rows_needed": rows})
            print(f"prompt {n_prompt:4d}  n {n:2d}  not run: the slots need {rows} rows, max_seq_len is {max_seq}", flush=True)
            continue
        prompts = [np.concatenate([[1], np.random.default_rng(1000 * n_prompt + j).integers(0, cfg.vocab_size, n_prompt - 1)]).astype(np.int32) for j in range(n)]
        states = [1234 + j for j in range(n)]
        fan_fits = n_prompt + n * (M - 1) <= max_seq
        ts = {"seq": [], "batch": [], "steps": [], "fan": []}
        for r in range(reps + 1):                          # (round 0 warms every form)
            ctx.set_option("spec_gemm", 0)
            dt, want, want_after = sequential(prompts, states)
            if r:
                ts["seq"].append(dt)
            ctx.set_option("spec_gemm", opt.gemm)
            dt, dsteps, got, after = batch(prompts, states)
            ok = ok and all(np.array_equal(a, b) for a, b in zip(got, want)) and after == want_after
            if r:
                ts["batch"].append(dt); ts["steps"].append(dsteps)
            if fan_fits:
                dt, _, _ = fan(prompts[0], states)
                if r:
                    ts["fan"].append(dt)
        ctx.set_option("spec_gemm", 0)
        tokens = sum(len(w) for w in want)
        med = {k: float(np.median(v)) for k, v in ts.items() if v}
        spread = {k: float(max(v) - min(v)) for k, v in ts.items() if v}
        row = {"prompt": n_prompt, "n": n, "fits": True, "tokens": tokens, "sequential_tok_s": round(tokens / med["seq"], 1), "batch_tok_s": round(tokens / med["batch"], 1),
               "ratio": round(med["seq"] / med["batch"], 2), "batch_ms": round(med["batch"] * 1e3, 2), "batch_spread_ms": round(spread["batch"] * 1e3, 2),
               "sequential_ms": round(med["seq"] * 1e3, 2), "sequential_spread_ms": round(spread["seq"] * 1e3, 2),
               "step_ms": round(med["steps"] * 1e3 / (M - 1), 3), "step_spread_ms": round(spread["steps"] * 1e3 / (M - 1), 3), "joins_ms": round((med["batch"] - med["steps"]) * 1e3, 2)}
        line = (f"prompt {n_prompt:4d}  n {n:2d}  sequential {row['sequential_tok_s']:8.1f} tok/s  flm_generate_batch {row['batch_tok_s']:8.1f} tok/s  ratio {row['ratio']:5.2f}  "
                f"({row['step_ms']} ms per step, spread {row['step_spread_ms']}; the {n} joins {row['joins_ms']} ms)")
        if fan_fits:
            row.update({"generate_n_tok_s": round(tokens / med["fan"], 1), "generate_n_step_ms": round(med["fan"] * 1e3 / M, 3), "generate_n_step_spread_ms": round(spread["fan"] * 1e3 / M, 3)})
            line += f"   flm_generate_n {row['generate_n_tok_s']:8.1f} tok/s  ({row['generate_n_step_ms']} ms per step: the call / {M}, spread {row['generate_n_step_spread_ms']})"
        res["rows"].append(row)
        print(line, flush=True)
res["ids_and_states_agree"] = bool(ok)
res["fallback"] = ctx.query("fallback")
print(json.dumps(res), flush=True)
ctx.close()
sys.exit(0 if ok else 1)
