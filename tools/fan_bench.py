"""Parallel sampling on the 32-layer 7B-shaped int8 synthetic model: aggregate tokens/s of flm_generate_n (n completions of one prompt, one batch per pass over the
weights) against n SEQUENTIAL flm_generate calls timed in the same run -- the path a caller had before.  A 16-token and a 512-token prompt, 64 new tokens per sequence,
n = 4, 8, 16, temperature 1.0 / top-p 0.9, sequence j at state 1234 + j.  Both forms are warmed once and timed `reps` times, alternating; the medians are reported.
flm_generate_n runs with "spec_gemm" 0 (the 64 x 64 tiles: the default, the table's headline rate and ratio) and 1 (the skinny kernel, beside it).
Exits non-zero unless every sequence's ids and final state equal flm_generate's.  Prints the table and one JSON line.
python tools/fan_bench.py [--new M] [--temperature T] [--topp P] [reps] [layers]"""
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
ap.add_argument("reps", nargs="?", type=int, default=3)
ap.add_argument("layers", nargs="?", type=int, default=None)
opt = ap.parse_args()
M, T, P, reps = opt.new, opt.temperature, opt.topp, opt.reps
NS, PROMPTS = (4, 8, 16), (16, 512)
cfg = synth.make_config(opt.target, ff.QT_INT8)
if opt.layers is not None:
    cfg.n_layers = opt.layers
max_seq = 2048                                             # 512 + 16 * 63 = 1520 rows for the largest fan
ctx = capi.Ctx(capi.desc_from_config(cfg, max_seq_len=max_seq))
ctx.upload_all(synth.make_tensors(cfg, seed=7, share_layers=True))
ok = True
res = {"layers": cfg.n_layers, "new_tokens": M, "temperature": T, "topp": P, "max_seq_len": max_seq, "reps": reps, "rows": []}


def sequential(prompt, states):
    ids, after = [], []
    t0 = time.perf_counter()
    for s in states:
        a, sa = ctx.generate(prompt, 0, M, temperature=T, topp=P, rng_state=s)
        ids.append(a); after.append(sa)
    return time.perf_counter() - t0, ids, after


def fan(prompt, states):
    t0 = time.perf_counter()
    ids, after = ctx.generate_n(prompt, 0, M, states=states, temperature=T, topp=P)
    return time.perf_counter() - t0, ids, after


for n_prompt in PROMPTS:
    prompt = np.concatenate([[1], np.random.default_rng(n_prompt).integers(0, cfg.vocab_size, n_prompt - 1)]).astype(np.int32)
    for n in NS:
        states = [1234 + j for j in range(n)]
        ts = {"seq": [], "fan_tiles": [], "fan_skinny": []}
        want = None
        for r in range(reps + 1):                          # (round 0 warms every form)
            dt, want, want_after = sequential(prompt, states)
            if r:
                ts["seq"].append(dt)
            for name, gemm in (("fan_tiles", 0), ("fan_skinny", 1)):
                ctx.set_option("spec_gemm", gemm)
                dt, got, after = fan(prompt, states)
                agree = all(np.array_equal(a, b) for a, b in zip(got, want)) and after == want_after
                ok = ok and agree
                if r:
                    ts[name].append(dt)
        ctx.set_option("spec_gemm", 0)
        tokens = sum(len(w) for w in want)
        med = {k: float(np.median(v)) for k, v in ts.items()}
        row = {"prompt": n_prompt, "n": n, "tokens": tokens, "sequential_tok_s": round(tokens / med["seq"], 1), "generate_n_tok_s": round(tokens / med["fan_tiles"], 1),
               "ratio": round(med["seq"] / med["fan_tiles"], 2), "skinny_tok_s": round(tokens / med["fan_skinny"], 1), "skinny_ratio": round(med["seq"] / med["fan_skinny"], 2),
               "step_ms": round(med["fan_tiles"] * 1e3 / M, 3), "skinny_step_ms": round(med["fan_skinny"] * 1e3 / M, 3)}
        res["rows"].append(row)
        print(f"prompt {n_prompt:4d}  n {n:2d}  sequential {row['sequential_tok_s']:8.1f} tok/s  flm_generate_n {row['generate_n_tok_s']:8.1f} tok/s  ratio {row['ratio']:5.2f}  "
              f"({row['step_ms']} ms per step)   spec_gemm 1: {row['skinny_tok_s']:8.1f} tok/s  ratio {row['skinny_ratio']:5.2f}  ({row['skinny_step_ms']} ms per step)", flush=True)
res["ids_and_states_agree"] = bool(ok)
res["fallback"] = ctx.query("fallback")
print(json.dumps(res), flush=True)
ctx.close()
sys.exit(0 if ok else 1)
