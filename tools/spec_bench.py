"""Greedy draft-and-verify on the 32-layer 7B-shaped int8 synthetic model: what a verify pass costs against a decode token, and what the loop delivers.
   (a) flm_decode_greedy: tokens/s for N tokens behind a prompt (wall time; the ids are the reference for everything below)
   (b) flm_verify_greedy fed the TRUE continuation as drafts, k = 4, 7 and 15 (batches of B = 5, 8, 16 rows: every draft is accepted, the call is one pass): the pass time
       t_B alone, median of `reps` calls, for "spec_gemm" 1 (the skinny kernel) and 0 (the 64 x 64 tiles; measured twice, in front of and behind the skinny runs: the spread
       is printed beside it); t_B / t_1 is the break-even number of ids per step
   (c) flm_generate_lookup on a prompt that repeats a block of its own continuation: tokens/s, accepted / steps
Exits non-zero unless the ids of (a), (b) and (c) agree.  Prints one JSON line.  python tools/spec_bench.py [N] [reps] [layers]"""
import json
import os
import sys
import time

sys.path.insert(0, os.getcwd())
import numpy as np
import __graft_entry__ as g; g.load_package()
from fast_llama_amd import capi, synth, flmfile as ff

N = int(sys.argv[1]) if len(sys.argv) > 1 else 128
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 9
cfg = synth.make_config("7B", ff.QT_INT8)
if len(sys.argv) > 3:
    cfg.n_layers = int(sys.argv[3])
ctx = capi.Ctx(capi.desc_from_config(cfg, max_seq_len=1024))
ctx.upload_all(synth.make_tensors(cfg, seed=7, share_layers=True))
seed = np.concatenate([[1], np.random.default_rng(1).integers(0, cfg.vocab_size, 15)]).astype(np.int32)
ok = True

# (a) the decode loop
first = ctx.forward_argmax(seed, 0)
ctx.decode_greedy(first, len(seed), 8)                    # warm
t0 = time.perf_counter(); ids = ctx.decode_greedy(first, len(seed), N); dt_a = time.perf_counter() - t0
t1_ms = dt_a * 1e3 / N
res = {"layers": cfg.n_layers, "N": N, "decode_tok_s": round(N / dt_a, 1), "t1_ms": round(t1_ms, 4)}

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
print(json.dumps(res), flush=True)
ctx.close()
sys.exit(0 if ok else 1)
