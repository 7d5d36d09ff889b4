"""flm_score_tokens against the way the same figures are obtained without it, on the 32-layer 7B-shaped int8 synthetic model at n = 512, pos = 0:
   batched   one flm_score_tokens call (wall time, median of `reps`)
   loop      flm_forward of one token per position + the host restatement of the row statistics (lib/libflm_host.so fh_score_row) on the logits that come back;
             timed over the first `prefix` positions and scaled to n (a position's cost grows with the context only through its attention: the prefix UNDERESTIMATES the loop)
The two must agree bit for bit on the prefix.  Prints one JSON line.  python tools/score_bench.py [n] [prefix] [reps] [layers]"""
import json
import os
import sys
import time

sys.path.insert(0, os.getcwd())
sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
import numpy as np
import __graft_entry__ as g; g.load_package()
from fast_llama_amd import capi, synth, flmfile as ff
from score_util import host_score, next_targets, same_scores

n = int(sys.argv[1]) if len(sys.argv) > 1 else 512
prefix = int(sys.argv[2]) if len(sys.argv) > 2 else 64
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 5
cfg = synth.make_config("7B", ff.QT_INT8)
if len(sys.argv) > 4:
    cfg.n_layers = int(sys.argv[4])
ctx = capi.Ctx(capi.desc_from_config(cfg, max_seq_len=1024))
ctx.upload_all(synth.make_tensors(cfg, seed=7, share_layers=True))
toks = np.concatenate([[1], np.random.default_rng(1).integers(0, cfg.vocab_size, n - 1)]).astype(np.int32)
tg = next_targets(toks)
host_score(np.zeros((1, cfg.vocab_size), np.float32))      # (load the host library outside the timed regions)

ctx.score(toks, 0)                                         # warm
batched = []
for _ in range(reps):
    t0 = time.perf_counter(); sc = ctx.score(toks, 0); batched.append((time.perf_counter() - t0) * 1e3)
ctx.reset_kv()
rows = []
t0 = time.perf_counter()
for i in range(prefix):
    lg = ctx.forward(toks[i:i + 1], i)
    rows.append(host_score(lg, [tg[i]]))
loop_prefix = (time.perf_counter() - t0) * 1e3
same = same_scores(np.concatenate(rows), sc[:prefix])
b = float(np.median(batched))
print(json.dumps({"n": n, "layers": cfg.n_layers, "batched_ms": round(b, 2), "batched_all_ms": [round(x, 2) for x in batched], "loop_prefix": prefix, "loop_prefix_ms": round(loop_prefix, 1),
                  "loop_scaled_ms": round(loop_prefix * n / prefix, 1), "ratio": round(loop_prefix * n / prefix / b, 1), "same_bits_on_prefix": bool(same),
                  "mean_loss": capi.nll(sc)[1], "fallback": ctx.query("fallback")}), flush=True)
ctx.close()
sys.exit(0 if same and b < loop_prefix * n / prefix else 1)
