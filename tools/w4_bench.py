"""W4A8 against int8 on the 32-layer 7B-shaped synthetic model, one GPU: per-phase GEMV times of an INT4 context and of an INT8 context with every "fuse_*" option 0 (the
same launch form), from flm_kernel_times at position 20, each with its bytes (flm_kernel_bytes), achieved bytes/s and share of the 8 TB/s peak; then tokens/s of
decode_greedy over 128 steps for INT4, INT8 per phase and INT8 default (one launch per token), the three alternating, medians of `reps`.
python tools/w4_bench.py [reps] [layers]   -- prints the tables and one JSON line"""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.getcwd())
import numpy as np
import __graft_entry__ as g; g.load_package()
from fast_llama_amd import capi, synth, flmfile as ff

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
layers = int(sys.argv[2]) if len(sys.argv) > 2 else None
PEAK, POS, STEPS = 8e12, 20, 128
FUSE = ("fuse_tail", "fuse_token", "fuse_layer", "fuse_back", "fuse_qkv", "fuse_attn_o", "fuse_ffn")
PHASES = ("qkv", "attn_o", "ffn13", "ffn2", "cls")


def context(qt, per_phase):
    cfg = synth.make_config("7B", qt)
    if layers is not None:
        cfg.n_layers = layers
    ctx = capi.Ctx(capi.desc_from_config(cfg, max_seq_len=1024))
    ctx.upload_all(synth.make_tensors(cfg, seed=7, share_layers=True))
    if per_phase:
        for k in FUSE:
            ctx.set_option(k, 0)
    return ctx


runs = {"int4": context(capi.QT_INT4, False), "int8 per phase": context(ff.QT_INT8, True), "int8 default": context(ff.QT_INT8, False)}
res = {"reps": reps, "layers": runs["int4"].desc.n_layers, "kernels": {}, "tokens_per_s": {}}
print(f"{'phase':8s} {'type':16s} {'us':>9s} {'MB':>9s} {'GB/s':>9s} {'of peak':>8s}")
for name in ("int4", "int8 per phase"):
    ctx = runs[name]
    kt = ctx.kernel_times(POS, iters=5)
    for k in PHASES:
        us, b = kt[k][0], ctx.kernel_bytes(k, POS)
        rate = b / (us * 1e-6) if us > 0 else 0.0
        res["kernels"][f"{name}/{k}"] = {"us": round(us, 2), "bytes": b, "GBps": round(rate / 1e9, 1)}
        print(f"{k:8s} {name:16s} {us:9.2f} {b / 1e6:9.2f} {rate / 1e9:9.1f} {rate / PEAK:8.1%}")
prompt = np.array([1, 17, 200, 45, 9], dtype=np.int32)
times = {k: [] for k in runs}
for r in range(reps + 1):                                   # the first round warms every form
    for name, ctx in runs.items():
        ctx.reset_kv()
        first = ctx.forward_argmax(prompt, 0)
        t0 = time.perf_counter()
        ctx.decode_greedy(first, len(prompt), STEPS)        # (returns behind a device synchronise: the ids are on the host)
        if r:
            times[name].append(time.perf_counter() - t0)
print(f"\ndecode_greedy, {STEPS} steps, median of {reps} (min .. max)")
for name, t in times.items():
    tps = [STEPS / x for x in t]
    res["tokens_per_s"][name] = round(statistics.median(tps), 1)
    print(f"{name:16s} {statistics.median(tps):8.1f} tokens/s  ({min(tps):.1f} .. {max(tps):.1f})")
print(json.dumps(res))
