"""W4A8 against int8 on the 32-layer 7B-shaped synthetic model, one GPU: per-phase GEMV times of an INT4 context and of an INT8 context with every "fuse_*" option 0 (the
same launch form), from flm_kernel_times at position 20, each with its bytes (flm_kernel_bytes), achieved bytes/s and share of the 8 TB/s peak; then tokens/s of
decode_greedy over 128 steps for INT4, INT8 per phase and INT8 default (one launch per token), the three alternating, medians of `reps`.
python tools/w4_bench.py [reps] [layers]   -- prints the tables and one JSON line

python tools/w4_bench.py --verify [reps] [layers]   -- the passes of up to 16 rows instead: the time of one flm_verify_greedy pass at B = 5, 8 and 16 rows (position 20) and
the time per step of flm_generate_batch with 16 slots, for an INT4 context under "spec_gemm" 1 and 0 and an INT8 context under "spec_gemm" 1 and 2 (the split-K skinny
kernel), the four alternating, medians of `reps` with min .. max.  FLM_GPU_LIB picks the library (capi.py): under the build of the commit before k_gemm_q4_skinny the first
row is unpack + int8 skinny, under the build of the commit before k_gemm_q8_skinny_sk the last row is "spec_gemm" 1 once more.
--type int16 (with --verify): the same table for an INT16 context in place of the INT4 one -- k_gemm_q16_skinny under "spec_gemm" 1, the hi / lo-plane tiles under 0; under
the build of the commit before k_gemm_q16_skinny both rows are the tiles.

python tools/w4_bench.py --prefill [reps] [layers]   -- the passes of more than 16 rows (and the tile route of a 16-row one): flm_forward of a 17-, 64-, 130- and 512-token
prompt, flm_score_tokens of 512 tokens with "score_rows" 128 (the classifier in 4 chunks) and a verify pass at B = 16 under "spec_gemm" 0 on an INT4 context, and the
512-token prompt on an INT8 context; medians of `reps` runs with min .. max, a run = the mean over 20 calls.  Under the build of the commit before k_gemm_q4_mfma the INT4
rows are unpack + int8 tiles."""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.getcwd())
import numpy as np
import __graft_entry__ as g; g.load_package()
from fast_llama_amd import capi, synth, flmfile as ff

verify, prefill = "--verify" in sys.argv, "--prefill" in sys.argv
wtype = sys.argv[sys.argv.index("--type") + 1] if "--type" in sys.argv else "int4"
args = [a for i, a in enumerate(sys.argv[1:], 1) if not a.startswith("--") and sys.argv[i - 1] != "--type"]
reps = int(args[0]) if len(args) > 0 else 5
layers = int(args[1]) if len(args) > 1 else None
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


def verify_bench():
    """every timed window ends behind a device synchronise: verify_greedy and generate_batch return ids that are on the host"""
    CALLS, SLOTS, SHORT, LONG = 20, 16, 9, 41
    runs = {}
    wqt = {"int4": capi.QT_INT4, "int16": ff.QT_INT16}[wtype]
    for name, qt, gemm in ((f"{wtype} spec_gemm 1", wqt, 1), (f"{wtype} spec_gemm 0", wqt, 0), ("int8 spec_gemm 1", ff.QT_INT8, 1), ("int8 spec_gemm 2", ff.QT_INT8, 2)):
        runs[name] = context(qt, False); runs[name].set_option("spec_gemm", gemm)
    prompt = (np.arange(POS, dtype=np.int32) * 7 + 1) % 1000
    reqs = lambda n: [capi.BatchReq((np.arange(4, dtype=np.int32) + 11 * s) % 1000 + 1, n) for s in range(SLOTS)]   # noqa: E731
    cases = [f"verify B={b}" for b in (5, 8, 16)] + ["batch step, 16 slots"]
    times = {(n, c): [] for n in runs for c in cases}
    for r in range(reps + 1):                               # the first round warms every form
        for name, ctx in runs.items():
            for b in (5, 8, 16):
                ctx.reset_kv()
                first = ctx.forward_argmax(prompt, 0)
                drafts = (np.arange(b - 1, dtype=np.int32) * 13 + 5) % 1000
                t0 = time.perf_counter()
                for _ in range(CALLS):
                    ctx.verify_greedy(first, drafts, POS)
                times[name, f"verify B={b}"].append((time.perf_counter() - t0) / CALLS)
            t = []
            for n in (SHORT, LONG):                         # the steps between the two lengths: joins and the calls' fixed parts cancel
                ctx.reset_kv()
                t0 = time.perf_counter()
                ctx.generate_batch(reqs(n))
                t.append(time.perf_counter() - t0)
            times[name, cases[-1]].append((t[1] - t[0]) / (LONG - SHORT))
    out = {"reps": reps, "layers": next(iter(runs.values())).desc.n_layers, "lib": os.environ.get("FLM_GPU_LIB", "default"), "us": {}}
    print(f"{'case':22s} {'context':18s} {'median us':>10s} {'min':>9s} {'max':>9s}")
    for c in cases:
        for n in runs:
            t = [x * 1e6 for x in times[n, c][1:]]
            out["us"][f"{c} / {n}"] = [round(statistics.median(t), 1), round(min(t), 1), round(max(t), 1)]
            print(f"{c:22s} {n:18s} {statistics.median(t):10.1f} {min(t):9.1f} {max(t):9.1f}")
    print(json.dumps(out))


def prefill_bench():
    """every timed window ends behind a device synchronise: forward, score and verify_greedy return values that are on the host"""
    CALLS = 20
    int4, int8 = context(capi.QT_INT4, False), context(ff.QT_INT8, False)
    int4.set_option("spec_gemm", 0); int4.set_option("score_rows", 128)
    toks = (np.arange(512, dtype=np.int32) * 7 + 1) % 1000
    drafts = (np.arange(15, dtype=np.int32) * 13 + 5) % 1000

    def verify16():
        int4.verify_greedy(int(toks[POS]), drafts, POS)
    cases = [(f"forward {n} / int4", (lambda n=n: int4.forward(toks[:n], 0))) for n in (17, 64, 130, 512)]
    cases += [("score 512, 4 chunks / int4", lambda: int4.score(toks, 0)), ("verify B=16 spec_gemm 0 / int4", verify16), ("forward 512 / int8", lambda: int8.forward(toks, 0))]
    times = {c: [] for c, _ in cases}
    for r in range(reps + 1):                               # the first round warms every case
        for c, call in cases:
            if c.startswith("verify"):
                int4.reset_kv(); int4.forward(toks[:POS], 0)
            t0 = time.perf_counter()
            for _ in range(CALLS):
                call()
            times[c].append((time.perf_counter() - t0) / CALLS)
    out = {"reps": reps, "layers": int4.desc.n_layers, "lib": os.environ.get("FLM_GPU_LIB", "default"), "us": {}}
    print(f"{'case':32s} {'median us':>10s} {'min':>9s} {'max':>9s}")
    for c, _ in cases:
        t = [x * 1e6 for x in times[c][1:]]
        out["us"][c] = [round(statistics.median(t), 1), round(min(t), 1), round(max(t), 1)]
        print(f"{c:32s} {statistics.median(t):10.1f} {min(t):9.1f} {max(t):9.1f}")
    print(json.dumps(out))


if verify or prefill:
    verify_bench() if verify else prefill_bench()
    sys.exit(0)
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
