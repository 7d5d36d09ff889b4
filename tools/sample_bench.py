#!/usr/bin/env python3
"""Sampled decoding on the device against greedy and against the host-sampled loop it replaces, on bench.py's model (LLaMA2-7B-shaped int8, synthetic portable
weights, 32 layers by default).  Prints one JSON line:
  * tokens/s of flm_decode_sample at -t 1 -p 0.9 with seed 0 (the CLI's: coin 0) and with a non-zero seed, and of flm_decode_greedy -- wall time of the call,
    K tokens after a 9-token prompt, median of R runs, all measured in the same process;
  * the old loop: flm_forward of one token + host Sampler (host/sampler.cpp) per token, same model, same parameters;
  * with --ops: op_sample (k_sample_advance) wall time per call on peaked / medium / flat 32 000-entry logits (the kernel's own time: run under
    rocprofv3 --kernel-trace --stats);
  * with --shape (and nothing else): the shaped loop against the unshaped one on the same context -- tokens/s of flm_generate at -t 1 -p 0.9, seed 1234 (the sampled loop as
    it was before the shaping stage existed: the same launches), of flm_generate_ex with a control that changes nothing (a bias of +0: the stage's launch on top of the same
    sampler work) and with a full set of controls (top-k 40, min-p 0.05, repeat penalty 1.1 over 64 ids, a bias and a ban: the sampler then sorts fewer candidates), the
    runs alternating; the stage's own duration: k_shape_logits in a rocprofv3 --kernel-trace --stats run of this command;
  * with --constraint (and nothing else): the shaped token with and without an armed automaton, in the same run -- flm_generate_ex with a bias of +0 (the stage's launch,
    no mask) against the same call armed with a Dfa.from_choices automaton whose every state on the way allows half the vocabulary (the even ids), alternating;
  * with --logprobs (and nothing else): flm_generate_ex with a bias of +0 (the shaped form) disarmed, and armed with flm_logprobs_arm at top_n 0, 5 and 20 from the raw and
    from the shaped row, alternating; the stage's own duration per launch from HIP events (flm_logprob_stage_time) and the sampler launch it follows (flm_kernel_times'
    class "argmax" on the sampled form is the greedy argmax: the sampled launch's own figure is op_sample's, --ops).  On a library without the feature (the parent commit
    through FLM_GPU_LIB) only the disarmed figure is measured: the same command gives the pair that shows the disarmed path did not move;
  * with --stop (and nothing else): the shaped token (flm_generate_ex with a bias of +0) with no stop rules installed and with the largest rule set installed -- 64 ids
    and 16 sequences of 32 ids, none of which ever fires --, alternating, every run's own figure listed (`runs_ms`) so that two commands' spreads can be compared.  On a
    library without the feature (the parent commit through FLM_GPU_LIB) only the rule-free figure is measured: (i) the parent, (ii) this commit without rules, (iii) with;
  * with --entropy (and nothing else): the entropy-driven samplers in one process -- tokens/s of flm_generate_ex with top-k 40 alone (the shaped form: the baseline), with
    flm_entropy_set at typical_p 0.5 and at Mirostat v2 (tau 5, eta 0.1) on top of the same top-k, the runs alternating, and of the host loop a caller needs without the
    feature (flm_forward's logits over the bus, fh_shape, fh_entropy, fh_sample_state, fh_mirostat_update per token); the same with every control neutral (the stages on the
    classifier's whole row: 32 000 live candidates)."""
import argparse
import importlib.util
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as graft  # noqa: E402

graft.load_package()
from fast_llama_amd import capi, flmfile as ff, synth  # noqa: E402
from sample_util import host_lib, host_sample, logits_case  # noqa: E402


def _bench_module():
    spec = importlib.util.spec_from_file_location("flm_bench", os.path.join(ROOT, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-steps", type=int, default=32)
    ap.add_argument("--ops", action="store_true", help="also time op_sample on peaked / medium / flat logits")
    ap.add_argument("--ops-only", action="store_true")
    ap.add_argument("--shape", action="store_true", help="time the shaped loop (flm_generate_ex) against the unshaped one (flm_generate) on the same context, nothing else")
    ap.add_argument("--constraint", action="store_true", help="time the shaped token with and without an armed automaton (half the vocabulary allowed), nothing else")
    ap.add_argument("--logprobs", action="store_true", help="time the shaped token disarmed and armed for per-token log-probabilities (top_n 0 / 5 / 20, raw / shaped), nothing else")
    ap.add_argument("--stop", action="store_true", help="time the shaped token with no stop rules and with the largest rule set (64 ids, 16 sequences of 32) that never fires, nothing else")
    ap.add_argument("--entropy", action="store_true", help="time flm_generate_ex with top-k alone, with typical sampling and with Mirostat v2 set, and the host loop, nothing else")
    args = ap.parse_args()
    out = {}
    if args.entropy:
        from entropy_util import host_loop
        cfg = synth.make_config("7B", ff.QT_INT8)
        cfg.n_layers = args.layers
        ctx = capi.Ctx(capi.desc_from_config(cfg), device=0)
        _bench_module().upload_synthetic(ctx, cfg)
        V, K = cfg.vocab_size, args.steps
        prompt = np.array([1] + [int(x) for x in (np.arange(1, 9) * 7919) % V], np.int32)
        topk = capi.Sampling(temperature=1.0, topp=0.9, top_k=40)
        noop = capi.Sampling(temperature=1.0, topp=0.9, bias={11: 0.0})
        typ, miro = capi.Entropy(typical_p=0.5), capi.Entropy(mirostat=2, tau=5.0, eta=0.1)

        def under(ent, s):
            def run():
                ctx.entropy_set(ent)
                r = ctx.generate_ex(prompt, 0, K, s, rng_state=1234)
                ctx.entropy_set(None)
                return r
            return run
        runs = {"topk": under(None, topk), "topk_typical": under(typ, topk), "topk_mirostat": under(miro, topk),
                "noop": under(None, noop), "typical": under(typ, noop), "mirostat": under(miro, noop)}
        ts = {k: [] for k in runs}
        for rep in range(args.reps + 1):
            for name, fn in runs.items():                # alternating: every form sees the same machine
                ctx.sync(); t0 = time.perf_counter(); ids = fn()[0]; dt = time.perf_counter() - t0
                assert len(ids) == K
                if rep:
                    ts[name].append(dt)
        for name in runs:
            med = float(np.median(ts[name]))
            out[f"{name}_tok_s"] = round(K / med, 1)
            out[f"{name}_spread_ms"] = round((max(ts[name]) - min(ts[name])) * 1e3, 2)
        for name, base in (("topk_typical", "topk"), ("topk_mirostat", "topk"), ("typical", "noop"), ("mirostat", "noop")):
            out[f"{name}_extra_us_per_token"] = round((np.median(ts[name]) - np.median(ts[base])) / K * 1e6, 1)
        H = host_lib()
        for name, ent in (("typical", typ), ("mirostat", miro)):
            hs = []
            for _ in range(2):
                ctx.sync(); t0 = time.perf_counter()
                host_loop(ctx, H, prompt, args.host_steps, topk, ent, 1234)
                hs.append(time.perf_counter() - t0)
            out[f"host_loop_topk_{name}_tok_s"] = round(args.host_steps / float(np.median(hs)), 1)
        out["tokens_per_call"] = K; out["prompt_tokens"] = len(prompt); out["layers"] = args.layers
        ctx.close()
        print(json.dumps(out), flush=True)
        return
    if args.stop:
        cfg = synth.make_config("7B", ff.QT_INT8)
        cfg.n_layers = args.layers
        ctx = capi.Ctx(capi.desc_from_config(cfg), device=0)
        _bench_module().upload_synthetic(ctx, cfg)
        V, K = cfg.vocab_size, args.steps
        prompt = np.array([1] + [int(x) for x in (np.arange(1, 9) * 7919) % V], np.int32)
        noop = capi.Sampling(temperature=1.0, topp=0.9, bias={11: 0.0})
        have = hasattr(capi.lib(), "flm_stop_set")
        plain = [int(x) for x in ctx.generate_ex(prompt, 0, K, noop, rng_state=1234)[0]]
        runs = {"no_rules": lambda: ctx.generate_ex(prompt, 0, K, noop, rng_state=1234)}
        if have:
            never = [t for t in range(V - 1, 0, -1) if t not in plain][:65]      # 64 ids that do not occur, and one more that every sequence ends in
            big = capi.StopRules(never[:64], [[plain[(s + j) % K] for j in range(31)] + [never[64]] for s in range(16)])

            def with_rules():
                ctx.stop_set(big)
                r = ctx.generate_ex(prompt, 0, K, noop, rng_state=1234)
                ctx.stop_set(None)
                return r
            runs["largest_rules"] = with_rules
        ts = {k: [] for k in runs}
        for rep_i in range(args.reps + 1):
            for name, fn in runs.items():                # alternating: both forms see the same machine
                ctx.sync(); t0 = time.perf_counter(); ids = fn()[0]; dt = time.perf_counter() - t0
                assert [int(x) for x in ids] == plain        # rules that never fire change no id
                if rep_i:
                    ts[name].append(dt)
        for name in runs:
            med = float(np.median(ts[name]))
            out[f"{name}_us_per_token"] = round(med / K * 1e6, 2)
            out[f"{name}_runs_ms"] = [round(x * 1e3, 3) for x in ts[name]]
        if have:
            out["rules_extra_us_per_token"] = round((np.median(ts["largest_rules"]) - np.median(ts["no_rules"])) / K * 1e6, 2)
        out["tokens_per_call"] = K; out["prompt_tokens"] = len(prompt); out["layers"] = args.layers; out["feature_present"] = bool(have)
        ctx.close()
        print(json.dumps(out), flush=True)
        return
    if args.logprobs:
        cfg = synth.make_config("7B", ff.QT_INT8)
        cfg.n_layers = args.layers
        ctx = capi.Ctx(capi.desc_from_config(cfg), device=0)
        _bench_module().upload_synthetic(ctx, cfg)
        V, K = cfg.vocab_size, args.steps
        prompt = np.array([1] + [int(x) for x in (np.arange(1, 9) * 7919) % V], np.int32)
        noop = capi.Sampling(temperature=1.0, topp=0.9, bias={11: 0.0})
        have = hasattr(capi.lib(), "flm_logprobs_arm")

        def armed(top_n, source):
            def run():
                ctx.logprobs_arm(top_n, source)
                r = ctx.generate_ex(prompt, 0, K, noop, rng_state=1234)
                ctx.logprobs_arm(-1)
                return r
            return run
        runs = {"disarmed": lambda: ctx.generate_ex(prompt, 0, K, noop, rng_state=1234)}
        if have:
            for source in ("raw", "shaped"):
                for top_n in (0, 5, 20):
                    runs[f"armed_{source}_top{top_n}"] = armed(top_n, source)
        ts = {k: [] for k in runs}
        ids = {}
        for rep in range(args.reps + 1):
            for name, fn in runs.items():                # alternating: every form sees the same machine
                ctx.sync(); t0 = time.perf_counter(); ids[name] = fn()[0]; dt = time.perf_counter() - t0
                if rep:
                    ts[name].append(dt)
        assert all(list(v) == list(ids["disarmed"]) for v in ids.values())      # arming changes no id
        base = float(np.median(ts["disarmed"]))
        for name in runs:
            med = float(np.median(ts[name]))
            out[f"{name}_tok_s"] = round(K / med, 1)
            out[f"{name}_spread_ms"] = round((max(ts[name]) - min(ts[name])) * 1e3, 2)
            if name != "disarmed":
                out[f"{name}_extra_us_per_token"] = round((med - base) / K * 1e6, 1)
                out[f"{name}_share_of_token"] = round((med - base) / base, 4)
        if have:
            for source in ("raw", "shaped"):
                for top_n in (0, 5, 20):
                    ctx.logprobs_arm(top_n, source)
                    ctx.generate_ex(prompt, 0, K, noop, rng_state=1234)
                    out[f"stage_{source}_top{top_n}_us"] = round(ctx.logprob_stage_time(50), 2)
            ctx.logprobs_arm(-1)
        out["tokens_per_call"] = K; out["prompt_tokens"] = len(prompt); out["layers"] = args.layers; out["feature_present"] = bool(have)
        ctx.close()
        print(json.dumps(out), flush=True)
        return
    if args.constraint:
        cfg = synth.make_config("7B", ff.QT_INT8)
        cfg.n_layers = args.layers
        ctx = capi.Ctx(capi.desc_from_config(cfg), device=0)
        _bench_module().upload_synthetic(ctx, cfg)
        V, K = cfg.vocab_size, args.steps
        prompt = np.array([1] + [int(x) for x in (np.arange(1, 9) * 7919) % V], np.int32)
        # one choice of K + 1 characters, every even id spells one character: states 0 .. K allow the V / 2 even ids each
        dfa = capi.Dfa.from_choices(["a" if i % 2 == 0 and i != 2 else "" for i in range(V)], ["a" * (K + 1)], end_id=2)
        ctx.constraint_set(dfa)
        noop = capi.Sampling(temperature=1.0, topp=0.9, bias={11: 0.0})

        def armed():
            ctx.constraint_arm(0)
            r = ctx.generate_ex(prompt, 0, K, noop, rng_state=1234)
            ctx.constraint_arm(-1)
            return r
        runs = {"shaped_unmasked": lambda: ctx.generate_ex(prompt, 0, K, noop, rng_state=1234), "shaped_masked": armed}
        ts = {k: [] for k in runs}
        ids = {}
        for rep in range(args.reps + 1):
            for name, fn in runs.items():                # alternating: both forms see the same machine
                ctx.sync(); t0 = time.perf_counter(); ids[name] = fn()[0]; dt = time.perf_counter() - t0
                if rep:
                    ts[name].append(dt)
        assert len(ids["shaped_masked"]) == K and all(int(x) % 2 == 0 for x in ids["shaped_masked"])
        for name in runs:
            med = float(np.median(ts[name]))
            out[f"{name}_tok_s"] = round(K / med, 1)
            out[f"{name}_ms_per_call"] = round(med * 1e3, 2)
            out[f"{name}_spread_ms"] = round((max(ts[name]) - min(ts[name])) * 1e3, 2)
        out["mask_extra_us_per_token"] = round((np.median(ts["shaped_masked"]) - np.median(ts["shaped_unmasked"])) / K * 1e6, 1)
        out["tokens_per_call"] = K; out["allowed_ids_per_state"] = int(dfa.edges(0)[0].size); out["dfa_edges"] = dfa.n_edges
        ctx.close()
        print(json.dumps(out), flush=True)
        return
    if args.shape:
        cfg = synth.make_config("7B", ff.QT_INT8)
        cfg.n_layers = args.layers
        ctx = capi.Ctx(capi.desc_from_config(cfg), device=0)
        _bench_module().upload_synthetic(ctx, cfg)
        prompt = np.array([1] + [int(x) for x in (np.arange(1, 9) * 7919) % cfg.vocab_size], np.int32)
        K = args.steps
        noop = capi.Sampling(temperature=1.0, topp=0.9, bias={11: 0.0})
        full = capi.Sampling(temperature=1.0, topp=0.9, top_k=40, min_p=0.05, repeat_penalty=1.1, penalty_last_n=64, bias={3: 1.0, 7: -np.inf})
        runs = {"unshaped": lambda: ctx.generate(prompt, 0, K, temperature=1.0, topp=0.9, rng_state=1234),
                "shaped_noop": lambda: ctx.generate_ex(prompt, 0, K, noop, rng_state=1234),
                "shaped_full": lambda: ctx.generate_ex(prompt, 0, K, full, rng_state=1234)}
        ts = {k: [] for k in runs}
        ids = {}
        for rep in range(args.reps + 1):
            for name, fn in runs.items():                # alternating: the three forms see the same machine
                ctx.sync(); t0 = time.perf_counter(); ids[name] = fn()[0]; dt = time.perf_counter() - t0
                if rep:
                    ts[name].append(dt)
        assert list(ids["unshaped"]) == list(ids["shaped_noop"]) and len(ids["shaped_full"]) == K
        for name in runs:
            med = float(np.median(ts[name]))
            out[f"{name}_tok_s"] = round(K / med, 1)
            out[f"{name}_ms_per_call"] = round(med * 1e3, 2)
            out[f"{name}_spread_ms"] = round((max(ts[name]) - min(ts[name])) * 1e3, 2)
        out["shaped_noop_extra_us_per_token"] = round((np.median(ts["shaped_noop"]) - np.median(ts["unshaped"])) / K * 1e6, 1)
        out["shaped_full_extra_us_per_token"] = round((np.median(ts["shaped_full"]) - np.median(ts["unshaped"])) / K * 1e6, 1)
        out["tokens_per_call"] = K; out["prompt_tokens"] = len(prompt); out["shaped_tokens"] = ctx.query("shaped_tokens")
        ctx.close()
        print(json.dumps(out), flush=True)
        return
    if not args.ops_only:
        cfg = synth.make_config("7B", ff.QT_INT8)
        cfg.n_layers = args.layers
        ctx = capi.Ctx(capi.desc_from_config(cfg), device=0)
        _bench_module().upload_synthetic(ctx, cfg)
        prompt = np.array([1] + [int(x) for x in (np.arange(1, 9) * 7919) % cfg.vocab_size], np.int32)
        first = ctx.forward_argmax(prompt, 0)
        pos, K = len(prompt), args.steps

        def timed(fn):
            ts = []
            for _ in range(args.reps + 1):
                ctx.sync(); t0 = time.perf_counter(); fn(); ts.append(time.perf_counter() - t0)
            return K / float(np.median(ts[1:]))
        out["greedy_tok_s"] = round(timed(lambda: ctx.decode_greedy(first, pos, K)), 1)
        out["greedy_device_tok_s"] = round(K / (np.median([ctx.decode_timed(first, pos, K) for _ in range(args.reps)]) / 1e3), 1)
        out["sampled_seed0_tok_s"] = round(timed(lambda: ctx.decode_sample(first, pos, K, 1.0, 0.9, 0)), 1)
        out["sampled_seed1234_tok_s"] = round(timed(lambda: ctx.decode_sample(first, pos, K, 1.0, 0.9, 1234)), 1)
        out["sampled_seed1234_p1_tok_s"] = round(timed(lambda: ctx.decode_sample(first, pos, K, 1.0, 1.0, 1234)), 1)
        H = host_lib()
        for name, seed in (("seed0", 0), ("seed1234", 1234)):
            ts = []
            for _ in range(3):
                tok, s = first, seed
                ctx.sync(); t0 = time.perf_counter()
                for i in range(args.host_steps):
                    lg = ctx.forward(np.array([tok], np.int32), pos + i)
                    tok, s = host_sample(H, lg, 1.0, 0.9, s)
                ts.append(time.perf_counter() - t0)
            out[f"host_loop_{name}_tok_s"] = round(args.host_steps / float(np.median(ts)), 1)
        out["sampled_vs_greedy"] = round(out["sampled_seed0_tok_s"] / out["greedy_tok_s"], 4)
        ctx.close()
    if args.ops or args.ops_only:
        H = host_lib()
        for kind, std in (("peaked", 8), ("medium", 3), ("flat", 1)):
            lg = (np.random.default_rng(3).standard_normal(32000) * std).astype(np.float32)
            for seed in (0, 1234):
                capi.op_sample(lg, 1.0, 0.9, seed)
                t0 = time.perf_counter()
                for _ in range(20):
                    capi.op_sample(lg, 1.0, 0.9, seed)
                out[f"op_{kind}_seed{seed}_call_us"] = round((time.perf_counter() - t0) / 20 * 1e6, 1)
            t0 = time.perf_counter()
            for _ in range(20):
                host_sample(H, lg, 1.0, 0.9, 1234)
            out[f"host_sampler_{kind}_us"] = round((time.perf_counter() - t0) / 20 * 1e6, 1)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
