"""Call scripts: seeded sequences of C-ABI calls on ONE context, and the CPU oracle's side of them (tests/test_gpu_longlived.py runs them on the GPU, tests/test_callscript_host.py
checks the generator and replays every committed seed on the oracle alone).

A script is a list of JSON-able dicts, so that a failing run can print what it did as a replayable list.  Everything in it is drawn from the seed -- the tokens a decode call
starts from too -- and nothing from what the model answers, so the same seed gives the same script for every model of the same vocabulary:

  {"op": "forward", "kind": "logits" | "argmax" | "sample", "tokens": [...], "pos": p [, "t", "p_top", "state"]}
  {"op": "decode", "kind": "greedy" | "sample", "tok": t, "pos": p, "n": n [, "t", "p_top", "state"]}       (pos below the fill = a rewind: the ABI's `pos` is "tokens in the cache")
  {"op": "reset_decode", "tok": t, "n": n}                   flm_reset_kv, then flm_decode_greedy(tok, 0, n) with no forward in between
  {"op": "set_option", "key": k, "value": v, "prepare": bool}
  {"op": "inject"}                                            option "inject_wait_failure": the next token call falls back and is re-run (at most twice per script, a probation apart)
  {"op": "age", "e": E}                                       option "age_epochs"
  {"op": "kernel_times", "pos": p}                            cache cleared, decode state undefined: the next op is a fresh prompt at 0

"state" of a sampled call is None where the call carries on the state the previous sampled call returned (the interpreter's), else a fresh one."""
import numpy as np

FORWARD_N = (1, 2, 5, 6, 7, 16, 17, 40, 130)        # 5 / 6: flm_forward's token-by-token / batched switch
DECODE_N = (1, 2, 15, 16, 17, 33)                   # the edges of the 16-token graphs
# the structure switches of include/flm_gpu.h that are legal on a live context; under tensor parallelism what a group runs is agreed when the blobs are exchanged, so a script
# there switches only what every rank may switch alone
LIVE_OPTIONS = {"use_graph": (0, 1), "graph_chunks": (0, 1), "fuse_tail": (0, 1), "fuse_token": (0, 1), "fuse_layer": (0, 1), "fuse_back": (0, 1), "gr_edges": (0, 1),
                "back_ao": (0, 1, 2, 3), "attn_split": (0, 1), "use_prefill": (0, 1)}
LIVE_OPTIONS_TP = {"use_graph": (0, 1), "graph_chunks": (0, 1), "use_prefill": (0, 1)}
SAMPLE_PARAMS = ((1.0, 0.9), (0.7, 1.0), (0.0, 0.9), (1.3, 0.5))
PROBATION = 64                                      # tokens a context stays on one kernel per phase after a wait gave up (flm_gpu.hip kFallbackProbation)
MAX_INJECTIONS = 2


def generate(seed, vocab, max_seq=1024, n_layers=2, n_ops=40, world=1, sample_ok=True, age=None):
    """the script of `seed`.  age: None = a third of the seeds age the context once, to just under 2^31; False = never"""
    rng = np.random.default_rng(seed)
    ops, fill, injections, since_inject, pending = [], 0, 0, 10 ** 9, False
    tp = world > 1
    do_age = (seed % 3 == 0) if age is None else bool(age)
    age_at = int(rng.integers(3, max(4, n_ops // 2))) if do_age else -1
    options = LIVE_OPTIONS_TP if tp else LIVE_OPTIONS

    def toks(n):
        return [int(x) for x in rng.integers(1, vocab, n)]

    def sample_args():
        t, p = SAMPLE_PARAMS[int(rng.integers(len(SAMPLE_PARAMS)))]
        return {"t": t, "p_top": p, "state": None if rng.random() < 0.6 else int(rng.integers(1, 1 << 62))}

    def position():
        """where the next call starts: mostly the fill, sometimes below it (0, 1, half, one short)"""
        if fill > 1 and rng.random() < 0.2:
            return int(rng.choice([0, 1, fill // 2, fill - 1]))
        return fill

    def token_call(force_prompt=False):
        nonlocal fill, since_inject, pending
        pos = 0 if force_prompt else position()
        room = max_seq - 1 - pos                                      # (the fill stays below max_seq)
        if room < 1:
            pos = int(rng.choice([0, 1, fill // 2])); room = max_seq - 1 - pos
        if force_prompt or rng.random() < 0.5:
            fits = [n for n in FORWARD_N if n <= room]
            w = np.array([3.0 if n >= 40 else 1.0 for n in fits]); n = int(rng.choice(fits, p=w / w.sum()))
            kind = str(rng.choice(["logits", "argmax", "sample"] if sample_ok else ["logits", "argmax"]))
            op = {"op": "forward", "kind": kind, "tokens": toks(n), "pos": pos}
        else:
            fits = [n for n in DECODE_N if n <= room]
            n = int(rng.choice(fits))
            kind = str(rng.choice(["greedy", "greedy", "sample"] if sample_ok else ["greedy"]))
            op = {"op": "decode", "kind": kind, "tok": toks(1)[0], "pos": pos, "n": n}
        if kind == "sample":
            op.update(sample_args())
        ops.append(op)
        fill = pos + n; since_inject += n; pending = False

    while len(ops) < n_ops:
        if len(ops) == age_at:
            stride = 1024 if tp else n_layers + 2
            ops.append({"op": "age", "e": (1 << 31) - int(rng.integers(5, 30)) * stride})
            age_at = -1
            continue
        r = rng.random()
        if not ops or pending or r < 0.62:
            token_call(force_prompt=not ops)
        elif r < 0.80:
            key = str(rng.choice(sorted(options)))
            ops.append({"op": "set_option", "key": key, "value": int(rng.choice(options[key])), "prepare": bool(rng.random() < 0.5)})
        elif r < 0.86 and not tp:
            n = int(rng.choice(DECODE_N))
            ops.append({"op": "reset_decode", "tok": toks(1)[0], "n": n})
            fill = n; since_inject += n
        elif r < 0.92 and not tp and injections < MAX_INJECTIONS and since_inject > PROBATION + 6:
            ops.append({"op": "inject"}); injections += 1; since_inject = 0; pending = True
        elif r < 0.96 and not tp:
            ops.append({"op": "kernel_times", "pos": int(rng.integers(0, max(1, fill)))})
            fill = 0
            token_call(force_prompt=True)
    if pending:                                                       # (an injection shows at the next token call: the script does not end on one)
        token_call()
    return ops


def check_script(ops, vocab, max_seq, sample_vocab_limit=None):
    """the preconditions every script keeps, whatever the seed; -> (tokens run, sampled tokens, injections)"""
    fill, injections, since, tokens, sampled = 0, 0, 10 ** 9, 0, 0
    for i, op in enumerate(ops):
        k = op["op"]
        if k in ("forward", "decode"):
            n = len(op["tokens"]) if k == "forward" else op["n"]
            assert 0 <= op["pos"] <= fill, (i, op["pos"], fill)                 # a rewind goes back, never past the fill
            assert n >= 1 and op["pos"] + n < max_seq, (i, op)
            ids = op["tokens"] if k == "forward" else [op["tok"]]
            assert all(0 <= t < vocab for t in ids), i
            if op["kind"] == "sample":
                assert sample_vocab_limit is None or vocab <= sample_vocab_limit, i
                assert op["t"] >= 0 and 0 <= op["p_top"] <= 1
                sampled += 1 if k == "forward" else n
            fill = op["pos"] + n; tokens += n; since += n
        elif k == "reset_decode":
            assert 1 <= op["n"] < max_seq and 0 <= op["tok"] < vocab
            fill = op["n"]; tokens += op["n"]; since += op["n"]
        elif k == "inject":
            injections += 1
            assert injections <= MAX_INJECTIONS and since > PROBATION, (i, since)
            since = 0
            assert i + 1 < len(ops), "a script does not end on an injection"
        elif k == "kernel_times":
            assert ops[i + 1]["op"] == "forward" and ops[i + 1]["pos"] == 0, i
            fill = 0
        elif k == "set_option":
            assert op["key"] in LIVE_OPTIONS and op["value"] in LIVE_OPTIONS[op["key"]], i
        else:
            assert k == "age" and 0 <= op["e"] < 1 << 32, i
    return tokens, sampled, injections


class OracleSide:
    """what the CPU oracle says each token call of a script returns.  The oracle's cache is a plain array of rows, so a call at a `pos` below the fill overwrites rows
    [pos, pos + n) and attends to rows [0, pos + n) like the library (tests/test_callscript_host.py checks that against a replay from an empty cache)."""

    def __init__(self, om, host_sampler=None):
        self.om, self.H, self.state = om, host_sampler, 1
        self.tokens = self.sampled = 0

    def _sample(self, logits, op):
        from sample_util import host_sample
        tok, self.state = host_sample(self.H, logits, op["t"], op["p_top"], self.state)
        self.sampled += 1
        return tok

    def expect(self, op):
        """-> {"logits": ndarray} | {"ids": [...]} | {"ids": [...], "state": s}; {} for an op that returns nothing"""
        k = op["op"]
        if k == "forward":
            lg = self.om.forward(np.array(op["tokens"], np.int32), op["pos"])
            self.tokens += len(op["tokens"])
            if op["kind"] == "logits":
                return {"logits": lg}
            if op["kind"] == "argmax":
                return {"ids": [int(np.argmax(lg))]}
            if op["state"] is not None:
                self.state = op["state"]
            return {"ids": [self._sample(lg, op)], "state": self.state}
        if k in ("decode", "reset_decode"):
            if k == "reset_decode":
                self.om.reset()
            pos, cur, ids = op.get("pos", 0), op["tok"], []
            sample = op.get("kind") == "sample"
            if sample and op["state"] is not None:
                self.state = op["state"]
            for i in range(op["n"]):
                lg = self.om.forward(np.array([cur], np.int32), pos + i)
                cur = self._sample(lg, op) if sample else int(np.argmax(lg))
                ids.append(cur)
            self.tokens += op["n"]
            return {"ids": ids, "state": self.state} if sample else {"ids": ids}
        if k == "kernel_times":
            self.om.reset()
        return {}


# ---- the fixed set of the GPU suite (tests/test_gpu_longlived.py part B; tests/test_callscript_host.py replays every one of them on the oracle alone) ----
SAMPLE_VOCAB_LIMIT = 36000            # the device sampler's LDS holds one workgroup's vocabulary (flm_host.h sample_supported); every model below stays under it
MAX_SEQ = 1024


def model(name):
    """-> (cfg, tensors) of a fixed-set model; `odd<seed>`: a shape tests/test_gpu_fuzz.py draws (odd group counts, head sizes 32 / 64 / 128)"""
    from fast_llama_amd import flmfile as ff, synth
    if name.startswith("odd"):
        from test_gpu_fuzz import _shape
        rng = np.random.default_rng(int(name[3:]))
        kw = _shape(rng)
        cfg = synth.make_config("tiny", ff.QT_INT8 if rng.random() < 0.6 else ff.QT_INT16, **kw)
        return cfg, synth.make_tensors(cfg, seed=100 + int(name[3:]))
    shape, qt, layers = {"small8": ("small", ff.QT_INT8, None), "small16": ("small", ff.QT_INT16, None), "tiny128_16": ("tiny128", ff.QT_INT16, None),
                         "7Bw2_8": ("7B", ff.QT_INT8, 2), "7Bw2_16": ("7B", ff.QT_INT16, 2)}[name]
    cfg = synth.make_config(shape, qt)
    if layers:
        cfg.n_layers = layers
    return cfg, synth.make_tensors(cfg, seed=97)


# (seed, model, world): 26 scripts of about 40 operations; the last two run on two ranks under CU masks
FIXED = ([(s, "small8", 1) for s in (101, 102, 103, 104, 105, 106, 107)] + [(s, "small16", 1) for s in (201, 202, 203, 204, 205, 206)] +
         [(s, "tiny128_16", 1) for s in (301, 302, 303, 304)] + [(s, "odd12", 1) for s in (401, 402, 403, 404)] + [(s, "7Bw2_8", 1) for s in (501, 502, 503)] +
         [(601, "small8", 2), (602, "small16", 2)])


def fixed_script(seed, name, world):
    cfg, _ = model(name)
    return generate(seed, cfg.vocab_size, MAX_SEQ, n_layers=cfg.n_layers, n_ops=40, world=world, sample_ok=cfg.vocab_size <= SAMPLE_VOCAB_LIMIT)
