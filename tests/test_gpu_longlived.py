"""Contexts that get OLD, and contexts driven through the entry points in other orders than "prompt, then decode".

Part A -- the epoch counters across their edges.  Every cross-workgroup / cross-rank wait compares a flag line (or a granule's tag) with a value that counts from a counter in
device memory: the one-launch token's epoch (+ n_layers + 2 per greedy token), the token's epoch base of the tensor-parallel hand-offs (+ 1024 per token), k_xchg's exchange
counters (+ 1 per exchange).  They reach 2^31 after hours to days of decoding, which no test can wait for: option "age_epochs" (csrc/flm_tuning.h) puts a context into the state
a real run would have left with its counters at a given value -- shown faithful against ~300 real tokens first --, and each cell carries a context across an edge INSIDE a
48-token greedy decode (inside a 16-token graph replay), then through a single-token forward (k_embed clears the local lines to 0), more greedy tokens, a batched prompt chunk
and sampled tokens, an injected wait failure with its 64-token probation and the return to the one-launch token -- ids, sampler state and logits against the CPU oracle, bit for
bit, and "fallback" counting exactly the injected episode.  Edges: 2^31 (where a signed difference changes sign against a cleared line) and kEpochWrap = 0xFFE0_0000, where
the one-launch token's epoch goes back to 4096 and the token's epoch base to 0 (flm_wait.h flag_reached); k_xchg's counters run through 2^32.

Part B -- call-order fuzz: the seeded scripts of tests/callscript.py (rewinds, decode directly after flm_reset_kv, prompt chunks behind decoded tokens, graph-chunk edges behind
one another, structure switches between calls, injected wait failures, flm_kernel_times and the documented recovery) on one context against one oracle."""
import functools
import json

import numpy as np
import pytest

import callscript as CS
import oracle_py as O
from sample_util import host_lib, host_sample
from test_gpu_tp import _prompt, _run_ranks, bits_equal

pytestmark = pytest.mark.gpu

WRAP, FIRST = 0xFFE00000, 4096           # flm_math.h kEpochWrap / kEpochFirst
M32 = (1 << 32) - 1
T, P_TOP, S0 = 1.0, 0.9, 1234            # the sampled leg's parameters


# ---- contexts: one GPU, or `world` ranks on one GPU under CU masks (threads as ranks: tests/test_gpu_tp.py) ----
class Group:
    def __init__(self, gpu, cfg, tensors, world=1, options=(), tp_options=()):
        self.world = world
        desc = gpu.desc_from_config(cfg, CS.MAX_SEQ)
        self.ctxs = [gpu.Ctx(desc, device=0, rank=r, world=world, comm_id=None) for r in range(world)]
        for c in self.ctxs:
            c.upload_all(tensors)
            if world > 1:
                c.set_option("cu_parts", world)
            for k, v in tuple(options) + (tuple(tp_options) if world > 1 else ()):
                c.set_option(k, v)
        if world > 1:
            gpu.Ctx.regroup(self.ctxs)
        elif options:
            self.ctxs[0].prepare()

    def run(self, fn):
        """fn(ctx) on every rank at once; the ranks must agree; -> rank 0's result"""
        if self.world == 1:
            return fn(self.ctxs[0])
        out = _run_ranks(self.ctxs, fn)
        for r, o in enumerate(out[1:], 1):
            assert _same(o, out[0]), f"rank {r} disagrees with rank 0"
        return out[0]

    def each(self, fn):
        return [fn(c) for c in self.ctxs]

    def close(self):
        for c in self.ctxs:
            c.close()


def _same(a, b):
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray):
        return a.shape == b.shape and np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a, b.view(np.uint32) if b.dtype == np.float32 else b)
    return a == b


def _greedy(om, cur, pos, n):
    ids = []
    for i in range(n):
        cur = int(np.argmax(om.forward(np.array([cur], np.int32), pos + i))); ids.append(cur)
    return ids


# ---- part A -------------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _truth(name, P):
    """the oracle's side of part A's script for one model and start position: the same for every launch structure, world size and edge"""
    cfg, tensors = CS.model(name)
    om, H = O.OracleModel(cfg, tensors, max_seq=CS.MAX_SEQ), host_lib()
    w = {"prompt": _prompt(cfg.vocab_size, P), "chunk": _prompt(cfg.vocab_size, 41)[1:]}
    w["lg0"] = om.forward(w["prompt"], 0)
    cur, pos = int(np.argmax(w["lg0"])), P
    w["pre"] = _greedy(om, cur, pos, 3); cur, pos = w["pre"][-1], pos + 3
    w["ids48"] = _greedy(om, cur, pos, 48); cur, pos = w["ids48"][-1], pos + 48
    w["lg1"] = om.forward(np.array([cur], np.int32), pos); cur, pos = int(np.argmax(w["lg1"])), pos + 1
    w["ids20"] = _greedy(om, cur, pos, 20); pos += 20
    first, s = host_sample(H, om.forward(w["chunk"], pos), T, P_TOP, S0); pos += 40
    w["first"], w["s1"] = first, s
    ids, cur = [], first
    for i in range(20):
        cur, s = host_sample(H, om.forward(np.array([cur], np.int32), pos + i), T, P_TOP, s); ids.append(cur)
    w["ids_s"], w["s2"] = ids, s; pos += 20
    w["ids70"] = _greedy(om, cur, pos, 70); cur, pos = w["ids70"][-1], pos + 70
    w["lg2"] = om.forward(np.array([cur], np.int32), pos)
    assert pos + 1 < CS.MAX_SEQ
    return w


def _cell(gpu, name, P, edge, world=1, options=(), tp_options=(), counter="tail"):
    """one cell of the matrix.  edge: None (the control: the same script, nothing aged) or the value the cell's counter crosses inside the 48-token decode"""
    cfg, tensors = CS.model(name)
    w = _truth(name, P)
    g = Group(gpu, cfg, tensors, world, options, tp_options)
    where = f"{name} from position {P}, world {world}, {dict(options + tp_options)}, edge {edge if edge is None else hex(edge)}"
    try:
        def before(c):
            lg0 = c.forward(w["prompt"], 0)
            return lg0, [int(x) for x in c.decode_greedy(int(np.argmax(lg0)), P, 3)]
        lg0, pre = g.run(before)
        assert bits_equal(lg0, w["lg0"]) and pre == w["pre"], f"{where}: before anything was aged"
        stride = {"tail": cfg.n_layers + 2, "eng": 1024, "xchg": 1}[counter]
        which = {"tail": 0, "eng": 1, "xchg": 2}[counter]
        if edge is not None:
            e = (edge - 20 * stride) & M32
            g.each(lambda c: c.age_epochs(e))
            for ep in g.each(lambda c: c.epochs()):
                assert ep == (e, e & ~1023, e), f"{where}: the counters after ageing"
        inject = world == 1            # (across ranks a wait that gives up is a group error, not a retry)

        def after(c):
            e0 = c.epochs()
            ids48 = [int(x) for x in c.decode_greedy(w["pre"][-1], P + 3, 48)]
            e1 = c.epochs()
            pos = P + 51
            lg1 = c.forward(np.array([ids48[-1]], np.int32), pos); pos += 1
            ids20 = [int(x) for x in c.decode_greedy(int(np.argmax(lg1)), pos, 20)]; pos += 20
            first, s1 = c.forward_sample(w["chunk"], pos, T, P_TOP, S0); pos += 40
            ids_s, s2 = c.decode_sample(first, pos, 20, T, P_TOP, s1); pos += 20
            fb0 = c.query("fallback")
            if inject:
                c.set_option("inject_wait_failure", 1)
            ids70 = [int(x) for x in c.decode_greedy(int(ids_s[-1]), pos, 70)]; pos += 70
            active = c.query("fallback_active")
            lg2 = c.forward(np.array([ids70[-1]], np.int32), pos)
            return e0, e1, ids48, lg1, ids20, first, s1, [int(x) for x in ids_s], s2, fb0, ids70, active, lg2, c.query("fallback"), c.epochs()
        e0, e1, ids48, lg1, ids20, first, s1, ids_s, s2, fb0, ids70, active, lg2, fb, e2 = g.run(after)
        print(f"{where}: counters {[hex(x) for x in e0]} -> {[hex(x) for x in e1]} -> {[hex(x) for x in e2]}, fallback {fb0} -> {fb}")
        if edge is not None and e1[which] != e0[which]:            # (a structure that never touches the counter has nothing to cross)
            crossed = e1[which] < e0[which] if edge in (WRAP, 1 << 32) else e0[which] < edge <= e1[which]
            assert crossed, f"{where}: the 48 tokens did not carry the counter across the edge: {hex(e0[which])} -> {hex(e1[which])}"
        assert ids48 == w["ids48"], f"{where}: the 48 greedy tokens across the edge"
        assert bits_equal(lg1, w["lg1"]), f"{where}: logits of the single-token forward behind them"
        assert ids20 == w["ids20"], f"{where}: greedy tokens behind a forward (k_embed cleared the lines)"
        assert (first, s1) == (w["first"], w["s1"]), f"{where}: the prompt chunk's sampled token / state"
        assert (ids_s, s2) == (w["ids_s"], w["s2"]), f"{where}: sampled tokens / final state"
        assert fb0 == 0, f"{where}: a wait gave up by itself before the injection (fallback {fb0})"
        assert ids70 == w["ids70"], f"{where}: 70 tokens across the injected failure, its probation and the return"
        assert bits_equal(lg2, w["lg2"]), f"{where}: logits at the end"
        assert fb == (1 if inject else 0) and active == 0, f"{where}: fallback {fb}, active {active}: exactly the injected episode, and over"
    finally:
        g.close()


ONE_GPU = [("small8", ()), ("small16", ()), ("7Bw2_8", ()), ("7Bw2_16", ()),
           ("small8", (("gr_edges", 0),)), ("7Bw2_8", (("gr_edges", 0),)),
           ("small8", (("fuse_tail", 0), ("fuse_token", 0)))]
EDGES = [1 << 31, WRAP]


@pytest.mark.parametrize("P", [10, 600])
@pytest.mark.parametrize("edge", EDGES, ids=hex)
@pytest.mark.parametrize("name,options", ONE_GPU)
def test_one_gpu_across_an_epoch_edge(gpu, name, options, edge, P):
    _cell(gpu, name, P, edge, options=options)


@pytest.mark.parametrize("P", [10, 600])
@pytest.mark.parametrize("name,options", [ONE_GPU[0], ONE_GPU[4], ONE_GPU[6]])
def test_one_gpu_control_nothing_aged(gpu, name, options, P):
    _cell(gpu, name, P, None, options=options)


# the launch structures of the sharded token: the rank-spanning launch (granules), the folded exchanges with the attention fused across ranks and without, the k_xchg launches
TP_STRUCTURES = {"span": (("tp_fuse_layers", 1),), "fold2": (("tp_fuse_layers", 0), ("fold_xchg", 1), ("tp_fuse_attn", 2)), "fold0": (("tp_fuse_layers", 0), ("fold_xchg", 1), ("tp_fuse_attn", 0)),
                 "xchg": (("tp_fuse_layers", 0), ("fold_xchg", 0))}
TP_MODELS = [("small8", 2), ("small16", 2), ("small8", 4), ("small16", 4), ("7Bw2_8", 2)]


@pytest.mark.parametrize("P", [10, 600])
@pytest.mark.parametrize("edge", EDGES, ids=hex)
@pytest.mark.parametrize("name,world", TP_MODELS)
@pytest.mark.parametrize("structure", ["span", "fold2", "fold0"])
def test_tensor_parallel_across_an_epoch_edge(gpu, structure, name, world, edge, P):
    _cell(gpu, name, P, edge, world=world, tp_options=TP_STRUCTURES[structure], counter="eng")


@pytest.mark.parametrize("P", [10, 600])
@pytest.mark.parametrize("edge", [1 << 31, 1 << 32], ids=hex)
@pytest.mark.parametrize("name,world", TP_MODELS)
def test_tensor_parallel_xchg_counters_across_an_edge(gpu, name, world, edge, P):
    _cell(gpu, name, P, edge, world=world, tp_options=TP_STRUCTURES["xchg"], counter="xchg")


@pytest.mark.parametrize("P", [10, 600])
@pytest.mark.parametrize("structure", sorted(TP_STRUCTURES))
def test_tensor_parallel_control_nothing_aged(gpu, structure, P):
    _cell(gpu, "small8", P, None, world=2, tp_options=TP_STRUCTURES[structure], counter="eng")


@pytest.mark.parametrize("world", [1, 2])
def test_ageing_is_what_real_tokens_leave(gpu, world):
    """~300 real tokens on a fresh context (flm_forward and flm_decode_greedy mixed, up into split heads), then a second fresh context aged to the counter the first one shows
    (one GPU: the one-launch token's epoch; two ranks: the token's epoch base): every never-cleared line and tag of the aged one that counts from that counter is at most what
    the real one holds and within one token's stride of it, and the same further calls leave the same counter and return the same ids -- the oracle's -- on both"""
    cfg, tensors = CS.model("small8")
    om = O.OracleModel(cfg, tensors, max_seq=CS.MAX_SEQ)
    V, L = cfg.vocab_size, cfg.n_layers
    which, stride = (0, L + 2) if world == 1 else (1, 1024)
    # flm_debug_read 11: [the classifier lines: 256] and under tensor parallelism [k_xchg: 32][folded exchanges: 32][heads / FFN across ranks: 264][rank-spanning launch: (1 + 4 world) 256]
    n_lines = 256 if world == 1 else 256 + 32 + 32 + 264 + (1 + 4 * world) * 256
    lines = slice(0, 256) if world == 1 else slice(256 + 32, n_lines)
    n_tags = (3 if world > 1 else 6) * cfg.dim + cfg.hidden_dim                  # (the granule vectors; the split heads' score granules behind them share their buffer with plain floats)
    prompt = _prompt(V, 90)

    def real(c):
        cur, pos, n = int(np.argmax(c.forward(prompt, 0))), len(prompt), 0
        while n < 300:
            ids = c.decode_greedy(cur, pos, 33); pos += 33; n += 33
            cur = int(np.argmax(c.forward(np.array([int(ids[-1])], np.int32), pos))); pos += 1; n += 1
        ids = c.decode_greedy(cur, pos, 2)                                        # (the last token a greedy one: the one-launch token's lines hold the last token's values)
        return int(ids[-1]), pos + 2

    old, new = Group(gpu, cfg, tensors, world), Group(gpu, cfg, tensors, world)
    try:
        cur, pos = old.run(real)
        assert pos > 128 + 200
        ep = old.each(lambda c: c.epochs())
        assert len(set(ep)) == 1, ep
        e = ep[0][which]
        assert e >= (FIRST + 100 * stride if world == 1 else 300 * stride), ep     # (one GPU: the greedy tokens only)
        new.each(lambda c: c.age_epochs(e))
        assert all(x[which] == e for x in new.each(lambda c: c.epochs()))
        for c_old, c_new in zip(old.ctxs, new.ctxs):
            for what, n, part, least in (("lines", n_lines, lines, 1), ("tags", n_tags, slice(0, n_tags), 2 * cfg.dim)):
                o, a = c_old.epoch_words(what, n).astype(np.int64)[part], c_new.epoch_words(what, n).astype(np.int64)[part]
                used = o != 0                                                     # (a line or tag no launch of this run ever wrote is 0 on the real context)
                d = o[used] - a[used]
                print(f"world {world}, {what}: {int(used.sum())} in use, real - aged in [{int(d.min())}, {int(d.max())}], counter {hex(e)}")
                assert used.sum() >= least and np.all((d >= 0) & (d < stride)), (what, int(d.min()), int(d.max()))
        # the same further calls on both, from a common prompt (the aged context has no cache rows yet)
        full = np.concatenate([prompt, (np.arange(len(prompt), pos) * 31 % (V - 1) + 1).astype(np.int32)])

        def further(c):
            first = c.forward_argmax(full, 0)
            a = [int(x) for x in c.decode_greedy(first, pos, 20)]
            b = int(np.argmax(c.forward(np.array([a[-1]], np.int32), pos + 20)))
            return first, a, b, [int(x) for x in c.decode_greedy(b, pos + 21, 5)], c.epochs()[which]
        before = [g.each(lambda c: c.epochs()[which]) for g in (old, new)]
        assert before[0] == before[1]
        got_old, got_new = old.run(further), new.run(further)
        assert got_old == got_new, "the same calls: the same ids and the same counter"
        first = int(np.argmax(om.forward(full, 0)))
        want = _greedy(om, first, pos, 20)
        assert (got_new[0], got_new[1]) == (first, want)
    finally:
        old.close(); new.close()


# ---- part B -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed,name,world", CS.FIXED)
def test_call_script(gpu, seed, name, world):
    cfg, tensors = CS.model(name)
    ops = CS.fixed_script(seed, name, world)
    _, sampled, injections = CS.check_script(ops, cfg.vocab_size, CS.MAX_SEQ, CS.SAMPLE_VOCAB_LIMIT)
    side = CS.OracleSide(O.OracleModel(cfg, tensors, max_seq=CS.MAX_SEQ), host_lib())
    g = Group(gpu, cfg, tensors, world)
    state = 1
    try:
        for i, op in enumerate(ops):
            so_far = f"seed {seed}, {name}, world {world}, operation {i}; replay: {json.dumps(ops[:i + 1])}"
            want = side.expect(op)
            k = op["op"]
            if k == "forward":
                toks = np.array(op["tokens"], np.int32)
                if op["kind"] == "logits":
                    assert bits_equal(g.run(lambda c: c.forward(toks, op["pos"])), want["logits"]), so_far
                elif op["kind"] == "argmax":
                    assert [g.run(lambda c: c.forward_argmax(toks, op["pos"]))] == want["ids"], so_far
                else:
                    s = state if op["state"] is None else op["state"]
                    tok, state = g.run(lambda c: c.forward_sample(toks, op["pos"], op["t"], op["p_top"], s))
                    assert ([tok], state) == (want["ids"], want["state"]), so_far
            elif k in ("decode", "reset_decode"):
                if k == "reset_decode":
                    g.each(lambda c: c.reset_kv())
                if op.get("kind") == "sample":
                    s = state if op["state"] is None else op["state"]
                    ids, state = g.run(lambda c: c.decode_sample(op["tok"], op["pos"], op["n"], op["t"], op["p_top"], s))
                    assert ([int(x) for x in ids], state) == (want["ids"], want["state"]), so_far
                else:
                    ids = g.run(lambda c: c.decode_greedy(op["tok"], op.get("pos", 0), op["n"]))
                    assert [int(x) for x in ids] == want["ids"], so_far
                assert [int(x) for x in g.run(lambda c: c.last_tokens(op["n"]))] == want["ids"], "flm_last_tokens: " + so_far
            elif k == "set_option":
                g.each(lambda c: c.set_option(op["key"], op["value"]))
                if op["prepare"]:
                    g.each(lambda c: c.prepare())
            elif k == "inject":
                g.each(lambda c: c.set_option("inject_wait_failure", 1))
            elif k == "age":
                g.each(lambda c: c.age_epochs(op["e"]))
            elif k == "kernel_times":
                g.each(lambda c: c.kernel_times(op["pos"], 1))
        done = f"seed {seed}, {name}, world {world}; replay: {json.dumps(ops)}"
        for c in g.ctxs:
            assert c.query("fallback") == injections, done
            assert c.query("sampled_tokens") == sampled, done
    finally:
        g.close()
