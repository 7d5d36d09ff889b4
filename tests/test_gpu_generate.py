"""flm_generate: ParallelTransformer::generate (transformer.cpp:76-103) as one call -- the stop token, the cancel and the per-token hand-over decided on the device.

Expected ids ("ref") come from the oracle-pinned entry points on the same context after reset_kv: forward_argmax / forward_sample, then decode_greedy / decode_sample.
Models: the 2-layer 7B-width model of test_greedy_token_as_one_launch_vs_oracle (the smallest shape that runs the one-launch token), int8 and int16, and "tiny" int8 (the
per-phase kernels).  The model seeds were picked on the CPU with tests/oracle_py.py (greedy ids of the two prompts below) so that a stop index exists where the tests want it:
7B-width seed 53 (int8 and int16) and tiny seed 59 give j = 6 behind the 5-token prompt and j = 8 behind the 122-token prompt; the tests assert that, they do not skip."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from fast_llama_amd import flmfile as ff, synth
from sample_util import advance_state

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_SEQ = 256                  # (every case below fits; the cache taps read [heads][max_seq][hs] per layer)
MODELS = {"7B-int8": ("7B", ff.QT_INT8, 2, 53), "7B-int16": ("7B", ff.QT_INT16, 2, 53), "tiny": ("tiny", ff.QT_INT8, None, 59)}
DEFAULTS = {"fuse_tail": 1, "graph_chunks": 1, "use_graph": 1, "fuse_token": 1, "fuse_back": 1, "fuse_attn_o": 1, "fuse_ffn": 1, "tuning": 0, "gr_edges": 1, "back_ao": 3, "attn_split": 1}
OPTION_SETS = ({}, {"fuse_tail": 0}, {"graph_chunks": 0}, {"use_graph": 0}, {"fuse_token": 0}, {"fuse_back": 0, "fuse_attn_o": 0, "fuse_ffn": 0}, {"tuning": 1, "gr_edges": 0}, {"back_ao": 0})

_tensors = {}


def _prompt(V, n):
    return np.array([1] + [int(x) for x in (np.arange(1, n) * 7919) % V], dtype=np.int32)


def _model(name):
    if name not in _tensors:
        shape, qt, layers, seed = MODELS[name]
        cfg = synth.make_config(shape, qt)
        if layers:
            cfg.n_layers = layers
        _tensors[name] = (cfg, synth.make_tensors(cfg, seed=seed))
    return _tensors[name]


def _ctx(gpu, name, max_seq=MAX_SEQ):
    cfg, tensors = _model(name)
    ctx = gpu.Ctx(gpu.desc_from_config(cfg, max_seq_len=max_seq)); ctx.upload_all(tensors)
    return cfg, ctx


@pytest.fixture(scope="module")
def ctxs(gpu):
    """one context per model, shared by the tests that leave it as they found it (options back at their defaults, no fallback)"""
    made = {}

    def get(name):
        if name not in made:
            made[name] = _ctx(gpu, name)
        return made[name]
    yield get
    for _, c in made.values():
        c.close()


def _caches(ctx, cfg, max_seq=MAX_SEQ):
    n = cfg.n_heads * max_seq * (cfg.dim // cfg.n_heads)
    return [ctx.debug_read(w, l, n).view(np.uint32).reshape(cfg.n_heads, max_seq, -1) for l in range(cfg.n_layers) for w in ("kcache", "vcache")]


def _ref_greedy(ctx, cfg, prompt, n):
    """the plain run: n ids (the first from the prompt's last logits) and the caches it leaves"""
    ctx.reset_kv()
    first = ctx.forward_argmax(prompt, 0)
    ids = [first] + [int(x) for x in ctx.decode_greedy(first, len(prompt), n - 1)]
    return ids, _caches(ctx, cfg)


def _stop_index(ref, lo, hi=20):
    """the smallest j >= lo whose token has not occurred before it: stopping on ref[j] stops AT j"""
    js = [j for j in range(lo, min(hi, len(ref))) if ref[j] not in ref[:j]]
    assert js, f"the model seed must give a first-occurrence token in ref[{lo}:{hi}] (picked on the CPU oracle): {ref}"
    return js[0]


def _check_stop(ctx, cfg, prompt, max_tokens, ref, ref_caches, j, what, **gen):
    """generate with stop_token = ref[j]: ids, callback sequence, cache rows, and the continuation from the stop"""
    n_p = len(prompt)
    ctx.reset_kv()
    seen = []
    ids, _ = ctx.generate(prompt, 0, max_tokens, stop_token=ref[j], on_token=lambda i, t, last: seen.append((i, t, last)) and None, **gen)
    assert [int(x) for x in ids] == ref[:j + 1], (what, list(ids), ref[:j + 1])
    assert seen == [(i, ref[i], i == j) for i in range(j + 1)], (what, seen)
    assert ctx.query("gen_tokens") == j + 1
    for got, want in zip(_caches(ctx, cfg), ref_caches):
        assert not got[:, n_p + j:, :].any(), (what, "rows behind the stop were written", np.nonzero(got[:, n_p + j:, :].any(axis=(0, 2)))[0][:8] + n_p + j)
        assert np.array_equal(got[:, :n_p + j, :], want[:, :n_p + j, :]), what
    # the state, the epochs and the flag lines are those of a context that decoded exactly the fed tokens: feeding the stop token goes on as the plain run did
    assert [int(x) for x in ctx.decode_greedy(ref[j], n_p + j, 6)] == ref[j + 1:j + 7], what
    assert ctx.query("fallback") == 0, what


@pytest.mark.parametrize("name", list(MODELS))
def test_stop_in_the_middle_of_a_chunk_every_launch_structure(gpu, ctxs, name):
    """prompt of 5, max_tokens 40 (decode graphs of 16, 16, 4, 2 tokens and a single one), stop at index 6 -- inside the first chunk: the launches queued behind it return at
    their top.  n_out, ids, the callback's (index, token, last), every layer's K / V rows (behind the stop: zero bits; below: the plain run's), the continuation."""
    cfg, ctx = ctxs(name)
    prompt = _prompt(cfg.vocab_size, 5)
    ref, ref_caches = _ref_greedy(ctx, cfg, prompt, 40)
    j = _stop_index(ref, 6)
    try:
        for opts in OPTION_SETS:
            for k, v in opts.items():
                ctx.set_option(k, v)
            _check_stop(ctx, cfg, prompt, 40, ref, ref_caches, j, (name, opts))
            for k in opts:
                ctx.set_option(k, DEFAULTS[k])
    finally:
        for k, v in DEFAULTS.items():
            ctx.set_option(k, v)


@pytest.mark.parametrize("name", ["7B-int8", "7B-int16"])
def test_halted_launches_with_split_heads(gpu, ctxs, name):
    """prompt of 122, max_tokens 24, stop at 122 + j >= 130: the stop and the halted launches are the split-head forms (128 positions on); and split heads forced at a 5-token prompt"""
    cfg, ctx = ctxs(name)
    prompt = _prompt(cfg.vocab_size, 122)
    ref, ref_caches = _ref_greedy(ctx, cfg, prompt, 24)
    j = _stop_index(ref, 8)
    assert 122 + j >= 130
    _check_stop(ctx, cfg, prompt, 24, ref, ref_caches, j, (name, "122"))
    prompt = _prompt(cfg.vocab_size, 5)
    try:
        ctx.set_option("attn_split", 2)
        ref, ref_caches = _ref_greedy(ctx, cfg, prompt, 40)
        _check_stop(ctx, cfg, prompt, 40, ref, ref_caches, _stop_index(ref, 6), (name, "attn_split 2"))
    finally:
        ctx.set_option("attn_split", 1)


@pytest.mark.parametrize("t,p,seed", [(0.8, 0.9, 1234), (1.0, 1.0, 1234), (1.0, 0.9, 0)])
@pytest.mark.parametrize("name", ["7B-int8", "tiny"])
def test_sampled_generate_equals_forward_sample_and_decode_sample(gpu, ctxs, name, t, p, seed):
    cfg, ctx = ctxs(name)
    prompt = _prompt(cfg.vocab_size, 5)
    ctx.reset_kv()
    first, s1 = ctx.forward_sample(prompt, 0, t, p, seed)
    rest, _ = ctx.decode_sample(first, 5, 39, t, p, s1)
    ref = [first] + [int(x) for x in rest]
    j = _stop_index(ref, 6, 40)
    ctx.reset_kv()
    assert ctx.forward_sample(prompt, 0, t, p, seed) == (first, s1)
    _, s_want = ctx.decode_sample(first, 5, j, t, p, s1)                      # the state after j + 1 draws
    assert s_want == advance_state(seed, j + 1)
    n0 = ctx.query("sampled_tokens")
    ctx.reset_kv()
    seen = []
    ids, s = ctx.generate(prompt, 0, 40, temperature=t, topp=p, rng_state=seed, stop_token=ref[j], on_token=lambda i, tok, last: seen.append((i, tok, last)) and None)
    assert [int(x) for x in ids] == ref[:j + 1] and s == s_want, (list(ids), ref[:j + 1], s, s_want)
    assert seen == [(i, ref[i], i == j) for i in range(j + 1)]
    assert ctx.query("sampled_tokens") == n0 + j + 1 and ctx.query("fallback") == 0
    # the sampler state on the device stayed at the last draw's: the loop goes on from the stop as the plain run did
    more, _ = ctx.decode_sample(ref[j], 5 + j, 4, t, p, s)
    assert [int(x) for x in more] == ref[j + 1:j + 5]


def test_edges(gpu, ctxs):
    cfg, ctx = ctxs("tiny")
    prompt = _prompt(cfg.vocab_size, 5)
    ref, _ = _ref_greedy(ctx, cfg, prompt, 40)
    # no stop token: all of max_tokens
    ctx.reset_kv()
    ids, _ = ctx.generate(prompt, 0, 40)
    assert [int(x) for x in ids] == ref and ctx.query("gen_tokens") == 40
    # max_tokens 1: one token, the cache holds the prompt's rows only
    ctx.reset_kv()
    seen = []
    ids, _ = ctx.generate(prompt, 0, 1, on_token=lambda i, t, last: seen.append((i, t, last)) and None)
    assert [int(x) for x in ids] == ref[:1] and seen == [(0, ref[0], True)]
    for c in _caches(ctx, cfg):
        assert c[:, :5, :].any() and not c[:, 5:, :].any()
    # the first token is the stop token
    ctx.reset_kv()
    ids, _ = ctx.generate(prompt, 0, 40, stop_token=ref[0])
    assert [int(x) for x in ids] == ref[:1]
    for c in _caches(ctx, cfg):
        assert not c[:, 5:, :].any()
    # one step past max_seq_len: FLM_ERR_INVALID, nothing launched, "gen_tokens" unchanged
    ctx.generate(prompt, 0, MAX_SEQ - 5 + 1)                                   # (pos + n_prompt + max_tokens - 1 == max_seq_len: allowed)
    assert ctx.query("gen_tokens") == MAX_SEQ - 5 + 1
    before = ctx.query("gen_tokens")
    with pytest.raises(gpu.FlmError, match="flm error -1"):
        ctx.generate(prompt, 0, MAX_SEQ - 5 + 2)
    assert ctx.query("gen_tokens") == before
    # no callback; no out_tokens (the ids then come through the callback)
    ctx.reset_kv()
    ids, _ = ctx.generate(prompt, 0, 12, on_token=None)
    assert [int(x) for x in ids] == ref[:12]
    ctx.reset_kv()
    seen = []
    ids, _ = ctx.generate(prompt, 0, 12, on_token=lambda i, t, last: seen.append(t) and None, want_ids=False)
    assert len(ids) == 0 and seen == ref[:12] and ctx.query("gen_tokens") == 12
    assert ctx.query("fallback") == 0
    # a tensor-parallel rank: refused before it touches a peer (this one has none)
    tp = gpu.Ctx(gpu.desc_from_config(cfg, max_seq_len=MAX_SEQ), rank=0, world=2)
    with pytest.raises(gpu.FlmError, match="flm error -2"):
        tp.generate(prompt, 0, 4)
    tp.close()


def test_old_entry_points_never_halt(gpu, ctxs):
    """after a halted generate: forward_argmax + decode_greedy run all their steps, the stop token included and passed"""
    cfg, ctx = ctxs("7B-int8")
    prompt = _prompt(cfg.vocab_size, 5)
    ref, _ = _ref_greedy(ctx, cfg, prompt, 24)
    j = _stop_index(ref, 6)
    ctx.reset_kv()
    ids, _ = ctx.generate(prompt, 0, 24, stop_token=ref[j])
    assert len(ids) == j + 1
    ctx.reset_kv()
    first = ctx.forward_argmax(prompt, 0)
    assert [first] + [int(x) for x in ctx.decode_greedy(first, 5, 23)] == ref


def test_cancel_from_the_callback(gpu, ctxs):
    """the callback returns 1 at index 3 of 200: the device halts one or more tokens behind it.  No upper bound on n_out is asserted (how far the device runs ahead of a Python
    callback is not specified); observed on an MI355X with this 2-layer model: see DESIGN.md section 5c."""
    cfg, ctx = ctxs("7B-int8")
    prompt = _prompt(cfg.vocab_size, 5)
    ref, _ = _ref_greedy(ctx, cfg, prompt, 200)
    ctx.reset_kv()
    entered = []

    def on_token(i, t, last):
        entered.append((i, t))
        return i == 3
    ids, _ = ctx.generate(prompt, 0, 200, on_token=on_token)
    n_out = len(ids)
    print(f"cancel at index 3 of 200: n_out = {n_out}")
    assert n_out >= 4 and [int(x) for x in ids] == ref[:n_out]
    assert entered == [(i, ref[i]) for i in range(4)]                           # never entered again after it returned 1
    assert ctx.query("gen_tokens") == n_out
    toks, last, tags = ctx.gen_ring(n_out)
    assert list(toks) == ref[:n_out] and len(set(tags)) == 1 and tags[0] != 0
    assert list(last) == [0] * (n_out - 1) + [1]                                # the granule marked last is the n_out - 1-th
    if n_out < 200:
        assert [int(x) for x in ctx.decode_greedy(ref[n_out - 1], 5 + n_out - 1, 6)] == ref[n_out:n_out + 6]
    assert ctx.query("fallback") == 0


@pytest.mark.parametrize("sampled", [False, True])
def test_a_retried_generate_delivers_every_index_once(gpu, sampled):
    """the injected wait failure of tests/test_gpu_longlived.py: the first attempt runs through on garbage (and publishes nothing: a wait of the call has given up), the call
    re-runs on one kernel per phase from the caller's state"""
    cfg, ctx = _ctx(gpu, "7B-int8")
    prompt = _prompt(cfg.vocab_size, 5)
    t, p, seed = (1.0, 0.9, 1234) if sampled else (0.0, 0.9, 0)
    ctx.reset_kv()
    if sampled:
        first, s1 = ctx.forward_sample(prompt, 0, t, p, seed)
        ref = [first] + [int(x) for x in ctx.decode_sample(first, 5, 39, t, p, s1)[0]]
    else:
        ref, _ = _ref_greedy(ctx, cfg, prompt, 40)
    j = _stop_index(ref, 6, 40)
    ctx.reset_kv()
    ctx.set_option("inject_wait_failure", 1)
    seen = []
    ids, s = ctx.generate(prompt, 0, 40, temperature=t, topp=p, rng_state=seed, stop_token=ref[j], on_token=lambda i, tok, last: seen.append((i, tok, last)) and None)
    assert [int(x) for x in ids] == ref[:j + 1]
    assert seen == [(i, ref[i], i == j) for i in range(j + 1)]                  # every index exactly once, from the sound attempt
    assert ctx.query("fallback") == 1
    if sampled:
        assert s == advance_state(seed, j + 1)
    ctx.close()


_ALLOC_CHILD = r"""
import ctypes, json, os, sys
import numpy as np
sys.path.insert(0, os.environ["FLM_ROOT"])
import __graft_entry__ as graft
graft.load_package()
from fast_llama_amd import capi, synth, flmfile as ff
cnt = ctypes.CDLL(None)                      # the LD_PRELOADed interposer (tests/helpers/hipcount.c)
cnt.hipcount_allocs.restype = ctypes.c_long
hip = ctypes.CDLL("libamdhip64.so")
def free_bytes():
    f, t = ctypes.c_size_t(0), ctypes.c_size_t(0)
    assert hip.hipMemGetInfo(ctypes.byref(f), ctypes.byref(t)) == 0
    return f.value
out = {}
for shape, qt, layers, nprompt, temp in (("7B", ff.QT_INT8, 2, 9, 0.0), ("tiny", ff.QT_INT8, None, 3, 1.0)):
    cfg = synth.make_config(shape, qt)
    if layers: cfg.n_layers = layers
    tensors = synth.make_tensors(cfg, seed=3)
    ctx = capi.Ctx(capi.desc_from_config(cfg, max_seq_len=256)); ctx.upload_all(tensors)
    prompt = np.array([1] + [int(x) for x in (np.arange(1, nprompt) * 7919) % cfg.vocab_size], np.int32)
    seen = []
    a0, f0 = cnt.hipcount_allocs(), free_bytes()
    ids, _ = ctx.generate(prompt, 0, 40, temperature=temp, topp=0.9, rng_state=1234, on_token=lambda i, t, last: seen.append(t) and None)     # the context's FIRST call
    a1, f1 = cnt.hipcount_allocs(), free_bytes()
    out[shape] = {"allocs": a1 - a0, "free_delta": f0 - f1, "n": len(ids), "same": [int(x) for x in ids] == seen, "counted_before": a0}
    ctx.close()
print("ALLOC " + json.dumps(out))
"""


def test_nothing_is_allocated_inside_generate(gpu):
    """the first flm_generate of a context (greedy behind a batched prompt; sampled on the per-phase kernels), bracketed with the allocation counter of tests/helpers/hipcount.c
    (hipMalloc & co. and hipHostMalloc: device and page-locked memory) and hipMemGetInfo, the way tests/test_gpu_configs.py brackets forward and decode"""
    so = os.path.join(ROOT, "tests", "helpers", "libhipcount.so")
    assert os.path.exists(so), "tests/helpers/libhipcount.so missing: run __graft_entry__.build()"
    preload = os.pathsep.join(x for x in (so, os.environ.get("LD_PRELOAD", "")) if x)      # (in front of whatever the environment already preloads)
    r = subprocess.run([sys.executable, "-c", _ALLOC_CHILD], capture_output=True, text=True, timeout=600, env=dict(os.environ, LD_PRELOAD=preload, FLM_ROOT=ROOT), cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads([l for l in r.stdout.splitlines() if l.startswith("ALLOC ")][-1][6:])
    for shape, v in res.items():
        assert v["counted_before"] > 20, f"{shape}: the interposer saw no allocation at create / upload -- it is not interposing"
        assert v["n"] == 40 and v["same"]
        assert v["allocs"] == 0, f"{shape}: {v['allocs']} allocation calls inside flm_generate"
        assert v["free_delta"] <= 0, f"{shape}: {v['free_delta']} bytes less free device memory after flm_generate"


def test_tokens_are_visible_before_the_stream_drains(gpu):
    """400 tokens, max_seq_len 512: at least one token reaches the callback while hipStreamQuery still says the stream is busy -- the host sees a kernel's system-scope store to
    coherent host memory while the graphs are still replaying.  (Correctness does not depend on it: what the poll misses is delivered behind the synchronise.)"""
    cfg, ctx = _ctx(gpu, "7B-int8", max_seq=512)
    prompt = _prompt(cfg.vocab_size, 5)
    ctx.reset_kv()
    first = ctx.forward_argmax(prompt, 0)
    ref = [first] + [int(x) for x in ctx.decode_greedy(first, 5, 399)]
    ctx.reset_kv()
    seen = []
    ids, _ = ctx.generate(prompt, 0, 400, on_token=lambda i, t, last: seen.append(t) and None)
    streamed = ctx.query("gen_streamed")
    print(f"gen_streamed = {streamed} of 400")
    assert [int(x) for x in ids] == ref and seen == ref and ctx.query("gen_tokens") == 400
    assert streamed >= 1
    assert ctx.query("fallback") == 0
    ctx.close()
