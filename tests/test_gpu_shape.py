"""Sampling controls on the device (include/flm_gpu.h: flm_sampling, flm_generate_ex, flm_forward_sample_ex, flm_op_shape_logits).

Op level: k_shape_logits equals the host restatement (fh_shape, itself pinned against NumPy in tests/test_shape_host.py) on the bit patterns.  Model level: with every control
neutral flm_generate_ex is flm_generate; with controls set its ids and final sampler state are those of a host loop -- flm_forward's logits, fh_shape, fh_sample_state --
element for element.  Models: "tiny" int8 / int16 (model seed 59, as tests/test_gpu_generate.py) and, for the retry path, the 2-layer 7B-width model whose fused launches wait
across workgroups.  The teeth test's sampler seed (1234: the run under repeat_penalty 1.3 leaves the unpenalised one at index 6) was picked on the CPU with tests/oracle_py.py."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import __graft_entry__ as graft
from fast_llama_amd import flmfile as ff, synth
from sample_util import advance_state, host_lib
from shape_util import NINF, SIZES, Sampling, bits, grid, host_loop, window_at, windows

pytestmark = pytest.mark.gpu
ROOT = graft.ROOT
MAIN = os.path.join(graft.PKG_DIR, "bin", "main")
MAX_SEQ = 256
MODELS = {"tiny": ("tiny", ff.QT_INT8, None, 59), "tiny16": ("tiny", ff.QT_INT16, None, 59), "7B-int8": ("7B", ff.QT_INT8, 2, 53)}
CONTROLS = dict(top_k=5, min_p=0.05, repeat_penalty=1.3, penalty_last_n=8, bias={3: 2.0, 7: -np.inf})
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


def _ctx(gpu, name):
    cfg, tensors = _model(name)
    ctx = gpu.Ctx(gpu.desc_from_config(cfg, max_seq_len=MAX_SEQ)); ctx.upload_all(tensors)
    return cfg, ctx


@pytest.fixture(scope="module")
def ctxs(gpu):
    made = {}

    def get(name):
        if name not in made:
            made[name] = _ctx(gpu, name)
        return made[name]
    yield get
    for _, c in made.values():
        c.close()


_refs = {}


def _ref(ctx, name, prompt, n, s, seed):
    """the host loop's ids and state, computed once per (model, controls, seed)"""
    key = (name, len(prompt), n, repr(s), seed)
    if key not in _refs:
        _refs[key] = host_loop(ctx, host_lib(), prompt, n, s, seed)
    return _refs[key]


# ---- op level ----------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES + (40000,))
def test_op_equals_the_host_restatement(gpu, n):
    """the grid of tests/test_shape_host.py; n = 40000 lies above the sampler's LDS bound: the shaper has none"""
    cases = grid(n)
    for name, L, s, w in cases:
        got, want = gpu.op_shape_logits(L, s, w), gpu.shape_host(L, s, w)
        assert np.array_equal(bits(got), bits(want)), (n, name, np.nonzero(bits(got) != bits(want))[0][:8])


def test_op_top_k_ties_admit_the_lowest_indices(gpu):
    """500 equal maxima over n = 4099, top_k = 37: exactly the 37 lowest indices survive; the same with every second maximum -0.0 and the rest +0.0"""
    n, k = 4099, 37
    L = np.full(n, -1.0, np.float32)
    mx = np.sort(np.random.default_rng(5).permutation(n)[:500])
    L[mx] = 0.0
    mixed = np.where(np.isin(np.arange(n), mx[::2]), np.float32(-0.0), L).astype(np.float32)
    for row in (L, mixed):
        S = gpu.op_shape_logits(row, Sampling(temperature=1.0, top_k=k))
        assert list(np.nonzero(S != NINF)[0]) == list(mx[:k])
        assert np.array_equal(bits(S), bits(gpu.shape_host(row, Sampling(temperature=1.0, top_k=k))))
    # ties BELOW the maximum at the cut, across several 1024-index blocks
    L2 = np.where(np.arange(n) % 3 == 0, np.float32(1.0), np.float32(0.5)).astype(np.float32)
    L2[[5, 2000, 4000]] = 9.0
    for k2 in (2, 3, 4, 700, 1369, 1370, 1371, 3000):
        s = Sampling(temperature=1.0, top_k=k2)
        assert np.array_equal(bits(gpu.op_shape_logits(L2, s)), bits(gpu.shape_host(L2, s))), k2


def test_op_window_of_1024_ids_from_3_values(gpu):
    n = 4099
    L = (np.random.default_rng(3).standard_normal(n) * 3).astype(np.float32)
    w = windows(n)["three"]
    s = Sampling(temperature=1.0, repeat_penalty=1.2, frequency_penalty=0.01, presence_penalty=0.5)
    got = gpu.op_shape_logits(L, s, w)
    assert np.array_equal(bits(got), bits(gpu.shape_host(L, s, w)))
    assert sorted(np.nonzero(bits(got) != bits(L))[0]) == sorted(set(int(x) for x in w))


def test_op_neutral_controls_leave_the_bits_alone(gpu):
    L = np.array([-0.0, 0.0, 1.5, -np.inf, -0.0, -3.0, 7.0] * 300, np.float32)
    for s, w in ((Sampling(temperature=0.8), [0, 4, 1]), (Sampling(temperature=0.8, top_k=L.size), ()), (Sampling(temperature=0.0, min_p=0.3), ()),
                 (Sampling(temperature=0.8, repeat_penalty=1.3, presence_penalty=1.0), ())):
        assert np.array_equal(bits(gpu.op_shape_logits(L, s, w)), bits(L))


# ---- model level -------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t,p", [(0.0, 0.9), (1.0, 0.9), (0.8, 1.0)])
def test_neutral_controls_are_flm_generate(gpu, ctxs, t, p):
    cfg, ctx = ctxs("tiny")
    prompt = _prompt(cfg.vocab_size, 5)
    ctx.reset_kv()
    want = ctx.generate(prompt, 0, 48, temperature=t, topp=p, rng_state=1234)
    n0 = ctx.query("shaped_tokens")
    for s in (Sampling(temperature=t, topp=p), Sampling(temperature=t, topp=p, top_k=cfg.vocab_size, repeat_penalty=1.3, penalty_last_n=0)):
        ctx.reset_kv()
        ids, st = ctx.generate_ex(prompt, 0, 48, s, rng_state=1234)
        assert list(ids) == list(want[0]) and len(ids) == 48 and st == want[1]
    assert ctx.query("shaped_tokens") == n0                                     # the existing forms ran
    # ... and with a control that is set but changes nothing (a bias of +0 on one id) the shaped form gives the same ids and state
    ctx.reset_kv()
    ids, st = ctx.generate_ex(prompt, 0, 48, Sampling(temperature=t, topp=p, bias={11: 0.0}), rng_state=1234)
    assert list(ids) == list(want[0]) and st == want[1] and ctx.query("shaped_tokens") == n0 + 48


@pytest.mark.parametrize("name,t,p", [("tiny", 0.0, 0.9), ("tiny", 1.0, 0.9), ("tiny16", 1.0, 0.9)])
def test_controls_set_equal_the_host_loop(gpu, ctxs, name, t, p):
    """48 tokens behind a 12-token prompt with penalty_last_n = 8: the window slides off the prompt and over generated ids; top-k 5, min-p 0.05, a bias and a ban"""
    cfg, ctx = ctxs(name)
    prompt = _prompt(cfg.vocab_size, 12)
    s = Sampling(temperature=t, topp=p, **CONTROLS)
    ref, sref = _ref(ctx, name, prompt, 48, s, 77)
    assert 7 not in ref and sref == (77 if t == 0 else advance_state(77, 48))
    n0, m0 = ctx.query("shaped_tokens"), ctx.query("sampled_tokens")
    ctx.reset_kv()
    seen = []
    ids, st = ctx.generate_ex(prompt, 0, 48, s, rng_state=77, on_token=lambda i, tok, last: seen.append((i, tok, last)) and None)
    assert [int(x) for x in ids] == ref and st == sref
    assert seen == [(i, ref[i], i == 47) for i in range(48)]
    assert ctx.query("shaped_tokens") == n0 + 48 and ctx.query("sampled_tokens") == m0 + (48 if t else 0) and ctx.query("fallback") == 0
    # the one-token prompt path and a call at pos > 0: the window holds this call's ids only
    ctx.reset_kv()
    ctx.forward(prompt[:4], 0)
    ids2, _ = ctx.generate_ex(prompt[4:6], 4, 6, s, rng_state=5)
    hist, state, want, pos = [int(x) for x in prompt[4:6]], 5, [], 6
    ctx.reset_kv()
    logits = ctx.forward(prompt[:6], 0)
    for _ in range(6):
        tok, state = _draw(gpu, logits, s, window_at(hist, s.penalty_last_n), state)
        want.append(tok); hist.append(tok)
        logits = ctx.forward(np.array([tok], np.int32), pos); pos += 1
    assert [int(x) for x in ids2] == want


def _draw(gpu, logits, s, window, state):
    from sample_util import host_sample
    return host_sample(host_lib(), gpu.shape_host(logits, s, window), s.temperature, s.topp, state)


def test_the_penalty_changes_the_ids_and_the_device_follows(gpu, ctxs):
    """teeth: seed 1234, repeat_penalty 1.3 over the last 64 ids -- the host loop's ids differ from the unpenalised ones within 32 tokens, and the device's are the penalised"""
    cfg, ctx = ctxs("tiny")
    prompt = _prompt(cfg.vocab_size, 5)
    s = Sampling(temperature=1.0, topp=0.9, repeat_penalty=1.3, penalty_last_n=64)
    pen, spen = _ref(ctx, "tiny", prompt, 32, s, 1234)
    plain, _ = host_loop(ctx, host_lib(), prompt, 32, s, 1234, shaped=False)
    assert pen != plain, "the seed must make the penalty matter (picked on the CPU oracle)"
    ctx.reset_kv()
    assert [int(x) for x in ctx.generate(prompt, 0, 32, temperature=1.0, topp=0.9, rng_state=1234)[0]] == plain
    ctx.reset_kv()
    ids, st = ctx.generate_ex(prompt, 0, 32, s, rng_state=1234)
    assert [int(x) for x in ids] == pen and st == spen


def _caches(ctx, cfg):
    n = cfg.n_heads * MAX_SEQ * (cfg.dim // cfg.n_heads)
    return [ctx.debug_read(w, l, n).view(np.uint32).reshape(cfg.n_heads, MAX_SEQ, -1) for l in range(cfg.n_layers) for w in ("kcache", "vcache")]


def test_stop_token_under_controls(gpu, ctxs):
    cfg, ctx = ctxs("tiny")
    prompt = _prompt(cfg.vocab_size, 12)
    s = Sampling(temperature=1.0, topp=0.9, **CONTROLS)
    ref, _ = _ref(ctx, "tiny", prompt, 48, s, 77)
    js = [j for j in range(6, 40) if ref[j] not in ref[:j]]
    assert js
    j = js[0]
    # a stop token that is reached: delivered with last = 1, the KV rows as in flm_generate (the stop token is not fed), out_tokens behind *n_out untouched
    ctx.reset_kv()
    t = np.ascontiguousarray(prompt); out = np.full(48, -7, np.int32); st = C.c_uint64(77); n_out = C.c_int(0)
    sp, keep = s.struct()
    seen = []
    cb = gpu.TOKEN_CB(lambda _u, i, tok, last: seen.append((i, tok, last)) or 0)
    rc = gpu.lib().flm_generate_ex(ctx._h, gpu._p(t), len(t), 0, 48, C.byref(sp), C.byref(st), C.c_int32(ref[j]), cb, None, gpu._p(out), C.byref(n_out))
    assert rc == 0 and n_out.value == j + 1
    assert list(out[:j + 1]) == ref[:j + 1] and (out[j + 1:] == -7).all()
    assert seen == [(i, ref[i], int(i == j)) for i in range(j + 1)]
    assert st.value == advance_state(77, j + 1) and ctx.query("gen_tokens") == j + 1
    for c in _caches(ctx, cfg):
        assert c[:, 12 + j - 1, :].any() and not c[:, 12 + j:, :].any()
    # a banned id as the stop token is never delivered: the run goes to max_tokens and equals the host loop under the ban
    ban = ref[3]
    sb = Sampling(temperature=1.0, topp=0.9, top_k=5, repeat_penalty=1.3, penalty_last_n=8, bias={ban: -np.inf})
    want, _ = _ref(ctx, "tiny", prompt, 24, sb, 77)
    ctx.reset_kv()
    ids, _ = ctx.generate_ex(prompt, 0, 24, sb, rng_state=77, stop_token=ban)
    assert [int(x) for x in ids] == want and len(ids) == 24 and ban not in ids


def test_cancel_from_the_callback_under_controls(gpu, ctxs):
    cfg, ctx = ctxs("tiny")
    prompt = _prompt(cfg.vocab_size, 12)
    s = Sampling(temperature=1.0, topp=0.9, **CONTROLS)
    ref, _ = _ref(ctx, "tiny", prompt, 200, s, 77)
    ctx.reset_kv()
    entered = []

    def on_token(i, tok, last):
        entered.append((i, tok))
        return i == 3
    ids, st = ctx.generate_ex(prompt, 0, 200, s, rng_state=77, on_token=on_token)
    n_out = len(ids)
    print(f"cancel at index 3 of 200: n_out = {n_out}")
    assert n_out >= 4 and [int(x) for x in ids] == ref[:n_out] and st == advance_state(77, n_out)
    assert entered == [(i, ref[i]) for i in range(4)]


def test_a_retried_call_delivers_every_index_once(gpu):
    """the injected wait failure: the first attempt runs through on garbage, the call re-runs from the caller's state and rebuilds its windows from the ids it draws again"""
    cfg, ctx = _ctx(gpu, "7B-int8")
    prompt = _prompt(cfg.vocab_size, 5)
    s = Sampling(temperature=1.0, topp=0.9, **CONTROLS)
    ref, sref = host_loop(ctx, host_lib(), prompt, 24, s, 1234)
    ctx.reset_kv()
    ctx.set_option("inject_wait_failure", 1)
    seen = []
    ids, st = ctx.generate_ex(prompt, 0, 24, s, rng_state=1234, on_token=lambda i, tok, last: seen.append((i, tok, last)) and None)
    assert [int(x) for x in ids] == ref and st == sref
    assert seen == [(i, ref[i], i == 23) for i in range(24)]
    assert ctx.query("fallback") == 1
    ctx.close()


def test_forward_sample_ex_is_one_step_of_the_host_loop(gpu, ctxs):
    cfg, ctx = ctxs("tiny")
    prompt = _prompt(cfg.vocab_size, 9)
    window = np.array([3, 3, 40, 7, 250, 40, 40], np.int32)
    for t, seed in ((1.0, 4321), (0.0, 0)):
        s = Sampling(temperature=t, topp=0.9, top_k=5, min_p=0.05, repeat_penalty=1.3, frequency_penalty=0.2, presence_penalty=0.1, bias={3: 2.0, 7: -np.inf})
        ctx.reset_kv()
        want = _draw(gpu, ctx.forward(prompt, 0), s, window, seed)
        ctx.reset_kv()
        assert ctx.forward_sample_ex(prompt, 0, s, window, rng_state=seed) == want
        # neutral: flm_forward_sample / flm_forward_argmax
        ctx.reset_kv()
        plain = ctx.forward_sample(prompt, 0, t, 0.9, seed) if t else (ctx.forward_argmax(prompt, 0), seed)
        ctx.reset_kv()
        assert ctx.forward_sample_ex(prompt, 0, Sampling(temperature=t, topp=0.9), (), rng_state=seed) == plain


def test_temperature_zero_has_no_vocabulary_bound(gpu):
    """vocab 40000 (above the sampler's LDS bound): at temperature 0 the shaped form runs and equals the host loop; at temperature != 0 the sampler's refusal stays"""
    cfg = synth.make_config("tiny", ff.QT_INT8)
    cfg.vocab_size = 40000
    ctx = gpu.Ctx(gpu.desc_from_config(cfg, max_seq_len=64)); ctx.upload_all(synth.make_tensors(cfg, seed=59))
    prompt = _prompt(cfg.vocab_size, 5)
    s = Sampling(temperature=0.0, top_k=5, repeat_penalty=1.3, penalty_last_n=8, bias={3: 2.0})
    ref, _ = host_loop(ctx, host_lib(), prompt, 12, s, 0)
    ctx.reset_kv()
    ids, _ = ctx.generate_ex(prompt, 0, 12, s)
    assert [int(x) for x in ids] == ref
    with pytest.raises(gpu.FlmError, match="flm error -2"):
        ctx.generate_ex(prompt, 0, 12, Sampling(temperature=1.0, top_k=5), rng_state=1)
    ctx.close()


def test_invalid_arguments_launch_nothing(gpu, ctxs):
    cfg, ctx = ctxs("tiny")
    V = cfg.vocab_size
    prompt = _prompt(V, 5)
    ctx.reset_kv()
    logits = ctx.forward(prompt, 0)
    nxt = ctx.forward(np.array([9], np.int32), 5)
    counts = [ctx.query(k) for k in ("shaped_tokens", "sampled_tokens", "gen_tokens")]
    nan, inf = float("nan"), float("inf")
    bad = [Sampling(top_k=-1), Sampling(min_p=1.0), Sampling(min_p=-0.5), Sampling(min_p=nan), Sampling(repeat_penalty=0.0), Sampling(repeat_penalty=nan),
           Sampling(frequency_penalty=nan), Sampling(presence_penalty=nan), Sampling(penalty_last_n=-1), Sampling(penalty_last_n=1025), Sampling(bias={V: 1.0}),
           Sampling(bias={-1: 1.0}), Sampling(bias=([3, 3], [1.0, 2.0])), Sampling(bias={3: nan}), Sampling(bias={3: inf}), Sampling(bias=(list(range(257)), [0.0] * 257))]
    for s in bad:
        s.temperature = 1.0
        with pytest.raises(gpu.FlmError, match="flm error -1"):
            ctx.generate_ex(prompt, 0, 8, s, rng_state=1)
        with pytest.raises(gpu.FlmError, match="flm error -1"):
            ctx.forward_sample_ex(np.array([9], np.int32), 5, s, (), rng_state=1)
    for w in ([V], [-1], [0] * 1025):
        with pytest.raises(gpu.FlmError, match="flm error -1"):
            ctx.forward_sample_ex(np.array([9], np.int32), 5, Sampling(temperature=1.0, repeat_penalty=1.1), w, rng_state=1)
    lib = gpu.lib()
    t = np.array([9], np.int32); one = C.c_int32(0); st = C.c_uint64(1); n_out = C.c_int(0)
    assert lib.flm_forward_sample_ex(ctx._h, gpu._p(t), 1, 5, None, None, 0, C.byref(st), C.byref(one)) == -1
    assert lib.flm_generate_ex(ctx._h, gpu._p(prompt), 5, 0, 8, None, C.byref(st), -1, C.cast(None, gpu.TOKEN_CB), None, None, C.byref(n_out)) == -1
    sp, keep = Sampling(temperature=1.0, top_k=5).struct()
    assert lib.flm_generate_ex(ctx._h, gpu._p(prompt), 5, 0, 8, C.byref(sp), None, -1, C.cast(None, gpu.TOKEN_CB), None, None, C.byref(n_out)) == -1     # no state at temperature != 0
    with pytest.raises(gpu.FlmError, match="flm error -1"):
        ctx.generate_ex(prompt, 0, MAX_SEQ, Sampling(temperature=1.0, top_k=5), rng_state=1)          # past max_seq_len
    # nothing ran: the counters stand, and the decode state and cache are what the forwards above left
    assert [ctx.query(k) for k in ("shaped_tokens", "sampled_tokens", "gen_tokens")] == counts
    assert np.array_equal(bits(ctx.forward(np.array([9], np.int32), 5)), bits(nxt))
    ctx.reset_kv()
    assert np.array_equal(bits(ctx.forward(prompt, 0)), bits(logits))
    tp = gpu.Ctx(gpu.desc_from_config(cfg, max_seq_len=MAX_SEQ), rank=0, world=2)
    with pytest.raises(gpu.FlmError, match="flm error -2"):
        tp.generate_ex(prompt, 0, 4, Sampling(temperature=0.0, top_k=5))
    tp.close()


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
    ctx.prepare()
    prompt = np.array([1] + [int(x) for x in (np.arange(1, nprompt) * 7919) % cfg.vocab_size], np.int32)
    s = capi.Sampling(temperature=temp, topp=0.9, top_k=5, min_p=0.05, repeat_penalty=1.3, penalty_last_n=8, bias={3: 2.0, 7: -np.inf})
    seen = []
    a0, f0 = cnt.hipcount_allocs(), free_bytes()
    ids, _ = ctx.generate_ex(prompt, 0, 40, s, rng_state=1234, on_token=lambda i, t, last: seen.append(t) and None)     # the context's FIRST call
    a1, f1 = cnt.hipcount_allocs(), free_bytes()
    out[shape] = {"allocs": a1 - a0, "free_delta": f0 - f1, "n": len(ids), "same": [int(x) for x in ids] == seen, "counted_before": a0, "shaped": ctx.query("shaped_tokens")}
    ctx.close()
print("ALLOC " + json.dumps(out))
"""


def test_nothing_is_allocated_inside_generate_ex(gpu):
    """the first flm_generate_ex behind flm_prepare, bracketed with the allocation counter of tests/helpers/hipcount.c and hipMemGetInfo (as tests/test_gpu_generate.py
    brackets flm_generate)"""
    so = os.path.join(ROOT, "tests", "helpers", "libhipcount.so")
    assert os.path.exists(so), "tests/helpers/libhipcount.so missing: run __graft_entry__.build()"
    preload = os.pathsep.join(x for x in (so, os.environ.get("LD_PRELOAD", "")) if x)
    r = subprocess.run([sys.executable, "-c", _ALLOC_CHILD], capture_output=True, text=True, timeout=600, env=dict(os.environ, LD_PRELOAD=preload, FLM_ROOT=ROOT), cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads([l for l in r.stdout.splitlines() if l.startswith("ALLOC ")][-1][6:])
    for shape, v in res.items():
        assert v["counted_before"] > 20, f"{shape}: the interposer saw no allocation at create / upload -- it is not interposing"
        assert v["n"] == 40 and v["same"] and v["shaped"] == 40
        assert v["allocs"] == 0, f"{shape}: {v['allocs']} allocation calls inside flm_generate_ex"
        assert v["free_delta"] <= 0, f"{shape}: {v['free_delta']} bytes less free device memory after flm_generate_ex"


# ---- bin/main ----------------------------------------------------------------------------------------------------------------------------------------------------
def test_cli_flags_give_the_host_loops_text(gpu, tmp_path):
    """bin/main on the tiny .flm with --top-k 5 --repeat-penalty 1.3 --repeat-last-n 8 --seed 7 -t 1 -p 0.9: the text is the host loop's ids decoded (the CLI's sampler state
    is the reference's: 0 whatever --seed says, so every coin is 0); without the new flags the transcript is what it is today (flm_generate's ids)"""
    from fast_llama_amd import capi
    cfg = synth.make_config("tiny", ff.QT_INT8)
    path = str(tmp_path / "tiny.flm")
    tensors = synth.write_synthetic_flm(path, cfg, seed=1)           # (model seed 1: picked on the CPU oracle so that the flags change the ids, at index 8)
    H = C.CDLL(os.path.join(graft.PKG_DIR, "lib", "libflm_host.so"))
    H.fh_open.restype = C.c_void_p
    H.fh_open.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_int]
    H.fh_decode_one.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_char_p, C.c_int]
    h = H.fh_open(path.encode(), b"", 0, 1)
    assert h

    def text_of(ids):
        out, prev, buf = b"", -1, C.create_string_buffer(256)
        for t in ids:
            H.fh_decode_one(h, int(t), prev, buf, 256)
            out += buf.value; prev = int(t)
        return out

    def run(*extra):
        r = subprocess.run([MAIN, "-c", path, "-j", "1", "-n", "24", "-i", "hello world and so on", "--seed", "7", "-t", "1", "-p", "0.9", *extra], capture_output=True, timeout=300)
        assert r.returncode == 0, r.stderr.decode(errors="replace")
        prompt = [int(x) for x in re.search(rb"Input tokens:\[([^\]]*)\]", r.stdout).group(1).replace(b",", b" ").split()]
        body = r.stdout[r.stdout.index(b"output: \x1b[32m") + len(b"output: \x1b[32m"):]
        return prompt, body[:body.index(b"\x1b[0m\n\nnum_threads")]

    ctx = capi.Ctx(capi.desc_from_config(cfg, max_seq_len=1024)); ctx.upload_all(tensors)

    def cut(ids):       # the CLI stops on token 0 (delivered)
        return ids[:ids.index(0) + 1] if 0 in ids else ids
    prompt, shaped_text = run("--top-k", "5", "--repeat-penalty", "1.3", "--repeat-last-n", "8")
    s = Sampling(temperature=1.0, topp=0.9, top_k=5, repeat_penalty=1.3, penalty_last_n=8)
    want, _ = host_loop(ctx, host_lib(), np.array(prompt, np.int32), 25, s, 0, stop=0)
    assert shaped_text == text_of(cut(want)) and len(shaped_text) > 0
    prompt2, plain_text = run()
    assert prompt2 == prompt and plain_text != shaped_text                     # (the texts differ too: equal text is not an accident of the tokenizer)
    ctx.reset_kv()
    plain = [int(x) for x in ctx.generate(np.array(prompt, np.int32), 0, 25, temperature=1.0, topp=0.9, rng_state=0, stop_token=0)[0]]
    assert plain_text == text_of(plain)
    assert plain != cut(want), "the flags must change the ids on this model, or the comparison above shows nothing"
    ctx.close(); H.fh_close.argtypes = [C.c_void_p]; H.fh_close(h)
