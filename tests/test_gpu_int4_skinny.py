"""The skinny W4A8 GEMM (k_gemm_q4_skinny): passes of up to 16 rows of an INT4 context under "spec_gemm" 1 read the packed nibbles.  The rule is test_gpu_int4's: the
expected values are the unchanged CPU oracle at QT_INT8 on the sign-extended nibbles (oracle_py.matmul_q, OracleModel on synth.int8_statement), compared bit for bit.
K/V rows, which the oracle does not hand out, are compared with the token path's on a second INT4 context (test_gpu_int4 ties that path's logits to the oracle)."""
import ctypes

import numpy as np
import pytest

import oracle_py as O
from fast_llama_amd import capi, flmfile as ff, synth

pytestmark = pytest.mark.gpu
MAX_SEQ, N_PROMPT = 256, 37
LAYERS = {"tiny": None, "7B": 2}
_made = {}
bits = lambda a: np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)   # noqa: E731


def _gemm_case(m, n, w):
    rng = np.random.default_rng([m, n, w])
    W = rng.integers(-8, 8, size=(m, n), dtype=np.int8)
    X = rng.integers(-127, 128, size=(w, n), dtype=np.int8)
    sW = (rng.random((m, n // 64), dtype=np.float32) + np.float32(0.5)) * np.float32(1e-2) * rng.choice(np.array([1, -1], np.float32), (m, n // 64))
    sX = (rng.random((w, n // 64), dtype=np.float32) + np.float32(0.5)) * np.float32(1e-2)
    X[0] = np.where(rng.random(n) < 0.5, -127, 127); W[0] = -8               # an all -8 row against +-127: the largest offset term
    W[1] = 7; W[2] = 0; sW[3, 0] = 0.0
    return capi.pack_int4(W), sW, X, sX, O.matmul_q(O.QT_INT8, W, sW, X, sX)


# n: one group / two / 11 (inside the ring's first fill, a tail round behind it) / 64 and 172 (the test-free full rounds of both ring depths, the wrap, a partial tail)
@pytest.mark.parametrize("nb", [0, 2], ids=["by-size", "two-fragments"])
@pytest.mark.parametrize("n", [64, 128, 704, 4096, 11008])
@pytest.mark.parametrize("m", [16, 48, 272])
def test_skinny_w4_gemm_is_the_oracles_int8_matmul(gpu, m, n, nb, monkeypatch):
    """m = one fragment / rows past the matrix / several workgroups.  Idle token columns and rows past the matrix store nothing (the op presets the output to NaN
    patterns); at w = 16 also equal to unpack + tiles."""
    if nb:
        monkeypatch.setenv("FLM_OP_SKINNY_NB", str(nb))
    for w in (1, 2, 5, 15, 16):
        P, sW, X, sX, want = _gemm_case(m, n, w)
        got = gpu.op_matmul_skinny(P, sW, X, sX, qt=capi.QT_INT4)
        assert np.array_equal(bits(got), bits(want)), (m, n, w, np.argwhere(bits(got) != bits(want))[:4].tolist())
        if w == 16:
            assert np.array_equal(bits(got), bits(gpu.op_matmul_q(capi.QT_INT4, P, sW, X, sX))), (m, n)


def test_skinny_w4_gemm_refuses_more_than_16_rows(gpu):
    P, sW, X, sX, _ = _gemm_case(16, 64, 16)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)   # noqa: E731
    out, X17, s17 = np.empty((17, 16), np.float32), np.zeros((17, 64), np.int8), np.zeros((17, 1), np.float32)
    assert gpu.lib().flm_op_matmul_skinny(capi.QT_INT4, p(out), p(P), p(sW), p(X17), p(s17), 16, 64, 17, 64) == -1


def _model(name):
    """-> (cfg, INT4 tensors, the prompt, {pos: the oracle's first token and 19 greedy ids from there}), made once"""
    if name not in _made:
        cfg, cfg8 = synth.make_config(name, capi.QT_INT4), synth.make_config(name, ff.QT_INT8)
        cfg.n_layers = cfg8.n_layers = LAYERS[name] or cfg.n_layers
        tensors = synth.make_tensors(cfg, seed=7)
        om = O.OracleModel(cfg8, synth.int8_statement(tensors), max_seq=MAX_SEQ)
        prompt = np.concatenate([[1], np.random.default_rng(3).integers(0, cfg.vocab_size, N_PROMPT - 1)]).astype(np.int32)
        loops = {}
        for pos in (0, N_PROMPT):
            om.reset()
            ids = [int(np.argmax(om.forward(prompt, 0))) if pos else 1]
            for i in range(19):
                ids.append(int(np.argmax(om.forward(np.array(ids[-1:], dtype=np.int32), pos + i))))
            loops[pos] = (ids[0], np.array(ids[1:], dtype=np.int32))
        _made[name] = (cfg, tensors, prompt, loops)
    return _made[name]


def _ctx(gpu, cfg, tensors):
    ctx = gpu.Ctx(gpu.desc_from_config(cfg, max_seq_len=MAX_SEQ)); ctx.upload_all(tensors)
    return ctx


def _caches(ctx, cfg):
    hs = cfg.dim // cfg.n_heads
    return [ctx.debug_read(w, l, cfg.n_heads * MAX_SEQ * hs).view(np.uint32).reshape(cfg.n_heads, MAX_SEQ, hs) for l in range(cfg.n_layers) for w in ("kcache", "vcache")]


@pytest.mark.parametrize("pos", [0, N_PROMPT])
@pytest.mark.parametrize("name", list(LAYERS))
def test_verify_greedy_on_int4_is_the_oracles_loop(gpu, name, pos):
    """k = 4 and 15 drafts with none / draft 0 / draft k - 1 made wrong, "spec_gemm" 1 and 0: the ids and their count are the oracle's greedy loop, the K/V rows pos ..
    pos + m of every layer the token path's, and three more tokens of the decode loop behind them the oracle's again (ROPE_KV, RESIDUAL, SWIGLU and the classifier stage)"""
    cfg, tensors, prompt, loops = _model(name)
    first, ids = loops[pos]
    ref, ctx = _ctx(gpu, cfg, tensors), _ctx(gpu, cfg, tensors)

    def start(c):
        c.reset_kv()
        return c.forward_argmax(prompt, 0) if pos else 1
    assert start(ref) == first and np.array_equal(ref.decode_greedy(first, pos, len(ids)), ids)
    kv_ref = _caches(ref, cfg)
    for k, wrong, gemm in [(k, wrong, gemm) for k in (4, 15) for wrong in (None, 0, k - 1) for gemm in (1, 0)]:
        drafts = ids[:k].copy()
        if wrong is not None:
            drafts[wrong] = (drafts[wrong] + 1) % cfg.vocab_size
        m = k if wrong is None else wrong
        ctx.set_option("spec_gemm", gemm)
        assert start(ctx) == first
        got = ctx.verify_greedy(first, drafts, pos)
        assert np.array_equal(got, ids[:m + 1]), (k, wrong, gemm, list(got), list(ids[:m + 1]))
        for a, b in zip(_caches(ctx, cfg), kv_ref):
            assert np.array_equal(a[:, :pos + m + 1], b[:, :pos + m + 1]), (k, wrong, gemm)
        assert np.array_equal(ctx.decode_greedy(int(got[-1]), pos + m + 1, 3), ids[m + 1:m + 4]), (k, wrong, gemm)
    assert ctx.query("fallback") == 0
    ref.close(); ctx.close()


def test_slots_and_fan_on_int4_under_both_settings(gpu):
    """one generate_batch of 5 short prompts and one generate_n with n = 4 on `tiny`: the same ids under "spec_gemm" 1 and 0, and those of a generate per request"""
    cfg, tensors, prompt, _ = _model("tiny")
    ctx = _ctx(gpu, cfg, tensors)
    prompts, alone = [prompt[:n] for n in (1, 3, 6, 9, 17)], []
    for p in prompts:
        ctx.reset_kv(); alone.append(ctx.generate(p, 0, 6)[0])
    for gemm in (1, 0):
        ctx.set_option("spec_gemm", gemm)
        ctx.reset_kv()
        got = ctx.generate_batch([capi.BatchReq(p, 6) for p in prompts])[0]
        assert all(np.array_equal(g, a) for g, a in zip(got, alone)), (gemm, "batch")
        ctx.reset_kv()
        assert all(np.array_equal(f, alone[3]) for f in ctx.generate_n(prompts[3], 0, 6, n=4)[0]), (gemm, "fan")
    assert ctx.query("fallback") == 0
    ctx.close()
