"""The split-K skinny int8 GEMM (k_gemm_q8_skinny_sk): passes of up to 16 rows of an INT8 context under "spec_gemm" 2 run four waves per workgroup, each on every
fourth quant group, and hand the exact group dots through LDS to the ordered chains.  Everything is bit equality: the op against the CPU oracle's matmul at QT_INT8,
the model against the oracle's greedy loop, K/V rows against the token path's."""
import ctypes

import numpy as np
import pytest

import oracle_py as O
from fast_llama_amd import capi, flmfile as ff, synth

pytestmark = pytest.mark.gpu
MAX_SEQ, N_PROMPT = 256, 9
LAYERS = {"tiny": None, "7B": 2}
_made = {}
bits = lambda a: np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)   # noqa: E731
ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)   # noqa: E731


# m: one fragment / a ragged second fragment under NB = 2 / 17 fragments
# n: one group (three waves idle throughout) / exactly one round / a ragged second round / 35 groups (past a wave's ring, a ragged last round) / 172 groups, m = 48
@pytest.mark.parametrize("nb", [0, 2], ids=["by-size", "two-fragments"])
@pytest.mark.parametrize("m,n", [(m, n) for m in (16, 48, 272) for n in (64, 256, 320, 2240)] + [(48, 11008)])
def test_splitk_skinny_gemm_is_the_oracles_matmul(gpu, m, n, nb, monkeypatch):
    """random int8 with the rows and columns that can go wrong planted; idle token columns and rows past the matrix store nothing (the op presets the output to NaN
    patterns)"""
    monkeypatch.setenv("FLM_OP_SKINNY_SPLITK", "1")
    if nb:
        monkeypatch.setenv("FLM_OP_SKINNY_NB", str(nb))
    for w in (1, 5, 16):
        rng = np.random.default_rng([m, n, w])
        W = rng.integers(-127, 128, size=(m, n), dtype=np.int8)
        X = rng.integers(-127, 128, size=(w, n), dtype=np.int8)
        sW = (rng.random((m, n // 64), dtype=np.float32) + np.float32(0.5)) * np.float32(1e-2) * rng.choice(np.array([1, -1], np.float32), (m, n // 64))
        sX = (rng.random((w, n // 64), dtype=np.float32) + np.float32(0.5)) * np.float32(1e-2)
        X[-1, -64:] = 0; sX[-1, -1] = 0.0                                       # a zero activation group with a zero scale
        X[0] = np.where(rng.random(n) < 0.5, -127, 127); X[0, :64] = 127        # +-127, group 0 all +: against row 0 the largest group dot, 64 * 127^2
        W[0] = 127; W[3] = 0; sW[4, 0] = 0.0                                    # (a saturated row; a zero row; a zero weight scale)
        got, want = gpu.op_matmul_skinny(W, sW, X, sX), O.matmul_q(ff.QT_INT8, W, sW, X, sX)
        assert np.array_equal(bits(got), bits(want)), (m, n, w, np.argwhere(bits(got) != bits(want))[:4].tolist())


def _model(gpu, name):
    """-> (cfg, a fresh INT8 context, the prompt, the oracle's first token behind the prompt, its 16 greedy ids from there); tensors and ids made once"""
    if name not in _made:
        cfg = synth.make_config(name, ff.QT_INT8)
        cfg.n_layers = LAYERS[name] or cfg.n_layers
        tensors = synth.make_tensors(cfg, seed=7)
        om = O.OracleModel(cfg, tensors, max_seq=MAX_SEQ)
        prompt = np.concatenate([[1], np.random.default_rng(3).integers(0, cfg.vocab_size, N_PROMPT - 1)]).astype(np.int32)
        ids = [int(np.argmax(om.forward(prompt, 0)))]
        for i in range(16):
            ids.append(int(np.argmax(om.forward(np.array(ids[-1:], dtype=np.int32), N_PROMPT + i))))
        _made[name] = (cfg, tensors, prompt, ids[0], np.array(ids[1:], dtype=np.int32))
    cfg, tensors, prompt, first, ids = _made[name]
    ctx = gpu.Ctx(gpu.desc_from_config(cfg, max_seq_len=MAX_SEQ)); ctx.upload_all(tensors)
    return cfg, ctx, prompt, first, ids


@pytest.mark.parametrize("name", list(LAYERS))
def test_verify_greedy_under_splitk_is_the_oracles_loop(gpu, name):
    """4 and 15 right drafts under "spec_gemm" 2 and 1: the ids are the oracle's greedy loop, the K/V rows of the accepted positions the token path's, and "pass_gemm"
    names the family that ran (ROPE_KV, RESIDUAL, SWIGLU and the classifier stage all go through it)"""
    (cfg, ref, prompt, first, ids), ctx = _model(gpu, name), _model(gpu, name)[1]
    hs = cfg.dim // cfg.n_heads
    caches = lambda c: [c.debug_read(w, l, cfg.n_heads * MAX_SEQ * hs).view(np.uint32).reshape(cfg.n_heads, MAX_SEQ, hs) for l in range(cfg.n_layers) for w in ("kcache", "vcache")]   # noqa: E731
    assert ref.forward_argmax(prompt, 0) == first and np.array_equal(ref.decode_greedy(first, N_PROMPT, len(ids)), ids)
    kv_ref = caches(ref)
    for k, gemm in [(k, gemm) for k in (4, 15) for gemm in (2, 1)]:
        ctx.set_option("spec_gemm", gemm)
        ctx.reset_kv()
        assert ctx.forward_argmax(prompt, 0) == first
        got = ctx.verify_greedy(first, ids[:k], N_PROMPT)
        assert np.array_equal(got, ids[:k + 1]), (k, gemm, list(got), list(ids[:k + 1]))
        assert ctx.query("pass_gemm") == (5 if gemm == 2 else 1), (k, gemm)
        assert all(np.array_equal(a[:, :N_PROMPT + k + 1], b[:, :N_PROMPT + k + 1]) for a, b in zip(caches(ctx), kv_ref)), (k, gemm)
    assert ctx.query("fallback") == 0
    ref.close(); ctx.close()


def test_slots_and_fan_under_splitk(gpu):
    """one generate_batch of 3 requests and one generate_n of 4 sequences on `tiny`: under "spec_gemm" 2 (through the new kernel) the ids of "spec_gemm" 0"""
    _, ctx, prompt, _, _ = _model(gpu, "tiny")
    reqs, got = [capi.BatchReq(prompt[:n], 6) for n in (1, 4, 9)], {}
    for gemm in (0, 2):
        ctx.set_option("spec_gemm", gemm)
        ctx.reset_kv()
        batch = ctx.generate_batch(reqs)[0]
        assert ctx.query("pass_gemm") == (5 if gemm else 0)
        ctx.reset_kv()
        fan = ctx.generate_n(prompt[:4], 0, 6, n=4)[0]
        assert ctx.query("pass_gemm") == (5 if gemm else 0)
        got[gemm] = [np.asarray(a) for a in list(batch) + list(fan)]
    assert all(np.array_equal(a, b) for a, b in zip(got[2], got[0])) and ctx.query("fallback") == 0
    ctx.close()


def test_splitk_refusals(gpu, monkeypatch):
    """a value past 2 is refused and leaves the option alone; 17 rows are refused as by the plain op; an INT4 context under 2 runs its own skinny kernel"""
    _, ctx, _, _, _ = _model(gpu, "tiny")
    ctx.set_option("spec_gemm", 2)
    with pytest.raises(capi.FlmError):
        ctx.set_option("spec_gemm", 3)
    assert ctx.query("spec_gemm") == 2
    ctx.close()
    W, sW, X, sX, out = np.ones((16, 64), np.int8), np.ones((16, 1), np.float32), np.ones((17, 64), np.int8), np.ones((17, 1), np.float32), np.empty((17, 16), np.float32)
    plain = gpu.lib().flm_op_matmul_skinny(ff.QT_INT8, ptr(out), ptr(W), ptr(sW), ptr(X), ptr(sX), 16, 64, 17, 64)
    monkeypatch.setenv("FLM_OP_SKINNY_SPLITK", "1")
    assert gpu.lib().flm_op_matmul_skinny(ff.QT_INT8, ptr(out), ptr(W), ptr(sW), ptr(X), ptr(sX), 16, 64, 17, 64) == plain == -1
    cfg4, prompt = synth.make_config("tiny", capi.QT_INT4), np.arange(1, N_PROMPT + 1, dtype=np.int32)
    int4 = gpu.Ctx(gpu.desc_from_config(cfg4, max_seq_len=MAX_SEQ)); int4.upload_all(synth.make_tensors(cfg4, seed=7))
    int4.set_option("spec_gemm", 2)
    int4.verify_greedy(int4.forward_argmax(prompt, 0), prompt[:4], N_PROMPT)
    assert int4.query("pass_gemm") == 2 and int4.query("fallback") == 0
    int4.close()
