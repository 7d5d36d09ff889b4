"""The skinny int16 GEMM (k_gemm_q16_skinny): passes of up to 16 rows of an INT16 context under "spec_gemm" 1 read int16 weights straight into byte-plane operands.
Everything is bit equality: the op against the CPU oracle's matmul at QT_INT16, the model against the oracle's greedy loop, K/V rows against the token path's."""
import ctypes

import numpy as np
import pytest

import oracle_py as O
from fast_llama_amd import capi, flmfile as ff, synth

pytestmark = pytest.mark.gpu
MAX_SEQ, N_PROMPT, QMAX = 256, 9, 5792                   # (QMAX: the int16 quantizer's range, 64 * 5792^2 < 2^31)
LAYERS = {"tiny": None, "7B": 2}
_made = {}
bits = lambda a: np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)   # noqa: E731
ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)   # noqa: E731


# m: one full fragment / three workgroups, or a half-used second fragment under NB = 2 / 17 fragments
# n: one group / two / 11 (less than a ring round plus a partial) / 64 and 172 groups, m = 48 (the test-free full rounds, the ring's wrap, a last round that is not full)
@pytest.mark.parametrize("nb", [0, 2], ids=["by-size", "two-fragments"])
@pytest.mark.parametrize("m,n", [(m, n) for m in (16, 48, 272) for n in (64, 128, 704)] + [(48, 4096), (48, 11008)])
def test_skinny_int16_gemm_is_the_oracles_matmul(gpu, m, n, nb, monkeypatch):
    """random int16 inside the quantizer's range with the rows and columns that can go wrong planted; idle token columns and rows past the matrix store nothing (the
    op presets the output to NaN patterns)"""
    monkeypatch.setenv("FLM_OP_GEMM", "skinny")
    if nb:
        monkeypatch.setenv("FLM_OP_SKINNY_NB", str(nb))
    for w in (1, 2, 5, 15, 16):
        rng = np.random.default_rng([m, n, w])
        W = rng.integers(-QMAX, QMAX + 1, size=(m, n)).astype(np.int16)
        X = rng.integers(-QMAX, QMAX + 1, size=(w, n)).astype(np.int16)
        sW = (rng.random((m, n // 64), dtype=np.float32) + np.float32(0.5)) * np.float32(1e-4) * rng.choice(np.array([1, -1], np.float32), (m, n // 64))
        sX = (rng.random((w, n // 64), dtype=np.float32) + np.float32(0.5)) * np.float32(1e-4)
        X[-1, -64:] = 0; sX[-1, -1] = 0.0                                       # a zero activation group with a zero scale
        X[0] = np.where(rng.random(n) < 0.5, -QMAX, QMAX); X[0, :64] = QMAX     # +-5792, group 0 all +: against row 0 the largest group dot, 64 * 5792^2
        W[0] = QMAX; W[1] = -1; W[3] = 0; sW[4, 0] = 0.0                        # (-1: lo = -1, hi = 0; a zero row; a zero weight scale)
        W[2] = np.resize(np.array([127, 128, -128, -129, 255, 256], np.int16), n)   # every carry of split16
        got, want = gpu.op_matmul_q(ff.QT_INT16, W, sW, X, sX), O.matmul_q(ff.QT_INT16, W, sW, X, sX)
        assert np.array_equal(bits(got), bits(want)), (m, n, w, np.argwhere(bits(got) != bits(want))[:4].tolist())


def test_skinny_int16_gemm_refusals(gpu, monkeypatch):
    W, sW, X, sX, out = np.ones((16, 64), np.int16), np.ones((16, 1), np.float32), np.ones((17, 64), np.int16), np.ones((17, 1), np.float32), np.empty((17, 16), np.float32)
    assert gpu.lib().flm_op_matmul_skinny(ff.QT_INT16, ptr(out), ptr(W), ptr(sW), ptr(X), ptr(sX), 16, 64, 16, 64) == -2      # int16 goes through flm_op_matmul_q
    monkeypatch.setenv("FLM_OP_GEMM", "skinny")
    assert gpu.lib().flm_op_matmul_q(ff.QT_INT16, ptr(out), ptr(W), ptr(sW), ptr(X), ptr(sX), 16, 64, 17, 64) == -1            # more than 16 rows


def _model(gpu, name):
    """-> (cfg, a fresh INT16 context, the prompt, the oracle's first token behind the prompt, its 16 greedy ids from there); tensors and ids made once"""
    if name not in _made:
        cfg = synth.make_config(name, ff.QT_INT16)
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
def test_verify_greedy_on_int16_is_the_oracles_loop(gpu, name):
    """4 and 15 right drafts under "spec_gemm" 1 and 0: the ids are the oracle's greedy loop, the K/V rows of the accepted positions the token path's, and "pass_gemm"
    names the family that ran (ROPE_KV, RESIDUAL, SWIGLU and the classifier stage all go through it)"""
    (cfg, ref, prompt, first, ids), ctx = _model(gpu, name), _model(gpu, name)[1]
    hs = cfg.dim // cfg.n_heads
    caches = lambda c: [c.debug_read(w, l, cfg.n_heads * MAX_SEQ * hs).view(np.uint32).reshape(cfg.n_heads, MAX_SEQ, hs) for l in range(cfg.n_layers) for w in ("kcache", "vcache")]   # noqa: E731
    assert ref.forward_argmax(prompt, 0) == first and np.array_equal(ref.decode_greedy(first, N_PROMPT, len(ids)), ids)
    kv_ref = caches(ref)
    for k, gemm in [(k, gemm) for k in (4, 15) for gemm in (1, 0)]:
        ctx.set_option("spec_gemm", gemm)
        ctx.reset_kv()
        assert ctx.forward_argmax(prompt, 0) == first
        got = ctx.verify_greedy(first, ids[:k], N_PROMPT)
        assert np.array_equal(got, ids[:k + 1]), (k, gemm, list(got), list(ids[:k + 1]))
        assert ctx.query("pass_gemm") == (4 if gemm else 0), (k, gemm)
        assert all(np.array_equal(a[:, :N_PROMPT + k + 1], b[:, :N_PROMPT + k + 1]) for a, b in zip(caches(ctx), kv_ref)), (k, gemm)
    assert ctx.query("fallback") == 0
    ref.close(); ctx.close()


def test_slots_and_fan_on_int16_under_both_settings(gpu):
    """one generate_batch of 3 requests and one generate_n of 4 sequences on `tiny`: under "spec_gemm" 1 (through the new kernel) the ids of "spec_gemm" 0"""
    _, ctx, prompt, _, _ = _model(gpu, "tiny")
    reqs, got = [capi.BatchReq(prompt[:n], 6) for n in (1, 4, 9)], {}
    for gemm in (0, 1):
        ctx.set_option("spec_gemm", gemm)
        ctx.reset_kv()
        batch = ctx.generate_batch(reqs)[0]
        assert ctx.query("pass_gemm") == (4 if gemm else 0)
        ctx.reset_kv()
        fan = ctx.generate_n(prompt[:4], 0, 6, n=4)[0]
        assert ctx.query("pass_gemm") == (4 if gemm else 0)
        got[gemm] = [np.asarray(a) for a in list(batch) + list(fan)]
    assert all(np.array_equal(a, b) for a, b in zip(got[1], got[0])) and ctx.query("fallback") == 0
    ctx.close()
