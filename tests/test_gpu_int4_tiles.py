"""The W4A8 GEMM tiles (k_gemm_q4_mfma): every batched pass of an INT4 context that is not a skinny one reads the packed nibbles through 64 x 64 / 128 x 128 tiles.
The rule is test_gpu_int4's: the expected values are the unchanged CPU oracle at QT_INT8 on the sign-extended nibbles, compared bit for bit -- there is no tolerance."""
import numpy as np
import pytest

import oracle_py as O
from fast_llama_amd import capi, flmfile as ff, synth
from score_util import same_scores
from test_gpu_int4_skinny import LAYERS, MAX_SEQ, _caches, _ctx, _gemm_case, bits

pytestmark = pytest.mark.gpu
N_PROMPT, K = 130, 15


# m: one tile / rows past the matrix inside a tile / several tiles with a partial last one (both shapes); n: one group (a stage with an empty half) / an odd group count
# over two stages / 11 groups; w: 48 or 112 dead token columns / a second 64-token tile with one live token / a second 128-token tile
@pytest.mark.parametrize("w", [16, 65, 130])
@pytest.mark.parametrize("n", [64, 192, 704])
@pytest.mark.parametrize("m", [64, 80, 272])
def test_w4_tiles_are_the_oracles_int8_matmul(gpu, m, n, w, monkeypatch):
    """both tile shapes on an all -8 row against +-127 activations, an all-7 row, a zero row and a zero scale"""
    P, sW, X, sX, want = _gemm_case(m, n, w)
    for shape in ("2", "3"):
        monkeypatch.setenv("FLM_OP_GEMM", shape)
        got = gpu.op_matmul_q(capi.QT_INT4, P, sW, X, sX)
        assert np.array_equal(bits(got), bits(want)), (m, n, w, shape, np.argwhere(bits(got) != bits(want))[:4].tolist())


@pytest.mark.parametrize("name", list(LAYERS))
def test_prompt_and_verify_pass_on_the_nibble_tiles(gpu, name):
    """a 130-token prompt batched, then a verify pass of 16 rows under "spec_gemm" 0: logits and ids the oracle's loop, K/V rows of every layer those of a context fed
    token by token (ROPE_KV, RESIDUAL, SWIGLU, the classifier stage); "pass_gemm" names the family that ran: 3 the nibble tiles, 2 the skinny nibbles"""
    cfg, cfg8 = synth.make_config(name, capi.QT_INT4), synth.make_config(name, ff.QT_INT8)
    cfg.n_layers = cfg8.n_layers = LAYERS[name] or cfg.n_layers
    tensors = synth.make_tensors(cfg, seed=7)
    om = O.OracleModel(cfg8, synth.int8_statement(tensors), max_seq=MAX_SEQ)
    prompt = np.concatenate([[1], np.random.default_rng(5).integers(0, cfg.vocab_size, N_PROMPT - 1)]).astype(np.int32)
    want = om.forward(prompt, 0)
    ids = [int(np.argmax(want))]
    for i in range(K + 4):
        ids.append(int(np.argmax(om.forward(np.array(ids[-1:], dtype=np.int32), N_PROMPT + i))))
    first, ids = ids[0], np.array(ids[1:], dtype=np.int32)
    ref, ctx = _ctx(gpu, cfg, tensors), _ctx(gpu, cfg, tensors)
    for i in range(N_PROMPT):
        ref.forward(prompt[i:i + 1], i)
    assert np.array_equal(ref.decode_greedy(first, N_PROMPT, len(ids)), ids)
    kv_ref = _caches(ref, cfg)
    assert np.array_equal(bits(ctx.forward(prompt, 0)), bits(want))
    assert ctx.query("pass_gemm") == 3
    for a, b in zip(_caches(ctx, cfg), kv_ref):
        assert np.array_equal(a[:, :N_PROMPT], b[:, :N_PROMPT])
    for gemm, kind in ((0, 3), (1, 2)):
        ctx.set_option("spec_gemm", gemm)
        ctx.reset_kv()
        assert ctx.forward_argmax(prompt, 0) == first
        got = ctx.verify_greedy(first, ids[:K], N_PROMPT)
        assert ctx.query("pass_gemm") == kind
        assert np.array_equal(got, ids[:K + 1]), (gemm, list(got))
        for a, b in zip(_caches(ctx, cfg), kv_ref):
            assert np.array_equal(a[:, :N_PROMPT + K + 1], b[:, :N_PROMPT + K + 1]), gemm
        assert np.array_equal(ctx.decode_greedy(int(got[-1]), N_PROMPT + K + 1, 3), ids[K + 1:K + 4]), gemm
    assert ctx.query("fallback") == 0
    ref.close(); ctx.close()


def test_score_tokens_in_two_classifier_chunks(gpu):
    """`tiny`, 40 positions, "score_rows" 20: the records of one row at a time"""
    cfg = synth.make_config("tiny", capi.QT_INT4)
    ctx = _ctx(gpu, cfg, synth.make_tensors(cfg, seed=7))
    toks = np.concatenate([[1], np.random.default_rng(9).integers(0, cfg.vocab_size, 39)]).astype(np.int32)
    ctx.set_option("score_rows", -1)
    one = ctx.score(toks, 0)
    ctx.set_option("score_rows", 20); ctx.reset_kv()
    two = ctx.score(toks, 0)
    assert ctx.query("pass_gemm") == 3 and same_scores(two, one)
    ctx.close()
