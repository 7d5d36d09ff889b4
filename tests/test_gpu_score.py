"""flm_score_tokens: every position's logits in one batched pass, reduced on the device to a flm_score per row (argmax, the clipped softmax's max / sequential sum, the
target's logit and probability).  Everything is compared on bit patterns.

Expected logits come from the CPU oracle fed token by token (or, at 7B width, from flm_forward on the same context), expected rows from the host restatement
(host/test_shim.cpp fh_score_row).  max_seq_len is 256 throughout."""
import ctypes

import numpy as np
import pytest

import oracle_py as O
from fast_llama_amd import flmfile as ff, synth
from sample_util import logits_case
from score_util import clipped_terms, diff_scores, host_score, next_targets, same_scores, teeth_row, tree_sum

pytestmark = pytest.mark.gpu
MAX_SEQ = 256
NS = (1, 2, 5, 6, 17, 64, 65, 130)
MODELS = {
    "tiny-int8": ("tiny", ff.QT_INT8, 5, False),
    "tiny-int16": ("tiny", ff.QT_INT16, 5, False),
    "tiny128-int8": ("tiny128", ff.QT_INT8, 5, False),
    "tiny-qemb": ("tiny", ff.QT_INT8, 3, True),                          # quantized embedding table
    "v323-int8": ((256, 512, 2, 4, 323), ff.QT_INT8, 5, False),         # vocabulary not a multiple of 64
}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _tokens(V, n, seed=1):
    rng = np.random.default_rng(seed)
    return np.concatenate([[1], rng.integers(0, V, n - 1)]).astype(np.int32)


_made = {}


def _model(name):
    """(cfg, tensors, tokens[130], the oracle's logits per position [130][V]) -- computed once per model, shared by the tests"""
    if name not in _made:
        shape, qt, seed, qemb = MODELS[name]
        cfg = synth.make_config(shape, qt)
        tensors = synth.make_tensors(cfg, seed=seed)
        if qemb:
            emb = tensors[(ff.T_TOKEN_EMBD, 0)]
            q, s = O.quantize(emb.reshape(-1), qt)
            tensors[(ff.T_TOKEN_EMBD, 0)] = (q.reshape(emb.shape), s.reshape(emb.shape[0], -1))
        toks = _tokens(cfg.vocab_size, max(NS))
        om = O.OracleModel(cfg, tensors, max_seq=MAX_SEQ)
        want = np.stack([om.forward(toks[i:i + 1], i) for i in range(len(toks))])
        _made[name] = (cfg, tensors, toks, want)
    return _made[name]


def _ctx(gpu, cfg, tensors):
    ctx = gpu.Ctx(gpu.desc_from_config(cfg, max_seq_len=MAX_SEQ)); ctx.upload_all(tensors)
    return ctx


def _caches(ctx, cfg):
    n = cfg.n_heads * MAX_SEQ * (cfg.dim // cfg.n_heads)
    return [ctx.debug_read(w, l, n).view(np.uint32) for l in range(cfg.n_layers) for w in ("kcache", "vcache")]


@pytest.mark.parametrize("name", list(MODELS))
def test_scores_and_logits_match_the_oracle(gpu, name):
    """every n (1 and 2: the token path; 5: the smallest batch; 64 / 65: a tile edge; 130: three token tiles): logits_all, every field of every row, the row without a target"""
    cfg, tensors, toks, want = _model(name)
    ctx = _ctx(gpu, cfg, tensors)
    for n in NS:
        ctx.reset_kv()
        got, lg = ctx.score(toks[:n], 0, want_logits=True)
        assert np.array_equal(bits(lg), bits(want[:n])), (name, n, np.nonzero((bits(lg) != bits(want[:n])).any(axis=1))[0][:8])
        exp = host_score(want[:n], next_targets(toks[:n]))
        assert same_scores(got, exp), (name, n, diff_scores(got, exp))
        assert got["prob"][-1] == 0.0 and got["target_logit"][-1] == 0.0 and got["argmax"][-1] == int(np.argmax(want[n - 1]))
    # explicit targets: none (-1), the argmax itself, an arbitrary id, the last row with a target
    n = 17
    tg = np.array([(-1, int(np.argmax(want[i])), (7 * i + 3) % cfg.vocab_size)[i % 3] for i in range(n)], np.int32)
    ctx.reset_kv()
    got = ctx.score(toks[:n], 0, targets=tg)
    exp = host_score(want[:n], tg)
    assert same_scores(got, exp), (name, "targets", diff_scores(got, exp))
    assert np.all(got["prob"][tg < 0] == 0.0) and np.all(got["target_logit"][tg < 0] == 0.0)
    hit = tg == got["argmax"]
    assert hit.any() and np.array_equal(bits(got["target_logit"][hit]), bits(got["max_logit"][hit]))
    assert ctx.query("fallback") == 0
    ctx.close()


def test_chunks_of_a_context(gpu):
    """40 tokens at position 0, then 30 at 40 == one call over the 70; the K / V rows are flm_forward's; the greedy continuation is the same behind both"""
    cfg, tensors, toks, want = _model("tiny-int8")
    ctx = _ctx(gpu, cfg, tensors)
    t = toks[:70]
    a = ctx.score(t[:40], 0, targets=next_targets(t)[:40])
    b = ctx.score(t[40:], 40)
    two = np.concatenate([a, b])
    kv_two = _caches(ctx, cfg)
    ids_two = ctx.decode_greedy(int(two["argmax"][-1]), 70, 8)
    ctx.reset_kv()
    one = ctx.score(t, 0)
    assert same_scores(two, one), diff_scores(two, one)
    assert same_scores(one, host_score(want[:70], next_targets(t)))
    kv_one = _caches(ctx, cfg)
    ids_one = ctx.decode_greedy(int(one["argmax"][-1]), 70, 8)
    ctx.reset_kv()
    lg = ctx.forward(t, 0)
    kv_fwd = _caches(ctx, cfg)
    ids_fwd = ctx.decode_greedy(int(np.argmax(lg)), 70, 8)
    for x, y, z in zip(kv_two, kv_one, kv_fwd):
        assert np.array_equal(x, z) and np.array_equal(y, z)
    assert list(ids_two) == list(ids_fwd) and list(ids_one) == list(ids_fwd)
    # a rewind: scoring again from a smaller pos overwrites the rows and gives the same figures
    again = ctx.score(t[40:], 40)
    assert same_scores(again, b)
    ctx.close()


def test_classifier_chunk_edges(gpu):
    """"score_rows" 1, 7 and 64 put chunk edges everywhere (chunks of one row, a ragged last chunk, a full tile); the bits are the default's"""
    cfg, tensors, toks, want = _model("v323-int8")
    ctx = _ctx(gpu, cfg, tensors)
    for n in (17, 130):
        ctx.set_option("score_rows", 0); ctx.reset_kv()
        ref, ref_lg = ctx.score(toks[:n], 0, want_logits=True)
        assert same_scores(ref, host_score(want[:n], next_targets(toks[:n])))
        for rows in (1, 7, 64):
            ctx.set_option("score_rows", rows); ctx.reset_kv()
            assert ctx.query("score_rows") == rows
            got, lg = ctx.score(toks[:n], 0, want_logits=True)
            assert same_scores(got, ref), (n, rows, diff_scores(got, ref))
            assert np.array_equal(bits(lg), bits(ref_lg)), (n, rows)
    ctx.close()


def test_token_by_token_and_staging_fallbacks(gpu):
    """"use_prefill" 0 (every token through the decode kernels) and "score_rows" -1 (the chunks staged one row at a time in the logits vector, as on a context without
    prefill scores) give the oracle's rows too, and the logits vector ends as the last row's, as behind flm_forward"""
    cfg, tensors, toks, want = _model("v323-int8")
    ctx = _ctx(gpu, cfg, tensors)
    exp = host_score(want[:17], next_targets(toks[:17]))
    ctx.set_option("use_prefill", 0)
    got = ctx.score(toks[:17], 0)
    assert same_scores(got, exp), diff_scores(got, exp)
    ctx.set_option("use_prefill", 1); ctx.set_option("score_rows", -1); ctx.reset_kv()
    got, lg = ctx.score(toks[:17], 0, want_logits=True)
    assert np.array_equal(bits(lg), bits(want[:17]))
    assert same_scores(got, exp), diff_scores(got, exp)
    assert np.array_equal(bits(ctx.debug_read("logits", 0, cfg.vocab_size)), bits(want[16]))
    ctx.close()


@pytest.mark.parametrize("qt,opts", [(ff.QT_INT8, {}), (ff.QT_INT8, {"use_mfma": 3}), (ff.QT_INT16, {})], ids=["int8", "int8-128x128", "int16"])
def test_width_and_tile_shapes(gpu, qt, opts):
    """the 2-layer 7B-width model (vocabulary 32000: 500 / 250 classifier tiles per token tile), n = 40: row i == flm_forward(tokens[:i + 1]) on the same context"""
    if ("7B", qt) not in _made:
        cfg = synth.make_config("7B", qt); cfg.n_layers = 2
        _made[("7B", qt)] = (cfg, synth.make_tensors(cfg, seed=53))
    cfg, tensors = _made[("7B", qt)]
    ctx = _ctx(gpu, cfg, tensors)
    for k, v in opts.items():
        ctx.set_option(k, v)
    toks = _tokens(cfg.vocab_size, 40, seed=2)
    got, lg = ctx.score(toks, 0, want_logits=True)
    for k in opts:
        ctx.set_option(k, 1)
    want = np.stack([ctx.forward(toks[:i + 1], 0) for i in range(len(toks))])
    assert np.array_equal(bits(lg), bits(want)), np.nonzero((bits(lg) != bits(want)).any(axis=1))[0][:8]
    exp = host_score(want, next_targets(toks))
    assert same_scores(got, exp), diff_scores(got, exp)
    ctx.close()


KINDS = ("peaked", "medium", "flat", "ties", "clip", "neginf")


def _row_targets(x):
    """the first maximum, a tied maximum's later copy, an entry at exactly d = -15, one just past it (where the row has them; else the last / a middle index), none"""
    x = np.asarray(x, np.float32)
    mx = x.max(); d = x - mx
    out = [int(np.argmax(x)), int(np.nonzero(x == mx)[0][-1])]
    for v, alt in ((np.float32(-15.0), x.size - 1), (np.nextafter(np.float32(-15.0), np.float32(-np.inf)), x.size // 3)):
        hit = np.nonzero(d == v)[0]
        out.append(int(hit[0]) if hit.size else alt)
    return out + [-1]


@pytest.mark.parametrize("n", [2, 320, 323, 32000, 32003])
def test_statistics_kernel_alone(gpu, n):
    """op_score_rows == the host restatement on every logit family, 3 rows each, for every kind of target"""
    for kind in KINDS:
        rows = np.stack([logits_case(kind, n, seed=s) for s in (11, 12, 13)])
        per_row = [_row_targets(r) for r in rows]
        for j in range(5):
            tg = np.array([t[j] for t in per_row], np.int32)
            got, exp = gpu.op_score_rows(rows, tg), host_score(rows, tg)
            assert same_scores(got, exp), (kind, n, j, diff_scores(got, exp))
        if kind == "clip" and n >= 320:
            tg = np.array([t[3] for t in per_row], np.int32)
            got = gpu.op_score_rows(rows, tg)
            assert np.all(got["prob"] == 0.0) and np.all(rows[np.arange(3), tg] - rows.max(axis=1) < -15)      # just past the clip: exactly 0
        if kind == "ties" and n >= 320:
            got = gpu.op_score_rows(rows)
            for r in range(3):
                first = int(np.nonzero(rows[r] == rows[r].max())[0][0])
                assert np.count_nonzero(rows[r] == rows[r].max()) > 1 and got["argmax"][r] == first


def test_statistics_kernel_sum_is_the_sequential_chain(gpu):
    """a row where the order of the sum decides its bits (checked here on the CPU first: the pairwise sum of the same terms is another float)"""
    y = teeth_row(0)
    e = clipped_terms(y)
    seq = np.float32(0)
    for v in e:
        seq = np.float32(seq + v)
    assert tree_sum(e) != seq
    tg = [int(np.argmax(y))]
    got, exp = gpu.op_score_rows(y, tg), host_score(y, tg)
    assert got["sum"][0].view(np.uint32) == seq.view(np.uint32)
    assert same_scores(got, exp), diff_scores(got, exp)


def test_nothing_is_allocated_inside_score(gpu):
    """the first and the second flm_score_tokens of a fresh context (batched, with logits; then the token path), bracketed with hipMemGetInfo: free memory unchanged"""
    hip = ctypes.CDLL("libamdhip64.so")

    def free_bytes():
        f, t = ctypes.c_size_t(0), ctypes.c_size_t(0)
        assert hip.hipMemGetInfo(ctypes.byref(f), ctypes.byref(t)) == 0
        return f.value
    cfg, tensors, toks, want = _model("tiny-int8")
    ctx = _ctx(gpu, cfg, tensors)
    host_score(want[:2], [0, -1])                  # (the host library is loaded before the bracket)
    f0 = free_bytes()
    a, _ = ctx.score(toks[:40], 0, want_logits=True)
    f1 = free_bytes()
    b = ctx.score(toks[:3], 40, targets=[5, -1, 9])
    f2 = free_bytes()
    assert f0 == f1 == f2, (f0, f1, f2)
    assert same_scores(a, host_score(want[:40], next_targets(toks[:40])))
    ctx.close()


def test_invalid_arguments_touch_nothing(gpu):
    cfg, tensors, toks, want = _model("tiny-int8")
    ctx = _ctx(gpu, cfg, tensors)
    ctx.score(toks[:20], 0)
    before = _caches(ctx, cfg)
    V = cfg.vocab_size
    bad_tok = toks[:8].copy(); bad_tok[3] = V
    neg_tok = toks[:8].copy(); neg_tok[0] = -1
    for args in ((np.zeros(0, np.int32), 0, None), (toks[:8], MAX_SEQ - 7, None), (toks[:8], -1, None), (bad_tok, 0, None), (neg_tok, 0, None),
                 (toks[:8], 0, [0, 1, 2, 3, 4, 5, 6, V]), (toks[:8], 0, [0, 1, -2, 3, 4, 5, 6, 7])):
        with pytest.raises(gpu.FlmError, match="flm error -1"):
            ctx.score(args[0], args[1], targets=args[2])
    t = np.ascontiguousarray(toks[:8])
    assert gpu.lib().flm_score_tokens(ctx._h, t.ctypes.data_as(ctypes.c_void_p), 8, 0, None, None, None) == -1       # out == NULL
    for x, y in zip(_caches(ctx, cfg), before):
        assert np.array_equal(x, y)
    fresh = gpu.Ctx(gpu.desc_from_config(cfg, max_seq_len=MAX_SEQ))
    with pytest.raises(gpu.FlmError, match="flm error -5"):
        fresh.score(toks[:8], 0)                                             # the model is not complete
    fresh.close()
    ctx.close()


def test_other_entry_points_undisturbed(gpu):
    """forward, decode_greedy and generate give the same logits and ids before and after a score call on the same context"""
    cfg, tensors, toks, want = _model("tiny-int8")
    ctx = _ctx(gpu, cfg, tensors)

    def run():
        ctx.reset_kv()
        lg = ctx.forward(toks[:12], 0)
        ids = ctx.decode_greedy(int(np.argmax(lg)), 12, 10)
        ctx.reset_kv()
        gen, _ = ctx.generate(toks[:12], 0, 10)
        return bits(lg).copy(), list(ids), list(gen)
    first = run()
    ctx.reset_kv()
    ctx.score(toks[:50], 0)
    ctx.score(toks[:3], 50)
    second = run()
    assert np.array_equal(first[0], second[0]) and first[1:] == second[1:]
    assert np.array_equal(first[0], bits(want[11]))
    ctx.close()
