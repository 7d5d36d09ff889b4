"""Tree draft-and-verify (include/flm_gpu.h: flm_verify_tree_greedy, flm_op_attention_tree; kernels: csrc/flm_tree.h).  Everything is equality on bit patterns.
Op level: k_rope_kv_tree + k_attn_tree against oracle_py.attention_head run on every row's OWN path (the cache rows [0, pos), then the path's rows).  Cache rows at and
behind pos + n hold NaN, and every case runs a second time with NaN in the k / v of two leaves: no other row may change.
Model level (tests/head_sizes.py's 2-layer models, max_seq_len 256): ids and K/V rows against the token loop, per-node logits against OracleModel.forward on the node's path."""
import numpy as np
import pytest

import head_sizes as HS
import oracle_py as O
from fast_llama_amd import flmfile as ff
from test_gpu_spec import MAX_SEQ, _caches, _ctx, bits

pytestmark = pytest.mark.gpu
HEADS = 2
RAGGED = [-1, 0, 0, 1, 1, 2, 3, 3, 4, 5, 6, 8, 8, 9, 11, 10]       # depths 0 1 1 2 2 2 3 3 | 3 3 4 4 4 4 5 5: both groups of 8 queries mix depths
TREES = {"chain": [-1] + list(range(15)), "star": [-1] + [0] * 15, "ragged": RAGGED}
POISON = {"chain": [15], "star": [3, 15], "ragged": [2, 7]}        # rows whose k / v are NaN in the second run: leaves, and (ragged) the inner node 2, whose subtree (5, 9, 13) is lost with it


def _paths(parent):
    out = []
    for i, p in enumerate(parent):
        out.append(out[p] + [i] if p >= 0 else [i])
    return out


def _op_case(hs, pos, n, seed, q_scale={}):
    rng = np.random.default_rng([seed, hs, pos])
    kc = np.full((HEADS, pos + n + 3, hs), np.nan, np.float32); vc = np.full_like(kc, np.nan)
    kc[:, :pos] = rng.standard_normal((HEADS, pos, hs)); vc[:, :pos] = rng.standard_normal((HEADS, pos, hs))
    q, k, v = ((rng.standard_normal((n, HEADS * hs)) * s).astype(np.float32) for s in (2, 1, 1))
    for row, s in q_scale.items():
        q[row] *= np.float32(s)
    return kc, vc, q, k, v


def _check_op(gpu, hs, pos, name, case):
    """per node and head the oracle on the node's own contiguous cache -> its output and the K / V row it appends; then the op, clean and with poisoned leaves"""
    parent, (kc0, vc0, q, k, v) = TREES[name], case
    n, max_seq, want = len(parent), kc0.shape[1], []
    for path in _paths(parent):
        o, kr, vr = [], [], []
        for h in range(HEADS):
            ck = np.zeros((pos + len(path), hs), np.float32); cv = np.zeros_like(ck)
            ck[:pos] = kc0[h, :pos]; cv[:pos] = vc0[h, :pos]; sl = slice(h * hs, (h + 1) * hs)
            o.append(O.attention_head(ck, cv, q[path][:, sl], k[path][:, sl], v[path][:, sl], pos)[-1]); kr.append(ck[-1]); vr.append(cv[-1])
        want.append((np.concatenate(o), np.stack(kr), np.stack(vr)))
    for poison in ([], POISON[name]):
        kc, vc, kk, vv = kc0.copy(), vc0.copy(), k.copy(), v.copy()
        kk[poison] = np.nan; vv[poison] = np.nan
        poison = [i for i, p in enumerate(_paths(parent)) if set(p) & set(poison)]       # (a poisoned node's descendants see it)
        out = gpu.op_attention_tree(kc, vc, q, kk, vv, HEADS, hs, max_seq, pos, parent)
        for i in set(range(n)) - set(poison):
            assert np.array_equal(bits(out[i]), bits(want[i][0])), (name, hs, pos, i, poison)
            assert np.array_equal(bits(kc[:, pos + i]), bits(want[i][1])) and np.array_equal(bits(vc[:, pos + i]), bits(want[i][2])), ("the node's K/V row", i)
        rest = np.r_[0:pos, pos + n:max_seq]
        assert np.array_equal(bits(kc[:, rest]), bits(kc0[:, rest])) and np.array_equal(bits(vc[:, rest]), bits(vc0[:, rest])), "a row outside the tree was written"


@pytest.mark.parametrize("name", list(TREES))
@pytest.mark.parametrize("hs", [32, 40, 64, 128])
def test_attention_tree_is_the_oracle_on_every_path(gpu, hs, name):
    """pos = 0 (no cache row: the root is logical row 0), one partial tile, 63 / 64 / 65 around the tile edge, 130 (two tiles and two rows)"""
    for pos in (0, 1, 63, 64, 65, 130):
        _check_op(gpu, hs, pos, name, _op_case(hs, pos, 16, 11))


@pytest.mark.parametrize("hs", [40, 64])
def test_attention_tree_peaked_neighbours(gpu, hs):
    """query 5 is peaked -- weights under the 1e-15 skip threshold next to weights that count (NumPy first) --, query 4 of the same group skips nothing.  hs = 40: fewer
    dimensions than rows in a tile, the lanes that own no dimension look at the weights too"""
    pos = 130
    case = _op_case(hs, pos, 16, 12, q_scale={5: 40.0, 4: 0.05})
    (kc, _, q, k, _), paths = case, _paths(RAGGED)
    for h in range(HEADS):
        sl = slice(h * hs, (h + 1) * hs)
        w = {i: HS.softmax_weights(np.concatenate([kc[h, :pos], np.stack([O.rope(k[a, sl], pos + d) for d, a in enumerate(paths[i][:-1])])]),
                                   q[i, sl], k[i, sl], hs, pos + len(paths[i]) - 1) for i in (4, 5)}
        assert HS.is_peaked(w[5]) and (w[4] > 1e-12).all(), "the case does not separate the two queries"
    _check_op(gpu, hs, pos, "ragged", case)


PARENT = [-1, 0, 0, 1, 2, 2, 4, 5, 5, 7, 8, 8]                       # depths 0 1 1 2 2 2 3 3 3 4 4 4
DEPTH = [len(p) - 1 for p in _paths(PARENT)]
# case -> the nodes that hold the token loop's id of their depth (every other node holds that id + 1), and the path that must come back
CASES = {"none": ([], [0]), "in-place": ([1], [0, 1]),
         "leaf": ([1, 3], [0, 1, 3]),                                # a root-to-leaf path; node 3 moves to row pos + 2
         "siblings": ([2, 5, 8, 10, 11], [0, 2, 5, 8, 10])}          # non-first siblings down to a leaf (k_tree_keep moves every row); 10 and 11 hold the same id
MODELS = [(64, ff.QT_INT8), (40, ff.QT_INT8), (40, ff.QT_INT16)]


def _tokens(cfg, first, ids, right):
    return np.array([first] + [(int(ids[DEPTH[i] - 1]) + (i not in right)) % cfg.vocab_size for i in range(1, len(PARENT))], np.int32)


@pytest.mark.parametrize("model", MODELS, ids=[HS.case_id(m) for m in MODELS])
def test_verify_tree_is_the_decode_loop(gpu, model):
    """Against the token loop on a second context, behind prompts of 37 and 60 tokens (the tree straddles row 64): ids, count and path; the K/V rows [0, pos + count) of
    every layer; the decode loop's continuation; "spec_gemm" 1 and 0.  Then every node's row of logits against OracleModel.forward fed the node's path: with "score_rows"
    -1 the classifier stages one row at a time in the logits vector, where the LAST row stays, and node i is the last row of the tree cut behind it (a prefix of a parent
    array is a tree; a node's row does not depend on the nodes behind it).  The host walk over the oracle's maxima is the delivered path"""
    cfg, tensors = HS.model(*model)
    ctx, ref = _ctx(gpu, cfg, tensors), _ctx(gpu, cfg, tensors)
    try:
        for pos, cases in ((60, ["siblings"]), (37, list(CASES))):
            prompt = HS.tokens(pos, salt=pos)
            ref.reset_kv(); first = ref.forward_argmax(prompt, 0)
            ids, kv_ref = ref.decode_greedy(first, pos, 8), _caches(ref, cfg)
            for case, gemm in [(c, g) for c in cases for g in (1, 0)]:
                right, path = CASES[case]
                ctx.set_option("spec_gemm", gemm); ctx.reset_kv()
                assert ctx.forward_argmax(prompt, 0) == first
                got, got_path = ctx.verify_tree(pos, _tokens(cfg, first, ids, right), PARENT)
                assert list(got_path) == path and np.array_equal(got, ids[:len(path)]), (case, pos, gemm, list(got), list(got_path), list(ids))
                for a, b in zip(_caches(ctx, cfg), kv_ref):
                    assert np.array_equal(a[:, :pos + len(path)], b[:, :pos + len(path)]), (case, pos, gemm)
                assert np.array_equal(ctx.decode_greedy(int(got[-1]), pos + len(path), 2), ids[len(path):len(path) + 2]), (case, pos, gemm)
        pos, prompt = 37, HS.tokens(37, salt=37)
        ref.reset_kv(); first = ref.forward_argmax(prompt, 0)
        toks = _tokens(cfg, first, ref.decode_greedy(first, pos, 8), CASES["siblings"][0])
        om = O.OracleModel(cfg, tensors, max_seq=MAX_SEQ)
        om.forward(prompt, 0)
        ctx.reset_kv(); ctx.forward_argmax(prompt, 0); ctx.set_option("score_rows", -1)
        a = [int(np.argmax(om.forward(toks[:1], pos)))]
        for i, p in enumerate(_paths(PARENT)[1:], 1):
            got, got_path = ctx.verify_tree(pos, toks[:i + 1], PARENT[:i + 1])
            want = om.forward(toks[p], pos)
            assert np.array_equal(bits(ctx.debug_read("logits", 0, cfg.vocab_size)), bits(want)), (model, i)
            a.append(int(np.argmax(want)))
        assert list(got_path) == list(gpu.tree_walk(toks, PARENT, a)) == CASES["siblings"][1] and list(got) == [a[i] for i in got_path]
        assert ctx.query("fallback") == 0
    finally:
        ctx.close(); ref.close()


def test_refusals_leave_the_cache_alone(gpu):
    """bad input (-1) and a head size the kernel refuses (-2), through the model-level call: the error, and a cache that is bit-identical"""
    for hs, code, calls in ((64, -1, [([1, 2, 3], [-1, 2, 1], 37), ([1, 2, 3], [-1, -1, 0], 37), ([1], [-1], 37), ([1] * 12, PARENT, MAX_SEQ - 11), ([1, 2, HS.VOCAB], [-1, 0, 0], 37)]),
                            (256, -2, [([1, 2, 3], [-1, 0, 0], 37)])):
        cfg, tensors = HS.model(hs, ff.QT_INT8)
        ctx = _ctx(gpu, cfg, tensors)
        try:
            ctx.forward_argmax(HS.tokens(37), 0)
            before = _caches(ctx, cfg)
            for toks, par, pos in calls:
                with pytest.raises(gpu.FlmError, match=f"flm error {code}"):
                    ctx.verify_tree(pos, toks, par)
            assert all(np.array_equal(a, b) for a, b in zip(_caches(ctx, cfg), before))
        finally:
            ctx.close()


@pytest.mark.parametrize("B", [2, 4])
def test_lookup_loop_with_branches_is_generate(gpu, B):
    """a repetitive prompt whose suffix 7 8 9 occurs four times with four different continuations: the ids and the final K/V rows of generate at temperature 0, in no
    more passes than the chain drafter needs ("spec_steps")"""
    cfg, tensors = HS.model(64, ff.QT_INT8)
    prompt, N = np.array([1, 7, 8, 9, 20, 7, 8, 9, 30, 7, 8, 9, 40, 7, 8, 9, 50, 21, 7, 8, 9], np.int32), 40
    ctx, ref = _ctx(gpu, cfg, tensors), _ctx(gpu, cfg, tensors)
    try:
        want = ref.generate(prompt, 0, N)[0]
        steps = {}
        for b in (1, B):
            ctx.set_option("spec_branches", b); ctx.reset_kv()
            assert np.array_equal(ctx.generate_lookup(prompt, 0, N, draft_len=7, ngram_max=3), want), b
            steps[b] = ctx.query("spec_steps")
            for x, y in zip(_caches(ctx, cfg), _caches(ref, cfg)):
                assert np.array_equal(x[:, :len(prompt) + N - 1], y[:, :len(prompt) + N - 1]), b
        assert 0 < steps[B] <= steps[1] and ctx.query("spec_branches") == B and ctx.query("fallback") == 0, steps
    finally:
        ctx.close(); ref.close()
