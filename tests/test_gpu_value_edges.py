"""Value edges on the GPU: the hard but finite inputs of tests/value_edges.py (outliers, saturated and all-zero groups, zero scales, denormals, overflowing sums of
squares, peaked softmaxes, gates beyond expf's range, tied logits) through the op-level kernels, the fused launches, the prefill kernels and the one-launch tail.
Everything is bit equality with the CPU oracle, which tests/test_value_edges_host.py pins to the reference on the same cases (and shows that each family reaches
its edge).  No case is skipped, filtered or tolerated at run time."""
import numpy as np
import pytest

import oracle_py as O
import value_edges as VE
from fast_llama_amd import flmfile as ff
from test_gpu_tp import _run_ranks

pytestmark = pytest.mark.gpu
QTS = [ff.QT_INT8, ff.QT_INT16]
QT_IDS = ["int8", "int16"]
OPTION_SETS = ({}, {"fuse_token": 0}, {"fuse_layer": 0}, {"fuse_back": 0}, {"fuse_attn_o": 0, "fuse_ffn": 0}, {"fuse_qkv": 2}, {"use_graph": 0})
OPT_IDS = ["default", "fuse_token0", "fuse_layer0", "fuse_back0", "attn_o0-ffn0", "fuse_qkv2", "use_graph0"]
CASES = {c[0]: c for c in VE.model_cases()}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same(a, b):
    return np.array_equal(bits(a), bits(b))


# ---- op level ---------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("qt", QTS, ids=QT_IDS)
def test_quantize(gpu, qt):
    """sizes 256 and 4096: groups x1e-36, denormal, all zero, x1e33, constant, wide range, plain and with an outlier at the last lane, shifted so that the edge groups
    fall on different waves"""
    for name, x in VE.quantize_cases():
        q, s = gpu.op_quantize(x, qt)
        qo, so = O.quantize(x, qt)
        assert np.array_equal(q, qo), (name, np.flatnonzero(q != qo)[:8])
        assert same(s, so), (name, np.flatnonzero(bits(s) != bits(so))[:8])


def test_rmsnorm(gpu):
    """n in {64, 256, 4096, 4096 + 64}: zeros, tiny, denormal, huge, overflowing and outlier x against norm weights holding 0, -1.5, 40 and 1e-6"""
    for name, x, w in VE.rmsnorm_cases():
        assert same(gpu.op_rmsnorm(x, w), O.rmsnorm(x, w)), name


@pytest.mark.parametrize("qt", QTS, ids=QT_IDS)
@pytest.mark.parametrize("w", [1, 3])
def test_matmul_gemv(gpu, qt, w):
    for regime in VE.matmul_regimes():
        W, sW, X, sX = VE.matmul_case(qt, 96, 256, w, regime)
        got, want = gpu.op_matmul_q(qt, W, sW, X, sX), O.matmul_q(qt, W, sW, X, sX)
        assert same(got, want), (regime, np.argwhere(bits(got) != bits(want))[:4])


@pytest.mark.parametrize("qt", QTS, ids=QT_IDS)
@pytest.mark.parametrize("m,n,w", [(80, 192, 16), (130, 256, 17), (70, 128, 65)])
def test_matmul_tiles(gpu, qt, m, n, w, monkeypatch):
    """the prefill GEMMs (tile shape by size / 64 x 64 / 128 x 128) and a GEMV per row on saturated, zero and zero-scale rows in W and in X, in every scale regime"""
    for regime in VE.matmul_regimes():
        W, sW, X, sX = VE.matmul_case(qt, m, n, w, regime)
        want = O.matmul_q(qt, W, sW, X, sX)
        for variant in ("1", "2", "3", "gemv"):
            monkeypatch.setenv("FLM_OP_GEMM", variant)
            got = gpu.op_matmul_q(qt, W, sW, X, sX)
            assert same(got, want), (regime, variant, np.argwhere(bits(got) != bits(want))[:4])


@pytest.mark.parametrize("w", [1, 5, 16])
def test_matmul_skinny(gpu, w):
    for regime in VE.matmul_regimes():
        for m, n in ((96, 256), (80, 192)):
            W, sW, X, sX = VE.matmul_case(ff.QT_INT8, m, n, w, regime)
            got, want = gpu.op_matmul_skinny(W, sW, X, sX), O.matmul_q(ff.QT_INT8, W, sW, X, sX)
            assert same(got, want), (regime, m, n, np.argwhere(bits(got) != bits(want))[:4])


def test_swiglu(gpu):
    """the a x b grid (gates at +-0, +-30, around expf's overflow and underflow, +-1e30, +-1e-40, +-3e38) and the grid scattered into Gaussian vectors"""
    for name, a, b in VE.swiglu_cases():
        got, want = gpu.op_swiglu(a, b), O.swiglu(a, b)
        bad = np.flatnonzero(bits(got) != bits(want))
        assert bad.size == 0, (name, a[bad[:4]], b[bad[:4]], got[bad[:4]], want[bad[:4]])


def test_softmax(gpu):
    for name, x, cols in VE.softmax_cases():
        assert same(gpu.op_softmax(x, cols)[:cols], O.softmax(x, cols)[:cols]), name


@pytest.mark.parametrize("parts", [0, 2, 4])
@pytest.mark.parametrize("hs,heads", [(64, 2), (128, 2), (32, 3)])
def test_attention_decode(gpu, hs, heads, parts, monkeypatch):
    """un-split and split decode attention at positions 0, 1, 63, 64, 65 and 257: a peaked softmax at EVERY position, all-zero K rows (uniform weights), V x1e30,
    V x1e-41 (denormal), q and k x1e-20"""
    if parts:
        monkeypatch.setenv("FLM_OP_ATTN_PARTS", str(parts))
    max_seq = 1024
    last = max(VE.ATTN_POSITIONS)
    for fam in VE.ATTN_FAMILIES:
        q, k, v = VE.attention_inputs(fam, heads, hs, last + 1)
        kc = np.zeros((heads, max_seq, hs), np.float32); vc = np.zeros_like(kc)
        pos = 0
        for target in VE.ATTN_POSITIONS:
            if target > pos:                                    # rows pos .. target - 1 enter the cache through the oracle's batched path
                for h in range(heads):
                    O.attention_head(kc[h], vc[h], q[pos:target, h], k[pos:target, h], v[pos:target, h], pos)
                pos = target
            kg = kc.copy(); vg = vc.copy()
            want = np.stack([O.attention_head(kc[h], vc[h], q[pos:pos + 1, h], k[pos:pos + 1, h], v[pos:pos + 1, h], pos)[0] for h in range(heads)])
            got = gpu.op_attention(kg, vg, q[pos].reshape(-1), k[pos].reshape(-1), v[pos].reshape(-1), heads, hs, max_seq, pos).reshape(heads, hs)
            assert same(kg[:, pos], kc[:, pos]) and same(vg[:, pos], vc[:, pos]), (fam, pos)
            assert same(got, want), (fam, pos)
            pos += 1


# ---- model level ------------------------------------------------------------------------------------------------------------------------------------------------------
def _ctx(gpu, cfg, tensors, opts=(), **kw):
    ctx = gpu.Ctx(gpu.desc_from_config(cfg, **kw)); ctx.upload_all(tensors)
    for k, v in dict(opts).items():
        ctx.set_option(k, v)
    return ctx


def _check(ctx, sch, want, what):
    ctx.reset_kv()
    for i, (t, pos) in enumerate(sch):
        got = ctx.forward(t, pos)
        assert same(got, want[i]), (what, i, int((bits(got) != bits(want[i])).sum()))


def _run_case(gpu, case, opts):
    name, shape, qt, fam, layers = case
    cfg, tensors = VE.edge_model(shape, qt, fam, layers)
    want = VE.case_logits(case)
    ctx = _ctx(gpu, cfg, tensors, opts)
    for prefill in (1, 0):
        ctx.set_option("use_prefill", prefill)
        for sname, sch in VE.case_schedules(name, cfg):
            if prefill or not sname.startswith("decode"):       # (short and long prompts under use_prefill 1 and 0; the decode schedules once)
                _check(ctx, sch, want[sname], (name, opts, prefill, sname))
    assert ctx.query("fallback") == 0
    ctx.close()


@pytest.mark.parametrize("opts", OPTION_SETS, ids=OPT_IDS)
@pytest.mark.parametrize("name", ["tiny-int8-all", "tiny-int16-all", "tiny128-int8-all", "tiny128-int16-all"])
def test_all_families_at_once(gpu, name, opts):
    """every edge row through the short prompt (batched, then fed again at a decode position), the ragged long prompts (edge tokens first, in the middle, last and
    straddling a tile edge) batched and token by token, and decode steps that feed edge tokens at positions 63, 64 and 65: every logit of every call"""
    _run_case(gpu, CASES[name], opts)


@pytest.mark.parametrize("family", [f[0] for f in VE.SINGLE] + ["all"])
def test_one_family_at_a_time(gpu, family):
    """`small` int8 with one family of weight edits (a failure names its family), every option set"""
    for opts in OPTION_SETS:
        _run_case(gpu, CASES[f"small-int8-{family}"], opts)


def _oracle_greedy(om, first, pos, n):
    ids, cur = [], first
    for _ in range(n):
        cur = int(np.argmax(om.forward(np.array([cur], np.int32), pos))); ids.append(cur); pos += 1
    return ids


@pytest.mark.parametrize("name", ["tiny-int8-all", "tiny-int8-equal", "small-int8-all"])
def test_device_greedy_loop_on_tied_logits(gpu, name):
    """decode_greedy for 12 tokens from an edge token: with the mirrored / duplicated classifier every top logit occurs twice, in two workgroups of the one-launch
    tail; with all rows equal every workgroup holds a tie.  The ids are the oracle's stepwise argmax (the first maximum); from the row whose sum of squares overflows
    the first id is 0 (every logit is +-0), with all rows equal every id is 0."""
    case = CASES[name]
    cfg, tensors = VE.edge_model(*case[1:])
    ctx = _ctx(gpu, cfg, tensors)
    prompt = np.array([1, 50], np.int32)
    for first in (VE.edge_id("outliers"), VE.OVERFLOW_ID, VE.edge_id("wide range")):
        om = O.OracleModel(cfg, tensors)
        om.forward(prompt, 0)
        want = _oracle_greedy(om, first, 2, 12)
        ctx.reset_kv(); ctx.forward(prompt, 0)
        got = [int(x) for x in ctx.decode_greedy(first, 2, 12)]
        assert got == want, (name, first)
        if first == VE.OVERFLOW_ID:
            assert got[0] == 0
        if name.endswith("-equal"):
            assert got == [0] * 12
    assert ctx.query("fallback") == 0
    ctx.close()


def test_split_heads_with_edge_tokens_at_the_end_of_a_long_prompt(gpu):
    """`small` at attn_split 2: a 300-token prompt whose last 10 tokens are edge rows, then 3 decode steps (two of them edge rows)"""
    case = CASES["small-int8-all"]
    cfg, tensors = VE.edge_model(*case[1:])
    sch = VE.split_prompt(cfg)
    want = VE.run_schedule(O.OracleModel(cfg, tensors), sch)
    assert all(np.isfinite(l).all() for l in want)
    for split in (2, 1):
        ctx = _ctx(gpu, cfg, tensors, {"attn_split": split})
        _check(ctx, sch, want, ("attn_split", split))
        assert ctx.query("fallback") == 0
        ctx.close()


def test_score_of_the_ragged_prompt(gpu):
    """flm_score_tokens over the ragged long prompts: every row's logits and argmax are the oracle's token-by-token rows"""
    for name in ("tiny-int8-all", "tiny128-int16-all"):
        case = CASES[name]
        cfg, tensors = VE.edge_model(*case[1:])
        ctx = _ctx(gpu, cfg, tensors)
        for v in (0, 1):
            p = VE.long_prompt(cfg, v)
            om = O.OracleModel(cfg, tensors)
            want = np.stack([om.forward(p[i:i + 1], i) for i in range(len(p))])
            ctx.reset_kv()
            got, lg = ctx.score(p, 0, want_logits=True)
            assert np.array_equal(bits(lg), bits(want)), (name, v, np.flatnonzero((bits(lg) != bits(want)).any(axis=1))[:8])
            assert np.array_equal(got["argmax"], np.argmax(want, axis=1)), (name, v)
        assert ctx.query("fallback") == 0
        ctx.close()


@pytest.mark.parametrize("name", ["tiny-int8-all", "small-int8-all"])
def test_verify_greedy_accepts_the_oracles_ids(gpu, name):
    """flm_verify_greedy with 7 drafts = the oracle's greedy ids behind an edge token: the skinny GEMM (and the tiles) on a batch whose first row is an edge row, all
    eight ids delivered"""
    case = CASES[name]
    cfg, tensors = VE.edge_model(*case[1:])
    prompt = np.array([1, 50, VE.edge_id("zero group"), 77], np.int32)
    ctx = _ctx(gpu, cfg, tensors, max_seq_len=256)
    for first in (VE.edge_id("outliers"), VE.edge_id("x1e-41 denormal"), VE.edge_id("outlier at a group's last lane")):
        om = O.OracleModel(cfg, tensors)
        om.forward(prompt, 0)
        want = _oracle_greedy(om, first, len(prompt), 8)
        for gemm in (1, 0):
            ctx.set_option("spec_gemm", gemm)
            ctx.reset_kv(); ctx.forward(prompt, 0)
            got = ctx.verify_greedy(first, np.array(want[:7], np.int32), len(prompt))
            assert [int(x) for x in got] == want, (name, first, gemm)
    assert ctx.query("fallback") == 0
    ctx.close()


@pytest.mark.parametrize("name,opts", [("7B-int8-all", {}), ("7B-int8-all", {"fuse_token": 0}), ("7B-int8-all", {"fuse_qkv": 2}), ("7B-int16-all", {})],
                         ids=["int8-default", "int8-fuse_token0", "int8-fuse_qkv2", "int16-default"])
def test_production_geometry(gpu, name, opts):
    """one 7B-width layer and the 32000-row classifier with all families: the short prompt and 3 decode steps (the production pass geometry and LDS layouts)"""
    case = CASES[name]
    cfg, tensors = VE.edge_model(*case[1:])
    (sname, sch), = VE.case_schedules(name, cfg)
    want = VE.case_logits(case)[sname]
    ctx = _ctx(gpu, cfg, tensors, opts)
    _check(ctx, sch, want, (name, opts))
    assert ctx.query("fallback") == 0
    ctx.close()


@pytest.mark.parametrize("structure", ["default", "per-layer"])
def test_tensor_parallel_rehearsal_on_one_device(gpu, structure):
    """world 2 on one device (CU-masked ranks), `small` int8, all families: the short prompt and 2 decode steps on every rank, with the rank-spanning launch and with
    the per-layer launches (tp_fuse_layers 0)"""
    case = CASES["small-int8-all"]
    cfg, tensors = VE.edge_model(*case[1:])
    world = 2
    ctxs = [gpu.Ctx(gpu.desc_from_config(cfg), device=0, rank=r, world=world, comm_id=None) for r in range(world)]
    for c in ctxs:
        c.upload_all(tensors)
        c.set_option("cu_parts", world)
        if structure == "per-layer":
            c.set_option("tp_fuse_layers", 0)
    gpu.Ctx.regroup(ctxs)
    for c in ctxs:
        assert c.query("grp_tp_fuse_layers") == (1 if structure == "default" else 0)
    for edge in ("outliers", "x1e-41 denormal", "x1e20 sum of squares overflows"):
        sch = VE.short_schedule(VE.edge_id(edge))[:3]
        want = VE.case_logits(case).get(f"short {edge}") or VE.run_schedule(O.OracleModel(cfg, tensors), sch)
        for c in ctxs:
            c.reset_kv()
        for r, got in enumerate(_run_ranks(ctxs, lambda c: [c.forward(t, pos) for t, pos in sch])):
            for i, l in enumerate(got):
                assert same(l, want[i]), (structure, edge, r, i)
    for c in ctxs:
        c.close()
