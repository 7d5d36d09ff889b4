"""The value-edge builders (tests/value_edges.py) proven on the CPU before any of it goes near a GPU:
  * the oracle equals the reference library bit for bit on every op case and every model case (skipped where oracle/_ref/libflref.so is absent; the committed
    tests/golden/value_edges.npz, recorded from the reference, keeps the pin there);
  * every model case's logits are finite, every op case's output is NaN-free -- nothing is skipped, filtered or tolerated at run time;
  * each family bites: the edge it is named for is reached, re-derived with the oracle's op functions (value_edges.layer0_trace)."""
import hashlib
import os

import numpy as np
import pytest

import oracle_py as O
import value_edges as VE
from fast_llama_amd import flmfile as ff, synth

needs_ref = pytest.mark.skipif(not O.have_ref(), reason="oracle/_ref/libflref.so not built (needs /root/reference)")
GOLD = os.path.join(os.path.dirname(__file__), "golden", "value_edges.npz")
QTS = (ff.QT_INT8, ff.QT_INT16)
DENORM = np.float32(2.0 ** -126)
CASES = VE.model_cases()
case_logits = VE.case_logits


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---- oracle == reference ----------------------------------------------------------------------------------------------------------------------------------------------
@needs_ref
def test_ops_oracle_equals_reference():
    R = O.ref()
    for name, x in VE.quantize_cases():
        for qt in QTS:
            q, s = O.quantize(x, qt); q2, s2 = O.quantize(x, qt, lib=R)
            assert np.array_equal(q, q2) and np.array_equal(bits(s), bits(s2)), name
    for name, x, w in VE.rmsnorm_cases():
        o = O.rmsnorm(x, w)
        assert np.array_equal(bits(o), bits(O.rmsnorm(x, w, lib=R))), name
        for qt in QTS:                                                   # ... and `quantize` behind it
            q, s = O.quantize(o, qt); q2, s2 = O.quantize(o, qt, lib=R)
            assert np.array_equal(q, q2) and np.array_equal(bits(s), bits(s2)), name
    for name, a, b in VE.swiglu_cases():
        assert np.array_equal(bits(O.swiglu(a, b)), bits(O.swiglu(a, b, lib=R))), name
    for name, x, c in VE.softmax_cases():
        assert np.array_equal(bits(O.softmax(x, c)[:c]), bits(O.softmax(x, c, lib=R)[:c])), name
    for qt, m, n, w, reg in VE.op_cases()["matmul_q"]:
        W, sW, X, sX = VE.matmul_case(qt, m, n, w, reg)
        assert np.array_equal(bits(O.matmul_q(qt, W, sW, X, sX)), bits(O.matmul_q(qt, W, sW, X, sX, lib=R))), (qt, m, n, w, reg)


@needs_ref
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_model_oracle_equals_reference(tmp_path, case):
    name, shape, qt, fam, layers = case
    cfg, tensors = VE.edge_model(shape, qt, fam, layers)
    path = tmp_path / "m.flm"
    synth.write_synthetic_flm(str(path), cfg, tensors=tensors)
    rm = O.RefModel(path, qt, threads=2, max_batch=512)
    want = case_logits(case)
    for sname, sch in VE.case_schedules(name, cfg):
        for i, (t, pos) in enumerate(sch):
            assert np.array_equal(bits(rm.forward(t, pos)), bits(want[sname][i])), (sname, i)


# ---- finite -----------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_model_inputs_and_logits_are_finite(case):
    for sname, lgs in case_logits(case).items():                   # (the inputs: weight_edits asserts that every tensor it returns is finite)
        for i, l in enumerate(lgs):
            assert np.isfinite(l).all(), (sname, i)


def test_batched_prompt_equals_token_by_token():
    for case in CASES[:4]:
        name, shape, qt, fam, layers = case
        cfg, tensors = VE.edge_model(shape, qt, fam, layers)
        om = O.OracleModel(cfg, tensors)
        for v in (0, 1):
            p = VE.long_prompt(cfg, v)
            for i, t in enumerate(p):
                last = om.forward(np.array([t], np.int32), i)
            assert np.array_equal(bits(last), bits(case_logits(case)[f"long {v}"][0])), (name, v)
            om.reset()


def test_op_inputs_are_finite_and_outputs_nan_free():
    for name, x in VE.quantize_cases():
        assert np.isfinite(x).all()
        for qt in QTS:
            assert not np.isnan(O.quantize(x, qt)[1]).any(), name
    for name, x, w in VE.rmsnorm_cases():
        assert np.isfinite(x).all() and np.isfinite(w).all()
        assert not np.isnan(O.rmsnorm(x, w)).any(), name
    for name, a, b in VE.swiglu_cases():
        assert np.isfinite(a).all() and np.isfinite(b).all()
        assert not np.isnan(O.swiglu(a, b)).any(), name
    for name, x, c in VE.softmax_cases():
        assert np.isfinite(x).all()
        assert not np.isnan(O.softmax(x, c)[:c]).any(), name
    for qt, m, n, w, reg in VE.op_cases()["matmul_q"]:
        W, sW, X, sX = VE.matmul_case(qt, m, n, w, reg)
        assert np.isfinite(sW).all() and np.isfinite(sX).all()
        assert not np.isnan(O.matmul_q(qt, W, sW, X, sX)).any(), (qt, m, n, w, reg)
    for fam in VE.ATTN_FAMILIES:
        for hs in (64, 128, 32):
            q, k, v = VE.attention_inputs(fam, 2, hs, 258)
            assert np.isfinite(q).all() and np.isfinite(k).all() and np.isfinite(v).all()
            kc = np.zeros((1024, hs), np.float32); vc = np.zeros_like(kc)
            out = O.attention_head(kc, vc, q[:, 0], k[:, 0], v[:, 0], 0)
            assert not np.isnan(out).any(), (fam, hs)


# ---- each family bites ------------------------------------------------------------------------------------------------------------------------------------------------
ALL_SMALL = [c for c in CASES if c[0].endswith("-all") and c[1] != "7B"]


def _trace(case, edge_name, prefix=(1, 50)):
    name, shape, qt, fam, layers = case
    cfg, tensors = VE.edge_model(shape, qt, fam, layers)
    return cfg, tensors, VE.layer0_trace(cfg, tensors, list(prefix) + [77, 23, VE.edge_id(edge_name)])


@pytest.mark.parametrize("case", ALL_SMALL, ids=[c[0] for c in ALL_SMALL])
def test_bites_peaked_softmax(case):
    """family "peaked": in one softmax row of an even head, a weight under the 1e-15 skip threshold next to one at or above it"""
    for edge in ("outliers", "wide range", "constant +-0.75"):
        cfg, _, tr = _trace(case, edge)
        assert any((w < 1e-15).any() and (w >= 1e-15).any() for w in tr["weights"][0::2]), edge


@pytest.mark.parametrize("case", ALL_SMALL, ids=[c[0] for c in ALL_SMALL])
def test_bites_big_gate(case):
    """family "big_gate": gate values under -88.73 (expf(-a) is +inf) and over 88.73"""
    for edge in ("outliers", "zero row", "x1e-20", "one-hot", "outlier at a group's last lane"):
        _, _, tr = _trace(case, edge)
        assert (tr["gate"] < -88.73).any() and (tr["gate"] > 88.73).any(), edge


@pytest.mark.parametrize("case", ALL_SMALL, ids=[c[0] for c in ALL_SMALL])
def test_bites_denormals(case):
    """a nonzero |value| under 2^-126: among the quantizer's scales (the denormal row), the matmul's outputs (family "wv_tiny") and the products of QK^T (family
    "qk_tiny" with the "tiny q.k" row)"""
    den = lambda a: ((a != 0) & (np.abs(a) < DENORM)).any()      # noqa: E731
    cfg, _, tr = _trace(case, "x1e-41 denormal")
    assert den(tr["sx"]) and den(tr["x2"])
    hs = cfg.dim // cfg.n_heads
    assert den(tr["v"][:, hs:hs + 64])
    cfg, _, tr = _trace(case, "tiny q.k", prefix=(VE.edge_id("tiny q.k"), VE.edge_id("x1e-20")))
    assert den(tr["products"][cfg.n_heads - 1])
    for v in (0, 1):                                               # ... and in the long prompts, where the batched QK^T computes them
        p = [int(t) for t in VE.long_prompt(cfg, v)]
        at = p.index(VE.edge_id("tiny q.k"))
        assert VE.edge_id("x1e-20") in p[:at]
        assert den(VE.layer0_trace(cfg, VE.edge_model(*case[1:])[1], p[:at + 1])["products"][cfg.n_heads - 1])


@pytest.mark.parametrize("case", ALL_SMALL, ids=[c[0] for c in ALL_SMALL])
def test_bites_mixed_wave(case):
    """within one run of 256 consecutive activation elements (four group scales) one scale is zero or outside [2^-100, 2^100] and one is inside: the wave-wide
    fast / slow choice of the quantizer is taken on a wave that holds both"""
    def mixed(s):
        s = np.abs(s[:len(s) // 4 * 4].reshape(-1, 4))
        inside = (s >= 2.0 ** -100) & (s <= 2.0 ** 100)
        return (inside.any(axis=1) & (~inside).any(axis=1)).any()
    _, _, tr = _trace(case, "zero group")
    assert mixed(tr["sx"])
    _, _, tr = _trace(case, "outliers")
    assert mixed(tr["sa"])                     # the heads' output: head 1's first group is denormal (family "wv_tiny") next to plain heads


@pytest.mark.parametrize("case", ALL_SMALL, ids=[c[0] for c in ALL_SMALL])
def test_bites_weight_rows(case):
    """families "saturated", "zero", "out_huge" and "norm": the rows do what they are named for in layer 0's QKV and Wo outputs"""
    cfg, tensors, tr = _trace(case, "outliers")
    q = tr["q"]
    Wq = tensors[(ff.T_ATTN_Q, 0)][0]; lim = VE.F[cfg.quant_type]
    assert (Wq[3] == lim).all() and (Wq[4] == -lim).all() and (np.abs(Wq[5]) == lim).all() and (Wq[6, 64:128] == lim).all() and q[3] != 0 and q[4] != 0
    assert q[8] == 0 and tr["k"][-1][8] == 0 and q[10] == 0             # all scales zero / all weights zero
    big = np.abs(tr["wo"][[7, 130, cfg.dim - 64, cfg.dim - 1]])
    assert (big > 1e3 * np.median(np.abs(tr["wo"]))).all()
    assert tr["x2"][0] == 0 and tr["x3"][0] == 0                        # norm weight 0
    w = tensors[(ff.T_INPUT_NORM, 0)]
    assert w[0] == 0 and (w[64:72] == -1.5).all() and w[130] == 40 and w[200] == np.float32(1e-6)


def test_bites_saturated_int16_group_dot():
    """the saturated int16 rows: a group dot equal to +-64 * 5792^2 (it fits int32)"""
    W, sW, X, sX = VE.matmul_case(ff.QT_INT16, 96, 256, 3, "normal")
    d = (W[:3, :64].astype(np.int64) @ X[:3, :64].astype(np.int64).T)
    assert d[0, 0] == 64 * 5792 ** 2 < 2 ** 31 and d[1, 0] == -64 * 5792 ** 2 and d[1, 2] == 64 * 5792 ** 2


def test_bites_matmul_regimes():
    """regime "denormal": denormal scale products, and denormal outputs (int8); regime "inf": infinite outputs, no NaN"""
    for qt in QTS:
        W, sW, X, sX = VE.matmul_case(qt, 96, 256, 3, "denormal")
        p = sW[:, None, :] * sX[None, :, :]
        assert ((p != 0) & (np.abs(p) < DENORM)).any()
        o = O.matmul_q(qt, W, sW, X, sX)
        assert ((o != 0) & (np.abs(o) < DENORM)).any()
        o = O.matmul_q(qt, *VE.matmul_case(qt, 96, 256, 3, "inf")[:4])
        assert np.isinf(o).any() and not np.isnan(o).any()


def test_bites_swiglu_and_softmax():
    a, b = VE.swiglu_grid()
    o = O.swiglu(a, b)
    assert np.isinf(o).any() and (np.signbit(o) & (o == 0)).any() and not np.isnan(o).any()
    for name, x, c in VE.softmax_cases():
        if name.startswith("spread 250") and c >= 64:
            w = O.softmax(x, c)[:c]
            assert (w < 1e-15).any() and (w == 0).any() and (w >= 1e-15).any()


@pytest.mark.parametrize("case", ALL_SMALL + [c for c in CASES if c[0].endswith("-equal")], ids=lambda c: c[0])
def test_bites_ties_and_overflow(case):
    """families "cls_mirror" / "cls_dup" / "cls_equal": the top logit occurs at least twice and argmax is the lower id; the row whose sum of squares overflows: every
    logit is +-0"""
    name, shape, qt, fam, layers = case
    for sname, lgs in case_logits(case).items():
        for i, l in enumerate(lgs):
            top = np.flatnonzero(l == l.max())
            assert top.size >= 2 and int(np.argmax(l)) == top[0], (sname, i)
            for a, b in VE.CLS_PAIRS:
                assert bits(l[a]) == bits(l[b])
            if name.endswith("-equal"):
                assert top.size == l.size and int(np.argmax(l)) == 0
    l = case_logits(case)["short x1e20 sum of squares overflows"][2]      # the call that feeds the row at a decode position
    assert (l == 0).all()


# ---- goldens ----------------------------------------------------------------------------------------------------------------------------------------------------------
def sha(l):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(l).tobytes()).digest(), dtype=np.uint8)


def weights_checksum(tensors):
    chk = 0
    for key, v in sorted(tensors.items()):
        for a in (v if isinstance(v, tuple) else (v,)):
            chk = (chk * 1000003 + int(np.frombuffer(np.ascontiguousarray(a).tobytes(), dtype=np.uint8).astype(np.uint64).sum())) % (1 << 61)
    return chk


GOLD_CASES = [c for c in CASES if c[1] in ("tiny", "tiny128")]


@pytest.mark.parametrize("case", GOLD_CASES, ids=[c[0] for c in GOLD_CASES])
def test_oracle_matches_reference_goldens(case):
    """tests/golden/value_edges.npz (make_golden_edges.py: recorded from the reference library): same weights, same prompts, the digest of every call's logits"""
    name, shape, qt, fam, layers = case
    g = np.load(GOLD)
    cfg, tensors = VE.edge_model(shape, qt, fam, layers)
    assert int(g[f"{name}/weights_checksum"]) == weights_checksum(tensors)
    got = case_logits(case)
    scheds = VE.case_schedules(name, cfg)
    assert np.array_equal(g[f"{name}/tokens"], np.concatenate([t for _, sch in scheds for t, _ in sch]))
    n = 0
    for sname, sch in scheds:
        for i, l in enumerate(got[sname]):
            assert np.array_equal(g[f"{name}/head"][n].view(np.uint32), bits(l[:16])), (sname, i)
            assert np.array_equal(g[f"{name}/sha256"][n], sha(l)), (sname, i)
            assert int(g[f"{name}/ids"][n]) == int(np.argmax(l))
            n += 1
    assert n == g[f"{name}/ids"].size
