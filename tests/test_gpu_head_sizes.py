"""The head-size axis at op level: flm_op_rope, flm_op_attention (one workgroup per head and split), flm_op_attention_slots and flm_op_attention_fan at every size of
tests/head_sizes.py's table, against the CPU oracle DIRECTLY (never against another GPU kernel: two kernels cannot agree on a common mistake).  Everything is equality on
bit patterns.  In the attention tests every cache row behind a query's own range holds NaN, so an over-read poisons the result.

What each size exercises (csrc/flm_attn.h): 32 / 40 / 56 / 64 attn_head<1>, 72 / 96 / 120 / 128 attn_head<2>, 136 / 160 / 192 / 200 / 256 attn_head<4> (LDS row stride 72 /
136 / 264 against rows of hs floats; hs / 4 16-byte pieces per row, a divisor that is no power of two at most sizes); 96 with FLM_OP_ATTN_PARTS: three parts per head, which
do not divide the 16 position tiles of 1024 rows evenly."""
import ctypes

import numpy as np
import pytest

import head_sizes as HS
import oracle_py as O

pytestmark = pytest.mark.gpu
SIZE_IDS = [f"hs{hs}" for hs in HS.SIZES]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("hs", HS.SIZES, ids=SIZE_IDS)
def test_rope(gpu, hs):
    """hs / 2 table entries per position: 16 .. 128 pairs"""
    for pos in HS.ROPE_POSITIONS:
        x = HS.rope_input(hs, pos)
        assert np.array_equal(bits(gpu.op_rope(x, pos)), bits(O.rope(x, pos))), (hs, pos)


def _run_decode(gpu, hs, heads, positions, peaked_at, max_seq, seed):
    steps, kc, vc = HS.decode_steps(hs, heads, positions, peaked_at, max_seq, seed)
    for s in steps:
        pos = s["pos"]
        if pos == peaked_at:                                              # (NumPy first: the step is what it is named for)
            assert all(HS.is_peaked(HS.softmax_weights(kc[h], s["q"][h], s["k"][h], hs, pos)) for h in range(min(heads, 3))), "the case is not peaked enough"
        kg, vg = HS.cache_before(kc, pos), HS.cache_before(vc, pos)
        out = gpu.op_attention(kg, vg, s["q"].reshape(-1), s["k"].reshape(-1), s["v"].reshape(-1), heads, hs, max_seq, pos).reshape(heads, hs)
        assert np.array_equal(bits(kg[:, pos]), bits(s["krow"])), (hs, pos, "the appended K row")
        assert np.array_equal(bits(vg[:, pos]), bits(s["vrow"])), (hs, pos, "the appended V row")
        assert np.array_equal(bits(out), bits(s["out"])), (hs, pos, np.argwhere(bits(out) != bits(s["out"]))[:4].tolist())
        assert np.array_equal(bits(kg[:, :pos]), bits(kc[:, :pos])) and np.isnan(kg[:, pos + 1:]).all() and np.isnan(vg[:, pos + 1:]).all(), (hs, pos, "another row was written")


@pytest.mark.parametrize("hs", HS.SIZES, ids=SIZE_IDS)
def test_attention_decode(gpu, hs):
    """k_rope_kv + k_attn_decode<false>, three heads, max_seq 512, the positions of test_gpu_ops.test_attention_decode; the step at position 130 has a peaked query"""
    _run_decode(gpu, hs, 3, HS.DECODE_POSITIONS, HS.PEAKED_AT, 512, 0)


@pytest.mark.parametrize("heads", [3, 32])
def test_attention_decode_three_parts(gpu, heads, monkeypatch):
    """head size 96 with FLM_OP_ATTN_PARTS: G = 3 parts per head, ceil(nt / 3) position tiles each (1024 rows: 6, 6 and 4 tiles; 257 rows: 2, 2 and 1; up to 128 rows:
    parts without a tile); the peaked step at 700"""
    monkeypatch.setenv("FLM_OP_ATTN_PARTS", "3")
    assert HS.split_parts(96) == 3
    _run_decode(gpu, 96, heads, HS.SPLIT_POSITIONS, HS.SPLIT_PEAKED_AT, 1024, 1)


@pytest.mark.parametrize("hs", [40, 160], ids=["hs40", "hs160"])
def test_attention_decode_cannot_split(gpu, hs, monkeypatch):
    """FLM_OP_ATTN_PARTS at a size that is no multiple of 32 / above 128: the op quietly runs one workgroup per head and still equals the oracle"""
    monkeypatch.setenv("FLM_OP_ATTN_PARTS", "4")
    assert HS.split_parts(hs) == 1
    _run_decode(gpu, hs, 3, HS.SPLIT_POSITIONS, HS.SPLIT_PEAKED_AT, 1024, 2)


@pytest.mark.parametrize("hs", HS.SLOT_SIZES, ids=[f"hs{hs}" for hs in HS.SLOT_SIZES])
def test_attention_slots(gpu, hs):
    """k_rope_kv_slots + k_attn_slots, B = 3 at positions 0 / 64 / 130 in slots that abut: a read one row past a sequence's last lands in its neighbour or in NaN"""
    kc, vc, q, k, v, base, pos, max_seq, want = HS.slots_case(hs)
    assert all(base[r + 1] == base[r] + pos[r] + 1 for r in range(len(pos) - 1))
    kc0, vc0 = kc.copy(), vc.copy()
    out = gpu.op_attention_slots(kc, vc, q, k, v, HS.OP_HEADS, hs, max_seq, base, pos)
    written = np.zeros(max_seq, bool)
    for r, (b, p) in enumerate(zip(base, pos)):
        o, krow, vrow = want[r]
        assert np.array_equal(bits(out[r]), bits(o)), (hs, r, p)
        assert np.array_equal(bits(kc[:, b + p]), bits(krow)) and np.array_equal(bits(vc[:, b + p]), bits(vrow)), (hs, "the step's K/V row", r)
        written[b + p] = True
    assert np.array_equal(bits(kc[:, ~written]), bits(kc0[:, ~written])) and np.array_equal(bits(vc[:, ~written]), bits(vc0[:, ~written])), (hs, "a row nobody wrote has changed")


@pytest.mark.parametrize("n", [3, 9])
@pytest.mark.parametrize("hs", HS.FAN_SIZES, ids=[f"hs{hs}" for hs in HS.FAN_SIZES])
def test_attention_fan(gpu, hs, n):
    """k_rope_kv_fan + k_attn_fan: 64 / 128 threads per query of which hs are live; a shared prefix of 65 rows and tails of 69 earlier rows (both cross a tile); n = 3 (a
    partial group of queries) and n = 9 (a full group and a single query)"""
    kc, vc, q, k, v, base, max_seq, want = HS.fan_case(hs, n)
    kc0, vc0 = kc.copy(), vc.copy()
    out = gpu.op_attention_fan(kc, vc, q, k, v, HS.OP_HEADS, hs, max_seq, HS.FAN_S, HS.FAN_T, base)
    written = np.zeros(max_seq, bool)
    for j, b in enumerate(base):
        o, krow, vrow = want[j]
        assert np.array_equal(bits(out[j]), bits(o)), (hs, n, j)
        assert np.array_equal(bits(kc[:, b + HS.FAN_T]), bits(krow)) and np.array_equal(bits(vc[:, b + HS.FAN_T]), bits(vrow)), (hs, n, "the step's K/V row", j)
        written[b + HS.FAN_T] = True
    assert np.array_equal(bits(kc[:, ~written]), bits(kc0[:, ~written])) and np.array_equal(bits(vc[:, ~written]), bits(vc0[:, ~written])), (hs, n, "a row nobody owns was written")


def test_attention_fan_refuses_head_size_136(gpu):
    """above 128 there is no multi-query attention: -1 (FLM_ERR_INVALID), the cache untouched"""
    hs, n = 136, 3
    rng = np.random.default_rng(136)
    S, t = 8, 2
    max_seq = S + n * (t + 1) + 3
    kc = rng.standard_normal((HS.OP_HEADS, max_seq, hs)).astype(np.float32); vc = rng.standard_normal((HS.OP_HEADS, max_seq, hs)).astype(np.float32)
    q = rng.standard_normal((n, HS.OP_HEADS * hs)).astype(np.float32)
    out = np.empty_like(q); base = np.array([S + j * (t + 1) for j in range(n)], np.int32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)      # noqa: E731
    k0, v0 = kc.copy(), vc.copy()
    assert gpu.lib().flm_op_attention_fan(p(out), p(kc), p(vc), p(q), p(q), p(q), HS.OP_HEADS, hs, max_seq, n, S, t, p(base)) == -1
    assert np.array_equal(bits(kc), bits(k0)) and np.array_equal(bits(vc), bits(v0))
