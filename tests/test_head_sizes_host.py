"""The head-size table (tests/head_sizes.py) proven on the CPU before any of it goes near a GPU:
  * the table reaches every dispatch class the library accepts;
  * the oracle equals the reference library bit for bit at every table size -- the logits of a short prompt and five greedy steps, and RoPE at positions 0, 1, 37
    and 255 (skipped where oracle/_ref/libflref.so is absent; the committed tests/golden/head_sizes.npz, recorded from the reference, keeps the pin there);
  * nothing the GPU tests compare against holds a NaN or an Inf."""
import hashlib
import os

import numpy as np
import pytest

import head_sizes as HS
import oracle_py as O
from fast_llama_amd import flmfile as ff, synth

needs_ref = pytest.mark.skipif(not O.have_ref(), reason="oracle/_ref/libflref.so not built (needs /root/reference)")
GOLD = os.path.join(os.path.dirname(__file__), "golden", "head_sizes.npz")
SIZE_IDS = [f"hs{hs}" for hs in HS.SIZES]
CASE_IDS = [HS.case_id(c) for c in HS.CASES]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def sha(l):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(l).tobytes()).digest(), dtype=np.uint8)


def weights_checksum(tensors):
    chk = 0
    for key, v in sorted(tensors.items()):
        for a in (v if isinstance(v, tuple) else (v,)):
            chk = (chk * 1000003 + int(np.frombuffer(np.ascontiguousarray(a).tobytes(), dtype=np.uint8).astype(np.uint64).sum())) % (1 << 61)
    return chk


# ---- the table --------------------------------------------------------------------------------------------------------------------------------------------------------
def test_table_reaches_every_dispatch_class():
    """a later edit of the table cannot silently drop a class: every class some accepted head size falls in has a table entry; the issue's sizes and anchors stay"""
    accepted = {HS.dispatch_class(hs) for hs in HS.ACCEPTED}
    table = {HS.dispatch_class(hs) for hs in HS.SIZES}
    assert accepted == table, sorted(accepted - table)
    assert len(accepted) == 9                                              # three widths x (no multiple of 32, of 32 only, of 64)
    assert set(HS.SIZES) >= {40, 56, 72, 120, 96, 136, 200, 160, 192, 256, 64, 128} and set(HS.SIZES) <= set(HS.ACCEPTED)
    assert {HS.dispatch_class(hs)[0] for hs in HS.INT16_SIZES} == {0, 1, 2} and set(HS.INT16_SIZES) <= set(HS.SIZES) and set(HS.ENTRY_SIZES) <= set(HS.SIZES)
    assert HS.split_parts(96) == 3 and {hs for hs in HS.SIZES if HS.split_parts(hs) > 1} == {64, 96, 128}


@pytest.mark.parametrize("hs", HS.SIZES, ids=SIZE_IDS)
def test_table_shapes(hs):
    dim, hidden, layers, heads, vocab = HS.SHAPES[hs]
    assert dim == hs * heads and dim % 64 == 0 and 256 <= dim <= 2048 and dim * dim // 24576 >= 2      # (the reference runs it with two threads)
    assert hidden % 64 == 0 and (hidden // 64) % 2 == 1 and layers == 2 and vocab % 2 == 1
    assert max(int(HS.LONG_PROMPT.max()), int(HS.SHORT_PROMPT.max())) < vocab


# ---- oracle == reference ----------------------------------------------------------------------------------------------------------------------------------------------
@needs_ref
@pytest.mark.parametrize("case", HS.CASES, ids=CASE_IDS)
def test_model_oracle_equals_reference(tmp_path, case):
    hs, qt = case
    cfg, tensors = HS.model(hs, qt)
    path = tmp_path / "m.flm"
    synth.write_synthetic_flm(str(path), cfg, tensors=tensors)
    got = HS.greedy_run(O.RefModel(path, qt, threads=2), HS.SHORT_PROMPT, HS.N_GREEDY_REF)
    want = HS.short_logits(hs, qt)
    assert len(got) == len(want) == 1 + HS.N_GREEDY_REF
    for i, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(bits(g), bits(w)), (hs, qt, i)


@needs_ref
@pytest.mark.parametrize("hs", HS.SIZES, ids=SIZE_IDS)
def test_rope_oracle_equals_reference(hs):
    R = O.ref()
    for pos in HS.ROPE_POSITIONS:
        x = HS.rope_input(hs, pos)
        assert np.array_equal(bits(O.rope(x, pos)), bits(O.rope(x, pos, lib=R))), (hs, pos)


# ---- the golden fixture -----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", HS.CASES, ids=CASE_IDS)
def test_oracle_matches_reference_goldens(case):
    """tests/golden/head_sizes.npz (make_golden_heads.py: recorded from the reference library): same weights, same prompt, the digest, the argmax and the first 16
    values of every call's logits"""
    hs, qt = case
    name = HS.case_id(case)
    g = np.load(GOLD)
    cfg, tensors = HS.model(hs, qt)
    assert np.array_equal(g[f"{name}/shape"], np.array(HS.SHAPES[hs], np.int32))
    assert int(g[f"{name}/weights_checksum"]) == weights_checksum(tensors)
    assert np.array_equal(g[f"{name}/prompt"], HS.SHORT_PROMPT)
    got = HS.short_logits(hs, qt)
    assert g[f"{name}/ids"].size == len(got) == 1 + HS.N_GREEDY_REF
    for i, l in enumerate(got):
        assert np.isfinite(l).all(), (name, i)
        assert np.array_equal(g[f"{name}/head"][i].view(np.uint32), bits(l[:16])), (name, i)
        assert np.array_equal(g[f"{name}/sha256"][i], sha(l)), (name, i)
        assert int(g[f"{name}/ids"][i]) == int(np.argmax(l)), (name, i)


@pytest.mark.parametrize("hs", HS.SIZES, ids=SIZE_IDS)
def test_rope_matches_reference_goldens(hs):
    g = np.load(GOLD)
    assert np.array_equal(g["rope/positions"], np.array(HS.ROPE_POSITIONS, np.int32))
    for i, pos in enumerate(HS.ROPE_POSITIONS):
        x = HS.rope_input(hs, pos)
        assert np.array_equal(g[f"rope/hs{hs}/in"][i].view(np.uint32), bits(x)), (hs, pos)
        o = O.rope(x, pos)
        assert np.isfinite(o).all()
        assert np.array_equal(g[f"rope/hs{hs}/out"][i].view(np.uint32), bits(o)), (hs, pos)


# ---- what the GPU tests compare against is finite -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", HS.CASES, ids=CASE_IDS)
def test_model_schedule_is_finite(case):
    """the GPU model tests' schedule (tests/test_gpu_head_sizes_model.py): every logit finite, the batched prompt equal to the same prompt fed token by token"""
    hs, qt = case
    run = HS.long_run(hs, qt)
    for l in run["first5"] + [run["prompt"]] + run["steps"]:
        assert np.isfinite(l).all()
    assert len(run["ids"]) == HS.N_GREEDY and all(0 <= t < HS.VOCAB for t in run["ids"])
    form = HS.form_run(hs, qt)                                             # (the launch-form test's 128-row context, filled to its last row)
    assert np.isfinite(form["logits"]).all() and 5 + len(form["ids5"]) + 1 + len(form["ids"]) == HS.FORM_ROWS
    if hs in HS.INT16_SIZES and qt == ff.QT_INT8:                      # (four sizes, one per class and 96: the oracle's two prompt paths agree)
        om = O.OracleModel(*HS.model(hs, qt))
        for i in range(len(HS.LONG_PROMPT)):
            last = om.forward(HS.LONG_PROMPT[i:i + 1], i)
        assert np.array_equal(bits(last), bits(run["prompt"])), hs


@pytest.mark.parametrize("hs", HS.SIZES, ids=SIZE_IDS)
def test_op_cases_are_nan_free_and_peaked(hs):
    """every op-level reference output is finite although the caches hold NaN behind every query's own range (the oracle reads nothing there), and the peaked step has
    weights under the skip threshold next to weights that count"""
    steps, kc, vc = HS.decode_steps(hs, 3, HS.DECODE_POSITIONS, HS.PEAKED_AT, 512, 0)
    assert [s["pos"] for s in steps] == list(HS.DECODE_POSITIONS)
    for s in steps:
        assert np.isfinite(s["out"]).all() and np.isfinite(s["krow"]).all() and np.isfinite(s["vrow"]).all(), (hs, s["pos"])
        kg = HS.cache_before(kc, s["pos"])
        assert np.isnan(kg[:, s["pos"]:]).all() and np.isfinite(kg[:, :s["pos"]]).all()
        if s["pos"] == HS.PEAKED_AT:
            for h in range(3):
                assert HS.is_peaked(HS.softmax_weights(kc[h], s["q"][h], s["k"][h], hs, s["pos"])), (hs, h)
    if hs in HS.SLOT_SIZES:
        for o, kr, vr in HS.slots_case(hs)[-1]:
            assert np.isfinite(o).all() and np.isfinite(kr).all() and np.isfinite(vr).all()
    if hs in HS.FAN_SIZES:
        for n in (3, 9):
            for o, kr, vr in HS.fan_case(hs, n)[-1]:
                assert np.isfinite(o).all() and np.isfinite(kr).all() and np.isfinite(vr).all()


def test_split_case_is_peaked():
    """the three-part split at head size 96: the step at position 700 is peaked in every head"""
    for heads in (3, 32):
        steps, kc, _ = HS.decode_steps(96, heads, HS.SPLIT_POSITIONS, HS.SPLIT_PEAKED_AT, 1024, 1)
        s = [x for x in steps if x["pos"] == HS.SPLIT_PEAKED_AT][0]
        for h in range(heads):
            assert HS.is_peaked(HS.softmax_weights(kc[h], s["q"][h], s["k"][h], 96, s["pos"])), (heads, h)
        assert all(np.isfinite(x["out"]).all() for x in steps)
