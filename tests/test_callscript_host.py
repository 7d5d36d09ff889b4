"""The call-script generator of tests/callscript.py without a GPU: a seed is a script, every script keeps the preconditions of the calls it makes, and the oracle's side
of every committed seed runs to its end on the CPU -- the reference alone stays inside what the scripts assume."""
import json

import numpy as np
import pytest

import callscript as CS
import oracle_py as O
from sample_util import host_lib


def test_same_seed_same_script():
    for seed in (1, 2, 3, 77):
        a = CS.generate(seed, 1024, 1024, n_layers=2)
        assert a == CS.generate(seed, 1024, 1024, n_layers=2) and json.loads(json.dumps(a)) == a
        assert a != CS.generate(seed + 1000, 1024, 1024, n_layers=2)


def test_every_script_respects_the_preconditions():
    """pos + n inside max_seq_len with the fill below it, rewinds go back only, at most two injections a probation apart, tokens inside the vocabulary, and -- over many
    seeds -- every kind of operation and both directions across the split heads' 128-position switch occur"""
    seen, up, down = set(), 0, 0
    for seed in range(300):
        vocab, max_seq = (320, 1024) if seed % 2 else (1024, 300)
        ops = CS.generate(seed, vocab, max_seq, n_layers=2, world=2 if seed % 7 == 0 else 1)
        assert 40 <= len(ops) <= 42
        tokens, sampled, inj = CS.check_script(ops, vocab, max_seq)
        assert tokens > 0 and inj <= CS.MAX_INJECTIONS
        fill = 0
        for op in ops:
            seen.add(op["op"] + ":" + str(op.get("kind", "")))
            if op["op"] in ("forward", "decode"):
                up += fill < 128 <= op["pos"] + (len(op["tokens"]) if op["op"] == "forward" else op["n"])
                down += op["pos"] < 128 <= fill
                fill = op["pos"] + (len(op["tokens"]) if op["op"] == "forward" else op["n"])
            elif op["op"] in ("reset_decode", "kernel_times"):
                fill = op.get("n", 0)
        if seed % 7 == 0:
            assert not any(op["op"] in ("inject", "kernel_times", "reset_decode") for op in ops)
            assert all(op["key"] in CS.LIVE_OPTIONS_TP for op in ops if op["op"] == "set_option")
    assert {"forward:logits", "forward:argmax", "forward:sample", "decode:greedy", "decode:sample", "reset_decode:", "set_option:", "inject:", "age:", "kernel_times:"} <= seen, seen
    assert up > 50 and down > 50
    no_sample = CS.generate(5, 40000, 1024, sample_ok=False)
    assert not any(op.get("kind") == "sample" for op in no_sample)


def test_a_rewind_on_the_oracle_is_a_replay_from_an_empty_cache():
    """the oracle's cache is rows in an array: forward(tokens, pos) below the fill overwrites and attends like a model that never saw the rows beyond -- what OracleSide relies on"""
    cfg, tensors = CS.model("tiny128_16")
    a, b = O.OracleModel(cfg, tensors), O.OracleModel(cfg, tensors)
    rng = np.random.default_rng(3)
    first, second = rng.integers(1, cfg.vocab_size, 150).astype(np.int32), rng.integers(1, cfg.vocab_size, 20).astype(np.int32)
    a.forward(first, 0)
    got = a.forward(second, 70)
    b.forward(first[:70], 0)
    want = b.forward(second, 70)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("seed,name,world", CS.FIXED)
def test_committed_seeds_replay_on_the_oracle(seed, name, world):
    cfg, tensors = CS.model(name)
    ops = CS.fixed_script(seed, name, world)
    tokens, sampled, _ = CS.check_script(ops, cfg.vocab_size, CS.MAX_SEQ, CS.SAMPLE_VOCAB_LIMIT)
    side = CS.OracleSide(O.OracleModel(cfg, tensors, max_seq=CS.MAX_SEQ), host_lib())
    for op in ops:
        out = side.expect(op)
        if "logits" in out:
            assert np.all(np.isfinite(out["logits"]))
        for t in out.get("ids", []):
            assert 0 <= t < cfg.vocab_size
    assert side.tokens == tokens and side.sampled == sampled
