"""The entropy-driven samplers without a GPU (include/flm_gpu.h: flm_entropy): flm_logf's contract as the host compiles csrc/flm_logf.h; host/sampler.cpp entropy_logits /
mirostat_update (through lib/libflm_host.so) against the plain-Python restatement of the definition (tests/entropy_util.py) on the bit patterns; rows on which the summation
order of H, or of the walk's cumulative sum, decides the kept set; the ABI's host-side validation; the binding's surface; the CLI's flags; and, on the CPU oracle's logits,
that the model-level cases of tests/test_gpu_entropy.py are not vacuous."""
import os
import re
import subprocess

import numpy as np
import pytest

import __graft_entry__ as graft
from fast_llama_amd import capi, flmfile as ff, synth
from entropy_util import (Entropy, F, NINF, bits, hand_rows, host_loop, libm_logf, order_case_H, order_case_c, py_entropy, py_logf, py_mirostat_update,
                          tree_sum)
from sample_util import host_lib, logits_case
from shape_util import Sampling

ROOT = graft.ROOT
MAIN = os.path.join(graft.PKG_DIR, "bin", "main")
TYPICALS = (0.2, 0.5, 0.95)
MUS = (0.5, 3.0, 10.0, 40.0)


def logf_inputs():
    """about 10^6 floats of [1, 2^24]: every float of [1, 1 + 2^-8), a stride through the bit patterns up to 2^24, the binade edges and sqrt(2)'s neighbours"""
    dense = np.arange(0x3F800000, 0x3F800000 + (1 << 15), dtype=np.uint32)
    stride = np.arange(0x3F800000, 0x4B800000 + 1, 211, dtype=np.uint32)
    edges = np.array([0x3F800000 + (k << 23) + o for k in range(25) for o in (-1, 0, 1) if 0x3F800000 <= 0x3F800000 + (k << 23) + o <= 0x4B800000], dtype=np.uint32)
    r2 = np.array([0x3FB504F3 + o + (k << 23) for k in range(24) for o in range(-3, 4)], dtype=np.uint32)
    return np.concatenate([dense, stride, edges, r2]).view(np.float32)


def test_logf_is_exactly_zero_at_one_and_monotone_on_the_first_floats():
    assert bits(capi.logf_host([1.0]))[0] == 0                                   # +0, not -0
    x = np.arange(0x3F800000, 0x3F800000 + (1 << 15), dtype=np.uint32).view(np.float32)      # all floats of [1, 1 + 2^-8)
    assert x[-1] < F(1 + 2.0 ** -8) <= np.nextafter(x[-1], F(2))
    y = capi.logf_host(x)
    assert np.all(np.diff(y) >= 0) and y[1] > 0


def test_logf_is_within_one_ulp_of_libm_and_non_decreasing_on_the_sample():
    x = np.sort(logf_inputs())
    assert x.size > 900000 and x[0] == 1.0 and x[-1] == F(2.0 ** 24)
    y = capi.logf_host(x)
    assert np.all(np.diff(y) >= 0)
    ref = libm_logf(x)
    ulp = np.abs(bits(y).astype(np.int64) - bits(ref).astype(np.int64))           # both are >= +0: the bit patterns are ordered as the values
    assert int(ulp.max()) <= 1, (int(ulp.max()), x[np.argmax(ulp)])
    assert float(np.mean(ulp != 0)) < 0.01


def test_logf_is_the_operations_the_header_states():
    """csrc/flm_logf.h restated operation by operation (exact-rational fma) gives the host's bits: the function is defined by its operations"""
    rng = np.random.default_rng(2)
    x = np.concatenate([np.array([1.0, 1.4142135, 1.4142137, 2.0, 3.0, 32000.0, 2.0 ** 24], np.float32),
                        rng.uniform(1, 2, 300).astype(np.float32), np.exp(rng.uniform(0, 16, 300)).astype(np.float32)])
    got = capi.logf_host(x)
    want = np.array([py_logf(v) for v in x], np.float32)
    assert np.array_equal(bits(got), bits(want))


def _rows():
    rows = dict(hand_rows())
    for n in (2, 64, 1000):
        for kind in ("peaked", "medium", "flat", "ties", "clip", "neginf"):
            rows[f"{kind} {n}"] = logits_case(kind, n, seed=11)
    return rows


def test_host_restatement_equals_the_python_formulation():
    n_cases = 0
    for name, L in _rows().items():
        for T in (0.7, 1.0, 1.5):
            for ent in [Entropy(typical_p=p) for p in TYPICALS + (1e-6, 0.999)] + [Entropy(mirostat=2, mu=m) for m in MUS + (-1.0, 1e30)]:
                got, want = capi.entropy_host(L, T, ent), py_entropy(L, T, ent)
                assert np.array_equal(bits(got), bits(want)), (name, T, ent, np.nonzero(bits(got) != bits(want))[0][:8])
                n_cases += 1
    assert n_cases > 900


def test_extreme_parameters_keep_one_entry_or_all():
    for name, L in _rows().items():
        d = (L - L.max()).astype(np.float32)
        live = np.nonzero(~(d < -15))[0]
        first = int(np.argmax(L))
        # mu below every surprise: only the first maximum stays; mu huge: nothing goes
        S = capi.entropy_host(L, 1.0, Entropy(mirostat=2, mu=-1.0))
        assert list(np.nonzero((S != NINF) & ~(d < -15))[0]) == [first], name
        assert np.array_equal(bits(capi.entropy_host(L, 1.0, Entropy(mirostat=2, mu=1e30))), bits(L)), name
        # typical_p below every probability: exactly one live entry stays (the one closest to the entropy); dead entries are never touched
        S = capi.entropy_host(L, 1.0, Entropy(typical_p=1e-9))
        assert np.count_nonzero(S[live] != NINF) == 1, name
        dead = np.nonzero(d < -15)[0]
        assert np.array_equal(bits(S[dead]), bits(L[dead])), name
        # off, or temperature 0: the row as it is
        for ent, T in ((Entropy(), 1.0), (Entropy(typical_p=1.0), 1.0), (Entropy(typical_p=0.5), 0.0), (Entropy(mirostat=2, mu=0.1), 0.0)):
            assert np.array_equal(bits(capi.entropy_host(L, T, ent)), bits(L)), (name, ent, T)


def test_all_equal_logits_keep_a_prefix_in_index_order():
    """every key is equal: the order is the index order, the kept set the first ceil-ish(typical_p * n) indices"""
    n = 64
    S = capi.entropy_host(np.full(n, 0.5, np.float32), 1.0, Entropy(typical_p=0.5))
    kept = np.nonzero(S != NINF)[0]
    assert list(kept) == list(range(len(kept))) and 32 <= len(kept) <= 34


def test_mirostat_update_equals_the_python_formulation():
    rng = np.random.default_rng(5)
    for name, L in _rows().items():
        for T in (0.7, 1.5):
            for mu in MUS:
                ent = Entropy(mirostat=2, tau=3.0, eta=0.25, mu=mu)
                S = capi.entropy_host(L, T, ent)
                kept = np.nonzero(S != NINF)[0]
                for t in {int(kept[0]), int(kept[-1]), int(rng.choice(kept))}:
                    S2, obs, mu2 = capi.entropy_host(L, T, ent, chosen=t)
                    wobs, wmu = py_mirostat_update(S, T, t, ent, mu)
                    assert np.array_equal(bits(S2), bits(S)) and bits(obs) == bits(wobs) and bits(mu2) == bits(wmu), (name, T, mu, t)
    # one kept entry: sum' == 1, the observed surprise is exactly 0 and mu moves by eta * tau
    S, obs, mu2 = capi.entropy_host(np.array([0.0, -1.0, -2.0], np.float32), 1.0, Entropy(mirostat=2, tau=3.0, eta=0.25, mu=-5.0), chosen=0)
    assert list(S) == [0.0, -np.inf, -np.inf] and obs == 0 and mu2 == F(-5.0) - F(0.25) * F(-3.0)


def test_the_summation_order_of_H_decides_the_kept_set():
    """H as a pairwise tree gives another kept set than the sequential chain: the host restatement follows the chain"""
    L, ent = order_case_H()
    seq, tree = py_entropy(L, 1.0, ent), py_entropy(L, 1.0, ent, sum_h=tree_sum)
    assert not np.array_equal(bits(seq), bits(tree))
    assert np.array_equal(bits(capi.entropy_host(L, 1.0, ent)), bits(seq))


def test_the_summation_order_of_the_walk_decides_the_kept_set():
    L, ent = order_case_c()
    seq, tree = py_entropy(L, 1.0, ent), py_entropy(L, 1.0, ent, sum_c=tree_sum)
    assert not np.array_equal(bits(seq), bits(tree))
    assert np.array_equal(bits(capi.entropy_host(L, 1.0, ent)), bits(seq))


def test_invalid_settings_are_refused_without_a_gpu():
    for ent in (Entropy(typical_p=float("nan")), Entropy(mirostat=1), Entropy(mirostat=3), Entropy(mirostat=-2), Entropy(mirostat=2, tau=float("inf")),
                Entropy(mirostat=2, eta=float("nan")), Entropy(mirostat=2, mu=float("-inf")), Entropy(typical_p=0.5, mirostat=2)):
        with pytest.raises(capi.FlmError, match="flm error -1"):
            capi.entropy_validate(ent)
        with pytest.raises(capi.FlmError, match="flm error -1"):
            capi.op_entropy_rows(np.zeros((1, 8), np.float32), 8, 1.0, ent, mu=1.0)
    for ent in (Entropy(), Entropy(typical_p=0.3), Entropy(typical_p=-1.0), Entropy(typical_p=7.0), Entropy(mirostat=2), Entropy(typical_p=1.0, mirostat=2),
                Entropy(typical_p=0.5, tau=float("nan"))):
        capi.entropy_validate(ent)
    assert capi.lib().flm_entropy_validate(None) == -1
    L = np.zeros((1, 8), np.float32)
    for bad in (lambda: capi.op_entropy_rows(L, 9, 1.0, Entropy(typical_p=0.5)), lambda: capi.op_entropy_rows(L, 1, 1.0, Entropy(typical_p=0.5)),
                lambda: capi.op_entropy_rows(np.zeros((17, 8), np.float32), 8, 1.0, Entropy(typical_p=0.5)),
                lambda: capi.op_entropy_rows(L, 8, 1.0, Entropy(mirostat=2)), lambda: capi.op_entropy_rows(L, 8, 1.0, Entropy(mirostat=2), mu=1.0, chosen=[8]),
                lambda: capi.op_entropy_rows(L, 8, -1.0, Entropy(typical_p=0.5))):
        with pytest.raises(capi.FlmError, match="flm error -1"):
            bad()
    assert capi.lib().flm_entropy_set(None, None) == -1 and capi.lib().flm_entropy_mu(None, None) == -1


def test_the_binding_declares_the_new_entry_points():
    hdr = open(os.path.join(ROOT, "include", "flm_gpu.h")).read()
    lib = capi.lib()
    for sym in ("flm_entropy_validate", "flm_entropy_set", "flm_entropy_mu", "flm_op_entropy_rows", "flm_op_logf"):
        assert sym + "(" in hdr and sym in capi.SYMBOLS and hasattr(lib, sym)
    m = re.search(r"typedef struct flm_entropy \{(.*?)\} flm_entropy;", hdr, re.S)
    fields = re.findall(r"(\w+)\s*[,;]", re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S))
    assert fields == [f for f, _ in capi.EntropyStruct._fields_], fields
    for name in ("entropy_set", "entropy_mu"):
        assert hasattr(capi.Ctx, name)
    assert callable(capi.op_entropy_rows) and callable(capi.op_logf) and callable(capi.entropy_host)
    assert Entropy(mirostat=2, tau=4.0).struct().mu == 8.0                       # the usual starting state: 2 tau
    # the two combinations that are not built are listed where a caller looks
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    for text in (hdr, design):
        assert re.search(r"NOT built.{0,80}Mirostat through the draft-and-verify", text, re.S | re.I) and re.search(r"armed for log-probabilities", text)


def test_cli_parses_the_entropy_flags():
    for flags in (["--typical", "nan"], ["--typical", "x"], ["--mirostat", "1"], ["--mirostat", "3"], ["--mirostat", "2", "--mirostat-ent", "inf"],
                  ["--mirostat", "2", "--mirostat-lr", "nan"], ["--mirostat", "2", "--typical", "0.5"]):
        r = subprocess.run([MAIN, "-c", "/nonexistent.flm", *flags], capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and "Invalid sampling control" in r.stderr, (flags, r.stderr[-300:])
    for flags in (["--typical", "0.5"], ["--mirostat", "2", "--mirostat-ent", "4", "--mirostat-lr", "0.2"], ["--mirostat", "0"], ["--typical", "1"]):
        r = subprocess.run([MAIN, "-c", "/nonexistent.flm", *flags], capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and "Invalid sampling control" not in r.stderr, (flags, r.stderr[-300:])      # (accepted: it fails at the model file)
    r = subprocess.run([MAIN, "--help"], capture_output=True, text=True, timeout=60)
    for flag in ("--typical", "--mirostat", "--mirostat-ent", "--mirostat-lr"):
        assert re.search(re.escape(flag) + r"\s.*this build only", r.stderr), flag


# ---- the model-level cases of tests/test_gpu_entropy.py are not vacuous -------------------------------------------------------------------------------------------
class _OracleCtx:
    """flm_forward / flm_reset_kv on the CPU oracle"""

    def __init__(self, cfg, tensors):
        import oracle_py
        self.m = oracle_py.OracleModel(cfg, tensors)

    def reset_kv(self):
        pass

    def forward(self, tokens, pos):
        return self.m.forward(np.asarray(tokens, np.int32), pos)


def test_the_model_level_cases_mask_something_in_most_steps():
    """tests/test_gpu_entropy.py compares flm_generate_ex with the host loop under these settings; on the oracle's logits for the same model, prompt and seeds the stage
    masks between 1 and n - 1 live entries in at least half of the steps (the first maximum always stays: at most n - 1), so that equality says something"""
    import test_gpu_entropy as G
    for name in ("tiny", "tiny16"):
        shape, qt, seed = G.MODELS[name]
        cfg = synth.make_config(shape, qt)
        ctx = _OracleCtx(cfg, synth.make_tensors(cfg, seed=seed))
        prompt = G.prompt_of(cfg.vocab_size, G.N_PROMPT)
        for label, (s, ent) in G.plain_cases().items():
            _, _, _, _, counts = host_loop(ctx, host_lib(), prompt, G.N_TOKENS, s, ent, G.SEED)
            masked = [live - kept for kept, live in counts]
            assert all(0 <= m < live for m, (_, live) in zip(masked, counts))
            assert sum(1 for m in masked if m >= 1) * 2 >= len(masked), (name, label, masked)
