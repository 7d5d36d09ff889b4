"""The logit-shaping stage without a GPU: host/sampler.cpp shape_logits (through lib/libflm_host.so: fh_shape) against an independent NumPy formulation of the definition
in include/flm_gpu.h (tests/shape_util.py np_shape: a Counter for the penalties, a stable argsort for top-k, libm's logf through ctypes) -- bit for bit; the binding's surface;
the CLI's flags."""
import os
import re
import subprocess

import numpy as np
import pytest

import __graft_entry__ as graft
from fast_llama_amd import capi
from shape_util import NINF, SIZES, Sampling, bits, grid, logf, np_shape

ROOT = graft.ROOT
MAIN = os.path.join(graft.PKG_DIR, "bin", "main")


@pytest.mark.parametrize("n", SIZES)
def test_host_restatement_equals_the_numpy_formulation(n):
    cases = grid(n)
    assert len(cases) > 60
    for name, L, s, w in cases:
        got, want = capi.shape_host(L, s, w), np_shape(L, s, w)
        assert np.array_equal(bits(got), bits(want)), (n, name, np.nonzero(bits(got) != bits(want))[0][:8])


def test_top_k_keeps_exactly_k_and_ties_go_to_the_lower_index():
    n, k = 4099, 37
    L = np.full(n, -1.0, np.float32)
    mx = np.sort(np.random.default_rng(5).permutation(n)[:500])
    L[mx] = 0.0
    for row in (L, np.where(np.isin(np.arange(n), mx[::2]), np.float32(-0.0), L).astype(np.float32)):
        S = capi.shape_host(row, Sampling(temperature=1.0, top_k=k))
        assert list(np.nonzero(S != NINF)[0]) == list(mx[:k])
        assert np.array_equal(bits(S[mx[:k]]), bits(row[mx[:k]]))          # the survivors keep their bits (-0.0 stays -0.0)
        assert np.array_equal(bits(S), bits(np_shape(row, Sampling(temperature=1.0, top_k=k))))


def test_min_p_keeps_the_entry_at_the_threshold_and_drops_the_next_float_below():
    mp = 0.1
    lt = logf(np.float32(mp))
    L = np.array([0.0, lt, np.nextafter(lt, NINF), -1.0, -np.inf, np.nextafter(lt, np.float32(0))], np.float32)      # T = 1, max 0: y - mx = the logit itself
    S = capi.shape_host(L, Sampling(temperature=1.0, min_p=mp))
    assert list(S != NINF) == [True, True, False, True, False, True]
    assert np.array_equal(bits(S), bits(np_shape(L, Sampling(temperature=1.0, min_p=mp))))
    # temperature 0: min-p does not apply
    assert np.array_equal(bits(capi.shape_host(L, Sampling(temperature=0.0, min_p=mp))), bits(L))


def test_each_distinct_id_is_penalised_once_however_often_it_occurs():
    L = np.array([2.0, -2.0, 0.0, -np.inf, 1.0], np.float32)
    w = np.array([0] * 300 + [1, 1, 2, 3], np.int32)
    S = capi.shape_host(L, Sampling(temperature=1.0, repeat_penalty=2.0), w)
    assert list(S) == [1.0, -4.0, 0.0, -np.inf, 1.0]
    S = capi.shape_host(L, Sampling(temperature=1.0, frequency_penalty=0.5, presence_penalty=1.0), w)
    assert list(S) == [2.0 - 151.0, -2.0 - 2.0, -1.5, -np.inf, 1.0]


def test_neutral_controls_leave_the_bits_alone():
    L = np.array([-0.0, 0.0, 1.5, -np.inf, -0.0, -3.0, 7.0], np.float32)
    w = np.array([0, 4, 1, 0], np.int32)
    for s in (Sampling(temperature=0.8), Sampling(temperature=0.8, top_k=len(L)), Sampling(temperature=0.8, top_k=len(L) + 5),
              Sampling(temperature=0.8, repeat_penalty=1.0, frequency_penalty=0.0, presence_penalty=0.0)):
        assert np.array_equal(bits(capi.shape_host(L, s, w)), bits(L))
        assert np.array_equal(bits(np_shape(L, s, w)), bits(L))
    # penalties set and an empty window: neutral as well
    assert np.array_equal(bits(capi.shape_host(L, Sampling(temperature=0.8, repeat_penalty=1.3, presence_penalty=0.5), ())), bits(L))
    # a repetition penalty alone leaves a zero's sign alone: the frequency / presence stage does not run
    assert np.array_equal(bits(capi.shape_host(L, Sampling(temperature=0.8, repeat_penalty=1.3), w))[[0, 1, 4]], bits(L)[[0, 1, 4]])


def test_the_binding_declares_the_new_entry_points():
    hdr = open(os.path.join(ROOT, "include", "flm_gpu.h")).read()
    lib = capi.lib()
    for sym in ("flm_generate_ex", "flm_forward_sample_ex", "flm_op_shape_logits"):
        assert sym + "(" in hdr and sym in capi.SYMBOLS and hasattr(lib, sym)
    m = re.search(r"typedef struct flm_sampling \{(.*?)\} flm_sampling;", hdr, re.S)
    fields = re.findall(r"(\w+)\s*[,;]", re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S))
    assert fields == [f for f, _ in capi.SamplingStruct._fields_], fields
    assert "#define FLM_PENALTY_WINDOW_MAX 1024" in hdr and "#define FLM_BIAS_MAX 256" in hdr
    assert (capi.PENALTY_WINDOW_MAX, capi.BIAS_MAX) == (1024, 256)
    assert hasattr(capi.Ctx, "generate_ex") and hasattr(capi.Ctx, "forward_sample_ex") and callable(capi.op_shape_logits)


def test_invalid_controls_are_refused_without_a_gpu():
    """flm_op_shape_logits validates before it touches a device"""
    L = np.zeros(16, np.float32)
    bad = [Sampling(top_k=-1), Sampling(min_p=1.0), Sampling(min_p=-0.1), Sampling(min_p=float("nan")), Sampling(repeat_penalty=0.0), Sampling(repeat_penalty=-1.0),
           Sampling(repeat_penalty=float("nan")), Sampling(frequency_penalty=float("nan")), Sampling(presence_penalty=float("nan")), Sampling(penalty_last_n=-1),
           Sampling(penalty_last_n=1025), Sampling(bias={16: 1.0}), Sampling(bias={-1: 1.0}), Sampling(bias=([3, 3], [1.0, 2.0])), Sampling(bias={3: float("nan")}),
           Sampling(bias={3: float("inf")}), Sampling(bias=(list(range(257)), [0.0] * 257))]
    for s in bad:
        with pytest.raises(capi.FlmError, match="flm error -1"):
            capi.op_shape_logits(L, s)
    for w in ([16], [-1], [0] * 1025):
        with pytest.raises(capi.FlmError, match="flm error -1"):
            capi.op_shape_logits(L, Sampling(repeat_penalty=1.1), w)
    sp = capi.SamplingStruct()
    assert capi.lib().flm_op_shape_logits(capi._p(L), 16, None, None, 0, capi._p(L)) == -1


def test_cli_rejects_bad_sampling_flags():
    for flags in (["--top-k", "-1"], ["--min-p", "1"], ["--repeat-penalty", "0"], ["--repeat-last-n", "1025"], ["--logit-bias", "5"], ["--logit-bias", "5=inf"],
                  ["--logit-bias", "1=2,"], ["--presence-penalty", "x"]):
        r = subprocess.run([MAIN, "-c", "/nonexistent.flm", *flags], capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and "Invalid sampling control" in r.stderr, (flags, r.stderr[-300:])
    r = subprocess.run([MAIN, "--help"], capture_output=True, text=True, timeout=60)
    for flag in ("--top-k", "--min-p", "--repeat-penalty", "--repeat-last-n", "--presence-penalty", "--frequency-penalty", "--logit-bias"):
        assert re.search(re.escape(flag) + r"\s.*this build only", r.stderr), flag
