"""The record of a drawn token on the host (include/flm_gpu.h flm_logprob; host/sampler.cpp logprob_row through fh_logprob_row): equal to an independent NumPy statement of
the definition on the bit patterns, its statistics those of fh_score_row, the log-probability formula of capi.logprob_values, and the struct's layout.  No GPU."""
import ctypes as C

import numpy as np
import pytest

from fast_llama_amd import capi
from logprob_util import NMAX, diff_records, host_logprob, numpy_logprob, same_records
from sample_util import host_lib, logits_case
from score_util import host_score
from shape_util import KINDS

SIZES = (2, 63, 64, 65, 1000, 4099, 32000)
TOPS = (0, 1, 5, 20)


def _check(x, chosen, top_n):
    got, want = host_logprob(x, [chosen], top_n), numpy_logprob(x, chosen, top_n)
    assert same_records(got, want), (x.size, chosen, top_n, diff_records(got, want))
    return got


@pytest.mark.parametrize("n", SIZES)
def test_host_equals_the_numpy_statement(n):
    for kind in KINDS:
        x = logits_case(kind, n, seed=n)
        chosen = int(np.random.default_rng(n).integers(0, n))
        for top_n in TOPS:
            got = _check(x, chosen, top_n)
            assert int(got["n_top"][0]) == min(top_n, n) and not got["top_id"][0, min(top_n, n):].any() and not got["top_logit"][0, min(top_n, n):].view(np.uint32).any()


@pytest.mark.parametrize("n", SIZES)
def test_an_all_equal_row_lists_the_lowest_indices(n):
    x = np.full(n, 1.25, np.float32)
    for top_n in TOPS:
        got = _check(x, n - 1, top_n)
        k = min(top_n, n)
        assert got["top_id"][0, :k].tolist() == list(range(k))


def test_minus_zero_ties_plus_zero():
    x = np.full(100, -1.0, np.float32)
    x[[7, 3, 50, 20]] = [0.0, -0.0, -0.0, 0.0]
    got = _check(x, 50, 5)
    assert got["top_id"][0, :5].tolist() == [3, 7, 20, 50, 0]
    assert got["top_logit"][0, :4].view(np.uint32).tolist() == [0x80000000, 0, 0, 0x80000000]      # each entry's own bits
    assert got["logit"].view(np.uint32)[0] == 0x80000000


def test_two_entries_with_top_n_20():
    got = _check(np.array([-3.0, 4.0], np.float32), 0, 20)
    assert int(got["n_top"][0]) == 2 and got["top_id"][0].tolist() == [1, 0] + [0] * 18 and got["top_logit"][0].tolist() == [4.0, -3.0] + [0.0] * 18


def test_neginf_entries_take_part_by_index():
    x = np.full(40, -np.inf, np.float32)
    x[[30, 4]] = [1.0, 2.0]
    got = _check(x, 4, 5)
    assert got["top_id"][0, :5].tolist() == [4, 30, 0, 1, 2] and np.isneginf(got["top_logit"][0, 2:5]).all()


@pytest.mark.parametrize("n", SIZES)
def test_statistics_are_fh_score_rows(n):
    for kind in KINDS:
        x = logits_case(kind, n, seed=3 * n)
        chosen = n // 3
        got, sc = host_logprob(x, [chosen], 5), host_score(x, [chosen])
        for a, b in (("max_logit", "max_logit"), ("sum", "sum"), ("logit", "target_logit")):
            assert got[a].view(np.uint32)[0] == sc[b].view(np.uint32)[0], (n, kind, a)


def test_logprob_values_sum_to_one():
    """exp(logprob) over the whole row, from top_n = n at n <= 20, on a row nothing of which is clipped: checks the formula, not the kernel"""
    for n in (2, 7, 20):
        x = (np.random.default_rng(n).standard_normal(n) * 2).astype(np.float32)
        assert float(x.max() - x.min()) < 15
        rec = host_logprob(x, [n - 1], n)
        lp, top = capi.logprob_values(rec)
        # the formula is exact in double; what is left is `sum` itself, an fp32 chain of fp32 expf values: each term within an ulp (2^-23 relative) of exp(d), each of the
        # n - 1 additions rounding by at most 2^-24 relative -- the bound follows from the formats, not from what the code gives
        assert abs(np.exp(top[0, :n]).sum() - 1.0) <= (n + 1) * 2.0 ** -23
        assert np.isnan(top[0, n:]).all()
        j = rec["top_id"][0, :n].tolist().index(n - 1)
        assert lp[0] == top[0, j]
    x = np.array([1.0, -np.inf, 0.5], np.float32)
    lp, top = capi.logprob_values(host_logprob(x, [1], 3))
    assert lp[0] == -np.inf and top[0, 2] == -np.inf and np.isfinite(top[0, :2]).all()


def test_abi_layout():
    class Rec(C.Structure):
        _fields_ = [("token", C.c_int32), ("logit", C.c_float), ("max_logit", C.c_float), ("sum", C.c_float), ("n_top", C.c_int32),
                    ("top_id", C.c_int32 * NMAX), ("top_logit", C.c_float * NMAX), ("pad_", C.c_int32 * 3)]
    assert C.sizeof(Rec) == 192 and capi.LOGPROB_DTYPE.itemsize == 192 and NMAX == 20
    lay = (C.c_int * 9)()
    host_lib().fh_logprob_layout(lay)
    names = ("token", "logit", "max_logit", "sum", "n_top", "top_id", "top_logit", "pad_")
    assert lay[0] == 192
    assert [lay[1 + i] for i in range(8)] == [capi.LOGPROB_DTYPE.fields[f][1] for f in names] == [getattr(Rec, f).offset for f in names]
