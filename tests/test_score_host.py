"""Scoring without a GPU: the host restatement of a flm_score row (host/test_shim.cpp fh_score_row -- the expected value of the device tests) against an independent
NumPy / ctypes-libm evaluation of the specification in include/flm_gpu.h, the binding's surface, and capi.nll on hand-made rows."""
import math
import os
import re

import numpy as np
import pytest

from fast_llama_amd import capi
from sample_util import logits_case, teeth_logits
from score_util import FIELDS, clipped_terms, diff_scores, host_score, numpy_score, same_scores, teeth_row, tree_sum

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = ("peaked", "medium", "flat", "ties", "clip", "neginf")


def _targets(x):
    """the first maximum, a later copy of it (if any), an entry at exactly d = -15, one just past it (if the row has them), the last index, none"""
    x = np.asarray(x, np.float32)
    mx = x.max()
    tg = [int(np.argmax(x)), int(np.nonzero(x == mx)[0][-1]), x.size - 1, -1]
    d = x - mx
    for v in (np.float32(-15.0), np.nextafter(np.float32(-15.0), np.float32(-np.inf))):
        hit = np.nonzero(d == v)[0]
        if hit.size:
            tg.append(int(hit[0]))
    return tg


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", [2, 320, 323, 2003])
def test_host_restatement_matches_numpy_and_libm(kind, n):
    x = logits_case(kind, n, seed=7)
    for tg in _targets(x):
        got, want = host_score(x, [tg]), numpy_score(x, tg)
        assert same_scores(got, want), (kind, n, tg, diff_scores(got, want), got, want)


def test_host_restatement_clip_edge_and_ties_by_hand():
    """d = -15 exactly is kept (expf(-15)), the next float below is clipped to 0 with prob exactly 0; the first of two maxima is the argmax"""
    below = np.nextafter(np.float32(-15.0), np.float32(-np.inf))
    x = np.array([-15.0, 0.0, below, 0.0, -3.0], np.float32)
    r = host_score(np.tile(x, (4, 1)), [0, 2, 3, -1])
    assert list(r["argmax"]) == [1, 1, 1, 1] and np.all(r["max_logit"] == 0.0)
    e15, e3 = np.float32(math.exp(-15.0)), np.float32(math.exp(-3.0))
    want_sum = np.float32(np.float32(np.float32(np.float32(e15 + np.float32(1)) + np.float32(1))) + e3)       # index order; the clipped entry adds nothing
    assert np.all(r["sum"] == want_sum)
    assert r["prob"][0] > 0 and r["target_logit"][0] == np.float32(-15.0)
    assert r["prob"][1] == 0.0 and r["target_logit"][1] == below
    assert r["prob"][2] == np.float32(np.float32(1) * np.float32(1.0 / float(want_sum)))
    assert r["prob"][3] == 0.0 and r["target_logit"][3] == 0.0


def test_sequential_sum_is_what_the_restatement_computes():
    """exact terms (sample_util.teeth_logits: every exponential 1 or 0): the sum is the count of maxima.  Inexact terms (score_util.teeth_row): the restatement's sum is
    the sequential fp32 chain in index order, and a pairwise sum of the same terms is another number there -- the case the device test uses"""
    x = teeth_logits(0)
    assert host_score(x)["sum"][0] == np.float32(np.count_nonzero(x == 0.0))
    y = teeth_row(0)
    e = clipped_terms(y)
    seq = np.float32(0)
    for v in e:
        seq = np.float32(seq + v)
    assert host_score(y)["sum"][0].view(np.uint32) == seq.view(np.uint32)
    assert tree_sum(e) != seq


def test_nll_on_hand_made_rows():
    s = np.zeros(4, dtype=capi.SCORE_DTYPE)
    # a certain token; one of two equal ones; a clipped target (prob 0, loss finite); a row without a target
    s["target_logit"] = [2.0, 1.0, -30.0, 0.0]; s["max_logit"] = [2.0, 1.0, 0.0, 5.0]; s["sum"] = [1.0, 2.0, 1.5, 3.0]; s["prob"] = [1.0, 0.5, 0.0, 0.0]
    loss, mean = capi.nll(s)
    want = [0.0, math.log(2.0), 30.0 + math.log(1.5)]
    assert loss.dtype == np.float64 and np.isnan(loss[3])
    assert np.allclose(loss[:3], want, rtol=0, atol=1e-15) and math.isfinite(loss[2]) and s["prob"][2] == 0.0
    assert mean == pytest.approx(sum(want) / 3, rel=1e-14)
    loss2, mean2 = capi.nll(s, targets=[5, -1, 7, 9])
    assert np.isnan(loss2[1]) and loss2[3] == pytest.approx(5.0 + math.log(3.0), abs=1e-15)
    assert mean2 == pytest.approx((want[0] + want[2] + 5.0 + math.log(3.0)) / 3, rel=1e-14)        # (a double mean of three terms: a few units in the last place)
    # where nothing is clipped the loss is -log(prob) up to the roundings of prob's fp32 evaluation
    x = logits_case("flat", 320, seed=3)
    r = host_score(x, [17])
    assert capi.nll(r, targets=[17])[0][0] == pytest.approx(-math.log(float(r["prob"][0])), rel=1e-5)


def test_score_surface_is_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "flm_gpu.h")).read()
    m = re.search(r"typedef struct flm_score \{([^}]*)\} flm_score;", hdr)
    assert m and [w.strip(" ,;") for w in re.findall(r"\b(\w+)\s*[,;]", m.group(1))] == list(FIELDS)
    assert capi.SCORE_DTYPE.names == FIELDS and capi.SCORE_DTYPE.itemsize == 20
    lib = capi.lib()
    for sym in ("flm_score_tokens", "flm_op_score_rows"):
        assert sym in capi.SYMBOLS and hasattr(lib, sym) and sym in hdr
    assert lib.flm_score_tokens(None, None, 1, 0, None, None, None) != 0
    assert lib.flm_op_score_rows(None, 1, 2, None, None) != 0
    assert callable(capi.Ctx.score) and callable(capi.op_score_rows)
