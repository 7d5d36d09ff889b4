"""The prompt-lookup drafter of flm_generate_lookup, host side: capi.spec_draft_host (host/spec_draft.h through libflm_host.so) against a restatement of the rule
in Python, and the rule's hand cases.  No GPU.  tests/test_gpu_spec.py compares the device's drafter kernel with spec_draft_host on the same histories."""
import numpy as np
import pytest

from fast_llama_amd import capi


def draft_rule(h, k, ngram_max):
    """include/flm_gpu.h, flm_generate_lookup: longest n-gram first, the latest match of it, continued periodically"""
    h = list(h); n = len(h)
    for g in range(min(ngram_max, n - 1), 0, -1):
        js = [j for j in range(0, n - g) if h[j:j + g] == h[n - g:]]
        if js:
            p = n - g - max(js)
            d = []
            for i in range(k):
                d.append(h[n - p + i] if i < p else d[i - p])
            return d
    return [h[-1]] * k


def histories():
    """seeded random histories over 3 symbols (matches are dense): every length 1 .. 64 -> (history, ngram_max, k)"""
    rng = np.random.default_rng(20240607)
    for n in range(1, 65):
        h = rng.integers(0, 3, n).astype(np.int32)
        for g in range(1, 9):
            for k in (4, 15):
                yield h, g, k


def test_host_drafter_is_the_rule():
    cases = 0
    for h, g, k in histories():
        got = capi.spec_draft_host(h, k, g)
        assert list(got) == draft_rule(h, k, g), (list(h), g, k, list(got))
        cases += 1
    assert cases == 64 * 8 * 2


@pytest.mark.parametrize("k", [4, 15])
def test_no_match_repeats_the_last_token(k):
    for h in ([7], [1, 2, 3, 4], [5, 6, 7, 8, 9, 10, 11]):
        assert list(capi.spec_draft_host(h, k, 3)) == [h[-1]] * k


def test_period_shorter_than_k_continues_periodically():
    # ... 1 2 3 | 1 2 3: the 3-gram matches one period back, p = 3 < k
    h = [9, 1, 2, 3, 1, 2, 3]
    assert list(capi.spec_draft_host(h, 8, 3)) == [1, 2, 3, 1, 2, 3, 1, 2]
    # a run of one symbol: period 1
    assert list(capi.spec_draft_host([4, 5, 5, 5], 5, 2)) == [5] * 5


def test_of_two_matches_the_later_wins():
    # the 1-gram [1] occurs at 0 (followed by 2) and at 3 (followed by 8): the later one, p = 2, drafts 8 1 8 1
    h = [1, 2, 0, 1, 8, 1]
    assert list(capi.spec_draft_host(h, 4, 1)) == [8, 1, 8, 1]
    assert draft_rule(h, 4, 1) == [8, 1, 8, 1]


def test_a_longer_ngram_wins_over_a_later_shorter_one():
    # suffix (1, 2): the 2-gram matches at 0 (then 7 ...); the 1-gram [2] also matches later, at 5 (then 9 ...).  g = 2 is tried first
    h = [1, 2, 7, 7, 3, 2, 9, 1, 2]
    assert list(capi.spec_draft_host(h, 4, 2)) == [7, 7, 3, 2]
    assert list(capi.spec_draft_host(h, 4, 1)) == [9, 1, 2, 9]
