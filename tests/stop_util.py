"""Shared pieces of the stop-rule tests (tests/test_stop_host.py, tests/test_gpu_stop.py, tests/test_gpu_stop_cli.py): a Python restatement of the definition in
include/flm_gpu.h (flm_stop_rules: "when a rule fires"), written from the text and independent of host/stop_rules.h, and the seeded streams both suites compare on."""
import numpy as np

LENGTH, TOKEN, ID, SEQ, CANCEL = 0, 1, 2, 3, 4      # FLM_STOP_LENGTH .. FLM_STOP_CANCEL


def py_fires_at(ids, seqs, stop_token, t, i):
    """does index i of the delivered ids t fire? -> (kind, rule) or None; kinds preferred 1, 2, 3; the lowest position / sequence"""
    if stop_token >= 0 and t[i] == stop_token:
        return TOKEN, 0
    ids = list(ids)
    if t[i] in ids:
        return ID, ids.index(t[i])
    for s, q in enumerate(seqs):
        L = len(q)
        if L <= i + 1 and list(t[i - L + 1:i + 1]) == list(q):
            return SEQ, s
    return None


def py_stop_match(ids, seqs, stop_token, t):
    """-> (the first index that fires or len(t), kind, rule)"""
    t = [int(x) for x in t]
    for i in range(len(t)):
        hit = py_fires_at(ids, seqs, stop_token, t, i)
        if hit:
            return i, hit[0], hit[1]
    return len(t), LENGTH, 0


# the seed of the 2000 streams, picked here on the CPU so that the restatement alone meets the suite's two conditions: between 30 % and 90 % of the streams fire, and at
# least 100 of them fire through a sequence at an index >= its length (test_stop_host.py asserts both)
STREAM_SEED = 20240611


def seeded_streams(count=2000, seed=STREAM_SEED):
    """`count` cases (ids, seqs, stop_token, stream): alphabets of 2 - 4 symbols, streams of 1 .. 48 ids, random rule sets.  Sequences are drawn long enough, and ids rare
    enough, that a good share of the streams runs for a while before something fires"""
    rng = np.random.default_rng(seed)
    cases = []
    for _ in range(count):
        A = int(rng.integers(2, 5))
        n = int(rng.integers(1, 49))
        t = [int(x) for x in rng.integers(0, A, n)]
        # ids: mostly none (an id of a 2 - 4 symbol alphabet fires almost at once); sometimes a symbol outside the alphabet that never occurs
        ids = []
        if rng.random() < 0.15:
            ids.append(int(rng.integers(0, A)))
        if rng.random() < 0.3:
            ids.append(A + int(rng.integers(0, 3)))
        seqs = []
        for _s in range(int(rng.integers(0, 4))):
            L = int(rng.integers(3, 9))
            seqs.append([int(x) for x in rng.integers(0, A, L)])
        stop_token = int(rng.integers(0, A)) if rng.random() < 0.05 else -1
        cases.append((ids, seqs, stop_token, t))
    return cases
