"""bin/main --mode score on tests/golden/hf_tiny_int8.flm: the per-position lines (index, token id, argmax id, prob) parsed back equal Ctx.score on the ids the CLI's
own -e prints, and the summary line carries the mean loss and perplexity of those rows."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

import __graft_entry__ as graft
from fast_llama_amd import capi, flmfile as ff

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
MAIN = os.path.join(graft.PKG_DIR, "bin", "main")
PROMPT = "Once upon a time there was a small village among the mountains"


def test_cli_score_mode_matches_the_binding(gpu):
    path = os.path.join(GOLD, "hf_tiny_int8.flm")
    if not os.path.exists(MAIN):
        graft.build()
    enc = subprocess.run([MAIN, "-c", path, "-e", PROMPT], capture_output=True, text=True, timeout=120)
    assert enc.returncode == 0, enc.stderr
    ids = [int(x) for x in re.search(r"tokens: \[(.*)\]", enc.stdout).group(1).split(",")]
    assert len(ids) >= 6
    r = subprocess.run([MAIN, "-c", path, "-j", "1", "--mode", "score", "-i", PROMPT], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    rows = re.findall(r"^score:\s*(\d+)\ttoken:\s*(-?\d+)\targmax:\s*(-?\d+)\tprob:(\S+)$", r.stdout, re.M)
    assert [int(a) for a, _, _, _ in rows] == list(range(len(ids))) and [int(t) for _, t, _, _ in rows] == ids
    cfg, _, tensors = ff.read_flm(path)
    ctx = gpu.Ctx(gpu.desc_from_config(cfg, max_seq_len=1024)); ctx.upload_all(tensors)     # (the CLI's context length)
    want = ctx.score(np.array(ids, np.int32), 0)
    ctx.close()
    assert [int(a) for _, _, a, _ in rows] == [int(x) for x in want["argmax"]]
    got_prob = np.array([float(p) for _, _, _, p in rows], np.float64).astype(np.float32)       # (%.9g round-trips an fp32)
    assert np.array_equal(got_prob.view(np.uint32), want["prob"].view(np.uint32))
    m = re.search(r"^score_tokens:\s*(\d+)\tmean_loss:(\S+)\tperplexity:(\S+)\tscore_latancy:\s*(\S+)ms$", r.stdout, re.M)
    assert m and int(m.group(1)) == len(ids)
    _, mean = capi.nll(want)
    assert float(m.group(2)) == pytest.approx(mean, abs=1e-6) and float(m.group(3)) == pytest.approx(math.exp(mean), rel=1e-4)
    # the reference's summary line belongs to the other modes
    assert "total_latancy" not in r.stdout
