"""bin/main --prompts FILE: the file's lines as independent prompts through flm_generate_batch, the completions printed in the file's order, each behind a line
`--- prompt j ---`; prompt j runs with the sampler state --seed + j.

Each completion is compared with the CLI's own single run of that prompt at that state: `-i <prompt> --samples 1 --seed <seed + j>` (one sequence through plain
flm_generate; a run WITHOUT --samples keeps the reference CLI's sampler state 0 whatever --seed says, so it cannot serve)."""
import os
import re
import subprocess

import pytest

import __graft_entry__ as graft
from fast_llama_amd import flmfile as ff, synth

pytestmark = pytest.mark.gpu
MAIN = os.path.join(graft.PKG_DIR, "bin", "main")
PROMPTS = ["hello world and so on", "a", "the quick brown fox jumps over the lazy dog and runs away", "once upon a time"]
COMMON = ["-j", "1", "-n", "16", "-t", "1", "-p", "0.9"]


def _run(path, *extra):
    r = subprocess.run([MAIN, "-c", path, *COMMON, *extra], capture_output=True, timeout=300)
    assert r.returncode == 0, r.stderr.decode(errors="replace")
    return r.stdout


def _split(out, word):
    parts = re.split(rb"--- " + word + rb" (\d+) ---\n", out)
    assert [int(x) for x in parts[1::2]] == list(range(len(parts) // 2)), out
    return [t[:-1] for t in parts[2::2]], parts[0]      # (every text ends with the newline main prints behind it)


def test_prompts_are_the_single_runs_with_seed_plus_j(gpu, tmp_path):
    path = str(tmp_path / "tiny.flm")
    synth.write_synthetic_flm(path, synth.make_config("tiny", ff.QT_INT8), seed=1)
    if not os.path.exists(MAIN):
        graft.build()
    file = tmp_path / "prompts.txt"
    file.write_text("\n".join(PROMPTS) + "\n")
    texts, head = _split(_run(path, "--prompts", str(file), "--seed", "5"), b"prompt")
    assert len(texts) == len(PROMPTS)
    tokens = re.findall(rb"Input tokens:\[([^\]]*)\]", head)
    assert len(tokens) == len(PROMPTS) and len({len(t.split(b",")) for t in tokens}) > 1      # prompts of different lengths
    for j, p in enumerate(PROMPTS):
        single, _ = _split(_run(path, "-i", p, "--samples", "1", "--seed", str(5 + j)), b"sample")
        assert single == [texts[j]], (j, single, texts[j])
    assert len(set(texts)) > 1, "every prompt gave the same text: the case shows nothing"
    # one line: the same single run
    one = tmp_path / "one.txt"
    one.write_text(PROMPTS[0])
    texts1, _ = _split(_run(path, "--prompts", str(one), "--seed", "5"), b"prompt")
    assert texts1 == [texts[0]]
