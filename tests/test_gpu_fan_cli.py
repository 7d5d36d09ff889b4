"""bin/main --samples N: N completions of the prompt through flm_generate_n, printed one after another, each behind a line `--- sample j ---`; sample j runs with the
sampler state --seed + j.

Each sample is compared with two single runs at state seed + j:
  - `--samples 1 --seed <seed + j>`: one sequence through plain flm_generate with that state, the CLI's own single run;
  - independently of the CLI's sample code: the binding's generate(rng_state = seed + j) behind the tokens the CLI printed for the prompt, stop token 0, its ids decoded
    by the CLI's decode mode (`-d`).
A run WITHOUT --samples cannot serve: it keeps the reference CLI's behaviour, whose sampler state is 0 whatever --seed says (tests/test_gpu_entropy_cli.py relies on it),
so its text does not depend on the seed at all."""
import os
import re
import subprocess

import pytest

import __graft_entry__ as graft
from fast_llama_amd import flmfile as ff, synth

pytestmark = pytest.mark.gpu
MAIN = os.path.join(graft.PKG_DIR, "bin", "main")
PROMPT = "hello world and so on"


def _samples(path, *extra):
    r = subprocess.run([MAIN, "-c", path, "-j", "1", "-n", "16", "-i", PROMPT, "-t", "1", "-p", "0.9", *extra], capture_output=True, timeout=300)
    assert r.returncode == 0, r.stderr.decode(errors="replace")
    parts = re.split(rb"--- sample (\d+) ---\n", r.stdout)
    assert [int(x) for x in parts[1::2]] == list(range(len(parts) // 2)), r.stdout
    return [t[:-1] for t in parts[2::2]], parts[0]      # (every text ends with the newline main prints behind it)


def test_samples_are_the_single_runs_with_seed_plus_j(gpu, tmp_path):
    path = str(tmp_path / "tiny.flm")
    synth.write_synthetic_flm(path, synth.make_config("tiny", ff.QT_INT8), seed=1)
    if not os.path.exists(MAIN):
        graft.build()
    texts, head = _samples(path, "--samples", "3", "--seed", "5")
    assert len(texts) == 3 and b"prompt: " in head
    for j in range(3):
        single, _ = _samples(path, "--samples", "1", "--seed", str(5 + j))
        assert single == [texts[j]], (j, single, texts[j])
    assert len(set(texts)) > 1, "three states drew the same text: the case shows nothing"
    # the independent reference: the library's flm_generate on the prompt's tokens, decoded by the CLI's decode mode
    tokens = [int(x) for x in re.search(rb"Input tokens:\[([^\]]*)\]", head).group(1).split(b",")]
    cfg = synth.make_config("tiny", ff.QT_INT8)
    ctx = gpu.Ctx(gpu.desc_from_config(cfg)); ctx.upload_all(synth.make_tensors(cfg, seed=1))
    for j in range(3):
        ids, _ = ctx.generate(tokens, 0, 17, temperature=1.0, topp=0.9, rng_state=5 + j, stop_token=0)
        r = subprocess.run([MAIN, "-c", path, "-d", " ".join(str(int(x)) for x in ids)], capture_output=True, timeout=60)
        assert r.returncode == 0, r.stderr.decode(errors="replace")
        assert r.stdout.split(b"  text: ", 1)[1][:-1] == texts[j], (j, list(ids), r.stdout, texts[j])
    ctx.close()
    # not with this build's other extras: refused before a model is loaded
    r = subprocess.run([MAIN, "-c", path, "--samples", "3", "--top-k", "5"], capture_output=True, timeout=60)
    assert r.returncode != 0 and b"--samples applies to" in r.stderr
