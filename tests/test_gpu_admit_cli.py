"""bin/main --prompts FILE --batch-rows N: the prompts enter inside the steps' passes (option "batch_rows", flm_batch_admit / flm_batch_pass) and the run prints what
the run without --batch-rows prints, byte for byte."""
import os

import pytest

import __graft_entry__ as graft
from fast_llama_amd import flmfile as ff, synth
from test_gpu_batch_cli import MAIN, PROMPTS, _run, _split

pytestmark = pytest.mark.gpu


def test_batch_rows_prints_what_the_run_without_it_prints(gpu, tmp_path):
    path = str(tmp_path / "tiny.flm")
    synth.write_synthetic_flm(path, synth.make_config("tiny", ff.QT_INT8), seed=1)
    if not os.path.exists(MAIN):
        graft.build()
    file = tmp_path / "prompts.txt"
    file.write_text("\n".join(PROMPTS) + "\n")
    plain = _run(path, "--prompts", str(file), "--seed", "5")
    texts, _ = _split(plain, b"prompt")
    assert len(texts) == len(PROMPTS) and len(set(texts)) > 1, "every prompt gave the same text: the case shows nothing"
    for rows in ("8", "0", "3"):
        assert _run(path, "--prompts", str(file), "--seed", "5", "--batch-rows", rows) == plain, rows
