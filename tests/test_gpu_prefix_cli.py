"""bin/main --prompts FILE --system TEXT: every line of the file continues TEXT, which enters the cache once (flm_forward) with the lines served behind it
(flm_generate_batch_prefix).  Each completion is compared with the CLI's own single run of the whole text: `-i <TEXT + line> --samples 1 --seed <seed + j>`."""
import os

import pytest

import __graft_entry__ as graft
from fast_llama_amd import flmfile as ff, synth
from test_gpu_batch_cli import MAIN, PROMPTS, _run, _split

pytestmark = pytest.mark.gpu
SYSTEM = "you are a careful helper and answer briefly."      # (ends in a token no vocabulary piece merges with: the lines' tokens continue the text's)


@pytest.mark.parametrize("extra", [[], ["--batch-rows", "8"]], ids=["joins", "passes"])
def test_lines_continue_the_system_text(gpu, tmp_path, extra):
    path = str(tmp_path / "tiny.flm")
    synth.write_synthetic_flm(path, synth.make_config("tiny", ff.QT_INT8), seed=1)
    if not os.path.exists(MAIN):
        graft.build()
    file = tmp_path / "prompts.txt"
    file.write_text("\n".join(PROMPTS) + "\n")
    texts, _ = _split(_run(path, "--prompts", str(file), "--system", SYSTEM, "--seed", "5", *extra), b"prompt")
    assert len(texts) == len(PROMPTS)
    for j, p in enumerate(PROMPTS):
        single, _ = _split(_run(path, "-i", SYSTEM + p, "--samples", "1", "--seed", str(5 + j)), b"sample")
        assert single == [texts[j]], (j, single, texts[j])
    assert len(set(texts)) > 1, "every prompt gave the same text: the case shows nothing"
