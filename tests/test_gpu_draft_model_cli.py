"""bin/main --draft-model FILE prints the text of the run without the flag: at -t 0 and at the default temperature, with and without a control flag, on files written by
synth.write_synthetic_flm (the target: "tiny"; the draft: the same shape with one layer and another seed, same vocabulary and tokenizer).  The summary line gains the
draft model's accepted / steps."""
import os
import re
import subprocess

import pytest

import __graft_entry__ as graft
from fast_llama_amd import flmfile as ff, synth

pytestmark = pytest.mark.gpu
MAIN = os.path.join(graft.PKG_DIR, "bin", "main")
PROMPT = "hello world and so on"
FLAGS = ("--top-k", "5", "--repeat-penalty", "1.3", "--repeat-last-n", "8")


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("draft_model")
    cfg = synth.make_config("tiny", ff.QT_INT8)
    dcfg = synth.make_config("tiny", ff.QT_INT8, n_layers=1)
    vcfg = synth.make_config("tiny", ff.QT_INT8, n_layers=1, vocab_size=384)
    paths = {k: str(d / f"{k}.flm") for k in ("target", "draft", "vocab")}
    synth.write_synthetic_flm(paths["target"], cfg, seed=1)
    synth.write_synthetic_flm(paths["draft"], dcfg, seed=77)
    synth.write_synthetic_flm(paths["vocab"], vcfg, seed=78)
    return paths


def _main(files, *extra, ok=True):
    r = subprocess.run([MAIN, "-c", files["target"], "-j", "1", "-n", "32", "-i", PROMPT, *extra], capture_output=True, text=True, timeout=300)
    if ok:
        assert r.returncode == 0, r.stderr
    return r


def _text(out):
    return out[out.index("output: "):out.index("num_threads:")]


def test_cli_draft_model_prints_the_same_text(gpu, files):
    if not os.path.exists(MAIN):
        graft.build()
    size = lambda out: re.search(r"output_size:\s*(\d+)", out).group(1)
    plains = {}
    for temp, flags, k_flag, k in ((("-t", "0"), (), (), 7), (("-t", "0"), FLAGS, ("--draft", "4"), 4), ((), (), ("--draft", "4"), 4), ((), FLAGS, (), 7)):      # () = the default temperature (1.0, top-p 0.9)
        plain = plains[(temp, flags)] = _main(files, *temp, *flags)
        got = _main(files, *temp, *flags, "--draft-model", files["draft"], *k_flag)
        assert _text(got.stdout) == _text(plain.stdout) and len(_text(plain.stdout)) > len("output: "), (temp, flags, k)
        assert size(got.stdout) == size(plain.stdout)
        m = re.search(r"draft_model:%d\taccepted/steps:(?:\x1b\[\d+m)?(\d+)/(\d+)" % k, got.stdout)
        assert m and int(m.group(2)) >= 1, got.stdout[-400:]          # verify passes ran: the flag was not ignored
        assert "ignored" not in got.stderr and "draft_model:" not in plain.stdout
    # the target as its own draft accepts drafts; the text stands
    plain, own = plains[(("-t", "0"), ())], _main(files, "-t", "0", "--draft-model", files["target"])
    assert _text(own.stdout) == _text(plain.stdout)
    m = re.search(r"draft_model:7\taccepted/steps:(?:\x1b\[\d+m)?(\d+)/(\d+)", own.stdout)
    assert m and int(m.group(1)) > int(m.group(2)) >= 1, own.stdout[-400:]
    # the control flags matter on this model, or equal text under them shows nothing
    assert _text(plains[(("-t", "0"), FLAGS)].stdout) != _text(plain.stdout)


def test_cli_draft_model_errors_are_clean(gpu, files):
    r = _main(files, "--draft-model", files["draft"] + ".missing", ok=False)
    assert r.returncode != 0 and "Invalid --draft-model file" in r.stderr and "output: " not in r.stdout
    r = _main(files, "--draft-model", files["vocab"], ok=False)
    assert r.returncode == 1 and "Failed to load the draft model" in r.stderr and "vocabular" in r.stderr
