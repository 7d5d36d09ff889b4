"""bin/main -t 0 --lookup 7 on tests/golden/hf_tiny_int8.flm prints the text bin/main -t 0 prints; the summary line gains the lookup's accepted / steps."""
import os
import re
import subprocess

import pytest

import __graft_entry__ as graft

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
MAIN = os.path.join(graft.PKG_DIR, "bin", "main")
PROMPT = "Once upon a time there was a small village among the mountains. Once upon a time there was a small village among the mountains."


def _run(*extra):
    r = subprocess.run([MAIN, "-c", os.path.join(GOLD, "hf_tiny_int8.flm"), "-j", "1", "-t", "0", "-n", "48", "-i", PROMPT, *extra], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return r


def test_cli_lookup_prints_the_same_text(gpu):
    if not os.path.exists(MAIN):
        graft.build()
    plain, look = _run(), _run("--lookup", "7")
    text = lambda out: out[out.index("output: "):out.index("num_threads:")]
    assert text(look.stdout) == text(plain.stdout) and len(text(plain.stdout)) > len("output: ")
    m = re.search(r"lookup:7,3\taccepted/steps:(?:\x1b\[\d+m)?(\d+)/(\d+)", look.stdout)
    assert m and int(m.group(2)) >= 1, look.stdout[-400:]
    assert "lookup:" not in plain.stdout
    size = lambda out: re.search(r"output_size:\s*(\d+)", out).group(1)
    assert size(look.stdout) == size(plain.stdout)
    # sampled generation ignores the switch, with a warning
    warn = subprocess.run([MAIN, "-c", os.path.join(GOLD, "hf_tiny_int8.flm"), "-j", "1", "-t", "0.8", "-n", "8", "-i", PROMPT, "--lookup", "7,2"], capture_output=True, text=True, timeout=300)
    assert warn.returncode == 0 and "--lookup applies to -t 0" in warn.stderr and "lookup:" not in warn.stdout
