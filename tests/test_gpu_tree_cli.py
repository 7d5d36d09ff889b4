"""bin/main -t 0 --lookup K,G,2: the prompt-lookup drafter's tree (option "spec_branches") prints the text of the run without --lookup."""
import os
import subprocess

import pytest

import __graft_entry__ as graft
from fast_llama_amd import flmfile as ff, synth

MAIN = os.path.join(graft.PKG_DIR, "bin", "main")


@pytest.mark.gpu
def test_lookup_with_two_branches_prints_the_same_text(gpu, tmp_path):
    path = str(tmp_path / "tiny.flm")
    synth.write_synthetic_flm(path, synth.make_config("tiny", ff.QT_INT8), seed=1)

    def run(*extra):
        r = subprocess.run([MAIN, "-c", path, "-j", "1", "-n", "40", "-i", "so on and so on and on and so", "-t", "0", *extra], capture_output=True, timeout=300)
        assert r.returncode == 0, r.stderr.decode(errors="replace")
        body = r.stdout[r.stdout.index(b"output: \x1b[32m") + len(b"output: \x1b[32m"):]
        return body[:body.index(b"\x1b[0m\n\n")], r.stdout
    plain, _ = run()
    tree, out = run("--lookup", "7,3,2")
    assert tree == plain and len(plain) > 0 and b"lookup:7,3" in out
    r = subprocess.run([MAIN, "-c", "/nonexistent/model.flm", "--lookup", "7,3,5"], capture_output=True, timeout=60)
    assert r.returncode != 0 and b"Invalid --lookup" in r.stderr
