"""bin/main --constraint FILE (this build only): the automaton of capi.Dfa.save, armed at state 0, masks every generated token -- at -t 0 and under --top-k 5 --draft 7 the
transcript is the text of the ids Ctx.generate_ex returns under the same automaton (the CLI's sampler state is the reference's: 0, and it stops on token 0); a malformed
file is a usage error before any model is loaded."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import __graft_entry__ as graft
from fast_llama_amd import flmfile as ff, synth
from constraint_util import Dfa
from shape_util import Sampling

pytestmark = pytest.mark.gpu
MAIN = os.path.join(graft.PKG_DIR, "bin", "main")


def test_cli_constraint_prints_generate_ex_ids(gpu, tmp_path):
    cfg = synth.make_config("tiny", ff.QT_INT8)
    path = str(tmp_path / "tiny.flm")
    tensors = synth.write_synthetic_flm(path, cfg, seed=1)
    V = cfg.vocab_size
    # cycle3 without the stop id 0 and the other control tokens: every id has text, and the run never stops early
    dfa = Dfa.from_edges(3, [(q, t, (q + 1) % 3) for q in range(3) for t in range(q, V, 3) if t >= 259])
    dpath = str(tmp_path / "cycle3.dfa")
    dfa.save(dpath)
    H = C.CDLL(os.path.join(graft.PKG_DIR, "lib", "libflm_host.so"))
    H.fh_open.restype = C.c_void_p
    H.fh_open.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_int]
    H.fh_decode_one.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_char_p, C.c_int]
    h = H.fh_open(path.encode(), b"", 0, 1)
    assert h

    def text_of(ids):
        out, prev, buf = b"", -1, C.create_string_buffer(256)
        for t in ids:
            H.fh_decode_one(h, int(t), prev, buf, 256)
            out += buf.value; prev = int(t)
        return out

    def run(*extra):
        r = subprocess.run([MAIN, "-c", path, "-j", "1", "-n", "24", "-i", "hello world and so on", "--seed", "7", *extra], capture_output=True, timeout=300)
        assert r.returncode == 0, r.stderr.decode(errors="replace")
        prompt = [int(x) for x in re.search(rb"Input tokens:\[([^\]]*)\]", r.stdout).group(1).replace(b",", b" ").split()]
        body = r.stdout[r.stdout.index(b"output: \x1b[32m") + len(b"output: \x1b[32m"):]
        return prompt, body[:body.index(b"\x1b[0m\n\nnum_threads")]

    ctx = gpu.Ctx(gpu.desc_from_config(cfg, max_seq_len=1024)); ctx.upload_all(tensors)
    ctx.constraint_set(dfa)
    for flags, s in ((("-t", "0"), Sampling(temperature=0.0)),
                     (("-t", "1", "-p", "0.9", "--top-k", "5", "--draft", "7"), Sampling(temperature=1.0, topp=0.9, top_k=5))):
        prompt, text = run("--constraint", dpath, *flags)
        ctx.reset_kv(); ctx.constraint_arm(0)
        want, _ = ctx.generate_ex(np.array(prompt, np.int32), 0, 25, s, rng_state=0, stop_token=0)
        assert len(want) == 25 and [int(x) % 3 for x in want] == [i % 3 for i in range(25)]
        assert text == text_of(want) and len(text) > 0, (flags, text, text_of(want))
        _, plain = run(*flags)
        assert plain != text                                                   # the flag changes the transcript
    ctx.close(); H.fh_close.argtypes = [C.c_void_p]; H.fh_close(h)


def test_cli_malformed_constraint_is_a_usage_error(gpu, tmp_path):
    bad = {"header": "flm-dfb 1 3\n0 1 1\n", "line": "flm-dfa 1 2\n0 1 1\n1 x 0\n", "state": "flm-dfa 1 2\n0 1 2\n1 1 0\n", "no edge": "flm-dfa 1 2\n0 5 1\n",
           "twice": "flm-dfa 1 1\n0 5 0\n0 5 0\n"}
    for name, body in bad.items():
        p = str(tmp_path / "bad.dfa")
        open(p, "w").write(body)
        r = subprocess.run([MAIN, "-c", str(tmp_path / "no-such-model.flm"), "-i", "x", "--constraint", p], capture_output=True, timeout=60)
        err = r.stderr.decode(errors="replace")
        assert r.returncode != 0 and "Invalid --constraint file" in err and "Failed to load model" not in err, (name, err[:300])
    r = subprocess.run([MAIN, "-c", str(tmp_path / "no-such-model.flm"), "-i", "x", "--constraint", str(tmp_path / "missing.dfa")], capture_output=True, timeout=60)
    assert r.returncode != 0 and b"Invalid --constraint file" in r.stderr
