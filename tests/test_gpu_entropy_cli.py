"""bin/main --typical / --mirostat on the device: the text is the host loop's ids decoded (tests/entropy_util.py host_loop on flm_forward's logits).  The CLI's sampler
state is the reference's -- 0 whatever --seed says, so every coin is 0: under --typical the draw is the first maximum of the masked row, under --mirostat (multinomial) the
first kept entry, and mu still follows every id."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import __graft_entry__ as graft
from fast_llama_amd import flmfile as ff, synth
from entropy_util import Entropy, host_loop
from sample_util import host_lib
from shape_util import Sampling

pytestmark = pytest.mark.gpu
MAIN = os.path.join(graft.PKG_DIR, "bin", "main")


@pytest.fixture(scope="module")
def rig(gpu, tmp_path_factory):
    cfg = synth.make_config("tiny", ff.QT_INT8)
    path = str(tmp_path_factory.mktemp("flm") / "tiny.flm")
    tensors = synth.write_synthetic_flm(path, cfg, seed=1)
    H = C.CDLL(os.path.join(graft.PKG_DIR, "lib", "libflm_host.so"))
    H.fh_open.restype = C.c_void_p
    H.fh_open.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_int]
    H.fh_decode_one.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_char_p, C.c_int]
    H.fh_close.argtypes = [C.c_void_p]
    h = H.fh_open(path.encode(), b"", 0, 1)
    assert h
    ctx = gpu.Ctx(gpu.desc_from_config(cfg, max_seq_len=1024)); ctx.upload_all(tensors)

    def text_of(ids):
        out, prev, buf = b"", -1, C.create_string_buffer(256)
        for t in ids:
            H.fh_decode_one(h, int(t), prev, buf, 256)
            out += buf.value; prev = int(t)
        return out

    def run(*extra):
        r = subprocess.run([MAIN, "-c", path, "-j", "1", "-n", "24", "-i", "hello world and so on", "--seed", "7", "-t", "1", "-p", "0.9", *extra], capture_output=True, timeout=300)
        assert r.returncode == 0, r.stderr.decode(errors="replace")
        prompt = [int(x) for x in re.search(rb"Input tokens:\[([^\]]*)\]", r.stdout).group(1).replace(b",", b" ").split()]
        body = r.stdout[r.stdout.index(b"output: \x1b[32m") + len(b"output: \x1b[32m"):]
        return prompt, body[:body.index(b"\x1b[0m\n\nnum_threads")]
    yield ctx, text_of, run
    ctx.close(); H.fh_close(h)


def _cut(ids):       # the CLI stops on token 0 (delivered)
    return ids[:ids.index(0) + 1] if 0 in ids else ids


@pytest.mark.parametrize("flags,ent", [(("--typical", "0.5"), Entropy(typical_p=0.5)),
                                       (("--mirostat", "2"), Entropy(mirostat=2)),
                                       (("--mirostat", "2", "--mirostat-ent", "3", "--mirostat-lr", "0.25"), Entropy(mirostat=2, tau=3.0, eta=0.25))])
def test_cli_flags_give_the_host_loops_text(rig, flags, ent):
    ctx, text_of, run = rig
    prompt, text = run(*flags)
    want = host_loop(ctx, host_lib(), np.array(prompt, np.int32), 25, Sampling(temperature=1.0, topp=0.9), ent, 0, stop=0)[0]
    assert text == text_of(_cut(want)) and len(text) > 0
