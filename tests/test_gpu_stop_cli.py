"""bin/main's stop rules (--stop-ids, --stop-seq, --stop): the transcript ends at the index the host matcher gives and the finish reason is printed; a malformed value is a
usage error before any model is loaded (that part needs no GPU).  The tiny .flm of model seed 1 (tests/test_gpu_shape.py's CLI model): its greedy ids behind the prompt
below, looked at on the CPU oracle, hold no token 0 in 25, repeat the pair ids[3:5] at 10, and first show ids[12] there -- the tests assert what they rely on."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import __graft_entry__ as graft
from fast_llama_amd import capi, flmfile as ff, synth
from stop_util import ID, LENGTH, SEQ

MAIN = os.path.join(graft.PKG_DIR, "bin", "main")
PROMPT = "hello world and so on"


@pytest.mark.parametrize("flags", [["--stop-ids", "1,,2"], ["--stop-ids", "x"], ["--stop-ids", "3,-4"], ["--stop-ids", "5,5"], ["--stop-ids", ",".join(str(i) for i in range(65))],
                                   ["--stop-ids", "7", "--stop-ids", "7"], ["--stop-seq", ""], ["--stop-seq", "1,2,"], ["--stop-seq", ",".join(["1"] * 33)], ["--stop", ""],
                                   ["--stop-seq", "1"] * 17, ["--stop-seq", "1 2"]])
def test_a_malformed_value_is_a_usage_error_before_any_model_is_loaded(flags):
    r = subprocess.run([MAIN, "-c", "/nonexistent/model.flm", *flags], capture_output=True, timeout=60)
    assert r.returncode != 0
    assert b"Invalid stop rule" in r.stderr and b"Usage:" in r.stderr and b"Failed to load model" not in r.stderr, r.stderr


def test_stop_flags_are_refused_on_several_devices():
    r = subprocess.run([MAIN, "-c", "/nonexistent/model.flm", "--devices", "0,1", "--stop-ids", "2"], capture_output=True, timeout=60)
    assert r.returncode != 0 and b"one device only" in r.stderr and b"Failed to load model" not in r.stderr, r.stderr


@pytest.mark.gpu
def test_transcripts_end_where_the_host_matcher_says(gpu, tmp_path):
    cfg = synth.make_config("tiny", ff.QT_INT8)
    path = str(tmp_path / "tiny.flm")
    tensors = synth.write_synthetic_flm(path, cfg, seed=1)
    H = C.CDLL(os.path.join(graft.PKG_DIR, "lib", "libflm_host.so"))
    H.fh_open.restype = C.c_void_p
    H.fh_open.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_int]
    H.fh_decode_one.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_char_p, C.c_int]
    H.fh_encode.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.c_void_p, C.c_int]
    H.fh_close.argtypes = [C.c_void_p]
    h = H.fh_open(path.encode(), b"", 0, 1)
    assert h

    def text_of(ids):
        out, prev, buf = b"", -1, C.create_string_buffer(256)
        for t in ids:
            H.fh_decode_one(h, int(t), prev, buf, 256)
            out += buf.value; prev = int(t)
        return out

    def encode(text):
        buf = (C.c_int * 64)()
        n = H.fh_encode(h, text.encode(), 0, buf, 64)
        return [int(x) for x in buf[:n]]

    def run(*extra, mode=None):
        cmd = [MAIN, "-c", path, "-j", "1", "-n", "24", "-i", PROMPT, "-t", "0", *extra] + (["--mode", mode, "--rounds", "1"] if mode else [])
        r = subprocess.run(cmd, capture_output=True, timeout=300)
        assert r.returncode == 0, r.stderr.decode(errors="replace")
        prompt = [int(x) for x in re.search(rb"Input tokens:\[([^\]]*)\]", r.stdout).group(1).replace(b",", b" ").split()]
        fin = re.search(rb"finish_reason:(\w+)\trule:(\d+)\toutput_size:(\d+)", r.stdout)
        if mode:
            return prompt, None, fin
        body = r.stdout[r.stdout.index(b"output: \x1b[32m") + len(b"output: \x1b[32m"):]
        return prompt, body[:body.index(b"\x1b[0m\n\n")], fin

    prompt, plain_text, fin = run()
    assert fin is None                                               # (no stop flag, not --mode test: the transcript is what it was)
    assert run(mode="bm")[2] is None                                 # (the benchmark mode's own spellings print what they always did)
    fin = run(mode="test")[2]
    assert fin and fin.group(1) == b"length" and int(fin.group(2)) == 0
    ctx = gpu.Ctx(gpu.desc_from_config(cfg, max_seq_len=1024)); ctx.upload_all(tensors)
    plain = [int(x) for x in ctx.generate(np.array(prompt, np.int32), 0, 25, stop_token=0)[0]]
    ctx.close()
    assert len(plain) == 25 and 0 not in plain and plain_text == text_of(plain)
    assert plain[12] not in plain[:12] and plain[10:12] == plain[3:5], plain
    names = {LENGTH: b"length", ID: b"stop_id", SEQ: b"stop_seq"}
    never = [t for t in range(cfg.vocab_size - 1, 0, -1) if t not in plain][:2]
    word = encode(" so on")
    assert 1 <= len(word) <= 32
    cases = [
        (["--stop-ids", f"{never[0]},{plain[12]}"], capi.StopRules([never[0], plain[12]]), (12, ID, 1)),
        (["--stop-seq", f"{never[1]},{never[0]}", "--stop-seq", ",".join(str(t) for t in plain[10:13])], capi.StopRules([], [[never[1], never[0]], plain[10:13]]), (12, SEQ, 1)),
        (["--stop-ids", str(never[0]), "--stop-seq", f"{plain[5]},{never[1]}"], capi.StopRules([never[0]], [[plain[5], never[1]]]), (25, LENGTH, 0)),
        (["--stop", " so on"], capi.StopRules([], [word]), None),      # one tokenisation, matched token by token: wherever the host matcher says, if anywhere
    ]
    for flags, rules, want in cases:
        first, kind, rule = capi.stop_match_host(rules, plain, 0)
        assert want is None or (first, kind, rule) == want, (flags, first, kind, rule)
        n = min(first + 1, 25)
        p2, text, fin = run(*flags)
        assert p2 == prompt and text == text_of(plain[:n]), (flags, text)
        assert fin and fin.group(1) == names[kind] and int(fin.group(2)) == rule, (flags, fin and fin.group(0))
        _, _, fin = run(*flags, mode="test")
        assert fin and fin.group(1) == names[kind] and int(fin.group(2)) == rule, (flags, fin and fin.group(0))
    H.fh_close(h)
