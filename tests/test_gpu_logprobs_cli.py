"""bin/main --logprobs N[,shaped] on tests/golden/hf_tiny_int8.flm: after the text one line per generated token, `index id logprob | id:logprob ...`, whose ids and %.9g values
equal what the binding returns for the same arguments; the text and the ids in front are those of a run without the flag."""
import os
import re
import subprocess

import numpy as np
import pytest

import __graft_entry__ as graft
from fast_llama_amd import capi, flmfile as ff

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
MAIN = os.path.join(graft.PKG_DIR, "bin", "main")
PROMPT = "Once upon a time there was a small village among the mountains"
N_NEW = 24


def _run(*extra):
    r = subprocess.run([MAIN, "-c", os.path.join(GOLD, "hf_tiny_int8.flm"), "-j", "1", "-t", "1", "-p", "0.9", "-n", str(N_NEW), "-i", PROMPT, *extra], capture_output=True, timeout=300)
    assert r.returncode == 0, r.stderr.decode(errors="replace")
    out = r.stdout
    prompt = [int(x) for x in re.search(rb"Input tokens:\[([^\]]*)\]", out).group(1).replace(b",", b" ").split()]
    at = out.index(b"output: \x1b[32m") + len(b"output: \x1b[32m")
    end = out.index(b"\x1b[0m\n\n", at)
    tail = out[end + len(b"\x1b[0m\n\n"):out.index(b"num_threads", end)].decode()
    return prompt, out[at:end], [ln for ln in tail.split("\n") if ln]


def _fmt(v):
    return "%.9g" % v


@pytest.mark.parametrize("extra,source,ctl", [(("--logprobs", "3"), "raw", {}), (("--logprobs", "3,shaped", "--top-k", "5"), "shaped", dict(top_k=5))])
def test_cli_lines_equal_the_binding(gpu, extra, source, ctl):
    if not os.path.exists(MAIN):
        graft.build()
    flags = tuple(x for x in extra if x not in ("--logprobs", "3", "3,shaped"))
    prompt, text, lines = _run(*extra)
    prompt0, text0, lines0 = _run(*flags)
    assert prompt0 == prompt and text0 == text and lines0 == [] and len(text) > 0
    cfg, _, tensors = ff.read_flm(os.path.join(GOLD, "hf_tiny_int8.flm"))
    ctx = gpu.Ctx(gpu.desc_from_config(cfg, max_seq_len=1024)); ctx.upload_all(tensors)     # (the CLI's context length)
    ctx.logprobs_arm(3, source)
    s = capi.Sampling(temperature=1.0, topp=0.9, penalty_last_n=64 if ctl else 0, **ctl)
    ids, _ = ctx.generate_ex(np.array(prompt, np.int32), 0, N_NEW + 1, s, rng_state=0, stop_token=0)       # (the CLI's sampler state is the reference's: 0)
    rec = ctx.last_logprobs()
    ctx.close()
    lp, top = capi.logprob_values(rec)
    want = []
    for i in range(len(ids)):
        alts = " ".join(f"{int(rec['top_id'][i, j])}:{_fmt(top[i, j])}" for j in range(int(rec["n_top"][i])))
        want.append(f"{i} {int(ids[i])} {_fmt(lp[i])} |" + (" " + alts if alts else ""))
    assert lines == want and len(lines) == len(ids) >= 1


def test_cli_refuses_logprobs_with_several_devices():
    if not os.path.exists(MAIN):
        graft.build()
    r = subprocess.run([MAIN, "-c", "/nonexistent.flm", "--logprobs", "3", "--devices", "0,0"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "--logprobs applies to one device only" in r.stderr
    r = subprocess.run([MAIN, "-c", "/nonexistent.flm", "--logprobs", "21"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "Invalid --logprobs" in r.stderr
