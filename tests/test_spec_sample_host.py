"""Sampled draft-and-verify without a GPU: flm_verify_sample, flm_generate_lookup_sample and flm_op_sample_rows are declared in include/flm_gpu.h, listed in
capi.SYMBOLS, exported by the library and bound with as many arguments as the header declares; bin/main's --draft rejects what lies outside its ranges."""
import ctypes as C
import inspect
import os
import re
import subprocess

import pytest

import __graft_entry__ as graft
from fast_llama_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAIN = os.path.join(graft.PKG_DIR, "bin", "main")
# symbol -> the number of parameters its declaration has
DECLARED = {"flm_verify_sample": 10, "flm_generate_lookup_sample": 15, "flm_op_sample_rows": 8}


def _declared_params(hdr, name):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", hdr)
    assert m, name + " is not declared"
    args = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    return [a.strip() for a in args.split(",")]


def _binding_calls(name):
    """the argument lists of lib().<name>( ... ) in capi.py"""
    src = inspect.getsource(capi)
    out = []
    for m in re.finditer(r"lib\(\)\." + name + r"\(", src):
        depth, i, args, cur = 1, m.end(), [], ""
        while depth:
            ch = src[i]
            depth += ch in "([" ; depth -= ch in ")]"
            if ch == "," and depth == 1:
                args.append(cur); cur = ""
            elif depth:
                cur += ch
            i += 1
        out.append([a.strip() for a in args + [cur]])
    return out


@pytest.mark.parametrize("name", list(DECLARED))
def test_new_symbols_are_declared_listed_exported_and_bound(name):
    hdr = open(os.path.join(ROOT, "include", "flm_gpu.h")).read()
    params = _declared_params(hdr, name)
    assert len(params) == DECLARED[name], params
    assert name in capi.SYMBOLS and hasattr(capi.lib(), name)
    calls = _binding_calls(name)
    assert calls and all(len(c) == len(params) for c in calls), (name, calls)


def test_bindings_have_the_documented_shape():
    v = list(inspect.signature(capi.Ctx.verify_sample).parameters)
    assert v == ["self", "first_token", "drafts", "pos", "temperature", "topp", "rng_state"], v
    g = inspect.signature(capi.Ctx.generate_lookup_sample).parameters
    assert list(g)[:10] == ["self", "prompt", "pos", "max_tokens", "temperature", "topp", "rng_state", "stop_token", "draft_len", "ngram_max"], list(g)
    assert (g["temperature"].default, g["topp"].default, g["rng_state"].default, g["stop_token"].default, g["draft_len"].default, g["ngram_max"].default) == (1.0, 0.9, 0, -1, 7, 3)
    assert list(inspect.signature(capi.op_sample_rows).parameters) == ["logits", "n", "temperature", "topp", "rng_state"]


def test_the_header_no_longer_calls_sampling_unbuilt():
    hdr = open(os.path.join(ROOT, "include", "flm_gpu.h")).read()
    assert "Temperature > 0 is not built" not in hdr


def test_null_arguments_are_rejected_without_a_gpu():
    lib = capi.lib()
    n = C.c_int(0); st = C.c_uint64(0)
    assert lib.flm_verify_sample(None, 1, None, 4, 0, C.c_float(1), C.c_float(0.9), C.byref(st), None, C.byref(n)) != 0
    assert lib.flm_generate_lookup_sample(None, None, 1, 0, 1, C.c_float(1), C.c_float(0.9), C.byref(st), -1, 7, 3, None, None, None, C.byref(n)) != 0
    lg = (C.c_float * 8)(); out = (C.c_int32 * 16)()
    for rows, ld, nn in ((0, 8, 8), (17, 8, 8), (1, 8, 1), (1, 7, 8)):
        assert lib.flm_op_sample_rows(lg, rows, ld, nn, C.c_float(1), C.c_float(0.9), C.byref(st), out) == -1, (rows, ld, nn)
    assert lib.flm_op_sample_rows(lg, 1, 8, 8, C.c_float(1), C.c_float(0.9), None, out) == -1
    assert st.value == 0


@pytest.mark.parametrize("value", ["3", "7,9", "16", "7,0", "7,", "x", "7,3,1"])
def test_cli_rejects_a_draft_outside_its_ranges(value):
    if not os.path.exists(MAIN):
        graft.build()
    r = subprocess.run([MAIN, "--draft", value], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "Invalid --draft" in r.stderr and "Usage:" in r.stderr, (r.returncode, r.stderr[-300:])


def test_cli_usage_lists_draft():
    if not os.path.exists(MAIN):
        graft.build()
    r = subprocess.run([MAIN, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and re.search(r"--draft\s+<K\[,G\]>", r.stderr), r.stderr[-600:]
