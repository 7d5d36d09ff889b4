"""flm_generate without a GPU: declared in include/flm_gpu.h, listed in capi.SYMBOLS, exported by the library, bound as Ctx.generate; its argument
checks that need no device."""
import ctypes as C
import inspect
import os
import re

from fast_llama_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_generate_is_declared_listed_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "flm_gpu.h")).read()
    assert re.search(r"\bint\s+flm_generate\s*\(\s*flm_ctx\s*\*", hdr)
    assert re.search(r"typedef\s+int\s*\(\s*\*\s*flm_token_cb\s*\)\s*\(\s*void\s*\*\s*user\s*,\s*int\s+index\s*,\s*int32_t\s+token\s*,\s*int\s+last\s*\)", hdr)
    assert "flm_generate" in capi.SYMBOLS
    assert hasattr(capi.lib(), "flm_generate")
    params = list(inspect.signature(capi.Ctx.generate).parameters)
    assert params[:9] == ["self", "prompt", "pos", "max_tokens", "temperature", "topp", "rng_state", "stop_token", "on_token"], params
    sig = inspect.signature(capi.Ctx.generate).parameters
    assert (sig["temperature"].default, sig["topp"].default, sig["rng_state"].default, sig["stop_token"].default, sig["on_token"].default) == (0.0, 0.9, 0, -1, None)


def test_generate_query_keys_are_documented():
    hdr = open(os.path.join(ROOT, "include", "flm_gpu.h")).read()
    comment = hdr[hdr.index("/* What the context actually runs"):hdr.index("flm_query(flm_ctx*")]
    assert '"gen_tokens"' in comment and '"gen_streamed"' in comment


def test_generate_rejects_null_arguments_without_a_gpu():
    lib = capi.lib()
    n = C.c_int(0)
    assert lib.flm_generate(None, None, 1, 0, 1, C.c_float(0), C.c_float(0.9), None, -1, None, None, None, C.byref(n)) != 0
