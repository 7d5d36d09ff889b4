"""The model-based drafter without a GPU: include/flm_gpu.h declares flm_draft_set / flm_generate_draft and the library exports them, fast-llama_amd/capi.py calls them
with as many arguments as the header declares, bin/main knows --draft-model and refuses a file it cannot open before it loads anything."""
import os
import re
import subprocess

import numpy as np

import __graft_entry__ as graft
from fast_llama_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAIN = os.path.join(graft.PKG_DIR, "bin", "main")


def _declared(name):
    """the parameter list of `name` in the header, comments removed -> [parameter text]"""
    hdr = open(os.path.join(ROOT, "include", "flm_gpu.h")).read()
    m = re.search(r"^int\s+%s\s*\(([^;]*)\);" % name, hdr, re.M)
    assert m, f"{name} is not declared in include/flm_gpu.h"
    return [p.strip() for p in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")]


def test_header_declares_and_library_exports_both_functions():
    assert _declared("flm_draft_set") == ["flm_ctx* ctx", "flm_ctx* draft"]
    gen, look = _declared("flm_generate_draft"), _declared("flm_generate_lookup_ex")
    assert gen == [p for p in look if "ngram_max" not in p] and len(gen) == len(look) - 1 == 13      # flm_generate_lookup_ex's signature without ngram_max
    assert {"flm_draft_set", "flm_generate_draft"} <= set(capi.SYMBOLS)
    lib = capi.lib()
    assert hasattr(lib, "flm_draft_set") and hasattr(lib, "flm_generate_draft")
    assert lib.flm_draft_set(None, None) == -1 and lib.flm_generate_draft(None, None, 1, 0, 1, None, None, -1, 7, None, None, None, None) == -1


class _FakeLib:
    """records the arguments of every flm_* call and reports success"""

    def __init__(self):
        self.calls = {}

    def __getattr__(self, name):
        if not name.startswith("flm_"):
            raise AttributeError(name)

        def call(*args):
            self.calls[name] = args
            return 0
        return call


def test_capi_binds_both_with_the_headers_argument_counts(monkeypatch):
    fake = _FakeLib()
    monkeypatch.setattr(capi, "lib", lambda: fake)
    ctx, draft = object.__new__(capi.Ctx), object.__new__(capi.Ctx)
    ctx._h, draft._h = None, None                 # (never created: close() has nothing to destroy)
    ctx.draft_set(draft)
    assert len(fake.calls["flm_draft_set"]) == len(_declared("flm_draft_set"))
    ctx.draft_set(None)
    assert fake.calls["flm_draft_set"][1] is None
    for sampling in (capi.Sampling(temperature=1.0, top_k=5), None):
        ids, st = ctx.generate_draft(np.array([1, 2, 3], np.int32), 4, 9, sampling, rng_state=5, stop_token=2, draft_len=6, on_token=lambda i, t, last: False)
        args = fake.calls["flm_generate_draft"]
        assert len(args) == len(_declared("flm_generate_draft"))
        assert args[2:5] == (3, 4, 9) and args[7].value == 2 and args[8] == 6        # n_prompt, pos, max_tokens, stop_token, draft_len in the header's order
        assert (args[5] is None) == (sampling is None)
        assert len(ids) == 0 and st == 5


def test_main_knows_the_flag_and_refuses_a_missing_file():
    if not os.path.exists(MAIN):
        graft.build()
    r = subprocess.run([MAIN, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--draft-model" in r.stderr
    # a file that cannot be opened is a usage error before any model (or the GPU) is touched: a clean message, no crash
    r = subprocess.run([MAIN, "-c", "/nonexistent/model.flm", "--draft-model", "/nonexistent/draft.flm", "-i", "x"], capture_output=True, text=True, timeout=60)
    assert r.returncode not in (0, -6, -11) and "Invalid --draft-model file" in r.stderr and "/nonexistent/draft.flm" in r.stderr
    assert "Failed to load model" not in r.stderr
    # a flag without its value: usage
    r = subprocess.run([MAIN, "-c", "/nonexistent/model.flm", "--draft-model"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "--draft-model" in r.stderr
