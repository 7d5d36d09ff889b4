"""Parallel sampling without a GPU (include/flm_gpu.h: flm_generate_n, flm_fan_keep, flm_fan_layout_for, flm_op_attention_fan): the symbols and FLM_FAN_MAX in the
header, in capi.SYMBOLS and in the library; flm_fan_layout_for against a Python statement of the layout; the binding's argument checks; bin/main's --samples range."""
import ctypes as C
import os
import subprocess

import pytest

import __graft_entry__ as graft
from fast_llama_amd import capi

MAIN = os.path.join(graft.PKG_DIR, "bin", "main")


def test_symbols_and_binding():
    hdr = open(os.path.join(graft.ROOT, "include", "flm_gpu.h")).read()
    lib = capi.lib()
    for sym in ("flm_fan_layout_for", "flm_generate_n", "flm_fan_keep", "flm_op_attention_fan"):
        assert sym + "(" in hdr and sym in capi.SYMBOLS and hasattr(lib, sym)
    assert "#define FLM_FAN_MAX " in hdr and int(hdr.split("#define FLM_FAN_MAX ")[1].split()[0]) == capi.FAN_MAX == 16
    assert "flm_fan_cb" in hdr and "typedef struct flm_fan_layout" in hdr
    # flm_fan_layout: three words and FLM_FAN_MAX bases
    assert C.sizeof(capi.FanLayout) == 4 * (3 + capi.FAN_MAX)
    # the header says what the call ignores
    assert "IGNORES installed stop rules" in hdr


def py_layout(pos, n_prompt, max_tokens, n, max_seq_len):
    """the layout as the header states it: None where the call refuses"""
    if not 2 <= n <= 16 or pos < 0 or n_prompt < 1 or max_tokens < 1:
        return None
    S = pos + n_prompt
    if S + n * (max_tokens - 1) > max_seq_len:
        return None
    return S, max_tokens - 1, [S + j * (max_tokens - 1) for j in range(n)]


def c_layout(pos, n_prompt, max_tokens, n, max_seq_len):
    out = capi.FanLayout()
    for i in range(capi.FAN_MAX):
        out.base[i] = -7
    rc = capi.lib().flm_fan_layout_for(pos, n_prompt, max_tokens, n, max_seq_len, C.byref(out))
    if rc != 0:
        assert rc == -1 and all(out.base[i] == -7 for i in range(capi.FAN_MAX)), "a refused layout writes nothing"
        return None
    assert out.n == n
    return out.shared_rows, out.tail_rows, [out.base[j] for j in range(n)]


def test_layout_grid():
    cases = 0
    for pos in (0, 1, 17):
        for n_prompt in (1, 3, 40):
            for max_tokens in (1, 2, 9, 64):
                for n in (1, 2, 3, 5, 16, 17):
                    fit = pos + n_prompt + n * (max_tokens - 1)
                    for max_seq_len in (fit - 1, fit, fit + 1, 256):        # one row over, the exact fit, one to spare
                        if max_seq_len < 1:
                            continue
                        assert c_layout(pos, n_prompt, max_tokens, n, max_seq_len) == py_layout(pos, n_prompt, max_tokens, n, max_seq_len), (pos, n_prompt, max_tokens, n, max_seq_len)
                        cases += 1
    assert cases > 800


def test_layout_edges():
    # max_tokens == 1: no tail rows at all, every base is S
    assert c_layout(4, 6, 1, 5, 10) == (10, 0, [10] * 5)
    assert c_layout(4, 6, 1, 5, 9) is None
    # the exact fit and one row over
    assert c_layout(0, 8, 9, 16, 8 + 16 * 8) == (8, 8, [8 + 8 * j for j in range(16)])
    assert c_layout(0, 8, 9, 16, 8 + 16 * 8 - 1) is None
    # n = 1 and n = 17 are refused; negative / empty arguments too
    assert c_layout(0, 8, 4, 1, 256) is None and c_layout(0, 8, 4, 17, 256) is None
    assert c_layout(-1, 8, 4, 2, 256) is None and c_layout(0, 0, 4, 2, 256) is None and c_layout(0, 8, 0, 2, 256) is None
    # sizes whose product passes 2^31 do not wrap
    assert c_layout(0, 1, 2 ** 30, 16, 2 ** 31 - 1) is None
    assert capi.lib().flm_fan_layout_for(0, 8, 4, 2, 256, None) == -1
    # the binding: the struct, or FlmError
    lay = capi.fan_layout(3, 5, 4, 3, 64)
    assert (lay.shared_rows, lay.tail_rows, lay.n, list(lay.base[:3])) == (8, 3, 3, [8, 11, 14])
    with pytest.raises(capi.FlmError):
        capi.fan_layout(3, 5, 4, 3, 16)


class _NoCtx(capi.Ctx):
    """the binding's own checks run before anything reaches the library: no context is needed for them"""
    def __init__(self):
        self._h = C.c_void_p()
        self.desc = None


def test_binding_argument_checks():
    ctx = _NoCtx()
    with pytest.raises(ValueError):
        ctx.generate_n([1, 2], 0, 4)                                   # neither states nor n
    with pytest.raises(ValueError):
        ctx.generate_n([1, 2], 0, 4, n=3, temperature=1.0)            # no states at temperature != 0
    with pytest.raises(ValueError):
        ctx.generate_n([1, 2], 0, 4, states=[1, 2, 3], n=4)           # n differs from len(states)
    with pytest.raises(ValueError):
        ctx.generate_n([1, 2], 0, 4, states=[1])                      # n = 1
    with pytest.raises(ValueError):
        ctx.generate_n([1, 2], 0, 4, states=list(range(17)))          # n = 17
    with pytest.raises(ValueError):
        ctx.generate_n([1, 2], 0, 0, states=[1, 2])                   # max_tokens < 1
    # a NULL context: the library itself refuses, nothing is touched
    lib = capi.lib()
    assert lib.flm_generate_n(None, None, 0, 0, 1, 2, C.c_float(0), C.c_float(0), None, -1, None, None, None, None) == -1
    assert lib.flm_fan_keep(None, 0) == -1
    assert lib.flm_op_attention_fan(None, None, None, None, None, None, 1, 64, 16, 2, 1, 0, None) == -1


@pytest.mark.parametrize("bad", ["0", "17", "-1", "3x", ""])
def test_cli_samples_range(bad):
    if not os.path.exists(MAIN):
        graft.build()
    r = subprocess.run([MAIN, "-c", "/nonexistent.flm", "--samples", bad], capture_output=True, timeout=60)
    assert r.returncode != 0 and b"Invalid --samples" in r.stderr
