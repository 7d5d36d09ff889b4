"""Cache slots without a GPU (include/flm_gpu.h: flm_batch_layout_for, flm_batch_open / _join / _step / _state / _close, flm_generate_batch, flm_op_attention_slots): the
symbols and FLM_BATCH_MAX in the header, in capi.SYMBOLS and in the library; flm_batch_layout_for against a Python statement of the layout; the binding's argument checks;
bin/main's --prompts refusals."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import __graft_entry__ as graft
from fast_llama_amd import capi

MAIN = os.path.join(graft.PKG_DIR, "bin", "main")
SYMS = ("flm_batch_layout_for", "flm_batch_open", "flm_batch_join", "flm_batch_step", "flm_batch_state", "flm_batch_close", "flm_generate_batch", "flm_op_attention_slots")


def test_symbols_and_binding():
    hdr = open(os.path.join(graft.ROOT, "include", "flm_gpu.h")).read()
    lib = capi.lib()
    for sym in SYMS:
        assert sym + "(" in hdr and sym in capi.SYMBOLS and hasattr(lib, sym)
    assert "#define FLM_BATCH_MAX " in hdr and int(hdr.split("#define FLM_BATCH_MAX ")[1].split()[0]) == capi.BATCH_MAX == 16
    for t in ("flm_batch_layout", "flm_batch_req", "flm_batch_out"):
        assert "typedef struct " + t + " " in hdr
    # the structs as the header lays them out
    assert C.sizeof(capi.BatchLayout) == 4 * (1 + 2 * capi.BATCH_MAX)
    assert C.sizeof(capi.BatchOutStruct) == 4 * (capi.BATCH_MAX + 2)
    assert C.sizeof(capi.BatchReqStruct) == 40 and capi.BatchReqStruct.rng_state.offset == 24 and capi.BatchReqStruct.stop_token.offset == 32
    # the header says what the calls ignore
    assert "IGNORE installed sampling controls, stop rules, the constraint, armed log-probabilities and flm_entropy_set" in hdr
    for m in ("batch_open", "batch_join", "batch_step", "batch_state", "batch_close", "generate_batch"):
        assert callable(getattr(capi.Ctx, m))
    assert callable(capi.batch_layout) and callable(capi.op_attention_slots)


def py_layout(rows, max_seq_len):
    """the layout as the header states it: None where the call refuses"""
    if not 1 <= len(rows) <= 16 or any(r < 1 for r in rows) or sum(rows) > max_seq_len:
        return None
    return [sum(rows[:s]) for s in range(len(rows))], list(rows)


def c_layout(rows, max_seq_len, n=None):
    out = capi.BatchLayout()
    out.n_slots = -7
    for i in range(capi.BATCH_MAX):
        out.base[i] = -7; out.rows[i] = -7
    r = np.asarray(list(rows) + [1], dtype=np.int32)                  # (one entry to spare: n = 0 still passes a pointer)
    n = len(rows) if n is None else n
    rc = capi.lib().flm_batch_layout_for(n, r.ctypes.data_as(C.c_void_p), max_seq_len, C.byref(out))
    if rc != 0:
        assert rc == -1 and out.n_slots == -7 and all(out.base[i] == -7 and out.rows[i] == -7 for i in range(capi.BATCH_MAX)), "a refused layout writes nothing"
        return None
    assert out.n_slots == n
    return [out.base[s] for s in range(n)], [out.rows[s] for s in range(n)]


def test_layout_grid():
    rng = np.random.default_rng(5)
    cases = 0
    for n in (1, 2, 3, 5, 15, 16):
        for kind in ("ones", "equal", "ragged", "one-big"):
            rows = {"ones": [1] * n, "equal": [9] * n, "ragged": [int(x) for x in rng.integers(1, 70, n)], "one-big": [1] * (n - 1) + [200]}[kind]
            fit = sum(rows)
            for max_seq_len in (fit - 1, fit, fit + 1, 4096):         # one row over, the exact fit, one to spare
                if max_seq_len < 1:
                    continue
                assert c_layout(rows, max_seq_len) == py_layout(rows, max_seq_len), (rows, max_seq_len)
                cases += 1
            for s in (0, n - 1):                                      # a slot of no rows, or fewer
                for bad in (0, -1):
                    b = list(rows); b[s] = bad
                    assert c_layout(b, 4096) is None
                    cases += 1
    assert cases > 100


def test_layout_edges():
    # the exact fit and one row over; slot 0 starts at row 0, base is the prefix sum
    assert c_layout([8, 100, 20], 128) == ([0, 8, 108], [8, 100, 20])
    assert c_layout([8, 100, 20], 127) is None
    assert c_layout([16] * 16, 256) == ([16 * s for s in range(16)], [16] * 16)
    assert c_layout([16] * 16, 255) is None
    # n_slots 0 and 17 are refused
    assert c_layout([], 256, n=0) is None and c_layout([1] * 17, 256) is None and c_layout([1], 256, n=-1) is None
    # sums past 2^31 do not wrap
    assert c_layout([2 ** 30] * 4, 2 ** 31 - 1) is None
    lib = capi.lib()
    one = np.ones(1, np.int32)
    assert lib.flm_batch_layout_for(1, one.ctypes.data_as(C.c_void_p), 256, None) == -1
    assert lib.flm_batch_layout_for(1, None, 256, C.byref(capi.BatchLayout())) == -1
    # the binding: the struct, or FlmError
    lay = capi.batch_layout([5, 7, 3], 64)
    assert (lay.n_slots, list(lay.base[:3]), list(lay.rows[:3])) == (3, [0, 5, 12], [5, 7, 3])
    with pytest.raises(capi.FlmError, match="flm error -1"):
        capi.batch_layout([5, 7, 3], 14)
    with pytest.raises(capi.FlmError, match="flm error -1"):
        capi.batch_layout([5, 0, 3], 64)


def test_a_refused_layout_says_why():
    lib = capi.lib()
    r = np.array([200, 100], np.int32)
    assert lib.flm_batch_layout_for(2, r.ctypes.data_as(C.c_void_p), 256, C.byref(capi.BatchLayout())) == -1
    assert b"exceed max_seq_len" in lib.flm_last_error(None)
    assert lib.flm_batch_layout_for(17, r.ctypes.data_as(C.c_void_p), 256, C.byref(capi.BatchLayout())) == -1
    assert b"n_slots" in lib.flm_last_error(None)
    r[1] = 0
    assert lib.flm_batch_layout_for(2, r.ctypes.data_as(C.c_void_p), 256, C.byref(capi.BatchLayout())) == -1
    assert b"fewer than 1 row" in lib.flm_last_error(None)


class _NoCtx(capi.Ctx):
    """the binding's own checks run before anything reaches the library: no context is needed for them"""
    def __init__(self):
        self._h = C.c_void_p()
        self.desc = None


def test_binding_argument_checks():
    ctx = _NoCtx()
    R = capi.BatchReq
    with pytest.raises(ValueError):
        ctx.generate_batch([])                                         # no request
    with pytest.raises(ValueError):
        ctx.generate_batch([R([1, 2], 4)] * 17)                        # 17 requests
    with pytest.raises(ValueError):
        ctx.generate_batch([R([1, 2], 0)])                             # max_tokens < 1
    with pytest.raises(ValueError):
        ctx.generate_batch([R([], 4)])                                 # an empty prompt
    with pytest.raises(ValueError):
        ctx.batch_join(0, R([1, 2], 4, rng_state=-1))                  # a state outside 64 bits
    with pytest.raises(ValueError):
        ctx.batch_join(0, R([1, 2], 4, rng_state=1 << 64))
    st, keep = R([3, 4, 5], 7, 0.5, 0.25, (1 << 64) - 1, 2).struct()
    assert (st.n_prompt, st.max_tokens, st.temperature, st.topp, st.rng_state, st.stop_token) == (3, 7, 0.5, 0.25, (1 << 64) - 1, 2) and list(keep) == [3, 4, 5]
    # a NULL context: the library itself refuses, nothing is touched
    lib = capi.lib()
    lay = capi.batch_layout([8, 8], 64)
    first = C.c_int32(-5); live = C.c_int(-5); out = capi.BatchOutStruct()
    assert lib.flm_batch_open(None, C.byref(lay)) == -1
    assert lib.flm_batch_join(None, 0, C.byref(st), C.byref(first), C.byref(live)) == -1 and first.value == -5 and live.value == -5
    assert lib.flm_batch_step(None, C.byref(out)) == -1
    assert lib.flm_batch_state(None, 0, None, None, None) == -1
    assert lib.flm_batch_close(None, -1) == -1 and lib.flm_batch_close(None, 0) == -1
    assert lib.flm_generate_batch(None, None, 1, None, None, None, 4, None, None) == -1
    assert lib.flm_op_attention_slots(None, None, None, None, None, None, 1, 64, 16, 1, None, None) == -1


def _main(*args):
    if not os.path.exists(MAIN):
        graft.build()
    return subprocess.run([MAIN, "-c", "/nonexistent.flm", *args], capture_output=True, timeout=60)


def test_cli_prompts_file(tmp_path):
    """a file that cannot be read, is empty, has an empty line or more than 16 lines is a usage error before any model is loaded"""
    cases = {"none": None, "empty": "", "blank-line": "one\n\nthree\n", "seventeen": "".join(f"prompt {i}\n" for i in range(17))}
    for tag, text in cases.items():
        path = tmp_path / (tag + ".txt")
        if text is not None:
            path.write_text(text)
        r = _main("--prompts", str(path))
        assert r.returncode != 0 and b"Invalid --prompts file" in r.stderr, tag
    # 16 lines, the last one without a newline, pass the check: the run then fails at the model file
    path = tmp_path / "sixteen.txt"
    path.write_text("\n".join(f"prompt {i}" for i in range(16)))
    r = _main("--prompts", str(path))
    assert r.returncode != 0 and b"Invalid --prompts" not in r.stderr and b"--prompts applies to" not in r.stderr


@pytest.mark.parametrize("extra", [["--samples", "2"], ["--top-k", "5"], ["--draft", "7"], ["--lookup", "7", "-t", "0"], ["--logprobs", "2"], ["--stop-ids", "5"], ["--mode", "score"], ["--devices", "0,1"], ["--typical", "0.5"]])
def test_cli_prompts_refuses_the_extras(tmp_path, extra):
    """refused, not ignored, with the extras --samples refuses (and --samples itself), before a model is loaded"""
    path = tmp_path / "two.txt"
    path.write_text("hello world\nand so on\n")
    r = _main("--prompts", str(path), *extra)
    assert r.returncode != 0 and b"--prompts applies to" in r.stderr, r.stderr
