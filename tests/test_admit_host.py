"""Ragged passes over the cache slots without a GPU (include/flm_gpu.h: flm_batch_plan_for, flm_batch_admit, flm_batch_pass, flm_op_attention_segs; option "batch_rows"):
the symbols in the header, in capi.SYMBOLS and in the library; flm_batch_plan_for against a Python statement of the scheduling rule; the binding's argument checks;
bin/main's --batch-rows refusals."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import __graft_entry__ as graft
from fast_llama_amd import capi

MAIN = os.path.join(graft.PKG_DIR, "bin", "main")
SYMS = ("flm_batch_plan_for", "flm_batch_admit", "flm_batch_pass", "flm_op_attention_segs")


def test_symbols_and_binding():
    hdr = open(os.path.join(graft.ROOT, "include", "flm_gpu.h")).read()
    lib = capi.lib()
    for sym in SYMS:
        assert sym + "(" in hdr and sym in capi.SYMBOLS and hasattr(lib, sym)
    for t in ("flm_batch_seg", "flm_batch_plan", "flm_batch_pass_out"):
        assert "typedef struct " + t + " " in hdr
    assert C.sizeof(capi.BatchSegStruct) == 20
    assert C.sizeof(capi.BatchPlan) == 4 * 4 + 20 * capi.BATCH_MAX
    assert C.sizeof(capi.BatchPassOutStruct) == 4 * (capi.BATCH_MAX + 3)
    for m in ("batch_admit", "batch_pass"):
        assert callable(getattr(capi.Ctx, m))
    assert callable(capi.batch_plan) and callable(capi.op_attention_segs)
    # the header says how long the caller's prompt is read, and in which order the callbacks come
    assert "MUST STAY VALID until the slot has delivered its" in hdr and "(pass, slot) order" in hdr
    assert '"batch_rows"' in hdr and '"batch_passes"' in hdr
    assert "batch_rows" not in capi.TUNING_KEYS                        # a public option, not a dial


def py_plan(fed, pending, running, budget):
    """the scheduling rule as the header states it -> (segments, n_rows, n_step, n_draws), or None where the call refuses"""
    n = len(fed)
    if not 1 <= n <= 16 or budget < 0 or running >> n:
        return None
    if any(f < 0 or p < 0 for f, p in zip(fed, pending)) or any((running >> s) & 1 and pending[s] > 0 for s in range(n)):
        return None
    segs, rows = [], 0
    for s in range(n):                                                 # every running slot's one step row first, in slot order
        if (running >> s) & 1:
            segs.append((s, rows, 1, fed[s], 1)); rows += 1
    n_step = rows
    left = budget if budget > 0 else 1 << 40
    for s in range(n):                                                 # then the budget, in ascending slot order
        take = min(pending[s], left)
        if take < 1:
            continue
        segs.append((s, rows, take, fed[s], 1 if take == pending[s] else 0)); rows += take; left -= take
    return segs, rows, n_step, sum(g[4] for g in segs)


def c_plan(fed, pending, running, budget, n=None):
    out = capi.BatchPlan()
    out.n_segs = -7
    f = np.asarray(list(fed) + [0], dtype=np.int32); p = np.asarray(list(pending) + [0], dtype=np.int32)      # (one entry to spare: n = 0 still passes a pointer)
    n = len(fed) if n is None else n
    rc = capi.lib().flm_batch_plan_for(n, f.ctypes.data_as(C.c_void_p), p.ctypes.data_as(C.c_void_p), C.c_uint32(running), budget, C.byref(out))
    if rc != 0:
        assert rc == -1 and out.n_segs == -7, "a refused plan writes nothing"
        return None
    return out.segments(), out.n_rows, out.n_step, out.n_draws


def _consistent(plan, fed, pending, running):
    segs, n_rows, n_step, n_draws = plan
    assert n_rows == sum(g[2] for g in segs) and n_draws == sum(g[4] for g in segs) and len(segs) <= 16
    assert [g[1] for g in segs] == [sum(h[2] for h in segs[:i]) for i in range(len(segs))]                # the rows follow one another
    assert [g[0] for g in segs[:n_step]] == [s for s in range(len(fed)) if (running >> s) & 1]            # step rows first, in slot order
    assert all(g[2] == 1 and g[4] == 1 and g[1] == i for i, g in enumerate(segs[:n_step]))
    prompt = [g[0] for g in segs[n_step:]]
    assert prompt == sorted(prompt) and len(set(g[0] for g in segs)) == len(segs)                         # ascending slots, at most one segment per slot
    for s, _, n, pos0, draws in segs[n_step:]:
        assert 1 <= n <= pending[s] and pos0 == fed[s] and draws == (1 if n == pending[s] else 0)         # draws only where the prompt completes


def test_plan_grid():
    rng = np.random.default_rng(9)
    cases = 0
    for n in (1, 2, 3, 5, 15, 16):
        for trial in range(12):
            state = rng.integers(0, 3, n)                              # 0 empty, 1 running, 2 filling
            running = sum(1 << s for s in range(n) if state[s] == 1)
            fed = [int(rng.integers(0, 40)) if state[s] else 0 for s in range(n)]
            pending = [int(rng.integers(1, 70)) if state[s] == 2 else 0 for s in range(n)]
            total = sum(pending)
            for budget in sorted({0, 1, 2, 7, 8, 64, max(total - 1, 1), max(total, 1), total + 1}):
                want = py_plan(fed, pending, running, budget)
                got = c_plan(fed, pending, running, budget)
                assert got == want, (fed, pending, running, budget)
                _consistent(got, fed, pending, running)
                if budget:
                    assert got[1] - got[2] == min(budget, total)       # the budget is spent, and no more
                cases += 1
    assert cases > 400


def test_plan_edges():
    # a budget of 1: one row of the first filling slot
    assert c_plan([0, 0, 3], [5, 4, 0], 0b100, 1) == ([(2, 0, 1, 3, 1), (0, 1, 1, 0, 0)], 2, 1, 1)
    # a budget that ends exactly at a prompt's last row: slot 0 completes and draws, slot 1 gets nothing and has no segment ...
    assert c_plan([2, 0], [5, 4], 0, 5) == ([(0, 0, 5, 2, 1)], 5, 0, 1)
    # ... one row short of it: no draw, the pass classifies nothing
    assert c_plan([2, 0], [5, 4], 0, 4) == ([(0, 0, 4, 2, 0)], 4, 0, 0)
    # ... one row past it: the next slot's first row
    assert c_plan([2, 0], [5, 4], 0, 6) == ([(0, 0, 5, 2, 1), (1, 5, 1, 0, 0)], 6, 0, 1)
    # no bound: everything, every prompt completes
    assert c_plan([2, 0], [5, 4], 0, 0) == ([(0, 0, 5, 2, 1), (1, 5, 4, 0, 1)], 9, 0, 2)
    # 16 running slots and nothing pending: a step
    segs, n_rows, n_step, n_draws = c_plan(list(range(16)), [0] * 16, 0xFFFF, 8)
    assert (n_rows, n_step, n_draws) == (16, 16, 16) and segs == [(s, s, 1, s, 1) for s in range(16)]
    # 16 filling slots: 16 segments
    segs, n_rows, n_step, n_draws = c_plan([0] * 16, [3] * 16, 0, 0)
    assert (n_rows, n_step, n_draws) == (48, 0, 16) and segs == [(s, 3 * s, 3, 0, 1) for s in range(16)]
    # nothing to do
    assert c_plan([0, 0, 0], [0, 0, 0], 0, 0) == ([], 0, 0, 0)
    # the refusals
    assert c_plan([], [], 0, 0, n=0) is None and c_plan([0] * 17, [1] * 17, 0, 0) is None and c_plan([0], [1], 0, 0, n=-1) is None
    assert c_plan([0, 0], [3, 3], 0, -1) is None                       # a negative budget
    assert c_plan([0, -1], [3, 3], 0, 0) is None and c_plan([0, 0], [3, -3], 0, 0) is None
    assert c_plan([4, 0], [3, 3], 0b01, 0) is None                     # running and pending at once
    assert c_plan([4, 0], [0, 3], 0b100, 0) is None                    # a running slot outside the layout
    lib = capi.lib()
    one = np.ones(1, np.int32)
    assert lib.flm_batch_plan_for(1, one.ctypes.data_as(C.c_void_p), one.ctypes.data_as(C.c_void_p), C.c_uint32(0), 0, None) == -1
    assert lib.flm_batch_plan_for(1, None, one.ctypes.data_as(C.c_void_p), C.c_uint32(0), 0, C.byref(capi.BatchPlan())) == -1
    assert lib.flm_batch_plan_for(1, one.ctypes.data_as(C.c_void_p), None, C.c_uint32(0), 0, C.byref(capi.BatchPlan())) == -1


def test_a_refused_plan_says_why():
    lib = capi.lib()
    z = np.zeros(2, np.int32); p = np.array([3, 3], np.int32)
    a = lambda x: x.ctypes.data_as(C.c_void_p)
    assert lib.flm_batch_plan_for(2, a(z), a(p), C.c_uint32(0), -1, C.byref(capi.BatchPlan())) == -1
    assert b"negative budget" in lib.flm_last_error(None)
    assert lib.flm_batch_plan_for(17, a(z), a(p), C.c_uint32(0), 0, C.byref(capi.BatchPlan())) == -1
    assert b"n_slots" in lib.flm_last_error(None)
    assert lib.flm_batch_plan_for(2, a(z), a(p), C.c_uint32(1), 0, C.byref(capi.BatchPlan())) == -1
    assert b"at once" in lib.flm_last_error(None)


class _NoCtx(capi.Ctx):
    """the binding's own checks run before anything reaches the library: no context is needed for them"""
    def __init__(self):
        self._h = C.c_void_p()
        self.desc = None


def test_binding_argument_checks():
    ctx = _NoCtx()
    R = capi.BatchReq
    with pytest.raises(ValueError):
        ctx.batch_admit(0, R([1, 2], 0))                               # max_tokens < 1
    with pytest.raises(ValueError):
        ctx.batch_admit(0, R([], 4))                                   # an empty prompt
    with pytest.raises(ValueError):
        ctx.batch_admit(0, R([1, 2], 4, rng_state=-1))                 # a state outside 64 bits
    with pytest.raises(ValueError):
        capi.batch_plan([0, 0], [1], 0)                                # one entry per slot
    with pytest.raises(ValueError):
        capi.batch_plan([0], [1], -1)                                  # the mask
    with pytest.raises(capi.FlmError, match="flm error -1"):
        capi.batch_plan([0], [1], 0, -2)
    plan = capi.batch_plan([7, 0, 0], [0, 9, 2], 0b001, 10)
    assert isinstance(plan, capi.BatchPlan) and (plan.n_segs, plan.n_rows, plan.n_step, plan.n_draws) == (3, 11, 1, 2)
    assert plan.segments() == [(0, 0, 1, 7, 1), (1, 1, 9, 0, 1), (2, 10, 1, 0, 0)]
    kc = np.zeros((2, 16, 64), np.float32); x = np.zeros((3, 128), np.float32)
    with pytest.raises(ValueError):
        capi.op_attention_segs(kc, kc.copy(), x, x, x, 2, 64, 16, [0], [16, 1], [3], [0])      # one entry per segment
    with pytest.raises(ValueError):
        capi.op_attention_segs(kc, kc.copy(), x[:, :64], x[:, :64], x[:, :64], 2, 64, 16, [0], [16], [3], [0])      # rows of another width
    # a NULL context, NULL buffers: the library itself refuses, nothing is touched
    lib = capi.lib()
    st, _keep = R([3, 4, 5], 7).struct()
    out = capi.BatchPassOutStruct(); out.live = 77
    assert lib.flm_batch_admit(None, 0, C.byref(st)) == -1
    assert lib.flm_batch_pass(None, 0, C.byref(out)) == -1 and out.live == 77
    one = np.ones(1, np.int32); a = one.ctypes.data_as(C.c_void_p)
    assert lib.flm_op_attention_segs(None, None, None, None, None, None, 1, 64, 16, 1, 1, 0, a, a, a, a, 0) == -1


def _main(*args):
    if not os.path.exists(MAIN):
        graft.build()
    return subprocess.run([MAIN, "-c", "/nonexistent.flm", *args], capture_output=True, timeout=60)


def test_cli_batch_rows(tmp_path):
    """a value that is no count of rows, and --batch-rows without --prompts, are usage errors before any model is loaded"""
    path = tmp_path / "two.txt"
    path.write_text("hello world\nand so on\n")
    for bad in ("-1", "x", "8x", ""):
        r = _main("--prompts", str(path), "--batch-rows", bad)
        assert r.returncode != 0 and b"Invalid --batch-rows" in r.stderr, bad
    r = _main("-i", "hello", "--batch-rows", "8")
    assert r.returncode != 0 and b"--batch-rows applies to --prompts only" in r.stderr
    for good in ("0", "8", "256"):                                     # pass the checks: the run then fails at the model file
        r = _main("--prompts", str(path), "--batch-rows", good)
        assert r.returncode != 0 and b"Invalid --batch-rows" not in r.stderr and b"--batch-rows applies to" not in r.stderr and b"--prompts applies to" not in r.stderr
    r = _main("--prompts", str(path), "--batch-rows", "8", "--samples", "2")      # --prompts' own refusals stay
    assert r.returncode != 0 and b"--prompts applies to" in r.stderr
