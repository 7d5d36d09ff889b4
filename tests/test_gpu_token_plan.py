"""The token's launch plan, seen from outside: enqueue_token, flm_kernel_times and query("token_path") decide from ONE plan (csrc/flm_host.h TokenPlan), so
what each of them reports for a shape and an option set is pinned here against tests/golden/token_plan.json.

The fixture was recorded on an MI355X from a build of the commit in front of the one that introduced the plan (its header says which, and how many CUs the
device had): launch geometry is sized by the CU count, so the test insists on the same count instead of comparing against figures of another device.

  shapes       synth "tiny128" (2 heads of 128) and "tiny" (4 heads of 64): every fused form exists; "tiny_hs32" ("tiny" with 8 heads of 32): the head size is not a
               multiple of 64, so the SHAPE refuses the whole-layer, all-layers and one-launch-token forms (count 0) while the options, and with them token_path's bits
               128 / 256 / 512, still allow them -- the FLM_ERR_UNSUPPORTED path of the launch functions; bit 1024 is clear there, because it also asks that the
               one-launch token's argument block was planned, which the shape refuses too (token_path 967, not 1991).  All int8, 2 layers
  option sets  the defaults and each launch-structure option switched on its own
  per case     query("token_path") behind a 3-token prompt, the per-class `count` of kernel_times(pos=3, iters=1), kernel_bytes of every class at positions 3 and 200
"""
import ctypes
import json
import os

import numpy as np
import pytest

from fast_llama_amd import flmfile as ff, synth

pytestmark = pytest.mark.gpu
FIXTURE = os.path.join(os.path.dirname(__file__), "golden", "token_plan.json")

SHAPES = {"tiny128": "tiny128", "tiny": "tiny", "tiny_hs32": (256, 512, 2, 8, 320)}      # name -> synth.make_config's shape (dim, hidden, layers, heads, vocab)
OPTION_SETS = [{}, {"fuse_tail": 0}, {"fuse_token": 0}, {"fuse_layer": 0}, {"fuse_back": 0}, {"fuse_attn_o": 0}, {"fuse_ffn": 0}, {"fuse_qkv": 2}, {"fuse_qkv": 0},
               {"attn_split": 2}]
POSITIONS = [3, 200]
PROMPT = np.array([1, 17, 200], dtype=np.int32)


def opts_id(opts):
    return ",".join(f"{k}={v}" for k, v in opts.items()) or "defaults"


def device_cu_count(device=0):
    """the device's compute units as HIP reports them.  No query key exposes flm_ctx::cu_count; flm_ctx_create takes it from this very attribute
    (multiProcessorCount) of the device the context is created on, and the contexts here are created with the default device 0 and without "cu_parts", so the two agree."""
    hip = ctypes.CDLL("libamdhip64.so")
    n = ctypes.c_int(0)
    assert hip.hipDeviceGetAttribute(ctypes.byref(n), 63, device) == 0      # 63: hipDeviceAttributeMultiprocessorCount (hip_runtime_api.h, ROCm 7)
    return n.value


def make_ctx(capi, shape, opts):
    cfg = synth.make_config(SHAPES[shape], ff.QT_INT8)
    cfg.n_layers = 2
    ctx = capi.Ctx(capi.desc_from_config(cfg))
    ctx.upload_all(synth.make_tensors(cfg, seed=5))
    for k, v in opts.items():
        ctx.set_option(k, v)
    return ctx


def collect(capi, shape, opts):
    """what the three readers of the plan say about one context"""
    ctx = make_ctx(capi, shape, opts)
    try:
        ctx.forward(PROMPT, 0)
        out = {"token_path": ctx.query("token_path")}
        out["count"] = {k: c for k, (_, c) in ctx.kernel_times(3, iters=1).items()}
        out["token_path_after"] = ctx.query("token_path")
        out["bytes"] = {str(p): {k: ctx.kernel_bytes(k, p) for k in capi.KCLASSES} for p in POSITIONS}
    finally:
        ctx.close()
    return out


@pytest.fixture(scope="module")
def golden():
    with open(FIXTURE) as f:
        return json.load(f)


@pytest.mark.parametrize("opts", OPTION_SETS, ids=opts_id)
@pytest.mark.parametrize("shape", SHAPES)
def test_plan_readers_agree_with_recorded(gpu, golden, shape, opts):
    assert device_cu_count() == golden["header"]["cu_count"], "the fixture was recorded on a device with another CU count"
    got = collect(gpu, shape, opts)
    want = golden["cases"][f"{shape}|{opts_id(opts)}"]
    assert got["token_path"] == want["token_path"]
    assert got["token_path_after"] == want["token_path_after"]
    assert got["count"] == want["count"]
    assert got["bytes"] == want["bytes"]          # (doubles, every one a multiple of 1/16: JSON carries them exactly)


@pytest.mark.parametrize("shape", SHAPES)
def test_decode_unchanged_behind_kernel_times(gpu, shape):
    """flm_kernel_times leaves the context where the next operation is a fresh prompt at 0: the same prompt and greedy decode give the ids they gave before it"""
    ctx = make_ctx(gpu, shape, {})
    try:
        def run():
            tok = int(np.argmax(ctx.forward(PROMPT, 0)))
            return [tok] + [int(t) for t in ctx.decode_greedy(tok, len(PROMPT), 8)]
        before = run()
        ctx.kernel_times(3, iters=1)
        assert run() == before
    finally:
        ctx.close()
