"""INT4 contexts (W4A8: 4-bit weights, int8 activations).  One rule carries every test: an INT4 context computes, bit for bit, what the INT8 arithmetic computes on the
sign-extended nibbles with the same scales -- the expected values come from the unchanged CPU oracle at QT_INT8 on synth.int8_statement of the same tensors."""
import os
import re
import subprocess

import numpy as np
import pytest

import __graft_entry__ as graft
import oracle_py
from fast_llama_amd import capi, flmfile as ff, synth
from test_int4_host import quantizer_inputs

pytestmark = pytest.mark.gpu
PROMPT = np.array([1, 17, 200, 45, 9], dtype=np.int32)
N = len(PROMPT)
MODELS = {"tiny": None, "tiny128": None, "small": None, "7B": 2}          # shape: layers kept
_made = {}
bits = lambda a: np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)   # noqa: E731


# (m, n): one group, two lanes, one live row of 32 | CB = 2, odd rows | CB = 8, RB = 8, rows past the end | CB = 64, RB = 1 | CB = 8, 43 column blocks | unpack + tiles
@pytest.mark.parametrize("m,n,w", [(1, 64, 1), (5, 192, 1), (331, 256, 1), (130, 2048, 1), (70, 11008, 1), (331, 256, 16)])
def test_matmul_against_the_int8_oracle(gpu, m, n, w):
    rng = np.random.default_rng([m, n, w])
    W = rng.integers(-8, 8, size=(m, n), dtype=np.int8)
    X = rng.integers(-127, 128, size=(w, n), dtype=np.int8)
    sW, sX = ((rng.random((r, n // 64), dtype=np.float32) + np.float32(0.5)) * np.float32(1e-2) for r in (m, w))
    X[0] = np.where(rng.random(n) < 0.5, -127, 127); W[0] = -8               # an all -8 row against +-127: the largest offset term
    if m > 3:
        W[1] = 7; W[2] = 0; sW[3, 0] = 0.0
    got = gpu.op_matmul_q(capi.QT_INT4, capi.pack_int4(W), sW, X, sX)
    want = oracle_py.matmul_q(oracle_py.QT_INT8, W, sW, X, sX)
    assert np.array_equal(bits(got), bits(want)), np.argwhere(bits(got) != bits(want))[:4].tolist()


def test_quantizer_equals_its_numpy_statement(gpu):
    x = np.concatenate([quantizer_inputs(), np.random.default_rng(5).standard_normal(4096).astype(np.float32)])
    (q, s), (qh, sh) = gpu.op_quantize(x, capi.QT_INT4), capi.quantize_int4_host(x)
    assert np.array_equal(q, qh) and np.array_equal(bits(s), bits(sh))


def _model(name):
    """-> (cfg, INT4 tensors, the oracle's logits for the prompt token by token and three greedy steps, its ids, [the 130-token prompt and its logits]), made once"""
    if name not in _made:
        cfg, cfg8 = synth.make_config(name, capi.QT_INT4), synth.make_config(name, ff.QT_INT8)
        cfg.n_layers = cfg8.n_layers = MODELS[name] or cfg.n_layers
        tensors = synth.make_tensors(cfg, seed=7)
        om = oracle_py.OracleModel(cfg8, synth.int8_statement(tensors), max_seq=256)
        steps, ids = [], []
        for i in range(N + 3):
            steps.append(om.forward(np.array([PROMPT[i] if i < N else ids[-1]], dtype=np.int32), i))
            if i >= N - 1:
                ids.append(int(np.argmax(steps[-1])))
        long = None
        if name == "tiny":
            om.reset()
            long = [(np.arange(130, dtype=np.int32) * 7 + 3) % cfg.vocab_size]
            long.append(om.forward(long[0], 0))
        _made[name] = (cfg, tensors, steps, ids, long)
    return _made[name]


def _ctx(gpu, cfg, tensors):
    ctx = gpu.Ctx(gpu.desc_from_config(cfg, max_seq_len=256)); ctx.upload_all(tensors)
    return ctx


@pytest.mark.parametrize("name", list(MODELS))
def test_model_against_the_int8_oracle(gpu, name):
    cfg, tensors, steps, ids, long = _model(name)
    ctx = _ctx(gpu, cfg, tensors); ctx.set_option("use_prefill", 0)
    assert ctx.query("token_path") & ~64 == 0                            # no fused form (bit 6: the attention's split, not a fusion)
    for i in range(N + 3):                                               # the prompt token by token, then three decode steps
        tok = PROMPT[i] if i < N else ids[i - N]
        assert np.array_equal(bits(ctx.forward(np.array([tok], dtype=np.int32), i)), bits(steps[i])), (name, i)
    ctx.set_option("fuse_token", 1)                                      # accepted, decides nothing: the same form, the same logits at the last position again
    assert ctx.query("token_path") & ~64 == 0
    assert np.array_equal(bits(ctx.forward(np.array([ids[2]], dtype=np.int32), N + 2)), bits(steps[N + 2])), (name, "fuse_token")
    ctx.set_option("use_prefill", 1)                                     # the same prompt batched: the int8 tiles on the unpacked copy
    ctx.reset_kv()
    assert np.array_equal(bits(ctx.forward(PROMPT, 0)), bits(steps[N - 1])), (name, "batched")
    assert list(ctx.decode_greedy(ids[0], N, 3)) == ids[1:4], name
    ctx.reset_kv()
    assert list(ctx.generate(PROMPT, 0, 4)[0]) == ids[:4], name
    if long is not None:
        ctx.reset_kv()
        assert np.array_equal(bits(ctx.forward(long[0], 0)), bits(long[1])), (name, "130 tokens")
        ctx.reset_kv(); ctx.forward(PROMPT, 0)
        got = ctx.verify_greedy(ids[0], np.array(ids[1:4] + [0], dtype=np.int32), N)      # three right drafts, then a wrong one
        assert list(got[:3]) == ids[1:4] and len(got) >= 4, (name, list(got))
    assert ctx.query("fallback") == 0
    ctx.close()


def test_fp32_master_is_quantized_like_the_numpy_statement(gpu):
    cfg = synth.make_config("tiny", capi.QT_INT4)
    master = synth.make_tensors(cfg, seed=9, fp32_master=True)
    packed = {k: capi.quantize_int4_host(v) if k[0] in ff.LAYER_KINDS + (ff.T_CLASSIFIER,) and v.ndim == 2 else v for k, v in master.items()}
    logits = []
    for tensors in (master, packed):
        ctx = _ctx(gpu, cfg, tensors)
        logits.append(ctx.forward(PROMPT, 0)); ctx.close()
    assert np.array_equal(bits(logits[0]), bits(logits[1]))


def test_refusals_leave_the_context_usable(gpu):
    cfg, tensors, steps, ids, _ = _model("tiny")
    with pytest.raises(capi.FlmError, match="flm error -2"):                 # FLM_ERR_UNSUPPORTED: tensor parallelism
        gpu.Ctx(gpu.desc_from_config(cfg, max_seq_len=256), rank=0, world=2)
    ctx = _ctx(gpu, cfg, tensors)
    ctx8 = gpu.Ctx(gpu.desc_from_config(synth.make_config("tiny", ff.QT_INT8), max_seq_len=256))
    emb4 = (np.zeros((cfg.vocab_size, cfg.dim // 2), np.uint8), np.zeros((cfg.vocab_size, cfg.dim // 64), np.float32))
    key = (ff.T_ATTN_O, 0)
    # FLM_ERR_INVALID: an INT8 tuple into an INT4 context, the converse, an INT4 embedding table
    for c, k, v in ((ctx, key, synth.int8_statement(tensors)[key]), (ctx8, key, tensors[key]), (ctx, (ff.T_TOKEN_EMBD, 0), emb4)):
        with pytest.raises(capi.FlmError, match="flm error -1"):
            c.upload(*k, v)
    assert np.array_equal(bits(ctx.forward(PROMPT, 0)), bits(steps[N - 1]))
    ctx.close(); ctx8.close()


def test_cli_q_int4_prints_the_context_ids(gpu, tmp_path):
    """bin/main -q int4 on an fp32-master .flm: the text is Ctx.generate's ids on an INT4 context fed the same fp32 tensors, decoded by the host library"""
    cfg, path = synth.make_config("tiny", capi.QT_INT4), str(tmp_path / "tiny.flm")
    master = synth.write_synthetic_flm(path, cfg, seed=1, fp32_master=True)
    main = os.path.join(graft.PKG_DIR, "bin", "main")
    r = subprocess.run([main, "-c", path, "-j", "1", "-q", "int4", "-n", "24", "-i", "hello world and so on", "-t", "0"], capture_output=True, timeout=300)
    assert r.returncode == 0 and b"int4" in r.stdout, r.stderr.decode(errors="replace")
    prompt = [int(x) for x in re.search(rb"Input tokens:\[([^\]]*)\]", r.stdout).group(1).replace(b",", b" ").split()]
    body = r.stdout[r.stdout.index(b"output: \x1b[32m") + len(b"output: \x1b[32m"):]
    ctx = _ctx(gpu, cfg, master)
    ids = [int(x) for x in ctx.generate(np.array(prompt, np.int32), 0, 25, stop_token=0)[0]]
    ctx.close()
    d = subprocess.run([main, "-c", path, "-d", " ".join(map(str, ids))], capture_output=True, timeout=60)      # the CLI's decode mode on the context's ids
    assert d.returncode == 0 and body[:body.index(b"\x1b[0m\n\nnum_threads")] == d.stdout.split(b"  text: ", 1)[1][:-1] and len(ids) > 1
