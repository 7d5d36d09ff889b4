"""The head-size axis at model level: the 2-layer models of tests/head_sizes.py's table (int8 at every size, int16 at one size per class) against the CPU oracle, logits
bit for bit; and the entry points with kernels of their own (flm_score_tokens, flm_verify_greedy, flm_generate_batch, flm_generate_n) at head sizes 40, 96 and 256 against
the context's own plain path on a second context.  Everything is equality: logits and K / V rows on bit patterns, ids, 64-bit sampler states.

Every size names the launch form it is meant to cover (LAUNCH_FORM) and asserts it through the plan readers of test_gpu_token_plan.py -- query("token_path") and the
per-class count of kernel_times --, so a later dispatch change cannot move a size to another kernel and leave these tests green but empty:
  * a multiple of 64 (64, 128, 192, 256): the heads hand Wo a quantized output; the whole-layer, all-layers and one-launch-token forms exist.  Above 128 a head cannot be
    spread over workgroups, so the one-launch token (which takes a head's first two tiles at once) exists only where max_seq_len <= 128: the launch-form test runs a
    context of 128 rows.
  * everything else at one workgroup per head: the shape refuses those forms; attention + Wo runs as k_attn_o with fp32 hand-off.
  * 64, 96 and 128 from 128 rows on, and everywhere with "attn_split" 2: hs / 32 workgroups per head (96: three) inside the fused launches, the split instantiation
    of the one-launch token included; the other sizes cannot split and nothing changes."""
import numpy as np
import pytest

import head_sizes as HS
from fast_llama_amd import flmfile as ff
from test_gpu_batch import _check_batch, _requests
from test_gpu_fan import SETTINGS, _fill, _reference, _states
from test_gpu_spec import MAX_SEQ, _caches, _ctx, _prompt, _verify_cases, bits

pytestmark = pytest.mark.gpu
CASE_IDS = [HS.case_id(c) for c in HS.CASES]
SIZE_IDS = [f"hs{hs}" for hs in HS.SIZES]
ENTRY_IDS = [f"hs{hs}" for hs in HS.ENTRY_SIZES]
# the launch form a size covers at one workgroup per head: "token" = the one-launch token (k_layers<.., TAIL>), "attn_wo" = per-phase launches around k_attn_o
LAUNCH_FORM = {hs: "token" if hs % 64 == 0 else "attn_wo" for hs in HS.SIZES}
FORM_MAX_SEQ = 128


def _new_ctx(gpu, hs, qt, max_seq_len=1024, **opts):
    cfg, tensors = HS.model(hs, qt)
    ctx = gpu.Ctx(gpu.desc_from_config(cfg, max_seq_len=max_seq_len)); ctx.upload_all(tensors)
    for k, v in opts.items():
        ctx.set_option(k, v)
    return cfg, ctx


def _kv(ctx, cfg, rows, max_seq_len=1024):
    hs = cfg.dim // cfg.n_heads
    n = cfg.n_heads * max_seq_len * hs
    return [ctx.debug_read(w, l, n).view(np.uint32).reshape(cfg.n_heads, max_seq_len, hs)[:, :rows].copy() for l in range(cfg.n_layers) for w in ("kcache", "vcache")]


# ---- against the oracle ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", HS.CASES, ids=CASE_IDS)
def test_short_prompt_token_by_token(gpu, case):
    hs, qt = case
    want = HS.long_run(hs, qt)["first5"]
    cfg, ctx = _new_ctx(gpu, hs, qt)
    try:
        for i in range(5):
            lg = ctx.forward(HS.LONG_PROMPT[i:i + 1], i)
            assert np.array_equal(bits(lg), bits(want[i])), (hs, qt, i)
        assert ctx.query("fallback") == 0
    finally:
        ctx.close()


@pytest.mark.parametrize("case", HS.CASES, ids=CASE_IDS)
def test_long_prompt_batched_and_token_by_token(gpu, case):
    """130 tokens from an empty cache: the batched prompt path (two token tiles and two rows; QK^T on the matrix cores where hs % 32 == 0 and hs <= 128, the multi-query
    VALU form at the other sizes up to 128, one query per workgroup above), then the same with "use_prefill" 0: the same K / V rows in every layer, the same logits,
    the oracle's.  Which of the three attention forms ran is INFERRED from the shape and the options' defaults (flm_prompt.hip picks it; no plan reader reports the
    batched path's kernels): the comparison shows that the result is right, not which kernel produced it"""
    hs, qt = case
    want = HS.long_run(hs, qt)["prompt"]
    n = len(HS.LONG_PROMPT)
    out = {}
    for batched in (1, 0):
        cfg, ctx = _new_ctx(gpu, hs, qt, use_prefill=batched)
        try:
            out[batched] = (ctx.forward(HS.LONG_PROMPT, 0), _kv(ctx, cfg, n))
            assert ctx.query("fallback") == 0
        finally:
            ctx.close()
    assert np.array_equal(bits(out[1][0]), bits(want)), (hs, qt, "batched")
    assert np.array_equal(bits(out[0][0]), bits(want)), (hs, qt, "token by token")
    for i, (a, b) in enumerate(zip(out[1][1], out[0][1])):
        assert np.array_equal(a, b), (hs, qt, f"layer {i // 2} {'KV'[i % 2]} rows", np.argwhere(a != b)[:4].tolist())


def _counts(ctx, pos):
    return {k: c for k, (_, c) in ctx.kernel_times(pos, iters=1).items()}


def _decode_behind_prompt(gpu, hs, qt, forced, **opts):
    """forced: the options spread a head over hs / 32 workgroups at every position where the shape can split (else: from 128 rows on)"""
    run, form = HS.long_run(hs, qt), HS.form_run(hs, qt)
    cfg, ctx = _new_ctx(gpu, hs, qt, **opts)
    split = HS.split_parts(hs) > 1
    whole = hs % 64 == 0
    try:
        # the 5-token prompt token by token and eleven greedy tokens behind it: contexts of 1 .. 16 rows (forced split: parts without a position tile of their own)
        for i in range(5):
            lg = ctx.forward(HS.LONG_PROMPT[i:i + 1], i)
            assert np.array_equal(bits(lg), bits(run["first5"][i])), (hs, qt, opts, i)
        assert list(ctx.decode_greedy(int(np.argmax(lg)), 5, HS.N_GREEDY)) == form["ids5"][:HS.N_GREEDY], (hs, qt, opts)
        # ... and the plan there (flm_kernel_times decides with attn_parts(position + 1), as the token does).  Forced split where the shape can split: QKV + attention + Wo in
        # one launch and the split instantiations of the whole-layer forms and of the one-launch token.  One workgroup per head (every size without the option, the sizes
        # that cannot split with it): no QKV in that launch; the whole-layer forms at multiples of 64; the one-launch token at 64 and 128 only (in a 1024-row context it
        # asks that long contexts can split: not 192, 256)
        count = _counts(ctx, 5)                                           # (leaves the context ready for a prompt at 0)
        print(f"hs {hs} qt {qt} {opts} position 5: count {count}")
        if forced and split:
            assert count["qkv_attn_wo"] == cfg.n_layers and count["layer"] == cfg.n_layers and count["layers"] > 0 and count["token"] > 0, count
        else:
            assert count["qkv_attn_wo"] == 0 and count["layer"] == (cfg.n_layers if whole else 0) and (count["layers"] > 0) == whole, count
            assert (count["token"] > 0) == (whole and split), count
        ctx.reset_kv()
        lg = ctx.forward(HS.LONG_PROMPT, 0)
        assert np.array_equal(bits(lg), bits(run["prompt"])), (hs, qt, opts)
        pos = len(HS.LONG_PROMPT)
        for i in range(HS.N_STEPS):
            cur = int(np.argmax(lg))
            lg = ctx.forward(np.array([cur], np.int32), pos); pos += 1
            assert np.array_equal(bits(lg), bits(run["steps"][i])), (hs, qt, opts, i)
        assert (int(np.argmax(lg)), pos) == (run["cur"], run["pos"])
        assert list(ctx.decode_greedy(run["cur"], pos, HS.N_GREEDY)) == run["ids"], (hs, qt, opts)
        assert ctx.query("fallback") == 0
        count = _counts(ctx, pos)
        print(f"hs {hs} qt {qt} {opts} position {pos}: count {count}")
        # the plan at position 133 of a 1024-row context.  From 128 rows on a head is spread over hs / 32 workgroups where the shape can split (64, 96, 128), with or without the
        # option: the split forms -- at 96 too, where only the one-workgroup-per-head form asks for whole quant groups per head.  Where it cannot: the whole-layer forms at
        # multiples of 64 (192, 256), without the one-launch token
        assert count["qkv_attn_wo"] == (cfg.n_layers if split else 0), count
        assert count["layer"] == (cfg.n_layers if split or whole else 0) and (count["layers"] > 0) == (split or whole), count
        assert (count["token"] > 0) == split, count
        assert count["attn_wo"] == cfg.n_layers and count["attn"] == cfg.n_layers, count
    finally:
        ctx.close()


@pytest.mark.parametrize("case", HS.CASES, ids=CASE_IDS)
def test_decode_behind_long_prompt(gpu, case):
    """the body of test_gpu_fuzz.test_random_shapes_vs_oracle: the prompt, three forward steps, eleven tokens of the device-resident greedy loop; in front of it a short
    context, where no size splits under the default options (the plan at position 5 says so)"""
    hs, qt = case
    _decode_behind_prompt(gpu, hs, qt, forced=False)


@pytest.mark.parametrize("case", HS.CASES, ids=CASE_IDS)
def test_decode_with_split_heads(gpu, case):
    """ "attn_split" 2: hs / 32 workgroups per head at EVERY position where the shape can split (64, 96 -- three parts --, 128), also at contexts of 1 .. 16 rows where parts
    have no position tile of their own -- the plan at position 5 must show the split forms there, which it does not under the default (test_decode_behind_long_prompt);
    the other sizes cannot split: nothing changes"""
    hs, qt = case
    _decode_behind_prompt(gpu, hs, qt, forced=True, attn_split=2)


@pytest.mark.parametrize("hs", HS.SIZES, ids=SIZE_IDS)
def test_launch_form(gpu, hs):
    """A context of 128 rows (above it the one-launch token asks that heads can split, which 192 and 256 cannot) filled to its last row.  The form the size is meant to
    cover is read from the plan at positions 3 and 126 (one workgroup per head up to 127 rows); then a 5-token prompt token by token, the device greedy loop over
    positions 5 .. 64 (the second position tile begins: the one-launch token's heads take this token's K / V row as granules into whichever of their two tiles holds it),
    one forward at 65 compared on its logits, and the greedy loop again over 66 .. 127 (the sizes that can split do so at the last row), ids against the oracle's"""
    run, form = HS.long_run(hs, ff.QT_INT8), HS.form_run(hs, ff.QT_INT8)
    assert HS.FORM_ROWS == FORM_MAX_SEQ
    cfg, ctx = _new_ctx(gpu, hs, ff.QT_INT8, max_seq_len=FORM_MAX_SEQ)
    try:
        ctx.forward(HS.LONG_PROMPT[:3], 0)
        path = ctx.query("token_path")
        for at in (3, FORM_MAX_SEQ - 2):
            count = _counts(ctx, at)
            print(f"hs {hs} max_seq_len {FORM_MAX_SEQ} position {at}: token_path {path} count {count}")
            assert count["attn_wo"] == cfg.n_layers and count["attn"] == cfg.n_layers and count["qkv_attn_wo"] == 0, count
            if LAUNCH_FORM[hs] == "token":
                assert path & 1024 and count["token"] > 0 and count["layers"] > 0 and count["layer"] == cfg.n_layers, (path, count)
            else:
                assert not path & 1024 and count["token"] == 0 and count["layers"] == 0 and count["layer"] == 0 and count["back"] == 0, (path, count)
        for i in range(5):
            lg = ctx.forward(HS.LONG_PROMPT[i:i + 1], i)
            assert np.array_equal(bits(lg), bits(run["first5"][i])), (hs, i)
        at = HS.FORM_LOGITS_AT
        ids = list(ctx.decode_greedy(int(np.argmax(lg)), 5, at - 5))
        assert ids == form["ids5"], (hs, [i for i, (a, b) in enumerate(zip(ids, form["ids5"])) if a != b][:4])
        lg = ctx.forward(np.array([ids[-1]], np.int32), at)
        assert np.array_equal(bits(lg), bits(form["logits"])), hs
        ids = list(ctx.decode_greedy(int(np.argmax(lg)), at + 1, FORM_MAX_SEQ - at - 1))
        assert len(ids) == FORM_MAX_SEQ - at - 1 and ids == form["ids"], (hs, [i for i, (a, b) in enumerate(zip(ids, form["ids"])) if a != b][:4])
        assert ctx.query("fallback") == 0
    finally:
        ctx.close()


# ---- the entry points with kernels of their own, against the plain path on a second context (max_seq_len 256) -----------------------------------------------------------
_pairs = {}


@pytest.fixture(scope="module")
def pair(gpu):
    """(cfg, tensors, the context under test, the reference context) per head size, made once"""
    def get(hs):
        if hs not in _pairs:
            cfg, tensors = HS.model(hs, ff.QT_INT8)
            _pairs[hs] = (cfg, tensors, _ctx(gpu, cfg, tensors), _ctx(gpu, cfg, tensors))
        return _pairs[hs]
    yield get
    for _, _, a, b in _pairs.values():
        a.close(); b.close()
    _pairs.clear()


@pytest.mark.parametrize("hs", HS.ENTRY_SIZES, ids=ENTRY_IDS)
def test_score_is_forward_per_prefix(pair, hs):
    """flm_score_tokens on 70 tokens (a token tile and six rows): row i's logits are flm_forward's behind the prefix of i + 1 tokens, the K / V rows are its rows"""
    cfg, _, ctx, ref = pair(hs)
    toks = HS.tokens(70, salt=9)
    ctx.reset_kv(); ref.reset_kv()
    got, lg = ctx.score(toks, 0, want_logits=True)
    for i in range(len(toks)):
        want = ref.forward(toks[i:i + 1], i)
        assert np.array_equal(bits(lg[i]), bits(want)), (hs, i)
        assert int(got["argmax"][i]) == int(np.argmax(want)), (hs, i)
    for a, b in zip(_caches(ctx, cfg), _caches(ref, cfg)):
        assert np.array_equal(a[:, :len(toks)], b[:, :len(toks)]), hs
    assert ctx.query("fallback") == 0


@pytest.mark.parametrize("hs", HS.ENTRY_SIZES, ids=ENTRY_IDS)
def test_verify_greedy_seven_drafts(gpu, hs):
    """test_gpu_spec's cases with seven drafts (none / the first / draft 2 / the last made wrong), at position 0 and behind a 37-token prompt, "spec_gemm" 1 and 0"""
    cfg, tensors = HS.model(hs, ff.QT_INT8)
    _verify_cases(gpu, cfg, tensors, (1, 0), (0, 37), (7,))


@pytest.mark.parametrize("hs", HS.ENTRY_SIZES, ids=ENTRY_IDS)
def test_generate_batch_five_requests(pair, gpu, hs):
    """prompt lengths 65 / 1 / 64 / 5 / 63 in one call: ids and states of every request equal its own flm_generate, and every slot's K / V rows are that run's rows"""
    cfg, _, ctx, ref = pair(hs)
    name = f"hs{hs}"
    reqs = _requests(cfg.vocab_size, [65, 1, 64, 5, 63], 41 + hs)
    assert sum(len(q.prompt) + q.max_tokens - 1 for q in reqs) <= MAX_SEQ
    got = _check_batch(ctx, ref, name, reqs, name)
    assert [len(g) for g in got] == [q.max_tokens for q in reqs]
    mine = _caches(ctx, cfg)
    lay = gpu.batch_layout([len(q.prompt) + q.max_tokens - 1 for q in reqs], MAX_SEQ)
    for j, q in enumerate(reqs):
        ref.reset_kv()
        ref.generate(q.prompt, 0, q.max_tokens, temperature=q.temperature, topp=q.topp, rng_state=q.rng_state)
        rows, b = len(q.prompt) + len(got[j]) - 1, lay.base[j]
        for a, r in zip(mine, _caches(ref, cfg)):
            assert np.array_equal(a[:, b:b + rows], r[:, :rows]), (name, j)
    assert ctx.query("fallback") == 0


@pytest.mark.parametrize("hs", [40, 96], ids=["hs40", "hs96"])
def test_generate_n_five_rows(pair, hs):
    """n = 5 completions: ids and states equal flm_generate's with that state, behind a 3-token prompt at position 0 and a 40-token prompt behind 9 earlier rows, sampled
    and greedy; the shared rows stay flm_forward's"""
    cfg, _, ctx, ref = pair(hs)
    n, M = 5, 7
    for n_prompt, pos in ((3, 0), (40, 9)):
        prompt = _prompt(cfg.vocab_size, n_prompt, seed=n_prompt + pos)
        S = pos + n_prompt
        for si in (0, 3):
            t, p = SETTINGS[si]
            _fill((ctx, ref), cfg, pos)
            states = _states(n, 100 * n + si)
            want, after = _reference(ref, prompt, pos, M, t, p, states)
            got, st = ctx.generate_n(prompt, pos, M, states=states, temperature=t, topp=p)
            tag = (hs, n_prompt, pos, t, p)
            assert len(got) == n and all(np.array_equal(g, w) for g, w in zip(got, want)), (tag, [list(g) for g in got], [list(w) for w in want])
            assert st == after, tag
            if t != 0:
                assert any(not np.array_equal(got[0], g) for g in got[2:]), (tag, "every state drew the same ids: the case shows nothing")
            for a, b in zip(_caches(ctx, cfg), _caches(ref, cfg)):
                assert np.array_equal(a[:, :S], b[:, :S]), (tag, "the shared rows")
    assert ctx.query("fallback") == 0


def test_generate_n_refuses_head_size_256(pair, gpu):
    """above 128 there is no multi-query attention: FLM_ERR_UNSUPPORTED with its message, the cache bit for bit what it was"""
    cfg, _, ctx, _ = pair(256)
    ctx.reset_kv()
    ctx.forward(_prompt(cfg.vocab_size, 9, seed=11), 0)
    before = _caches(ctx, cfg)
    with pytest.raises(gpu.FlmError, match=r"flm error -2: generate_n: head sizes up to 128"):
        ctx.generate_n(_prompt(cfg.vocab_size, 3), 9, 7, n=5)
    for a, b in zip(_caches(ctx, cfg), before):
        assert np.array_equal(a, b)
