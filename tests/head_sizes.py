"""The head-size axis (TEST INFRASTRUCTURE): one table of small model shapes keyed by head size, the dispatch class of every size, and seeded builders of the
op-level cases.  No GPU here; tests/test_head_sizes_host.py pins the oracle at every table size (against the reference library where it is built, against
tests/golden/head_sizes.npz everywhere), tests/test_gpu_head_sizes.py and tests/test_gpu_head_sizes_model.py feed the same cases to the kernels.

flm_ctx_create and the op entry points accept every head size that is a multiple of 8 in [32, 256].  The kernels dispatch on it three ways (dispatch_class):
  * hs <= 64 / <= 128 / > 128   16-byte pieces of a K / V tile per thread (attn_head's NF = 1 / 2 / 4), the LDS row stride 72 / 136 / 264, threads per query of the
                                multi-query forms; above 128 no multi-query attention (prompt path: one query per workgroup; the fan is refused)
  * hs % 32 == 0                a head can be spread over hs / 32 workgroups (hs <= 128); the prompt path has QK^T on the matrix cores (hs <= 128)
  * hs % 64 == 0                a head's output is whole quant groups: the heads hand Wo a quantized output, the whole-layer / all-layers / one-launch-token forms exist
"""
from __future__ import annotations

import numpy as np

from fast_llama_amd import flmfile as ff, synth

SEED = 20250317
VOCAB = 331                                                        # odd: classifier workgroups with an uneven share of rows
HIDDEN = 192                                                       # three quant groups
# head size -> (dim, hidden_dim, layers, heads, vocab).  dim % 64 == 0 (whole quant groups), dim >= 256 (the reference's thread-group sizing: dim * dim / 24576 >= threads,
# so the reference runs these with 1 or 2 threads)
SHAPES = {
    32: (256, HIDDEN, 2, 8, VOCAB),        # NF 1, a multiple of 32 but not of 64: the smallest accepted size
    40: (320, HIDDEN, 2, 8, VOCAB),        # NF 1, no multiple of 32
    56: (448, HIDDEN, 2, 8, VOCAB),        # NF 1, no multiple of 32
    64: (256, HIDDEN, 2, 4, VOCAB),        # anchor
    72: (576, HIDDEN, 2, 8, VOCAB),        # NF 2, no multiple of 32
    96: (384, HIDDEN, 2, 4, VOCAB),        # NF 2, three parts per head, k_qk_mfma<3>, no multiple of 64
    120: (960, HIDDEN, 2, 8, VOCAB),       # NF 2, no multiple of 32
    128: (256, HIDDEN, 2, 2, VOCAB),       # anchor
    136: (1088, HIDDEN, 2, 8, VOCAB),      # NF 4, no multiple of 32
    160: (320, HIDDEN, 2, 2, VOCAB),       # NF 4, a multiple of 32 but not of 64
    192: (384, HIDDEN, 2, 2, VOCAB),       # NF 4, a multiple of 64: the one-launch token
    200: (1600, HIDDEN, 2, 8, VOCAB),      # NF 4, no multiple of 32
    256: (512, HIDDEN, 2, 2, VOCAB),       # NF 4, the largest accepted size
}
SIZES = tuple(SHAPES)
INT16_SIZES = (40, 96, 200, 256)                                   # one per class; int8 runs at every size
ENTRY_SIZES = (40, 96, 256)                                        # the entry points with kernels of their own (score, verify, batch, fan)
ACCEPTED = tuple(range(32, 257, 8))                                # what flm_ctx_create accepts
ROPE_POSITIONS = (0, 1, 37, 255)
QT_NAME = {ff.QT_INT8: "int8", ff.QT_INT16: "int16"}
CASES = [(hs, ff.QT_INT8) for hs in SIZES] + [(hs, ff.QT_INT16) for hs in INT16_SIZES]


def case_id(case):
    return f"hs{case[0]}-{QT_NAME[case[1]]}"


def dispatch_class(hs):
    """-> (0 / 1 / 2 for hs <= 64 / <= 128 / > 128, hs % 32 == 0, hs % 64 == 0)"""
    return (0 if hs <= 64 else 1 if hs <= 128 else 2, hs % 32 == 0, hs % 64 == 0)


def split_parts(hs):
    """workgroups per head when a head is split (attn_parts): hs / 32 where hs is a multiple of 32, at least 64 and at most 128; else 1"""
    return hs // 32 if hs % 32 == 0 and 64 <= hs <= 128 else 1


# ---- models ------------------------------------------------------------------------------------------------------------------------------------------------------------
_models = {}


def model(hs, qt):
    """-> (cfg, tensors) of the table's model at head size hs; built once per key and shared (never modify the arrays)"""
    if (hs, qt) not in _models:
        cfg = synth.make_config(SHAPES[hs], qt)
        assert cfg.dim // cfg.n_heads == hs and cfg.dim % 64 == 0 and cfg.dim >= 256
        _models[(hs, qt)] = (cfg, synth.make_tensors(cfg, seed=1000 + hs))
    return _models[(hs, qt)]


def tokens(n, salt=0):
    return np.array([1] + [int(x) for x in ((np.arange(1, n) + salt) * 7919) % VOCAB], np.int32)


SHORT_PROMPT = tokens(11)
LONG_PROMPT = tokens(130, salt=5)                                  # the batched prompt path; crosses two 64-row tiles
N_GREEDY_REF = 5
N_STEPS, N_GREEDY = 3, 11
_short, _long = {}, {}


def greedy_run(m, prompt, steps):
    """the prompt in one call, then `steps` greedy tokens one by one on `m` (anything with forward(tokens, pos)) -> [logits per call]"""
    out = [m.forward(prompt, 0).copy()]
    pos = len(prompt)
    for _ in range(steps):
        out.append(m.forward(np.array([int(np.argmax(out[-1]))], np.int32), pos).copy()); pos += 1
    return out


def short_logits(hs, qt):
    """the oracle's logits of SHORT_PROMPT and N_GREEDY_REF greedy steps (what the reference comparison and the golden fixture pin); computed once"""
    import oracle_py as O
    if (hs, qt) not in _short:
        _short[(hs, qt)] = greedy_run(O.OracleModel(*model(hs, qt)), SHORT_PROMPT, N_GREEDY_REF)
    return _short[(hs, qt)]


def long_run(hs, qt):
    """the oracle on the GPU model tests' schedule, computed once and shared (never modify it) -> dict:
      first5   the logits of LONG_PROMPT[:5] fed token by token from an empty cache
      prompt   the logits of LONG_PROMPT fed in one call from an empty cache
      steps    the logits of N_STEPS greedy tokens behind it
      ids      the N_GREEDY greedy ids behind those (cur, pos: the token and the position the device loop starts from)"""
    import oracle_py as O
    if (hs, qt) not in _long:
        om = O.OracleModel(*model(hs, qt))
        first5 = [om.forward(LONG_PROMPT[i:i + 1], i).copy() for i in range(5)]
        om.reset()
        lg = greedy_run(om, LONG_PROMPT, N_STEPS)
        cur, pos = int(np.argmax(lg[-1])), len(LONG_PROMPT) + N_STEPS
        ids, oc = [], cur
        for k in range(N_GREEDY):
            oc = int(np.argmax(om.forward(np.array([oc], np.int32), pos + k))); ids.append(oc)
        _long[(hs, qt)] = dict(first5=first5, prompt=lg[0], steps=lg[1:], cur=cur, pos=pos, ids=ids)
    return _long[(hs, qt)]


FORM_ROWS = 128                                                     # the launch-form test's context: the one-launch token exists at 192 and 256 only up to 128 rows
FORM_LOGITS_AT = 65                                                 # ... where one forward's logits are compared in between (66 rows: a tile and two)
_form = {}


def form_run(hs, qt):
    """the oracle filling a context of FORM_ROWS rows to its last row, computed once and shared -> dict:
      ids5     the greedy ids behind LONG_PROMPT[:5], fed at positions 5 .. FORM_LOGITS_AT - 1 (the last of them is not fed by the loop that produced it)
      logits   the logits of that last id fed at position FORM_LOGITS_AT
      ids      the greedy ids of the loop that starts with their argmax at FORM_LOGITS_AT + 1 and feeds every position up to FORM_ROWS - 1"""
    import oracle_py as O
    if (hs, qt) not in _form:
        om = O.OracleModel(*model(hs, qt))
        for i in range(5):
            lg = om.forward(LONG_PROMPT[i:i + 1], i)

        def loop(cur, pos, n):
            out = []
            for k in range(n):
                cur = int(np.argmax(om.forward(np.array([cur], np.int32), pos + k))); out.append(cur)
            return out
        ids5 = loop(int(np.argmax(lg)), 5, FORM_LOGITS_AT - 5)
        logits = om.forward(np.array([ids5[-1]], np.int32), FORM_LOGITS_AT).copy()
        ids = loop(int(np.argmax(logits)), FORM_LOGITS_AT + 1, FORM_ROWS - FORM_LOGITS_AT - 1)
        _form[(hs, qt)] = dict(ids5=ids5, logits=logits, ids=ids)
    return _form[(hs, qt)]


# ---- op level ----------------------------------------------------------------------------------------------------------------------------------------------------------
# Every cache row behind a query's own range holds NaN: a read outside it poisons the result.
DECODE_POSITIONS = (0, 1, 2, 5, 63, 64, 65, 130, 257)
PEAKED_AT = 130                                                     # the decode position whose query is scaled by 40
SPLIT_POSITIONS = (0, 3, 63, 64, 200, 255, 256, 257, 700, 1023)
SPLIT_PEAKED_AT = 700
_decode = {}


def rope_input(hs, pos):
    return np.random.default_rng([SEED, 1, hs, pos]).standard_normal(hs).astype(np.float32)


def softmax_weights(kr, q, k, hs, pos):
    """the softmax weights of one head's query at `pos` over its cache rows kr[:pos] and its own new row (NumPy, float64; RoPE from the oracle)"""
    import oracle_py as O
    qr = O.rope(q, pos); kn = O.rope(k, pos)
    K = np.concatenate([kr[:pos], kn[None]]).astype(np.float64)
    sc = (K @ qr.astype(np.float64)) / np.sqrt(hs)
    e = np.exp(sc - sc.max())
    return e / e.sum()


def is_peaked(w):
    """weights under the 1e-15 skip threshold (with a margin of 100 for the fp32 arithmetic of the real thing) next to weights that count: behind row 0, which is never
    skipped, at least one row is kept (its weight above the threshold by the same margin), so the weighted sum's chain has skipped and kept rows side by side.  (With the
    query scaled by 40 the softmax is close to one-hot: a second weight of ordinary size is not there to ask for.)"""
    return (w[1:] < 1e-17).sum() > 5 and (w[1:] > 1e-13).sum() >= 1


def decode_steps(hs, heads, positions, peaked_at, max_seq, seed):
    """The oracle's decode attention at `positions`, the cache filled by the oracle's batched path in between -> ([dict per position], kc, vc): pos, q / k / v
    [heads][hs], the oracle's output and the K / V row it appended; kc, vc [heads][max_seq][hs] the oracle's cache behind the last step (a row never changes once it
    is written: cache_before gives the cache in front of a step).  Computed once per key and shared (never modify it)."""
    import oracle_py as O
    key = (hs, heads, tuple(positions), peaked_at, max_seq, seed)
    if key in _decode:
        return _decode[key]
    rng = np.random.default_rng([SEED, 2, hs, heads, seed])
    kc = np.zeros((heads, max_seq, hs), np.float32); vc = np.zeros_like(kc)
    out, pos = [], 0
    for target in positions:
        if target > pos:
            bs = target - pos
            q = rng.standard_normal((heads, bs, hs)).astype(np.float32); k = rng.standard_normal((heads, bs, hs)).astype(np.float32)
            v = rng.standard_normal((heads, bs, hs)).astype(np.float32)
            for h in range(heads):
                O.attention_head(kc[h], vc[h], q[h], k[h], v[h], pos)
            pos = target
        q = rng.standard_normal((heads, hs)).astype(np.float32) * 2; k = rng.standard_normal((heads, hs)).astype(np.float32)
        v = rng.standard_normal((heads, hs)).astype(np.float32)
        if target == peaked_at:
            q *= np.float32(40.0)
        ref = np.stack([O.attention_head(kc[h], vc[h], q[h:h + 1], k[h:h + 1], v[h:h + 1], pos)[0] for h in range(heads)])
        out.append(dict(pos=pos, q=q, k=k, v=v, out=ref, krow=kc[:, pos].copy(), vrow=vc[:, pos].copy()))
        pos += 1
    _decode[key] = (out, kc, vc)
    return _decode[key]


def cache_before(c, pos):
    """a copy of the cache c [heads][max_seq][hs] as it stands in front of the step at `pos`: the pos earlier rows, NaN behind"""
    g = np.full_like(c, np.nan)
    g[:, :pos] = c[:, :pos]
    return g


OP_HEADS = 2                                                        # the slots' and the fan's cases
SLOT_POSITIONS = (0, 64, 130)
SLOT_SIZES = (40, 96, 200, 256)
FAN_SIZES = (40, 72, 96, 120)
FAN_S, FAN_T = 65, 69                                               # a prefix that crosses a tile, a tail that crosses a tile


def _oracle_row(kr, vr, q, k, v, hs, pos):
    """one query on its own contiguous cache kr, vr [heads][rows][hs] (updated in place: row pos) -> out [heads * hs]"""
    import oracle_py as O
    return np.concatenate([O.attention_head(kr[h], vr[h], q[h * hs:(h + 1) * hs][None], k[h * hs:(h + 1) * hs][None], v[h * hs:(h + 1) * hs][None], pos)[0]
                           for h in range(OP_HEADS)])


def slots_case(hs):
    """B = 3 slots that ABUT (slot s has pos[s] + 1 rows: pos[s] fed earlier, one for this step), three rows nobody owns behind them, NaN wherever no earlier token lies
    -> kc, vc, q, k, v, base, pos, max_seq and per row the oracle's (out, K row, V row) on the row's own contiguous cache"""
    rng = np.random.default_rng([SEED, 3, hs])
    pos = list(SLOT_POSITIONS)
    base = [int(x) for x in np.concatenate([[0], np.cumsum([p + 1 for p in pos])[:-1]])]
    max_seq = base[-1] + pos[-1] + 1 + 3
    kc = np.full((OP_HEADS, max_seq, hs), np.nan, np.float32); vc = np.full_like(kc, np.nan)
    for b, p in zip(base, pos):
        kc[:, b:b + p] = rng.standard_normal((OP_HEADS, p, hs)); vc[:, b:b + p] = rng.standard_normal((OP_HEADS, p, hs))
    n = len(pos)
    q = (rng.standard_normal((n, OP_HEADS * hs)) * 2).astype(np.float32)
    k = rng.standard_normal((n, OP_HEADS * hs)).astype(np.float32); v = rng.standard_normal((n, OP_HEADS * hs)).astype(np.float32)
    want = []
    for r, (b, p) in enumerate(zip(base, pos)):
        kr = np.full((OP_HEADS, p + 3, hs), np.nan, np.float32); vr = np.full_like(kr, np.nan)
        kr[:, :p] = kc[:, b:b + p]; vr[:, :p] = vc[:, b:b + p]
        o = _oracle_row(kr, vr, q[r], k[r], v[r], hs, p)
        want.append((o, kr[:, p].copy(), vr[:, p].copy()))
    return kc, vc, q, k, v, base, pos, max_seq, want


def fan_case(hs, n, S=FAN_S, t=FAN_T):
    """the fan's caches: S shared rows, then n tails of t + 1 rows (t fed earlier, one for this step), three rows nobody owns, NaN wherever no row lives
    -> kc, vc, q, k, v, base, max_seq and per row the oracle's (out, K row, V row) on the row's own contiguous cache (the prefix, then its tail)"""
    rng = np.random.default_rng([SEED, 4, hs, n])
    R = t + 1
    base = [S + j * R for j in range(n)]
    max_seq = S + n * R + 3
    kc = np.full((OP_HEADS, max_seq, hs), np.nan, np.float32); vc = np.full_like(kc, np.nan)
    kc[:, :S] = rng.standard_normal((OP_HEADS, S, hs)); vc[:, :S] = rng.standard_normal((OP_HEADS, S, hs))
    for b in base:
        kc[:, b:b + t] = rng.standard_normal((OP_HEADS, t, hs)); vc[:, b:b + t] = rng.standard_normal((OP_HEADS, t, hs))
    q = (rng.standard_normal((n, OP_HEADS * hs)) * 2).astype(np.float32)
    k = rng.standard_normal((n, OP_HEADS * hs)).astype(np.float32); v = rng.standard_normal((n, OP_HEADS * hs)).astype(np.float32)
    want = []
    for j, b in enumerate(base):
        kr = np.full((OP_HEADS, S + t + 3, hs), np.nan, np.float32); vr = np.full_like(kr, np.nan)
        kr[:, :S] = kc[:, :S]; vr[:, :S] = vc[:, :S]
        kr[:, S:S + t] = kc[:, b:b + t]; vr[:, S:S + t] = vc[:, b:b + t]
        o = _oracle_row(kr, vr, q[j], k[j], v[j], hs, S + t)
        want.append((o, kr[:, S + t].copy(), vr[:, S + t].copy()))
    return kc, vc, q, k, v, base, max_seq, want
