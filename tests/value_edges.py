"""Value edges for the fused paths (TEST INFRASTRUCTURE): seeded, deterministic builders of hard but FINITE inputs -- outliers, saturated and all-zero groups,
zero scales, denormals, sums of squares that overflow, peaked softmaxes, gates beyond expf's range, tied logits.  No GPU here; tests/test_value_edges_host.py proves
on the CPU that every case is NaN-free and that each family reaches the edge it is named for, tests/test_gpu_value_edges.py feeds the same cases to the kernels.

Rules the builders keep (the host test asserts them): every input is finite; no case whose reference output holds a NaN (model level: a non-finite logit) is built.
Cases dropped at design time, with the reason:
  * matmul_q with a scale pair whose product overflows (e.g. 1e20 x 1e20): an all-zero group then contributes inf * 0 = NaN.  The largest regime kept is 1e19 x 1e15
    with weights and activations of one sign per row ("inf"), where saturated rows reach +-inf and nothing cancels.
  * matmul_q regime "inf" on the mixed-sign random rows: +inf and -inf partial sums meet, NaN.  The regime keeps only its one-signed rows (see matmul_case).
  * softmax / swiglu / rmsnorm: none dropped (swiglu's a = +-3e38 against b = 1e30 gives +-inf, not NaN; a = -3e38 gives -0 through x / inf).
"""
from __future__ import annotations

import numpy as np

from fast_llama_amd import flmfile as ff, synth

F = {ff.QT_INT8: 127, ff.QT_INT16: 5792}
DT = {ff.QT_INT8: np.int8, ff.QT_INT16: np.int16}
EDGE_BASE = 200                      # the edge embedding rows are written over token ids EDGE_BASE .. EDGE_BASE + 11 (every synthetic vocabulary has >= 320 ids)
SEED = 20240611
LINEAR = (ff.T_ATTN_Q, ff.T_ATTN_K, ff.T_ATTN_V, ff.T_ATTN_O, ff.T_MLP_GATE, ff.T_MLP_UP, ff.T_MLP_DOWN)
CLS_PAIRS = ((300, 17), (319, 18), (100, 0), (257, 256))          # classifier row a is a copy of row b

FAMILIES = ("saturated", "zero", "peaked", "qk_tiny", "big_gate", "wv_tiny", "out_huge", "norm", "cls_dup", "cls_mirror")
ALL = FAMILIES                                                    # "all families at once" ("cls_equal" replaces the classifier: a model of its own)


# ---- embedding rows ------------------------------------------------------------------------------------------------------------------------------------------------
def embedding_rows(cfg):
    """-> [(name, token id, fp32 row)]: the twelve edge rows"""
    d = cfg.dim
    rng = np.random.default_rng([SEED, d])
    g = lambda: rng.standard_normal(d).astype(np.float32)          # noqa: E731
    rows = []
    x = g(); x[7] = 2000.0; x[130] = -1500.0; rows.append(("outliers", x))
    x = g(); x[64:128] = 0.0; rows.append(("zero group", x))
    rows.append(("zero row", np.zeros(d, np.float32)))
    rows.append(("x1e-20", g() * np.float32(1e-20)))
    rows.append(("x1e-41 denormal", (g().astype(np.float64) * 1e-41).astype(np.float32)))
    rows.append(("x1e15", g() * np.float32(1e15)))
    rows.append(("x1e20 sum of squares overflows", g() * np.float32(1e20)))
    rows.append(("constant +-0.75", np.where(rng.random(d) < 0.5, np.float32(0.75), np.float32(-0.75)).astype(np.float32)))
    rows.append(("wide range", (g() * np.exp2(rng.uniform(-30, 30, d))).astype(np.float32)))
    x = np.zeros(d, np.float32); x[77] = 1.0; rows.append(("one-hot", x))
    rows.append(("tiny q.k", g() * np.float32(1e-20)))              # with family "qk_tiny": the products of QK^T are denormal
    x = g(); x[d - 1] = 3000.0; x[63] = -2500.0; rows.append(("outlier at a group's last lane", x))
    out = [(name, EDGE_BASE + i, np.ascontiguousarray(r, dtype=np.float32)) for i, (name, r) in enumerate(rows)]
    assert all(np.isfinite(r).all() for _, _, r in out)
    return out


EDGE_NAMES = ("outliers", "zero group", "zero row", "x1e-20", "x1e-41 denormal", "x1e15", "x1e20 sum of squares overflows", "constant +-0.75", "wide range", "one-hot",
              "tiny q.k", "outlier at a group's last lane")
N_EDGES = len(EDGE_NAMES)
OVERFLOW_ID = EDGE_BASE + 6


def edge_id(name):
    return EDGE_BASE + EDGE_NAMES.index(name)


# ---- weight edits --------------------------------------------------------------------------------------------------------------------------------------------------
def _copy(v):
    return (v[0].copy(), v[1].copy()) if isinstance(v, tuple) else v.copy()


def weight_edits(tensors, families, cfg, copy=True):
    """-> a copy of `tensors` (copy=False: `tensors` itself, edited in place) (quantized, from synth.make_tensors) with the edge embedding rows and the named families written in, per layer and kind:
      saturated   rows 3 / 4 / 5 of every linear matrix all +F / all -F / alternating +-F, row 6 with its second group saturated
      zero        row 8 with all scales 0, row 9 with the scale of its first and last group 0, row 10 all-zero weights
      peaked      Wq scales x60 on the even heads (softmax weights under the 1e-15 skip threshold)
      qk_tiny     Wq and Wk scales x2^-10 on the last head (with the "tiny q.k" row: denormal products in QK^T)
      big_gate    W1 scales x200 (gate values beyond +-88.73: expf(-a) is +inf / 0)
      wv_tiny     Wv scales x1e-38 on the first 64 rows of head 1 (one whole quant group of the heads' output; V values and V * weight products are denormal)
      out_huge    Wo and W2 scales x1e6 on four rows (outlier channels in the residual stream, through the residual epilogue)
      norm        every norm weight vector holds 0, a run of -1.5, 40 and 1e-6
      cls_dup     classifier rows CLS_PAIRS duplicated
      cls_mirror  the classifier's upper half is a copy of its lower half (every top logit occurs twice, in two workgroups of the one-launch tail)
      cls_equal   every classifier row is row 0 (every workgroup holds a tie; the answer must be id 0)"""
    unknown = set(families) - set(FAMILIES) - {"cls_equal"}
    assert not unknown, unknown
    t = {k: _copy(v) for k, v in tensors.items()} if copy else tensors
    lim = F[cfg.quant_type]
    emb = t[(ff.T_TOKEN_EMBD, 0)]
    for _, tid, row in embedding_rows(cfg):
        emb[tid] = row
    hs = cfg.dim // cfg.n_heads
    for l in range(cfg.n_layers):
        for kind in LINEAR:
            q, s = t[(kind, l)]
            if "saturated" in families:
                q[3] = lim; q[4] = -lim
                q[5, 0::2] = lim; q[5, 1::2] = -lim
                q[6, 64:128] = lim
            if "zero" in families:
                s[8] = 0.0
                s[9, 0] = 0.0; s[9, -1] = 0.0
                q[10] = 0
        qq, sq = t[(ff.T_ATTN_Q, l)]; qk, sk = t[(ff.T_ATTN_K, l)]; qv, sv = t[(ff.T_ATTN_V, l)]
        if "peaked" in families:
            for h in range(0, cfg.n_heads, 2):
                sq[h * hs:(h + 1) * hs] *= np.float32(60.0)
        if "qk_tiny" in families:
            h = cfg.n_heads - 1
            sq[h * hs:(h + 1) * hs] *= np.float32(2.0 ** -10); sk[h * hs:(h + 1) * hs] *= np.float32(2.0 ** -10)
        if "big_gate" in families:
            t[(ff.T_MLP_GATE, l)][1][:] *= np.float32(200.0)
        if "wv_tiny" in families:
            sv[hs:hs + 64] = (sv[hs:hs + 64].astype(np.float64) * 1e-38).astype(np.float32)
        if "out_huge" in families:
            for kind in (ff.T_ATTN_O, ff.T_MLP_DOWN):
                s = t[(kind, l)][1]
                for r in (7, 130, cfg.dim - 64, cfg.dim - 1):
                    s[r] *= np.float32(1e6)
    if "norm" in families:
        for key in [(ff.T_OUTPUT_NORM, 0)] + [(k, l) for l in range(cfg.n_layers) for k in (ff.T_INPUT_NORM, ff.T_POST_NORM)]:
            w = t[key]
            w[0] = 0.0; w[64:72] = -1.5; w[130] = 40.0; w[200] = 1e-6
    q, s = t[(ff.T_CLASSIFIER, 0)]
    V = cfg.vocab_size
    if "cls_mirror" in families:
        q[V // 2:] = q[:V - V // 2]; s[V // 2:] = s[:V - V // 2]
    if "cls_dup" in families:
        for a, b in CLS_PAIRS:
            q[a] = q[b]; s[a] = s[b]
            if "cls_mirror" in families and a < V - V // 2:        # (keep the mirror image of a rewritten lower-half row its twin)
                q[a + V // 2] = q[a]; s[a + V // 2] = s[a]
    if "cls_equal" in families:
        q[:] = q[0]; s[:] = s[0]
    for v in t.values():
        for a in (v if isinstance(v, tuple) else (v,)):
            assert a.dtype.kind != "f" or np.isfinite(a).all()
    return t


_models = {}


def edge_model(shape, qt, families=ALL, layers=None, seed=4321):
    """-> (cfg, tensors) of the synthetic model `shape` with the edge rows and `families`; built once per key and shared (never modify the arrays)"""
    key = (shape, qt, tuple(families), layers, seed)
    if key not in _models:
        if shape == "7B":                                             # (close to a gigabyte each: keep one at a time)
            for k in [k for k in _models if k[0] == "7B"]:
                del _models[k]
        cfg = synth.make_config(shape, qt)
        if layers:
            cfg.n_layers = layers
        _models[key] = (cfg, weight_edits(synth.make_tensors(cfg, seed=seed), families, cfg, copy=False))
    return _models[key]


# ---- prompts -------------------------------------------------------------------------------------------------------------------------------------------------------
def short_schedule(edge):
    """[(tokens, pos)]: `[1, 50, edge, 77]` batched, then three single tokens, the edge token fed again at a decode position"""
    return [(np.array([1, 50, edge, 77], np.int32), 0), (np.array([23], np.int32), 4), (np.array([edge], np.int32), 5), (np.array([9], np.int32), 6)]


def _friendly(cfg, n, salt):
    return [int(x) for x in ((np.arange(1, n + 1) + salt) * 7919) % EDGE_BASE]      # ids below EDGE_BASE: never an edge row


def long_prompt(cfg, variant=0):
    """the ragged long prompt: 70 tokens (33 at head size 128), edge tokens at the first, a middle and the last place and straddling position 64 (the end of the
    first 64-row tile; at 33 tokens: the end of the second 16-row tile).  variant 0 / 1 takes the first / second six edge rows, and one more place pairs the two
    x1e-20 rows, the tiny query behind the tiny key: with family "qk_tiny" the batched QK^T sees denormal products."""
    n = 33 if cfg.dim // cfg.n_heads == 128 else 70
    p = _friendly(cfg, n, 11 * variant)
    slots = (0, n // 2, 63, 64, 65, n - 1) if n == 70 else (0, 8, 15, 16, 17, n - 1)
    for i, at in enumerate(slots):
        p[at] = EDGE_BASE + 6 * variant + i
    if variant == 0:
        p[slots[4] + 1] = edge_id("tiny q.k")                      # behind "x1e-20" at slots[3]
    else:
        p[slots[1] + 1] = edge_id("x1e-20")                        # in front of "tiny q.k" at slots[4]
    return np.array(p, np.int32)


def decode_schedule(cfg, variant=0):
    """[(tokens, pos)]: a 60-token friendly prompt, then single tokens at 60 .. 66 with edge tokens at positions 63, 64 and 65; variant 0 .. 3 covers the twelve rows"""
    p = _friendly(cfg, 67, 5 * variant)
    for i, at in enumerate((63, 64, 65)):
        p[at] = EDGE_BASE + 3 * variant + i
    return [(np.array(p[:60], np.int32), 0)] + [(np.array([p[i]], np.int32), i) for i in range(60, 67)]


def split_prompt(cfg):
    """300 tokens whose last 10 are edge tokens (all rows but "zero row" and "one-hot"), then three decode tokens"""
    p = _friendly(cfg, 300, 3)
    p[290:] = [edge_id(n) for n in EDGE_NAMES if n not in ("zero row", "one-hot")]
    return [(np.array(p, np.int32), 0), (np.array([edge_id("outliers")], np.int32), 300), (np.array([31], np.int32), 301), (np.array([edge_id("wide range")], np.int32), 302)]


def prompts(cfg):
    return {"short": [short_schedule(EDGE_BASE + i) for i in range(N_EDGES)], "long": [[(long_prompt(cfg, v), 0), (np.array([42], np.int32), len(long_prompt(cfg, v)))] for v in (0, 1)],
            "decode": [decode_schedule(cfg, v) for v in range(4)]}


def run_schedule(model, schedule):
    """-> the logits of every call of `schedule` on `model` (anything with forward(tokens, pos))"""
    return [model.forward(t, pos).copy() for t, pos in schedule]


# ---- op level ------------------------------------------------------------------------------------------------------------------------------------------------------
NORM_W = (0.0, -1.5, 40.0, 1e-6)


def norm_weights(n, rng):
    w = (0.8 + 0.4 * rng.random(n)).astype(np.float32)
    w[0] = 0.0; w[n // 2:n // 2 + 8] = -1.5; w[n - 1] = 40.0; w[17 % n] = 1e-6
    if n > 130:
        w[130] = 40.0
    return w


def rmsnorm_cases():
    """-> [(name, x, w)]: six x families x n in {64, 256, 4096, 4096 + 64}, against the edge norm weights"""
    out = []
    for n in (64, 256, 4096, 4096 + 64):
        rng = np.random.default_rng([SEED, 1, n])
        g = lambda: rng.standard_normal(n).astype(np.float32)      # noqa: E731
        w = norm_weights(n, rng)
        o = g(); o[7] = 2000.0; o[n - 1] = -1500.0
        fam = (("zeros", np.zeros(n, np.float32)), ("tiny", g() * np.float32(1e-20)), ("denormal", (g().astype(np.float64) * 1e-41).astype(np.float32)),
               ("huge", g() * np.float32(1e15)), ("overflowing", g() * np.float32(1e20)), ("outlier", o))
        out += [(f"{name} n={n}", x, w) for name, x in fam]
    return out


def quantize_vector(n, seed=0):
    """groups of 64 cycling through: x1e-36, 1e-42 (denormal), all zero, x1e33, constant, wide range, plain, one outlier at the last lane.  Eight kinds over groups of
    64: a 256-element wave run always mixes groups the fast quantizer takes with groups it must not (scale zero or outside [2^-100, 2^100])"""
    rng = np.random.default_rng([SEED, 2, n, seed])
    x = rng.standard_normal(n).astype(np.float32)
    for gi in range(n // 64):
        s = slice(64 * gi, 64 * gi + 64)
        k = (gi + seed) % 8
        if k == 0: x[s] *= np.float32(1e-36)
        elif k == 1: x[s] = (x[s].astype(np.float64) * 1e-42).astype(np.float32)
        elif k == 2: x[s] = 0.0
        elif k == 3: x[s] *= np.float32(1e33)
        elif k == 4: x[s] = np.where(x[s] < 0, np.float32(-0.75), np.float32(0.75))
        elif k == 5: x[s] = (x[s] * np.exp2(rng.uniform(-30, 30, 64))).astype(np.float32)
        elif k == 7: x[64 * gi + 63] = 3000.0
    return x


def quantize_cases():
    return [(f"n={n} shift={sh}", quantize_vector(n, sh)) for n in (256, 4096) for sh in (0, 1, 3)]


# scale regimes (magnitude of sW, magnitude of sX, one-signed rows only)
REGIMES = {"normal": (1e-4, 1e-2, False), "denormal": (1e-25, 1e-20, False), "straddle": (1e-22, 1e-16, False), "large": (1e15, 1e16, False), "inf": (1e19, 1e15, True)}
# "denormal": the PRODUCT sW * sX is a denormal of one to three ulps (int8: so is every output; int16: outputs of the sparse rows)


def matmul_case(qt, m, n, w, regime, seed=0):
    """-> (W, sW, X, sX): saturated, all-zero and zero-scale rows in W and in X; scales of magnitude REGIMES[regime].  Regime "inf" overflows on the saturated rows; its
    weights, activations and scales are all non-negative so that no +inf meets a -inf."""
    lim = F[qt]; dt = DT[qt]
    a, b, one_sign = REGIMES[regime]
    if regime != "denormal":
        a *= 127.0 / lim; b *= 127.0 / lim                           # (the same output magnitudes for both types: a saturated int16 group dot is 64 * 5792^2)
    rng = np.random.default_rng([SEED, 3, qt, m, n, w, seed])
    W = rng.integers(0 if one_sign else -lim, lim + 1, (m, n)).astype(dt)
    X = rng.integers(0 if one_sign else -lim, lim + 1, (w, n)).astype(dt)
    sW = (np.float32(a) * (0.5 + rng.random((m, n // 64)))).astype(np.float32)
    sX = (np.float32(b) * (0.5 + rng.random((w, n // 64)))).astype(np.float32)
    W[0] = lim; X[0] = lim                                           # saturated row x saturated row: every group dot is 64 F^2
    if m > 1: W[1] = 0 if one_sign else -lim
    if m > 2: W[2, 0::2] = lim; W[2, 1::2] = lim if one_sign else -lim
    if m > 3: W[3] = 0
    if m > 4: sW[4] = 0.0
    if m > 5: sW[5, 0] = 0.0; W[5, :64] = lim
    if m > 6: W[6, -64:] = lim
    if w > 1: X[1] = 0; sX[1] = 0.0                                  # an all-zero activation row as the quantizer leaves it (scale 0)
    if w > 2: X[2] = 0 if one_sign else -lim
    if w > 3: X[3, :64] = 0; sX[3, 0] = 0.0
    if w > 4: X[w - 1, -64:] = lim
    return W, sW, X, sX


def matmul_regimes():
    return tuple(REGIMES)


SWIGLU_A = np.array([0.0, -0.0, 30.0, -30.0, -88.0, -88.8, -89.0, -104.0, -150.0, 88.8, 104.0, 1e30, -1e30, 1e-40, -1e-40, 3e38, -3e38], np.float32)
SWIGLU_B = np.array([1.0, -2.5, 0.0, -0.0, 1e30, 1e-30], np.float32)


def swiglu_grid():
    a = np.repeat(SWIGLU_A, SWIGLU_B.size); b = np.tile(SWIGLU_B, SWIGLU_A.size)
    return a.copy(), b.copy()


def swiglu_cases():
    """-> [(name, a, b)]: the a x b grid, and n in {1, 63, 65, 11008} with the grid values scattered into Gaussian vectors"""
    ga, gb = swiglu_grid()
    out = [("grid", ga, gb)]
    for n in (1, 63, 65, 11008):
        rng = np.random.default_rng([SEED, 4, n])
        a = (rng.standard_normal(n) * 4).astype(np.float32); b = rng.standard_normal(n).astype(np.float32)
        k = min(n, ga.size)
        at = rng.choice(n, k, replace=False); pick = rng.choice(ga.size, k, replace=False)
        a[at] = ga[pick]; b[at] = gb[pick]
        out.append((f"scattered n={n}", a, b))
    return out


def softmax_cases():
    """-> [(name, x, cols)]: five families at (n, cols) in {(1, 1), (64, 64), (65, 65), (1000, 997), (1024, 1024)}"""
    out = []
    for n, cols in ((1, 1), (64, 64), (65, 65), (1000, 997), (1024, 1024)):
        rng = np.random.default_rng([SEED, 5, n])
        g = rng.standard_normal(n).astype(np.float32)
        spread = np.linspace(0, 250, n).astype(np.float32)[rng.permutation(n)]
        last = g.copy(); last[cols - 1] = 60.0
        fam = (("equal", np.full(n, 3.25, np.float32)), ("spread 250", spread), ("maximum last", last), ("x1e4", g * np.float32(1e4)), ("all -3e38", np.full(n, -3e38, np.float32)))
        out += [(f"{name} n={n}", x, cols) for name, x in fam]
    return out


ATTN_FAMILIES = ("peaked", "zero K", "V x1e30", "V x1e-41", "qk x1e-20")
ATTN_POSITIONS = (0, 1, 63, 64, 65, 257)


def attention_inputs(family, heads, hs, n):
    """-> q, k, v [n][heads][hs]: the rows fed at positions 0 .. n - 1 (row p is the query / new K / new V of position p)"""
    rng = np.random.default_rng([SEED, 6, heads, hs, ATTN_FAMILIES.index(family)])
    q = rng.standard_normal((n, heads, hs)).astype(np.float32) * 2; k = rng.standard_normal((n, heads, hs)).astype(np.float32); v = rng.standard_normal((n, heads, hs)).astype(np.float32)
    if family == "peaked": q *= np.float32(40.0)
    elif family == "zero K": k[:] = 0.0
    elif family == "V x1e30": v *= np.float32(1e30)
    elif family == "V x1e-41": v = (v.astype(np.float64) * 1e-41).astype(np.float32)
    elif family == "qk x1e-20": q *= np.float32(1e-20); k *= np.float32(1e-20)
    return q, k, v


def op_cases():
    """every op-level input, by op"""
    return {"quantize": quantize_cases(), "rmsnorm": rmsnorm_cases(), "swiglu": swiglu_cases(), "softmax": softmax_cases(),
            "matmul_q": [(qt, m, n, w, r) for qt in (ff.QT_INT8, ff.QT_INT16) for (m, n, w) in ((96, 256, 1), (96, 256, 3), (80, 192, 16), (130, 256, 17), (70, 128, 65))
                         for r in matmul_regimes()],
            "attention": [(f, hs) for f in ATTN_FAMILIES for hs in (64, 128, 32)]}


# ---- layer 0, re-derived with the oracle's op functions ---------------------------------------------------------------------------------------------------------------
def layer0_trace(cfg, tensors, tokens):
    """The layer-0 input of a token is its embedding row, so layer 0 of `tokens` (fed at positions 0 ..) can be re-derived op by op: rmsnorm -> quantize -> matmul_q ->
    rope -> scores -> softmax -> weighted sum -> Wo -> residual -> rmsnorm -> quantize -> W1.  -> a dict of the LAST token's intermediates (the tests of "each family
    bites" read it).  The score dot products are numpy's (their summation order is not the reference's; they are compared with thresholds only)."""
    import oracle_py as O
    qt, d, H = cfg.quant_type, cfg.dim, cfg.n_heads
    hs = d // H
    emb = tensors[(ff.T_TOKEN_EMBD, 0)]
    x1 = np.stack([emb[t] for t in tokens]).astype(np.float32)
    n = len(tokens)
    x2 = np.stack([O.rmsnorm(x1[i], tensors[(ff.T_INPUT_NORM, 0)]) for i in range(n)])
    qx, sx = O.quantize(x2.reshape(-1), qt)
    qx = qx.reshape(n, d); sx = sx.reshape(n, d // 64)
    mm = lambda kind, a, s: O.matmul_q(qt, tensors[(kind, 0)][0], tensors[(kind, 0)][1], a, s)      # noqa: E731
    q, k, v = mm(ff.T_ATTN_Q, qx, sx), mm(ff.T_ATTN_K, qx, sx), mm(ff.T_ATTN_V, qx, sx)
    att_out = np.zeros(d, np.float32)
    weights, products = [], []
    scale = np.float32(1.0 / np.sqrt(np.float32(hs)))
    for h in range(H):
        s = slice(h * hs, (h + 1) * hs)
        kr = np.stack([O.rope(k[i, s], i) for i in range(n)])
        qr = O.rope(q[n - 1, s], n - 1)
        products.append(kr * qr[None, :])
        sc = ((kr * qr[None, :]).sum(axis=1, dtype=np.float32) * scale).astype(np.float32)
        w = O.softmax(sc)
        weights.append(w)
        att_out[s] = O.weighted_sum(np.ascontiguousarray(v[:, s]), w.reshape(1, n))[0]
    qa, sa = O.quantize(att_out, qt)
    wo = mm(ff.T_ATTN_O, qa.reshape(1, d), sa.reshape(1, -1))[0]
    x1b = x1[n - 1] + wo
    x3 = O.rmsnorm(x1b, tensors[(ff.T_POST_NORM, 0)])
    q3, s3 = O.quantize(x3, qt)
    gate = mm(ff.T_MLP_GATE, q3.reshape(1, d), s3.reshape(1, -1))[0]
    up = mm(ff.T_MLP_UP, q3.reshape(1, d), s3.reshape(1, -1))[0]
    hd = O.swiglu(gate, up)
    qh, sh = O.quantize(hd, qt)
    return dict(x2=x2[n - 1], sx=sx[n - 1], q=q[n - 1], k=k, v=v, weights=weights, products=products, att_out=att_out, sa=sa, wo=wo, x3=x3, s3=s3, gate=gate, up=up, hd=hd, sh=sh)


# ---- model cases ------------------------------------------------------------------------------------------------------------------------------------------------------
SINGLE = tuple((f,) for f in FAMILIES) + (("cls_equal",),)


def model_cases():
    """-> [(name, shape, quant type, families, layers)]: tiny and tiny128 in both types with all families at once (and with the all-rows-equal classifier), `small`
    int8 with one family at a time, the 7B-width layer"""
    out = []
    for shape in ("tiny", "tiny128"):
        for qt in (ff.QT_INT8, ff.QT_INT16):
            out.append((f"{shape}-{'int8' if qt == ff.QT_INT8 else 'int16'}-all", shape, qt, ALL, None))
    out.append(("tiny-int8-equal", "tiny", ff.QT_INT8, ALL + ("cls_equal",), None))
    out += [(f"small-int8-{fam[0]}", "small", ff.QT_INT8, fam, None) for fam in SINGLE]
    out.append(("small-int8-all", "small", ff.QT_INT8, ALL, None))
    out += [("7B-int8-all", "7B", ff.QT_INT8, ALL, 1), ("7B-int16-all", "7B", ff.QT_INT16, ALL, 1)]
    return out


def case_schedules(name, cfg):
    """the schedules a model case runs: everything for the all-families models, the short prompts of four rows and one long prompt for the one-family models, one
    short prompt at 7B width"""
    if name.startswith("7B"):
        return [("short outliers", short_schedule(edge_id("outliers")))]
    P = prompts(cfg)
    if name.endswith("-all") or name.endswith("-equal"):
        return [(f"short {EDGE_NAMES[i]}", s) for i, s in enumerate(P["short"])] + [(f"long {i}", s) for i, s in enumerate(P["long"])] + [(f"decode {i}", s) for i, s in enumerate(P["decode"])]
    pick = ("outliers", "x1e-41 denormal", "x1e20 sum of squares overflows", "tiny q.k")
    return [(f"short {n}", P["short"][EDGE_NAMES.index(n)]) for n in pick] + [("long 0", P["long"][0])]


_logits = {}


def case_logits(case):
    """the oracle's logits of every schedule of a model case, computed once and shared (never modify them) -> {schedule name: [logits per call]}"""
    import oracle_py as O
    name, shape, qt, fam, layers = case
    if name not in _logits:
        cfg, tensors = edge_model(shape, qt, fam, layers)
        out = {}
        for sname, sch in case_schedules(name, cfg):
            out[sname] = run_schedule(O.OracleModel(cfg, tensors), sch)
        _logits[name] = out
    return _logits[name]
