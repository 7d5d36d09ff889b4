"""ctypes binding of the C ABI in include/flm_gpu.h (test and bench plumbing; not the product).

The product library is fast-llama_amd/lib/libflm_gpu.so (hand-written HIP, built by
__graft_entry__.build()).  There is NO CPU fallback: if the library is missing or a call fails,
FlmError is raised.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("FLM_GPU_LIB") or os.path.join(_HERE, "lib", "libflm_gpu.so")   # FLM_GPU_LIB: tools/variants.sh builds

QT_NONE, QT_INT16, QT_INT8 = 0, 1, 2
KCLASSES = ("embed", "qkv", "attn", "attn_o", "ffn13", "ffn2", "cls", "argmax", "allreduce", "attn_wo", "ffn", "qkv_attn_wo", "layer", "back", "layers", "token")   # from "attn_wo" on: the fused launches of the single-GPU token path ("layer": k_attn_ffn, the whole decoder layer in one launch; "back": the same without the QKV GEMV; "layers": k_layers, all layers of the token in one launch; "token": k_layers<.., TAIL>, the whole greedy token in one launch)

# every symbol include/flm_gpu.h declares (tests check the library exports all of them)
SYMBOLS = (
    "flm_comm_unique_id", "flm_ctx_create", "flm_ctx_destroy", "flm_p2p_export", "flm_p2p_import", "flm_last_error", "flm_upload_tensor",
    "flm_forward", "flm_forward_argmax", "flm_decode_greedy", "flm_decode_timed", "flm_decode_timed_each", "flm_last_tokens", "flm_reset_kv", "flm_prepare", "flm_sync",
    "flm_kernel_times", "flm_kernel_bytes", "flm_set_option", "flm_query", "flm_debug_read",
    "flm_op_quantize", "flm_op_matmul_q", "flm_op_rmsnorm", "flm_op_swiglu", "flm_op_rope", "flm_op_softmax",
    "flm_op_attention", "flm_op_expf", "flm_op_math", "flm_op_square_sum", "flm_op_argmax", "flm_op_handoff_litmus", "flm_plan_shards",
    "flm_forward_sample", "flm_decode_sample", "flm_op_sample", "flm_generate", "flm_score_tokens", "flm_op_score_rows",
    "flm_verify_greedy", "flm_generate_lookup", "flm_op_matmul_skinny", "flm_op_spec_draft",
    "flm_verify_sample", "flm_generate_lookup_sample", "flm_op_sample_rows",
    "flm_generate_ex", "flm_forward_sample_ex", "flm_op_shape_logits",
    "flm_verify_sample_ex", "flm_generate_lookup_ex", "flm_op_shape_rows",
    "flm_dfa_validate", "flm_constraint_set", "flm_constraint_arm", "flm_op_constrain_rows",
    "flm_logprobs_arm", "flm_last_logprobs", "flm_op_logprob_rows", "flm_logprob_stage_time",
    "flm_stop_validate", "flm_stop_match", "flm_stop_set", "flm_op_stop_match",
    "flm_draft_set", "flm_generate_draft",
    "flm_entropy_validate", "flm_entropy_set", "flm_entropy_mu", "flm_op_logf", "flm_op_entropy_rows",
    "flm_fan_layout_for", "flm_generate_n", "flm_fan_keep", "flm_op_attention_fan",
    "flm_batch_layout_for", "flm_batch_open", "flm_batch_join", "flm_batch_step", "flm_batch_state", "flm_batch_close", "flm_generate_batch", "flm_op_attention_slots",
    "flm_batch_plan_for", "flm_batch_admit", "flm_batch_pass", "flm_op_attention_segs",
)

# flm_score (include/flm_gpu.h): one row of flm_score_tokens / flm_op_score_rows
SCORE_DTYPE = np.dtype([("argmax", np.int32), ("target_logit", np.float32), ("max_logit", np.float32), ("sum", np.float32), ("prob", np.float32)])

# flm_logprob (include/flm_gpu.h): the record of one delivered token, 192 bytes
LOGPROBS_MAX = 20                                  # FLM_LOGPROBS_MAX
LOGPROB_SOURCES = {"raw": 0, "shaped": 1}          # FLM_LOGPROBS_RAW, FLM_LOGPROBS_SHAPED
LOGPROB_DTYPE = np.dtype([("token", np.int32), ("logit", np.float32), ("max_logit", np.float32), ("sum", np.float32), ("n_top", np.int32),
                          ("top_id", np.int32, (LOGPROBS_MAX,)), ("top_logit", np.float32, (LOGPROBS_MAX,)), ("pad_", np.int32, (3,))])

# flm_fan_cb: int (*)(void* user, int seq, int index, int32_t token, int last); a non-zero return cancels the whole call
FAN_CB = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int32, C.c_int)
FAN_MAX = 16                                       # FLM_FAN_MAX


class FanLayout(C.Structure):
    """flm_fan_layout (include/flm_gpu.h)"""
    _fields_ = [("shared_rows", C.c_int32), ("tail_rows", C.c_int32), ("n", C.c_int32), ("base", C.c_int32 * FAN_MAX)]


BATCH_MAX = 16                                     # FLM_BATCH_MAX


class BatchLayout(C.Structure):
    """flm_batch_layout (include/flm_gpu.h)"""
    _fields_ = [("n_slots", C.c_int32), ("base", C.c_int32 * BATCH_MAX), ("rows", C.c_int32 * BATCH_MAX)]


class BatchReqStruct(C.Structure):
    """flm_batch_req (include/flm_gpu.h)"""
    _fields_ = [("prompt", C.c_void_p), ("n_prompt", C.c_int32), ("max_tokens", C.c_int32), ("temperature", C.c_float), ("topp", C.c_float),
                ("rng_state", C.c_uint64), ("stop_token", C.c_int32)]


class BatchOutStruct(C.Structure):
    """flm_batch_out (include/flm_gpu.h)"""
    _fields_ = [("ids", C.c_int32 * BATCH_MAX), ("live", C.c_uint32), ("finished", C.c_uint32)]


class BatchSegStruct(C.Structure):
    """flm_batch_seg (include/flm_gpu.h)"""
    _fields_ = [("slot", C.c_int32), ("row0", C.c_int32), ("n", C.c_int32), ("pos0", C.c_int32), ("draws", C.c_int32)]


class BatchPlan(C.Structure):
    """flm_batch_plan (include/flm_gpu.h): the segments of one flm_batch_pass -- the running slots' step rows first, then the filling slots' prompt chunks"""
    _fields_ = [("n_segs", C.c_int32), ("n_rows", C.c_int32), ("n_step", C.c_int32), ("n_draws", C.c_int32), ("seg", BatchSegStruct * BATCH_MAX)]

    def segments(self):
        """-> [(slot, row0, n, pos0, draws)] of the plan's n_segs segments"""
        return [(g.slot, g.row0, g.n, g.pos0, g.draws) for g in self.seg[:self.n_segs]]


class BatchPassOutStruct(C.Structure):
    """flm_batch_pass_out (include/flm_gpu.h)"""
    _fields_ = [("ids", C.c_int32 * BATCH_MAX), ("live", C.c_uint32), ("finished", C.c_uint32), ("filling", C.c_uint32)]


@dataclasses.dataclass
class BatchReq:
    """one request of batch_join / generate_batch: what flm_generate takes for one sequence on a fresh context"""
    prompt: object
    max_tokens: int
    temperature: float = 0.0
    topp: float = 0.9
    rng_state: int = 0
    stop_token: int = -1

    def struct(self):
        """-> (flm_batch_req, the array it points into: keep it alive for the call)"""
        t = np.ascontiguousarray(self.prompt, dtype=np.int32).reshape(-1)
        if int(self.max_tokens) < 1:
            raise ValueError("batch request: max_tokens < 1")
        if t.size < 1:
            raise ValueError("batch request: an empty prompt")
        if not 0 <= int(self.rng_state) < 1 << 64:
            raise ValueError("batch request: rng_state outside 64 bits")
        return BatchReqStruct(_p(t), int(t.size), int(self.max_tokens), float(self.temperature), float(self.topp), int(self.rng_state), int(self.stop_token)), t


# flm_token_cb: int (*)(void* user, int index, int32_t token, int last); a non-zero return cancels
TOKEN_CB = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_int32, C.c_int)


# the experiment dials: the kOptDial rows of csrc/flm_tuning.h, in its order (tests/test_capi_host.py compares)
TUNING_KEYS = ("wg_per_cu", "inject_wait_failure", "age_epochs", "use_mfma", "tok_nstq", "tok_preq", "back_nst13", "back_nst13_head", "back_nst2", "back_pre13", "back_pre2", "back_ao2", "back_nwo", "attn_kpre")


PENALTY_WINDOW_MAX, BIAS_MAX = 1024, 256      # FLM_PENALTY_WINDOW_MAX, FLM_BIAS_MAX


class SamplingStruct(C.Structure):
    """flm_sampling (include/flm_gpu.h)"""
    _fields_ = [("temperature", C.c_float), ("topp", C.c_float), ("top_k", C.c_int32), ("min_p", C.c_float), ("repeat_penalty", C.c_float),
                ("frequency_penalty", C.c_float), ("presence_penalty", C.c_float), ("penalty_last_n", C.c_int32), ("n_bias", C.c_int32),
                ("bias_ids", C.c_void_p), ("bias_values", C.c_void_p)]


@dataclasses.dataclass
class Sampling:
    """the sampling controls of flm_generate_ex / flm_forward_sample_ex / flm_op_shape_logits; the defaults are the neutral values.  bias: {id: value} or (ids, values)"""
    temperature: float = 0.0
    topp: float = 0.9
    top_k: int = 0
    min_p: float = 0.0
    repeat_penalty: float = 1.0
    frequency_penalty: float = 0.0
    presence_penalty: float = 0.0
    penalty_last_n: int = 0
    bias: object = None

    def bias_arrays(self):
        if self.bias is None:
            return np.empty(0, dtype=np.int32), np.empty(0, dtype=np.float32)
        ids, vals = (list(self.bias.keys()), list(self.bias.values())) if isinstance(self.bias, dict) else self.bias
        return np.ascontiguousarray(ids, dtype=np.int32), np.ascontiguousarray(vals, dtype=np.float32)

    def struct(self):
        """-> (flm_sampling, the arrays it points into: keep them alive for the call)"""
        ids, vals = self.bias_arrays()
        st = SamplingStruct(self.temperature, self.topp, int(self.top_k), self.min_p, self.repeat_penalty, self.frequency_penalty, self.presence_penalty,
                            int(self.penalty_last_n), int(ids.size), _p(ids) if ids.size else None, _p(vals) if ids.size else None)
        return st, (ids, vals)


class FlmError(RuntimeError):
    pass


class EntropyStruct(C.Structure):
    """flm_entropy (include/flm_gpu.h)"""
    _fields_ = [("typical_p", C.c_float), ("mirostat", C.c_int32), ("tau", C.c_float), ("eta", C.c_float), ("mu", C.c_float)]


@dataclasses.dataclass
class Entropy:
    """the entropy-driven samplers of flm_entropy_set: locally typical sampling (0 < typical_p < 1) or Mirostat v2 (mirostat = 2, target entropy tau, learning rate eta,
    starting state mu; None: 2 * tau).  The defaults are off"""
    typical_p: float = 0.0
    mirostat: int = 0
    tau: float = 5.0
    eta: float = 0.1
    mu: object = None

    def struct(self):
        return EntropyStruct(self.typical_p, int(self.mirostat), self.tau, self.eta, 2.0 * self.tau if self.mu is None else self.mu)

    @property
    def mode(self):
        return 2 if self.mirostat == 2 else 1 if 0.0 < self.typical_p < 1.0 else 0


DFA_STATES_MAX, DFA_EDGES_MAX = 65536, 1 << 24      # FLM_DFA_STATES_MAX, FLM_DFA_EDGES_MAX


class DfaStruct(C.Structure):
    """flm_dfa (include/flm_gpu.h)"""
    _fields_ = [("n_states", C.c_int32), ("n_edges", C.c_int32), ("row_ptr", C.c_void_p), ("edge_token", C.c_void_p), ("edge_next", C.c_void_p)]


class Dfa:
    """A token-level deterministic automaton in CSR form (flm_dfa): the edges of state q are [row_ptr[q], row_ptr[q + 1]), their tokens strictly ascending.  Holds the three
    int32 arrays as given -- validation is flm_dfa_validate's (dfa_validate below)."""

    def __init__(self, row_ptr, edge_token, edge_next):
        self.row_ptr = np.ascontiguousarray(row_ptr, dtype=np.int32)
        self.edge_token = np.ascontiguousarray(edge_token, dtype=np.int32)
        self.edge_next = np.ascontiguousarray(edge_next, dtype=np.int32)

    @property
    def n_states(self):
        return int(self.row_ptr.size) - 1

    @property
    def n_edges(self):
        return int(self.edge_token.size)

    def struct(self):
        """-> flm_dfa pointing into this object's arrays (keep the object alive for the call)"""
        return DfaStruct(self.n_states, self.n_edges, _p(self.row_ptr), _p(self.edge_token), _p(self.edge_next))

    def edges(self, q):
        """-> (tokens, next states) of state q"""
        a, b = int(self.row_ptr[q]), int(self.row_ptr[q + 1])
        return self.edge_token[a:b], self.edge_next[a:b]

    @classmethod
    def from_edges(cls, n_states, triples):
        """(state, token, next) triples in any order -> Dfa, sorted by (state, token)"""
        tr = sorted((int(q), int(t), int(n)) for q, t, n in triples)
        row = np.zeros(int(n_states) + 1, dtype=np.int64)
        for q, _, _ in tr:
            if not 0 <= q < n_states:
                raise ValueError(f"dfa: state {q} outside [0, {n_states})")
            row[q + 1] += 1
        return cls(np.cumsum(row), [t for _, t, _ in tr], [n for _, _, n in tr])

    def save(self, path):
        """the text format: a header line `flm-dfa 1 <n_states>`, then one `state token next` line per edge"""
        with open(path, "w") as f:
            f.write(f"flm-dfa 1 {self.n_states}\n")
            for q in range(self.n_states):
                for t, n in zip(*self.edges(q)):
                    f.write(f"{q} {int(t)} {int(n)}\n")

    @classmethod
    def load(cls, path):
        """reads what save writes; the edge lines may come in any order (sorted here)"""
        with open(path) as f:
            head = f.readline().split()
            if len(head) != 3 or head[0] != "flm-dfa" or head[1] != "1":
                raise ValueError(f"{path}: not a `flm-dfa 1 <n_states>` file")
            n_states = int(head[2])
            triples = []
            for line in f:
                w = line.split()
                if not w:
                    continue
                if len(w) != 3:
                    raise ValueError(f"{path}: expected `state token next`, got {line!r}")
                triples.append((int(w[0]), int(w[1]), int(w[2])))
        return cls.from_edges(n_states, triples)

    @classmethod
    def from_choices(cls, pieces, choices, end_id):
        """"answer with one of these strings": pieces[id] = the text token id decodes to (empty / None: never allowed), choices = the strings, end_id = the token that
        ends the answer.  States are the nodes of the character trie of `choices` (state 0 = the root) plus one final state (the last); there is an edge u -> v on every
        piece that walks from u to v inside the trie; a node that completes a choice has an edge on end_id to the final state, which loops on end_id."""
        children, done = [{}], [False]
        for ch in choices:
            if not ch:
                raise ValueError("from_choices: an empty choice")
            u = 0
            for x in ch:
                if x not in children[u]:
                    children[u][x] = len(children); children.append({}); done.append(False)
                u = children[u][x]
            done[u] = True
        final = len(children)
        triples = [(final, int(end_id), final)]
        for u in range(final):
            if done[u]:
                triples.append((u, int(end_id), final))
            for tid, piece in enumerate(pieces):
                if not piece or tid == int(end_id):
                    continue
                v = u
                for x in piece:
                    v = children[v].get(x)
                    if v is None:
                        break
                if v is not None:
                    triples.append((u, tid, v))
        return cls.from_edges(final + 1, triples)


STOP_IDS_MAX, STOP_SEQS_MAX, STOP_SEQ_LEN_MAX = 64, 16, 32      # FLM_STOP_IDS_MAX, FLM_STOP_SEQS_MAX, FLM_STOP_SEQ_LEN_MAX
STOP_LENGTH, STOP_TOKEN, STOP_ID, STOP_SEQ, STOP_CANCEL = 0, 1, 2, 3, 4      # FLM_STOP_LENGTH .. FLM_STOP_CANCEL
STOP_REASONS = ("length", "stop_token", "stop_id", "stop_seq", "cancel")


class StopRulesStruct(C.Structure):
    """flm_stop_rules (include/flm_gpu.h)"""
    _fields_ = [("n_ids", C.c_int32), ("ids", C.c_void_p), ("n_seqs", C.c_int32), ("seq_ptr", C.c_void_p), ("seq_tokens", C.c_void_p)]


class StopRules:
    """A set of stop ids and stop sequences (flm_stop_rules): ids = the ids that end a call, seqs = sequences of ids that end it at their last id.  Holds the arrays as
    given -- validation is flm_stop_validate's (validate below).  raw=(ids, seq_ptr, seq_tokens) takes the three arrays as they are (the tests build broken ones)."""

    def __init__(self, ids=(), seqs=(), raw=None):
        if raw is not None:
            self.ids, self.seq_ptr, self.seq_tokens = (np.ascontiguousarray(a, dtype=np.int32) for a in raw)
            return
        seqs = [[int(t) for t in s] for s in seqs]
        self.ids = np.ascontiguousarray(list(ids), dtype=np.int32)
        self.seq_ptr = np.ascontiguousarray(np.concatenate(([0], np.cumsum([len(s) for s in seqs]))), dtype=np.int32)
        self.seq_tokens = np.ascontiguousarray([t for s in seqs for t in s], dtype=np.int32)

    @property
    def n_seqs(self):
        return max(int(self.seq_ptr.size) - 1, 0)

    @property
    def seqs(self):
        return [[int(t) for t in self.seq_tokens[self.seq_ptr[s]:self.seq_ptr[s + 1]]] for s in range(self.n_seqs)]

    def struct(self, n_ids=None, n_seqs=None):
        """-> flm_stop_rules pointing into this object's arrays (keep the object alive for the call); n_ids / n_seqs override the counts"""
        return StopRulesStruct(int(self.ids.size) if n_ids is None else int(n_ids), _p(self.ids), self.n_seqs if n_seqs is None else int(n_seqs),
                               _p(self.seq_ptr), _p(self.seq_tokens))

    def validate(self, vocab):
        """flm_stop_validate: raises FlmError naming the rule that is broken"""
        st = self.struct()
        _check(lib().flm_stop_validate(C.byref(st), int(vocab)))


def stop_match_host(rules, ids, stop_token=-1):
    """flm_stop_match, the host restatement of the stop rules (host/stop_rules.h; no GPU): -> (the first index of ids that fires or len(ids), kind, rule); rules may be None"""
    t = np.ascontiguousarray(ids, dtype=np.int32)
    st = rules.struct() if rules is not None else None
    kind, rule = C.c_int(-1), C.c_int(-1)
    first = lib().flm_stop_match(C.byref(st) if st is not None else None, C.c_int32(int(stop_token)), _p(t), int(t.size), C.byref(kind), C.byref(rule))
    return int(first), int(kind.value), int(rule.value)


def op_stop_match(rules, ids, stop_token=-1):
    """flm_op_stop_match: the device's matcher (csrc/flm_stop.h, what the shaped token form runs) on ids -> (first, kind, rule) as stop_match_host"""
    t = np.ascontiguousarray(ids, dtype=np.int32)
    st = rules.struct()
    first, kind, rule = C.c_int(-1), C.c_int(-1), C.c_int(-1)
    _check(lib().flm_op_stop_match(C.byref(st), C.c_int32(int(stop_token)), _p(t), int(t.size), C.byref(first), C.byref(kind), C.byref(rule)))
    return int(first.value), int(kind.value), int(rule.value)


def dfa_validate(dfa: Dfa, vocab: int):
    """flm_dfa_validate: raises FlmError naming the rule that failed"""
    st = dfa.struct()
    _check(lib().flm_dfa_validate(C.byref(st), int(vocab)))


class ModelDesc(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("dim", "hidden_dim", "n_layers", "n_heads", "n_kv_heads", "vocab_size",
                                          "max_seq_len", "quant_type", "quant_group_size")]


class ShardPlan(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("head_begin", "head_count", "hidden_begin", "hidden_count", "dim_begin", "dim_count", "vocab_begin", "vocab_count")]


_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise FlmError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` (no CPU fallback exists)")
        _lib = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
        _lib.flm_last_error.restype = C.c_char_p
        _lib.flm_last_error.argtypes = [C.c_void_p]
    return _lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _check(rc, ctx=None):
    if rc != 0:
        msg = lib().flm_last_error(ctx)
        raise FlmError(f"flm error {rc}: {msg.decode() if msg else ''}")


def desc_from_config(cfg, max_seq_len=1024) -> ModelDesc:
    return ModelDesc(cfg.dim, cfg.hidden_dim, cfg.n_layers, cfg.n_heads, cfg.n_kv_heads, cfg.vocab_size,
                     max_seq_len, cfg.quant_type, cfg.quant_group_size)


def plan_shards(desc: ModelDesc, rank: int, world: int) -> ShardPlan:
    out = ShardPlan()
    _check(lib().flm_plan_shards(C.byref(desc), rank, world, C.byref(out)))
    return out


def comm_unique_id() -> bytes:
    buf = C.create_string_buffer(128)
    _check(lib().flm_comm_unique_id(buf))
    return buf.raw


class Ctx:
    """flm_ctx wrapper.  tensors: {(kind, layer): fp32 ndarray | (q, scales)} as produced by synth/flmfile."""

    def __init__(self, desc: ModelDesc, device=0, rank=0, world=1, comm_id: bytes | None = None):
        self.desc = desc
        self._h = C.c_void_p()
        _check(lib().flm_ctx_create(C.byref(desc), device, rank, world, comm_id, C.byref(self._h)))

    def close(self):
        if self._h:
            lib().flm_ctx_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def p2p_export(self) -> bytes:
        buf = C.create_string_buffer(128)
        _check(lib().flm_p2p_export(self._h, buf), self._h)
        return buf.raw

    def p2p_import(self, blobs):
        raw = b"".join(blobs)
        _check(lib().flm_p2p_import(self._h, raw, len(blobs)), self._h)

    @staticmethod
    def regroup(ctxs):
        """ranks of one process: exchange the blobs again (after tensor-parallel options changed: the group's launch structure is agreed at import)"""
        blobs = [c.p2p_export() for c in ctxs]
        for c in ctxs:
            c.p2p_import(blobs)

    def upload(self, kind, layer, value):
        if isinstance(value, tuple):
            q, s = value
            q = np.ascontiguousarray(q); s = np.ascontiguousarray(s, dtype=np.float32)
            qt = QT_INT8 if q.dtype == np.int8 else QT_INT16
            _check(lib().flm_upload_tensor(self._h, kind, layer, qt, _p(q), _p(s), q.shape[0], q.shape[1]), self._h)
        else:
            v = np.ascontiguousarray(value, dtype=np.float32)
            rows, cols = v.shape if v.ndim == 2 else (1, v.shape[0])
            _check(lib().flm_upload_tensor(self._h, kind, layer, QT_NONE, _p(v), None, rows, cols), self._h)

    def upload_all(self, tensors):
        for (kind, layer), v in tensors.items():
            self.upload(kind, layer, v)

    def forward(self, tokens, pos) -> np.ndarray:
        t = np.ascontiguousarray(tokens, dtype=np.int32)
        out = np.empty(self.desc.vocab_size, dtype=np.float32)
        _check(lib().flm_forward(self._h, _p(t), len(t), int(pos), _p(out)), self._h)
        return out

    def forward_argmax(self, tokens, pos) -> int:
        t = np.ascontiguousarray(tokens, dtype=np.int32)
        nxt = C.c_int32(-1)
        _check(lib().flm_forward_argmax(self._h, _p(t), len(t), int(pos), C.byref(nxt)), self._h)
        return nxt.value

    def decode_greedy(self, first_token, pos, n_steps) -> np.ndarray:
        out = np.empty(n_steps, dtype=np.int32)
        _check(lib().flm_decode_greedy(self._h, int(first_token), int(pos), int(n_steps), _p(out)), self._h)
        return out

    def forward_sample(self, tokens, pos, temperature, topp, rng_state):
        """flm_forward_sample -> (next token, the sampler state after the draw)"""
        t = np.ascontiguousarray(tokens, dtype=np.int32)
        nxt = C.c_int32(-1); st = C.c_uint64(int(rng_state))
        _check(lib().flm_forward_sample(self._h, _p(t), len(t), int(pos), C.c_float(temperature), C.c_float(topp), C.byref(st), C.byref(nxt)), self._h)
        return nxt.value, st.value

    def decode_sample(self, first_token, pos, n_steps, temperature, topp, rng_state):
        """flm_decode_sample -> (ids[n_steps], the sampler state after the draws)"""
        out = np.empty(n_steps, dtype=np.int32); st = C.c_uint64(int(rng_state))
        _check(lib().flm_decode_sample(self._h, int(first_token), int(pos), int(n_steps), C.c_float(temperature), C.c_float(topp), C.byref(st), _p(out)), self._h)
        return out, st.value

    def _stream(self, call, max_tokens, on_token, want_ids, rng_state=0, sampling=None):
        """what the five generate* wrappers share: out_tokens / n_out / the sampler state, the trampoline around on_token (kept alive, like the Sampling's arrays, for the
        duration of the call), the call itself -- call(sp, st, cb, out, n_out), sp the flm_sampling of `sampling` or None --, a callback's exception re-raised behind it, and
        for the _ex forms (sampling given) the *n_out last_logprobs() asks for (1 where the call failed) -> (ids[n_out], the sampler state after the n_out draws)"""
        out = np.empty(max(int(max_tokens), 1), dtype=np.int32) if want_ids else None
        st = C.c_uint64(int(rng_state)); n_out = C.c_int(0)
        sp, keep = sampling.struct() if sampling is not None else (None, None)
        raised = []

        def tramp(_user, index, token, last):
            try:
                return 1 if on_token(int(index), int(token), bool(last)) else 0
            except BaseException as e:      # (an exception must not unwind through the C frames: cancel, re-raise behind the call)
                raised.append(e)
                return 1
        cb = TOKEN_CB(tramp) if on_token is not None else C.cast(None, TOKEN_CB)
        rc = call(C.byref(sp) if sp is not None else None, C.byref(st), cb, _p(out), C.byref(n_out))
        del cb, keep
        if sampling is not None:
            self._ex_n_out = int(n_out.value) if rc == 0 else 1
        if raised:
            raise raised[0]
        _check(rc, self._h)
        return (out[:n_out.value].copy() if want_ids else np.empty(0, dtype=np.int32)), st.value

    def generate(self, prompt, pos, max_tokens, temperature=0.0, topp=0.9, rng_state=0, stop_token=-1, on_token=None, want_ids=True):
        """flm_generate -> (ids[n_out], the sampler state after the n_out draws).  on_token(index, token, last) is called per token while the device computes the next
        ones; a truthy return cancels.  want_ids=False passes out_tokens = NULL (the ids then come through on_token only; the returned array is empty)."""
        t = np.ascontiguousarray(prompt, dtype=np.int32)
        return self._stream(lambda sp, st, cb, out, n_out: lib().flm_generate(
            self._h, _p(t), len(t), int(pos), int(max_tokens), C.c_float(temperature), C.c_float(topp), st, C.c_int32(int(stop_token)), cb, None, out, n_out),
            max_tokens, on_token, want_ids, rng_state)

    def generate_ex(self, prompt, pos, max_tokens, sampling, rng_state=0, stop_token=-1, on_token=None, want_ids=True):
        """flm_generate_ex: generate() with the sampling controls of a Sampling -> (ids[n_out], the sampler state after the n_out draws)"""
        t = np.ascontiguousarray(prompt, dtype=np.int32)
        return self._stream(lambda sp, st, cb, out, n_out: lib().flm_generate_ex(
            self._h, _p(t), len(t), int(pos), int(max_tokens), sp, st, C.c_int32(int(stop_token)), cb, None, out, n_out),
            max_tokens, on_token, want_ids, rng_state, sampling)

    def forward_sample_ex(self, tokens, pos, sampling, window=(), rng_state=0):
        """flm_forward_sample_ex -> (next token, the sampler state after the draw); window: the ids the penalties look at, used as given"""
        t = np.ascontiguousarray(tokens, dtype=np.int32)
        w = np.ascontiguousarray(window, dtype=np.int32)
        nxt = C.c_int32(-1); st = C.c_uint64(int(rng_state))
        sp, keep = sampling.struct()
        self._ex_n_out = 1
        _check(lib().flm_forward_sample_ex(self._h, _p(t), len(t), int(pos), C.byref(sp), _p(w) if w.size else None, int(w.size), C.byref(st), C.byref(nxt)), self._h)
        del keep
        return nxt.value, st.value

    def constraint_set(self, dfa):
        """flm_constraint_set: install or replace the automaton (None: remove it); the context is disarmed afterwards"""
        if dfa is None:
            _check(lib().flm_constraint_set(self._h, None), self._h)
            return
        st = dfa.struct()
        _check(lib().flm_constraint_set(self._h, C.byref(st)), self._h)

    def constraint_arm(self, state):
        """flm_constraint_arm: the state the _ex entry points mask in from now on (-1: disarm); query("constraint_state") reads it back"""
        _check(lib().flm_constraint_arm(self._h, C.c_int32(int(state))), self._h)

    def stop_set(self, rules):
        """flm_stop_set: install or replace the stop rules flm_generate_ex / flm_generate_lookup_ex end on (None: remove them); query("stop_rules") reads back whether any are installed"""
        if rules is None:
            _check(lib().flm_stop_set(self._h, None), self._h)
            return
        st = rules.struct()
        _check(lib().flm_stop_set(self._h, C.byref(st)), self._h)

    def stop_reason(self):
        """why the last generate-family call ended -> (STOP_LENGTH | STOP_TOKEN | STOP_ID | STOP_SEQ | STOP_CANCEL, the id's position / the sequence's index)"""
        return self.query("stop_reason"), self.query("stop_rule")

    def entropy_set(self, entropy):
        """flm_entropy_set: from now on flm_generate_ex / flm_forward_sample_ex (typical: the draft-and-verify _ex entry points too) apply the stage (None: off);
        query("entropy") reads the mode back"""
        if entropy is None:
            _check(lib().flm_entropy_set(self._h, None), self._h)
            return
        st = entropy.struct()
        _check(lib().flm_entropy_set(self._h, C.byref(st)), self._h)

    def entropy_mu(self) -> float:
        """flm_entropy_mu: Mirostat's state behind the ids delivered so far (np.float32)"""
        mu = C.c_float(0)
        _check(lib().flm_entropy_mu(self._h, C.byref(mu)), self._h)
        return np.float32(mu.value)

    def logprobs_arm(self, top_n, source="raw"):
        """flm_logprobs_arm: from now on the _ex entry points leave one record per delivered id (top_n alternatives, 0 .. 20; -1: off) from the classifier's row ("raw") or
        the row the sampler reads ("shaped"); query("logprobs_top_n") reads the setting back"""
        _check(lib().flm_logprobs_arm(self._h, int(top_n), int(LOGPROB_SOURCES.get(source, source))), self._h)

    def last_logprobs(self, first=0, n=None):
        """flm_last_logprobs -> LOGPROB_DTYPE[n]: records [first, first + n) of the last _ex call; n None: all of them from `first` on (the *n_out this wrapper saw)"""
        if n is None:
            n = max(getattr(self, "_ex_n_out", 1) - int(first), 1)      # (no _ex call through this wrapper yet: one record is asked for and the library says why not)
        out = np.zeros(int(n), dtype=LOGPROB_DTYPE)
        _check(lib().flm_last_logprobs(self._h, int(first), int(n), _p(out)), self._h)
        return out

    def logprob_stage_time(self, iters=50) -> float:
        """flm_logprob_stage_time: the mean duration in microseconds of one launch of the token form's stage, on what the last armed call left"""
        us = C.c_float(0)
        _check(lib().flm_logprob_stage_time(self._h, int(iters), C.byref(us)), self._h)
        return us.value

    def logprob_records_raw(self, n):
        """the first n record slots as the device holds them, the ones behind the last call's *n_out included (flm_debug_read 14) -> LOGPROB_DTYPE[n]"""
        out = np.empty(48 * int(n), dtype=np.float32)
        _check(lib().flm_debug_read(self._h, 14, 0, _p(out), C.c_size_t(out.size)), self._h)
        return out.view(LOGPROB_DTYPE)

    def score(self, tokens, pos, targets=None, want_logits=False):
        """flm_score_tokens -> a structured array (SCORE_DTYPE) with one row per position; with want_logits also the [n][vocab] logits.  targets None: the next token of
        the sequence, none for the last row; an entry of -1: none."""
        t = np.ascontiguousarray(tokens, dtype=np.int32)
        tg = None if targets is None else np.ascontiguousarray(targets, dtype=np.int32)
        if tg is not None and tg.size != t.size:
            raise ValueError("score: one target per token")
        out = np.zeros(len(t), dtype=SCORE_DTYPE)
        lg = np.empty((len(t), self.desc.vocab_size), dtype=np.float32) if want_logits else None
        _check(lib().flm_score_tokens(self._h, _p(t), len(t), int(pos), _p(tg), _p(out), _p(lg)), self._h)
        return (out, lg) if want_logits else out

    def verify_greedy(self, first_token, drafts, pos) -> np.ndarray:
        """flm_verify_greedy -> the m + 1 ids the decode loop started with first_token at pos produces, m = the drafts that were right (len(drafts) = k, 4..15)"""
        d = np.ascontiguousarray(drafts, dtype=np.int32)
        out = np.empty(len(d) + 1, dtype=np.int32); n_out = C.c_int(0)
        _check(lib().flm_verify_greedy(self._h, int(first_token), _p(d), len(d), int(pos), _p(out), C.byref(n_out)), self._h)
        return out[:n_out.value].copy()

    def generate_lookup(self, prompt, pos, max_tokens, stop_token=-1, draft_len=7, ngram_max=3, on_token=None, want_ids=True) -> np.ndarray:
        """flm_generate_lookup -> ids[n_out]: flm_generate at temperature 0 through draft-and-verify steps.  on_token(index, token, last) as in generate."""
        t = np.ascontiguousarray(prompt, dtype=np.int32)
        return self._stream(lambda sp, st, cb, out, n_out: lib().flm_generate_lookup(
            self._h, _p(t), len(t), int(pos), int(max_tokens), C.c_int32(int(stop_token)), int(draft_len), int(ngram_max), cb, None, out, n_out),
            max_tokens, on_token, want_ids)[0]

    def verify_sample(self, first_token, drafts, pos, temperature, topp, rng_state):
        """flm_verify_sample -> (the m + 1 ids the sampled decode loop started with first_token at pos and rng_state draws, m = the drafts that were right; the state after
        those m + 1 draws).  rng_state None: a NULL pointer (allowed at temperature 0)."""
        d = np.ascontiguousarray(drafts, dtype=np.int32)
        out = np.empty(len(d) + 1, dtype=np.int32); n_out = C.c_int(0)
        st = None if rng_state is None else C.c_uint64(int(rng_state))
        _check(lib().flm_verify_sample(self._h, int(first_token), _p(d), len(d), int(pos), C.c_float(temperature), C.c_float(topp),
                                       C.byref(st) if st is not None else None, _p(out), C.byref(n_out)), self._h)
        return out[:n_out.value].copy(), (st.value if st is not None else None)

    def generate_lookup_sample(self, prompt, pos, max_tokens, temperature=1.0, topp=0.9, rng_state=0, stop_token=-1, draft_len=7, ngram_max=3, on_token=None, want_ids=True):
        """flm_generate_lookup_sample -> (ids[n_out], the sampler state after the n_out draws): flm_generate at any temperature through draft-and-verify steps.
        on_token(index, token, last) as in generate."""
        t = np.ascontiguousarray(prompt, dtype=np.int32)
        return self._stream(lambda sp, st, cb, out, n_out: lib().flm_generate_lookup_sample(
            self._h, _p(t), len(t), int(pos), int(max_tokens), C.c_float(temperature), C.c_float(topp), st, C.c_int32(int(stop_token)), int(draft_len), int(ngram_max),
            cb, None, out, n_out), max_tokens, on_token, want_ids, rng_state)

    def verify_sample_ex(self, first_token, drafts, pos, sampling, window=(), rng_state=0):
        """flm_verify_sample_ex -> (the m + 1 ids a flm_forward_sample_ex loop started with first_token at pos draws when it slides `window` over them, m = the drafts that
        were right; the state after those draws).  rng_state None: a NULL pointer (allowed at temperature 0)."""
        d = np.ascontiguousarray(drafts, dtype=np.int32)
        w = np.ascontiguousarray(window, dtype=np.int32)
        out = np.empty(len(d) + 1, dtype=np.int32); n_out = C.c_int(0)
        st = None if rng_state is None else C.c_uint64(int(rng_state))
        sp, keep = sampling.struct()
        _check(lib().flm_verify_sample_ex(self._h, int(first_token), _p(d), len(d), int(pos), C.byref(sp), _p(w) if w.size else None, int(w.size),
                                          C.byref(st) if st is not None else None, _p(out), C.byref(n_out)), self._h)
        del keep
        self._ex_n_out = int(n_out.value)
        return out[:n_out.value].copy(), (st.value if st is not None else None)

    def generate_lookup_ex(self, prompt, pos, max_tokens, sampling, rng_state=0, stop_token=-1, draft_len=7, ngram_max=3, on_token=None, want_ids=True):
        """flm_generate_lookup_ex -> (ids[n_out], the sampler state after the n_out draws): flm_generate_ex through draft-and-verify steps.
        on_token(index, token, last) as in generate."""
        t = np.ascontiguousarray(prompt, dtype=np.int32)
        return self._stream(lambda sp, st, cb, out, n_out: lib().flm_generate_lookup_ex(
            self._h, _p(t), len(t), int(pos), int(max_tokens), sp, st, C.c_int32(int(stop_token)), int(draft_len), int(ngram_max), cb, None, out, n_out),
            max_tokens, on_token, want_ids, rng_state, sampling)

    def generate_n(self, prompt, pos, max_tokens, states=None, n=None, temperature=0.0, topp=0.9, stop_token=-1, on_token=None):
        """flm_generate_n: n completions of one prompt, one batch per pass over the weights -> (a list of n id arrays, the n sampler states after each sequence's draws).
        states: the n sequences' sampler states (n = len(states)); None with n given: a NULL pointer (temperature 0 only; the returned states are None).
        on_token(seq, index, token, last) is called per delivered id; a truthy return cancels the whole call."""
        if states is None:
            if n is None:
                raise ValueError("generate_n: give the sequences' states, or n at temperature 0")
            if temperature != 0:
                raise ValueError("generate_n: states must be given at temperature != 0")
        else:
            if n is not None and int(n) != len(states):
                raise ValueError("generate_n: n differs from len(states)")
            n = len(states)
        n = int(n)
        if not 2 <= n <= FAN_MAX:
            raise ValueError(f"generate_n: n = {n} outside 2 .. {FAN_MAX}")
        if int(max_tokens) < 1:
            raise ValueError("generate_n: max_tokens < 1")
        t = np.ascontiguousarray(prompt, dtype=np.int32)
        st = None if states is None else np.array([int(x) for x in states], dtype=np.uint64)
        out = np.full((n, int(max_tokens)), -1, dtype=np.int32); n_out = np.zeros(n, dtype=np.int32)
        raised = []

        def tramp(_user, seq, index, token, last):
            try:
                return 1 if on_token(int(seq), int(index), int(token), bool(last)) else 0
            except BaseException as e:      # (an exception must not unwind through the C frames: cancel, re-raise behind the call)
                raised.append(e)
                return 1
        cb = FAN_CB(tramp) if on_token is not None else C.cast(None, FAN_CB)
        rc = lib().flm_generate_n(self._h, _p(t), len(t), int(pos), int(max_tokens), n, C.c_float(temperature), C.c_float(topp), _p(st),
                                  C.c_int32(int(stop_token)), cb, None, _p(out), _p(n_out))
        del cb
        if raised:
            raise raised[0]
        _check(rc, self._h)
        return [out[j, :n_out[j]].copy() for j in range(n)], (None if st is None else [int(x) for x in st])

    def fan_keep(self, seq):
        """flm_fan_keep: move sequence `seq`'s tail of the last generate_n behind the shared rows; any entry point continues from pos + n_prompt + n_out[seq] - 1"""
        _check(lib().flm_fan_keep(self._h, int(seq)), self._h)

    def batch_open(self, layout):
        """flm_batch_open: divide the cache into the layout's slots (batch_layout) and empty them all; launches nothing"""
        _check(lib().flm_batch_open(self._h, C.byref(layout)), self._h)

    def batch_join(self, slot, req):
        """flm_batch_join: the request's prompt enters the empty slot `slot` -> (token 0, whether the slot is live behind it)"""
        st, keep = req.struct()
        first = C.c_int32(-1); live = C.c_int(0)
        _check(lib().flm_batch_join(self._h, int(slot), C.byref(st), C.byref(first), C.byref(live)), self._h)
        del keep
        return int(first.value), bool(live.value)

    def batch_step(self):
        """flm_batch_step: one pass over the weights for all live slots -> (ids[BATCH_MAX] by slot, -1 where a slot delivered nothing; the live mask behind the step; the
        mask of the slots whose last id is in it)"""
        out = BatchOutStruct()
        _check(lib().flm_batch_step(self._h, C.byref(out)), self._h)
        return np.array(out.ids[:], dtype=np.int32), int(out.live), int(out.finished)

    def batch_admit(self, slot, req):
        """flm_batch_admit: the request is recorded in the empty slot `slot`, which is filling from now on; launches nothing.  The library reads the prompt's ids until
        the slot has delivered its token 0: this object keeps them alive until then (or until the next batch_open / close)"""
        st, keep = req.struct()
        _check(lib().flm_batch_admit(self._h, int(slot), C.byref(st)), self._h)
        if not hasattr(self, "_admitted"):
            self._admitted = {}
        self._admitted[int(slot)] = keep

    def batch_pass(self, prompt_rows_max=0):
        """flm_batch_pass: one pass over the weights -- every running slot's step row and up to prompt_rows_max rows (0: no bound) of the filling slots' prompts ->
        (ids[BATCH_MAX] by slot: a running slot's next id, token 0 of a slot whose prompt completed, -1 otherwise; the running mask behind the pass; the mask of the slots
        whose last id is in it; the mask of the slots still filling)"""
        out = BatchPassOutStruct()
        _check(lib().flm_batch_pass(self._h, int(prompt_rows_max), C.byref(out)), self._h)
        held = getattr(self, "_admitted", {})
        for s in [s for s in held if not (out.filling >> s) & 1]:
            del held[s]
        return np.array(out.ids[:], dtype=np.int32), int(out.live), int(out.finished), int(out.filling)

    def batch_state(self, slot):
        """flm_batch_state -> (the sampler state behind the slot's delivered ids, their count, FLM_STOP_TOKEN (1) / FLM_STOP_LENGTH (0); 0 while the slot runs)"""
        st = C.c_uint64(0); n = C.c_int(0); why = C.c_int(0)
        _check(lib().flm_batch_state(self._h, int(slot), C.byref(st), C.byref(n), C.byref(why)), self._h)
        return int(st.value), int(n.value), int(why.value)

    def batch_close(self, keep_slot=-1):
        """flm_batch_close: end the batch; keep_slot >= 0: that slot's rows move to [0, len) and any entry point continues its conversation from pos = len"""
        _check(lib().flm_batch_close(self._h, int(keep_slot)), self._h)

    def generate_batch(self, reqs, on_token=None):
        """flm_generate_batch: the requests (BatchReq, 1 .. BATCH_MAX of them) served together, one batch per pass over the weights -> (a list of id arrays, the sampler
        states after each request's draws).  on_token(seq, index, token, last) is called per delivered id; a truthy return ends the call behind that step."""
        reqs = list(reqs)
        n = len(reqs)
        if not 1 <= n <= BATCH_MAX:
            raise ValueError(f"generate_batch: {n} requests outside 1 .. {BATCH_MAX}")
        pairs = [r.struct() for r in reqs]
        arr = (BatchReqStruct * n)(*[p[0] for p in pairs])
        stride = max(int(r.max_tokens) for r in reqs)
        out = np.full((n, stride), -1, dtype=np.int32); n_out = np.zeros(n, dtype=np.int32); st = np.zeros(n, dtype=np.uint64)
        raised = []

        def tramp(_user, seq, index, token, last):
            try:
                return 1 if on_token(int(seq), int(index), int(token), bool(last)) else 0
            except BaseException as e:      # (an exception must not unwind through the C frames: cancel, re-raise behind the call)
                raised.append(e)
                return 1
        cb = FAN_CB(tramp) if on_token is not None else C.cast(None, FAN_CB)
        rc = lib().flm_generate_batch(self._h, arr, n, cb, None, _p(out), stride, _p(n_out), _p(st))
        del cb, pairs
        if raised:
            raise raised[0]
        _check(rc, self._h)
        return [out[j, :n_out[j]].copy() for j in range(n)], [int(x) for x in st]

    def draft_set(self, draft):
        """flm_draft_set: pair this (target) context with the draft context `draft` for generate_draft (None: detach).  The target does not own the draft: detach before
        closing either"""
        _check(lib().flm_draft_set(self._h, draft._h if draft is not None else None), self._h)
        self._draft = draft      # (kept alive while attached)

    def generate_draft(self, prompt, pos, max_tokens, sampling, rng_state=0, stop_token=-1, draft_len=7, on_token=None, want_ids=True):
        """flm_generate_draft -> (ids[n_out], the sampler state after the n_out draws): flm_generate_ex through draft-and-verify steps drafted by the attached draft
        context.  sampling None: a NULL struct (every control neutral, temperature 0).  on_token(index, token, last) as in generate."""
        t = np.ascontiguousarray(prompt, dtype=np.int32)
        ids, st = self._stream(lambda sp, st, cb, out, n_out: lib().flm_generate_draft(
            self._h, _p(t), len(t), int(pos), int(max_tokens), sp, st, C.c_int32(int(stop_token)), int(draft_len), cb, None, out, n_out),
            max_tokens, on_token, want_ids, rng_state, sampling)
        if sampling is None:
            self._ex_n_out = max(len(ids), 1)
        return ids, st

    def decode_timed(self, first_token, pos, n_steps) -> float:
        ms = C.c_float(0)
        _check(lib().flm_decode_timed(self._h, int(first_token), int(pos), int(n_steps), C.byref(ms)), self._h)
        return ms.value

    def decode_timed_each(self, first_token, pos, n_steps) -> np.ndarray:
        ms = np.zeros(n_steps, dtype=np.float32)
        _check(lib().flm_decode_timed_each(self._h, int(first_token), int(pos), int(n_steps), _p(ms)), self._h)
        return ms

    def last_tokens(self, n) -> np.ndarray:
        out = np.empty(n, dtype=np.int32)
        _check(lib().flm_last_tokens(self._h, int(n), _p(out)), self._h)
        return out

    def reset_kv(self):
        _check(lib().flm_reset_kv(self._h), self._h)

    def prepare(self):
        """build every argument block / token graph now (flm_prepare): nothing is left to allocate inside a forward"""
        _check(lib().flm_prepare(self._h), self._h)

    def sync(self):
        _check(lib().flm_sync(self._h), self._h)

    def set_option(self, key, value, unlock=True):
        """flm_set_option.  The experiment dials (csrc/flm_tuning.h) are not part of the boundary: the library refuses them until option "tuning" is 1 -- the tests and
        tools that sweep them go through here, which unlocks them first (unlock=False: the raw call, as a deployment would make it)."""
        if unlock and key in TUNING_KEYS and not self.query("tuning"):
            _check(lib().flm_set_option(self._h, b"tuning", 1), self._h)
        _check(lib().flm_set_option(self._h, key.encode(), int(value)), self._h)

    def query(self, key) -> int:
        v = C.c_int(0)
        _check(lib().flm_query(self._h, key.encode(), C.byref(v)), self._h)
        return int(v.value)

    def age_epochs(self, e):
        """option "age_epochs": the device state of a context whose epoch counters stand at the 32-bit value `e` (csrc/flm_tuning.h)"""
        e &= 0xFFFFFFFF
        self.set_option("age_epochs", e - (1 << 32) if e >= 1 << 31 else e)

    def epochs(self):
        """the epoch counters as unsigned values: (the one-launch token's, the token's epoch base, k_xchg's logits exchanges)"""
        return tuple(self.query(k) & 0xFFFFFFFF for k in ("epoch_tail", "epoch_eng", "epoch_xchg"))

    def epoch_words(self, what, n):
        """the never-cleared flag lines ("lines") / granule tags ("tags") that count from the epoch counters, as uint32 (flm_debug_read 11 / 12)"""
        out = np.empty(n, dtype=np.float32)
        _check(lib().flm_debug_read(self._h, {"lines": 11, "tags": 12}[what], 0, _p(out), C.c_size_t(n)), self._h)
        return out.view(np.uint32)

    def gen_ring(self, n):
        """the first n granules of flm_generate's ring as the last call left them (flm_debug_read 13) -> (tokens, last bits, tags)"""
        out = np.empty(2 * n, dtype=np.float32)
        _check(lib().flm_debug_read(self._h, 13, 0, _p(out), C.c_size_t(2 * n)), self._h)
        w = out.view(np.uint32).reshape(n, 2)
        return (w[:, 0] & 0x7FFFFFFF).astype(np.int64), (w[:, 0] >> 31).astype(np.int64), w[:, 1].astype(np.int64)

    def debug_read(self, what, layer, n):
        names = {"x1": 0, "q": 1, "att_out": 2, "hd": 3, "kcache": 4, "vcache": 5, "logits": 6, "trace": 7, "trace_abs": 8, "back_trace": 10}
        out = np.empty(n, dtype=np.float32)
        _check(lib().flm_debug_read(self._h, names[what], int(layer), _p(out), C.c_size_t(n)), self._h)
        return out

    def kernel_times(self, pos, iters=3):
        avg = np.zeros(len(KCLASSES), dtype=np.float32); cnt = np.zeros(len(KCLASSES), dtype=np.int32)
        _check(lib().flm_kernel_times(self._h, int(pos), int(iters), _p(avg), _p(cnt)), self._h)
        return {k: (float(avg[i]), int(cnt[i])) for i, k in enumerate(KCLASSES)}

    def kernel_bytes(self, kclass, pos) -> float:
        b = C.c_double(0)
        _check(lib().flm_kernel_bytes(self._h, KCLASSES.index(kclass), int(pos), C.byref(b)), self._h)
        return b.value


# ---- op level ---------------------------------------------------------------------------------
def op_quantize(x, qt, gs=64):
    x = np.ascontiguousarray(x, dtype=np.float32)
    q = np.empty(x.size, dtype=np.int8 if qt == QT_INT8 else np.int16)
    s = np.empty(x.size // gs, dtype=np.float32)
    _check(lib().flm_op_quantize(qt, _p(q), _p(s), _p(x), C.c_size_t(x.size), gs))
    return q, s


def op_matmul_q(qt, W, sW, X, sX, gs=64):
    W = np.ascontiguousarray(W); X = np.ascontiguousarray(X)
    sW = np.ascontiguousarray(sW, dtype=np.float32); sX = np.ascontiguousarray(sX, dtype=np.float32)
    m, n = W.shape; w = X.shape[0]
    out = np.empty((w, m), dtype=np.float32)
    _check(lib().flm_op_matmul_q(qt, _p(out), _p(W), _p(sW), _p(X), _p(sX), m, n, w, gs))
    return out


def op_matmul_skinny(W, sW, X, sX, gs=64):
    """flm_op_matmul_skinny: the verify pass's int8 GEMM (k_gemm_q8_skinny), 1 <= X.shape[0] <= 16 -> out[w][m]"""
    W = np.ascontiguousarray(W, dtype=np.int8); X = np.ascontiguousarray(X, dtype=np.int8)
    sW = np.ascontiguousarray(sW, dtype=np.float32); sX = np.ascontiguousarray(sX, dtype=np.float32)
    m, n = W.shape; w = X.shape[0]
    out = np.empty((w, m), dtype=np.float32)
    _check(lib().flm_op_matmul_skinny(QT_INT8, _p(out), _p(W), _p(sW), _p(X), _p(sX), m, n, w, gs))
    return out


def op_spec_draft(history, k, ngram_max) -> np.ndarray:
    """k_spec_draft, the device's prompt-lookup drafter, on a history -> d[k]"""
    h = np.ascontiguousarray(history, dtype=np.int32)
    d = np.empty(int(k), dtype=np.int32)
    _check(lib().flm_op_spec_draft(_p(h), len(h), int(k), int(ngram_max), _p(d)))
    return d


_host = None


def spec_draft_host(history, k, ngram_max) -> np.ndarray:
    """the drafter's host restatement (host/spec_draft.h through lib/libflm_host.so: fh_spec_draft); needs no GPU"""
    global _host
    if _host is None:
        _host = C.CDLL(os.path.join(_HERE, "lib", "libflm_host.so"))
    h = np.ascontiguousarray(history, dtype=np.int32)
    d = np.empty(int(k), dtype=np.int32)
    _host.fh_spec_draft(_p(h), len(h), int(k), int(ngram_max), _p(d))
    return d


def op_argmax(logits) -> int:
    a = np.ascontiguousarray(logits, dtype=np.float32)
    idx = C.c_int32(-1)
    _check(lib().flm_op_argmax(_p(a), int(a.size), C.byref(idx)))
    return idx.value


def op_sample(logits, temperature, topp, rng_state):
    """Sampler::sample through k_sample_advance -> (token, the sampler state after the draw); logits are not modified"""
    a = np.ascontiguousarray(logits, dtype=np.float32)
    out = C.c_int32(-1); st = C.c_uint64(int(rng_state))
    _check(lib().flm_op_sample(_p(a), int(a.size), C.c_float(temperature), C.c_float(topp), C.byref(st), C.byref(out)))
    return out.value, st.value


def op_shape_logits(logits, sampling, window=()) -> np.ndarray:
    """k_shape_logits, the shaping stage of flm_generate_ex, on one row of logits -> the shaped row"""
    a = np.ascontiguousarray(logits, dtype=np.float32)
    w = np.ascontiguousarray(window, dtype=np.int32)
    out = np.empty_like(a)
    sp, keep = sampling.struct()
    _check(lib().flm_op_shape_logits(_p(a), int(a.size), C.byref(sp), _p(w) if w.size else None, int(w.size), _p(out)))
    del keep
    return out


def row_windows(window, drafts, last_n):
    """the windows of a verify batch's rows: row r looks at the last min(last_n, len(window) + r) ids of window ++ drafts[0 .. r), r = 0 .. len(drafts) (pure Python; with
    shape_host the host restatement of k_shape_rows)"""
    base = [int(x) for x in window]
    d = [int(x) for x in drafts]
    out = []
    for r in range(len(d) + 1):
        h = base + d[:r]
        w = min(int(last_n), len(h))
        out.append(np.array(h[len(h) - w:] if w > 0 else [], dtype=np.int32))
    return out


def op_shape_rows(logits, n, sampling, window=(), drafts=()) -> np.ndarray:
    """k_shape_rows, the shaper of a verify batch under the controls, on logits[rows][ld], the first n entries of each row -> the shaped rows [rows][n]; row r over the last
    min(penalty_last_n, len(window) + r) ids of window ++ drafts[0 .. r) (drafts: rows - 1 ids)"""
    a = np.ascontiguousarray(logits, dtype=np.float32)
    a = a.reshape(1, -1) if a.ndim == 1 else a
    w = np.ascontiguousarray(window, dtype=np.int32)
    d = np.ascontiguousarray(drafts, dtype=np.int32)
    if d.size != a.shape[0] - 1:
        raise ValueError("op_shape_rows: rows - 1 drafts")
    out = np.empty((a.shape[0], int(n)), dtype=np.float32)
    sp, keep = sampling.struct()
    _check(lib().flm_op_shape_rows(_p(a), int(a.shape[0]), int(a.shape[1]), int(n), C.byref(sp), _p(w) if w.size else None, int(w.size), _p(d) if d.size else None, _p(out)))
    del keep
    return out


def op_constrain_rows(logits, n, sampling, dfa, state, window=(), drafts=()):
    """k_shape_rows with the constraint's step 0 on logits[rows][ld] -> (the shaped rows [rows][n], states[rows]): row r masked in delta folded over drafts[0 .. r) from `state`"""
    a = np.ascontiguousarray(logits, dtype=np.float32)
    a = a.reshape(1, -1) if a.ndim == 1 else a
    w = np.ascontiguousarray(window, dtype=np.int32)
    d = np.ascontiguousarray(drafts, dtype=np.int32)
    if d.size != a.shape[0] - 1:
        raise ValueError("op_constrain_rows: rows - 1 drafts")
    out = np.empty((a.shape[0], int(n)), dtype=np.float32)
    states = np.full(a.shape[0], -2, dtype=np.int32)
    sp, keep = sampling.struct()
    st = dfa.struct()
    _check(lib().flm_op_constrain_rows(_p(a), int(a.shape[0]), int(a.shape[1]), int(n), C.byref(sp), _p(w) if w.size else None, int(w.size), _p(d) if d.size else None,
                                       C.byref(st), C.c_int32(int(state)), _p(out), _p(states)))
    del keep
    return out, states


def _host_lib():
    global _host
    if _host is None:
        _host = C.CDLL(os.path.join(_HERE, "lib", "libflm_host.so"))
    return _host


def constrain_host(logits, tokens) -> np.ndarray:
    """step 0's host restatement (host/sampler.cpp constrain_logits through lib/libflm_host.so: fh_constrain): -inf wherever the index is not in `tokens` (ascending); no GPU"""
    a = np.ascontiguousarray(logits, dtype=np.float32)
    t = np.ascontiguousarray(tokens, dtype=np.int32)
    out = np.empty_like(a)
    _host_lib().fh_constrain(_p(a), int(a.size), _p(t), int(t.size), _p(out))
    return out


def dfa_next_host(dfa: Dfa, q, t) -> int:
    """delta(q, t) through the host restatement (host/sampler.cpp dfa_next: fh_dfa_next); no GPU"""
    return int(_host_lib().fh_dfa_next(_p(dfa.row_ptr), _p(dfa.edge_token), _p(dfa.edge_next), int(q), int(t)))


def shape_host(logits, sampling, window=()) -> np.ndarray:
    """the shaping stage's host restatement (host/sampler.cpp shape_logits through lib/libflm_host.so: fh_shape); needs no GPU"""
    global _host
    if _host is None:
        _host = C.CDLL(os.path.join(_HERE, "lib", "libflm_host.so"))
    a = np.ascontiguousarray(logits, dtype=np.float32)
    w = np.ascontiguousarray(window, dtype=np.int32)
    ids, vals = sampling.bias_arrays()
    out = np.empty_like(a)
    _host.fh_shape(_p(a), int(a.size), C.c_float(sampling.temperature), int(sampling.top_k), C.c_float(sampling.min_p), C.c_float(sampling.repeat_penalty),
                   C.c_float(sampling.frequency_penalty), C.c_float(sampling.presence_penalty), int(ids.size), _p(ids), _p(vals), _p(w), int(w.size), _p(out))
    return out


def entropy_validate(entropy):
    """flm_entropy_validate (pure host arithmetic): raises FlmError naming the rule that failed"""
    st = entropy.struct()
    _check(lib().flm_entropy_validate(C.byref(st)))


def op_logf(x) -> np.ndarray:
    """flm_logf as the device evaluates it, over positive normal floats"""
    a = np.array(x, dtype=np.float32, copy=True).reshape(-1)
    _check(lib().flm_op_logf(_p(a), C.c_size_t(a.size)))
    return a


def logf_host(x) -> np.ndarray:
    """flm_logf as the host compiles it (csrc/flm_logf.h through lib/libflm_host.so: fh_logf); needs no GPU"""
    a = np.array(x, dtype=np.float32, copy=True).reshape(-1)
    _host_lib().fh_logf(_p(a), C.c_size_t(a.size))
    return a


def entropy_host(logits, temperature, entropy, mu=None, chosen=None):
    """the entropy-driven stages' host restatement (host/sampler.cpp entropy_logits / mirostat_update through lib/libflm_host.so) on one row; needs no GPU.
    -> the masked row; with chosen (Mirostat): (the masked row, obs, the updated mu) as np.float32.  mu None: entropy's starting state"""
    a = np.ascontiguousarray(logits, dtype=np.float32).reshape(-1)
    st = entropy.struct()
    m = st.mu if mu is None else mu
    out = np.empty_like(a)
    h = _host_lib()
    h.fh_entropy(_p(a), int(a.size), C.c_float(temperature), C.c_float(st.typical_p), int(st.mirostat), C.c_float(m), _p(out))
    if chosen is None:
        return out
    h.fh_mirostat_update.restype = C.c_float
    obs = C.c_float(0)
    m2 = h.fh_mirostat_update(_p(out), int(a.size), C.c_float(temperature), int(chosen), C.c_float(st.tau), C.c_float(st.eta), C.c_float(m), C.byref(obs))
    return out, np.float32(obs.value), np.float32(m2)


def op_entropy_rows(logits, n, temperature, entropy, mu=None, chosen=None):
    """k_entropy_rows on logits[rows][ld], the first n entries of each row -> the masked rows [rows][n]; Mirostat: mu[rows] the rows' states, and with chosen[rows]
    -> (the masked rows, obs[rows], the updated mu[rows])"""
    a = np.ascontiguousarray(logits, dtype=np.float32)
    a = a.reshape(1, -1) if a.ndim == 1 else a
    rows = int(a.shape[0])
    st = entropy.struct()
    m = None if mu is None else np.ascontiguousarray(np.broadcast_to(np.asarray(mu, dtype=np.float32), (rows,)))
    ch = None if chosen is None else np.ascontiguousarray(chosen, dtype=np.int32).reshape(-1)
    out = np.empty((rows, int(n)), dtype=np.float32)
    obs = np.zeros(rows, dtype=np.float32); mu2 = np.zeros(rows, dtype=np.float32)
    _check(lib().flm_op_entropy_rows(_p(a), rows, int(a.shape[1]), int(n), C.c_float(temperature), C.byref(st), _p(m), _p(ch), _p(out), _p(obs), _p(mu2)))
    return out if chosen is None else (out, obs, mu2)


def op_sample_rows(logits, n, temperature, topp, rng_state):
    """k_sample_rows on logits[rows][ld], the first n entries of each row -> (ids[rows], the sampler state after `rows` draws): row i with the (i + 1)-th coin"""
    a = np.ascontiguousarray(logits, dtype=np.float32)
    a = a.reshape(1, -1) if a.ndim == 1 else a
    out = np.full(a.shape[0], -1, dtype=np.int32); st = C.c_uint64(int(rng_state))
    _check(lib().flm_op_sample_rows(_p(a), int(a.shape[0]), int(a.shape[1]), int(n), C.c_float(temperature), C.c_float(topp), C.byref(st), _p(out)))
    return out, st.value


def op_score_rows(logits, targets=None):
    """k_score_rows on logits[rows][n] -> SCORE_DTYPE[rows]; targets[rows] (-1 / None: no target)"""
    a = np.ascontiguousarray(logits, dtype=np.float32)
    a = a.reshape(1, -1) if a.ndim == 1 else a
    tg = None if targets is None else np.ascontiguousarray(targets, dtype=np.int32).reshape(-1)
    if tg is not None and tg.size != a.shape[0]:
        raise ValueError("op_score_rows: one target per row")
    out = np.zeros(a.shape[0], dtype=SCORE_DTYPE)
    _check(lib().flm_op_score_rows(_p(a), int(a.shape[0]), int(a.shape[1]), _p(tg), _p(out)))
    return out


def op_logprob_rows(logits, n, chosen, top_n):
    """k_logprob_rows on logits[rows][ld], the first n entries of each row -> LOGPROB_DTYPE[rows]: row r's record with drawn id chosen[r]"""
    a = np.ascontiguousarray(logits, dtype=np.float32)
    a = a.reshape(1, -1) if a.ndim == 1 else a
    ch = np.ascontiguousarray(chosen, dtype=np.int32).reshape(-1)
    if ch.size != a.shape[0]:
        raise ValueError("op_logprob_rows: one drawn id per row")
    out = np.zeros(a.shape[0], dtype=LOGPROB_DTYPE)
    _check(lib().flm_op_logprob_rows(_p(a), int(a.shape[0]), int(a.shape[1]), int(n), _p(ch), int(top_n), _p(out)))
    return out


def logprob_host(logits, chosen, top_n):
    """the record's host restatement (host/sampler.cpp logprob_row through lib/libflm_host.so: fh_logprob_row) on one row -> LOGPROB_DTYPE[1]; needs no GPU"""
    a = np.ascontiguousarray(logits, dtype=np.float32).reshape(-1)
    out = np.zeros(1, dtype=LOGPROB_DTYPE)
    _host_lib().fh_logprob_row(_p(a), int(a.size), int(chosen), int(top_n), _p(out))
    return out


def logprob_values(rec):
    """float64 log-probabilities from flm_logprob records, (logit - max_logit) - log(sum) evaluated in double from the bit-exact ingredients
    -> (logprob[rows], top_logprob[rows][20]); -inf where the logit is -inf, NaN in the top slots at and beyond n_top"""
    r = np.atleast_1d(np.asarray(rec))
    mx = r["max_logit"].astype(np.float64); ls = np.log(r["sum"].astype(np.float64))
    with np.errstate(invalid="ignore"):
        lp = (r["logit"].astype(np.float64) - mx) - ls
        top = (r["top_logit"].astype(np.float64) - mx[:, None]) - ls[:, None]
    lp[np.isneginf(r["logit"])] = -np.inf
    top[np.isneginf(r["top_logit"])] = -np.inf
    top[np.arange(LOGPROBS_MAX)[None, :] >= r["n_top"][:, None]] = np.nan
    return lp, top


def nll(scores, targets=None):
    """per-position natural-log loss in float64 from flm_score rows, -((target_logit - max_logit) - log(sum)) -- the UNCLIPPED log-probability, finite where the sampler's
    clipped prob is 0 --, and its mean over the rows that have a target.  targets: what was passed to score (rows with -1 have none); None: every row but the last has one.
    -> (loss[n] with NaN where a row has no target, mean)"""
    s = np.asarray(scores)
    valid = np.ones(s.shape[0], dtype=bool)
    if targets is None:
        valid[-1:] = False
    else:
        valid = np.asarray(targets).reshape(-1) >= 0
    loss = np.full(s.shape[0], np.nan, dtype=np.float64)
    loss[valid] = -((s["target_logit"][valid].astype(np.float64) - s["max_logit"][valid].astype(np.float64)) - np.log(s["sum"][valid].astype(np.float64)))
    return loss, (float(loss[valid].mean()) if valid.any() else float("nan"))


def op_handoff_litmus(rounds):
    """(wrong values read, waits timed out) after `rounds` rounds of the fused launches' publish / poll / coherent-read sequence"""
    bad, to = C.c_int(0), C.c_int(0)
    _check(lib().flm_op_handoff_litmus(int(rounds), C.byref(bad), C.byref(to)))
    return bad.value, to.value


def op_rmsnorm(x, w):
    x = np.ascontiguousarray(x, dtype=np.float32); w = np.ascontiguousarray(w, dtype=np.float32)
    o = np.empty_like(x)
    _check(lib().flm_op_rmsnorm(_p(o), _p(x), _p(w), C.c_size_t(x.size)))
    return o


def op_square_sum(x):
    """-> (total from the speculative wave evaluation, total from the sequential chains, the 4 strided partial sums)"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    o = np.empty(6, dtype=np.float32)
    _check(lib().flm_op_square_sum(_p(x), C.c_size_t(x.size), _p(o)))
    return o[0], o[1], o[2:6]


def op_swiglu(xo, xr):
    a = np.array(xo, dtype=np.float32, copy=True); b = np.ascontiguousarray(xr, dtype=np.float32)
    _check(lib().flm_op_swiglu(_p(a), _p(b), C.c_size_t(a.size)))
    return a


def op_rope(x, pos):
    x = np.ascontiguousarray(x, dtype=np.float32); o = np.empty_like(x)
    _check(lib().flm_op_rope(_p(o), _p(x), x.size, int(pos)))
    return o


def op_softmax(x, n=None):
    a = np.array(x, dtype=np.float32, copy=True)
    _check(lib().flm_op_softmax(_p(a), int(a.size if n is None else n)))
    return a


def op_expf(x):
    a = np.array(x, dtype=np.float32, copy=True).reshape(-1)
    _check(lib().flm_op_expf(_p(a), C.c_size_t(a.size)))
    return a


def op_math(fn, x, y=None):
    a = np.array(x, dtype=np.float32, copy=True).reshape(-1)
    b = None if y is None else np.ascontiguousarray(y, dtype=np.float32).reshape(-1)
    _check(lib().flm_op_math(int(fn), _p(a), _p(b), C.c_size_t(a.size)))
    return a


def fan_layout(pos, n_prompt, max_tokens, n, max_seq_len) -> FanLayout:
    """flm_fan_layout_for (pure host arithmetic): the rows flm_generate_n uses, or FlmError where the call would refuse"""
    out = FanLayout()
    _check(lib().flm_fan_layout_for(int(pos), int(n_prompt), int(max_tokens), int(n), int(max_seq_len), C.byref(out)))
    return out


def batch_layout(rows, max_seq_len) -> BatchLayout:
    """flm_batch_layout_for (pure host arithmetic): slot s owns the cache rows [base[s], base[s] + rows[s]), or FlmError where the layout is refused"""
    r = np.ascontiguousarray(rows, dtype=np.int32).reshape(-1)
    out = BatchLayout()
    _check(lib().flm_batch_layout_for(int(r.size), _p(r), int(max_seq_len), C.byref(out)))
    return out


def batch_plan(fed, pending, running, prompt_rows_max=0) -> BatchPlan:
    """flm_batch_plan_for (pure host arithmetic): the segments flm_batch_pass runs for slots with fed[s] rows in the cache and pending[s] prompt rows to go, `running` the
    mask of running slots and a budget of prompt_rows_max prompt rows (0: no bound), or FlmError where the call would refuse"""
    f = np.ascontiguousarray(fed, dtype=np.int32).reshape(-1); p = np.ascontiguousarray(pending, dtype=np.int32).reshape(-1)
    if f.size != p.size:
        raise ValueError("batch_plan: fed and pending have one entry per slot")
    if not 0 <= int(running) < 1 << 32:
        raise ValueError("batch_plan: running is a 32-bit mask")
    out = BatchPlan()
    _check(lib().flm_batch_plan_for(int(f.size), _p(f), _p(p), C.c_uint32(int(running)), int(prompt_rows_max), C.byref(out)))
    return out


def op_attention_segs(kc, vc, q, k, v, n_heads, hs, max_seq, base, rows, n, pos0, n_step=0, one_query=False):
    """one flm_batch_pass's attention: q, k, v [B, n_heads*hs], B = sum(n); segment s (n[s] consecutive rows) lies in the slot [base[s], base[s] + rows[s]) and enters at
    logical position pos0[s]; the first n_step segments are step rows.  one_query: the one-query form although the multi-query one would fit.  kc, vc
    [n_heads, max_seq, hs] are updated in place; returns out [B, n_heads*hs]."""
    for a in (kc, vc):
        assert a.dtype == np.float32 and a.flags.c_contiguous
    b = np.ascontiguousarray(base, dtype=np.int32); rw = np.ascontiguousarray(rows, dtype=np.int32)
    ns = np.ascontiguousarray(n, dtype=np.int32); ps = np.ascontiguousarray(pos0, dtype=np.int32)
    if not len(b) == len(rw) == len(ns) == len(ps):
        raise ValueError("op_attention_segs: base, rows, n and pos0 have one entry per segment")
    q = np.ascontiguousarray(q, dtype=np.float32); k = np.ascontiguousarray(k, dtype=np.float32); v = np.ascontiguousarray(v, dtype=np.float32)
    if not (q.ndim == 2 and q.shape == k.shape == v.shape and q.shape[1] == n_heads * hs):
        raise ValueError("op_attention_segs: q, k, v are [B, n_heads*hs]")
    out = np.empty_like(q)
    _check(lib().flm_op_attention_segs(_p(out), _p(kc), _p(vc), _p(q), _p(k), _p(v), n_heads, hs, max_seq, int(q.shape[0]), len(b), int(n_step), _p(b), _p(rw), _p(ns), _p(ps),
                                       1 if one_query else 0))
    return out


def op_attention_slots(kc, vc, q, k, v, n_heads, hs, max_seq, base, pos):
    """one flm_batch_step's attention: q, k, v [n, n_heads*hs]; row r at logical position pos[r] of the slot that starts at cache row base[r]: its k / v go to cache row
    base[r] + pos[r].  kc, vc [n_heads, max_seq, hs] are updated in place; returns out [n, n_heads*hs]."""
    for a in (kc, vc):
        assert a.dtype == np.float32 and a.flags.c_contiguous
    b = np.ascontiguousarray(base, dtype=np.int32); ps = np.ascontiguousarray(pos, dtype=np.int32); n = len(b)
    assert len(ps) == n
    q = np.ascontiguousarray(q, dtype=np.float32); k = np.ascontiguousarray(k, dtype=np.float32); v = np.ascontiguousarray(v, dtype=np.float32)
    assert q.shape == k.shape == v.shape == (n, n_heads * hs)
    out = np.empty((n, n_heads * hs), dtype=np.float32)
    _check(lib().flm_op_attention_slots(_p(out), _p(kc), _p(vc), _p(q), _p(k), _p(v), n_heads, hs, max_seq, n, _p(b), _p(ps)))
    return out


def op_attention_fan(kc, vc, q, k, v, n_heads, hs, max_seq, S, t, base):
    """one flm_generate_n step's attention: q, k, v [n, n_heads*hs] at logical position S + t; row j's k / v go to cache row base[j] + t.  kc, vc [n_heads, max_seq, hs]
    are updated in place; returns out [n, n_heads*hs]."""
    for a in (kc, vc):
        assert a.dtype == np.float32 and a.flags.c_contiguous
    b = np.ascontiguousarray(base, dtype=np.int32); n = len(b)
    q = np.ascontiguousarray(q, dtype=np.float32); k = np.ascontiguousarray(k, dtype=np.float32); v = np.ascontiguousarray(v, dtype=np.float32)
    assert q.shape == k.shape == v.shape == (n, n_heads * hs)
    out = np.empty((n, n_heads * hs), dtype=np.float32)
    _check(lib().flm_op_attention_fan(_p(out), _p(kc), _p(vc), _p(q), _p(k), _p(v), n_heads, hs, max_seq, n, int(S), int(t), _p(b)))
    return out


def op_attention(kc, vc, q, k, v, n_heads, hs, max_seq, pos):
    """kc, vc [n_heads, max_seq, hs] are updated in place; returns out [n_heads*hs]."""
    out = np.empty(n_heads * hs, dtype=np.float32)
    for a in (kc, vc):
        assert a.dtype == np.float32 and a.flags.c_contiguous
    q = np.ascontiguousarray(q, dtype=np.float32); k = np.ascontiguousarray(k, dtype=np.float32); v = np.ascontiguousarray(v, dtype=np.float32)
    _check(lib().flm_op_attention(_p(out), _p(kc), _p(vc), _p(q), _p(k), _p(v), n_heads, hs, max_seq, int(pos)))
    return out
