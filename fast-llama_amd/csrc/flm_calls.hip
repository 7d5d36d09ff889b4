// flm_calls.hip -- what a call does: the plumbing every model-level entry point shares (check_ready, feed, the retry wrapper, the by-value block setters, the bounce-buffer
// copies, the draw plan of flm_host.h) and the entry points themselves (include/flm_gpu.h: forward / decode / generate / score / draft-and-verify, the constraint, the
// log-probabilities).  What outlives a call -- the context, its memory, options, graphs and preparation -- is flm_gpu.hip.
#include "flm_host.h"
#include "../host/stop_rules.h"
#include <algorithm>

namespace fh {

// decode state <- {pos, tok, step}: by value through a one-thread kernel (an async copy from a host stack frame would be
// read after the frame is gone)
// (all of it: the latch open, and the generate words -- stop token -1, tag 0 for every entry point but flm_generate, which sets c->gen_* around its enqueue: they never halt)
__global__ void k_set_state(DecodeState* st, const DecodeState v) { if (threadIdx.x == 0 && blockIdx.x == 0) *st = v; }
int set_state(flm_ctx* c, int pos, int tok, int step) {
    DecodeState v{};
    v.pos = pos; v.tok = tok; v.step = step; v.halt = 0; v.stop_tok = c->gen_stop; v.gen_tag = c->gen_tag; v.max_tokens = c->gen_max; v.stop_rules = c->gen_rules;
    v.ring_cap = c->gen_cap; v.ring = c->gen_ring_dev; v.cancel = c->gen_cancel_dev;
    hipLaunchKernelGGL(k_set_state, dim3(1), dim3(64), 0, c->stream, c->state, v);
    HIPC(c, hipGetLastError());
    return FLM_OK;
}
// the device sampler's parameters for this call (by value, like the decode state): a retried call starts again from the caller's state
__global__ void k_set_sample(SampleParams* sp, float temperature, float topp, unsigned long long rng) {
    if (threadIdx.x == 0 && blockIdx.x == 0) { sp->temperature = temperature; sp->topp = topp; sp->rng = rng; }
}
static int set_sample(flm_ctx* c, float temperature, float topp, unsigned long long rng) {
    hipLaunchKernelGGL(k_set_sample, dim3(1), dim3(64), 0, c->stream, c->sparams, temperature, topp, rng);
    HIPC(c, hipGetLastError());
    return FLM_OK;
}
// the shaper's parameter block for this call: through a page-locked staging copy of its own (allocated at create), moved by a kernel on the context's stream like every
// other upload -- not through the bounce buffer, which carries the prompt in the same call, so no synchronise is needed.  The stream is idle when an entry point starts
// (every entry point, and every attempt of a retried call, returns behind a synchronise): the previous call's copy has left the staging block
static int copy_words(flm_ctx* c, const void* src, void* dst, size_t bytes, bool with_err);
static int set_shape(flm_ctx* c, const ShapeParams& sp) {
    static_assert(sizeof(ShapeParams) % 4 == 0, "whole words");
    if (hipStreamQuery(c->stream) != hipSuccess) { (void)hipGetLastError(); HIPC(c, hipStreamSynchronize(c->stream)); }   // (never taken today; an entry point that one day returns without a synchronise must not race the copy below)
    memcpy(c->shape_stage, &sp, sizeof sp);
    return copy_words(c, c->shape_stage, c->shape_p, sizeof sp, false);
}
// the constraint's block, by value like the decode state: {the arrays, n_states, q, applied = 0}.  One tiny launch on the context's stream: no allocation, no graph touched
__global__ void k_set_dfa(DfaBlock* blk, const DfaBlock v) { if (threadIdx.x == 0 && blockIdx.x == 0) *blk = v; }
static int set_dfa(flm_ctx* c, int q) {
    DfaBlock v{};
    const int ns = (int)c->dfa_row.size() - 1;
    if (c->dfa_dev && ns > 0) { v.row_ptr = c->dfa_dev; v.edge_token = c->dfa_dev + (ns + 1); v.edge_next = v.edge_token + c->dfa_tok.size(); v.n_states = ns; }
    v.q = v.n_states > 0 ? q : -1; v.applied = 0;
    hipLaunchKernelGGL(k_set_dfa, dim3(1), dim3(64), 0, c->stream, c->dfa_blk, v);
    HIPC(c, hipGetLastError());
    return FLM_OK;
}
// the log-probability stage's block, by value like the decode state: {top_n (-1: off), source, the record index of step 0}.  One tiny launch: no allocation, no graph touched
__global__ void k_set_lp(LogprobBlock* blk, const LogprobBlock v) { if (threadIdx.x == 0 && blockIdx.x == 0) *blk = v; }
static int set_lp(flm_ctx* c, int base) {
    LogprobBlock v{}; v.top_n = c->lp_top_n; v.source = c->lp_source; v.base = base;
    hipLaunchKernelGGL(k_set_lp, dim3(1), dim3(64), 0, c->stream, c->lp_blk, v);
    HIPC(c, hipGetLastError());
    return FLM_OK;
}
// the entropy-driven samplers' block, by value like the decode state, from the host's copy: the parameters and Mirostat's mu behind the ids delivered so far -- written
// at the start of every attempt, so a retried attempt updates nothing twice.  One tiny launch: no allocation, no graph touched
__global__ void k_set_entropy(EntropyBlock* blk, const EntropyBlock v) { if (threadIdx.x == 0 && blockIdx.x == 0) *blk = v; }
static int set_entropy(flm_ctx* c) {
    EntropyBlock v{}; v.typical_p = c->ent.typical_p; v.mirostat = c->ent.mirostat; v.tau = c->ent.tau; v.eta = c->ent.eta; v.mu = c->ent.mu;
    hipLaunchKernelGGL(k_set_entropy, dim3(1), dim3(64), 0, c->stream, c->ent_blk, v);
    HIPC(c, hipGetLastError());
    return FLM_OK;
}
// the rules of flm_entropy_validate: null, or which one failed
static const char* entropy_check(const flm_entropy* e) {
    if (!e) return "entropy: null struct";
    if (e->typical_p != e->typical_p) return "entropy: typical_p is NaN";
    if (e->mirostat != 0 && e->mirostat != 2) return "entropy: mirostat must be 0 or 2";
    if (e->mirostat == 2 && !(isfinite(e->tau) && isfinite(e->eta) && isfinite(e->mu))) return "entropy: tau, eta and mu must be finite";
    if (e->mirostat == 2 && typical_on(e->typical_p)) return "entropy: typical_p and mirostat are both set";
    return nullptr;
}
// delta(q, t): the edge_next of t's edge in q, or q itself when t has no edge there -- reachable only through the multinomial branch's last-index fallback of Sampler::sample
// (`return _n - 1`), which can name a masked id; folded over the ids a call delivered
int dfa_fold(const flm_ctx* c, int q, const int32_t* ids, int n) {
    for (int i = 0; i < n; ++i) {
        const int32_t* b = c->dfa_tok.data() + c->dfa_row[q]; const int32_t* e = c->dfa_tok.data() + c->dfa_row[q + 1];
        const int32_t* it = std::lower_bound(b, e, ids[i]);
        if (it != e && *it == ids[i]) q = c->dfa_nxt[it - c->dfa_tok.data()];
    }
    return q;
}
const char* dfa_check(const flm_dfa* a, int vocab) {
    if (!a) return "dfa: null struct";
    if (vocab < 1) return "dfa: vocab < 1";
    if (a->n_states < 1 || a->n_states > FLM_DFA_STATES_MAX) return "dfa: n_states outside [1, FLM_DFA_STATES_MAX]";
    if (a->n_edges < 1 || a->n_edges > FLM_DFA_EDGES_MAX) return "dfa: n_edges outside [1, FLM_DFA_EDGES_MAX]";
    if (!a->row_ptr || !a->edge_token || !a->edge_next) return "dfa: null array";
    if (a->row_ptr[0] != 0 || a->row_ptr[a->n_states] != a->n_edges) return "dfa: row_ptr must start at 0 and end at n_edges";
    for (int q = 0; q < a->n_states; ++q) {
        if (a->row_ptr[q + 1] < a->row_ptr[q] || a->row_ptr[q + 1] > a->n_edges) return "dfa: row_ptr is not non-decreasing within [0, n_edges]";
    }
    for (int q = 0; q < a->n_states; ++q) if (a->row_ptr[q + 1] == a->row_ptr[q]) return "dfa: a state has no edge";
    for (int q = 0; q < a->n_states; ++q) {
        for (int e = a->row_ptr[q]; e < a->row_ptr[q + 1]; ++e) {
            if (a->edge_token[e] < 0 || a->edge_token[e] >= vocab) return "dfa: edge token outside [0, vocab)";
            if (a->edge_next[e] < 0 || a->edge_next[e] >= a->n_states) return "dfa: edge_next outside [0, n_states)";
            if (e > a->row_ptr[q] && a->edge_token[e] == a->edge_token[e - 1]) return "dfa: a token is listed twice in a state";
            if (e > a->row_ptr[q] && a->edge_token[e] < a->edge_token[e - 1]) return "dfa: tokens must be strictly ascending inside a state";
        }
    }
    return nullptr;
}
const char* shape_fill(const flm_sampling* sp, int vocab, const int32_t* window, int n_window, bool follow, ShapeParams* out, bool* active) {
    if (!sp) return "sampling: null struct";
    if (!(sp->temperature >= 0.0f) || sp->topp != sp->topp) return "sampling: temperature must be >= 0, top-p a number";
    if (sp->top_k < 0) return "sampling: top_k < 0";
    if (!(sp->min_p >= 0.0f && sp->min_p < 1.0f)) return "sampling: min_p outside [0, 1)";
    if (!(sp->repeat_penalty > 0.0f) || isinf(sp->repeat_penalty)) return "sampling: repeat_penalty must be a positive number";
    if (sp->frequency_penalty != sp->frequency_penalty || sp->presence_penalty != sp->presence_penalty) return "sampling: a penalty is NaN";
    if (sp->penalty_last_n < 0 || sp->penalty_last_n > FLM_PENALTY_WINDOW_MAX) return "sampling: penalty_last_n outside [0, FLM_PENALTY_WINDOW_MAX]";
    if (n_window < 0 || n_window > FLM_PENALTY_WINDOW_MAX || (n_window > 0 && !window)) return "sampling: n_window outside [0, FLM_PENALTY_WINDOW_MAX]";
    if (sp->n_bias < 0 || sp->n_bias > FLM_BIAS_MAX || (sp->n_bias > 0 && (!sp->bias_ids || !sp->bias_values))) return "sampling: n_bias outside [0, FLM_BIAS_MAX]";
    for (int i = 0; i < sp->n_bias; ++i) {
        const int id = sp->bias_ids[i]; const float b = sp->bias_values[i];
        if (id < 0 || id >= vocab) return "sampling: bias id outside [0, vocab)";
        if (b != b || b == INFINITY) return "sampling: a bias is NaN or +inf";
        for (int k = 0; k < i; ++k) if (sp->bias_ids[k] == id) return "sampling: a bias id is listed twice";
    }
    for (int i = 0; i < n_window; ++i) if (window[i] < 0 || window[i] >= vocab) return "sampling: window id outside [0, vocab)";
    static_assert(kShapeWindowMax == FLM_PENALTY_WINDOW_MAX && kShapeBiasMax == FLM_BIAS_MAX, "flm_shape.h mirrors the header's limits");
    ShapeParams& o = *out;
    memset(&o, 0, sizeof o);
    const bool pen = sp->repeat_penalty != 1.0f || sp->frequency_penalty != 0.0f || sp->presence_penalty != 0.0f;
    o.temperature = sp->temperature;
    o.minp_on = sp->min_p > 0.0f && sp->temperature != 0.0f ? 1 : 0;
    if (o.minp_on) { volatile float mp = sp->min_p; o.lt = logf(mp); }        // (glibc's logf, at run time: the one logarithm of the definition)
    o.top_k = sp->top_k > 0 && sp->top_k < vocab ? sp->top_k : 0;
    o.repeat = sp->repeat_penalty; o.freq = sp->frequency_penalty; o.pres = sp->presence_penalty;
    o.follow = follow ? 1 : 0;
    o.last_n = follow && pen ? sp->penalty_last_n : 0;
    // follow: the tail of the prompt that can still be inside the window at the first token
    int nh = pen ? n_window : 0;
    if (follow && nh > o.last_n) { window += nh - o.last_n; nh = o.last_n; }
    o.n_head = nh;
    for (int i = 0; i < nh; ++i) o.head[i] = window[i];
    o.n_bias = sp->n_bias;
    for (int i = 0; i < sp->n_bias; ++i) { o.bias_ids[i] = sp->bias_ids[i]; o.bias_vals[i] = sp->bias_values[i]; }
    const bool pen_on = pen && (follow ? o.last_n > 0 : nh > 0);
    *active = o.n_bias > 0 || pen_on || o.top_k > 0 || o.minp_on;
    return nullptr;
}

int check_ready(flm_ctx* c, int n, int pos) {
    if (!c) return FLM_ERR_INVALID;
    c->err_word_fresh = false;                                                  // (an error word a previous call's read-back brought along says nothing about this call)
    c->fan_valid = false;                                                       // (every entry point that writes the cache comes through here: flm_fan_keep's tails are gone)
    c->batch_open = false;                                                      // (... and so are an open batch's slots: flm_batch_join / _step / _close(keep) answer FLM_ERR_STATE)
    if (!model_complete(c)) return fail(c, FLM_ERR_STATE, "forward before all tensors were uploaded");
    if (n < 1 || pos < 0 || pos + n > c->d.max_seq_len) return fail(c, FLM_ERR_INVALID, "tokens/pos outside [0, max_seq_len]");
    HIPC(c, hipSetDevice(c->device));
    return FLM_OK;
}

// device -> caller's buffer / caller's buffer -> device through the context's page-locked bounce buffer (flm_host.h: bounce), in pieces of its size; d2h synchronises.
// The bytes are moved by a KERNEL on the context's stream (the bounce buffer is mapped into the device's address space), not by hipMemcpyAsync: a copy engine's queue is
// shared by every context of the process and served in order, and a copy that waits for its stream's kernels blocks it -- under tensor parallelism (rank A's copy of token t
// in front of rank B's copy of token t - 1, A's kernels waiting for B's next slice) that is a deadlock; the engines' queues are also created lazily (device memory taken
// inside a forward: tools/alloc_diag.py).
// (word_src -> word_dst: one more word from elsewhere -- the cross-workgroup error flag rides along with a call's results, so that xwg_check needs no copy of its own)
__global__ void k_copy_words(const unsigned* __restrict__ src, unsigned* __restrict__ dst, unsigned n, const unsigned* __restrict__ word_src, unsigned* __restrict__ word_dst) {
    for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) dst[i] = src[i];
    if (word_src && blockIdx.x == 0 && threadIdx.x == 0) *word_dst = *word_src;
}
static int copy_words(flm_ctx* c, const void* src, void* dst, size_t bytes, bool with_err) {
    const unsigned n = (unsigned)(bytes / 4);                                       // (ids, logits: whole words)
    const unsigned blocks = n < 256 * 64 ? (n + 255) / 256 : 64;
    hipLaunchKernelGGL(k_copy_words, dim3(blocks ? blocks : 1), dim3(256), 0, c->stream, (const unsigned*)src, (unsigned*)dst, n,
                       with_err ? (const unsigned*)c->xwg_err : (const unsigned*)nullptr, (unsigned*)(c->bounce + c->bounce_bytes));
    HIPC(c, hipGetLastError());
    return FLM_OK;
}
int d2h(flm_ctx* c, void* dst, const void* src_dev, size_t bytes) {
    for (size_t o = 0; o < bytes; o += c->bounce_bytes) {
        const size_t nb = bytes - o < c->bounce_bytes ? bytes - o : c->bounce_bytes;
        const bool last = o + nb >= bytes;
        int r = copy_words(c, (const char*)src_dev + o, c->bounce, nb, last); if (r) return r;
        HIPC(c, hipStreamSynchronize(c->stream));
        memcpy((char*)dst + o, c->bounce, nb);
        if (last) { c->err_word = *(volatile int*)(c->bounce + c->bounce_bytes); c->err_word_fresh = true; }   // (read behind the call's last kernel: what xwg_check looks at)
    }
    return FLM_OK;
}
int h2d(flm_ctx* c, void* dst_dev, const void* src, size_t bytes) {
    for (size_t o = 0; o < bytes; o += c->bounce_bytes) {
        const size_t nb = bytes - o < c->bounce_bytes ? bytes - o : c->bounce_bytes;
        if (o) HIPC(c, hipStreamSynchronize(c->stream));                          // (the previous piece has left the buffer)
        memcpy(c->bounce, (const char*)src + o, nb);
        int r = copy_words(c, c->bounce, (char*)dst_dev + o, nb, false); if (r) return r;
    }
    return FLM_OK;
}
int Draw::arm_with(flm_ctx* c, const ShapeParams& blk, unsigned long long rng, int q, int rec_base) const {
    int r = shaped() ? set_shape(c, blk) : FLM_OK;
    if (!r && q >= 0) r = set_dfa(c, q);
    if (!r && lp) r = set_lp(c, rec_base);
    if (!r && ent) r = set_entropy(c);
    if (!r && form != TokenForm::Greedy) r = set_sample(c, temperature, topp, coins() ? rng : 0ull);
    return r;
}
int Draw::arm_step(flm_ctx* c, unsigned long long rng, int q, int rec_base, const int32_t* prompt, int n_prompt, const int32_t* drawn, int n_drawn) const {
    if (!shaped()) return arm_with(c, block, rng, q, rec_base);
    ShapeParams one = block;       // (follow 0: set_state has reset the step counter the follow form counts by)
    const int n_hist = n_prompt + n_drawn, w = one.last_n < n_hist ? one.last_n : n_hist;
    for (int j = 0; j < w; ++j) { const int g = n_hist - w + j; one.head[j] = g < n_prompt ? prompt[g] : drawn[g - n_prompt]; }
    one.n_head = w; one.follow = 0;
    return arm_with(c, one, rng, q, rec_base);
}
int Draw::arm_block(flm_ctx* c) const { return shaped() ? set_shape(c, block) : FLM_OK; }
SpecDraw Draw::batch(const flm_ctx* c, unsigned long long base, const int* win, int n_win, int q, int rec_base) const {
    SpecDraw sd{temperature, topp, base};
    if (shaped()) { sd.shape = c->shape_p; sd.win = win ? win : c->shape_p->head; sd.n_win = win ? n_win : block.n_head; sd.cstate = q; }
    if (lp) { sd.lp_top_n = c->lp_top_n; sd.lp_source = c->lp_source; sd.lp_base = rec_base; }
    sd.typical_p = typical_p;
    return sd;
}
int Draw::fetch(flm_ctx* c, unsigned long long* after) const {
    if (mu_moves()) { const int r = d2h(c, &c->ent_mu_fetched, &c->ent_blk->mu, sizeof(float)); if (r) return r; }
    return coins() ? d2h(c, after, &c->sparams->rng, sizeof *after) : FLM_OK;
}
void Draw::commit(flm_ctx* c, const int32_t* ids, int n, unsigned long long after) const { commit(c, n, after, cstate >= 0 ? dfa_fold(c, cstate, ids, n) : -1); }
void Draw::commit(flm_ctx* c, int n, unsigned long long after, int q_after) const {
    if (coins()) { *rng_state = after; c->sampled += n; }
    if (shaped()) c->shaped += n;
    if (q_after >= 0) c->dfa_state = q_after;
    if (lp) c->lp_count = n;
    if (mu_moves()) c->ent.mu = c->ent_mu_fetched;
}
// feed tokens[0..n) sequentially (row i of the reference's batched prefill depends only on rows
// <= i through the KV cache, so token-by-token evaluation performs the same per-row arithmetic).
int feed(flm_ctx* c, const int32_t* tokens, int n, int pos, TokenForm last) {
    int r;
    if (n > c->prompt_cap) return fail(c, FLM_ERR_INVALID, "more tokens than max_seq_len");
    if (!ids_in_vocab(c, tokens, n)) return fail(c, FLM_ERR_INVALID, "token id out of range");
    { const int rc = h2d(c, c->prompt_dev, tokens, sizeof(int) * (size_t)n); if (rc) return rc; }     // (prompt_cap <= the bounce buffer: one piece; the stream orders it in front of the kernels, nothing touches the buffer before the call's read-back)
    // batched: single GPU always; tensor parallel over the peer-to-peer exchange with the matrix-core kernels (the kernels that store their
    // column slices into the peers' buffers)
    const bool tp_ok = c->world > 1 && c->p2p && c->tp_prefill;          // agreed by all ranks at flm_p2p_import
    if (c->use_prefill && (c->world == 1 || tp_ok) && n - 1 >= kPrefillMin) {
        // all tokens but the last in one batch (cache rows only), then the last one through the decode kernels
        r = prefill_batched_qt(c, n - 1, pos);
        if (r) return r;
        r = set_state(c, pos + n - 1, tokens[n - 1], 0); if (r) return r;
        return run_token(c, true, last, pos + n);
    }
    r = set_state(c, pos, tokens[0], 0); if (r) return r;
    for (int i = 0; i + 1 < n; ++i) { r = run_token(c, false, TokenForm::Prompt, pos + i + 1); if (r) return r; }
    // last token: classifier; state.step is reset so out_tokens[0] receives the argmax
    if (n > 1) {
        // step was used as the prompt cursor; zero it for the argmax slot
        hipLaunchKernelGGL(k_set_step, dim3(1), dim3(64), 0, c->stream, c->state, 0);
        HIPC(c, hipGetLastError());
    }
    return run_token(c, true, last, pos + n);
}

// Every token entry point runs its work and then looks at the cross-workgroup error flag (xwg_check); if a hand-off
// inside the fused attention + Wo launch timed out, the SAME work runs again on one kernel per phase: the cache rows
// and logits of the failed attempt are simply overwritten, and the caller gets correct results and FLM_OK.
// body: one attempt, up to the read-back of its results; commit: what only a verified attempt may change in the caller's state.
template <class Body, class Commit>
static int with_retry(flm_ctx* c, int tokens, Body body, Commit commit) {
    for (int attempt = 0; attempt < 2; ++attempt) {
        int r = body(); if (r) return r;
        r = xwg_check(c);
        if (r == FLM_OK) { commit(); return maybe_recover(c, tokens); }
        if (r != FLM_RETRY) return r;
    }
    return fail(c, FLM_ERR_HIP, "cross-workgroup wait timed out twice");
}
template <class Body> static int with_retry(flm_ctx* c, int tokens, Body body) { return with_retry(c, tokens, body, [] {}); }
// the context is armed for per-token log-probabilities (flm_logprobs_arm refuses where logprobs_supported is false; "force_tp" may have been set since)
static bool lp_armed(const flm_ctx* c) { return c->lp_top_n >= 0 && logprobs_supported(c) && c->lp_rec != nullptr; }
// The _ex entry points' plan: flm_sampling, the window (follow: flm_generate_ex's sliding window over the prompt's tail, else as given) and the caller's state, with what the
// context is armed for, resolved into `dr` -- or into the error the call returns.  An armed constraint counts as a control that is set (the shaped form runs, masking
// only), and so does a context armed for log-probabilities (the shaped form with the record stage behind its sampler).  own(block, active): what one entry point checks or
// changes between the block's validation and that decision (null, or what is wrong)
struct NoOwn { const char* operator()(ShapeParams&, bool&) const { return nullptr; } };
// honour_rules (flm_generate_ex / flm_generate_lookup_ex): installed stop rules count as a control that is set too -- the matcher lives in the shaped form's last launch.
// flm_entropy_set counts as one as well (the ShapedEnt form); batch (the draft-and-verify entry points): Mirostat is refused -- row r's mu depends on the draws in front of it
template <class Own = NoOwn>
static int draw_resolve(flm_ctx* c, const flm_sampling* sampling, const int32_t* window, int n_window, bool follow, uint64_t* rng_state, Draw& dr, Own own = Own(), bool honour_rules = false, bool batch = false) {
    bool active = false;
    const char* why = shape_fill(sampling, c->d.vocab_size, window, n_window, follow, &dr.block, &active);
    if (!why) why = own(dr.block, active);
    if (why) return fail(c, FLM_ERR_INVALID, why);
    if (sampling->temperature != 0.0f && !rng_state) return fail(c, FLM_ERR_INVALID, "sample: rng_state must be given at temperature != 0");
    dr.plain(sampling->temperature, sampling->topp, rng_state);
    const int cq = sharded(c) ? -1 : c->dfa_state;
    const bool lp = lp_armed(c);
    const bool rules = honour_rules && !sharded(c) && stop_installed(c);
    const int ent = entropy_supported(c) ? c->ent_mode : 0;
    if (ent && lp) return fail(c, FLM_ERR_UNSUPPORTED, "entropy: not built on a context armed for log-probabilities");
    if (ent == 2 && batch) return fail(c, FLM_ERR_UNSUPPORTED, "entropy: Mirostat is not built through the draft-and-verify entry points");
    if (active || cq >= 0 || lp || rules || ent) { dr.shape_by(cq, lp, ent, c->ent.typical_p); dr.rules = rules; }
    return FLM_OK;
}
// flm_score_tokens: where a chunk of rows' logits is staged -- the prefill scores (free once the last layer's attention is done) or, a row at a time, the logits vector --
// and how many rows a chunk has (option "score_rows" caps it; a negative value takes the logits vector although the scores exist: how the tests reach that staging on small shapes)
float* score_stage(const flm_ctx* c, int* chunk) {
    const size_t row_bytes = (size_t)c->d.vocab_size * 4;
    const size_t sc_rows = c->pf_scores && c->score_rows >= 0 ? ((size_t)c->heads_local * c->pf_cap * c->d.max_seq_len * 4) / row_bytes : 0;
    *chunk = sc_rows >= 1 ? (int)(sc_rows < (size_t)c->pf_cap ? sc_rows : (size_t)c->pf_cap) : 1;
    if (c->score_rows > 0 && c->score_rows < *chunk) *chunk = c->score_rows;
    return sc_rows >= 1 ? c->pf_scores : c->logits;
}
// the host's view of the installed rules (pointers into the context's copy), and why a generate-family call that delivered ids[0 .. n) of max_tokens ended: the host
// restatement at the last delivered index; no rule fires there: fewer ids than asked for = behind a cancel, else length ("stop_reason" / "stop_rule")
static flm_stop_rules stop_view(const flm_ctx* c) {
    const StopBlock& b = c->stop_host;
    return flm_stop_rules{b.n_ids, b.ids, b.n_seqs, b.seq_ptr, b.seq_tok};
}
static void stop_note(flm_ctx* c, bool with_rules, int32_t stop_token, const int32_t* ids, int n, int max_tokens) {
    const flm_stop_rules v = stop_view(c);
    int kind = FLM_STOP_LENGTH, rule = 0;
    if (n < 1 || !flmhost::stop_fires_at(with_rules ? &v : nullptr, stop_token, ids, n - 1, &kind, &rule)) { kind = n < max_tokens ? FLM_STOP_CANCEL : FLM_STOP_LENGTH; rule = 0; }
    c->stop_reason = kind; c->stop_rule = rule;
}
// The model-based drafter (flm_generate_draft): how the target context c and its draft d share the device.  The one-launch token spins on co-resident workgroups, so a
// launch of one context must never be resident next to a launch of the other (two resident grids: timed-out waits).  The two streams are therefore JOINED around
// everything the draft enqueues: draft_open -- event [0], recorded on the target's stream, waited for on the draft's: the draft starts behind whatever the target has
// queued --, the draft's work, draft_close -- event [1], recorded on the draft's stream, waited for on the target's: the target's batch starts behind the draft.  Target ->
// the NEXT step's draft needs no event: the host reads the step's result block (a synchronise of the target's stream) before it enqueues anything more.
static int draft_open(flm_ctx* c, flm_ctx* d) {
    HIPC(c, hipEventRecord(c->draft_ev[0], c->stream));
    HIPC(c, hipStreamWaitEvent(d->stream, c->draft_ev[0], 0));
    return FLM_OK;
}
static int draft_close(flm_ctx* c, flm_ctx* d) {
    HIPC(c, hipEventRecord(c->draft_ev[1], d->stream));
    HIPC(c, hipStreamWaitEvent(c->stream, c->draft_ev[1], 0));
    return FLM_OK;
}
// where the draft's error word lands on the host: the second word of the target's bounce line (d2h puts the target's own into the first), read behind the same synchronise
static int* draft_err_word(const flm_ctx* c) { return (int*)(c->bounce + c->bounce_bytes + 4); }
// ... carried there by a copy on the TARGET's stream behind draft_close (the attempts whose batch does not run k_spec_take_drafts, which carries it itself)
static int draft_err_along(flm_ctx* c, const flm_ctx* d) {
    hipLaunchKernelGGL(k_copy_words, dim3(1), dim3(64), 0, c->stream, (const unsigned*)d->xwg_err, (unsigned*)draft_err_word(c), 1u, (const unsigned*)nullptr, (unsigned*)nullptr);
    HIPC(c, hipGetLastError());
    return FLM_OK;
}
// an error of a call made on the draft's behalf is the target's call's error
static int draft_rc(flm_ctx* c, const flm_ctx* d, int r) { if (r) { c->err = "draft: " + d->err; g_last_error = c->err; } return r; }
// with_retry for an attempt that ran work of BOTH contexts: a wait that gave up in either re-runs the whole attempt (each context falls back and recovers by its own
// policy: xwg_check / maybe_recover, untouched); d_tokens: what the draft computed in it.  d null: with_retry
template <class Body, class Commit>
static int with_retry_pair(flm_ctx* c, flm_ctx* d, int tokens, int d_tokens, Body body, Commit commit) {
    if (!d) return with_retry(c, tokens, body, commit);
    for (int attempt = 0; attempt < 2; ++attempt) {
        int r = body();
        if (r) { (void)hipStreamSynchronize(d->stream); (void)hipStreamSynchronize(c->stream); return r; }
        d->err_word = *(volatile int*)draft_err_word(c); d->err_word_fresh = true;        // (behind the body's read-back, like the target's own)
        const int rd = xwg_check(d), rc = xwg_check(c);
        if (rd != FLM_OK && rd != FLM_RETRY) return draft_rc(c, d, rd);
        if (rc != FLM_OK && rc != FLM_RETRY) return rc;
        if (rd == FLM_OK && rc == FLM_OK) {
            commit();
            r = maybe_recover(c, tokens);
            return r ? r : draft_rc(c, d, maybe_recover(d, d_tokens));
        }
    }
    return fail(c, FLM_ERR_HIP, "cross-workgroup wait timed out twice");
}

// One verify pass at `pos` over the batch prompt_dev[0 .. k] (draft: written by the drafter from the history spec_hist[0 .. n_hist) first): all layers, the classifier in
// chunks, the rows' ids -- drawn by k_sample_rows with the coins of draw.base, at temperature 0 their first maxima --, the accept step, which also leaves the state after
// the step's draws.  Enqueues only; the result block spec_res is read by the caller.
// rules (the loop under installed stop rules; null otherwise): the accept step also cuts the run behind the first index a rule fires at (k_spec_accept_rules), evaluated
// against spec_hist[n_prompt .. n_hist) ++ the run
// drafter (flm_generate_draft; null otherwise): the batch's drafts are the k ids that context's token loop left in its out_tokens_dev (k_spec_take_drafts, behind the wait
// on its event: draft_close) instead of the prompt-lookup drafter's; its error word rides along
static int spec_step(flm_ctx* c, int pos, int k, int ngram_max, int n_hist, int stop, int room, bool draft, const SpecDraw& draw, const StopBlock* rules = nullptr, int n_prompt = 0, const flm_ctx* drafter = nullptr) {
    const int B = k + 1;
    if (draft && drafter) {
        hipLaunchKernelGGL(k_spec_take_drafts, dim3(1), dim3(kWave), 0, c->stream, (const int*)c->spec_hist, n_hist, (const int*)drafter->out_tokens_dev, k, c->d.vocab_size, c->prompt_dev,
                           (const int*)drafter->xwg_err, draft_err_word(c));
        HIPC(c, hipGetLastError());
    }
    else if (draft) {
        hipLaunchKernelGGL(k_spec_draft, dim3(1), dim3(kSampleBlock), 0, c->stream, (const int*)c->spec_hist, n_hist, k, ngram_max, c->prompt_dev);
        HIPC(c, hipGetLastError());
    }
    const bool skinny = c->spec_gemm != 0;
    int r = prefill_batched_qt(c, B, pos, true, skinny); if (r) return r;
    int chunk = 1; float* const stage = score_stage(c, &chunk);
    for (int r0 = 0; r0 < B; r0 += chunk) {
        const int m = B - r0 < chunk ? B - r0 : chunk;
        r = spec_classify(c, r0, m, stage, skinny, c->spec_arg, draw); if (r) return r;
    }
    if (rules && draft) hipLaunchKernelGGL(k_spec_accept_rules, dim3(1), dim3(kSampleBlock), 0, c->stream, c->spec_res, (const int*)c->spec_arg, (const int*)c->prompt_dev, k, c->spec_hist, n_prompt, n_hist, stop, room, draw.base, draw.temperature != 0.0f ? 1 : 0, rules);
    else hipLaunchKernelGGL(k_spec_accept_sample, dim3(1), dim3(64), 0, c->stream, c->spec_res, (const int*)c->spec_arg, (const int*)c->prompt_dev, k, draft ? c->spec_hist : (int*)nullptr, n_hist, stop, room, draw.base, draw.temperature != 0.0f ? 1 : 0);
    HIPC(c, hipGetLastError());
    return FLM_OK;
}

} // namespace fh

extern "C" {

int flm_forward(flm_ctx* c, const int32_t* tokens, int n, int pos, float* logits_host) {
    if (!tokens || !logits_host) return FLM_ERR_INVALID;
    int r = check_ready(c, n, pos); if (r) return r;
    return with_retry(c, n, [&] {
        int r = feed(c, tokens, n, pos, TokenForm::Logits); if (r) return r;
        return d2h(c, logits_host, c->logits, (size_t)c->d.vocab_size * 4);
    });
}

int flm_forward_argmax(flm_ctx* c, const int32_t* tokens, int n, int pos, int32_t* next_token) {
    if (!tokens || !next_token) return FLM_ERR_INVALID;
    int r = check_ready(c, n, pos); if (r) return r;
    return with_retry(c, n, [&] {
        int r = feed(c, tokens, n, pos, TokenForm::Greedy); if (r) return r;
        return d2h(c, next_token, c->out_tokens_dev, 4);
    });
}

static int decode_loop(flm_ctx* c, int32_t first_token, int pos, int n_steps, hipEvent_t e0, hipEvent_t e1, TokenForm form = TokenForm::Greedy) {
    int r = check_ready(c, n_steps, pos); if (r) return r;
    if (!ids_in_vocab(c, &first_token, 1)) return fail(c, FLM_ERR_INVALID, "token id out of range");
    if (n_steps > c->out_cap) return fail(c, FLM_ERR_INVALID, "more steps than max_seq_len");
    r = set_state(c, pos, first_token, 0); if (r) return r;
    if (e0) HIPC(c, hipEventRecord(e0, c->stream));
    r = run_tokens(c, pos, n_steps, form); if (r) return r;
    if (e1) HIPC(c, hipEventRecord(e1, c->stream));
    return FLM_OK;
}

int flm_decode_greedy(flm_ctx* c, int32_t first_token, int pos, int n_steps, int32_t* out_tokens) {
    if (!out_tokens) return FLM_ERR_INVALID;
    return with_retry(c, n_steps, [&] {
        int r = decode_loop(c, first_token, pos, n_steps, nullptr, nullptr); if (r) return r;
        return d2h(c, out_tokens, c->out_tokens_dev, sizeof(int) * (size_t)n_steps);
    });
}

int flm_decode_timed(flm_ctx* c, int32_t first_token, int pos, int n_steps, float* ms) {
    if (!ms || !c) return FLM_ERR_INVALID;
    HIPC(c, hipSetDevice(c->device));
    EvPair ev; HIPC(c, hipEventCreate(&ev.e0)); HIPC(c, hipEventCreate(&ev.e1));
    return with_retry(c, n_steps, [&]() -> int {
        int r = decode_loop(c, first_token, pos, n_steps, ev.e0, ev.e1); if (r) return r;
        hipError_t e = hipEventSynchronize(ev.e1); if (e == hipSuccess) e = hipEventElapsedTime(ms, ev.e0, ev.e1);
        if (e != hipSuccess) { c->err = hipGetErrorString(e); return FLM_ERR_HIP; }
        return FLM_OK;
    });
}

// Sampler::sample on the device (flm_sample.h): the parameters and the caller's state go to the device block first, the sampled token graphs (captured at prepare,
// next to the greedy ones) replay, then the state comes back.  A retried call (xwg_check) starts again from the caller's state: nothing is drawn twice.
static int sample_args_ok(flm_ctx* c, float temperature, float topp, const uint64_t* rng_state) {
    if (!rng_state || !(temperature >= 0.0f) || topp != topp) return fail(c, FLM_ERR_INVALID, "sample: temperature must be >= 0, top-p a number, rng_state given");
    if (!sample_supported(c)) return fail(c, FLM_ERR_UNSUPPORTED, "device sampler: vocabulary too large for one workgroup's LDS (sample on the host)");
    return FLM_OK;
}
// one token drawn behind tokens[0 .. n): flm_forward_sample and, with the shaper's block, flm_forward_sample_ex
static int forward_draw(flm_ctx* c, const int32_t* tokens, int n, int pos, const Draw& dr, int32_t* next_token) {
    int r = check_ready(c, n, pos); if (r) return r;
    if (dr.coins()) { r = sample_args_ok(c, dr.temperature, dr.topp, dr.rng_state); if (r) return r; }
    unsigned long long after = 0;
    return with_retry(c, n, [&] {
        int r = dr.arm(c); if (r) return r;
        r = feed(c, tokens, n, pos, dr.form); if (r) return r;
        r = dr.fetch(c, &after); if (r) return r;
        return d2h(c, next_token, c->out_tokens_dev, 4);
    }, [&] { dr.commit(c, next_token, 1, after); });
}
int flm_forward_sample(flm_ctx* c, const int32_t* tokens, int n, int pos, float temperature, float topp, uint64_t* rng_state, int32_t* next_token) {
    if (!tokens || !next_token) return FLM_ERR_INVALID;
    return forward_draw(c, tokens, n, pos, Draw(temperature, topp, rng_state, true), next_token);
}
int flm_decode_sample(flm_ctx* c, int32_t first_token, int pos, int n_steps, float temperature, float topp, uint64_t* rng_state, int32_t* out_tokens) {
    if (!c || !out_tokens) return FLM_ERR_INVALID;
    int r = sample_args_ok(c, temperature, topp, rng_state); if (r) return r;
    const Draw dr(temperature, topp, rng_state, true);
    unsigned long long after = 0;
    return with_retry(c, n_steps, [&] {
        int r = check_ready(c, n_steps, pos); if (r) return r;       // (in front of set_sample's launch: this entry point has selected no device yet)
        r = dr.arm(c); if (r) return r;
        r = decode_loop(c, first_token, pos, n_steps, nullptr, nullptr, dr.form); if (r) return r;
        r = dr.fetch(c, &after); if (r) return r;
        return d2h(c, out_tokens, c->out_tokens_dev, sizeof(int) * (size_t)n_steps);
    }, [&] { dr.commit(c, out_tokens, n_steps, after); });
}

// ParallelTransformer::generate (transformer.cpp:76-103) as one call: the prompt and ALL of max_tokens - 1 decode tokens go onto the stream at once (the graphs flm_decode_* replay:
// nothing new is captured), the loop's two decisions are taken on the device by every token's last act (flm_math.h gen_last_act) -- stop on `stop_token`: the latch, behind which
// the launches still queued return at their top; per-token callback: one granule per token into the page-locked ring, which this thread polls while the graphs replay.
// Correctness does not depend on the host SEEING a granule before the stream drains: what the poll did not deliver is delivered behind the synchronise, from out_tokens_dev.
namespace {
struct GenWords {     // the decode state's generate words hold for the enqueue of one attempt only: every other entry point's set_state writes -1 / 0 / 0
    flm_ctx* c;
    GenWords(flm_ctx* c_, int stop, unsigned tag, int max_tokens, bool rules) : c(c_) { c->gen_stop = stop; c->gen_tag = tag; c->gen_max = max_tokens; c->gen_rules = rules ? 1 : 0; }
    ~GenWords() { c->gen_stop = -1; c->gen_tag = 0; c->gen_max = 0; c->gen_rules = 0; }
};
inline void cpu_relax() {
#if defined(__x86_64__) || defined(__i386__)
    __builtin_ia32_pause();
#endif
}
}
// dr: flm_generate's plain plan, or flm_generate_ex's: where its form is shaped the block goes to the device first and every token takes that form
static int generate_impl(flm_ctx* c, const int32_t* prompt, int n_prompt, int pos, int max_tokens, const Draw& dr,
                         int32_t stop_token, flm_token_cb cb, void* user, int32_t* out_tokens, int* n_out) {
    if (!c || !prompt || !n_out) return FLM_ERR_INVALID;
    // (in front of everything else: a tensor-parallel rank must not touch a peer -- halting and cancelling across ranks is not built)
    if (sharded(c)) return fail(c, FLM_ERR_UNSUPPORTED, "generate: one GPU only (tensor-parallel callers keep the flm_decode_* loop)");
    if (max_tokens < 1 || !(dr.temperature >= 0.0f) || stop_token >= c->d.vocab_size) return fail(c, FLM_ERR_INVALID, "generate: max_tokens >= 1, temperature >= 0, stop_token < vocab_size (or -1)");
    int r = check_ready(c, n_prompt, pos); if (r) return r;
    if (pos + n_prompt + max_tokens - 1 > c->d.max_seq_len || max_tokens > c->out_cap || max_tokens > c->gen_cap) return fail(c, FLM_ERR_INVALID, "generate: pos + n_prompt + max_tokens - 1 exceeds max_seq_len");
    if (dr.coins()) { r = sample_args_ok(c, dr.temperature, dr.topp, dr.rng_state); if (r) return r; }
    volatile unsigned long long* ring = c->gen_host;
    int* cancel_word = (int*)((char*)c->gen_host + (((size_t)c->gen_cap * 8 + 63) & ~(size_t)63));
    int32_t* ids = c->gen_ids.data();
    // across the attempts of a retried call: how many tokens went to the callback (never delivered twice), whether it cancelled, how many were seen while the stream was busy
    int delivered = 0, streamed = 0, total = 0; bool cancelled = false;
    unsigned long long after = 0;                                     // the sampler's state behind the attempt's draws
    auto deliver = [&](int index, int32_t token, int last) {
        if (index < delivered) return;
        delivered = index + 1;
        if (cancelled || !cb) return;
        if (cb(user, index, token, last) != 0) { cancelled = true; __atomic_store_n(cancel_word, 1, __ATOMIC_RELEASE); }
    };
    r = with_retry(c, n_prompt + max_tokens - 1, [&]() -> int {
        // a tag per ATTEMPT: the granules a failed attempt left behind never carry the tag the next one polls for
        c->gen_seq += 1; if (c->gen_seq == 0) c->gen_seq = 1;
        const unsigned tag = c->gen_seq;
        // (the stream is idle: every entry point returns behind a synchronise.)  A call whose callback cancelled in an attempt that is now re-run starts with the word CLEAR:
        // the re-run must first reproduce the tokens the callback has already received -- the poll sets the word again once it has passed them, so *n_out never falls below
        // what was delivered
        __atomic_store_n(cancel_word, 0, __ATOMIC_RELEASE);
        {
            const GenWords words(c, stop_token < 0 ? -1 : stop_token, tag, max_tokens, dr.rules);       // (dr.rules: the plan is flm_generate_ex's and rules are installed)
            int r = dr.arm(c);
            if (!r) r = feed(c, prompt, n_prompt, pos, dr.form);              // token 0: drawn from the prompt's last logits
            if (!r && max_tokens > 1) r = run_tokens(c, pos + n_prompt, max_tokens - 1, dr.form);
            if (r) { (void)hipStreamSynchronize(c->stream); return r; }
        }
        // poll: the granules in index order as they arrive, until the one marked last -- or until the stream has drained (looked at every kPollsPerQuery empty polls: the
        // kernels' own waits are bounded, so the stream drains whatever happens, and the poll cannot spin for ever)
        constexpr int kPollsPerQuery = 512, kTokensPerQuery = 16;
        int next = 0, idle = 0, unconfirmed = 0; bool seen_last = false;
        while (!seen_last && next < max_tokens) {
            const unsigned long long g = __atomic_load_n(ring + next, __ATOMIC_ACQUIRE);
            if ((unsigned)(g >> 32) == tag) {
                const unsigned v = (unsigned)g;
                if (next >= delivered) ++unconfirmed;
                deliver(next, (int32_t)(v & 0x7fffffffu), (int)(v >> 31));
                seen_last = (v >> 31) != 0; ++next; idle = 0;
                if (cancelled && next >= delivered) __atomic_store_n(cancel_word, 1, __ATOMIC_RELEASE);      // (a re-run: behind the tokens the callback already has)
                // "gen_streamed": one look at the stream per kTokensPerQuery tokens (and behind the last one), not per token -- a stream still busy NOW was busy when the
                // tokens since the previous look were handed out
                if ((seen_last || next % kTokensPerQuery == 0) && unconfirmed) { if (hipStreamQuery(c->stream) == hipErrorNotReady) streamed += unconfirmed; unconfirmed = 0; }
                continue;
            }
            if (++idle % kPollsPerQuery == 0 && hipStreamQuery(c->stream) != hipErrorNotReady) break;
            cpu_relax();
        }
        (void)hipGetLastError();                                                    // (hipErrorNotReady is not an error of the call)
        HIPC(c, hipStreamSynchronize(c->stream));
        // behind the synchronise: how many tokens were drawn (the state's step counter: a halting token counts, nothing behind it ran), their ids, the sampler's state
        DecodeState stt{};
        int r = d2h(c, &stt, c->state, sizeof stt); if (r) return r;
        r = dr.fetch(c, &after); if (r) return r;
        total = stt.step < 1 ? 1 : stt.step > max_tokens ? max_tokens : stt.step;
        return d2h(c, ids, c->out_tokens_dev, sizeof(int) * (size_t)total);     // (the error word rides along: xwg_check looks at it next)
    }, [&] {
        for (int i = delivered; i < total; ++i) deliver(i, ids[i], i + 1 == total ? 1 : 0);
        if (out_tokens) memcpy(out_tokens, ids, sizeof(int32_t) * (size_t)total);
        *n_out = total;
        dr.commit(c, ids, total, after);                                  // (the stop token, when delivered, included; armed: record i is out_tokens[i]'s)
        c->gen_tokens = total; c->gen_streamed = streamed;
        stop_note(c, dr.rules, stop_token, ids, total, max_tokens);
    });
    return r;
}
int flm_generate(flm_ctx* c, const int32_t* prompt, int n_prompt, int pos, int max_tokens, float temperature, float topp, uint64_t* rng_state,
                 int32_t stop_token, flm_token_cb cb, void* user, int32_t* out_tokens, int* n_out) {
    return generate_impl(c, prompt, n_prompt, pos, max_tokens, Draw(temperature, topp, rng_state), stop_token, cb, user, out_tokens, n_out);
}
// flm_generate with the sampling controls (include/flm_gpu.h; the stage: flm_shape.h).  Every control neutral: flm_generate itself.  Otherwise the same call with the shaped
// token form: the controls, the bias pairs and the prompt's last penalty_last_n ids go to the device block first; the kernel assembles each token's window from that tail and
// the ids drawn so far (out_tokens_dev at the state's step), so a retried attempt rebuilds the same windows from the same ids.
int flm_generate_ex(flm_ctx* c, const int32_t* prompt, int n_prompt, int pos, int max_tokens, const flm_sampling* sampling, uint64_t* rng_state,
                    int32_t stop_token, flm_token_cb cb, void* user, int32_t* out_tokens, int* n_out) {
    if (!c || !prompt || !n_out) return FLM_ERR_INVALID;
    c->lp_count = -1;                                                 // (flm_last_logprobs: until this call has delivered armed)
    if (n_prompt < 1 || n_prompt > c->d.max_seq_len) return fail(c, FLM_ERR_INVALID, "tokens/pos outside [0, max_seq_len]");
    if (!ids_in_vocab(c, prompt, n_prompt)) return fail(c, FLM_ERR_INVALID, "token id out of range");
    const int tail = n_prompt < FLM_PENALTY_WINDOW_MAX ? n_prompt : FLM_PENALTY_WINDOW_MAX;
    Draw dr;
    if (int r = draw_resolve(c, sampling, prompt + (n_prompt - tail), tail, true, rng_state, dr, NoOwn(), true)) return r;
    return generate_impl(c, prompt, n_prompt, pos, max_tokens, dr, stop_token, cb, user, out_tokens, n_out);
}
// flm_forward_sample with the controls and the caller's window (used as given).  Every control neutral: flm_forward_sample / flm_forward_argmax.
int flm_forward_sample_ex(flm_ctx* c, const int32_t* tokens, int n, int pos, const flm_sampling* sampling, const int32_t* window, int n_window, uint64_t* rng_state, int32_t* next_token) {
    if (!c || !tokens || !next_token) return FLM_ERR_INVALID;
    c->lp_count = -1;
    Draw dr;
    if (int r = draw_resolve(c, sampling, window, n_window, false, rng_state, dr)) return r;
    if (!dr.shaped()) return dr.coins() ? flm_forward_sample(c, tokens, n, pos, dr.temperature, dr.topp, rng_state, next_token) : flm_forward_argmax(c, tokens, n, pos, next_token);
    if (sharded(c)) return fail(c, FLM_ERR_UNSUPPORTED, "shaped token: one GPU only");
    return forward_draw(c, tokens, n, pos, dr, next_token);
}

// Score a sequence: every position's logits in one batched pass, reduced on the device to a flm_score per row (flm_score.h).  The call is flm_forward's work plus the rows
// flm_forward drops: the batch of the first n - 1 tokens runs with its LAST layer completed (prefill_batched, all_layers), its final residual rows go through the output norm
// and the classifier on the GEMM tiles in chunks that fit the staging (score_classify), and the last token runs through the decode kernels exactly as in flm_forward -- so the
// cache rows, c->logits and the decode state are literally what flm_forward leaves.  Fewer than kPrefillMin + 1 tokens (the batches the layer kernels have never run at) and
// "use_prefill" 0: token by token, every token with its classifier.
static_assert(sizeof(flm_score) == sizeof(ScoreRow) && sizeof(flm_score) == 20, "flm_score is k_score_rows' ScoreRow");
int flm_score_tokens(flm_ctx* c, const int32_t* tokens, int n, int pos, const int32_t* targets, flm_score* out, float* logits_all) {
    if (!c || !tokens || !out) return fail(c, FLM_ERR_INVALID, "score: null argument");
    if (sharded(c)) return fail(c, FLM_ERR_UNSUPPORTED, "score: one GPU only (tensor-parallel scoring is not built)");
    int r = check_ready(c, n, pos); if (r) return r;
    const int V = c->d.vocab_size;
    if (!sample_supported(c)) return fail(c, FLM_ERR_UNSUPPORTED, "score: the vocabulary does not fit one workgroup's LDS (the device sampler's bound)");
    if (!ids_in_vocab(c, tokens, n)) return fail(c, FLM_ERR_INVALID, "token id out of range");
    for (int i = 0; targets && i < n; ++i) if (targets[i] < -1 || targets[i] >= V) return fail(c, FLM_ERR_INVALID, "score: target outside [0, vocab) and not -1");
    const size_t row_bytes = (size_t)V * 4;
    int chunk = 1; float* const stage = score_stage(c, &chunk);
    return with_retry(c, n, [&]() -> int {
        int r = h2d(c, c->prompt_dev, tokens, sizeof(int) * (size_t)n); if (r) return r;
        HIPC(c, hipStreamSynchronize(c->stream));                                    // (the ids have left the bounce buffer)
        int32_t* tg = c->gen_ids.data();                                             // (pageable staging of max_seq_len ids, there since create)
        for (int i = 0; i < n; ++i) tg[i] = targets ? targets[i] : (i + 1 < n ? tokens[i + 1] : -1);
        r = h2d(c, c->score_tgt, tg, sizeof(int) * (size_t)n); if (r) return r;
        const bool batched = c->use_prefill && n - 1 >= kPrefillMin;
        const int nb = batched ? n - 1 : 0;                                          // rows of the batch; the rest go through the decode kernels
        if (batched) {
            r = prefill_batched_qt(c, nb, pos, true); if (r) return r;
            for (int r0 = 0; r0 < nb; r0 += chunk) {
                const int m = nb - r0 < chunk ? nb - r0 : chunk;
                r = score_classify(c, r0, m, stage); if (r) return r;
                if (logits_all) for (int i = 0; i < m; ++i) { r = d2h(c, logits_all + (size_t)(r0 + i) * V, stage + (size_t)i * V, row_bytes); if (r) return r; }
            }
        }
        for (int i = nb; i < n; ++i) {
            r = set_state(c, pos + i, tokens[i], 0); if (r) return r;
            r = run_token(c, true, TokenForm::Logits, pos + i + 1); if (r) return r;
            r = launch_score_rows(c, c->stream, c->logits, 0, V, c->score_tgt + i, c->score_dev + i, 1); if (r) return r;
            if (logits_all) { r = d2h(c, logits_all + (size_t)i * V, c->logits, row_bytes); if (r) return r; }
        }
        return d2h(c, out, c->score_dev, sizeof(flm_score) * (size_t)n);       // (the error word rides along: xwg_check looks at it next)
    });
}

// Draft-and-verify (include/flm_gpu.h), greedy and sampled in one implementation.  A verify pass: first_token and the k drafts as ONE batch of k + 1 rows through the batched
// kernels with the last layer completed; row i's id a[i] is the id the token path draws behind first_token, a[0 .. i) -- as long as the drafts were those ids, so the accept
// step keeps a[0 .. m], m = the first i with a[i] != drafts[i].  Temperature 0: a[i] is the row's first maximum; no coin, the state untouched (rng_state may be null, the
// vocabulary is not bound by the sampler).  Otherwise: the sampler is a function of (logits, the coin), the coin of the sampled decode loop's i-th token is the i-th draw of
// its xorshift state, and a batched row's logits are flm_forward's bits: row i drawn with the (i + 1)-th coin of the step's state (k_sample_rows: the draw k_sample_advance
// makes, one function) is the id the loop draws; the accept step leaves the state after as many draws as ids it delivers, the coins drawn for the rows behind the cut are
// simply not counted.  Equality with flm_decode_sample, not rejection sampling.  Everything up to the result block's trip back is on the stream; nothing is allocated.
// shape (flm_verify_sample_ex with a control set): the shaper's block -- the controls, the caller's window as its head, penalty_last_n -- goes to the device in front of the
// batch, and k_shape_rows shapes every row over its own window (the head ++ the drafts in front of the row) before it is drawn.  The shaped row is a function of (raw row,
// window, controls) and the draw one of (shaped row, coin): row i is flm_forward_sample_ex's id behind first_token, a[0 .. i) for a caller who slides that window.
static int verify_impl(flm_ctx* c, int32_t first_token, const int32_t* drafts, int k, int pos, const Draw& dr, int32_t* out_tokens, int* n_out) {
    if (!c || !drafts || !out_tokens || !n_out) return fail(c, FLM_ERR_INVALID, "verify: null argument");
    if (sharded(c)) return fail(c, FLM_ERR_UNSUPPORTED, "verify: one GPU only");
    if (k < 4 || k > 15) return fail(c, FLM_ERR_INVALID, "verify: 4 <= k <= 15 drafts");
    if (!(dr.temperature >= 0.0f) || dr.topp != dr.topp) return fail(c, FLM_ERR_INVALID, "verify: temperature must be >= 0, top-p a number");
    int r = check_ready(c, k + 1, pos); if (r) return r;
    if (!ids_in_vocab(c, &first_token, 1)) return fail(c, FLM_ERR_INVALID, "token id out of range");
    if (!ids_in_vocab(c, drafts, k)) return fail(c, FLM_ERR_INVALID, "verify: draft outside [0, vocab)");
    if (dr.coins()) { r = sample_args_ok(c, dr.temperature, dr.topp, dr.rng_state); if (r) return r; }
    SpecOut so{};
    return with_retry(c, k + 1, [&]() -> int {
        int32_t* b = c->gen_ids.data();                                               // (pageable staging of max_seq_len ids, there since create)
        b[0] = first_token; for (int i = 0; i < k; ++i) b[1 + i] = drafts[i];
        int r = dr.arm_block(c); if (r) return r;
        r = h2d(c, c->prompt_dev, b, sizeof(int) * (size_t)(k + 1)); if (r) return r;
        // (the rows' windows: the block's head ++ the drafts; row r's record is out_tokens[r]'s)
        r = spec_step(c, pos, k, 0, 0, -1, k + 1, false, dr.batch(c, dr.coins() ? (unsigned long long)*dr.rng_state : 0ull, nullptr, 0, dr.cstate, 0)); if (r) return r;
        return d2h(c, &so, c->spec_res, sizeof so);                                   // (the ids and the state in one trip; the error word rides along: xwg_check looks at it next)
    }, [&] {
        memcpy(out_tokens, so.ids, sizeof(int32_t) * (size_t)so.n_emit);
        *n_out = so.n_emit;
        dr.commit(c, so.ids, so.n_emit, so.rng);
    });
}
int flm_verify_greedy(flm_ctx* c, int32_t first_token, const int32_t* drafts, int k, int pos, int32_t* out_tokens, int* n_out) {
    return verify_impl(c, first_token, drafts, k, pos, Draw(0.0f, 0.0f, nullptr), out_tokens, n_out);
}
int flm_verify_sample(flm_ctx* c, int32_t first_token, const int32_t* drafts, int k, int pos, float temperature, float topp, uint64_t* rng_state, int32_t* out_tokens, int* n_out) {
    return verify_impl(c, first_token, drafts, k, pos, Draw(temperature, topp, rng_state), out_tokens, n_out);
}
// flm_verify_sample with the controls: row r shaped over the last min(penalty_last_n, n_window + r) ids of window ++ drafts[0 .. r).  Every control neutral: flm_verify_sample.
int flm_verify_sample_ex(flm_ctx* c, int32_t first_token, const int32_t* drafts, int k, int pos, const flm_sampling* sampling, const int32_t* window, int n_window,
                         uint64_t* rng_state, int32_t* out_tokens, int* n_out) {
    if (!c || !drafts || !out_tokens || !n_out) return fail(c, FLM_ERR_INVALID, "verify: null argument");
    c->lp_count = -1;
    if (sharded(c)) return fail(c, FLM_ERR_UNSUPPORTED, "verify: one GPU only");
    Draw dr;
    const int r = draw_resolve(c, sampling, window, n_window, false, rng_state, dr, [&](ShapeParams& sp, bool& active) -> const char* {
        if (n_window > sampling->penalty_last_n) return "verify: n_window > penalty_last_n (row 0 takes the window as given)";
        // the rows' windows slide at penalty_last_n (the token form ignores it without follow); the drafts bring the penalties to life behind row 0 even where the caller's
        // window is empty
        const bool pen = sampling->repeat_penalty != 1.0f || sampling->frequency_penalty != 0.0f || sampling->presence_penalty != 0.0f;
        if (pen && sampling->penalty_last_n > 0) { sp.last_n = sampling->penalty_last_n; active = true; }
        return nullptr;
    }, false, true);
    if (r) return r;
    return verify_impl(c, first_token, drafts, k, pos, dr, out_tokens, n_out);
}

// flm_generate with several ids per pass over the weights: the prompt enters as in flm_forward_argmax / flm_forward_sample (token 0 is drawn from its last logits, with the
// first coin); then every step drafts draft_len tokens ON THE DEVICE from the call's history (k_spec_draft), verifies them in one batch of draft_len + 1 rows and accepts the
// longest prefix the model would have produced itself (k_spec_accept_sample: cut at the stop token and at max_tokens, appended to the history).  The batched kernels take the
// position as a launch argument, so the host reads the step's result block -- m, the ids and the state after the draws it delivers, one trip -- before it enqueues the next
// step: ONE synchronisation per step.  Where a batch would run past max_seq_len, or fewer than 2 ids are still wanted, the step is an ordinary one-launch greedy token or the
// sampled token graph (k_sample_advance reads the device parameter block, written from the host's state first) and the accept kernel with K = 0.  Every step is re-runnable:
// its inputs are the history below n_hist and launch arguments -- n_hist, room and the state the HOST holds at the step's start, so a re-run step draws the same coins --,
// which is what the retry wrapper needs.  The caller's state is written once, at the end.
// A shaped plan (flm_generate_lookup_ex with a control set; the block filled as flm_generate_ex fills it: follow, the prompt's tail as its head): token 0 is the shaped token form
// behind the prompt; a batch step's rows are shaped by k_shape_rows over the call's history in device memory (spec_hist[0 .. n_hist) ++ the drafts in front of the row, the
// window flm_generate_ex has at that token); a single-token step runs the shaped token graph with its window written into the block from the ids the host holds (follow 0:
// set_state has reset the step counter the follow form counts by).  Every step's inputs stay the history below n_hist, launch arguments and the block.
// The drafter is a parameter: d null = the prompt-lookup drafter above (the six lookup exports: what they enqueue is unchanged); d given (flm_generate_draft, ngram_max
// unused) = the paired draft context.  Then token 0's attempt also feeds the prompt to the draft (its own draw discarded), and a batch step drafts with the draft's
// device-resident token loop: joined in front of the target's batch (draft_open / draft_close), first what the draft lacks -- only ever the last draft of a step that
// accepted them all, which was never fed: one token, its output discarded --, then set_state {last id, at} and draft_len tokens, greedy at temperature 0, else the plain
// sampled form with the draft's sampler block written with the STEP's base state and the call's temperature / top-p: draft i is drawn with the (i + 1)-th coin, the coin
// k_sample_rows uses for row i of the batch -- where the two models agree on a row they draw the same id.  The controls, the constraint, the stop rules and the
// log-probability stage act on the target's rows only.  k_spec_take_drafts turns the draft's out_tokens_dev into the batch; no id goes through the host, and a step keeps
// its ONE synchronisation.  How many rows the draft has (d_rows) is host-held like n_hist, room and the state, so a re-run step -- after a wait that gave up in EITHER
// context: with_retry_pair -- enqueues the same work.  Single-token steps run on the target alone; what the draft lacks at the end is fed once before the call returns, so
// both caches hold pos + n_prompt + *n_out - 1 rows of the same sequence.
static int generate_lookup_impl(flm_ctx* c, const int32_t* prompt, int n_prompt, int pos, int max_tokens, const Draw& dr,
                                int32_t stop_token, int draft_len, int ngram_max, flm_token_cb cb, void* user, int32_t* out_tokens, int* n_out, flm_ctx* d = nullptr) {
    if (!c || !prompt || !n_out) return FLM_ERR_INVALID;
    if (sharded(c)) return fail(c, FLM_ERR_UNSUPPORTED, "generate_lookup: one GPU only");
    if (max_tokens < 1 || !(dr.temperature >= 0.0f) || dr.topp != dr.topp || stop_token >= c->d.vocab_size || draft_len < 4 || draft_len > 15 || ngram_max < 1 || ngram_max > 8)
        return fail(c, FLM_ERR_INVALID, "generate_lookup: max_tokens >= 1, temperature >= 0, stop_token < vocab_size (or -1), 4 <= draft_len <= 15, 1 <= ngram_max <= 8");
    int r = check_ready(c, n_prompt, pos); if (r) return r;
    if (pos + n_prompt + max_tokens - 1 > c->d.max_seq_len || max_tokens > c->out_cap) return fail(c, FLM_ERR_INVALID, "generate_lookup: pos + n_prompt + max_tokens - 1 exceeds max_seq_len");
    if (!ids_in_vocab(c, prompt, n_prompt)) return fail(c, FLM_ERR_INVALID, "token id out of range");
    if (d) {
        if (!model_complete(d)) return fail(c, FLM_ERR_STATE, "generate_draft: the draft model is not complete");
        if (pos + n_prompt + max_tokens - 1 > d->d.max_seq_len) return fail(c, FLM_ERR_INVALID, "generate_draft: pos + n_prompt + max_tokens - 1 exceeds the draft's max_seq_len");
        d->err_word_fresh = false;
    }
    const bool sampled = dr.coins();
    if (sampled) { r = sample_args_ok(c, dr.temperature, dr.topp, dr.rng_state); if (r) return r; }
    const TokenForm d_form = dr.temperature != 0.0f ? TokenForm::Sampled : TokenForm::Greedy;      // the draft's plain form
    int d_rows = pos, d_tokens = 0;                                  // draft: the cache rows it holds of this sequence / tokens it computed in this call
    const int stop = stop_token < 0 ? -1 : stop_token;
    int total = 0, steps = 0, accepted = 0; bool done = false, cancelled = false;
    int32_t last_tok = 0;
    // the running copies the host holds for re-runnable steps, handed to the plan's commit at the end: the sampler's state and the constraint's state behind the ids
    // delivered so far (the host folds every step's ids into it and passes the result on; armed for log-probabilities, record i is the call's i-th id's: the base is `total`)
    uint64_t state = sampled ? *dr.rng_state : 0;
    int cst = dr.cstate;
    int32_t* const drawn = c->gen_ids.data();                        // shaped: the ids delivered so far, for the single-token steps' windows and the finish reason (pageable, max_seq_len ids, there since create)
    const StopBlock* const rules = dr.rules ? c->stop_blk : nullptr;  // installed stop rules (flm_generate_lookup_ex): token 0 and every accept step evaluate them on the device
    SpecOut so{};
    auto deliver = [&]() {                       // the step's ids, in index order, on this thread; the state moves with them
        for (int i = 0; i < so.n_emit; ++i) {
            const int index = total + i;
            const bool last = i + 1 == so.n_emit && (so.stopped || index + 1 == max_tokens);
            if (out_tokens) out_tokens[index] = so.ids[i];
            drawn[index] = so.ids[i];
            if (cb && !cancelled && cb(user, index, so.ids[i], last ? 1 : 0) != 0) cancelled = true;
        }
        if (cst >= 0) cst = dfa_fold(c, cst, so.ids, so.n_emit);
        total += so.n_emit; last_tok = so.ids[so.n_emit - 1]; state = so.rng;
        done = so.stopped || total >= max_tokens || cancelled;
    };
    // token 0: the prompt, exactly as flm_forward_argmax / flm_forward_sample feeds it; the history starts as the prompt and that id
    r = with_retry_pair(c, d, n_prompt, n_prompt, [&]() -> int {
        int r = dr.arm(c); if (r) return r;
        if (d) {       // the draft feeds the same prompt at the same position, in front of the target (the streams joined: draft_open); its own draw is discarded
            r = draft_open(c, d); if (r) return r;
            r = draft_rc(c, d, feed(d, prompt, n_prompt, pos, TokenForm::Greedy)); if (r) return r;
            r = draft_close(c, d); if (r) return r;
        }
        r = feed(c, prompt, n_prompt, pos, dr.form); if (r) return r;
        hipLaunchKernelGGL(k_spec_begin, dim3(1), dim3(rules ? kSampleBlock : 256), 0, c->stream, c->spec_hist, (const int*)c->prompt_dev, n_prompt, (const int*)c->out_tokens_dev, c->spec_res, stop, (unsigned long long)state, sampled ? 1 : 0, rules);
        HIPC(c, hipGetLastError());
        if (d) { r = draft_err_along(c, d); if (r) return r; }
        return d2h(c, &so, c->spec_res, sizeof so);
    }, [&] { if (d) { d_rows = pos + n_prompt; d_tokens += n_prompt; } deliver(); });
    if (r) return r;
    while (!done) {
        const int at = pos + n_prompt + total - 1, room = max_tokens - total, n_hist = n_prompt + total;       // the last id is fed at `at`
        const bool batch = room >= 2 && at + draft_len + 1 <= c->d.max_seq_len && (!d || at + draft_len <= d->d.max_seq_len);
        const int d_lacks = d && batch ? at - d_rows : 0;                // rows the draft has to feed in front of its drafts (the ids the host holds: drawn)
        r = with_retry_pair(c, batch ? d : nullptr, batch ? draft_len + 1 : 1, d_lacks + draft_len, [&]() -> int {
            int r;
            if (batch && d) {       // the draft's side of the step, joined in front of the target's batch; nothing of it is copied back
                r = draft_open(c, d); if (r) return r;
                if (d_lacks > 0) { r = draft_rc(c, d, feed(d, drawn + (d_rows - pos - n_prompt), d_lacks, d_rows, TokenForm::Greedy)); if (r) return r; }
                if (sampled) { r = draft_rc(c, d, set_sample(d, dr.temperature, dr.topp, (unsigned long long)state)); if (r) return r; }
                r = draft_rc(c, d, set_state(d, at, last_tok, 0)); if (r) return r;
                r = draft_rc(c, d, run_tokens(d, at, draft_len, d_form)); if (r) return r;
                r = draft_close(c, d); if (r) return r;
            }
            if (batch) {       // (the block: as token 0's attempt left it; the rows' windows: the history; records land behind the ids delivered so far)
                r = spec_step(c, at, draft_len, ngram_max, n_hist, stop, room, true, dr.batch(c, state, c->spec_hist, n_hist, cst, total), rules, n_prompt, d);
            }
            else {      // one token through the token graph and the accept kernel with K = 0: the id from the decode state's first output slot, cut / appended / counted like a verified run of one
                // (its window, as given: the last min(last_n, n_hist) ids of prompt ++ drawn[0 .. total); the constraint's block: {the folded state, 0}; the record stage's: step 0 is record `total`)
                r = dr.arm_step(c, state, cst, total, prompt, n_prompt, drawn, total);
                if (r) return r;
                r = set_state(c, at, last_tok, 0); if (r) return r;
                r = run_token(c, true, dr.form, at + 1); if (r) return r;
                if (rules) hipLaunchKernelGGL(k_spec_accept_rules, dim3(1), dim3(kSampleBlock), 0, c->stream, c->spec_res, (const int*)c->out_tokens_dev, (const int*)c->prompt_dev, 0, c->spec_hist, n_prompt, n_hist, stop, room, (unsigned long long)state, sampled ? 1 : 0, rules);
                else hipLaunchKernelGGL(k_spec_accept_sample, dim3(1), dim3(64), 0, c->stream, c->spec_res, (const int*)c->out_tokens_dev, (const int*)c->prompt_dev, 0, c->spec_hist, n_hist, stop, room, (unsigned long long)state, sampled ? 1 : 0);
                r = hipGetLastError() == hipSuccess ? FLM_OK : fail(c, FLM_ERR_HIP, "generate_lookup: launch failed");
            }
            if (r) return r;
            return d2h(c, &so, c->spec_res, sizeof so);
        }, [&] {
            if (batch) { steps += 1; accepted += so.n_emit - 1; }
            // (the draft fed the last id and its first draft_len - 1 drafts: of the rows behind `at` as many are this sequence's as ids were delivered, draft_len at the most)
            if (batch && d) { d_rows = at + (so.n_emit < draft_len ? so.n_emit : draft_len); d_tokens += d_lacks + draft_len; }
            deliver();
        });
        if (r) return r;
    }
    if (d) {       // the draft is caught up before the call returns: what it lacks of pos + n_prompt + total - 1 rows, fed once (the target's stream is idle behind the last read-back)
        const int need = pos + n_prompt + total - 1, n = need - d_rows;
        if (n > 0) {
            r = with_retry(d, n, [&]() -> int { return feed(d, drawn + (d_rows - pos - n_prompt), n, d_rows, TokenForm::Greedy); });
            if (r) return draft_rc(c, d, r);
            d_tokens += n;
        }
        HIPC(c, hipStreamSynchronize(d->stream));
        c->draft_tokens = d_tokens;
    }
    *n_out = total;
    dr.commit(c, total, state, cst);
    c->spec_steps = steps; c->spec_accepted = accepted;
    stop_note(c, dr.rules, stop_token, drawn, total, max_tokens);
    return FLM_OK;
}
int flm_generate_lookup(flm_ctx* c, const int32_t* prompt, int n_prompt, int pos, int max_tokens, int32_t stop_token, int draft_len, int ngram_max,
                        flm_token_cb cb, void* user, int32_t* out_tokens, int* n_out) {
    return generate_lookup_impl(c, prompt, n_prompt, pos, max_tokens, Draw(0.0f, 0.0f, nullptr), stop_token, draft_len, ngram_max, cb, user, out_tokens, n_out);
}
int flm_generate_lookup_sample(flm_ctx* c, const int32_t* prompt, int n_prompt, int pos, int max_tokens, float temperature, float topp, uint64_t* rng_state,
                               int32_t stop_token, int draft_len, int ngram_max, flm_token_cb cb, void* user, int32_t* out_tokens, int* n_out) {
    return generate_lookup_impl(c, prompt, n_prompt, pos, max_tokens, Draw(temperature, topp, rng_state), stop_token, draft_len, ngram_max, cb, user, out_tokens, n_out);
}
// flm_generate_ex's ids through draft-and-verify steps.  Every control neutral: flm_generate_lookup_sample.
int flm_generate_lookup_ex(flm_ctx* c, const int32_t* prompt, int n_prompt, int pos, int max_tokens, const flm_sampling* sampling, uint64_t* rng_state, int32_t stop_token,
                           int draft_len, int ngram_max, flm_token_cb cb, void* user, int32_t* out_tokens, int* n_out) {
    if (!c || !prompt || !n_out) return FLM_ERR_INVALID;
    c->lp_count = -1;
    if (sharded(c)) return fail(c, FLM_ERR_UNSUPPORTED, "generate_lookup: one GPU only");
    if (n_prompt < 1 || n_prompt > c->d.max_seq_len) return fail(c, FLM_ERR_INVALID, "tokens/pos outside [0, max_seq_len]");
    if (!ids_in_vocab(c, prompt, n_prompt)) return fail(c, FLM_ERR_INVALID, "token id out of range");
    const int tail = n_prompt < FLM_PENALTY_WINDOW_MAX ? n_prompt : FLM_PENALTY_WINDOW_MAX;
    Draw dr;
    if (int r = draw_resolve(c, sampling, prompt + (n_prompt - tail), tail, true, rng_state, dr, NoOwn(), true, true)) return r;
    return generate_lookup_impl(c, prompt, n_prompt, pos, max_tokens, dr, stop_token, draft_len, ngram_max, cb, user, out_tokens, n_out);
}
// flm_generate_lookup_ex with the paired draft context (flm_draft_set) as the drafter: the same loop, the same plan.  sampling null: every control neutral at temperature 0.
int flm_generate_draft(flm_ctx* c, const int32_t* prompt, int n_prompt, int pos, int max_tokens, const flm_sampling* sampling, uint64_t* rng_state, int32_t stop_token,
                       int draft_len, flm_token_cb cb, void* user, int32_t* out_tokens, int* n_out) {
    if (!c || !prompt || !n_out) return FLM_ERR_INVALID;
    c->lp_count = -1;
    if (sharded(c)) return fail(c, FLM_ERR_UNSUPPORTED, "generate_draft: one GPU only");
    flm_ctx* const d = c->draft;
    if (!d) return fail(c, FLM_ERR_STATE, "generate_draft: no draft context attached (flm_draft_set)");
    if (n_prompt < 1 || n_prompt > c->d.max_seq_len) return fail(c, FLM_ERR_INVALID, "tokens/pos outside [0, max_seq_len]");
    if (!ids_in_vocab(c, prompt, n_prompt)) return fail(c, FLM_ERR_INVALID, "token id out of range");
    const int tail = n_prompt < FLM_PENALTY_WINDOW_MAX ? n_prompt : FLM_PENALTY_WINDOW_MAX;
    flm_sampling neutral{}; neutral.repeat_penalty = 1.0f;
    Draw dr;
    if (int r = draw_resolve(c, sampling ? sampling : &neutral, prompt + (n_prompt - tail), tail, true, rng_state, dr, NoOwn(), true, true)) return r;
    return generate_lookup_impl(c, prompt, n_prompt, pos, max_tokens, dr, stop_token, draft_len, 1, cb, user, out_tokens, n_out, d);
}

// Parallel sampling (include/flm_gpu.h; kernels: flm_fan.h; the batch pass: flm_prompt.hip prefill_batched with a FanDesc).  The layout is pure host arithmetic and the one
// place the capacity condition is written
int flm_fan_layout_for(int pos, int n_prompt, int max_tokens, int n, int max_seq_len, flm_fan_layout* out) {
    if (!out) return FLM_ERR_INVALID;
    const char* why = nullptr;
    if (n < 2 || n > FLM_FAN_MAX) why = "fan: n outside 2 .. FLM_FAN_MAX";
    else if (pos < 0 || n_prompt < 1 || max_tokens < 1 || max_seq_len < 1) why = "fan: pos >= 0, n_prompt >= 1, max_tokens >= 1";
    else if ((long long)pos + n_prompt + (long long)n * (max_tokens - 1) > max_seq_len) why = "fan: pos + n_prompt + n * (max_tokens - 1) exceeds max_seq_len";
    if (why) { g_last_error = why; return FLM_ERR_INVALID; }
    flm_fan_layout l{};
    l.shared_rows = pos + n_prompt; l.tail_rows = max_tokens - 1; l.n = n;
    for (int j = 0; j < n; ++j) l.base[j] = l.shared_rows + j * l.tail_rows;
    *out = l;
    return FLM_OK;
}
// The loop follows generate_lookup_impl's pattern: the prompt through feed (its last token leaves the logits), token 0 of every sequence drawn from that one row, then one
// step per token with ONE synchronisation (the result block).  The host holds every sequence's last id, state and the live mask; a step starts by writing them into its
// launches (k_fan_load, the by-value FanIn of the draw and accept kernels) and its kernels write nothing a re-run reads, which is what the retry wrapper needs.  Rows that
// finished stay in the batch -- they feed their last id again into their own tail rows -- and their outputs are dropped.
int flm_generate_n(flm_ctx* c, const int32_t* prompt, int n_prompt, int pos, int max_tokens, int n, float temperature, float topp, uint64_t* rng_states,
                   int32_t stop_token, flm_fan_cb cb, void* user, int32_t* out_tokens, int* n_out) {
    if (!c || !prompt || !out_tokens || !n_out) return FLM_ERR_INVALID;
    if (sharded(c)) return fail(c, FLM_ERR_UNSUPPORTED, "generate_n: one GPU only");
    flm_fan_layout lay{};
    if (flm_fan_layout_for(pos, n_prompt, max_tokens, n, c->d.max_seq_len, &lay)) { c->err = g_last_error; return FLM_ERR_INVALID; }
    if (!(temperature >= 0.0f) || topp != topp || stop_token >= c->d.vocab_size || (temperature != 0.0f && !rng_states))
        return fail(c, FLM_ERR_INVALID, "generate_n: temperature >= 0, top-p a number, stop_token < vocab_size (or -1), rng_states given at temperature != 0");
    if (!ids_in_vocab(c, prompt, n_prompt)) return fail(c, FLM_ERR_INVALID, "token id out of range");
    if (temperature != 0.0f && !sample_supported(c)) return fail(c, FLM_ERR_UNSUPPORTED, "device sampler: vocabulary too large for one workgroup's LDS (sample on the host)");
    if (c->hs > 128 || fan_lds_bytes(1, c->d.max_seq_len, c->hs) > kLdsMax) return fail(c, FLM_ERR_UNSUPPORTED, "generate_n: head sizes up to 128 (the multi-query attention's bound)");
    int r = check_ready(c, n_prompt, pos); if (r) return r;
    const bool draws = temperature != 0.0f;
    const int stop = stop_token < 0 ? -1 : stop_token, S = lay.shared_rows;
    FanIn in{}; in.live = (1u << n) - 1u;
    for (int j = 0; j < n; ++j) in.rng[j] = draws ? (unsigned long long)rng_states[j] : 0ull;
    int count[FLM_FAN_MAX] = {0};
    FanOut fo{};
    bool cancelled = false;
    auto accept = [&]() -> int {      // the step's last launch and its one trip back (the error word rides along: xwg_check looks at it next)
        hipLaunchKernelGGL(k_fan_accept, dim3(1), dim3(64), 0, c->stream, c->fan_res, (const int*)c->fan_drawn, (const unsigned long long*)c->fan_after, in, n, stop);
        HIPC(c, hipGetLastError());
        return d2h(c, &fo, c->fan_res, sizeof fo);
    };
    auto deliver = [&](int index) {   // a verified step's ids, in sequence order, on this thread; the host's copies move with them
        for (int j = 0; j < n; ++j) {
            if (!((in.live >> j) & 1u)) continue;
            const int32_t id = fo.ids[j];
            const bool last = !((fo.live >> j) & 1u) || index + 1 == max_tokens;
            out_tokens[(size_t)j * max_tokens + index] = id; count[j] = index + 1;
            in.ids[j] = id; in.rng[j] = fo.rng[j];
            if (cb && !cancelled && cb(user, j, index, id, last ? 1 : 0) != 0) cancelled = true;
        }
        in.live = fo.live;
    };
    // token 0: the prompt exactly as flm_forward feeds it; every sequence draws from the one row of logits with its own first coin
    r = with_retry(c, n_prompt, [&]() -> int {
        int r = feed(c, prompt, n_prompt, pos, TokenForm::Logits); if (r) return r;
        r = launch_sample_fan(c, c->stream, c->logits, 0, c->d.vocab_size, 0, n, temperature, topp, in, c->sort_buf, c->fan_drawn, c->fan_after); if (r) return r;
        return accept();
    }, [&] { deliver(0); });
    if (r) return r;
    const bool skinny = c->spec_gemm != 0;
    int chunk = 1; float* const stage = score_stage(c, &chunk);
    for (int index = 1; index < max_tokens && in.live && !cancelled; ++index) {
        FanDesc f{}; f.S = S; f.t = index - 1; f.n = n;
        for (int j = 0; j < n; ++j) f.base[j] = lay.base[j];
        r = with_retry(c, n, [&]() -> int {
            hipLaunchKernelGGL(k_fan_load, dim3(1), dim3(64), 0, c->stream, in, n, c->prompt_dev);
            HIPC(c, hipGetLastError());
            int r = prefill_batched_qt(c, n, S + f.t, true, skinny, &f); if (r) return r;
            for (int r0 = 0; r0 < n; r0 += chunk) {
                const int m = n - r0 < chunk ? n - r0 : chunk;
                r = fan_classify(c, r0, m, stage, skinny, temperature, topp, in); if (r) return r;
            }
            return accept();
        }, [&] { deliver(index); });
        if (r) return r;
    }
    long long total = 0;
    for (int j = 0; j < n; ++j) { n_out[j] = count[j]; total += count[j]; if (draws) rng_states[j] = in.rng[j]; }
    if (draws) c->sampled += total;
    // "stop_reason" over the whole call: cancel; else length where any sequence ran to max_tokens; else every sequence ended on the stop token
    bool any_full = false; for (int j = 0; j < n; ++j) any_full = any_full || count[j] == max_tokens;
    c->stop_reason = cancelled ? FLM_STOP_CANCEL : any_full ? FLM_STOP_LENGTH : FLM_STOP_TOKEN; c->stop_rule = 0;
    c->fan_lay = lay; for (int j = 0; j < FLM_FAN_MAX; ++j) c->fan_count[j] = j < n ? count[j] : 0;
    c->fan_valid = true;
    return FLM_OK;
}
int flm_fan_keep(flm_ctx* c, int seq) {
    if (!c) return FLM_ERR_INVALID;
    if (!c->fan_valid) return fail(c, FLM_ERR_INVALID, "fan_keep: no flm_generate_n precedes, or the cache was written since");
    if (seq < 0 || seq >= c->fan_lay.n) return fail(c, FLM_ERR_INVALID, "fan_keep: seq outside [0, n)");
    HIPC(c, hipSetDevice(c->device));
    const int rows = c->fan_count[seq] - 1;
    c->fan_valid = false;                                             // (the move overwrites tail 0's rows: once)
    if (seq > 0 && rows > 0) {
        hipLaunchKernelGGL(k_fan_keep, dim3(c->d.n_layers * c->heads_local), dim3(256), 0, c->stream, c->kcache, c->vcache, c->kv_rows, c->hs, c->fan_lay.base[seq], c->fan_lay.shared_rows, rows);
        HIPC(c, hipGetLastError());
        HIPC(c, hipStreamSynchronize(c->stream));
    }
    return FLM_OK;
}

// Cache slots (include/flm_gpu.h; kernels: flm_batch.h; the batch pass: flm_prompt.hip prefill_batched with a row origin / a SlotDesc).  The layout is pure host arithmetic
// and the one place the capacity condition is written
int flm_batch_layout_for(int n_slots, const int32_t* rows, int max_seq_len, flm_batch_layout* out) {
    if (!out || !rows) return FLM_ERR_INVALID;
    const char* why = nullptr;
    long long sum = 0;
    if (n_slots < 1 || n_slots > FLM_BATCH_MAX) why = "batch: n_slots outside 1 .. FLM_BATCH_MAX";
    else {
        for (int s = 0; s < n_slots && !why; ++s) { if (rows[s] < 1) why = "batch: a slot of fewer than 1 row"; sum += rows[s]; }
        if (!why && sum > max_seq_len) why = "batch: the slots' rows exceed max_seq_len";
    }
    if (why) { g_last_error = why; return FLM_ERR_INVALID; }
    flm_batch_layout l{};
    l.n_slots = n_slots;
    for (int s = 0, b = 0; s < n_slots; ++s) { l.base[s] = b; l.rows[s] = rows[s]; b += rows[s]; }
    *out = l;
    return FLM_OK;
}
// what every batch entry point behind open starts with: check_ready's work WITHOUT ending the batch
static int batch_ready(flm_ctx* c, const char* who) {
    if (!c) return FLM_ERR_INVALID;
    if (sharded(c)) return fail(c, FLM_ERR_UNSUPPORTED, "batch: one GPU only");
    if (!c->batch_open) { c->err = std::string(who) + ": no open batch (flm_batch_open), or the cache was written since"; g_last_error = c->err; return FLM_ERR_STATE; }
    c->err_word_fresh = false;
    HIPC(c, hipSetDevice(c->device));
    return FLM_OK;
}
int flm_batch_open(flm_ctx* c, const flm_batch_layout* layout) {
    if (!c || !layout) return FLM_ERR_INVALID;
    if (sharded(c)) return fail(c, FLM_ERR_UNSUPPORTED, "batch: one GPU only");
    if (!model_complete(c)) return fail(c, FLM_ERR_STATE, "batch_open before all tensors were uploaded");
    if (attn_lds_bytes(c->d.max_seq_len, c->hs) > kLdsMax) return fail(c, FLM_ERR_UNSUPPORTED, "batch: the one-query attention's LDS does not fit at this head size and max_seq_len");
    flm_batch_layout lay{};
    if (layout->n_slots < 1 || layout->n_slots > FLM_BATCH_MAX) return fail(c, FLM_ERR_INVALID, "batch: n_slots outside 1 .. FLM_BATCH_MAX");
    if (flm_batch_layout_for(layout->n_slots, layout->rows, c->d.max_seq_len, &lay)) { c->err = g_last_error; return FLM_ERR_INVALID; }
    for (int s = 0; s < lay.n_slots; ++s) if (layout->base[s] != lay.base[s]) return fail(c, FLM_ERR_INVALID, "batch: the layout is not flm_batch_layout_for's (base is the prefix sum of rows)");
    c->fan_valid = false;
    c->batch_lay = lay;
    for (auto& s : c->batch_slot) s = flm_ctx::BatchSlot{};
    c->batch_open = true;
    c->batch_passes = 0;
    return FLM_OK;
}
// the result block's trip back behind the accept step (the error word rides along: xwg_check looks at it next)
static int batch_accept(flm_ctx* c, const SlotIn& in, const SlotDesc& f, SlotOut* so) {
    hipLaunchKernelGGL(k_batch_accept, dim3(1), dim3(64), 0, c->stream, c->batch_res, (const int*)c->fan_drawn, (const unsigned long long*)c->fan_after, in, f);
    HIPC(c, hipGetLastError());
    return d2h(c, so, c->batch_res, sizeof *so);
}
// a verified draw of slot s: the host's copy of the slot moves behind it
static void batch_take(flm_ctx* c, int s, const SlotOut& so) {
    flm_ctx::BatchSlot& b = c->batch_slot[s];
    b.last = so.ids[s]; b.rng = so.rng[s]; b.n_out += 1;
    if (b.temp != 0.0f) c->sampled += 1;
    if ((so.finished >> s) & 1u) { b.live = false; b.reason = (b.stop >= 0 && b.last == b.stop) ? FLM_STOP_TOKEN : FLM_STOP_LENGTH; }
}
int flm_batch_join(flm_ctx* c, int slot, const flm_batch_req* q, int32_t* first_token, int* live) {
    if (!c || !q || !first_token || !live) return FLM_ERR_INVALID;
    int r = batch_ready(c, "batch_join"); if (r) return r;
    const flm_batch_layout& lay = c->batch_lay;
    if (slot < 0 || slot >= lay.n_slots) return fail(c, FLM_ERR_INVALID, "batch_join: slot outside the layout");
    flm_ctx::BatchSlot& b = c->batch_slot[slot];
    if (b.live || b.filling) return fail(c, FLM_ERR_INVALID, "batch_join: the slot's sequence is still running, or still taking in its prompt");
    if (!q->prompt || q->n_prompt < 1 || q->max_tokens < 1 || (long long)q->n_prompt + q->max_tokens - 1 > lay.rows[slot] || q->n_prompt > c->pf_cap || q->n_prompt > c->prompt_cap)
        return fail(c, FLM_ERR_INVALID, "batch_join: n_prompt >= 1, max_tokens >= 1, n_prompt + max_tokens - 1 <= the slot's rows");
    if (!(q->temperature >= 0.0f) || q->topp != q->topp || q->stop_token >= c->d.vocab_size)
        return fail(c, FLM_ERR_INVALID, "batch_join: temperature >= 0, top-p a number, stop_token < vocab_size (or -1)");
    if (!ids_in_vocab(c, q->prompt, q->n_prompt)) return fail(c, FLM_ERR_INVALID, "token id out of range");
    if (q->temperature != 0.0f && !sample_supported(c)) return fail(c, FLM_ERR_UNSUPPORTED, "device sampler: vocabulary too large for one workgroup's LDS (sample on the host)");
    const int n = q->n_prompt, stop = q->stop_token < 0 ? -1 : q->stop_token;
    // the draw's one row: row 0 of a SlotIn / SlotDesc of its own
    SlotIn in{}; in.rng[0] = (unsigned long long)q->rng_state; in.temp[0] = q->temperature; in.topp[0] = q->topp; in.stop[0] = stop; in.left[0] = q->max_tokens;
    for (int s = 0; s < lay.n_slots; ++s) if (c->batch_slot[s].live) in.live |= 1u << s;
    in.live |= 1u << slot;
    SlotDesc f{}; f.n = 1; f.slot[0] = slot; f.base[0] = lay.base[slot]; f.pos[0] = n - 1; f.rows[0] = lay.rows[slot];
    const bool skinny = c->spec_gemm != 0 && n <= kSkinnyTokens;
    int chunk = 1; float* const stage = score_stage(c, &chunk);
    SlotOut so{};
    return with_retry(c, n, [&]() -> int {
        int r = h2d(c, c->prompt_dev, q->prompt, sizeof(int) * (size_t)n); if (r) return r;
        r = prefill_batched_qt(c, n, 0, true, skinny, nullptr, lay.base[slot], nullptr); if (r) return r;
        r = batch_classify(c, n - 1, 0, 1, stage, skinny, in); if (r) return r;          // (only the prompt's last row goes through the classifier and the draw)
        return batch_accept(c, in, f, &so);
    }, [&] {
        b = flm_ctx::BatchSlot{};
        b.used = true; b.live = true; b.pos = n; b.max_tokens = q->max_tokens; b.stop = stop; b.temp = q->temperature; b.topp = q->topp;
        batch_take(c, slot, so);
        *first_token = b.last; *live = b.live ? 1 : 0;
        c->batch_passes += 1;
    });
}
int flm_batch_step(flm_ctx* c, flm_batch_out* out) {
    if (!c || !out) return FLM_ERR_INVALID;
    int r = batch_ready(c, "batch_step"); if (r) return r;
    const flm_batch_layout& lay = c->batch_lay;
    SlotIn in{}; SlotDesc f{};
    for (int s = 0; s < lay.n_slots; ++s) {
        const flm_ctx::BatchSlot& b = c->batch_slot[s];
        if (!b.live) continue;
        const int i = f.n++;
        f.slot[i] = s; f.base[i] = lay.base[s]; f.pos[i] = b.pos; f.rows[i] = lay.rows[s];
        in.ids[i] = b.last; in.rng[i] = b.rng; in.temp[i] = b.temp; in.topp[i] = b.topp; in.stop[i] = b.stop; in.left[i] = b.max_tokens - b.n_out;
        in.live |= 1u << s;
    }
    for (int s = 0; s < FLM_BATCH_MAX; ++s) out->ids[s] = -1;
    out->live = 0; out->finished = 0;
    if (!f.n) return FLM_OK;
    const int B = f.n;
    const bool skinny = c->spec_gemm != 0;
    int chunk = 1; float* const stage = score_stage(c, &chunk);
    SlotOut so{};
    return with_retry(c, B, [&]() -> int {
        hipLaunchKernelGGL(k_slots_load, dim3(1), dim3(64), 0, c->stream, in, B, c->prompt_dev);
        HIPC(c, hipGetLastError());
        int r = prefill_batched_qt(c, B, 0, true, skinny, nullptr, 0, &f); if (r) return r;
        for (int r0 = 0; r0 < B; r0 += chunk) {
            const int m = B - r0 < chunk ? B - r0 : chunk;
            r = batch_classify(c, r0, r0, m, stage, skinny, in); if (r) return r;
        }
        return batch_accept(c, in, f, &so);
    }, [&] {
        for (int i = 0; i < B; ++i) { c->batch_slot[f.slot[i]].pos += 1; batch_take(c, f.slot[i], so); }     // (the fed id's row is in the cache; the drawn one is the next to feed)
        for (int s = 0; s < FLM_BATCH_MAX; ++s) out->ids[s] = so.ids[s];
        out->live = so.live; out->finished = so.finished;
        c->batch_passes += 1;
    });
}
// Ragged passes (include/flm_gpu.h; kernels: flm_segs.h; the batch pass: flm_prompt.hip prefill_batched with a SegDesc).  The scheduling rule is pure host arithmetic
// and written here alone: every running slot's one step row first, in slot order; then the filling slots in ascending slot order, each min(pending, what is left of
// the budget) rows of its prompt; a slot that gets no rows has no segment
int flm_batch_plan_for(int n_slots, const int32_t* fed, const int32_t* pending, uint32_t running, int prompt_rows_max, flm_batch_plan* out) {
    if (!out || !fed || !pending) return FLM_ERR_INVALID;
    const char* why = nullptr;
    if (n_slots < 1 || n_slots > FLM_BATCH_MAX) why = "batch_plan: n_slots outside 1 .. FLM_BATCH_MAX";
    else if (prompt_rows_max < 0) why = "batch_plan: a negative budget of prompt rows";
    else if (n_slots < 32 && (running >> n_slots) != 0) why = "batch_plan: a running slot outside the layout";
    for (int s = 0; !why && s < n_slots; ++s) {
        if (fed[s] < 0 || pending[s] < 0 || (long long)fed[s] + pending[s] > 0x7fffffffLL) why = "batch_plan: fed and pending are row counts";
        else if (((running >> s) & 1u) && pending[s] > 0) why = "batch_plan: a slot cannot run and take in its prompt at once";
    }
    if (why) { g_last_error = why; return FLM_ERR_INVALID; }
    flm_batch_plan p{};
    for (int s = 0; s < n_slots; ++s) {
        if (!((running >> s) & 1u)) continue;
        flm_batch_seg& g = p.seg[p.n_segs++];
        g.slot = s; g.row0 = p.n_rows; g.n = 1; g.pos0 = fed[s]; g.draws = 1;
        p.n_rows += 1; p.n_step += 1; p.n_draws += 1;
    }
    long long budget = prompt_rows_max > 0 ? prompt_rows_max : 0x7fffffffLL;
    for (int s = 0; s < n_slots && budget > 0; ++s) {
        if (pending[s] < 1) continue;
        const int n = pending[s] < budget ? pending[s] : (int)budget;
        if ((long long)p.n_rows + n > 0x7fffffffLL) { g_last_error = "batch_plan: more rows than an int holds"; return FLM_ERR_INVALID; }
        flm_batch_seg& g = p.seg[p.n_segs++];
        g.slot = s; g.row0 = p.n_rows; g.n = n; g.pos0 = fed[s]; g.draws = n == pending[s] ? 1 : 0;
        p.n_rows += n; p.n_draws += g.draws; budget -= n;
    }
    *out = p;
    return FLM_OK;
}
int flm_batch_admit(flm_ctx* c, int slot, const flm_batch_req* q) {
    if (!c || !q) return FLM_ERR_INVALID;
    int r = batch_ready(c, "batch_admit"); if (r) return r;
    const flm_batch_layout& lay = c->batch_lay;
    if (slot < 0 || slot >= lay.n_slots) return fail(c, FLM_ERR_INVALID, "batch_admit: slot outside the layout");
    flm_ctx::BatchSlot& b = c->batch_slot[slot];
    if (b.live || b.filling) return fail(c, FLM_ERR_INVALID, "batch_admit: the slot's sequence is still running, or still taking in its prompt");
    if (!q->prompt || q->n_prompt < 1 || q->max_tokens < 1 || (long long)q->n_prompt + q->max_tokens - 1 > lay.rows[slot] || q->n_prompt > c->pf_cap || q->n_prompt > c->prompt_cap)
        return fail(c, FLM_ERR_INVALID, "batch_admit: n_prompt >= 1, max_tokens >= 1, n_prompt + max_tokens - 1 <= the slot's rows");
    if (!(q->temperature >= 0.0f) || q->topp != q->topp || q->stop_token >= c->d.vocab_size)
        return fail(c, FLM_ERR_INVALID, "batch_admit: temperature >= 0, top-p a number, stop_token < vocab_size (or -1)");
    if (!ids_in_vocab(c, q->prompt, q->n_prompt)) return fail(c, FLM_ERR_INVALID, "token id out of range");
    if (q->temperature != 0.0f && !sample_supported(c)) return fail(c, FLM_ERR_UNSUPPORTED, "device sampler: vocabulary too large for one workgroup's LDS (sample on the host)");
    b = flm_ctx::BatchSlot{};
    b.filling = true; b.prompt = q->prompt; b.n_prompt = q->n_prompt; b.fed = 0;
    b.max_tokens = q->max_tokens; b.stop = q->stop_token < 0 ? -1 : q->stop_token; b.temp = q->temperature; b.topp = q->topp; b.rng = (unsigned long long)q->rng_state;
    return FLM_OK;
}
int flm_batch_pass(flm_ctx* c, int prompt_rows_max, flm_batch_pass_out* out) {
    if (!c || !out) return FLM_ERR_INVALID;
    int r = batch_ready(c, "batch_pass"); if (r) return r;
    if (prompt_rows_max < 0) return fail(c, FLM_ERR_INVALID, "batch_pass: a negative budget of prompt rows");
    const flm_batch_layout& lay = c->batch_lay;
    int32_t fed[FLM_BATCH_MAX] = {0}, pending[FLM_BATCH_MAX] = {0};
    uint32_t running = 0, filling = 0;
    for (int s = 0; s < lay.n_slots; ++s) {
        const flm_ctx::BatchSlot& b = c->batch_slot[s];
        if (b.live) { running |= 1u << s; fed[s] = b.pos; }
        else if (b.filling) { filling |= 1u << s; fed[s] = b.fed; pending[s] = b.n_prompt - b.fed; }
    }
    for (int s = 0; s < FLM_BATCH_MAX; ++s) out->ids[s] = -1;
    out->live = 0; out->finished = 0; out->filling = 0;
    if (!running && !filling) return FLM_OK;
    flm_batch_plan plan{};
    if (flm_batch_plan_for(lay.n_slots, fed, pending, running, prompt_rows_max, &plan)) { c->err = g_last_error; return FLM_ERR_INVALID; }
    const int B = plan.n_rows, L = plan.n_step;
    if (B > c->pf_cap || B > c->prompt_cap) return fail(c, FLM_ERR_INVALID, "batch_pass: more rows than max_seq_len");
    // the pass's geometry, the step rows' SlotDesc, and the draw rows: the step rows, then the last row of every segment that completes its prompt (gathered behind them)
    SegDesc sg{}; SlotDesc fs{}; SlotDesc fd{}; SlotIn in_step{}; SlotIn in{}; GatherDesc ga{};
    sg.n_segs = plan.n_segs; sg.n_step = L; ga.dst0 = L;
    in.live = running;
    for (int i = 0; i < plan.n_segs; ++i) {
        const flm_batch_seg& g = plan.seg[i];
        const flm_ctx::BatchSlot& b = c->batch_slot[g.slot];
        sg.slot[i] = g.slot; sg.row0[i] = g.row0; sg.n[i] = g.n; sg.base[i] = lay.base[g.slot]; sg.pos0[i] = g.pos0; sg.rows[i] = lay.rows[g.slot];
        if (i < L) {
            fs.slot[i] = g.slot; fs.base[i] = lay.base[g.slot]; fs.pos[i] = b.pos; fs.rows[i] = lay.rows[g.slot]; fs.n = i + 1;
            in_step.ids[i] = b.last;
        } else {
            memcpy(c->pass_ids.data() + (g.row0 - L), b.prompt + g.pos0, sizeof(int32_t) * (size_t)g.n);
        }
        if (!g.draws) continue;
        const int j = fd.n++;                                        // the draw's row: a SlotIn / SlotDesc of the draw rows
        fd.slot[j] = g.slot; fd.base[j] = lay.base[g.slot]; fd.pos[j] = g.pos0 + g.n - 1; fd.rows[j] = lay.rows[g.slot];
        in.ids[j] = i < L ? b.last : b.prompt[b.n_prompt - 1]; in.rng[j] = b.rng; in.temp[j] = b.temp; in.topp[j] = b.topp; in.stop[j] = b.stop;
        in.left[j] = b.max_tokens - b.n_out;
        in.live |= 1u << g.slot;
        if (i >= L) ga.src[ga.n++] = g.row0 + g.n - 1;
    }
    const int D = fd.n;                                              // (= plan.n_draws; 0: a pass of unfinished chunks -- the cache rows only, nothing is classified)
    const bool skinny = c->spec_gemm != 0 && B <= kSkinnyTokens;
    int chunk = 1; float* const stage = score_stage(c, &chunk);
    SlotOut so{};
    return with_retry(c, B, [&]() -> int {
        int r = FLM_OK;
        if (B > L) { r = h2d(c, c->prompt_dev + L, c->pass_ids.data(), sizeof(int) * (size_t)(B - L)); if (r) return r; }
        if (L > 0) {
            hipLaunchKernelGGL(k_slots_load, dim3(1), dim3(64), 0, c->stream, in_step, L, c->prompt_dev);
            HIPC(c, hipGetLastError());
        }
        r = prefill_batched_qt(c, B, 0, D > 0, skinny, nullptr, 0, L > 0 ? &fs : nullptr, &sg); if (r) return r;
        if (ga.n > 0) {
            hipLaunchKernelGGL(k_gather_rows, dim3(1), dim3(256), 0, c->stream, c->pf_x, c->d.dim, ga);
            HIPC(c, hipGetLastError());
        }
        for (int r0 = 0; r0 < D; r0 += chunk) {
            const int m = D - r0 < chunk ? D - r0 : chunk;
            r = batch_classify(c, r0, r0, m, stage, skinny, in); if (r) return r;
        }
        return batch_accept(c, in, fd, &so);       // (D == 0: every slot delivers -1, live = the running slots; the one trip back carries the error word)
    }, [&] {
        for (int i = 0; i < plan.n_segs; ++i) {
            const flm_batch_seg& g = plan.seg[i];
            flm_ctx::BatchSlot& b = c->batch_slot[g.slot];
            if (i < L) { b.pos += 1; batch_take(c, g.slot, so); continue; }     // (the fed id's row is in the cache; the drawn one is the next to feed)
            b.fed += g.n;
            if (!g.draws) continue;
            b.filling = false; b.prompt = nullptr; b.used = true; b.live = true; b.pos = b.n_prompt;     // the prompt is in: the slot runs from the next pass on ...
            batch_take(c, g.slot, so);                                                                   // ... unless token 0 ended it
        }
        uint32_t still = 0;
        for (int s = 0; s < lay.n_slots; ++s) if (c->batch_slot[s].filling) still |= 1u << s;
        for (int s = 0; s < FLM_BATCH_MAX; ++s) out->ids[s] = so.ids[s];
        out->live = so.live; out->finished = so.finished; out->filling = still;
        c->batch_passes += 1;
    });
}
int flm_batch_state(flm_ctx* c, int slot, uint64_t* rng_state, int* n_out, int* stop_reason) {
    if (!c) return FLM_ERR_INVALID;
    if (!c->batch_open) return fail(c, FLM_ERR_STATE, "batch_state: no open batch (flm_batch_open), or the cache was written since");
    if (slot < 0 || slot >= c->batch_lay.n_slots) return fail(c, FLM_ERR_INVALID, "batch_state: slot outside the layout");
    const flm_ctx::BatchSlot& b = c->batch_slot[slot];
    if (rng_state) *rng_state = (uint64_t)b.rng;
    if (n_out) *n_out = b.n_out;
    if (stop_reason) *stop_reason = b.live ? 0 : b.reason;
    return FLM_OK;
}
int flm_batch_close(flm_ctx* c, int keep_slot) {
    if (!c) return FLM_ERR_INVALID;
    if (keep_slot < 0) { c->batch_open = false; return FLM_OK; }
    int r = batch_ready(c, "batch_close"); if (r) return r;
    if (keep_slot >= c->batch_lay.n_slots || !c->batch_slot[keep_slot].used || c->batch_slot[keep_slot].filling)
        return fail(c, FLM_ERR_INVALID, "batch_close: keep_slot outside the layout, a slot that never held a sequence, or one that is still taking in its prompt");
    const int base = c->batch_lay.base[keep_slot], len = c->batch_slot[keep_slot].pos;      // (pos: the rows the sequence has in the cache = n_prompt + n_out - 1)
    c->batch_open = false;
    // rows [base, base + len) -> [0, len).  base < len: source and destination overlap -- chunks of at most `base` rows, ascending, each launch's ranges disjoint (a chunk's
    // destination was the source of the chunks in front of it, which the stream has finished)
    for (int off = 0; base > 0 && off < len; off += base) {
        const int count = len - off < base ? len - off : base;
        hipLaunchKernelGGL(k_fan_keep, dim3(c->d.n_layers * c->heads_local), dim3(256), 0, c->stream, c->kcache, c->vcache, c->kv_rows, c->hs, base + off, off, count);
        HIPC(c, hipGetLastError());
    }
    HIPC(c, hipStreamSynchronize(c->stream));
    return FLM_OK;
}
int flm_generate_batch(flm_ctx* c, const flm_batch_req* reqs, int n, flm_fan_cb cb, void* user, int32_t* out_tokens, int stride, int* n_out, uint64_t* rng_out) {
    if (!c || !reqs || !out_tokens || !n_out) return FLM_ERR_INVALID;
    if (sharded(c)) return fail(c, FLM_ERR_UNSUPPORTED, "generate_batch: one GPU only");
    if (n < 1 || n > FLM_BATCH_MAX) return fail(c, FLM_ERR_INVALID, "generate_batch: n outside 1 .. FLM_BATCH_MAX");
    int32_t rows[FLM_BATCH_MAX];
    for (int j = 0; j < n; ++j) {
        if (reqs[j].n_prompt < 1 || reqs[j].max_tokens < 1 || reqs[j].max_tokens > stride || (long long)reqs[j].n_prompt + reqs[j].max_tokens - 1 > c->d.max_seq_len)
            return fail(c, FLM_ERR_INVALID, "generate_batch: n_prompt >= 1, 1 <= max_tokens <= stride, n_prompt + max_tokens - 1 <= max_seq_len");
        rows[j] = reqs[j].n_prompt + reqs[j].max_tokens - 1;
    }
    flm_batch_layout lay{};
    if (flm_batch_layout_for(n, rows, c->d.max_seq_len, &lay)) { c->err = g_last_error; return FLM_ERR_INVALID; }
    int r = flm_batch_open(c, &lay); if (r) return r;
    bool cancelled = false;
    unsigned live_mask = 0;
    for (int j = 0; j < n; ++j) n_out[j] = 0;
    if (c->batch_rows >= 0) {      // option "batch_rows": every request admitted, then ragged passes until nobody runs or fills; callbacks in (pass, slot) order
        for (int j = 0; j < n; ++j) { r = flm_batch_admit(c, j, &reqs[j]); if (r) { c->batch_open = false; return r; } }
        unsigned busy = 1;
        while (busy && !cancelled) {
            flm_batch_pass_out po{};
            r = flm_batch_pass(c, c->batch_rows, &po); if (r) { c->batch_open = false; return r; }
            for (int j = 0; j < n; ++j) {
                if (po.ids[j] < 0) continue;
                const int index = n_out[j];
                out_tokens[(size_t)j * stride + index] = po.ids[j]; n_out[j] = index + 1;
                if (cb && !cancelled && cb(user, j, index, po.ids[j], (po.finished >> j) & 1u ? 1 : 0) != 0) cancelled = true;
            }
            busy = po.live | po.filling;
        }
    }
    else
    for (int j = 0; j < n && !cancelled; ++j) {
        int32_t id = -1; int live = 0;
        r = flm_batch_join(c, j, &reqs[j], &id, &live); if (r) { c->batch_open = false; return r; }
        out_tokens[(size_t)j * stride] = id; n_out[j] = 1;
        if (live) live_mask |= 1u << j;
        if (cb && cb(user, j, 0, id, live ? 0 : 1) != 0) cancelled = true;
    }
    while (live_mask && !cancelled) {
        flm_batch_out bo{};
        r = flm_batch_step(c, &bo); if (r) { c->batch_open = false; return r; }
        for (int j = 0; j < n; ++j) {
            if (bo.ids[j] < 0) continue;
            const int index = n_out[j];
            out_tokens[(size_t)j * stride + index] = bo.ids[j]; n_out[j] = index + 1;
            if (cb && !cancelled && cb(user, j, index, bo.ids[j], (bo.finished >> j) & 1u ? 1 : 0) != 0) cancelled = true;
        }
        live_mask = bo.live;
    }
    bool any_full = false;
    for (int j = 0; j < n; ++j) {
        if (rng_out) rng_out[j] = (uint64_t)c->batch_slot[j].rng;
        any_full = any_full || (c->batch_slot[j].used && n_out[j] == reqs[j].max_tokens);
    }
    c->stop_reason = cancelled ? FLM_STOP_CANCEL : any_full ? FLM_STOP_LENGTH : FLM_STOP_TOKEN; c->stop_rule = 0;
    return flm_batch_close(c, -1);
}

// Constrained decoding (include/flm_gpu.h): the automaton lives in ONE device allocation made here, off the steady path; the shaped token graphs reach it through the block
// allocated at create, whose contents the launches below rewrite -- nothing is re-captured.
int flm_dfa_validate(const flm_dfa* dfa, int vocab) {
    if (const char* why = dfa_check(dfa, vocab)) { g_last_error = why; return FLM_ERR_INVALID; }
    return FLM_OK;
}
int flm_constraint_set(flm_ctx* c, const flm_dfa* dfa) {
    if (!c) return FLM_ERR_INVALID;
    if (sharded(c)) return fail(c, FLM_ERR_UNSUPPORTED, "constraint: one GPU only");
    if (!model_complete(c)) return fail(c, FLM_ERR_STATE, "constraint_set before all tensors were uploaded");
    if (dfa) if (const char* why = dfa_check(dfa, c->d.vocab_size)) return fail(c, FLM_ERR_INVALID, why);
    HIPC(c, hipSetDevice(c->device));
    HIPC(c, hipStreamSynchronize(c->stream));
    int* fresh = nullptr;
    if (dfa) {
        const size_t ns = (size_t)dfa->n_states, ne = (size_t)dfa->n_edges, words = ns + 1 + 2 * ne;
        if (hipMalloc((void**)&fresh, words * 4) != hipSuccess) { (void)hipGetLastError(); return fail(c, FLM_ERR_OOM, "constraint_set: out of device memory"); }
        hipError_t e = hipMemcpyAsync(fresh, dfa->row_ptr, (ns + 1) * 4, hipMemcpyHostToDevice, c->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(fresh + ns + 1, dfa->edge_token, ne * 4, hipMemcpyHostToDevice, c->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(fresh + ns + 1 + ne, dfa->edge_next, ne * 4, hipMemcpyHostToDevice, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess) { hipFree(fresh); HIPC(c, e); }
        c->dfa_row.assign(dfa->row_ptr, dfa->row_ptr + ns + 1); c->dfa_tok.assign(dfa->edge_token, dfa->edge_token + ne); c->dfa_nxt.assign(dfa->edge_next, dfa->edge_next + ne);
    } else { c->dfa_row.clear(); c->dfa_tok.clear(); c->dfa_nxt.clear(); }
    int* const old = c->dfa_dev;
    c->dfa_dev = fresh; c->dfa_state = -1;
    int r = set_dfa(c, -1); if (r) return r;                                  // the block: the new arrays, disarmed
    HIPC(c, hipStreamSynchronize(c->stream));
    if (old) HIPC(c, hipFree(old));                                           // (behind the block's rewrite: no launch can still name the old arrays)
    return FLM_OK;
}
int flm_constraint_arm(flm_ctx* c, int32_t state) {
    if (!c) return FLM_ERR_INVALID;
    const int ns = (int)c->dfa_row.size() - 1;
    if (state != -1 && (ns < 1 || state < 0 || state >= ns)) return fail(c, FLM_ERR_INVALID, ns < 1 ? "constraint_arm: no automaton installed" : "constraint_arm: state outside [0, n_states)");
    if (state == -1 && ns < 1) { c->dfa_state = -1; return FLM_OK; }
    HIPC(c, hipSetDevice(c->device));
    int r = set_dfa(c, state); if (r) return r;
    c->dfa_state = state;
    return FLM_OK;
}

// Stop rules (include/flm_gpu.h; the matcher: flm_stop.h; the host restatement: host/stop_rules.h).  The block exists since flm_ctx_create: installing rules rewrites its
// contents through the bounce buffer (one small copy kernel on the context's stream) -- no allocation, no graph touched
int flm_stop_validate(const flm_stop_rules* r, int vocab) {
    if (const char* why = flmhost::stop_check(r, vocab)) { g_last_error = why; return FLM_ERR_INVALID; }
    return FLM_OK;
}
int flm_stop_match(const flm_stop_rules* r, int32_t stop_token, const int32_t* ids, int n, int* kind, int* rule) {
    int k = FLM_STOP_LENGTH, ru = 0;
    const int first = ids && n > 0 ? flmhost::stop_match(r, stop_token, ids, n, &k, &ru) : (n > 0 ? n : 0);
    if (kind) *kind = k;
    if (rule) *rule = ru;
    return first;
}
int flm_stop_set(flm_ctx* c, const flm_stop_rules* r) {
    if (!c) return FLM_ERR_INVALID;
    if (sharded(c)) return fail(c, FLM_ERR_UNSUPPORTED, "stop rules: one GPU only");
    if (!model_complete(c)) return fail(c, FLM_ERR_STATE, "stop_set before all tensors were uploaded");
    if (!sample_supported(c)) return fail(c, FLM_ERR_UNSUPPORTED, "stop rules: the vocabulary does not fit one workgroup's LDS (the device sampler's bound)");
    if (r) if (const char* why = flmhost::stop_check(r, c->d.vocab_size)) return fail(c, FLM_ERR_INVALID, why);
    static_assert(kStopIdsMax == FLM_STOP_IDS_MAX && kStopSeqsMax == FLM_STOP_SEQS_MAX && kStopSeqLenMax == FLM_STOP_SEQ_LEN_MAX, "flm_stop.h mirrors the header's limits");
    static_assert(sizeof(StopBlock) % 4 == 0, "whole words");
    StopBlock b{};
    if (r) {
        b.n_ids = r->n_ids; b.n_seqs = r->n_seqs; b.n_tok = r->n_seqs > 0 ? r->seq_ptr[r->n_seqs] : 0;
        for (int i = 0; i < r->n_ids; ++i) b.ids[i] = r->ids[i];
        for (int s = 0; s <= r->n_seqs && r->n_seqs > 0; ++s) b.seq_ptr[s] = r->seq_ptr[s];
        for (int k = 0; k < b.n_tok; ++k) b.seq_tok[k] = r->seq_tokens[k];
    }
    HIPC(c, hipSetDevice(c->device));
    HIPC(c, hipStreamSynchronize(c->stream));
    // (a HIP error between the pieces of the copy would leave the device block half rewritten: the host copy, which alone decides whether a call looks at the block, then says "none")
    int rc = h2d(c, c->stop_blk, &b, sizeof b);
    if (!rc && hipStreamSynchronize(c->stream) != hipSuccess) rc = fail(c, FLM_ERR_HIP, "stop_set: the copy of the rule block failed");   // (`b` has left the bounce buffer; the next call's first launch sees the block)
    c->stop_host = rc ? StopBlock{} : b;
    return rc;
}

// The entropy-driven samplers (include/flm_gpu.h; the stages: flm_entropy.h; the host restatement: host/sampler.cpp entropy_logits).  A context setting like
// flm_logprobs_arm: the block and the entropy token graphs exist since flm_ctx_create / flm_prepare, so the setting changes the host copy and nothing else -- the block is
// rewritten from it at the start of every attempt (Draw::arm)
int flm_entropy_validate(const flm_entropy* e) {
    if (const char* why = entropy_check(e)) { g_last_error = why; return FLM_ERR_INVALID; }
    return FLM_OK;
}
int flm_entropy_set(flm_ctx* c, const flm_entropy* e) {
    if (!c) return FLM_ERR_INVALID;
    if (e) if (const char* why = entropy_check(e)) return fail(c, FLM_ERR_INVALID, why);
    if (sharded(c)) return fail(c, FLM_ERR_UNSUPPORTED, "entropy: one GPU only");
    if (!sample_supported(c) || !c->ent_blk) return fail(c, FLM_ERR_UNSUPPORTED, "entropy: the vocabulary does not fit one workgroup's LDS (the device sampler's bound)");
    if (!model_complete(c)) return fail(c, FLM_ERR_STATE, "entropy_set before all tensors were uploaded");
    const int mode = !e ? 0 : e->mirostat == 2 ? 2 : typical_on(e->typical_p) ? 1 : 0;
    c->ent = mode ? *e : flm_entropy{};
    c->ent_mode = mode;
    return FLM_OK;
}
int flm_entropy_mu(flm_ctx* c, float* mu) {
    if (!c || !mu) return FLM_ERR_INVALID;
    if (c->ent_mode != 2) return fail(c, FLM_ERR_STATE, "entropy_mu: Mirostat is not set");
    *mu = c->ent.mu;
    return FLM_OK;
}

// Per-token log-probabilities (include/flm_gpu.h; the stage: flm_logprob.h).  A context setting like flm_constraint_arm: the block, the records and the armed token graphs
// exist since flm_ctx_create / flm_prepare, so arming rewrites the block's contents and nothing else
static_assert(sizeof(flm_logprob) == sizeof(LogprobRec) && sizeof(flm_logprob) == 192 && FLM_LOGPROBS_MAX == kLogprobsMax, "flm_logprob is the stage's LogprobRec");
int flm_logprobs_arm(flm_ctx* c, int top_n, int source) {
    if (!c) return FLM_ERR_INVALID;
    if (top_n < -1 || top_n > FLM_LOGPROBS_MAX || (source != FLM_LOGPROBS_RAW && source != FLM_LOGPROBS_SHAPED)) return fail(c, FLM_ERR_INVALID, "logprobs_arm: top_n outside [-1, FLM_LOGPROBS_MAX] or source not 0 / 1");
    if (sharded(c)) return fail(c, FLM_ERR_UNSUPPORTED, "logprobs: one GPU only");
    if (!sample_supported(c) || !c->lp_rec) return fail(c, FLM_ERR_UNSUPPORTED, "logprobs: the vocabulary does not fit one workgroup's LDS (the device sampler's bound)");
    if (!model_complete(c)) return fail(c, FLM_ERR_STATE, "logprobs_arm before all tensors were uploaded");
    HIPC(c, hipSetDevice(c->device));
    const int old_n = c->lp_top_n, old_s = c->lp_source;
    c->lp_top_n = top_n; c->lp_source = source;
    const int r = set_lp(c, 0);
    if (r) { c->lp_top_n = old_n; c->lp_source = old_s; }
    return r;
}
// the stage's own duration: `iters` launches of k_logprob_token back to back between ONE pair of events on the context's stream (flm_kernel_times' way: launch duration +
// the dependent-dispatch gap), on the rows and the decode state the last armed call left -- every launch rewrites that call's last record with the same bytes
int flm_logprob_stage_time(flm_ctx* c, int iters, float* avg_us) {
    if (!c || !avg_us || iters < 1) return FLM_ERR_INVALID;
    if (!lp_armed(c) || c->lp_count < 1) return fail(c, FLM_ERR_STATE, "logprob_stage_time: behind an armed _ex call that delivered ids");
    HIPC(c, hipSetDevice(c->device));
    EvPair ev; HIPC(c, hipEventCreate(&ev.e0)); HIPC(c, hipEventCreate(&ev.e1));
    int r = launch_logprob_token(c, c->stream); if (r) return r;      // (one launch outside the events: the first one's set-up)
    HIPC(c, hipEventRecord(ev.e0, c->stream));
    for (int i = 0; i < iters && !r; ++i) r = launch_logprob_token(c, c->stream);
    if (r) return r;
    HIPC(c, hipEventRecord(ev.e1, c->stream));
    HIPC(c, hipEventSynchronize(ev.e1));
    float ms = 0.0f; HIPC(c, hipEventElapsedTime(&ms, ev.e0, ev.e1));
    *avg_us = ms * 1000.0f / (float)iters;
    return FLM_OK;
}
int flm_last_logprobs(flm_ctx* c, int first, int n, flm_logprob* out) {
    if (!c || !out) return FLM_ERR_INVALID;
    if (c->lp_count < 0 || !c->lp_rec) return fail(c, FLM_ERR_STATE, "last_logprobs: the last _ex call ran disarmed or failed, or there was none");
    if (first < 0 || n < 1 || first > c->lp_count - n) return fail(c, FLM_ERR_INVALID, "last_logprobs: first + n passes the call's n_out");
    HIPC(c, hipSetDevice(c->device));
    return d2h(c, out, c->lp_rec + first, sizeof(flm_logprob) * (size_t)n);      // (through the bounce buffer, in pieces of its size: the one place records cross the bus)
}

// the ids the last flm_decode_greedy / flm_decode_sample / flm_decode_timed* call generated (still in device memory): out[n]
int flm_last_tokens(flm_ctx* c, int n, int32_t* out) {
    if (!c || !out || n < 1 || n > c->out_cap) return FLM_ERR_INVALID;
    HIPC(c, hipSetDevice(c->device));
    return d2h(c, out, c->out_tokens_dev, sizeof(int) * (size_t)n);
}

// the same loop with an event after every token: ms_each[n_steps] (for a median; the events cost a few us per token, so the
// headline figure comes from flm_decode_timed)
int flm_decode_timed_each(flm_ctx* c, int32_t first_token, int pos, int n_steps, float* ms_each) {
    if (!ms_each || !c || n_steps < 1) return FLM_ERR_INVALID;
    int r = check_ready(c, n_steps, pos); if (r) return r;
    if (first_token < 0 || first_token >= c->d.vocab_size || n_steps > c->out_cap) return fail(c, FLM_ERR_INVALID, "token id / steps out of range");
    struct Evs { std::vector<hipEvent_t> e; ~Evs() { for (auto x : e) if (x) hipEventDestroy(x); } } ev;
    ev.e.assign((size_t)n_steps + 1, nullptr);
    for (auto& x : ev.e) HIPC(c, hipEventCreate(&x));
    r = set_state(c, pos, first_token, 0); if (r) return r;
    HIPC(c, hipEventRecord(ev.e[0], c->stream));
    for (int i = 0; i < n_steps; ++i) { r = run_token(c, true, TokenForm::Greedy, pos + i + 1); if (r) return r; HIPC(c, hipEventRecord(ev.e[i + 1], c->stream)); }
    HIPC(c, hipEventSynchronize(ev.e[n_steps]));
    for (int i = 0; i < n_steps; ++i) HIPC(c, hipEventElapsedTime(&ms_each[i], ev.e[i], ev.e[i + 1]));
    r = xwg_check(c);
    return r == FLM_RETRY ? fail(c, FLM_ERR_HIP, "cross-workgroup wait timed out while timing") : r;
}

} // extern "C"
