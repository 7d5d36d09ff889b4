// flm_shape.h -- the logit-shaping stage of the "shaped" token form: classifier -> k_shape_logits -> k_sample_advance, and of a verify batch under the sampling controls:
// classifier GEMM -> k_shape_rows -> k_sample_rows / k_argmax_rows (one workgroup per row, each row over a window of its own, in place).  Both kernels are shape_row behind
// their own window arithmetic.  One 1024-thread workgroup turns the raw logits row L
// into the shaped row S (a row of its own, vocab floats, allocated at flm_ctx_create) that the UNCHANGED sampler (flm_sample.h sample_draw) then reads.  No reference
// counterpart: the reference samples with temperature and top-p only.  The definition (restated sequentially in host/sampler.cpp shape_logits, which this
// kernel equals bit for bit), all arithmetic fp32 round-to-nearest without contraction:
//   0 constraint a context armed with a token-level DFA at state q (the host restatement: host/sampler.cpp constrain_logits): S = L; S[i] = -inf for
//                every i without an edge in q.  The state's sorted edge list is scattered, 32768 indices at a time, into a bit map in the `hist` area (free until top-k) with
//                integer LDS atomics; one pass clears what has no bit.  A masked entry stays -inf under steps 1 - 4 (-inf + b = -inf for every allowed bias)
//   1 bias       S = L; S[id] += b for each of n_bias distinct ids (b finite or -inf)
//   2 penalties  for every DISTINCT id t of the window W[0 .. w), c = its occurrences: x = S[t]; repeat_penalty != 1: x = x > 0 ? x / rp : x * rp; frequency or presence
//                != 0: x = x - ((float)c * fp + pp); S[t] = x.  Window entry j belongs to thread j; the thread of an id's FIRST occurrence counts and writes: no order dependence
//   3 top-k      0 < k < n: keep the k entries first in (larger value, then lower index), -0.0 == +0.0; the rest -> -inf.  A radix select over an order-preserving 32-bit key
//                (-0.0 canonicalised): four 8-bit passes, most significant digit first, each an integer LDS histogram of the entries that match the prefix so far; they leave the
//                threshold key and `need`, how many threshold-equal entries to admit; those are the `need` lowest indices, found by an index-ordered count (ballot + per-wave
//                bases, as the radix sort of flm_sample.h ranks its elements).  Integer atomics only; nothing depends on the order in which waves run
//   4 min-p      min_p > 0 and temperature != 0: y = S[i] / temperature over the entries that are not -inf, mx = max y, S[i] = -inf where y - mx < lt; lt = logf(min_p) comes
//                from the HOST (glibc) as a parameter: no logarithm is evaluated here
// A stage whose control is neutral writes nothing, so with every control neutral S is L bit for bit.  The rows stay in global memory (L2-resident: a few passes over 4 * n
// bytes), so there is no vocabulary bound; LDS holds the window (<= 1024 ids), four 256-bin histograms and a few scan words.
// The window at generated step s (ShapeParams::follow): the last min(last_n, n_head + s) ids of head[0 .. n_head) -- the tail of the call's prompt, uploaded at the start of
// the call -- followed by out_tokens[0 .. s), the ids this call has drawn so far (s = DecodeState::step); follow == 0: head[0 .. n_head) as given (flm_forward_sample_ex).
// Part of flm_kernels.h; include that header.
#pragma once
#include "flm_math.h"
#include "flm_sample.h"
#pragma clang fp contract(off)

namespace flm {

constexpr int kShapeWindowMax = 1024;      // == FLM_PENALTY_WINDOW_MAX
constexpr int kShapeBiasMax = 256;         // == FLM_BIAS_MAX
// the per-call parameter block in device memory (written at the start of each call; the shaped token graphs read it)
struct ShapeParams {
    float temperature;                     // min-p's divisor (the sampler's own copy lives in SampleParams)
    float lt; int minp_on;                 // logf(min_p) from the host; min_p > 0
    int top_k;
    float repeat; float freq; float pres;
    int last_n;                            // follow: penalty_last_n
    int n_head; int follow;
    int n_bias;
    int pad_;
    int bias_ids[kShapeBiasMax]; float bias_vals[kShapeBiasMax];
    int head[kShapeWindowMax];
};
// The constraint's device block (allocated at flm_ctx_create; flm_constraint_set / flm_constraint_arm / Draw::arm rewrite its contents, so the token graphs captured at
// flm_prepare with its ADDRESS as their argument follow an automaton that arrives or changes later).  CSR: the edges of state s are [row_ptr[s], row_ptr[s + 1]), their tokens
// strictly ascending (flm_dfa_validate).  q: the state of the token at generated step `applied` (-1: disarmed); k_shape_logits moves the pair on
struct DfaBlock {
    const int* row_ptr; const int* edge_token; const int* edge_next;
    int n_states;
    int q, applied;
    int pad_;
};
// delta(q, t): the edge_next of t's edge in q (binary search in the sorted list), q itself where t has no edge there.  q in [0, n_states)
__device__ __forceinline__ int dfa_step(const DfaBlock* d, const int ns, const int q, const int t) {
    int lo = d->row_ptr[q], hi = d->row_ptr[q + 1];
    while (lo < hi) { const int mid = lo + ((hi - lo) >> 1); if (d->edge_token[mid] < t) lo = mid + 1; else hi = mid; }
    if (lo < d->row_ptr[q + 1] && d->edge_token[lo] == t) return min(max(d->edge_next[lo], 0), ns - 1);
    return q;
}
struct ShapeArgs {
    const float* logits; float* out; int n;
    const ShapeParams* p;
    const DecodeState* st;                 // the latch and, under follow, the step; null: flm_op_shape_logits
    const int* out_tokens; int out_cap;
    DfaBlock* dfa;                         // the constraint's block (q < 0: none); null: flm_op_shape_logits
};

// larger float <-> larger key; -0.0 and +0.0 share a key
__device__ __forceinline__ unsigned shape_key(float x) {
    unsigned u = __float_as_uint(x);
    if (u == 0x80000000u) u = 0u;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// the LDS of one row's shaping: the window (<= 1024 ids), four 256-bin histograms, the scan words
struct ShapeLds {
    int win[kShapeWindowMax];
    int hist[4 * 256];
    int misc[64];                          // [0..15] per-wave words, [16] digit, [17] rem, [18] equal-count, [20..35] per-wave floats, [40] the constraint's state
};
constexpr int kMaskChunk = 4 * 256 * 32;   // indices one bit map in ShapeLds::hist covers
// one state's edge list (step 0's allowed ids); ne < 0: no constraint
struct ShapeMask { const int* tok; int ne; };
// The window of one row: entry j = element skip + j of a[0 .. na) followed by b[..], j < w; both kernels below describe their window this way (k_shape_logits: the block's
// head and the ids drawn so far; k_shape_rows: the base window and the batch's drafts in front of the row)
struct ShapeWindow { const int* a; int na; const int* b; int skip; int w; };

// The radix select of step 3 (and of flm_logprob.h's top-N) by one 1024-thread workgroup: the key that is K-th in descending order among keyf(i), i < n (0 < K <= n) -- four
// 8-bit passes, most significant digit first, each an integer LDS histogram of the entries that match the prefix so far.  Returns that threshold key; *need: how many
// threshold-equal entries belong to the first K, *eqc: how many there are (need <= eqc).  hist: 4 * 256 words, misc: 64 words ([16] digit, [17] rem, [18] equal-count: read
// by every thread on return, so a caller writes them only behind a barrier of its own).  Integer atomics only; nothing depends on the order in which waves run
template <class KF>
__device__ __forceinline__ unsigned radix_select(KF keyf, const int n, const int K, int* const hist, int* const misc, int* need, int* eqc) {
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    for (int k = t; k < 4 * 256; k += kSampleBlock) hist[k] = 0;
    if (t == 0) misc[17] = K;
    __syncthreads();
    unsigned prefix = 0u;              // the digits chosen so far, in the key's top bits
#pragma unroll 1
    for (int d = 0; d < 4; ++d) {
        const int shift = 24 - 8 * d;
        int* h = hist + d * 256;
#pragma unroll 1
        for (int b0 = 0; b0 < n; b0 += kSampleBlock) {
            const int i = b0 + t;
            bool valid = i < n;
            unsigned key = 0u;
            if (valid) { key = keyf(i); valid = d == 0 || (key >> (shift + 8)) == (prefix >> (shift + 8)); }
            const unsigned dig = (key >> shift) & 255u;
            // the lanes of this wave with the same digit add once, through their lowest lane
            unsigned long long m = __ballot(valid);
#pragma unroll
            for (int bb = 0; bb < 8; ++bb) { const unsigned long long bm = __ballot((dig >> bb) & 1u); m &= ((dig >> bb) & 1u) ? bm : ~bm; }
            if (valid && (m & ((1ull << lane) - 1ull)) == 0ull) atomicAdd(&h[dig], __popcll(m));
        }
        __syncthreads();
        if (wv == 0) {
            // the digit at which the count from the top reaches rem: lane l holds bins 4l .. 4l + 3
            const int rem = misc[17];
            const int a0 = h[4 * lane], a1 = h[4 * lane + 1], a2 = h[4 * lane + 2], a3 = h[4 * lane + 3];
            const int s = a0 + a1 + a2 + a3;
            int suf = s;
            for (int o = 1; o < 64; o <<= 1) { const int u = __shfl_down(suf, o, kWave); if (lane + o < 64) suf += u; }
            int above = suf - s;       // entries in the bins of higher lanes
            const int bins[4] = {a3, a2, a1, a0};
            int fd = -1, frem = 0, feq = 0;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                if (fd < 0 && above < rem && above + bins[q] >= rem) { fd = 4 * lane + 3 - q; frem = rem - above; feq = bins[q]; }
                above += bins[q];
            }
            if (fd >= 0) { misc[16] = fd; misc[17] = frem; misc[18] = feq; }
        }
        __syncthreads();
        prefix |= (unsigned)misc[16] << shift;
    }
    *need = misc[17]; *eqc = misc[18];
    return prefix;
}

// Steps 0 - 4 of the definition on ONE row, by one 1024-thread workgroup: L[0 .. n) -> S[0 .. n) (S == L: shaped in place, the copy is skipped).  THE definition: k_shape_logits
// (the shaped token form) and k_shape_rows (the rows of a verify batch) are both this function behind their own window and state arithmetic
__device__ __forceinline__ void shape_row(const float* L, float* S, const int n, const ShapeParams* p, const ShapeWindow wd, const ShapeMask mk, ShapeLds& lds) {
    int* const win = lds.win; int* const hist = lds.hist; int* const misc = lds.misc;
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    // 1: the copy, then the biases (distinct ids: one writer per entry)
    if (S != L) {
        for (int i = t; i < n; i += kSampleBlock) S[i] = L[i];
        __syncthreads();
    }
    // 0: the constraint.  Per chunk of 32768 indices: clear the bit map, the threads stride over the edge list and set the bits of the tokens inside the chunk, one pass
    // writes -inf where the bit is clear.  Any list length, any n; the order in which waves run changes nothing (OR is commutative)
    if (mk.ne >= 0) {
        unsigned* const bitmap = (unsigned*)hist;
#pragma unroll 1
        for (int c0 = 0; c0 < n; c0 += kMaskChunk) {
            bitmap[t] = 0u;                // (4 * 256 words, kSampleBlock threads)
            __syncthreads();
            for (int e = t; e < mk.ne; e += kSampleBlock) {
                const unsigned o = (unsigned)(mk.tok[e] - c0);
                if (o < (unsigned)kMaskChunk) atomicOr(&bitmap[o >> 5], 1u << (o & 31u));
            }
            __syncthreads();
            const int c1 = min(n, c0 + kMaskChunk);
            for (int i = c0 + t; i < c1; i += kSampleBlock) { const unsigned o = (unsigned)(i - c0); if (!((bitmap[o >> 5] >> (o & 31u)) & 1u)) S[i] = -INFINITY; }
            __syncthreads();
        }
    }
    const int nb = min(p->n_bias, kShapeBiasMax);
    if (t < nb) { const int id = p->bias_ids[t]; if ((unsigned)id < (unsigned)n) S[id] = __fadd_rn(S[id], p->bias_vals[t]); }
    // 2: the window into LDS, then one thread per entry
    const int w = wd.w;
    const float rp = p->repeat, fp = p->freq, pp = p->pres;
    const bool rep_on = rp != 1.0f, fpp_on = fp != 0.0f || pp != 0.0f;
    if (w > 0 && (rep_on || fpp_on)) {
        if (t < w) { const int g = wd.skip + t; win[t] = g < wd.na ? wd.a[g] : wd.b[g - wd.na]; }
        __syncthreads();
        if (t < w) {
            const int id = win[t];
            int c = 0; bool first = true;
            for (int k = 0; k < w; ++k) { const bool same = win[k] == id; c += same ? 1 : 0; first = first && !(same && k < t); }
            if (first && (unsigned)id < (unsigned)n) {
                float x = S[id];
                if (rep_on) x = x > 0.0f ? __fdiv_rn(x, rp) : __fmul_rn(x, rp);
                if (fpp_on) x = __fsub_rn(x, __fadd_rn(__fmul_rn((float)c, fp), pp));
                S[id] = x;
            }
        }
    }
    __syncthreads();
    // 3: top-k
    const int K = p->top_k;
    if (K > 0 && K < n) {
        int need, eqc;
        const unsigned T = radix_select([&](int i) { return shape_key(S[i]); }, n, K, hist, misc, &need, &eqc);
        if (need >= eqc) {
            // every threshold-equal entry is admitted (no tie at the cut): one pass
            for (int i = t; i < n; i += kSampleBlock) if (shape_key(S[i]) < T) S[i] = -INFINITY;
        } else {
            int base = 0;                  // threshold-equal entries in front of this block of 1024 indices
#pragma unroll 1
            for (int b0 = 0; b0 < n; b0 += kSampleBlock) {
                const int i = b0 + t;
                const unsigned key = i < n ? shape_key(S[i]) : 0u;
                const bool eq = i < n && key == T;
                const unsigned long long m = __ballot(eq);
                if (lane == 0) misc[wv] = __popcll(m);
                __syncthreads();
                int before = base, all = 0;
                for (int k = 0; k < kSampleWaves; ++k) { const int c = misc[k]; before += k < wv ? c : 0; all += c; }
                const int rank = before + __popcll(m & ((1ull << lane) - 1ull));
                if (i < n && (key < T || (eq && rank >= need))) S[i] = -INFINITY;
                base += all;
                __syncthreads();
            }
        }
        __syncthreads();
    }
    // 4: min-p
    const float temp = p->temperature;
    if (p->minp_on && temp != 0.0f) {
        float mx = -INFINITY;
        for (int i = t; i < n; i += kSampleBlock) { const float x = S[i]; if (x != -INFINITY) mx = fmaxf(mx, __fdiv_rn(x, temp)); }
        mx = wave_max(mx);
        if (lane == 0) misc[20 + wv] = __float_as_int(mx);
        __syncthreads();
        mx = __int_as_float(misc[20]);
        for (int k = 1; k < kSampleWaves; ++k) mx = fmaxf(mx, __int_as_float(misc[20 + k]));
        const float lt = p->lt;
        for (int i = t; i < n; i += kSampleBlock) { const float x = S[i]; if (x != -INFINITY && __fsub_rn(__fdiv_rn(x, temp), mx) < lt) S[i] = -INFINITY; }
    }
}

inline __global__ void __launch_bounds__(kSampleBlock) k_shape_logits(const ShapeArgs a) {
    __shared__ ShapeLds lds;
    if (a.st != nullptr && halted(&a.st->halt)) return;
    const ShapeParams* p = a.p;
    int w = min(max(p->n_head, 0), kShapeWindowMax);
    int skip = 0;
    const int nh = w;
    if (p->follow) {
        const int s = a.st ? min(max(a.st->step, 0), a.out_cap) : 0;
        const int total = nh + s;
        w = min(min(max(p->last_n, 0), kShapeWindowMax), total);
        skip = total - w;
    }
    // the constraint: thread 0 moves {q, applied} on over the ids drawn since (out_tokens[applied .. s): normally one), stores the pair and hands q to the workgroup.  A
    // retried attempt starts from the pair Draw::arm wrote, {the armed state, 0}, and rebuilds the same states from the ids it draws again
    ShapeMask mk{nullptr, -1};
    if (a.dfa != nullptr) {
        static_assert(kSampleBlock == 4 * 256, "one bit-map word per thread");
        if (threadIdx.x == 0) {
            DfaBlock* d = a.dfa;
            const int ns = d->n_states;
            int q = d->q;
            if (q >= 0 && ns > 0) {
                q = min(q, ns - 1);
                const int s = (p->follow && a.st) ? min(max(a.st->step, 0), a.out_cap) : 0;
                for (int j = min(max(d->applied, 0), s); j < s; ++j) q = dfa_step(d, ns, q, a.out_tokens[j]);
                d->q = q; d->applied = s;
            } else q = -1;
            lds.misc[40] = q;
        }
        __syncthreads();
        const int q = lds.misc[40];
        if (q >= 0) { const int e0 = a.dfa->row_ptr[q]; mk.tok = a.dfa->edge_token + e0; mk.ne = a.dfa->row_ptr[q + 1] - e0; }
    }
    shape_row(a.logits, a.out, a.n, p, ShapeWindow{p->head, nh, a.out_tokens, skip, w}, mk, lds);
}

// The shaper over the rows of a verify batch's classifier chunk: one 1024-thread workgroup per row, grid = the chunk's rows (<= 16); block r shapes batch row row0 + r (the
// convention of k_sample_rows).  The window of batch row i is the one the shaped token loop has when it draws that token PROVIDED the drafts in front of the row were the
// loop's ids -- the only case in which the accept step keeps the row: the last w = min(last_n, n_base + i) ids of base[0 .. n_base) ++ drafts[0 .. i), last_n the block's.
// w <= 1024 whatever n_base is.  No latch: a verify batch has none.  out == logits: in place (the verify pass: its staged rows are never returned)
struct ShapeRowsArgs {
    const float* logits; int ld;           // the chunk's rows, ld floats apart
    float* out; int ld_out;
    int n; int row0;
    const ShapeParams* p;                  // the controls, the bias pairs, last_n
    const int* base; int n_base;           // flm_verify_sample_ex: the caller's window (the block's head); flm_generate_lookup_ex: the call's history
    const int* drafts;                     // the batch's drafts d[0 .. 15): row i looks at d[0 .. i)
    // the constraint: the batch's base state as a launch argument (-1: none), like n_base and the coin state; row i is masked in delta folded over d[0 .. i) from it -- the
    // loop's state for that token exactly when the accept step keeps the row (the windows' argument).  states_out (may be null; flm_op_constrain_rows): [16], row i's state
    const DfaBlock* dfa; int state; int* states_out;
};
inline __global__ void __launch_bounds__(kSampleBlock) k_shape_rows(const ShapeRowsArgs a) {
    __shared__ ShapeLds lds;
    const int r = blockIdx.x, row = a.row0 + r;
    const int nbase = max(a.n_base, 0);
    const int total = nbase + row;
    const int w = min(min(max(a.p->last_n, 0), kShapeWindowMax), total);
    ShapeMask mk{nullptr, -1};
    if (a.dfa != nullptr && a.state >= 0) {
        if (threadIdx.x == 0) {            // at most 15 searches: cheaper than a dependency between the rows, as with the xorshift steps
            const int ns = a.dfa->n_states;
            int q = -1;
            if (ns > 0) {
                q = min(a.state, ns - 1);
                for (int j = 0; j < row; ++j) q = dfa_step(a.dfa, ns, q, a.drafts[j]);
                if (a.states_out) a.states_out[row] = q;
            }
            lds.misc[40] = q;
        }
        __syncthreads();
        const int q = lds.misc[40];
        if (q >= 0) { const int e0 = a.dfa->row_ptr[q]; mk.tok = a.dfa->edge_token + e0; mk.ne = a.dfa->row_ptr[q + 1] - e0; }
    }
    shape_row(a.logits + (size_t)r * a.ld, a.out + (size_t)r * a.ld_out, a.n, a.p, ShapeWindow{a.base, nbase, a.drafts, total - w, w}, mk, lds);
}

} // namespace flm
