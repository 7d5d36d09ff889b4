// flm_spec.h -- draft-and-verify (flm_verify_greedy / flm_generate_lookup and their sampled forms, one implementation: flm_gpu.hip verify_impl / generate_lookup_impl): the
// prompt-lookup drafter, the per-row argmax of a batch's logits and the accept step.  Part of flm_kernels.h; include that header.  The weight pass of a verify batch is the
// prompt path's (flm_prefill.h: the tiles, or k_gemm_q8_skinny).
//
// A step: k_spec_draft writes the batch's tokens {h[n - 1], d[0 .. K)}; the batched layer kernels and the classifier produce K + 1 rows of logits; row i is reduced to
// a[i]; k_spec_accept_sample keeps a[0 .. m] where m is the first i with a[i] != d[i] -- a[i] is the id the token path would draw behind a[0 .. i), because row i saw
// exactly those tokens -- and leaves the sampler's state after as many draws as the step delivers ids.
//   temperature 0: a[i] = the row's first maximum (k_argmax_rows: sample_argmax, sampler.cpp:36-47: block_first_max, what k_argmax_advance computes); no coin, the state
//                  passes through untouched;
//   otherwise:     k_sample_rows (flm_sample.h) draws row i with the (i + 1)-th coin of the step's xorshift state, i.e. Sampler::sample as the sampled decode loop calls
//                  it for its i-th token.  The ids are flm_decode_sample's element for element; nothing is rejected or re-drawn.
// With a draft MODEL as the drafter (flm_generate_draft) k_spec_take_drafts takes k_spec_draft's place: the batch's drafts are the ids a second context's token loop drew.
#pragma once
#include "flm_sample.h"

namespace flm {

// what a step leaves for the host, read back in ONE trip: the accepted run ids[0 .. n_emit) and the sampler's state after exactly n_emit draws -- one per id the step
// delivers, so the next step's row 0 draws with the coin the sampled decode loop uses for that token.  (Not m + 1 draws: `room` and the stop token can cut the run
// shorter; the rows behind the cut drew coins the loop never does.)  Temperature 0: the state the step started from.
struct SpecOut { int m; int n_emit; int stopped; int pad; int ids[16]; unsigned long long rng; };

// The prompt-lookup drafter over the token history h[0 .. n), n >= 1 (host restatement: host/spec_draft.h, pinned by tests/test_spec_host.py):
//   for g = min(ngram_max, n - 1) down to 1: the LARGEST j with j + g <= n - 1 and h[j .. j + g) == h[n - g .. n); the first g with a match wins, period p = n - g - j;
//   d[i] = h[n - p + i] for i < p, else d[i - p] (the history continued periodically); no match at any g: d[i] = h[n - 1].
// Evaluated in one pass: for every end e = j + g in [1, n - 1] the length len(e) of the common suffix of h[0 .. e) and h[0 .. n), capped at min(ngram_max, e); the
// rule's g is the maximum of len, its j + g the largest e that reaches it.  The key (len << 24 | e) is reduced with max -- order-free, so the result does not depend on
// which wave or workgroup finishes first.  One workgroup of 1024 threads; n < 2^24.  Writes batch[0] = h[n - 1], batch[1 + i] = d[i], i < K.
inline __global__ void __launch_bounds__(kSampleBlock) k_spec_draft(const int* __restrict__ h, int n, int K, int ngram_max, int* __restrict__ batch) {
    __shared__ unsigned red[kSampleWaves];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    unsigned best = 0;
    for (int e = 1 + t; e <= n - 1; e += kSampleBlock) {
        const int cap = ngram_max < e ? ngram_max : e;
        int len = 0;
        while (len < cap && h[e - 1 - len] == h[n - 1 - len]) ++len;
        const unsigned key = len ? ((unsigned)len << 24) | (unsigned)e : 0u;
        best = key > best ? key : best;
    }
    for (int o = 32; o > 0; o >>= 1) { const unsigned ov = (unsigned)__shfl_xor((int)best, o, kWave); best = ov > best ? ov : best; }
    if (lane == 0) red[w] = best;
    __syncthreads();
    best = red[0];
    for (int k = 1; k < kSampleWaves; ++k) best = red[k] > best ? red[k] : best;
    if (t == 0) batch[0] = h[n - 1];
    if (t < K) {
        int v = h[n - 1];
        if (best) { const int e = (int)(best & 0xffffffu), p = n - e; v = h[e + t % p]; }
        batch[1 + t] = v;
    }
}

// The model-based drafter's hand-off (flm_generate_draft): the K ids a DRAFT context's device-resident token loop left in its out_tokens_dev become the verify batch of the
// target, in the layout k_spec_draft leaves -- batch[0] = h[n - 1], batch[1 + i] = draft_out[i], i < K -- so everything behind it is the lookup loop's.  Runs on the
// target's stream behind a wait on the draft's event; no draft id travels to the host.  An id outside [0, vocab) (impossible with a sound draft of the same vocabulary) is
// replaced by h[n - 1]: a re-run step never indexes the embedding out of range, and a wrong draft costs acceptance, never an id.  err_src -> err_dst: the draft context's
// "a cross-workgroup wait gave up" word rides along to the target's page-locked line, where the host finds it behind the step's ONE read-back.  One wave.
inline __global__ void __launch_bounds__(kWave) k_spec_take_drafts(const int* __restrict__ h, int n, const int* __restrict__ draft_out, int K, int vocab, int* __restrict__ batch,
                                                                   const int* __restrict__ err_src, int* __restrict__ err_dst) {
    const int t = threadIdx.x;
    if (blockIdx.x != 0) return;
    const int last = h[n - 1];
    if (t == 0) { batch[0] = last; if (err_src) *err_dst = *err_src; }
    if (t < K) { const int d = draft_out[t]; batch[1 + t] = d >= 0 && d < vocab ? d : last; }
}

// a[r] = the first maximum of row r of logits[rows][ld], n entries: one workgroup of 1024 threads per row
inline __global__ void __launch_bounds__(kSampleBlock) k_argmax_rows(const float* __restrict__ logits, int ld, int n, int* __restrict__ out) {
    __shared__ int red[2 * kSampleWaves];
    const float* x = logits + (size_t)blockIdx.x * ld;
    const int a = block_first_max([&](int i) { return x[i]; }, n, 0, red);
    if (threadIdx.x == 0) out[blockIdx.x] = a;
}

// The accept step (one thread): m = the first i < K with a[i] != batch[1 + i] (K if none); the run a[0 .. m] is cut to `room` ids (what the call may still deliver)
// and behind the first `stop` id (-1: none), stored into out->ids and, where hist is given, appended at hist[n_hist ..).  K = 0: one id from a single-token launch.
// out->rng = base after n_emit steps of the xorshift state when `draws`, else base.  n_hist, room and base (the state at the step's start) come from the host (it learns m
// every step), so a step that is re-run stores the same words again.
inline __global__ void k_spec_accept_sample(SpecOut* out, const int* __restrict__ a, const int* __restrict__ batch, int K, int* hist, int n_hist, int stop, int room,
                                            unsigned long long base, int draws) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    int m = 0;
    while (m < K && a[m] == batch[1 + m]) ++m;
    int n = m + 1 < room ? m + 1 : room, stopped = 0;
    for (int i = 0; i < n; ++i) if (a[i] == stop) { n = i + 1; stopped = 1; break; }
    for (int i = 0; i < n; ++i) { const int id = a[i]; out->ids[i] = id; if (hist) hist[n_hist + i] = id; }
    out->m = m; out->n_emit = n; out->stopped = stopped; out->pad = 0;
    unsigned long long s = base;
    if (draws) for (int i = 0; i < n; ++i) s = sample_step(s);
    out->rng = s;
}
// The accept step under stop rules (flm_stop_set; flm_generate_lookup_ex): the same words as k_spec_accept_sample, with the run also cut behind the first index at which a
// rule fires.  The ids this call has delivered are hist[n_prompt .. n_hist); the run a[0 .. n) follows them, so the matcher's t[j] is hist[n_prompt + j] below n_gen =
// n_hist - n_prompt and a[j - n_gen] from there on -- ids in front of n_prompt are never read.  One workgroup of 1024 threads: thread 0 finds m and the cut at `room` as
// before, the workgroup evaluates stop_match (flm_stop.h) at the run's n indices -- the mismatch words alternate between two sets, one barrier per index --, thread 0 keeps
// the first index that fires or holds the stop token and stores the block.  hist must be given (the loop's call; flm_verify_sample_ex ignores the rules)
inline __global__ void __launch_bounds__(kSampleBlock) k_spec_accept_rules(SpecOut* out, const int* __restrict__ a, const int* __restrict__ batch, int K, int* hist, int n_prompt,
                                                                           int n_hist, int stop, int room, unsigned long long base, int draws, const StopBlock* rules) {
    __shared__ unsigned lds[2][kStopLdsWords];
    __shared__ int run[2];
    if (threadIdx.x == 0) {
        int m = 0;
        while (m < K && a[m] == batch[1 + m]) ++m;
        run[0] = m; run[1] = m + 1 < room ? m + 1 : room;
    }
    __syncthreads();
    const int m = run[0], n_gen = n_hist - n_prompt;
    int n = run[1], stopped = 0;
    const bool armed = stop_armed(rules);
    const int* const h = hist + n_prompt;
    int cut = n;
    for (int i = 0; i < n; ++i) {
        const int id = a[i];
        bool ends = id == stop;
        if (armed) ends = stop_match(rules, id, [&](int j) { return j < n_gen ? h[j] : a[j - n_gen]; }, n_gen + i, lds[i & 1]).kind != 0 || ends;
        if (ends && cut == n && !stopped) { cut = i + 1; stopped = 1; }       // (valid in wave 0; thread 0 stores)
    }
    if (threadIdx.x != 0) return;
    n = cut;
    for (int i = 0; i < n; ++i) { const int id = a[i]; out->ids[i] = id; hist[n_hist + i] = id; }
    out->m = m; out->n_emit = n; out->stopped = stopped; out->pad = 0;
    unsigned long long s = base;
    if (draws) for (int i = 0; i < n; ++i) s = sample_step(s);
    out->rng = s;
}
// flm_generate_lookup's start: the history = the prompt and the id drawn from its last logits (tok0[0], the decode state's first output slot); the whole result block of
// that one id (the state after its one draw).  rules (may be null; then launched with any block size): index 0 of the call stops on a listed id or a sequence of length 1
// too -- launched with 1024 threads, the matcher's workgroup
inline __global__ void __launch_bounds__(kSampleBlock) k_spec_begin(int* __restrict__ hist, const int* __restrict__ prompt, int n_prompt, const int* __restrict__ tok0,
                                                                    SpecOut* out, int stop, unsigned long long base, int draws, const StopBlock* rules = nullptr) {
    __shared__ unsigned lds[kStopLdsWords];
    for (int i = threadIdx.x; i < n_prompt; i += blockDim.x) hist[i] = prompt[i];
    const int id = tok0[0];
    bool fired = false;
    if (stop_armed(rules)) fired = stop_match(rules, id, [](int) { return -1; }, 0, lds).kind != 0;
    if (threadIdx.x == 0) {
        hist[n_prompt] = id; out->ids[0] = id; out->m = 0; out->n_emit = 1; out->stopped = id == stop || fired ? 1 : 0; out->pad = 0;
        out->rng = draws ? sample_step(base) : base;
    }
}

} // namespace flm
