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
// flm_generate_lookup's start: the history = the prompt and the id drawn from its last logits (tok0[0], the decode state's first output slot); the whole result block of
// that one id (the state after its one draw)
inline __global__ void k_spec_begin(int* __restrict__ hist, const int* __restrict__ prompt, int n_prompt, const int* __restrict__ tok0, SpecOut* out, int stop,
                                    unsigned long long base, int draws) {
    for (int i = threadIdx.x; i < n_prompt; i += blockDim.x) hist[i] = prompt[i];
    if (threadIdx.x == 0) {
        const int id = tok0[0];
        hist[n_prompt] = id; out->ids[0] = id; out->m = 0; out->n_emit = 1; out->stopped = id == stop ? 1 : 0; out->pad = 0;
        out->rng = draws ? sample_step(base) : base;
    }
}

} // namespace flm
