// flm_score.h -- per-row statistics of a [rows][n] block of logits: what flm_score_tokens (and its op-level mirror flm_op_score_rows) reports for every position of a
// scored sequence.  Part of flm_kernels.h; include that header.
//
// A row's figures are sample_argmax (sampler.cpp:36-47: the first maximum) and the reference sampler's clipped softmax (tf_operators.cpp:188-209) at temperature 1, read
// at the row's target: d = x - max, e = d < -15 ? 0 : expf(d), sum = the SEQUENTIAL fp32 chain of the e in index order, prob = e_target * (float)(1.0 / sum).
// Exactness is flm_sample.h's: the max is order-free, exp is expf_ref (glibc's expf bit for bit), the sum is evaluated by ONE wave with chain_spec_t<0, OP = 1> over
// the lane-major strip (zero padding and clipped zeros are identities of a chain of non-negative terms).  Nothing of k_sample_advance is restated: the strip layout, the
// reductions and the chain are its device functions.
#pragma once
#include "flm_sample.h"
#pragma clang fp contract(off)

namespace flm {

// == flm_score (include/flm_gpu.h): the C ABI's struct, field for field
struct ScoreRow { int argmax; float target_logit, max_logit, sum, prob; };
struct ScoreArgs {
    const float* logits; int ld;          // row r = logits + r * ld
    int n;                                // entries per row (the vocabulary)
    const int* targets;                   // [rows]: the index whose term is read, -1 = none (target_logit = prob = 0)
    ScoreRow* out;                        // [rows]
};
// LDS: the strip [64 lanes][B + 4] floats, then 64 words (block_first_max's slots, the sum): inside sample_lds_bytes(n), the bound the device sampler has
__host__ __device__ inline size_t score_lds_bytes(int n) { return ((size_t)64 * (sample_lane_elems(n) + 4) + 64) * 4; }

// One workgroup of 1024 threads per row, score_lds_bytes(n) of dynamic LDS.
inline __global__ void __launch_bounds__(kSampleBlock) k_score_rows(const ScoreArgs a) {
    extern __shared__ float4 score_lds4[];
    float* strip = reinterpret_cast<float*>(score_lds4);
    const int n = a.n, B = sample_lane_elems(n), LS = B + 4;
    int* misc = reinterpret_cast<int*>(strip + 64 * LS);          // [0..31] reductions, [32] the sum
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const float* x = a.logits + (size_t)blockIdx.x * a.ld;
    auto spos = [&](int i) { const int L = i / B; return L * LS + (i - L * B); };       // element i's place in the strip
    // sample_argmax: the first maximum wins (index 0 where nothing beats -inf); the row's max is that element
    const int amax = block_first_max([&](int i) { return x[i]; }, n, 0, misc);
    const float mx = x[amax];
    // the clipped exponentials (d < -15: 0) into the strip, zero padding past n; then sum = the sequential chain in index order
    for (int i = t; i < 64 * B; i += kSampleBlock) {
        float e = 0.0f;
        if (i < n) { const float d = __fsub_rn(x[i], mx); e = d < -15.0f ? 0.0f : expf_ref(d); }
        strip[spos(i)] = e;
    }
    __syncthreads();
    if (w == 0) { const float s = chain_spec_t<0, 1, 4>(strip, 0, nullptr, nullptr, B); if (lane == 0) misc[32] = __float_as_int(s); }
    __syncthreads();
    if (t == 0) {
        const float sum = __int_as_float(misc[32]);
        const int tg = a.targets ? a.targets[blockIdx.x] : -1;
        ScoreRow r; r.argmax = amax; r.max_logit = mx; r.sum = sum; r.target_logit = 0.0f; r.prob = 0.0f;
        if (tg >= 0 && tg < n) {
            const float inv = (float)(1.0 / (double)sum);                              // multiply(x, 1. / sum, n): the reciprocal in double, rounded once
            r.target_logit = x[tg]; r.prob = __fmul_rn(strip[spos(tg)], inv);
        }
        a.out[blockIdx.x] = r;
    }
}

} // namespace flm
