// flm_logprob.h -- the record of one drawn token (include/flm_gpu.h flm_logprob): the drawn id and its logit, the clipped softmax's max and exact
// sequential sum at temperature 1 (flm_score.h's fields), and the first n_top indices of the row in "larger value, equal values by lower index, -0.0 ties +0.0" -- step 3's
// order of flm_shape.h -- with their logits.  No logarithm is taken here: the caller evaluates (logit - max_logit) - log(sum) in double from these bit-exact ingredients.
// One device function, logprob_row, run by one 1024-thread workgroup; k_logprob_token (behind the shaped token form's sampler, while the context is armed) and
// k_logprob_rows (one workgroup per row of a verify batch, behind the rows' draws) wrap it -- the shape_row / sample_draw pattern.  The host restatement is
// host/sampler.cpp logprob_row, which this equals element for element.
//   statistics   flm_sample.h / flm_score.h's device functions: block_first_max, expf_ref, the lane-major strip, chain_spec_t<0, 1, 4> on one wave -- nothing is restated
//   top-N        radix_select (flm_shape.h) over shape_key leaves the threshold key and `need`; the entries above the threshold take their slots by an integer LDS counter
//                (at most 19 of them), the `need` lowest threshold-equal indices by an index-ordered count (ballot + per-wave bases, as step 3 admits them); one wave then
//                ranks the at most 20 winners by (key descending, index ascending) -- a total order, so the slots' arrival order changes nothing.  -inf entries take part
// The row stays in global memory (L2-resident right behind the classifier: a handful of passes over 4 * n bytes).  LDS: the strip and kLogprobAux words, inside
// sample_lds_bytes(n) -- the device sampler's bound -- and fixed at capture time: sized for FLM_LOGPROBS_MAX, never for the armed top_n.
// Part of flm_kernels.h; include that header.
#pragma once
#include "flm_sample.h"
#include "flm_shape.h"
#pragma clang fp contract(off)

namespace flm {

constexpr int kLogprobsMax = 20;           // == FLM_LOGPROBS_MAX
// == flm_logprob (include/flm_gpu.h): the C ABI's struct, field for field, 192 bytes
struct LogprobRec { int token; float logit, max_logit, sum; int n_top; int top_id[kLogprobsMax]; float top_logit[kLogprobsMax]; int pad_[3]; };
constexpr int kLogprobWords = (int)(sizeof(LogprobRec) / 4);
static_assert(sizeof(LogprobRec) == 192 && kLogprobWords == 48, "flm_logprob is 192 bytes");
// LDS behind the strip: [0..63] block_first_max's slots and the sum, [64 ..) radix_select's four histograms, its 64 words, the winners {32 keys, 32 indices}, the record's
// words and the slot counter
constexpr int kLogprobAux = 64 + 4 * 256 + 64 + 64 + 64;
static_assert(kLogprobAux <= kSampleAuxWords, "inside the sampler's LDS bound");
__host__ __device__ inline size_t logprob_lds_bytes(int n) { return ((size_t)64 * (sample_lane_elems(n) + 4) + kLogprobAux) * 4; }

// The context's device block (allocated at flm_ctx_create; flm_logprobs_arm and every armed call's start rewrite its contents, so the token graphs captured at flm_prepare
// with its ADDRESS follow a setting that changes later).  top_n < 0: disarmed, the stage returns at its top.  base: the record index of the call's token at step 0 (a
// single-token step of flm_generate_lookup_ex: the ids delivered so far)
struct LogprobBlock { int top_n; int source; int base; int pad_; };

// THE definition on one row R[0 .. n), n >= 2, drawn id `chosen`, top_n in [0, kLogprobsMax], by one 1024-thread workgroup: *out <- the record.  strip: logprob_lds_bytes(n)
__device__ __forceinline__ void logprob_row(const float* R, const int n, const int chosen, const int top_n, float* strip, LogprobRec* out) {
    const int B = sample_lane_elems(n), LS = B + 4;
    int* const red = reinterpret_cast<int*>(strip + 64 * LS);     // [0..31] reductions, [32] the sum
    int* const hist = red + 64;
    int* const sel = hist + 4 * 256;                              // radix_select's words; [0..15] the per-wave counts of the index-ordered pass
    int* const wkey = sel + 64; int* const widx = wkey + 32;      // the winners, at most kLogprobsMax
    int* const recw = widx + 32;                                  // [0..47] the record, [48] the slot counter
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    auto spos = [&](int i) { const int L = i / B; return L * LS + (i - L * B); };       // element i's place in the strip
    // flm_score.h's statistics: the first maximum, the clipped exponentials into the strip (zero padding past n), the sequential chain on wave 0
    const int amax = block_first_max([&](int i) { return R[i]; }, n, 0, red);
    const float mx = R[amax];
    for (int i = t; i < 64 * B; i += kSampleBlock) {
        float e = 0.0f;
        if (i < n) { const float d = __fsub_rn(R[i], mx); e = d < -15.0f ? 0.0f : expf_ref(d); }
        strip[spos(i)] = e;
    }
    if (t <= kLogprobWords) recw[t] = 0;                          // the record's words (entries at and beyond n_top stay 0) and the counter
    __syncthreads();
    if (wv == 0) { const float s = chain_spec_t<0, 1, 4>(strip, 0, nullptr, nullptr, B); if (lane == 0) red[32] = __float_as_int(s); }
    const int K = min(min(max(top_n, 0), kLogprobsMax), n);
    if (K > 0) {
        int need, eqc;
        const unsigned T = radix_select([&](int i) { return shape_key(R[i]); }, n, K, hist, sel, &need, &eqc);
        const int ngt = K - need;                                 // entries above the threshold
        const bool all_eq = need >= eqc;                          // no tie at the cut: every threshold-equal entry is a winner
        for (int i = t; i < n; i += kSampleBlock) {
            const unsigned key = shape_key(R[i]);
            if (key > T || (all_eq && key == T)) { const int slot = atomicAdd(&recw[kLogprobWords], 1); if (slot < kLogprobsMax) { wkey[slot] = (int)key; widx[slot] = i; } }
        }
        if (!all_eq) {
            int base = 0;                  // threshold-equal entries in front of this block of 1024 indices (the same value in every thread)
#pragma unroll 1
            for (int b0 = 0; b0 < n && base < need; b0 += kSampleBlock) {
                const int i = b0 + t;
                const bool eq = i < n && shape_key(R[i]) == T;
                const unsigned long long m = __ballot(eq);
                if (lane == 0) sel[wv] = __popcll(m);
                __syncthreads();
                int before = base, all = 0;
                for (int k = 0; k < kSampleWaves; ++k) { const int c = sel[k]; before += k < wv ? c : 0; all += c; }
                const int rank = before + __popcll(m & ((1ull << lane) - 1ull));
                if (eq && rank < need && ngt + rank < kLogprobsMax) { wkey[ngt + rank] = (int)T; widx[ngt + rank] = i; }
                base += all;
                __syncthreads();
            }
        }
        __syncthreads();
        if (wv == 0 && lane < K) {         // one wave orders the winners: (key descending, index ascending)
            const unsigned kj = (unsigned)wkey[lane]; const int ij = widx[lane];
            int rank = 0;
            for (int m = 0; m < K; ++m) { const unsigned km = (unsigned)wkey[m]; const int im = widx[m]; rank += (km > kj || (km == kj && im < ij)) ? 1 : 0; }
            if (rank < kLogprobsMax && (unsigned)ij < (unsigned)n) { recw[5 + rank] = ij; recw[5 + kLogprobsMax + rank] = __float_as_int(R[ij]); }
        }
    }
    __syncthreads();
    if (t == 0) {
        recw[0] = chosen;
        recw[1] = (unsigned)chosen < (unsigned)n ? __float_as_int(R[chosen]) : 0;
        recw[2] = __float_as_int(mx); recw[3] = red[32]; recw[4] = K;
    }
    __syncthreads();
    if (t < kLogprobWords) reinterpret_cast<int*>(out)[t] = recw[t];
}

// The token form's stage, behind k_sample_advance / k_argmax_advance of the shaped form: the record of the token that launch drew, out_tokens[step - 1], into
// rec[base + step - 1], from the classifier's row (source 0) or the shaped row the sampler read (source 1) -- both are still alive here.
// The stop-token hazard: a stop token's own sampler sets the latch, yet that token is delivered and needs its record, while the launches queued behind it must write
// nothing -- and a halted launch does not move `step`, so both see the SAME state.  What tells them apart is tags[]: a record's word holds the tag (DecodeState::gen_tag,
// one per attempt of a flm_generate_ex call) of the attempt that wrote it.  A launch that finds the latch set AND its record already carrying the attempt's tag returns:
// the stage is idempotent.  The latch is read at the top only (halted()) and never written here: flm_math.h's invariant stands
struct LogprobArgs {
    const float* raw; const float* shaped; int n;
    const LogprobBlock* blk;
    const DecodeState* st; const int* out_tokens; int out_cap;
    LogprobRec* rec; unsigned* tags; int rec_cap;
};
inline __global__ void __launch_bounds__(kSampleBlock) k_logprob_token(const LogprobArgs a) {
    extern __shared__ float4 logprob_lds4[];
    const int top_n = a.blk->top_n;
    if (top_n < 0) return;
    const bool h = halted(&a.st->halt);
    const int s = a.st->step - 1, idx = a.blk->base + s;
    if (s < 0 || s >= a.out_cap || idx < 0 || idx >= a.rec_cap) return;
    const unsigned tag = a.st->gen_tag;
    if (h && a.tags[idx] == tag) return;                          // (uniform: the word is written by the last statement of an earlier launch only)
    logprob_row(a.blk->source ? a.shaped : a.raw, a.n, a.out_tokens[s], top_n, reinterpret_cast<float*>(logprob_lds4), a.rec + idx);
    if (threadIdx.x == 0) a.tags[idx] = tag;
}

// One workgroup per row of a verify batch's classifier chunk, grid = the chunk's rows: block r is batch row row0 + r (k_sample_rows' convention), its drawn id
// chosen[row0 + r], its record rec[rec_base + row0 + r] -- rec_base: the ids the call has delivered so far, a launch argument (the host knows it before it enqueues the step).
// The rows behind the accept step's cut are overwritten by the next step
struct LogprobRowsArgs { const float* rows; int ld; int n; int row0; const int* chosen; int top_n; LogprobRec* rec; int rec_base; int rec_cap; };
inline __global__ void __launch_bounds__(kSampleBlock) k_logprob_rows(const LogprobRowsArgs a) {
    extern __shared__ float4 logprob_lds4[];
    const int r = blockIdx.x, row = a.row0 + r, idx = a.rec_base + row;
    if (idx < 0 || idx >= a.rec_cap) return;
    logprob_row(a.rows + (size_t)r * a.ld, a.n, a.chosen[row], a.top_n, reinterpret_cast<float*>(logprob_lds4), a.rec + idx);
}

} // namespace flm
