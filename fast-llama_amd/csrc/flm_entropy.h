// flm_entropy.h -- the entropy-driven samplers behind the shaping stage: stage 5, locally typical sampling, and stage 6, Mirostat v2 (include/flm_gpu.h flm_entropy;
// DESIGN.md section 5j; restated sequentially in host/sampler.cpp entropy_logits / mirostat_update, which these kernels equal bit for bit).  No reference counterpart.
// One 1024-thread workgroup masks, IN PLACE, the row R the sampler is about to read; the UNCHANGED sampler (flm_sample.h sample_draw) then draws from it.
// The definition, all arithmetic fp32 round-to-nearest without contraction:
//   statistics  y = R / T, mx = max y, d = y - mx, e = d < -15 ? 0 : expf_ref(d) (the sampler's clip), sum = the sequential chain of e in index order (one wave,
//               chain_spec_t<0, 1, 4>: exact), p = e * (float)(1.0 / sum), ls = flm_logf(sum) (flm_logf.h, evaluated by one lane), surprise a = ls - d.  e == 0: DEAD -- never a
//               candidate, left untouched.  d is recomputed from R wherever it is needed (a division and a subtraction: the same bits) instead of being kept: the strip is the
//               only LDS there is (sample_lds_bytes(n), the sampler's layout and vocabulary bound)
//   5 typical   H = the sequential chain of h = p * a (dead: 0): the strip again, the same wave; key = fabsf(a - H) -- non-negative, so its bits order as the values do; the
//               live entries through the sampler's stable radix sort (sort_count / sort_run: ascending key, equal keys by ascending index; [2][n] ping-pong buffer in device
//               memory, free here: the sampler runs behind this stage on the same stream); the strip rebuilt from the sorted order's p (recomputed: expf_ref is a function of d);
//               the cut = the first position whose running sum passes typical_p (chain_spec_t<.., STARTS> + chain_first); -inf scattered through the sorted index list behind it
//   6 mirostat  one pass: a live entry stays iff a * 1.44269504f <= mu, the first maximum always; the e of what goes is cleared in the strip, so a second chain gives sum', the
//               sum of the masked row, and ls' = flm_logf(sum') -- with mx what the update behind the draw needs: obs = (ls' - d[t]) * 1.44269504f, mu = mu - eta * (obs - tau)
// Lone-wave costs (MI355X_MICROARCH.md: a lone wave issues one instruction per ~8 clocks): each chain is a dozen passes of B = n / 64 dependent adds per lane (the
// approximate sums, the head, the two increment chains, the rounds); typical runs three chains (sum, H, the cut) and up to four sort passes, Mirostat two chains and no
// sort.  Measured per token: DESIGN.md section 5j.
// Part of flm_kernels.h; include that header.
#pragma once
#include "flm_math.h"
#include "flm_logf.h"
#include "flm_sample.h"
#pragma clang fp contract(off)

namespace flm {

// the setting's device block (allocated at flm_ctx_create; written at the start of every attempt from the host's copy, so a retried attempt updates nothing twice; the
// entropy token graphs hold its address).  mu: Mirostat's running state, moved by k_entropy_advance with every id it draws
struct EntropyBlock { float typical_p; int mirostat; float tau, eta; float mu; int pad_[3]; };
constexpr float kLog2e = 1.44269504f;
__host__ __device__ inline bool typical_on(float p) { return p > 0.0f && p < 1.0f; }

// what the stage hands to the update behind the draw (every thread): mx, and ls' = flm_logf(sum of the masked row) (Mirostat only)
struct EntropyStats { float mx; float ls_kept; };

// Stages 5 / 6 on ONE row by one 1024-thread workgroup, in place: S[0 .. n), n >= 2, temp != 0, exactly one of typical_on(typical_p) / mirostat == 2.
// strip: sample_lds_bytes(n) of LDS; sort_buf: [2][n] of the workgroup's own.  THE definition: k_entropy_advance (the token form) and k_entropy_rows (a verify batch) are both
// this function
__device__ __forceinline__ EntropyStats entropy_row(float* S, const int n, const float temp, const float typical_p, const int mirostat, const float mu,
                                                    unsigned long long* sort_buf, float* strip) {
    const int B = sample_lane_elems(n), LS = B + 4;
    int* cnt = reinterpret_cast<int*>(strip + 64 * LS);
    int* dbase = cnt + kSampleWaves * 256;
    int* hist = dbase + 256;
    int* misc = hist + 4 * 256;            // sample_draw's words, free until it runs: [0..31] reductions, [32] result, [33] the sort's count, [34] sum, [35] ls / H, [36..39] the sort's
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    auto spos = [&](int i) { const int L = i / B; return L * LS + (i - L * B); };
    // y and its maximum, then the clipped exponentials and their exact sum: sample_draw's first steps
    float mx = -INFINITY;
    for (int i = t; i < 64 * B; i += kSampleBlock) {
        float x = 0.f;
        if (i < n) { x = __fdiv_rn(S[i], temp); mx = fmaxf(mx, x); }
        strip[spos(i)] = x;
    }
    mx = wave_max(mx);
    if (lane == 0) misc[w] = __float_as_int(mx);
    __syncthreads();
    mx = __int_as_float(misc[0]);
    for (int k = 1; k < kSampleWaves; ++k) mx = fmaxf(mx, __int_as_float(misc[k]));
    for (int i = t; i < n; i += kSampleBlock) { const int q = spos(i); const float d = __fsub_rn(strip[q], mx); strip[q] = d < -15.0f ? 0.0f : expf_ref(d); }
    __syncthreads();
    if (w == 0) {
        const float s = chain_spec_t<0, 1, 4>(strip, 0, nullptr, nullptr, B);
        if (lane == 0) { misc[34] = __float_as_int(s); misc[35] = __float_as_int(flm_logf(s)); }
    }
    __syncthreads();
    const float sum = __int_as_float(misc[34]), ls = __int_as_float(misc[35]);
    auto dof = [&](int i) { return __fsub_rn(__fdiv_rn(S[i], temp), mx); };       // d[i], the bits of the pass above
    EntropyStats out{mx, ls};
    if (mirostat == 2) {
        // 6: the threshold filter; the first maximum (the lowest i with d == 0) always stays
        const int first = block_first([&](int i) { return dof(i) == 0.0f; }, n, 0, misc);
        for (int i = t; i < n; i += kSampleBlock) {
            const int q = spos(i);
            if (strip[q] == 0.0f || i == first) continue;
            const float a = __fsub_rn(ls, dof(i));
            if (!(__fmul_rn(a, kLog2e) <= mu)) { S[i] = -INFINITY; strip[q] = 0.0f; }
        }
        __syncthreads();
        if (w == 0) {
            const float s2 = chain_spec_t<0, 1, 4>(strip, 0, nullptr, nullptr, B);
            if (lane == 0) misc[35] = __float_as_int(flm_logf(s2));
        }
        __syncthreads();
        out.ls_kept = __int_as_float(misc[35]);
        __syncthreads();                   // (misc is sample_draw's from here on)
        return out;
    }
    // 5: h = p * a into the strip (dead entries and the padding: 0, identities of the chain), H = its sequential sum
    const float inv = (float)(1.0 / (double)sum);
    for (int i = t; i < n; i += kSampleBlock) {
        const int q = spos(i);
        const float e = strip[q];
        strip[q] = e == 0.0f ? 0.0f : __fmul_rn(__fmul_rn(e, inv), __fsub_rn(ls, dof(i)));
    }
    __syncthreads();
    if (w == 0) {
        const float h = chain_spec_t<0, 1, 4>(strip, 0, nullptr, nullptr, B);
        if (lane == 0) misc[35] = __float_as_int(h);
    }
    __syncthreads();
    const float H = __int_as_float(misc[35]);
    __syncthreads();                       // (every thread has H: sort_count clears the words around it)
    // the live entries ordered by key = |a - H| ascending, ties by ascending index.  live <=> !(d < -15): expf_ref is positive there
    auto cand = [&](int i, unsigned& key) {
        const float d = dof(i);
        key = __float_as_uint(fabsf(__fsub_rn(__fsub_rn(ls, d), H)));
        return !(d < -15.0f);
    };
    const int n0 = sort_count(cand, n, hist, misc);
    if (n0 > 0) {                          // (always: the maximum is live)
        const unsigned long long* sorted = sort_run(cand, n, n0, sort_buf, cnt, dbase, hist, misc);
        // the sorted order's p as a strip of its own, the cut, the scatter
        const int B2 = sample_lane_elems(n0), LS2 = B2 + 4;
        for (int j = t; j < 64 * B2; j += kSampleBlock) {
            float p = 0.0f;
            if (j < n0) { const int i = (int)(unsigned)(sorted[j] & 0xffffffffull); p = __fmul_rn(expf_ref(dof(i)), inv); }
            const int L = j / B2;
            strip[L * LS2 + (j - L * B2)] = p;
        }
        __syncthreads();
        if (w == 0) {
            float lst, c;
            (void)chain_spec_t<0, 1, 4, true>(strip, 0, nullptr, nullptr, B2, &lst);
            const int last = chain_first(strip, B2, LS2, lst, [&](float cum) { return cum > typical_p; }, &c);
            if (lane == 0) misc[32] = last < 0 ? n0 - 1 : last;
        }
        __syncthreads();
        const int last = misc[32];
        for (int j = last + 1 + t; j < n0; j += kSampleBlock) S[(int)(unsigned)(sorted[j] & 0xffffffffull)] = -INFINITY;
    }
    __syncthreads();                       // (misc and the strip are sample_draw's from here on; S's stores are seen by the workgroup behind this barrier)
    return out;
}

// Mirostat's update behind the draw of id tok from the masked row (one thread): obs, then mu - eta * (obs - tau) in three operations
__device__ __forceinline__ float mirostat_step(const float* S, const float temp, const int tok, const EntropyStats st, const float tau, const float eta, const float mu, float* obs_out) {
    const float d = __fsub_rn(__fdiv_rn(S[tok], temp), st.mx);
    const float obs = __fmul_rn(__fsub_rn(st.ls_kept, d), kLog2e);
    if (obs_out) *obs_out = obs;
    return __fsub_rn(mu, __fmul_rn(eta, __fsub_rn(obs, tau)));
}

// The entropy token form's last launch: the stage on the row the shaper left (a.logits: masked in place), the UNCHANGED draw, mu's update, the token's tail (sample_finish:
// what k_sample_advance runs) -- one launch, so mu is "the state after exactly the delivered ids' updates", the halting id included, without a second pass over a row that the
// next token overwrites.  A halted launch touches nothing.  One workgroup of 1024 threads, sample_lds_bytes(n) of dynamic LDS (k_sample_advance's), n >= 2.
// Temperature 0: both stages are neutral, the draw is the first maximum, mu does not move.  Mirostat: the draw is multinomial (topp = 1.0f), the block's topp is ignored
struct EntropyArgs { SampleArgs s; EntropyBlock* e; };
inline __global__ void __launch_bounds__(kSampleBlock) k_entropy_advance(const EntropyArgs a) {
    extern __shared__ float4 sample_lds4[];
    if (halted(&a.s.st->halt)) return;
    float* const strip = reinterpret_cast<float*>(sample_lds4);
    float* const row = const_cast<float*>(a.s.logits);
    const float temp = a.s.sp->temperature;
    const float tp = a.e->typical_p; const int miro = a.e->mirostat; const float mu = a.e->mu;
    const bool on = temp != 0.0f && (miro == 2 || typical_on(tp));
    EntropyStats es{0.0f, 0.0f};
    if (on) es = entropy_row(row, a.s.n, temp, tp, miro, mu, a.s.sort_buf, strip);
    unsigned long long rng = a.s.sp->rng;
    const int tok = sample_draw(row, a.s.n, temp, on && miro == 2 ? 1.0f : a.s.sp->topp, rng, a.s.sort_buf, strip);
    if (on && miro == 2 && threadIdx.x == 0) a.e->mu = mirostat_step(row, temp, tok, es, a.e->tau, a.e->eta, mu, nullptr);
    sample_finish(a.s, tok, rng, strip);
}

// The stage over the rows of a verify batch's classifier chunk, in place, between k_shape_rows and k_sample_rows: one workgroup per row, grid = the chunk's rows (<= 16),
// sample_lds_bytes(n) of dynamic LDS; row r sorts in its own [2][n] slice of sort_buf (k_sample_rows' convention).  mu (Mirostat; flm_op_entropy_rows only -- the verify
// entry points refuse Mirostat): [rows], row r's state.  chosen given: obs_out[r] / mu_out[r] = the update behind the draw of chosen[r] from the masked row
struct EntropyRowsArgs {
    float* rows; int ld; int n;
    float temp; float typical_p; int mirostat; float tau, eta;
    const float* mu;
    unsigned long long* sort_buf;
    const int* chosen; float* obs_out; float* mu_out;
};
inline __global__ void __launch_bounds__(kSampleBlock) k_entropy_rows(const EntropyRowsArgs a) {
    extern __shared__ float4 sample_lds4[];
    const int r = blockIdx.x;
    if (a.temp == 0.0f || !(a.mirostat == 2 || typical_on(a.typical_p))) return;
    float* const row = a.rows + (size_t)r * a.ld;
    const float mu = a.mirostat == 2 && a.mu ? a.mu[r] : 0.0f;
    const EntropyStats es = entropy_row(row, a.n, a.temp, a.typical_p, a.mirostat, mu, a.sort_buf + (size_t)r * 2 * a.n, reinterpret_cast<float*>(sample_lds4));
    if (a.mirostat == 2 && a.chosen && threadIdx.x == 0) {
        float obs;
        const float m2 = mirostat_step(row, a.temp, a.chosen[r], es, a.tau, a.eta, mu, &obs);
        if (a.obs_out) a.obs_out[r] = obs;
        if (a.mu_out) a.mu_out[r] = m2;
    }
}

// flm_logf over an array (flm_op_logf)
inline __global__ void k_op_logf(float* x, size_t n) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) x[i] = flm_logf(x[i]);
}

} // namespace flm
