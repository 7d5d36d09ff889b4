// flm_sample.h -- Sampler::sample (src/transformer/sampler.cpp:113-137 of the reference; restated in host/sampler.cpp) on the device: temperature, the clipped
// softmax (tf_operators.cpp:188-209), the xorshift* coin, multinomial / top-p selection, and the decode state's advance -- the sampled counterpart of k_argmax_advance.
// Part of flm_kernels.h; include that header.
//
// Exactness.  Every fp32 value is the reference's: x / T is an IEEE division, the max is order-free, exp is expf_ref (glibc), the softmax sum and both cumulative
// sums are SEQUENTIAL fp32 chains of non-negative terms in the reference's order.  A chain is evaluated by one wave with chain_spec_t<.., OP = 1, .., STARTS> (flm_gemv.h):
// exact, and with STARTS it also hands every lane the exact chain value in front of its run of B elements, so "the first i whose running sum passes a bound" is one
// more pass of B steps per lane (chain_first) instead of n dependent steps.  The clipped zeros are exact identities of the chain.
// Top-p orders its candidates (p >= (1 - topp) / (n - 1)) by probability, descending, ties by ascending index -- what glibc's merge-sort qsort leaves -- with a stable
// LSD radix sort over the inverted probability bits (one workgroup, 8-bit digits, ping-pong buffers in device memory: 32 000 candidates x 8 B do not fit LDS next to
// the strip); digits that are equal in every candidate are skipped.
// Coin == 0 (the CLI's seed 0 keeps the state at 0 for ever): multinomial returns the first index with p > 0, top-p the lowest index among the maximal probabilities;
// both still need the exact sum (p = e * (1 / sum) can tie where the logits differ), neither needs the sort or a cumulative chain.
// k_sample_rows is the same draw (sample_draw, the one function both kernels call) over the rows of a verify batch, row i with the (i + 1)-th coin of the step's state:
// what the sampled decode loop draws at its i-th token (flm_spec.h).
#pragma once
#include "flm_math.h"
#include "flm_gemv.h"
#include "flm_stop.h"
#pragma clang fp contract(off)

namespace flm {

// the per-call parameters in device memory (written at the start of each call; the token graphs read them): temperature, top-p, the sampler's xorshift state
struct SampleParams { float temperature; float topp; unsigned long long rng; };
constexpr int kSampleBlock = 1024;
constexpr int kSampleWaves = kSampleBlock / 64;
// LDS: the strip [64 lanes][B + 4] floats, then the radix sort's per-wave digit counts [16][256], digit bases [256], the four digit histograms [4][256], 64 words
constexpr int kSampleAuxWords = kSampleWaves * 256 + 256 + 4 * 256 + 64;
__host__ __device__ inline int sample_lane_elems(int n) { const int b = (n + 63) / 64; return (b + 3) & ~3; }
__host__ __device__ inline size_t sample_lds_bytes(int n) { return ((size_t)64 * (sample_lane_elems(n) + 4) + kSampleAuxWords) * 4; }

struct SampleArgs {
    const float* logits; int n;
    SampleParams* sp;                     // in: temperature, top-p, state; out: the state after the draw
    DecodeState* st; int* out_tokens; int out_cap; int advance;
    unsigned long long* sort_buf;         // [2][n]: the radix sort's ping-pong buffers
    const int* err;                       // the cross-workgroup waits' error word (gen_last_act; may be null)
    const StopBlock* stop;                // the stop rules' block (flm_stop.h; the shaped token forms pass it, every other launch null): looked at where DecodeState::stop_rules is set
};

// xorshift* (sampler.cpp random_u32 / random_f32): the coin of one draw
__host__ __device__ __forceinline__ unsigned long long sample_step(unsigned long long s) { s ^= s >> 12; s ^= s << 25; s ^= s >> 27; return s; }
__device__ __forceinline__ float sample_coin(unsigned long long& s) {
    s = sample_step(s);
    const unsigned r = (unsigned)((s * 0x2545F4914F6CDD1Dull) >> 32);
    return __fdiv_rn((float)(r >> 8), 16777216.0f);
}

// the first maximum of v(i), i < n (strict '>' in ascending order per thread, the lower index across threads): what k_argmax_advance computes; n_none when nothing beats -inf
template <class F>
__device__ __forceinline__ int block_first_max(F v, int n, int n_none, int* red) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    float best = -INFINITY; int idx = 0x7fffffff;
    for (int i = threadIdx.x; i < n; i += kSampleBlock) { const float x = v(i); if (x > best) { best = x; idx = i; } }
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(best, o, kWave); const int oi = __shfl_xor(idx, o, kWave);
        if (ov > best || (ov == best && oi < idx)) { best = ov; idx = oi; }
    }
    if (lane == 0) { red[2 * w] = __float_as_int(best); red[2 * w + 1] = idx; }
    __syncthreads();
    best = __int_as_float(red[0]); idx = red[1];
    for (int k = 1; k < kSampleWaves; ++k) { const float bv = __int_as_float(red[2 * k]); const int bi = red[2 * k + 1]; if (bv > best || (bv == best && bi < idx)) { best = bv; idx = bi; } }
    __syncthreads();
    return idx == 0x7fffffff ? n_none : idx;
}
// the smallest i < n with pred(i); n_none if there is none
template <class F>
__device__ __forceinline__ int block_first(F pred, int n, int n_none, int* red) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int idx = 0x7fffffff;
    for (int i = threadIdx.x; i < n; i += kSampleBlock) if (pred(i)) { idx = i; break; }
    for (int o = 32; o > 0; o >>= 1) idx = min(idx, __shfl_xor(idx, o, kWave));
    if (lane == 0) red[w] = idx;
    __syncthreads();
    idx = red[0];
    for (int k = 1; k < kSampleWaves; ++k) idx = min(idx, red[k]);
    __syncthreads();
    return idx == 0x7fffffff ? n_none : idx;
}
// one wave: given the lane's exact chain start ls (chain_spec_t<.., STARTS>), the first strip position whose running sum satisfies pred; -1 if none.  *val: that running sum
template <class P>
__device__ __forceinline__ int chain_first(const float* strip, int B, int LS, float ls, P pred, float* val) {
    const int lane = threadIdx.x & 63;
    const float4* r = reinterpret_cast<const float4*>(strip + lane * LS);
    float l = ls, hv = 0.f; int hit = -1;
    for (int q = 0; q < (B >> 2); ++q) {
        const float4 v = r[q];
        l = __fadd_rn(l, v.x); if (hit < 0 && pred(l)) { hit = 4 * q; hv = l; }
        l = __fadd_rn(l, v.y); if (hit < 0 && pred(l)) { hit = 4 * q + 1; hv = l; }
        l = __fadd_rn(l, v.z); if (hit < 0 && pred(l)) { hit = 4 * q + 2; hv = l; }
        l = __fadd_rn(l, v.w); if (hit < 0 && pred(l)) { hit = 4 * q + 3; hv = l; }
    }
    const unsigned long long m = __ballot(hit >= 0);
    if (!m) return -1;
    const int f = __ffsll((long long)m) - 1;
    *val = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(hv), f));
    return f * B + __builtin_amdgcn_readlane(hit, f);
}
// exclusive prefix of 256 counters, by one wave (4 per lane)
__device__ __forceinline__ void wave_excl_scan256(const int* in, int* out) {
    const int lane = threadIdx.x & 63;
    const int a0 = in[4 * lane], a1 = in[4 * lane + 1], a2 = in[4 * lane + 2], a3 = in[4 * lane + 3];
    const int s = a0 + a1 + a2 + a3;
    int incl = s;
    for (int o = 1; o < 64; o <<= 1) { const int u = __shfl_up(incl, o, kWave); if (lane >= o) incl += u; }
    const int e = incl - s;
    out[4 * lane] = e; out[4 * lane + 1] = e + a0; out[4 * lane + 2] = e + a0 + a1; out[4 * lane + 3] = e + a0 + a1 + a2;
}

// The stable LSD radix sort of sample_draw's candidates (and of flm_entropy.h's), by one 1024-thread workgroup, in two steps.  cand(i, key): index i < n is a candidate, and
// its 32-bit key; the order is ascending key, equal keys by ascending index.  hist: 4 * 256 words, misc: sample_draw's ([33] the count, [36..39] "digit d is the same in every
// candidate").
// sort_count: the candidates' digit histograms and their number (returned to every thread)
template <class CF>
__device__ __forceinline__ int sort_count(CF cand, const int n, int* const hist, int* const misc) {
    const int t = threadIdx.x, lane = t & 63;
    for (int k = t; k < 4 * 256; k += kSampleBlock) hist[k] = 0;
    if (t < 8) misc[32 + t] = 0;
    __syncthreads();
    int mine = 0;
    for (int i = t; i < n; i += kSampleBlock) {
        unsigned key;
        if (cand(i, key)) {
            ++mine;
#pragma unroll
            for (int d = 0; d < 4; ++d) atomicAdd(&hist[d * 256 + ((key >> (8 * d)) & 255u)], 1);
        }
    }
    for (int o = 32; o > 0; o >>= 1) mine += __shfl_xor(mine, o, kWave);
    if (lane == 0) atomicAdd(&misc[33], mine);
    __syncthreads();
    const int n0 = misc[33];
    for (int k = t; k < 4 * 256; k += kSampleBlock) if (n0 > 0 && hist[k] == n0) misc[36 + (k >> 8)] = 1;
    __syncthreads();
    return n0;
}
// sort_run (behind sort_count, n0 > 0): the passes, index order in -- ties keep ascending index.  The first pass reads the candidates through cand (and filters), the others
// a half of sort_buf [2][n].  Returns the sorted entries {key << 32 | index} [n0]: one of the halves
template <class CF>
__device__ __forceinline__ const unsigned long long* sort_run(CF cand, const int n, const int n0, unsigned long long* sort_buf, int* const cnt, int* const dbase, int* const hist, int* const misc) {
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    bool any = false;
#pragma unroll 1
    for (int d = 0; d < 4; ++d) any = any || !misc[36 + d];
    int src = -1;                                                 // -1: the strip; 0 / 1: sort_buf half
#pragma unroll 1
    for (int d = 0; d < 4; ++d) {
        if (misc[36 + d] && (any || d < 3 || src >= 0)) continue;          // (a digit equal in every candidate orders nothing; one pass runs in any case)
        if (w == 0) wave_excl_scan256(hist + d * 256, dbase);
        const int dstb = src < 0 ? 0 : src ^ 1;
        const unsigned long long* sb = sort_buf + (size_t)(src < 0 ? 0 : src) * n;
        unsigned long long* db = sort_buf + (size_t)dstb * n;
        const int N = src < 0 ? n : n0;
#pragma unroll 1
        for (int b0 = 0; b0 < N; b0 += kSampleBlock) {
            const int i = b0 + t;
            bool valid = i < N;
            unsigned long long e = 0ull;
            if (src < 0) {
                unsigned key = 0u;
                valid = valid && cand(i, key);
                e = ((unsigned long long)key << 32) | (unsigned)i;
            } else if (valid) e = sb[i];
            const unsigned dig = (unsigned)(e >> (32 + 8 * d)) & 255u;
            for (int k = t; k < kSampleWaves * 256; k += kSampleBlock) cnt[k] = 0;
            unsigned long long m = __ballot(valid);
#pragma unroll
            for (int bb = 0; bb < 8; ++bb) { const unsigned long long bm = __ballot((dig >> bb) & 1u); m &= ((dig >> bb) & 1u) ? bm : ~bm; }
            const int rank = __popcll(m & ((1ull << lane) - 1ull));
            __syncthreads();
            if (valid && rank == 0) cnt[w * 256 + dig] = __popcll(m);
            __syncthreads();
            if (t < 256) { int run = dbase[t]; for (int k = 0; k < kSampleWaves; ++k) { const int c = cnt[k * 256 + t]; cnt[k * 256 + t] = run; run += c; } dbase[t] = run; }
            __syncthreads();
            if (valid) db[cnt[w * 256 + dig] + rank] = e;
            __syncthreads();
        }
        src = dstb;
    }
    return sort_buf + (size_t)src * n;
}

// ONE draw of Sampler::sample by one workgroup of 1024 threads: the token for `logits[0 .. n)` at (temp, topp), n >= 2, with the coin drawn from `rng` (advanced by that one
// draw; untouched at temp == 0).  strip: sample_lds_bytes(n) of LDS; sort_buf: [2][n] of the workgroup's own.  Every thread returns the token.  Both sampler kernels are this
// function: k_sample_advance (the token path: one row, then the decode state's advance) and k_sample_rows (a verify batch: one workgroup per row).
__device__ __forceinline__ int sample_draw(const float* logits, int n, float temp, float topp, unsigned long long& rng, unsigned long long* sort_buf, float* strip) {
    const int B = sample_lane_elems(n), LS = B + 4;
    int* cnt = reinterpret_cast<int*>(strip + 64 * LS);
    int* dbase = cnt + kSampleWaves * 256;
    int* hist = dbase + 256;
    int* misc = hist + 4 * 256;            // [0..31] reductions, [32] result, [33] sum / n0, [36..39] "digit d is the same in every candidate"; [40..55] are k_sample_advance's (sample_misc)
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    auto spos = [&](int i) { const int L = i / B; return L * LS + (i - L * B); };       // element i's place in the strip
    int tok;
    if (temp == 0.0f) {
        // sample_argmax: first maximum wins, the state is not touched
        tok = block_first_max([&](int i) { return logits[i]; }, n, 0, misc);
    } else {
        // logits[q] /= temperature; the max of the divided values
        float mx = -INFINITY;
        for (int i = t; i < 64 * B; i += kSampleBlock) {
            float x = 0.f;
            if (i < n) { x = __fdiv_rn(logits[i], temp); mx = fmaxf(mx, x); }
            strip[spos(i)] = x;
        }
        mx = wave_max(mx);
        if (lane == 0) misc[w] = __float_as_int(mx);
        __syncthreads();
        mx = __int_as_float(misc[0]);
        for (int k = 1; k < kSampleWaves; ++k) mx = fmaxf(mx, __int_as_float(misc[k]));
        // the clipped exponentials (d < -15: 0), then sum = the sequential chain in index order (zero padding past n: identities)
        for (int i = t; i < n; i += kSampleBlock) { const int q = spos(i); const float d = __fsub_rn(strip[q], mx); strip[q] = d < -15.0f ? 0.0f : expf_ref(d); }
        __syncthreads();
        if (w == 0) { const float s = chain_spec_t<0, 1, 4>(strip, 0, nullptr, nullptr, B); if (lane == 0) misc[33] = __float_as_int(s); }
        __syncthreads();
        const float inv = (float)(1.0 / (double)__int_as_float(misc[33]));
        for (int i = t; i < n; i += kSampleBlock) { const int q = spos(i); strip[q] = __fmul_rn(strip[q], inv); }
        __syncthreads();
        const float coin = sample_coin(rng);
        if (topp <= 0.0f || topp >= 1.0f) {
            // multinomial: the first i with coin < cdf_i, n - 1 if none
            if (coin == 0.0f) tok = block_first([&](int i) { return strip[spos(i)] > 0.0f; }, n, n - 1, misc);
            else {
                if (w == 0) {
                    float ls, v;
                    (void)chain_spec_t<0, 1, 4, true>(strip, 0, nullptr, nullptr, B, &ls);
                    const int pos = chain_first(strip, B, LS, ls, [&](float cdf) { return coin < cdf; }, &v);
                    if (lane == 0) misc[32] = pos < 0 ? n - 1 : pos;
                }
                __syncthreads();
                tok = misc[32];
            }
        } else {
            const float cutoff = __fdiv_rn(__fsub_rn(1.0f, topp), (float)(n - 1));
            int n0 = 0;
            // the candidates and their keys: inverted probability bits -- ascending key = descending probability
            auto cand = [&](int i, unsigned& key) { const float p = strip[spos(i)]; key = ~__float_as_uint(p); return p >= cutoff; };
            if (coin != 0.0f) {
                n0 = sort_count(cand, n, hist, misc);
            }
            if (coin == 0.0f || n0 == 0) {
                // coin 0: r = 0 * cum = 0 < cdf at the first sorted element -- the lowest index among the maximal probabilities.  (n0 == 0, reachable only for
                // top-p below ~1 / n: the reference reads the element in front of its array; here: the same choice as coin 0.)
                tok = block_first_max([&](int i) { return strip[spos(i)]; }, n, 0, misc);
            } else {
                // stable LSD radix sort of the candidates, index order in: ties keep ascending index.  The first pass reads the strip (and filters), the others a buffer.
                const unsigned long long* sorted = sort_run(cand, n, n0, sort_buf, cnt, dbase, hist, misc);
                // the sorted probabilities as a strip of their own; cum = the chain up to the first element where cum > topp (last), r = coin * cum,
                // then the first element up to last with r < cdf -- the same chain again
                const int B2 = sample_lane_elems(n0), LS2 = B2 + 4;
                for (int i = t; i < 64 * B2; i += kSampleBlock) { const int L = i / B2; strip[L * LS2 + (i - L * B2)] = i < n0 ? __uint_as_float(~(unsigned)(sorted[i] >> 32)) : 0.0f; }
                __syncthreads();
                if (w == 0) {
                    float ls, cum;
                    const float total = chain_spec_t<0, 1, 4, true>(strip, 0, nullptr, nullptr, B2, &ls);
                    int last = chain_first(strip, B2, LS2, ls, [&](float c) { return c > topp; }, &cum);
                    if (last < 0) { last = n0 - 1; cum = total; }
                    const float r = __fmul_rn(coin, cum);
                    float v;
                    int pos = chain_first(strip, B2, LS2, ls, [&](float c) { return r < c; }, &v);
                    if (pos < 0 || pos > last) pos = last;
                    if (lane == 0) misc[32] = (int)(unsigned)(sorted[pos] & 0xffffffffull);
                }
                __syncthreads();
                tok = misc[32];
            }
        }
    }
    return tok;
}

// the 64 words at the end of sample_draw's LDS (its `misc`): sample_draw uses [0..39]; [40..55] hold the stop matcher's mismatch words (kStopLdsWords) in k_sample_advance,
// so the kernel's LDS does not grow and the sampler's vocabulary bound stays where it is
__device__ __forceinline__ unsigned* sample_misc(float* strip, int n) {
    return reinterpret_cast<unsigned*>(strip + 64 * (sample_lane_elems(n) + 4)) + kSampleWaves * 256 + 256 + 4 * 256;
}
static_assert(40 + kStopLdsWords <= 64, "the stop matcher's words fit behind sample_draw's");

// The tail of a sampled token, by the whole workgroup behind the draw of `tok` (k_sample_advance, and flm_entropy.h's k_entropy_advance): the stop rules, out_tokens[step],
// the token's last act, the decode state's advance, the sampler state's write-back.
// a.stop given, not empty, and the call one that honours rules in the token form (DecodeState::stop_rules, set by flm_generate_ex alone): the stop rules are
// matched against out_tokens[0 .. step) ++ tok by the whole workgroup (flm_stop.h) in front of the last act, which then halts as on the stop token.  The ids of THIS
// attempt lie in out_tokens from index 0 on (a retried attempt rewrites them before it reads them), and every read stays below out_cap.
__device__ __forceinline__ void sample_finish(const SampleArgs& a, const int tok, const unsigned long long rng, float* const strip) {
    bool fired = false;
    if (stop_armed(a.stop) && a.out_tokens != nullptr && a.st->stop_rules != 0) {       // (uniform: every thread takes the same branch)
        const int step = a.st->step;                                                   // (written behind the matcher's barrier only: by thread 0, below)
        const int* const ot = a.out_tokens; const int cap = a.out_cap;
        if (step >= 0 && step < cap)
            fired = stop_match(a.stop, tok, [&](int j) { return j < cap ? ot[j] : -1; }, step, sample_misc(strip, a.n) + 40).kind != 0;
    }
    if (threadIdx.x == 0) {
        DecodeState* st = a.st;
        if (a.out_tokens && st->step >= 0 && st->step < a.out_cap) a.out_tokens[st->step] = tok;
        const bool halt = gen_last_act(st, st->step, tok, a.err, fired);                        // (the token's last act: flm_math.h)
        if (a.advance && !halt) { st->tok = tok; st->pos += 1; }
        st->step += 1;
        a.sp->rng = rng;
    }
}
// One workgroup of 1024 threads, sample_lds_bytes(n) of dynamic LDS, n >= 2.  Writes out_tokens[step], advances the state like k_argmax_advance, and the sampler state
// (sample_finish).
inline __global__ void __launch_bounds__(kSampleBlock) k_sample_advance(const SampleArgs a) {
    extern __shared__ float4 sample_lds4[];
    if (halted(&a.st->halt)) return;       // (flm_math.h DecodeState::halt: the sampler state stays at the last drawn token's)
    unsigned long long rng = a.sp->rng;
    const int tok = sample_draw(a.logits, a.n, a.sp->temperature, a.sp->topp, rng, a.sort_buf, reinterpret_cast<float*>(sample_lds4));
    sample_finish(a, tok, rng, reinterpret_cast<float*>(sample_lds4));
}

// The same draw over the rows of a verify batch's classifier chunk: one workgroup per row, grid = the chunk's rows, sample_lds_bytes(n) of dynamic LDS.  Row r of the
// chunk (logits + r * ld) is batch row row0 + r: its coin is the (row0 + r + 1)-th draw from `base`, the state at the step's start -- every workgroup steps the state
// there itself (row0 + r < kSpecRows steps), so no row waits for another.  Row r sorts in its own [2][n] slice of sort_buf.  Writes out[row0 + r] and nothing else.
// temp == 0: the first maximum, no coin.
constexpr int kSpecRows = 16;
inline __global__ void __launch_bounds__(kSampleBlock) k_sample_rows(const float* __restrict__ logits, int ld, int n, int row0, float temp, float topp,
                                                                     unsigned long long base, unsigned long long* sort_buf, int* __restrict__ out) {
    extern __shared__ float4 sample_lds4[];
    const int r = blockIdx.x, row = row0 + r;
    unsigned long long rng = base;
    for (int i = 0; i < row && i < kSpecRows; ++i) rng = sample_step(rng);
    const int tok = sample_draw(logits + (size_t)r * ld, n, temp, topp, rng, sort_buf + (size_t)r * 2 * n, reinterpret_cast<float*>(sample_lds4));
    if (threadIdx.x == 0) out[row] = tok;
}

} // namespace flm
