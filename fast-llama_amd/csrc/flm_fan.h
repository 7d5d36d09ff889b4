// flm_fan.h -- parallel sampling (flm_generate_n: n completions of ONE prompt per pass over the weights; host side: flm_calls.hip, the batch pass: flm_prompt.hip
// prefill_batched with a FanDesc).  Part of flm_kernels.h; include that header.  Ordinary grid launches: nothing here waits for another workgroup.
//
// The cache stays one cache.  Its rows [0, S), S = pos + n_prompt, are the prompt's and belong to every sequence; sequence j's fed tokens live in physical rows
// base[j] + i (FanDesc; include/flm_gpu.h flm_fan_layout_for).  Token i of a tail is at LOGICAL position S + i -- for RoPE and for the attention's order -- whatever
// its physical row:  logical row r of sequence j  ->  physical row  r < S ? r : base[j] + (r - S).
// A step feeds the n sequences' last ids as one batch of n rows at tail index t (logical position S + t):
//   k_fan_load      the ids the host holds become the batch (a step's inputs are launch arguments: a re-run step enqueues the same work)
//   k_rope_kv_fan   k_rope_kv_rows with ONE RoPE position for all rows and a cache row per row
//   k_attn_fan      row j attends the shared prefix followed by its own tail, per query attn_head's arithmetic in the LOGICAL order
//   k_sample_fan    row j drawn by the unchanged sample_draw with ITS OWN state's next coin (temperature 0: the first maximum)
//   k_fan_accept    the step's result block: ids, the live mask behind the stop token, the states (moved for live rows only); the host reads it once per step
//   k_fan_keep      flm_fan_keep: tail j moved to rows [S, S + count) in every layer and head
#pragma once
#include "flm_attn.h"
#include "flm_sample.h"
#pragma clang fp contract(off)

namespace flm {

constexpr int kFanMax = 16;
// one step's geometry: S shared rows, the batch's tail index t, n rows; row j's K/V go to physical row base[j] + t
struct FanDesc { int S, t, n; int base[kFanMax]; };
// what the host holds between two steps, by value into the step's launches: every row's last id, its sampler state, the live mask
struct FanIn { int ids[kFanMax]; unsigned long long rng[kFanMax]; unsigned live; int pad; };
// what a step leaves for the host, read back in ONE trip: ids[j] (-1: the row was not live), the live mask behind this step's stop tokens, the states behind the step's draws
struct FanOut { int ids[kFanMax]; unsigned live; int pad; unsigned long long rng[kFanMax]; };

inline __global__ void k_fan_load(const FanIn in, int n, int* __restrict__ batch) {
    if (blockIdx.x == 0 && (int)threadIdx.x < n) batch[threadIdx.x] = in.ids[threadIdx.x];
}

// qkv [n][3 dim] (the plain-store GEMM) -> q rotated into qout [n][dim], k rotated and v into the layer's cache rows; every row at RoPE position pos = S + t
inline __global__ void k_rope_kv_fan(const float* qkv, float* qout, float* kcache, float* vcache, const float* rope_cos, const float* rope_sin,
                                     int dim, int hs, int max_seq, const FanDesc f) {
    const int b = blockIdx.x, pos = f.S + f.t, prow = f.base[b] + f.t;
    const float* in = qkv + (size_t)b * 3 * dim;
    for (int i = threadIdx.x; i < dim / 2; i += blockDim.x) {
        const int row = 2 * i, h = row / hs, d = row - h * hs;
        const float c = rope_cos[(size_t)pos * (hs / 2) + d / 2], s = rope_sin[(size_t)pos * (hs / 2) + d / 2];
        float o0, o1;
        rope_pair(in[row], in[row + 1], c, s, o0, o1);
        qout[(size_t)b * dim + row] = o0; qout[(size_t)b * dim + row + 1] = o1;
        rope_pair(in[dim + row], in[dim + row + 1], c, s, o0, o1);
        float* kp = kcache + ((size_t)h * max_seq + prow) * hs + d; kp[0] = o0; kp[1] = o1;
        float* vp = vcache + ((size_t)h * max_seq + prow) * hs + d; vp[0] = in[2 * dim + row]; vp[1] = in[2 * dim + row + 1];
    }
}

// ------------------------------------------------------------------------------------------
// The fan's attention, attn_prefill_mq's multi-query form (hs <= 128).  Workgroup (h, g) takes the G consecutive sequences i0 = g * G ... of head h (G = 8, 4, 2 or 1:
// what the LDS allows, fan_group).  All of them see T = S + t + 1 logical rows.  The tiles of 64 rows a workgroup walks, for K and again for V:
//   x < ntS                 the shared prefix, physical rows x * 64 ...: brought to LDS ONCE, used by all G queries
//   x = ntS + jt * ntL + u  query jt's own tail, physical rows base[i0 + jt] + u * 64 ...: used by that query alone
// Every query's arithmetic is attn_head's, operation for operation, as attn_prefill_mq restates it: a score is 8 strided accumulators added 0..7, * attn_scale; the
// scores of a query lie in LDS in the LOGICAL order (prefix, then tail), so max, expf_ref, the softmax sum (ONE chain, t ascending over that order) and the division are
// the code of attn_prefill_mq; the weighted sum is one chain per (query, dimension) over the prefix tiles and then the query's tail tiles -- row 0 (always a prefix
// row: S >= 1) by multiplication, every later row by FMA, |w| <= 1e-15 skipped.  Nothing is reduced per segment and combined.
// ------------------------------------------------------------------------------------------
__host__ __device__ inline size_t fan_lds_bytes(int G, int max_seq, int hs) {
    return (size_t)(G * hs + G * (((max_seq + 3) & ~3) + 8) + 2 * kAttnTile * attn_row_stride(hs)) * 4;
}
// queries per workgroup: kMqQueries where attn_mq_lds_bytes fits (fan_lds_bytes(8, ..) is that figure), else halved down to one
__host__ inline int fan_group(int max_seq, int hs, size_t lds_max) {
    int G = kMqQueries;
    while (G > 1 && fan_lds_bytes(G, max_seq, hs) > lds_max) G >>= 1;
    return G;
}
template <int NF>
__device__ __forceinline__ void attn_fan(const AttnArgs& a, const FanDesc& f, const int h, char* lds, const int i0, const int nq, const int G, const int row_stride) {
    typedef float v4f __attribute__((ext_vector_type(4)));
    constexpr int rs = NF * 64 + 8;
    const int hs = a.hs, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int scs = ((a.max_seq + 3) & ~3) + 8;                                 // stride of a query's score row
    float* qs = reinterpret_cast<float*>(lds);                                  // [G][hs]
    float* sc = qs + G * hs;                                                    // [G][scs]
    float* tile0 = sc + G * scs;
    float* tile1 = tile0 + kAttnTile * rs;
    const int S = f.S, L = f.t + 1, T = S + L;                                  // prefix rows, tail rows (the batch's own included), rows every query sees
    const int ntS = (S + kAttnTile - 1) / kAttnTile, ntL = (L + kAttnTile - 1) / kAttnTile, nt = ntS + nq * ntL;
    const float* K = a.kcache + (size_t)h * (a.kv_rows ? a.kv_rows : a.max_seq) * hs;
    const float* V = a.vcache + (size_t)h * (a.kv_rows ? a.kv_rows : a.max_seq) * hs;
    const __amdgpu_buffer_rsrc_t rK = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(K), 0, a.max_seq * hs * 4, 0x00020000);
    const __amdgpu_buffer_rsrc_t rV = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(V), 0, a.max_seq * hs * 4, 0x00020000);
    const float scale = (float)(1.0 / (double)__builtin_sqrtf((float)hs));      // attn_scale, transformer.cpp:418
    // tile x: its first physical row, how many rows, the logical index of its first row, whose it is (-1: every query's)
    struct Tile { int row0, rows, t0, owner; };
    auto tile_of = [&](int x) {
        Tile t;
        if (x < ntS) { t.row0 = x * kAttnTile; t.rows = S - t.row0; t.t0 = t.row0; t.owner = -1; }
        else {
            const int y = x - ntS, jt = y / ntL, u = y - jt * ntL;
            t.row0 = f.base[i0 + jt] + u * kAttnTile; t.rows = L - u * kAttnTile; t.t0 = S + u * kAttnTile; t.owner = jt;
        }
        t.rows = t.rows > kAttnTile ? kAttnTile : t.rows;
        return t;
    };
    // this thread's pieces of a tile (as in attn_head)
    const int f4r = hs >> 2, tile_f4 = kAttnTile * f4r;
    int prow[NF], goff[NF], loff[NF];
#pragma unroll
    for (int j = 0; j < NF; ++j) {
        const int e = tid + j * kAttnBlock, row = e / f4r, c4 = e - row * f4r;
        prow[j] = e < tile_f4 ? row : (1 << 28);
        goff[j] = (row * hs + c4 * 4) * 4;
        loff[j] = row * rs + c4 * 4;
    }
    auto request = [&](const __amdgpu_buffer_rsrc_t& r, int x, v4f (&reg)[NF]) {     // rows past the tile's last (and tiles past the last) read as zero
        Tile t{0, 0, 0, -1};
        if (x < nt) t = tile_of(x);
#pragma unroll
        for (int j = 0; j < NF; ++j) {
            const unsigned off = prow[j] < t.rows ? (unsigned)(t.row0 * hs * 4 + goff[j]) : 0x80000000u;
            reg[j] = __builtin_bit_cast(v4f, __builtin_amdgcn_raw_buffer_load_b128(r, (int)off, 0, 0));
        }
    };
    auto park = [&](float* buf, const v4f (&reg)[NF]) {
#pragma unroll
        for (int j = 0; j < NF; ++j)
            if (prow[j] < kAttnTile) *reinterpret_cast<float4*>(buf + loff[j]) = make_float4(reg[j].x, reg[j].y, reg[j].z, reg[j].w);
    };
    v4f ring[NF];
    request(rK, 0, ring);
    for (int e = tid; e < G * hs; e += kAttnBlock) {
        const int j = e / hs, d = e - j * hs;
        qs[e] = j < nq ? a.q[(size_t)(i0 + j) * row_stride + (size_t)h * hs + d] : 0.f;
    }
    // ---- scores.  thread = (query half, position p, accumulator k); its 4 queries share the K operand of every step (a tail tile: only its owner keeps the result)
    {
        const int k = tid & 7, p = (tid >> 3) & 63, jh = (tid >> 9) * 4;
        auto qrow = [&](int j) { return qs + (j < G ? j : G - 1) * hs + k; };    // (queries past the group: any row of qs, the result is dropped)
        const float* q0 = qrow(jh + 0); const float* q1 = qrow(jh + 1); const float* q2 = qrow(jh + 2); const float* q3 = qrow(jh + 3);
        for (int x = 0; x < nt; ++x) {
            float* cur = (x & 1) ? tile1 : tile0;
            const Tile tl = tile_of(x);
            park(cur, ring);
            __syncthreads();                                                    // (also orders qs before its first use)
            request(rK, x + 1, ring);
            const float* kp = cur + p * rs + k;
            float l0 = 0.f, l1 = 0.f, l2 = 0.f, l3 = 0.f;
#pragma unroll 8
            for (int i = 0; i < hs; i += 8) {
                const float kv = kp[i];
                l0 = __fmaf_rn(kv, q0[i], l0); l1 = __fmaf_rn(kv, q1[i], l1); l2 = __fmaf_rn(kv, q2[i], l2); l3 = __fmaf_rn(kv, q3[i], l3);
            }
            auto fold = [&](float l, int j) {                                   // the 8 partials added 0..7 (lane k = 0 collects them)
                const int li = __float_as_int(l);
                float tot = __fadd_rn(0.f, l);
                tot = __fadd_rn(tot, __int_as_float(__builtin_amdgcn_update_dpp(0, li, 0x101 /* row_shl:1 */, 0xF, 0xF, true)));
                tot = __fadd_rn(tot, __int_as_float(__builtin_amdgcn_update_dpp(0, li, 0x102, 0xF, 0xF, true)));
                tot = __fadd_rn(tot, __int_as_float(__builtin_amdgcn_update_dpp(0, li, 0x103, 0xF, 0xF, true)));
                tot = __fadd_rn(tot, __int_as_float(__builtin_amdgcn_update_dpp(0, li, 0x104, 0xF, 0xF, true)));
                tot = __fadd_rn(tot, __int_as_float(__builtin_amdgcn_update_dpp(0, li, 0x105, 0xF, 0xF, true)));
                tot = __fadd_rn(tot, __int_as_float(__builtin_amdgcn_update_dpp(0, li, 0x106, 0xF, 0xF, true)));
                tot = __fadd_rn(tot, __int_as_float(__builtin_amdgcn_update_dpp(0, li, 0x107, 0xF, 0xF, true)));
                if (k == 0 && j < nq && p < tl.rows && (tl.owner < 0 || tl.owner == j)) sc[j * scs + tl.t0 + p] = __fmul_rn(tot, scale);   // att.multiply(attn_scale) :443
            };
            fold(l0, jh + 0); fold(l1, jh + 1); fold(l2, jh + 2); fold(l3, jh + 3);
        }
    }
    request(rV, 0, ring);                                                       // the first V tile travels under the softmax
    __syncthreads();
    // ---- softmax: wave j = query j over its T scores in the logical order (max is order-free; the sum is the reference's sequential one, tf_operators.cpp:180-183)
    if (wave < nq) {
        float* row = sc + wave * scs;
        float m = -INFINITY;
        for (int t = lane; t < T; t += 64) m = fmaxf(m, row[t]);
        m = wave_max(m);
        for (int t = lane; t < T; t += 64) row[t] = expf_ref(__fsub_rn(row[t], m));
        float sum = 0.f;
        if (lane == 0) {                                                        // T dependent adds; the LDS reads run 16 elements ahead
            int t = 0;
            if (T >= 16) {
                const float4* r4 = reinterpret_cast<const float4*>(row);
                float4 a0 = r4[0], a1 = r4[1], a2 = r4[2], a3 = r4[3];
#define FLM_ADD4(q) sum = __fadd_rn(sum, q.x); sum = __fadd_rn(sum, q.y); sum = __fadd_rn(sum, q.z); sum = __fadd_rn(sum, q.w);
                for (; t + 32 <= T; t += 16) {
                    const float4 b0 = r4[t / 4 + 4], b1 = r4[t / 4 + 5], b2 = r4[t / 4 + 6], b3 = r4[t / 4 + 7];
                    FLM_ADD4(a0) FLM_ADD4(a1) FLM_ADD4(a2) FLM_ADD4(a3)
                    a0 = b0; a1 = b1; a2 = b2; a3 = b3;
                }
                FLM_ADD4(a0) FLM_ADD4(a1) FLM_ADD4(a2) FLM_ADD4(a3)
#undef FLM_ADD4
                t += 16;
            }
            for (; t < T; ++t) sum = __fadd_rn(sum, row[t]);
        }
        sum = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(sum)));
        // att[t] = exp / sum; rows t >= 1 with |att| <= 1e-15 are skipped by the weighted sum (transformer.cpp:449): stored as exact zeros
        for (int t = lane; t < T; t += 64) { const float w = __fdiv_rn(row[t], sum); row[t] = (t > 0 && fabsf(w) <= 1e-15f) ? 0.f : w; }
    }
    // ---- o[j][d] = sum_t att_j[t] V[t][d]: one thread per (query, output dimension), t ascending in the logical order: the shared tiles, then the query's own
    const int tpq = hs <= 64 ? 64 : 128;                                        // threads per query (a multiple of the wave: the skip test stays wave-uniform)
    const int j = tid / tpq, d = tid - j * tpq;
    const bool mine = j < nq && d < hs;
    float o = 0.f;
    for (int x = 0; x < nt; ++x) {
        float* cur = (x & 1) ? tile1 : tile0;
        const Tile tl = tile_of(x);
        park(cur, ring);
        __syncthreads();                                                        // (the first one also orders the softmax's writes before the reads below)
        request(rV, x + 1, ring);
        if (mine && (tl.owner < 0 || tl.owner == j)) {
            const float* vp = cur + d;
            const float* wp = sc + j * scs + tl.t0;
            const int np = tl.rows;
            int p = 0;
            if (x == 0) { o = __fmul_rn(vp[0], wp[0]); p = 1; }                 // logical row 0 always (tf_operators.cpp:331-336)
            // the weights are wave-uniform (a wave's lanes belong to ONE query): if no row of the tile is skipped the walk is 8 reads ahead of 8 dependent FMAs
            const float wl = lane < np ? wp[lane] : 1.f;
            if (__all(wl != 0.f)) {
                for (; p < np && (p & 7); ++p) o = __fmaf_rn(vp[p * rs], wp[p], o);
                for (; p + 8 <= np; p += 8) {
                    const float* vq = vp + p * rs; const float* wq = wp + p;    // (a tail's weights start at S: no 16-byte alignment to read them by)
                    const float w0 = wq[0], w1 = wq[1], w2 = wq[2], w3 = wq[3], w4 = wq[4], w5 = wq[5], w6 = wq[6], w7 = wq[7];
                    const float a0 = vq[0], a1 = vq[rs], a2 = vq[2 * rs], a3 = vq[3 * rs], a4 = vq[4 * rs], a5 = vq[5 * rs], a6 = vq[6 * rs], a7 = vq[7 * rs];
                    o = __fmaf_rn(a0, w0, o); o = __fmaf_rn(a1, w1, o); o = __fmaf_rn(a2, w2, o); o = __fmaf_rn(a3, w3, o);
                    o = __fmaf_rn(a4, w4, o); o = __fmaf_rn(a5, w5, o); o = __fmaf_rn(a6, w6, o); o = __fmaf_rn(a7, w7, o);
                }
                for (; p < np; ++p) o = __fmaf_rn(vp[p * rs], wp[p], o);
            } else {
                for (; p < np; ++p) { const float w = wp[p]; o = w == 0.f ? o : __fmaf_rn(vp[p * rs], w, o); }
            }
        }
    }
    if (mine) a.out[(size_t)(i0 + j) * row_stride + (size_t)h * hs + d] = o;
}
// grid (heads, ceil(n / G)), kAttnBlock threads, fan_lds_bytes(G, a.max_seq, a.hs) of dynamic LDS; a.q / a.out [n][row_stride]
inline __global__ void __launch_bounds__(kAttnBlock) k_attn_fan(const AttnArgs a, const FanDesc f, int row_stride, int G) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    const int i0 = blockIdx.y * G, nq = f.n - i0 < G ? f.n - i0 : G;
    if (a.hs <= 64) attn_fan<1>(a, f, blockIdx.x, lds, i0, nq, G, row_stride); else attn_fan<2>(a, f, blockIdx.x, lds, i0, nq, G, row_stride);
}

// One workgroup of 1024 threads per row of a classifier chunk: chunk row r (logits + r * ld; ld == 0: every row draws from the ONE row the prompt left) is batch row
// row0 + r, drawn by sample_draw with that row's OWN state in.rng[row0 + r] -- its next coin --, in its own [2][n] slice of sort_buf.  temp == 0: the first maximum (no
// strip: any vocabulary), the state passes through.  Writes drawn[row0 + r] and after[row0 + r], nothing else.
inline __global__ void __launch_bounds__(kSampleBlock) k_sample_fan(const float* __restrict__ logits, int ld, int n, int row0, float temp, float topp, const FanIn in,
                                                                    unsigned long long* sort_buf, int* __restrict__ drawn, unsigned long long* __restrict__ after) {
    extern __shared__ float4 sample_lds4[];       // temp != 0: sample_lds_bytes(n); temp == 0: the first maximum's 2 * kSampleWaves words (no static LDS: the strip may take the CU's whole)
    const int r = blockIdx.x, row = row0 + r;
    const float* x = logits + (size_t)r * ld;
    unsigned long long rng = in.rng[row];
    int tok;
    if (temp == 0.0f) tok = block_first_max([&](int i) { return x[i]; }, n, 0, reinterpret_cast<int*>(sample_lds4));
    else tok = sample_draw(x, n, temp, topp, rng, sort_buf + (size_t)row * 2 * n, reinterpret_cast<float*>(sample_lds4));
    if (threadIdx.x == 0) { drawn[row] = tok; after[row] = rng; }
}

// The accept step (one wave, lane j = row j): a live row delivers its id, moves its state to the one behind the draw and leaves the live set at the stop token; a row
// that finished earlier delivers nothing and keeps the state behind its last delivered draw.  Everything it reads besides the two arrays the draw kernel wrote is a
// launch argument, and it writes the result block alone: a step that is re-run stores the same words again.
inline __global__ void k_fan_accept(FanOut* out, const int* __restrict__ drawn, const unsigned long long* __restrict__ after, const FanIn in, int n, int stop) {
    const int j = threadIdx.x;
    if (blockIdx.x != 0 || j >= 64) return;
    const bool live = j < n && ((in.live >> j) & 1u);
    const int id = live ? drawn[j] : -1;
    const unsigned long long keep = __ballot(live && id != stop);
    if (j < kFanMax) { out->ids[j] = id; out->rng[j] = live ? after[j] : in.rng[j < n ? j : 0]; }
    if (j == 0) { out->live = (unsigned)keep; out->pad = 0; }
}

// flm_fan_keep: rows [src, src + count) -> [dst, dst + count) of every layer's and head's K and V (dst + count <= src: the ranges never overlap).  blockIdx.x = layer * heads
// + head (the caches are [layers][heads][kv_rows][hs]); 16-byte pieces
inline __global__ void k_fan_keep(float* kcache, float* vcache, int kv_rows, int hs, int src, int dst, int count) {
    const size_t head = (size_t)blockIdx.x * kv_rows * hs;
    const int n4 = count * hs / 4;
    const float4* ks = reinterpret_cast<const float4*>(kcache + head + (size_t)src * hs); float4* kd = reinterpret_cast<float4*>(kcache + head + (size_t)dst * hs);
    const float4* vs = reinterpret_cast<const float4*>(vcache + head + (size_t)src * hs); float4* vd = reinterpret_cast<float4*>(vcache + head + (size_t)dst * hs);
    for (int i = threadIdx.x; i < n4; i += blockDim.x) { kd[i] = ks[i]; vd[i] = vs[i]; }
}

} // namespace flm
