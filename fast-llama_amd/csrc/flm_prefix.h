// flm_prefix.h -- cache slots behind a SHARED PREFIX (flm_batch_open_prefix; host side: flm_calls.hip, the batch pass: flm_prompt.hip prefill_batched with a PrefixDesc).
// Part of flm_kernels.h; include that header.  Ordinary grid launches: nothing here waits for another workgroup.
//
// The cache rows [0, S) hold a conversation that every slot continues.  It is in the cache ONCE; the slots lie behind it.  A sequence in the slot that starts at physical
// row base keeps LOGICAL position p -- for RoPE and for the attention's order -- in physical row  p < S ? p : base + (p - S).  RoPE and the cache rows need no kernel of their
// own: k_rope_kv_slots / k_rope_kv_segs place a row at base + pos, and the host hands them base - S.  The attention does:
//   k_attn_slots_prefix    workgroup (h, g) takes G consecutive STEP rows -- different sequences at different positions -- walks the prefix tiles once for all of them and
//                          then every row's own tiles: attn_fan's walk with a tail length and an origin PER ROW
//   k_attn_segs_prefix_mq  workgroup (h, g) finds its prompt segment and its group of G consecutive queries of that ONE sequence: they share the prefix tiles and the
//                          tiles of the sequence's own rows under attn_prefill_mq's causal bound
// Both are one walk (attn_prefix) over a list of tiles, each with a range of the cache it may read, a logical offset and the SET of queries it belongs to; the two kernels
// differ in the list alone (PfxSlotsGeo, PfxSegsGeo).  Every query's arithmetic is attn_head's, operation for operation, as attn_prefill_mq and attn_fan restate it: a score is
// 8 strided accumulators added 0..7, * attn_scale; a query's scores lie in LDS in the LOGICAL order, so max, expf_ref, the softmax sum (ONE chain, ascending over that order)
// and the division are attn_prefill_mq's; the weighted sum is one chain per (query, dimension) over the prefix tiles and then the query's own -- logical row 0 (always a prefix
// row: S >= 1) by multiplication, every later row by FMA, |w| <= 1e-15 skipped.  Nothing is reduced per range and combined.
#pragma once
#include "flm_segs.h"
#pragma clang fp contract(off)

namespace flm {

// the prefix beside a pass's SlotDesc / SegDesc: S shared rows; tmax = the longest logical length in the launch (S + the largest rows[] among its rows: a query's score row
// is sized by it); G = queries per workgroup (prefix_group).  The host states S; the launchers fill in the other two
struct PrefixDesc { int S, tmax, G; };

// LDS: G queries, G score rows of tmax logical rows, two tiles -- fan_lds_bytes' figure with the score rows sized by the pass, not by the cache
__host__ __device__ inline size_t prefix_lds_bytes(int G, int tmax, int hs) { return fan_lds_bytes(G, tmax, hs); }
// queries per workgroup, for both kernels: kMqQueries where that fits the LDS, else halved down to one (fan_group's rule).  Long own tails make every extra query of a
// step group cost its own tiles' score passes: this is the first dial to revisit, and the one place it is written
__host__ inline int prefix_group(int tmax, int hs, size_t lds_max) { return fan_group(tmax, hs, lds_max); }

// one tile of a walk: the range of the cache it lies in -- origin `org` (a physical row) and `bound` rows: the buffer resource the loads go through ends there --, its first row
// inside that range, how many rows (<= kAttnTile), the LOGICAL index of its first row, and the queries of the group it belongs to (bit j: query j)
struct PfxTile { int org, bound, row0, rows, t0; unsigned owners; };

// this thread's 16-byte pieces of a tile (as in attn_head): the tile row each lies in (1 << 28: none), its byte offset behind the tile's first row, its LDS offset
template <int NF> struct PfxLanes { int prow[NF], goff[NF], loff[NF]; };
template <int NF>
__device__ __forceinline__ void pfx_lanes(PfxLanes<NF>& l, const int hs, const int tid) {
    constexpr int rs = NF * 64 + 8;
    const int f4r = hs >> 2, tile_f4 = kAttnTile * f4r;
#pragma unroll
    for (int j = 0; j < NF; ++j) {
        const int e = tid + j * kAttnBlock, row = e / f4r, c4 = e - row * f4r;
        l.prow[j] = e < tile_f4 ? row : (1 << 28);
        l.goff[j] = (row * hs + c4 * 4) * 4;
        l.loff[j] = row * rs + c4 * 4;
    }
}
typedef float pfx_v4f __attribute__((ext_vector_type(4)));
// a tile's rows on their way to registers, through a resource that covers the tile's RANGE and nothing else: rows past the tile's last (and an empty tile) read as zero
template <int NF>
__device__ __forceinline__ void pfx_request(const float* head, const int hs, const PfxTile& t, const PfxLanes<NF>& l, pfx_v4f (&reg)[NF]) {
    const __amdgpu_buffer_rsrc_t r = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(head + (size_t)t.org * hs), 0, t.bound * hs * 4, 0x00020000);
#pragma unroll
    for (int j = 0; j < NF; ++j) {
        const unsigned off = l.prow[j] < t.rows ? (unsigned)(t.row0 * hs * 4 + l.goff[j]) : 0x80000000u;
        reg[j] = __builtin_bit_cast(pfx_v4f, __builtin_amdgcn_raw_buffer_load_b128(r, (int)off, 0, 0));
    }
}
template <int NF>
__device__ __forceinline__ void pfx_park(float* buf, const PfxLanes<NF>& l, const pfx_v4f (&reg)[NF]) {
#pragma unroll
    for (int j = 0; j < NF; ++j)
        if (l.prow[j] < kAttnTile) *reinterpret_cast<float4*>(buf + l.loff[j]) = make_float4(reg[j].x, reg[j].y, reg[j].z, reg[j].w);
}
// the 8 partials of a score added 0..7 (lane k = 0 of every 8 collects them)
__device__ __forceinline__ float pfx_fold(const float l) {
    const int li = __float_as_int(l);
    float tot = __fadd_rn(0.f, l);
    tot = __fadd_rn(tot, __int_as_float(__builtin_amdgcn_update_dpp(0, li, 0x101 /* row_shl:1 */, 0xF, 0xF, true)));
    tot = __fadd_rn(tot, __int_as_float(__builtin_amdgcn_update_dpp(0, li, 0x102, 0xF, 0xF, true)));
    tot = __fadd_rn(tot, __int_as_float(__builtin_amdgcn_update_dpp(0, li, 0x103, 0xF, 0xF, true)));
    tot = __fadd_rn(tot, __int_as_float(__builtin_amdgcn_update_dpp(0, li, 0x104, 0xF, 0xF, true)));
    tot = __fadd_rn(tot, __int_as_float(__builtin_amdgcn_update_dpp(0, li, 0x105, 0xF, 0xF, true)));
    tot = __fadd_rn(tot, __int_as_float(__builtin_amdgcn_update_dpp(0, li, 0x106, 0xF, 0xF, true)));
    tot = __fadd_rn(tot, __int_as_float(__builtin_amdgcn_update_dpp(0, li, 0x107, 0xF, 0xF, true)));
    return tot;
}
// one wave = one query over its T scores in the logical order: max (order-free), expf_ref, the reference's sequential sum (tf_operators.cpp:180-183), the division; rows
// t >= 1 with |att| <= 1e-15 are skipped by the weighted sum (transformer.cpp:449): stored as exact zeros
__device__ __forceinline__ void pfx_softmax_wave(float* row, const int T, const int lane) {
    float m = -INFINITY;
    for (int t = lane; t < T; t += 64) m = fmaxf(m, row[t]);
    m = wave_max(m);
    for (int t = lane; t < T; t += 64) row[t] = expf_ref(__fsub_rn(row[t], m));
    float sum = 0.f;
    if (lane == 0) {                                                            // T dependent adds; the LDS reads run 16 elements ahead
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
    for (int t = lane; t < T; t += 64) { const float w = __fdiv_rn(row[t], sum); row[t] = (t > 0 && fabsf(w) <= 1e-15f) ? 0.f : w; }
}
// one (query, dimension) chain over the np rows of a parked tile: vp = the tile's column, wp = the query's weights from the tile's logical offset; `first`: the tile holds
// logical row 0, which enters by multiplication (tf_operators.cpp:331-336).  The weights are wave-uniform (a wave's lanes belong to ONE query): if no row of the tile is
// skipped the walk is 8 reads ahead of 8 dependent FMAs
template <int NF>
__device__ __forceinline__ float pfx_weighted(float o, const float* vp, const float* wp, const int np, const bool first, const int lane) {
    constexpr int rs = NF * 64 + 8;
    int p = 0;
    if (first) { o = __fmul_rn(vp[0], wp[0]); p = 1; }
    const float wl = lane < np ? wp[lane] : 1.f;
    if (__all(wl != 0.f)) {
        for (; p < np && (p & 7); ++p) o = __fmaf_rn(vp[p * rs], wp[p], o);
        for (; p + 8 <= np; p += 8) {
            const float* vq = vp + p * rs; const float* wq = wp + p;            // (an own range's weights start at S: no 16-byte alignment to read them by)
            const float w0 = wq[0], w1 = wq[1], w2 = wq[2], w3 = wq[3], w4 = wq[4], w5 = wq[5], w6 = wq[6], w7 = wq[7];
            const float a0 = vq[0], a1 = vq[rs], a2 = vq[2 * rs], a3 = vq[3 * rs], a4 = vq[4 * rs], a5 = vq[5 * rs], a6 = vq[6 * rs], a7 = vq[7 * rs];
            o = __fmaf_rn(a0, w0, o); o = __fmaf_rn(a1, w1, o); o = __fmaf_rn(a2, w2, o); o = __fmaf_rn(a3, w3, o);
            o = __fmaf_rn(a4, w4, o); o = __fmaf_rn(a5, w5, o); o = __fmaf_rn(a6, w6, o); o = __fmaf_rn(a7, w7, o);
        }
        for (; p < np; ++p) o = __fmaf_rn(vp[p * rs], wp[p], o);
    } else {
        for (; p < np; ++p) { const float w = wp[p]; o = w == 0.f ? o : __fmaf_rn(vp[p * rs], w, o); }
    }
    return o;
}

// ------------------------------------------------------------------------------------------
// The two tile lists.  A Geo answers: nt() tiles; tile(x), x < nt(); len(j) = the logical rows query j sees; qrow(j) = its batch row.  Everything is read from the launch
// arguments with workgroup-uniform indices: nothing is copied, nothing lives in scratch.  Tiles [0, ntS) are the prefix's (origin row 0, bound S, every query's).
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ PfxTile pfx_prefix_tile(const int S, const int x) {
    PfxTile t; t.org = 0; t.bound = S; t.row0 = x * kAttnTile; t.rows = S - t.row0; t.rows = t.rows > kAttnTile ? kAttnTile : t.rows; t.t0 = t.row0; t.owners = ~0u;
    return t;
}
// step rows i0 .. i0 + nq of a pass: query j is row i0 + j at logical position pos[i0 + j], with own(j) = pos - S + 1 rows of its own from physical row base[i0 + j].  The own
// tiles follow the prefix's query by query, each query's ceil(own / 64) of them and no more: a short tail has no entry in the list, so it costs the walk nothing
struct PfxSlotsGeo {
    const SlotDesc& f; const int S, i0, nq;
    __device__ __forceinline__ int len(const int j) const { return f.pos[i0 + (j < nq ? j : nq - 1)] + 1; }     // (queries past the group: any row's, the result is dropped)
    __device__ __forceinline__ int own_tiles(const int j) const { return (f.pos[i0 + j] - S + kAttnTile) / kAttnTile; }
    __device__ __forceinline__ int qrow(const int j) const { return i0 + j; }
    __device__ __forceinline__ int nt() const { int n = (S + kAttnTile - 1) / kAttnTile; for (int j = 0; j < nq; ++j) n += own_tiles(j); return n; }
    __device__ __forceinline__ PfxTile tile(const int x) const {
        const int ntS = (S + kAttnTile - 1) / kAttnTile;
        if (x < ntS) return pfx_prefix_tile(S, x);
        int u = x - ntS, j = 0;
        for (; j < nq - 1; ++j) { const int n = own_tiles(j); if (u < n) break; u -= n; }
        const int r = i0 + j;
        PfxTile t; t.org = f.base[r]; t.bound = f.rows[r]; t.row0 = u * kAttnTile; t.rows = f.pos[r] - S + 1 - t.row0; t.rows = t.rows > kAttnTile ? kAttnTile : t.rows;
        t.t0 = S + t.row0; t.owners = 1u << j;
        return t;
    }
};
// queries i0 .. i0 + nq of prompt segment s: ONE sequence, so the own tiles are every query's too; query j sees pos0[s] + i0 + j + 1 logical rows (pos0 counts the prefix),
// attn_prefill_mq's causal bound over the two ranges
struct PfxSegsGeo {
    const SegDesc& f; const int S, s, i0, nq;
    __device__ __forceinline__ int len(const int j) const { return f.pos0[s] + i0 + (j < nq ? j : nq - 1) + 1; }
    __device__ __forceinline__ int qrow(const int j) const { return f.row0[s] + i0 + j; }
    __device__ __forceinline__ int own() const { return f.pos0[s] - S + i0 + nq; }                              // own rows the group's last query sees
    __device__ __forceinline__ int nt() const { return (S + kAttnTile - 1) / kAttnTile + (own() + kAttnTile - 1) / kAttnTile; }
    __device__ __forceinline__ PfxTile tile(const int x) const {
        const int ntS = (S + kAttnTile - 1) / kAttnTile;
        if (x < ntS) return pfx_prefix_tile(S, x);
        PfxTile t; t.org = f.base[s]; t.bound = f.rows[s]; t.row0 = (x - ntS) * kAttnTile; t.rows = own() - t.row0; t.rows = t.rows > kAttnTile ? kAttnTile : t.rows;
        t.t0 = S + t.row0; t.owners = ~0u;
        return t;
    }
};

// ------------------------------------------------------------------------------------------
// The walk.  G queries of head h: their q rows to LDS; the tiles' K through the two-buffer request / park pipeline (the next tile's loads travel under this tile's FMAs),
// scores into the owners' score rows at the tile's LOGICAL offset, each query up to its own length; the first V tile travels under the softmax (wave j = query j); then the
// tiles' V the same way, one thread per (query, dimension), a tile entering the chains of its owners alone.
// LDS: qs [G][hs], sc [G][scs], two tiles (prefix_lds_bytes(G, tmax, hs)).
// ------------------------------------------------------------------------------------------
template <int NF, class Geo>
__device__ __forceinline__ void attn_prefix(const AttnArgs& a, const Geo& geo, const int h, char* lds, const int G, const int nq, const int tmax, const int row_stride) {
    constexpr int rs = NF * 64 + 8;
    const int hs = a.hs, tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int scs = ((tmax + 3) & ~3) + 8;                                      // stride of a query's score row
    float* qs = reinterpret_cast<float*>(lds);                                  // [G][hs]
    float* sc = qs + G * hs;                                                    // [G][scs]
    float* tile0 = sc + G * scs;
    float* tile1 = tile0 + kAttnTile * rs;
    const size_t head = (size_t)h * (a.kv_rows ? a.kv_rows : a.max_seq) * hs;
    const float* K = a.kcache + head;
    const float* V = a.vcache + head;
    const float scale = (float)(1.0 / (double)__builtin_sqrtf((float)hs));      // attn_scale, transformer.cpp:418
    const int nt = geo.nt();
    const PfxTile none{0, 0, 0, 0, 0, 0u};
    PfxLanes<NF> ln; pfx_lanes<NF>(ln, hs, tid);
    pfx_v4f ring[NF];
    PfxTile cur = geo.tile(0);
    pfx_request<NF>(K, hs, cur, ln, ring);
    for (int e = tid; e < G * hs; e += kAttnBlock) {
        const int j = e / hs, d = e - j * hs;
        qs[e] = j < nq ? a.q[(size_t)geo.qrow(j) * row_stride + (size_t)h * hs + d] : 0.f;
    }
    // ---- scores.  thread = (query half, position p, accumulator k); its 4 queries share the K operand of every step (an own tile: only its owners keep the result)
    {
        const int k = tid & 7, p = (tid >> 3) & 63, jh = __builtin_amdgcn_readfirstlane(tid >> 9) * 4;
        auto qrow = [&](int j) { return qs + (j < G ? j : G - 1) * hs + k; };    // (queries past the group: any row of qs, the result is dropped)
        const float* q0 = qrow(jh + 0); const float* q1 = qrow(jh + 1); const float* q2 = qrow(jh + 2); const float* q3 = qrow(jh + 3);
        const int T0 = geo.len(jh + 0), T1 = geo.len(jh + 1), T2 = geo.len(jh + 2), T3 = geo.len(jh + 3);
        for (int x = 0; x < nt; ++x) {
            float* buf = (x & 1) ? tile1 : tile0;
            pfx_park<NF>(buf, ln, ring);
            __syncthreads();                                                    // (also orders qs before its first use)
            const PfxTile nxt = x + 1 < nt ? geo.tile(x + 1) : none;
            pfx_request<NF>(K, hs, nxt, ln, ring);
            const float* kp = buf + p * rs + k;
            float l0 = 0.f, l1 = 0.f, l2 = 0.f, l3 = 0.f;
#pragma unroll 8
            for (int i = 0; i < hs; i += 8) {
                const float kv = kp[i];
                l0 = __fmaf_rn(kv, q0[i], l0); l1 = __fmaf_rn(kv, q1[i], l1); l2 = __fmaf_rn(kv, q2[i], l2); l3 = __fmaf_rn(kv, q3[i], l3);
            }
            auto keep = [&](float l, int j, int Tj) {
                const float tot = pfx_fold(l);
                if (k == 0 && j < nq && ((cur.owners >> j) & 1u) && p < cur.rows && cur.t0 + p < Tj) sc[j * scs + cur.t0 + p] = __fmul_rn(tot, scale);   // att.multiply(attn_scale) :443
            };
            keep(l0, jh + 0, T0); keep(l1, jh + 1, T1); keep(l2, jh + 2, T2); keep(l3, jh + 3, T3);
            cur = nxt;
        }
    }
    cur = geo.tile(0);
    pfx_request<NF>(V, hs, cur, ln, ring);                                      // the first V tile travels under the softmax
    __syncthreads();
    if (wave < nq) pfx_softmax_wave(sc + wave * scs, geo.len(wave), lane);
    // ---- o[j][d] = sum_t att_j[t] V[t][d]: one thread per (query, output dimension), t ascending in the logical order: the prefix tiles, then the query's own
    const int tpq = hs <= 64 ? 64 : 128;                                        // threads per query (a multiple of the wave: the skip test stays wave-uniform)
    const int j = __builtin_amdgcn_readfirstlane(tid / tpq), d = tid - j * tpq;
    const bool mine = j < nq && d < hs;
    const int Tj = geo.len(j);
    float o = 0.f;
    for (int x = 0; x < nt; ++x) {
        float* buf = (x & 1) ? tile1 : tile0;
        pfx_park<NF>(buf, ln, ring);
        __syncthreads();                                                        // (the first one also orders the softmax's writes before the reads below)
        const PfxTile nxt = x + 1 < nt ? geo.tile(x + 1) : none;
        pfx_request<NF>(V, hs, nxt, ln, ring);
        if (mine && ((cur.owners >> j) & 1u)) {
            int np = Tj - cur.t0; np = np < 0 ? 0 : (np > cur.rows ? cur.rows : np);
            if (np > 0) o = pfx_weighted<NF>(o, buf + d, sc + j * scs + cur.t0, np, x == 0, lane);
        }
        cur = nxt;
    }
    if (mine) a.out[(size_t)geo.qrow(j) * row_stride + (size_t)h * hs + d] = o;
}

// grid (heads, ceil(f.n / px.G)), kAttnBlock threads, prefix_lds_bytes(px.G, px.tmax, a.hs) of dynamic LDS; a.q / a.out [f.n][row_stride]; f.base: the slots' PHYSICAL origins,
// f.pos: the rows' logical positions (>= px.S)
inline __global__ void __launch_bounds__(kAttnBlock) k_attn_slots_prefix(const AttnArgs a, const SlotDesc f, const PrefixDesc px, int row_stride) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    const int i0 = blockIdx.y * px.G, left = f.n - i0, nq = left < px.G ? left : px.G;
    if (nq < 1) return;                                                             // (uniform)
    const PfxSlotsGeo geo{f, px.S, i0, nq};
    if (a.hs <= 64) attn_prefix<1>(a, geo, blockIdx.x, lds, px.G, nq, px.tmax, row_stride); else attn_prefix<2>(a, geo, blockIdx.x, lds, px.G, nq, px.tmax, row_stride);
}
// grid (heads, sum over the prompt segments of ceil(n[s] / px.G)), kAttnBlock threads, prefix_lds_bytes(px.G, px.tmax, a.hs); a.q / a.out: the WHOLE batch's.  Workgroup
// (h, g): the group's segment by k_attn_segs_mq's scan, then the walk for queries i0 .. i0 + nq of that segment
inline __global__ void __launch_bounds__(kAttnBlock) k_attn_segs_prefix_mq(const AttnArgs a, const SegDesc f, const PrefixDesc px, int row_stride) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    int g = blockIdx.y, s = f.n_step;
    for (; s < f.n_segs - 1; ++s) {
        const int groups = (f.n[s] + px.G - 1) / px.G;
        if (g < groups) break;
        g -= groups;
    }
    const int i0 = g * px.G, left = f.n[s] - i0, nq = left < px.G ? left : px.G;
    if (nq < 1) return;                                                             // (a grid larger than the segments' groups: nothing to do; uniform)
    const PfxSegsGeo geo{f, px.S, s, i0, nq};
    if (a.hs <= 64) attn_prefix<1>(a, geo, blockIdx.x, lds, px.G, nq, px.tmax, row_stride); else attn_prefix<2>(a, geo, blockIdx.x, lds, px.G, nq, px.tmax, row_stride);
}

} // namespace flm
