// flm_tree.h -- tree draft-and-verify, greedy (flm_verify_tree_greedy; host side: flm_calls.hip, the batch pass: flm_prompt.hip prefill_batched with a TreeDesc).  Part of
// flm_kernels.h; include that header.  Ordinary grid launches: nothing here waits for another workgroup.
//
// A verify batch of n <= 16 rows that is a TREE of candidates: node 0 is the token fed at `pos`, node i > 0 a draft behind node parent[i] < i.  During the pass node i lives
// in PHYSICAL cache row pos + i; its LOGICAL position -- for RoPE and for the attention's order -- is pos + depth(i).  Node i attends the cache rows [0, pos) followed by its
// ancestors root .. itself.  A parent's index is smaller than its child's, so a node's ancestors in ascending INDEX order are its ancestors in ascending DEPTH order: the
// ancestor at depth e is the e-th set bit of the node's 16-bit ancestor mask, and its score lies at logical index pos + e.
//   k_rope_kv_tree  k_rope_kv_fan with a RoPE position per row: row i rotated at pos + depth[i], stored into cache row pos + i
//   k_attn_tree     every row over "the cache, then its ancestors", per query attn_head's arithmetic in the logical order
//   k_tree_accept   the walk from the rows' first maxima: root, then the lowest-indexed child whose token is the current row's id, until there is none
//   k_spec_draft_tree  the lookup loop's tree drafter ("spec_branches"): k_spec_draft's search B times over, the continuations merged by common prefix
//   k_tree_keep     the accepted node at depth d moved from physical row pos + path[d] to pos + d in every layer and head
#pragma once
#include "flm_fan.h"
#pragma clang fp contract(off)

namespace flm {

constexpr int kTreeMax = 16;
// one pass's geometry, built and checked by the host (tree_fill), by value into the launches: node i's parent, depth and ancestor mask (bit a: node a is i or above it)
struct TreeDesc { int pos, n; signed char parent[kTreeMax]; unsigned char depth[kTreeMax]; unsigned short mask[kTreeMax]; };
// what a pass leaves for the host, read back in ONE trip: count nodes on the accepted path (the root included), their indices by depth and the rows' ids along it
struct TreeOut { int count; int moved; int pad[2]; int ids[kTreeMax]; int path[kTreeMax]; };

// the rules of flm_tree_validate: null, or which one is broken
__host__ inline const char* tree_check(int n, const int* parent) {
    if (n < 2 || n > kTreeMax) return "tree: 2 <= n <= 16 nodes";
    if (!parent) return "tree: null parent array";
    if (parent[0] != -1) return "tree: parent[0] must be -1 (node 0 is the root)";
    for (int i = 1; i < n; ++i) if (parent[i] < 0 || parent[i] >= i) return "tree: 0 <= parent[i] < i for every draft (one root, parents in front of their children)";
    return nullptr;
}
// a checked parent array -> the launch descriptor
__host__ inline TreeDesc tree_fill(int pos, int n, const int* parent) {
    TreeDesc f{}; f.pos = pos; f.n = n;
    f.parent[0] = -1; f.depth[0] = 0; f.mask[0] = 1;
    for (int i = 1; i < n; ++i) {
        f.parent[i] = (signed char)parent[i]; f.depth[i] = (unsigned char)(f.depth[parent[i]] + 1);
        f.mask[i] = (unsigned short)(f.mask[parent[i]] | (1u << i));
    }
    return f;
}
// The accept walk (host restatement of k_tree_accept; a[i]: row i's first maximum): path[0] = 0; from node cur the LOWEST index i with parent[i] == cur and tokens[i] ==
// a[cur] is next; none: the walk ends.  -> the nodes on the path
__host__ inline int tree_walk(int n, const int* tokens, const int* parent, const int* a, int* path) {
    int cur = 0, len = 0;
    path[len++] = 0;
    for (;;) {
        int nxt = -1;
        for (int i = cur + 1; i < n && nxt < 0; ++i) if (parent[i] == cur && tokens[i] == a[cur]) nxt = i;
        if (nxt < 0) return len;
        path[len++] = cur = nxt;
    }
}

// qkv [n][3 dim] (the plain-store GEMM) -> q rotated into qout [n][dim], k rotated and v into cache row pos + b; row b at RoPE position pos + depth[b]
inline __global__ void k_rope_kv_tree(const float* qkv, float* qout, float* kcache, float* vcache, const float* rope_cos, const float* rope_sin,
                                      int dim, int hs, int max_seq, const TreeDesc f, const TreeDesc* dev) {
    const int b = blockIdx.x, pos = f.pos + (dev ? dev->depth[b] : f.depth[b]), prow = f.pos + b;
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
// The tree's attention (hs <= 128).  Workgroup (h, g) takes the G consecutive tree rows i0 = g * G ... of head h (G = 8, 4, 2 or 1: what the LDS allows, fan_group; the
// LDS layout is the fan's, fan_lds_bytes).  The tiles it walks, for K and again for V, each brought to LDS ONCE and used by every query of the group:
//   x < ntS   the cache rows [0, pos), physical rows x * 64 ...: every query sees all of them, logical index = physical row
//   x = ntS   the tree's own n rows, physical rows pos .. pos + n: query j keeps row a only where bit a of its ancestor mask is set, at logical index pos + (set bits below a)
// Rows of the tree tile that are not a query's ancestors are multiplied like the others (the K operand is shared) and the product dropped: nothing of them reaches a score
// row, and the weighted sum reads a V row only through a set mask bit.  Query j sees T_j = pos + depth(j) + 1 logical rows, so the queries of one group have score rows of
// different lengths.  Per query the arithmetic is attn_head's, operation for operation, as attn_fan restates it: a score is 8 strided accumulators added 0..7, * attn_scale;
// max, expf_ref, ONE sequential softmax-sum chain over the logical order and the division; the weighted sum is one chain per (query, dimension) -- logical row 0 (a cache
// row, or the root where pos == 0) by multiplication, every later row by FMA, |w| <= 1e-15 skipped.  Nothing is reduced per segment and combined.
// ------------------------------------------------------------------------------------------
template <int NF>
__device__ __forceinline__ void attn_tree(const AttnArgs& a, const TreeDesc& f, const TreeDesc* dev, const int h, char* lds, const int i0, const int nq, const int G, const int row_stride) {
    const unsigned short* const masks = dev ? dev->mask : f.mask;                 // (a tree drafted on the device: pos and n are the host's, the rows' masks and depths the drafter's)
    const unsigned char* const depths = dev ? dev->depth : f.depth;
    typedef float v4f __attribute__((ext_vector_type(4)));
    constexpr int rs = NF * 64 + 8;
    const int hs = a.hs, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int scs = ((a.max_seq + 3) & ~3) + 8;                                 // stride of a query's score row
    float* qs = reinterpret_cast<float*>(lds);                                  // [G][hs]
    float* sc = qs + G * hs;                                                    // [G][scs]
    float* tile0 = sc + G * scs;
    float* tile1 = tile0 + kAttnTile * rs;
    const int S = f.pos, n = f.n;
    const int ntS = (S + kAttnTile - 1) / kAttnTile, nt = ntS + 1;              // the cache tiles, then the tree's one
    const float* K = a.kcache + (size_t)h * (a.kv_rows ? a.kv_rows : a.max_seq) * hs;
    const float* V = a.vcache + (size_t)h * (a.kv_rows ? a.kv_rows : a.max_seq) * hs;
    const __amdgpu_buffer_rsrc_t rK = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(K), 0, a.max_seq * hs * 4, 0x00020000);
    const __amdgpu_buffer_rsrc_t rV = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(V), 0, a.max_seq * hs * 4, 0x00020000);
    const float scale = (float)(1.0 / (double)__builtin_sqrtf((float)hs));      // attn_scale, transformer.cpp:418
    // tile x: its first physical row (= the logical index of its first row for a cache tile) and how many rows it holds
    auto tile_row0 = [&](int x) { return x < ntS ? x * kAttnTile : S; };
    auto tile_rows = [&](int x) { const int r = x < ntS ? S - x * kAttnTile : n; return r > kAttnTile ? kAttnTile : r; };
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
        const int rows = x < nt ? tile_rows(x) : 0, row0 = x < nt ? tile_row0(x) : 0;
#pragma unroll
        for (int j = 0; j < NF; ++j) {
            const unsigned off = prow[j] < rows ? (unsigned)(row0 * hs * 4 + goff[j]) : 0x80000000u;
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
    // ---- scores.  thread = (query half, position p, accumulator k); its 4 queries share the K operand of every step
    {
        const int k = tid & 7, p = (tid >> 3) & 63, jh = (tid >> 9) * 4;
        auto qrow = [&](int j) { return qs + (j < G ? j : G - 1) * hs + k; };    // (queries past the group: any row of qs, the result is dropped)
        const float* q0 = qrow(jh + 0); const float* q1 = qrow(jh + 1); const float* q2 = qrow(jh + 2); const float* q3 = qrow(jh + 3);
        for (int x = 0; x < nt; ++x) {
            float* cur = (x & 1) ? tile1 : tile0;
            const int rows = tile_rows(x), t0 = tile_row0(x);
            const bool own = x == ntS;
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
                if (k != 0 || j >= nq || p >= rows) return;
                int t = t0 + p;                                                 // a cache row: every query's, at its own index
                if (own) {                                                      // a tree row: an ancestor's only, behind the ancestors in front of it
                    const unsigned m = masks[i0 + j];
                    if (!((m >> p) & 1u)) return;
                    t = S + __builtin_popcount(m & ((1u << p) - 1u));
                }
                sc[j * scs + t] = __fmul_rn(tot, scale);                        // att.multiply(attn_scale) :443
            };
            fold(l0, jh + 0); fold(l1, jh + 1); fold(l2, jh + 2); fold(l3, jh + 3);
        }
    }
    request(rV, 0, ring);                                                       // the first V tile travels under the softmax
    __syncthreads();
    // ---- softmax: wave j = query j over its OWN T scores in the logical order (max is order-free; the sum is the reference's sequential one, tf_operators.cpp:180-183)
    if (wave < nq) {
        const int T = S + depths[i0 + wave] + 1;
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
    // ---- o[j][d] = sum_t att_j[t] V[t][d]: one thread per (query, output dimension), t ascending in the logical order: the cache tiles, then the query's ancestors
    const int tpq = hs <= 64 ? 64 : 128;                                        // threads per query (a multiple of the wave: the skip test stays wave-uniform)
    const int j = tid / tpq, d = tid - j * tpq;
    const bool mine = j < nq && d < hs;
    const unsigned anc = mine ? masks[i0 + j] : 0u;
    float o = 0.f;
    for (int x = 0; x < nt; ++x) {
        float* cur = (x & 1) ? tile1 : tile0;
        const int np = tile_rows(x);
        park(cur, ring);
        __syncthreads();                                                        // (the first one also orders the softmax's writes before the reads below)
        request(rV, x + 1, ring);
        // the weights are wave-uniform (a wave's lanes belong to ONE query): if no row of the tile is skipped the walk is 8 reads ahead of 8 dependent FMAs.  All 64
        // lanes look, the ones that own no dimension (hs < 64) included: every row of the tile is inspected at every head size
        const bool whole = __all(!(x < ntS && j < nq && lane < np) || sc[j * scs + x * kAttnTile + lane] != 0.f);
        if (!mine) continue;
        const float* vp = cur + d;
        if (x < ntS) {
            const float* wp = sc + j * scs + x * kAttnTile;
            int p = 0;
            if (x == 0) { o = __fmul_rn(vp[0], wp[0]); p = 1; }                 // logical row 0 (tf_operators.cpp:331-336)
            if (whole) {
                for (; p < np && (p & 7); ++p) o = __fmaf_rn(vp[p * rs], wp[p], o);
                for (; p + 8 <= np; p += 8) {
                    const float* vq = vp + p * rs; const float4 wa = *reinterpret_cast<const float4*>(wp + p), wb = *reinterpret_cast<const float4*>(wp + p + 4);
                    const float a0 = vq[0], a1 = vq[rs], a2 = vq[2 * rs], a3 = vq[3 * rs], a4 = vq[4 * rs], a5 = vq[5 * rs], a6 = vq[6 * rs], a7 = vq[7 * rs];
                    o = __fmaf_rn(a0, wa.x, o); o = __fmaf_rn(a1, wa.y, o); o = __fmaf_rn(a2, wa.z, o); o = __fmaf_rn(a3, wa.w, o);
                    o = __fmaf_rn(a4, wb.x, o); o = __fmaf_rn(a5, wb.y, o); o = __fmaf_rn(a6, wb.z, o); o = __fmaf_rn(a7, wb.w, o);
                }
                for (; p < np; ++p) o = __fmaf_rn(vp[p * rs], wp[p], o);
            } else {
                for (; p < np; ++p) { const float w = wp[p]; o = w == 0.f ? o : __fmaf_rn(vp[p * rs], w, o); }
            }
        } else {                                                                // the ancestors by depth = the mask's set bits, lowest first
            const float* wp = sc + j * scs + S;
            unsigned m = anc;
            for (int e = 0; m; ++e, m &= m - 1) {
                const float v = vp[__builtin_ctz(m) * rs], w = wp[e];
                if (S + e == 0) o = __fmul_rn(v, w);                            // no cache row: the root is logical row 0
                else o = w == 0.f ? o : __fmaf_rn(v, w, o);
            }
        }
    }
    if (mine) a.out[(size_t)(i0 + j) * row_stride + (size_t)h * hs + d] = o;
}
// grid (heads, ceil(n / G)), kAttnBlock threads, fan_lds_bytes(G, a.max_seq, a.hs) of dynamic LDS; a.q / a.out [n][row_stride]
inline __global__ void __launch_bounds__(kAttnBlock) k_attn_tree(const AttnArgs a, const TreeDesc f, const TreeDesc* dev, int row_stride, int G) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    const int i0 = blockIdx.y * G, nq = f.n - i0 < G ? f.n - i0 : G;
    if (a.hs <= 64) attn_tree<1>(a, f, dev, blockIdx.x, lds, i0, nq, G, row_stride); else attn_tree<2>(a, f, dev, blockIdx.x, lds, i0, nq, G, row_stride);
}

// The accept step (one wave, lane i = node i).  a[i]: row i's first maximum; batch[i]: node i's token.  From the root the walk steps to the lowest-indexed child of the
// current node whose token is the current row's id (a ballot's lowest set bit), until there is none.  Writes the result block alone: a pass that is re-run stores the same words.
// so given (the lookup loop's step): the run is also cut to `room` ids and behind the first `stop` id, appended at hist[n_hist ..) and left in the loop's SpecOut block
// (temperature 0: the state passes through), as k_spec_accept_sample leaves a chain's
inline __global__ void __launch_bounds__(kWave) k_tree_accept(TreeOut* out, const int* __restrict__ a, const int* __restrict__ batch, const TreeDesc f, const TreeDesc* dev,
                                                              SpecOut* so, int* hist, int n_hist, int stop, int room, unsigned long long base) {
    const int i = threadIdx.x;
    if (blockIdx.x != 0) return;
    const int par = i < f.n ? (dev ? dev->parent[i] : f.parent[i]) : -2, tok = i < f.n ? batch[i] : -1;
    int cur = 0, len = 1, moved = 0, my_id = -1, my_node = -1;
    if (i == 0) { my_id = a[0]; my_node = 0; }
    for (;;) {
        const int want = a[cur];
        const unsigned long long hit = __ballot(par == cur && tok == want);
        if (!hit) break;
        cur = __builtin_ctzll(hit);
        if (i == len) { my_id = a[cur]; my_node = cur; }
        moved |= cur != len;
        ++len;
    }
    if (i < kTreeMax) { out->ids[i] = i < len ? my_id : -1; out->path[i] = i < len ? my_node : -1; }
    if (i == 0) { out->count = len; out->moved = moved; out->pad[0] = out->pad[1] = 0; }
    if (!so) return;
    int n = len < room ? len : room;
    const unsigned long long ends = __ballot(i < n && my_id == stop) ;
    const int stopped = ends != 0;
    if (stopped) n = __builtin_ctzll(ends) + 1;
    if (i < n) { so->ids[i] = my_id; hist[n_hist + i] = my_id; }
    if (i == 0) { so->m = len - 1; so->n_emit = n; so->stopped = stopped; so->pad = 0; so->rng = base; }
}

// The tree drafter of the lookup loop ("spec_branches" B > 1): k_spec_draft's search, B times over.  Round r keeps the largest key (len << 24 | e) below round r - 1's
// whose continuation -- cont(e)[i] = h[e + i % (n - e)], i < K -- differs from every continuation kept so far: the B most recent, longest-matching DISTINCT places of the
// history that continue the current suffix (fewer where the history has fewer; none: the one continuation h[n - 1] repeated, as k_spec_draft drafts without a match).  A max
// reduction per round: order-free.  Thread 0 then merges the continuations by common prefix into a tree of EXACTLY K + 1 nodes, breadth first: for depth i = 0 .. K - 1, for
// candidate c = 0 .. : the child of c's current node with token cont(c)[i] is reused or appended, until the nodes are used up -- candidate 0 appends one node per depth, so
// the budget is always met and the host knows n without a trip.  Parents precede children.  Writes batch[0 .. K] (the nodes' tokens) and the descriptor's parent / depth /
// mask arrays (pos and n are launch arguments of the kernels that read it).  B = 1 gives k_spec_draft's chain.  One workgroup of 1024 threads; n < 2^24
inline __global__ void __launch_bounds__(kSampleBlock) k_spec_draft_tree(const int* __restrict__ h, int n, int K, int ngram_max, int B, int* __restrict__ batch, TreeDesc* out) {
    __shared__ unsigned red[kSampleWaves];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    auto cont = [&](int e, int i) { return h[e + i % (n - e)]; };
    unsigned ch[4] = {0, 0, 0, 0}, last = 0xffffffffu;
    int nch = 0;
    for (int r = 0; r < B && r < 4; ++r) {
        unsigned best = 0;
        for (int e = 1 + t; e <= n - 1; e += kSampleBlock) {
            const int cap = ngram_max < e ? ngram_max : e;
            int len = 0;
            while (len < cap && h[e - 1 - len] == h[n - 1 - len]) ++len;
            const unsigned key = len ? ((unsigned)len << 24) | (unsigned)e : 0u;
            if (!key || key >= last || key <= best) continue;
            bool dup = false;
            for (int c = 0; c < nch && !dup; ++c) {
                const int ec = (int)(ch[c] & 0xffffffu);
                int i = 0;
                while (i < K && cont(e, i) == cont(ec, i)) ++i;
                dup = i == K;
            }
            if (!dup) best = key;
        }
        for (int o = 32; o > 0; o >>= 1) { const unsigned ov = (unsigned)__shfl_xor((int)best, o, kWave); best = ov > best ? ov : best; }
        __syncthreads();                                                        // (the previous round's reads of red)
        if (lane == 0) red[w] = best;
        __syncthreads();
        best = red[0];
        for (int k = 1; k < kSampleWaves; ++k) best = red[k] > best ? red[k] : best;
        if (!best) break;
        ch[nch++] = last = best;
    }
    if (t != 0) return;
    const int N = K + 1, nc = nch ? nch : 1;
    int tok[kTreeMax], par[kTreeMax], node[4] = {0, 0, 0, 0}, cnt = 1;
    tok[0] = h[n - 1]; par[0] = -1;
    for (int i = 0; i < K && cnt < N; ++i)
        for (int c = 0; c < nc && cnt < N; ++c) {
            const int v = nch ? cont((int)(ch[c] & 0xffffffu), i) : h[n - 1];
            int found = -1;
            for (int j = 1; j < cnt && found < 0; ++j) if (par[j] == node[c] && tok[j] == v) found = j;
            if (found < 0) { tok[cnt] = v; par[cnt] = node[c]; found = cnt++; }
            node[c] = found;
        }
    out->pos = 0; out->n = N;
    for (int i = 0; i < N; ++i) {
        batch[i] = tok[i];
        out->parent[i] = (signed char)par[i];
        out->depth[i] = i ? (unsigned char)(out->depth[par[i]] + 1) : 0;
        out->mask[i] = i ? (unsigned short)(out->mask[par[i]] | (1u << i)) : 1;
    }
}

// The accepted node at depth e, physical row pos + path[e], becomes row pos + e of every layer's and head's K and V; ascending depth, which is safe because path[e] >= e and
// path is ascending: a later depth's source lies behind every row written so far.  Does nothing where the path is in place already (res->moved == 0).  blockIdx.x = layer *
// heads + head (the caches are [layers][heads][kv_rows][hs]); 16-byte pieces, thread t < hs / 4 the K piece, hs / 4 <= t < hs / 2 the V piece
inline __global__ void k_tree_keep(float* kcache, float* vcache, int kv_rows, int hs, int pos, const TreeOut* __restrict__ res) {
    if (!res->moved) return;
    const size_t head = (size_t)blockIdx.x * kv_rows * hs;
    const int f4r = hs / 4, t = threadIdx.x;
    if (t >= 2 * f4r) return;
    float* base = (t < f4r ? kcache : vcache) + head;
    const int c4 = t < f4r ? t : t - f4r, count = res->count;
    for (int e = 1; e < count; ++e) {
        const int src = res->path[e];
        if (src == e) continue;
        reinterpret_cast<float4*>(base + (size_t)(pos + e) * hs)[c4] = reinterpret_cast<const float4*>(base + (size_t)(pos + src) * hs)[c4];
    }
}

} // namespace flm
