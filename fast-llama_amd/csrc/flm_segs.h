// flm_segs.h -- ragged passes over the cache slots (flm_batch_admit / flm_batch_pass; host side: flm_calls.hip, the batch pass: flm_prompt.hip prefill_batched with a
// SegDesc).  Part of flm_kernels.h; include that header.  Ordinary grid launches: nothing here waits for another workgroup.
//
// A pass is a list of at most 16 segments, at most one per slot.  The batch's rows [0, L) are the running slots' step rows (n = 1 segments, in slot order): they keep
// flm_batch.h's kernels.  Rows [L, L + P) are the prompt segments of the filling slots in ascending slot order: segment s is a chunk of n[s] rows of its slot's prompt
// that enters at LOGICAL position pos0[s] (0: the prompt's first chunk; > 0: the rows in front of it were written by earlier passes).  For those rows:
//   k_rope_kv_segs   k_rope_kv_slots with row b's position pos0[s] + (b - row0[s]) and cache row base[s] + that position
//   k_seg_views      segment s's view of the cache AND of the batch -- origin at its slot, bound = the slot's rows, q and out moved to its first row -- as an AttnArgs in
//                    device memory
//   k_attn_segs_mq   workgroup (h, g) finds its segment and its group of kMqQueries queries inside it and runs attn_prefill_mq on the segment's view: the queries of ONE
//                    sequence share every K / V tile of that sequence's slot
//   k_attn_segs      workgroup (h, row) runs attn_head on the row's segment view (head sizes above 128, slots whose multi-query LDS does not fit, "use_prefill_mq" 0)
//   k_gather_rows    the draw rows -- the last row of every segment that completes its prompt -- brought together behind the step rows, so that the classifier reads
//                    its weights once for all of them
#pragma once
#include "flm_batch.h"
#pragma clang fp contract(off)

namespace flm {

// segments [0, n_step) are the step rows (row0[s] = s, n[s] = 1), [n_step, n_segs) the prompt segments; segment s belongs to slot slot[s], whose region starts at
// physical row base[s] and has rows[s] rows; its n[s] batch rows start at batch row row0[s] and at logical position pos0[s]
struct SegDesc { int n_segs, n_step; int slot[kBatchMax]; int row0[kBatchMax]; int n[kBatchMax]; int base[kBatchMax]; int pos0[kBatchMax]; int rows[kBatchMax]; };

// the prompt segment batch row b lies in (b >= n_step; uniform per workgroup)
__device__ __forceinline__ int seg_of_row(const SegDesc& f, const int b) {
    int s = f.n_step;
    for (int i = f.n_step; i < f.n_segs; ++i) if (b >= f.row0[i]) s = i;
    return s;
}

// qkv [B][3 dim] (the plain-store GEMM) -> q rotated into qout [B][dim], k rotated and v into the layer's cache rows; one workgroup per PROMPT row b = n_step + blockIdx.x
// (k_rope_kv_slots' arithmetic; max_seq: the stride between two heads' rows)
inline __global__ void k_rope_kv_segs(const float* qkv, float* qout, float* kcache, float* vcache, const float* rope_cos, const float* rope_sin,
                                      int dim, int hs, int max_seq, const SegDesc f) {
    const int b = f.n_step + blockIdx.x, s = seg_of_row(f, b);
    const int pos = f.pos0[s] + (b - f.row0[s]), prow = f.base[s] + pos;
    const float* in = qkv + (size_t)b * 3 * dim;
    for (int i = threadIdx.x; i < dim / 2; i += blockDim.x) {
        const int row = 2 * i, h = row / hs, d = row - h * hs;
        const float c = rope_cos[(size_t)pos * (hs / 2) + d / 2], sn = rope_sin[(size_t)pos * (hs / 2) + d / 2];
        float o0, o1;
        rope_pair(in[row], in[row + 1], c, sn, o0, o1);
        qout[(size_t)b * dim + row] = o0; qout[(size_t)b * dim + row + 1] = o1;
        rope_pair(in[dim + row], in[dim + row + 1], c, sn, o0, o1);
        float* kp = kcache + ((size_t)h * max_seq + prow) * hs + d; kp[0] = o0; kp[1] = o1;
        float* vp = vcache + ((size_t)h * max_seq + prow) * hs + d; vp[0] = in[2 * dim + row]; vp[1] = in[2 * dim + row + 1];
    }
}

// k_slot_views for the prompt segments: views[s] (s in [n_step, n_segs)) is segment s's cache AND batch -- the heads keep their stride, the origin moves by base[s] rows,
// the bound shrinks to the slot's rows, and q / out move by row0[s] rows, so that the segment's queries are rows 0 .. n[s] of its view (what attn_prefill_mq indexes)
inline __global__ void k_seg_views(const AttnArgs a, const SegDesc f, int row_stride, AttnArgs* __restrict__ views) {
    const int s = threadIdx.x;
    if (blockIdx.x != 0 || s < f.n_step || s >= f.n_segs) return;
    AttnArgs v = a;
    v.kv_rows = a.kv_rows ? a.kv_rows : a.max_seq;
    v.kcache = a.kcache + (size_t)f.base[s] * a.hs; v.vcache = a.vcache + (size_t)f.base[s] * a.hs;
    v.max_seq = f.rows[s];
    v.q = a.q + (size_t)f.row0[s] * row_stride; v.out = a.out + (size_t)f.row0[s] * row_stride;
    views[s] = v;
}

// grid (heads, sum over the prompt segments of ceil(n[s] / kMqQueries)), kAttnBlock threads, attn_mq_lds_bytes(the largest rows[s], hs) of dynamic LDS (a view's score
// rows are laid out by ITS bound).  Workgroup (h, g): the group's segment by a scan, then attn_prefill_mq on that segment's view -- queries i0 .. i0 + nq of the segment at
// logical positions pos0[s] + i0 ..: every query's arithmetic is attn_head's, operation for operation (flm_attn.h)
inline __global__ void __launch_bounds__(kAttnBlock) k_attn_segs_mq(const AttnArgs* __restrict__ views, const SegDesc f, int row_stride) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    int g = blockIdx.y, s = f.n_step;
    for (; s < f.n_segs - 1; ++s) {
        const int groups = (f.n[s] + kMqQueries - 1) / kMqQueries;
        if (g < groups) break;
        g -= groups;
    }
    const int i0 = g * kMqQueries, left = f.n[s] - i0, nq = left < kMqQueries ? left : kMqQueries;
    if (nq < 1) return;                                                             // (a grid larger than the segments' groups: nothing to do; uniform)
    const AttnArgs& a = views[s];
    if (a.hs <= 64) attn_prefill_mq<1, false>(a, blockIdx.x, lds, f.pos0[s], i0, nq, row_stride); else attn_prefill_mq<2, false>(a, blockIdx.x, lds, f.pos0[s], i0, nq, row_stride);
}

// grid (heads, P), kAttnBlock threads, attn_lds_bytes(the largest rows[s], hs): workgroup (h, r) is prompt row b = n_step + r, query i = b - row0[s] of its segment, over
// T = pos0[s] + i + 1 rows of the segment's view: k_attn_slots' call, any accepted head size
inline __global__ void __launch_bounds__(kAttnBlock) k_attn_segs(const AttnArgs* __restrict__ views, const SegDesc f, int row_stride) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    const int b = f.n_step + blockIdx.y, s = seg_of_row(f, b), i = b - f.row0[s];
    const AttnArgs& a = views[s];
    attn_head_any<false, false>(a, blockIdx.x, lds, f.pos0[s] + i + 1, a.q + (size_t)i * row_stride, a.out + (size_t)i * row_stride);
}

// The draw rows of a pass: rows [0, dst0) are the step rows and stay; row src[j] (the last row of the j-th completing segment, ascending) moves to row dst0 + j.
// dst0 + j <= src[j] < src[j + 1]: a destination is never the source of a LATER copy, but it can be the source of an earlier one -- so ONE workgroup copies in ascending
// order, each row read into registers by all threads in front of a barrier and stored behind it.
struct GatherDesc { int n, dst0; int src[kBatchMax]; };
inline __global__ void __launch_bounds__(256) k_gather_rows(float* x, int dim, const GatherDesc g) {
    if (blockIdx.x != 0) return;
    for (int j = 0; j < g.n; ++j) {
        const int src = g.src[j], dst = g.dst0 + j;
        if (src == dst) continue;                                                   // (uniform)
        for (int i0 = 0; i0 < dim; i0 += 256) {
            const int i = i0 + threadIdx.x;
            if (i < dim) x[(size_t)dst * dim + i] = x[(size_t)src * dim + i];     // (src != dst rows: the row's own reads and writes do not overlap)
        }
        __syncthreads();
    }
}

} // namespace flm
