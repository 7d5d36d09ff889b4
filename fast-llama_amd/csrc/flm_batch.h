// flm_batch.h -- cache slots (flm_batch_*: up to 16 INDEPENDENT sequences per pass over the weights; host side: flm_calls.hip, the batch pass: flm_prompt.hip
// prefill_batched with a SlotDesc).  Part of flm_kernels.h; include that header.  Ordinary grid launches: nothing here waits for another workgroup.
//
// The cache stays one cache.  Slot s owns the physical rows [base[s], base[s] + rows[s]) of every layer and head (include/flm_gpu.h flm_batch_layout_for); its sequence's
// LOGICAL position p -- for RoPE and for the attention's order -- lives in physical row base[s] + p.  A prompt enters a slot as one ordinary batch whose cache pointers are
// shifted by the slot's origin (prefill_batched's row0).  A step feeds the live slots' last ids as one batch of B rows, compacted (a finished or empty slot is not in it):
//   k_slots_load     the ids the host holds become the batch (a step's inputs are launch arguments: a re-run step enqueues the same work)
//   k_rope_kv_slots  k_rope_kv_fan with row r's OWN RoPE position pos[r] and cache row base[r] + pos[r]
//   k_slot_views     row r's view of the cache -- origin at its slot, bound = the slot's rows -- as an AttnArgs in device memory
//   k_attn_slots     workgroup (h, r) runs attn_head on row r's view over T = pos[r] + 1 rows: k_attn_prefill's call, the token path's arithmetic
//   k_sample_slots   k_sample_fan with row r's own temperature, top-p and state
//   k_batch_accept   the step's result block: ids by SLOT, the live and finished masks, the states behind the draws; the host reads it once per step
#pragma once
#include "flm_fan.h"
#pragma clang fp contract(off)

namespace flm {

constexpr int kBatchMax = kFanMax;
// one step's geometry: n live rows; row r is slot slot[r], whose region starts at physical row base[r] and has rows[r] rows; it is fed at logical position pos[r]
struct SlotDesc { int n; int slot[kBatchMax]; int base[kBatchMax]; int pos[kBatchMax]; int rows[kBatchMax]; };
// what the host holds of the step's rows, by value into its launches: row r's last id, sampler state and parameters, its stop token (-1: none) and how many ids it may
// still deliver (this step's included); live: the slots running in front of the step
struct SlotIn { int ids[kBatchMax]; unsigned long long rng[kBatchMax]; float temp[kBatchMax]; float topp[kBatchMax]; int stop[kBatchMax]; int left[kBatchMax]; unsigned live; int pad; };
// what a step leaves for the host, read back in ONE trip, indexed by SLOT: ids (-1: the slot delivered nothing), the slots still running behind the step, the slots whose
// last id is in it, the states behind the step's draws
struct SlotOut { int ids[kBatchMax]; unsigned live; unsigned finished; unsigned long long rng[kBatchMax]; };

inline __global__ void k_slots_load(const SlotIn in, int n, int* __restrict__ batch) {
    if (blockIdx.x == 0 && (int)threadIdx.x < n) batch[threadIdx.x] = in.ids[threadIdx.x];
}

// qkv [n][3 dim] (the plain-store GEMM) -> q rotated into qout [n][dim], k rotated and v into the layer's cache rows; row b at ITS RoPE position pos[b], cache row base[b] + pos[b]
// (max_seq: the stride between two heads' rows)
inline __global__ void k_rope_kv_slots(const float* qkv, float* qout, float* kcache, float* vcache, const float* rope_cos, const float* rope_sin,
                                       int dim, int hs, int max_seq, const SlotDesc f) {
    const int b = blockIdx.x, pos = f.pos[b], prow = f.base[b] + pos;
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

// Row r sees its slot as a cache of its own: an AttnArgs whose heads keep their stride (a.kv_rows, or a.max_seq where that is 0), whose origin has moved by base[r] rows and
// whose buffer bound has shrunk to the slot's rows, so no read reaches a neighbour's region.  attn_head takes its arguments by reference and indexes into them; a modified
// COPY inside the attention kernel would live in scratch.  So the n views are written to device memory (views [kBatchMax], there since create) by this one-wave kernel in
// front of the attention, which then reads its row's view as it would read launch arguments.
inline __global__ void k_slot_views(const AttnArgs a, const SlotDesc f, AttnArgs* __restrict__ views) {
    const int r = threadIdx.x;
    if (blockIdx.x != 0 || r >= f.n) return;
    AttnArgs s = a;
    s.kv_rows = a.kv_rows ? a.kv_rows : a.max_seq;
    s.kcache = a.kcache + (size_t)f.base[r] * a.hs; s.vcache = a.vcache + (size_t)f.base[r] * a.hs;
    s.max_seq = f.rows[r];
    views[r] = s;
}
// grid (heads, n), kAttnBlock threads, attn_lds_bytes(the largest rows[r], hs) of dynamic LDS; q / out [n][row_stride].  Workgroup (h, r): attn_head over row r's view,
// T = pos[r] + 1 rows (T = 1: a sequence's first fed token behind a 1-token prompt -- attn_head's first row is a multiplication, nothing follows): k_attn_prefill's call,
// the token path's arithmetic
inline __global__ void __launch_bounds__(kAttnBlock) k_attn_slots(const AttnArgs* __restrict__ views, const SlotDesc f, int row_stride) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    const int r = blockIdx.y;
    const AttnArgs& s = views[r];
    attn_head_any<false, false>(s, blockIdx.x, lds, f.pos[r] + 1, s.q + (size_t)r * row_stride, s.out + (size_t)r * row_stride);
}

// One workgroup of 1024 threads per row of a classifier chunk: chunk row r (logits + r * ld) is batch row row0 + r, drawn by sample_draw with that row's OWN state, temperature
// and top-p, in its own [2][n] slice of sort_buf.  temp == 0: the first maximum, the state passes through.  Writes drawn[row0 + r] and after[row0 + r], nothing else.
inline __global__ void __launch_bounds__(kSampleBlock) k_sample_slots(const float* __restrict__ logits, int ld, int n, int row0, const SlotIn in,
                                                                      unsigned long long* sort_buf, int* __restrict__ drawn, unsigned long long* __restrict__ after) {
    extern __shared__ float4 sample_lds4[];       // a sampled row in the batch: sample_lds_bytes(n); else the first maximum's 2 * kSampleWaves words
    const int r = blockIdx.x, row = row0 + r;
    const float* x = logits + (size_t)r * ld;
    const float temp = in.temp[row], topp = in.topp[row];
    unsigned long long rng = in.rng[row];
    int tok;
    if (temp == 0.0f) tok = block_first_max([&](int i) { return x[i]; }, n, 0, reinterpret_cast<int*>(sample_lds4));
    else tok = sample_draw(x, n, temp, topp, rng, sort_buf + (size_t)row * 2 * n, reinterpret_cast<float*>(sample_lds4));
    if (threadIdx.x == 0) { drawn[row] = tok; after[row] = rng; }
}

// The accept step (one wave, lane s = SLOT s): a slot whose row is in the batch delivers the row's id, with the state behind the draw, and leaves the live set when the id
// is its stop token or its last allowed one; every other slot delivers -1.  Everything it reads besides the two arrays the draw kernel wrote is a launch argument, and it
// writes the result block alone: a step that is re-run stores the same words again.
inline __global__ void k_batch_accept(SlotOut* out, const int* __restrict__ drawn, const unsigned long long* __restrict__ after, const SlotIn in, const SlotDesc f) {
    const int s = threadIdx.x;
    if (blockIdx.x != 0 || s >= 64) return;
    int r = -1;
    for (int i = 0; i < f.n; ++i) if (f.slot[i] == s) r = i;
    const int id = r >= 0 ? drawn[r] : -1;
    const bool done = r >= 0 && ((in.stop[r] >= 0 && id == in.stop[r]) || in.left[r] <= 1);
    const unsigned fin = (unsigned)__ballot(done);
    if (s < kBatchMax) { out->ids[s] = id; out->rng[s] = r >= 0 ? after[r] : 0ull; }
    if (s == 0) { out->finished = fin; out->live = in.live & ~fin; }
}

} // namespace flm
