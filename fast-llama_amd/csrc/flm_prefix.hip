// flm_prefix.hip -- the launchers of the attention behind a shared prefix (kernels: flm_prefix.h; callers: flm_prompt.hip prefill_batched with a PrefixDesc, flm_ops.hip).
// The only translation unit that instantiates k_attn_slots_prefix / k_attn_segs_prefix_mq.
#include "flm_host.h"

namespace fh {

// both kernels' score rows and tiles can take most of the LDS: raise their dynamic-LDS limit, once per device
static int prefix_lds_limit(flm_ctx* c) {
    static std::mutex mu; static bool done[64] = {false};
    int dev = 0; HIPC(c, hipGetDevice(&dev));
    std::lock_guard<std::mutex> lk(mu);
    if (dev >= 0 && dev < 64 && !done[dev]) {
        HIPC(c, hipFuncSetAttribute(reinterpret_cast<const void*>(&k_attn_slots_prefix), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsMax));
        HIPC(c, hipFuncSetAttribute(reinterpret_cast<const void*>(&k_attn_segs_prefix_mq), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsMax));
        done[dev] = true;
    }
    return FLM_OK;
}
// S shared rows, the launch's longest logical length, and the queries per workgroup that length allows; G = 0: not even one query's scores fit
static PrefixDesc prefix_desc(int S, int largest_rows, int hs) {
    PrefixDesc px{S, S + largest_rows, 0};
    const int G = prefix_group(px.tmax, hs, kLdsMax);
    px.G = prefix_lds_bytes(G, px.tmax, hs) <= kLdsMax ? G : 0;
    return px;
}

// k_attn_slots_prefix on the n live rows of a batch step behind S shared rows: f.base = the slots' physical origins (>= S), f.pos = the rows' logical positions (>= S).
// c may be null (flm_op_attention_slots_prefix)
int launch_attn_slots_prefix(flm_ctx* c, hipStream_t st, const AttnArgs& aa, const SlotDesc& f, int S, int heads, int row_stride) {
    int r = prefix_lds_limit(c); if (r) return r;
    if (aa.hs > 128 || aa.hs % 8 || f.n < 1 || f.n > kBatchMax || aa.n_peer || S < 1) return fail(c, FLM_ERR_INVALID, "attn_slots_prefix: head size <= 128, 1 .. 16 rows, one GPU, at least one shared row");
    int largest = 0;
    for (int i = 0; i < f.n; ++i) {
        if (f.base[i] < S || f.rows[i] < 1 || (long long)f.base[i] + f.rows[i] > aa.max_seq || f.pos[i] < S || f.pos[i] - S >= f.rows[i])
            return fail(c, FLM_ERR_INVALID, "attn_slots_prefix: a row outside its slot, a slot outside the cache, or a slot inside the prefix");
        largest = f.rows[i] > largest ? f.rows[i] : largest;
    }
    const PrefixDesc px = prefix_desc(S, largest, aa.hs);
    if (!px.G) return fail(c, FLM_ERR_UNSUPPORTED, "attn_slots_prefix: one query's scores do not fit the LDS");
    hipLaunchKernelGGL(k_attn_slots_prefix, dim3(heads, (f.n + px.G - 1) / px.G), dim3(kAttnBlock), prefix_lds_bytes(px.G, px.tmax, aa.hs), st, aa, f, px, row_stride);
    HIPC(c, hipGetLastError());
    return FLM_OK;
}
// k_attn_segs_prefix_mq on the prompt segments [n_step, n_segs) of a ragged pass behind S shared rows: f.base physical (>= S), f.pos0 logical (>= S); q / out are the WHOLE
// batch's.  The caller has run seg_check on the pass with pos0 - S.  c may be null (flm_op_attention_segs_prefix)
int launch_attn_segs_prefix(flm_ctx* c, hipStream_t st, const AttnArgs& aa, const SegDesc& f, int S, int heads, int row_stride) {
    int r = prefix_lds_limit(c); if (r) return r;
    if (aa.hs > 128 || aa.hs % 8 || aa.n_peer || S < 1 || f.n_step < 0 || f.n_step >= f.n_segs || f.n_segs > kBatchMax) return fail(c, FLM_ERR_INVALID, "attn_segs_prefix: head size <= 128, one GPU, at least one shared row and one prompt segment");
    int largest = 0;
    for (int s = f.n_step; s < f.n_segs; ++s) {
        if (f.base[s] < S || f.rows[s] < 1 || (long long)f.base[s] + f.rows[s] > aa.max_seq || f.n[s] < 1 || f.pos0[s] < S || (long long)f.pos0[s] - S + f.n[s] > f.rows[s])
            return fail(c, FLM_ERR_INVALID, "attn_segs_prefix: a segment outside its slot, a slot outside the cache, or a slot inside the prefix");
        largest = f.rows[s] > largest ? f.rows[s] : largest;
    }
    const PrefixDesc px = prefix_desc(S, largest, aa.hs);
    if (!px.G) return fail(c, FLM_ERR_UNSUPPORTED, "attn_segs_prefix: one query's scores do not fit the LDS");
    int groups = 0;
    for (int s = f.n_step; s < f.n_segs; ++s) groups += (f.n[s] + px.G - 1) / px.G;
    hipLaunchKernelGGL(k_attn_segs_prefix_mq, dim3(heads, groups), dim3(kAttnBlock), prefix_lds_bytes(px.G, px.tmax, aa.hs), st, aa, f, px, row_stride);
    HIPC(c, hipGetLastError());
    return FLM_OK;
}

} // namespace fh
