// flm_prompt.hip -- the batched prompt path: all tokens of a prompt but the last through GEMM tiles on the int8 matrix cores and prompt attention on the fp32 matrix
// cores; they leave the K/V rows the token-by-token path would (flm_prefill.h).
#include "flm_host.h"

namespace fh {

// ---------------------------------------------------------------------------------------------
// Batched prefill of B prompt tokens at positions pos .. pos+B-1 (single GPU): leaves their K/V rows in the cache, exactly
// the rows the token-by-token path would write (flm_kernels.h, "Batched prefill").  The prompt's LAST token is not part
// of the batch: it runs through the decode kernels and produces the logits.
// ---------------------------------------------------------------------------------------------
template <int QT, int PRO>
int launch_rows(flm_ctx* c, hipStream_t st, const RowsArgs& r, int B, bool coh = false) {
    const size_t lds = (size_t)gemv_lds_layout(r.n, QTraits<QT>::kEsz, true, 4, 4, false).total;
    const int rounds = (r.n + kGemvBlock * 4 - 1) / (kGemvBlock * 4);
    if (coh) {   // the rows lie in the exchange buffer and were partly written by peer GPUs
        if (rounds <= 1)      hipLaunchKernelGGL((k_rows_prologue<QT, PRO, 1, true>), dim3(B), dim3(kGemvBlock), lds, st, r);
        else if (rounds <= 3) hipLaunchKernelGGL((k_rows_prologue<QT, PRO, 3, true>), dim3(B), dim3(kGemvBlock), lds, st, r);
        else                  hipLaunchKernelGGL((k_rows_prologue<QT, PRO, 0, true>), dim3(B), dim3(kGemvBlock), lds, st, r);
    }
    else if (rounds <= 1) hipLaunchKernelGGL((k_rows_prologue<QT, PRO, 1>), dim3(B), dim3(kGemvBlock), lds, st, r);
    else if (rounds <= 3) hipLaunchKernelGGL((k_rows_prologue<QT, PRO, 3>), dim3(B), dim3(kGemvBlock), lds, st, r);
    else                  hipLaunchKernelGGL((k_rows_prologue<QT, PRO, 0>), dim3(B), dim3(kGemvBlock), lds, st, r);
    HIPC(c, hipGetLastError());
    return FLM_OK;
}
// use_mfma (int8): 1 tile shape by size, 2 (and 0) always 64 x 64, 3 always 128 x 128 matrix-core tiles; int16: always the hi / lo byte planes on the int8 matrix cores
template <int QT, int EPI>
int launch_gemm(flm_ctx* c, hipStream_t st, const GemmArgs& g, int use_mfma) {
    const int tiles = ((g.rows + 63) / 64) * ((g.B + 63) / 64);
    if (use_mfma == 0) use_mfma = 2;
    if (QT == QT_INT8) {   // exact int32 group dots on v_mfma_i32_32x32x32_i8
        using Big = GemmTile<4, 2, 2>; using Small = GemmTile<2, 2, 1>;
        {   // the 128 x 128 tiles stage 76 KiB of LDS: raise the kernels' dynamic-LDS limit, once per device
            static std::mutex mu; static bool done[64] = {false};
            int dev = 0; HIPC(c, hipGetDevice(&dev));
            std::lock_guard<std::mutex> lk(mu);
            if (dev >= 0 && dev < 64 && !done[dev]) {
                HIPC(c, hipFuncSetAttribute(reinterpret_cast<const void*>(&k_gemm_q8_mfma<EPI_STORE, 4, 2, 2>), hipFuncAttributeMaxDynamicSharedMemorySize, Big::kLds));
                HIPC(c, hipFuncSetAttribute(reinterpret_cast<const void*>(&k_gemm_q8_mfma<EPI_RESIDUAL, 4, 2, 2>), hipFuncAttributeMaxDynamicSharedMemorySize, Big::kLds));
                HIPC(c, hipFuncSetAttribute(reinterpret_cast<const void*>(&k_gemm_q8_mfma<EPI_SWIGLU, 4, 2, 2>), hipFuncAttributeMaxDynamicSharedMemorySize, Big::kLds));
                HIPC(c, hipFuncSetAttribute(reinterpret_cast<const void*>(&k_gemm_q8_mfma<EPI_ROPE_KV, 4, 2, 2>), hipFuncAttributeMaxDynamicSharedMemorySize, Big::kLds));
                done[dev] = true;
            }
        }
        if constexpr (EPI == EPI_SWIGLU) {   // g.rows = hidden: a tile = 64 rows of W1 and of W3 (gemm_fuses_swiglu decides)
            const int tiles = ((g.rows + Big::TR / 2 - 1) / (Big::TR / 2)) * ((g.B + Big::TT - 1) / Big::TT);
            hipLaunchKernelGGL((k_gemm_q8_mfma<EPI_SWIGLU, 4, 2, 2>), dim3(tiles), dim3(Big::NT), Big::kLds, st, g);
            HIPC(c, hipGetLastError());
            return FLM_OK;
        } else {
        const int tiles128 = ((g.rows + Big::TR - 1) / Big::TR) * ((g.B + Big::TT - 1) / Big::TT);
        // 128 x 128 tiles move 0.6x the LDS cycles and half the bytes per product; they pay once every CU has one (measured, 7B width:
        // 512 tokens qkv / ffn13 100.8 vs 115.3 us, Wo / ffn2 (128 tiles) 95.4 vs 65.4; 1000 tokens 171 vs 221 and 110 vs 117)
        if (use_mfma == 3 || (use_mfma == 1 && tiles128 >= 256)) hipLaunchKernelGGL((k_gemm_q8_mfma<EPI, 4, 2, 2>), dim3(tiles128), dim3(Big::NT), Big::kLds, st, g);
        else hipLaunchKernelGGL((k_gemm_q8_mfma<EPI, 2, 2, 1>), dim3(tiles), dim3(Small::NT), Small::kLds, st, g);
        }
    }
    else if constexpr (EPI == EPI_SWIGLU) {   // g.rows = hidden: a tile = 32 rows of W1 and the same rows of W3
        const int tiles2 = ((g.rows + 31) / 32) * ((g.B + 63) / 64);
        hipLaunchKernelGGL((k_gemm_q16_mfma<EPI_SWIGLU>), dim3(tiles2), dim3(256), Gemm16Tile::kLds, st, g);
    }
    else hipLaunchKernelGGL((k_gemm_q16_mfma<EPI>), dim3(tiles), dim3(256), Gemm16Tile::kLds, st, g);   // hi / lo byte planes on the int8 matrix cores
    HIPC(c, hipGetLastError());
    return FLM_OK;
}

// The skinny int8 GEMM of the verify pass (flm_prefill.h k_gemm_q8_skinny): B <= 16 tokens, one wave per workgroup.  Two fragments (32 rows) per wave where that still
// gives every CU a workgroup, else one (16 rows: Wo and W2 of the 7B shape = 256 workgroups); SwiGLU: the same 16 rows of W1 and W3.
template <int EPI>
int launch_gemm_skinny(flm_ctx* c, hipStream_t st, const GemmArgs& g, int force_nb = 0) {
    if (g.B < 1 || g.B > kSkinnyTokens || g.n_peer) return fail(c, FLM_ERR_INVALID, "skinny gemm: 1 .. 16 tokens, one GPU");
    if ((double)g.rows * g.n * (EPI == EPI_SWIGLU ? 2 : 1) >= 2147483648.0 || skinny_lds_bytes(g.n, 1) > 64 * 1024) return fail(c, FLM_ERR_UNSUPPORTED, "skinny gemm: matrix of 2 GiB or more, or rows longer than 65536");
    const int cus = c ? c->cu_count : 256;
    if constexpr (EPI == EPI_SWIGLU) hipLaunchKernelGGL((k_gemm_q8_skinny<EPI_SWIGLU, 2>), dim3((g.rows + 15) / 16), dim3(64), skinny_lds_bytes(g.n, 2), st, g);
    else if (force_nb == 2 || (force_nb == 0 && (g.rows + 31) / 32 >= cus)) hipLaunchKernelGGL((k_gemm_q8_skinny<EPI, 2>), dim3((g.rows + 31) / 32), dim3(64), skinny_lds_bytes(g.n, 2), st, g);
    else hipLaunchKernelGGL((k_gemm_q8_skinny<EPI, 1>), dim3((g.rows + 15) / 16), dim3(64), skinny_lds_bytes(g.n, 1), st, g);
    HIPC(c, hipGetLastError());
    return FLM_OK;
}
// one GEMM of the batched path: the tiles, or -- int8, `skinny` (the verify pass under "spec_gemm" 1) -- the skinny kernel
template <int QT, int EPI>
int launch_gemm_any(flm_ctx* c, hipStream_t st, const GemmArgs& g, int use_mfma, bool skinny) {
    if constexpr (QT == QT_INT8) { if (skinny) return launch_gemm_skinny<EPI>(c, st, g); }
    return launch_gemm<QT, EPI>(c, st, g, use_mfma);
}

// k_attn_fan on the n rows of a fan step (flm_fan.h): queries per workgroup by what the LDS allows; c may be null (flm_op_attention_fan)
int launch_attn_fan(flm_ctx* c, hipStream_t st, const AttnArgs& aa, const FanDesc& f, int heads, int row_stride) {
    {   // a group's score rows and tiles can take most of the LDS: raise the kernel's dynamic-LDS limit, once per device
        static std::mutex mu; static bool done[64] = {false};
        int dev = 0; HIPC(c, hipGetDevice(&dev));
        std::lock_guard<std::mutex> lk(mu);
        if (dev >= 0 && dev < 64 && !done[dev]) {
            HIPC(c, hipFuncSetAttribute(reinterpret_cast<const void*>(&k_attn_fan), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsMax));
            done[dev] = true;
        }
    }
    if (aa.hs > 128 || aa.hs % 8 || f.n < 1 || f.n > kFanMax || f.S < 1 || f.t < 0 || f.S + f.t + 1 > aa.max_seq) return fail(c, FLM_ERR_INVALID, "attn_fan: head size <= 128, 1 .. 16 rows, S + t + 1 <= max_seq_len");
    for (int j = 0; j < f.n; ++j) if (f.base[j] < 0 || f.base[j] + f.t >= aa.max_seq) return fail(c, FLM_ERR_INVALID, "attn_fan: a tail row outside the cache");
    const int G = fan_group(aa.max_seq, aa.hs, kLdsMax);
    if (fan_lds_bytes(G, aa.max_seq, aa.hs) > kLdsMax) return fail(c, FLM_ERR_UNSUPPORTED, "attn_fan: one query's scores do not fit the LDS");
    hipLaunchKernelGGL(k_attn_fan, dim3(heads, (f.n + G - 1) / G), dim3(kAttnBlock), fan_lds_bytes(G, aa.max_seq, aa.hs), st, aa, f, row_stride, G);
    HIPC(c, hipGetLastError());
    return FLM_OK;
}
int launch_rope_kv_fan(flm_ctx* c, hipStream_t st, const float* qkv, float* qout, float* kcache, float* vcache, const float* rope_cos, const float* rope_sin, int dim, int hs, int kv_rows, const FanDesc& f) {
    hipLaunchKernelGGL(k_rope_kv_fan, dim3(f.n), dim3(256), 0, st, qkv, qout, kcache, vcache, rope_cos, rope_sin, dim, hs, kv_rows, f);
    HIPC(c, hipGetLastError());
    return FLM_OK;
}

// k_slot_views + k_attn_slots on the n live rows of a batch step (flm_batch.h): one workgroup per (head, row), the LDS of the largest slot; views: device memory for 16
// AttnArgs; c may be null (flm_op_attention_slots)
int launch_attn_slots(flm_ctx* c, hipStream_t st, const AttnArgs& aa, const SlotDesc& f, int heads, int row_stride, AttnArgs* views) {
    {   // a long slot's score row can take more than the default limit: raise the kernel's dynamic-LDS limit, once per device
        static std::mutex mu; static bool done[64] = {false};
        int dev = 0; HIPC(c, hipGetDevice(&dev));
        std::lock_guard<std::mutex> lk(mu);
        if (dev >= 0 && dev < 64 && !done[dev]) {
            HIPC(c, hipFuncSetAttribute(reinterpret_cast<const void*>(&k_attn_slots), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsMax));
            done[dev] = true;
        }
    }
    if (aa.hs > 256 || aa.hs % 8 || f.n < 1 || f.n > kBatchMax || aa.n_peer || !views) return fail(c, FLM_ERR_INVALID, "attn_slots: head size <= 256, 1 .. 16 rows, one GPU");
    int largest = 0;
    for (int r = 0; r < f.n; ++r) {
        if (f.base[r] < 0 || f.rows[r] < 1 || f.base[r] + f.rows[r] > aa.max_seq || f.pos[r] < 0 || f.pos[r] >= f.rows[r]) return fail(c, FLM_ERR_INVALID, "attn_slots: a row outside its slot, or a slot outside the cache");
        largest = f.rows[r] > largest ? f.rows[r] : largest;
    }
    if (attn_lds_bytes(largest, aa.hs) > kLdsMax) return fail(c, FLM_ERR_UNSUPPORTED, "attn_slots: one query's scores do not fit the LDS");
    hipLaunchKernelGGL(k_slot_views, dim3(1), dim3(64), 0, st, aa, f, views);
    HIPC(c, hipGetLastError());
    hipLaunchKernelGGL(k_attn_slots, dim3(heads, f.n), dim3(kAttnBlock), attn_lds_bytes(largest, aa.hs), st, (const AttnArgs*)views, f, row_stride);
    HIPC(c, hipGetLastError());
    return FLM_OK;
}
int launch_rope_kv_slots(flm_ctx* c, hipStream_t st, const float* qkv, float* qout, float* kcache, float* vcache, const float* rope_cos, const float* rope_sin, int dim, int hs, int kv_rows, const SlotDesc& f) {
    hipLaunchKernelGGL(k_rope_kv_slots, dim3(f.n), dim3(256), 0, st, qkv, qout, kcache, vcache, rope_cos, rope_sin, dim, hs, kv_rows, f);
    HIPC(c, hipGetLastError());
    return FLM_OK;
}

// A ragged pass's geometry (flm_segs.h), checked in front of the first launch (k_rope_kv_segs writes cache rows): the step rows first, one each; the prompt segments
// behind them in batch order, each inside its slot, the slots inside the cache, the rows adding up to B
const char* seg_check(const SegDesc& f, int B, int max_seq) {
    if (f.n_segs < 1 || f.n_segs > kBatchMax || f.n_step < 0 || f.n_step > f.n_segs) return "segs: 1 .. 16 segments, the step rows first";
    int at = 0;
    for (int s = 0; s < f.n_segs; ++s) {
        if (f.row0[s] != at || f.n[s] < 1 || (s < f.n_step && f.n[s] != 1)) return "segs: the segments' rows follow one another, a step segment has one row";
        if (f.base[s] < 0 || f.rows[s] < 1 || (long long)f.base[s] + f.rows[s] > max_seq) return "segs: a slot outside the cache";
        if (f.pos0[s] < 0 || (long long)f.pos0[s] + f.n[s] > f.rows[s]) return "segs: a segment outside its slot";
        if ((long long)at + f.n[s] > B) return "segs: the segments' rows do not add up to the batch";
        at += f.n[s];
    }
    return at == B ? nullptr : "segs: the segments' rows do not add up to the batch";
}
// k_seg_views + k_attn_segs_mq / k_attn_segs on the prompt segments of a ragged pass (flm_segs.h); the LDS of the largest slot among them
int launch_attn_segs(flm_ctx* c, hipStream_t st, const AttnArgs& aa, const SegDesc& f, int heads, int row_stride, AttnArgs* views, bool one_query) {
    {   // a long slot's score rows can take more than the default limit: raise the kernels' dynamic-LDS limit, once per device
        static std::mutex mu; static bool done[64] = {false};
        int dev = 0; HIPC(c, hipGetDevice(&dev));
        std::lock_guard<std::mutex> lk(mu);
        if (dev >= 0 && dev < 64 && !done[dev]) {
            HIPC(c, hipFuncSetAttribute(reinterpret_cast<const void*>(&k_attn_segs_mq), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsMax));
            HIPC(c, hipFuncSetAttribute(reinterpret_cast<const void*>(&k_attn_segs), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsMax));
            done[dev] = true;
        }
    }
    if (aa.hs > 256 || aa.hs % 8 || aa.n_peer || !views || f.n_step >= f.n_segs) return fail(c, FLM_ERR_INVALID, "attn_segs: head size <= 256, one GPU, at least one prompt segment");
    int largest = 0, groups = 0, P = 0;
    for (int s = f.n_step; s < f.n_segs; ++s) {
        largest = f.rows[s] > largest ? f.rows[s] : largest;
        groups += (f.n[s] + kMqQueries - 1) / kMqQueries; P += f.n[s];
    }
    hipLaunchKernelGGL(k_seg_views, dim3(1), dim3(64), 0, st, aa, f, row_stride, views);
    HIPC(c, hipGetLastError());
    if (!one_query && aa.hs <= 128 && attn_mq_lds_bytes(largest, aa.hs) <= kLdsMax)      // kMqQueries queries of one sequence per workgroup share every K / V tile
        hipLaunchKernelGGL(k_attn_segs_mq, dim3(heads, groups), dim3(kAttnBlock), attn_mq_lds_bytes(largest, aa.hs), st, (const AttnArgs*)views, f, row_stride);
    else {
        if (attn_lds_bytes(largest, aa.hs) > kLdsMax) return fail(c, FLM_ERR_UNSUPPORTED, "attn_segs: one query's scores do not fit the LDS");
        hipLaunchKernelGGL(k_attn_segs, dim3(heads, P), dim3(kAttnBlock), attn_lds_bytes(largest, aa.hs), st, (const AttnArgs*)views, f, row_stride);
    }
    HIPC(c, hipGetLastError());
    return FLM_OK;
}
int launch_rope_kv_segs(flm_ctx* c, hipStream_t st, const float* qkv, float* qout, float* kcache, float* vcache, const float* rope_cos, const float* rope_sin, int dim, int hs, int kv_rows, const SegDesc& f, int B) {
    const int P = B - (f.n_step < f.n_segs ? f.row0[f.n_step] : B);
    if (P < 1) return fail(c, FLM_ERR_INVALID, "rope_kv_segs: no prompt rows");
    hipLaunchKernelGGL(k_rope_kv_segs, dim3(P), dim3(256), 0, st, qkv, qout, kcache, vcache, rope_cos, rope_sin, dim, hs, kv_rows, f);
    HIPC(c, hipGetLastError());
    return FLM_OK;
}

// all_layers (flm_score_tokens): the last layer runs to its end as well -- pf_x then holds every row's final residual, the classifier's input
// fan (flm_generate_n; null: every launch is the one made without it): the B rows are the sequences of a fan step (flm_fan.h) -- `pos` is their one LOGICAL position, the
// QKV GEMM takes the plain-store route with k_rope_kv_fan behind it, the attention is k_attn_fan; everything else is a row's own and stays what it is
// row0 (flm_batch_join; 0: every launch is the one made without it): the batch is a prompt entering the cache slot whose region starts at physical row row0 -- the layer's
// cache pointers move by row0 rows for every kernel that writes or reads them, the attention's bound shrinks to what lies behind row0; `pos` stays the LOGICAL position
// slots (a flm_batch_step; null: as above): the B rows are the live slots' last ids, each at its own position in its own region -- the fan's route with k_rope_kv_slots and k_attn_slots
// segs (a flm_batch_pass; null: every launch is the one made without it): a ragged pass (flm_segs.h) -- rows [0, n_step) are a step's rows (`slots` describes them, null
// where n_step is 0) and keep the step's launches, the rest are prompt segments: k_rope_kv_segs and k_attn_segs_mq / k_attn_segs on the same q / out buffers
template <int QT>
int prefill_batched(flm_ctx* c, int B, int pos, bool all_layers, bool skinny_req = false, const FanDesc* fan = nullptr, int row0 = 0, const SlotDesc* slots = nullptr, const SegDesc* segs = nullptr) {
    const bool skinny = skinny_req && QT == QT_INT8 && B <= kSkinnyTokens && c->world == 1;      // (the verify pass; int16: the tiles)
    const auto& d = c->d;
    const int L = d.n_layers, dim = d.dim, hid = d.hidden_dim, hs = c->hs;
    hipStream_t st = c->stream;
    int r = B <= c->pf_cap ? FLM_OK : fail(c, FLM_ERR_INVALID, "prefill: more tokens than max_seq_len"); if (r) return r;
    const size_t kv_layer = (size_t)c->heads_local * c->kv_rows * hs;
    if (!c->st_ready) {   // once per set of weights: the scales group-major (no allocation: the copies' memory came with the matrices)
        for (auto& w : c->layers)
            for (QMat* m : {&w.qkv, &w.o, &w.w13, &w.w2}) {
                const size_t n = (size_t)m->rows * (m->cols / kGroup);
                hipLaunchKernelGGL(k_transpose_scales, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (const float*)m->s, m->st, m->rows, m->cols / kGroup);
            }
        HIPC(c, hipGetLastError());
        c->st_ready = true;
    }
    // Tensor parallel (peer-to-peer; the matrix-core kernels): this rank's heads / rows / hidden slice of every step, as in the decode path
    // (split_rows, transformer.cpp:264-287); the attention output, the residual stream and hd are full-width in every rank's exchange
    // region: the kernel that produces a column slice stores it into all of them, a flag round (k_xchg) closes the step, the row
    // prologues read with coherent loads.  Single GPU: dimL == dim, slices = everything, no peers.
    const bool tp = c->world > 1;
    const int dimL = c->dim_local, hidL = c->hidden_local, col_o = c->drow_begin, rows_o = c->drow_count, col_h = c->plan.hidden_begin, col_a = c->plan.head_begin * hs;
    auto peers = [&](GemmArgs& g, float* p) { g.n_peer = 0; if (tp) { const size_t off = (char*)p - c->xbuf; for (int r2 = 0; r2 < c->world; ++r2) if (r2 != c->rank) g.out_peer[g.n_peer++] = (float*)(c->peer[r2] + off); } };
    hipLaunchKernelGGL(k_embed_rows, dim3(B), dim3(256), 0, st, c->pf_x, (const void*)c->emb, (const float*)c->emb_s, c->emb_qt, dim, (const int*)c->prompt_dev);
    HIPC(c, hipGetLastError());
    for (int l = 0; l < L; ++l) {
        LayerW& w = c->layers[l];
        float* const kc = c->kcache + (size_t)l * kv_layer + (size_t)row0 * hs;    // (row0: the slot's origin; the stride between two heads' rows stays kv_rows)
        float* const vc = c->vcache + (size_t)l * kv_layer + (size_t)row0 * hs;
        // x2 = rmsnorm(x1); qx = quantize(x2); q,k,v = W x; RoPE; cache rows   (transformer.cpp:132-135, 386-395, 431-439)
        RowsArgs ra{c->pf_x, w.att_norm, c->pf_xq, c->pf_xs, dim, c->pf_xst};
        r = launch_rows<QT, PRO_RMSNORM_QUANT>(c, st, ra, B, tp); if (r) return r;
        GemmArgs g{w.qkv.q, w.qkv.s, c->pf_xq, c->pf_xs, c->pf_qkv, 3 * dimL, dim, 3 * dimL, B, c->pf_xst, w.qkv.st};
        if (fan) {
            r = launch_gemm_any<QT, EPI_STORE>(c, st, g, c->use_mfma, skinny); if (r) return r;
            r = launch_rope_kv_fan(c, st, c->pf_qkv, c->pf_q, kc, vc, c->rope_cos, c->rope_sin, dimL, hs, c->kv_rows, *fan); if (r) return r;
        }
        else if (segs) {
            r = launch_gemm_any<QT, EPI_STORE>(c, st, g, c->use_mfma, skinny); if (r) return r;
            if (segs->n_step > 0) { r = launch_rope_kv_slots(c, st, c->pf_qkv, c->pf_q, kc, vc, c->rope_cos, c->rope_sin, dimL, hs, c->kv_rows, *slots); if (r) return r; }
            if (segs->n_step < B) { r = launch_rope_kv_segs(c, st, c->pf_qkv, c->pf_q, kc, vc, c->rope_cos, c->rope_sin, dimL, hs, c->kv_rows, *segs, B); if (r) return r; }
        }
        else if (slots) {
            r = launch_gemm_any<QT, EPI_STORE>(c, st, g, c->use_mfma, skinny); if (r) return r;
            r = launch_rope_kv_slots(c, st, c->pf_qkv, c->pf_q, kc, vc, c->rope_cos, c->rope_sin, dimL, hs, c->kv_rows, *slots); if (r) return r;
        }
        else if ((QT == QT_INT16 || c->use_mfma || skinny) && dimL % 32 == 0 && hs % 2 == 0) {      // (int16: always the matrix-core tiles -- round 5: with the same epilogues as the int8 tiles)
            // RoPE and the cache rows as the epilogue of the matrix-core tiles: no [tokens][3 dim] round trip, no k_rope_kv_rows
            g.qout = c->pf_q; g.kcache = kc; g.vcache = vc;
            g.rope_cos = c->rope_cos; g.rope_sin = c->rope_sin; g.dim = dimL; g.hs = hs; g.max_seq = c->kv_rows /* (the stride between two heads' cache rows) */; g.pos0 = pos;
            r = launch_gemm_any<QT, EPI_ROPE_KV>(c, st, g, c->use_mfma, skinny); if (r) return r;
        } else {
            r = launch_gemm_any<QT, EPI_STORE>(c, st, g, c->use_mfma, skinny); if (r) return r;
            hipLaunchKernelGGL(k_rope_kv_rows, dim3(B), dim3(256), 0, st, (const float*)c->pf_qkv, c->pf_q, kc, vc,
                               (const float*)c->rope_cos, (const float*)c->rope_sin, dimL, hs, c->kv_rows, pos);
            HIPC(c, hipGetLastError());
        }
        if (l == L - 1 && !all_layers) break;             // the batch only has to fill the cache: nothing downstream of the last layer's K/V is needed
        // attention of every query over the cache rows 0 .. its own position   (execute_attn :441-449): the local heads' columns of att
        AttnArgs aa{}; aa.q = c->pf_q; aa.kcache = kc; aa.vcache = vc;
        aa.out = c->pf_att + col_a; aa.pos_ptr = &c->state->pos; aa.hs = hs; aa.max_seq = d.max_seq_len - row0; aa.kv_rows = c->kv_rows;
        if (tp) { const size_t off = (char*)aa.out - c->xbuf; for (int r2 = 0; r2 < c->world; ++r2) if (r2 != c->rank) aa.out_peer[aa.n_peer++] = (float*)(c->peer[r2] + off); }
        // which kernels: the exps of a tile of queries (weighted sum on the matrix cores) or the scores of 8 queries (VALU) must fit the LDS;
        // one query per workgroup needs 4 bytes per position and always fits (flm_ctx_create checked max_seq_len against it)
        const bool mq_fits = attn_mq_lds_bytes(d.max_seq_len, hs) <= kLdsMax;
        const bool pv_mfma = c->use_pv_mfma && (hs & 1) == 0;
        if (fan) { r = launch_attn_fan(c, st, aa, *fan, c->heads_local, dim); if (r) return r; }
        else if (segs) {
            if (segs->n_step > 0) { r = launch_attn_slots(c, st, aa, *slots, c->heads_local, dim, c->batch_views); if (r) return r; }
            if (segs->n_step < B) { r = launch_attn_segs(c, st, aa, *segs, c->heads_local, dim, c->seg_views, !c->use_prefill_mq); if (r) return r; }
        }
        else if (slots) { r = launch_attn_slots(c, st, aa, *slots, c->heads_local, dim, c->batch_views); if (r) return r; }
        else if (hs <= 128 && c->use_prefill_mq && c->use_qk_mfma && c->pf_scores && (pv_mfma || mq_fits)) {
            // scores on the matrix cores (fp32 MFMA = the reference's chains, bit for bit), then softmax + weighted sum per tile of queries
            aa.sc_global = c->pf_scores;
            const dim3 gq(c->heads_local, (B + kQkQ - 1) / kQkQ);
            switch (hs >> 5) {
            case 1: hipLaunchKernelGGL(k_qk_mfma<1>, gq, dim3(256), 0, st, aa, pos, dimL, B); break;
            case 2: hipLaunchKernelGGL(k_qk_mfma<2>, gq, dim3(256), 0, st, aa, pos, dimL, B); break;
            case 3: hipLaunchKernelGGL(k_qk_mfma<3>, gq, dim3(256), 0, st, aa, pos, dimL, B); break;
            default: hipLaunchKernelGGL(k_qk_mfma<4>, gq, dim3(256), 0, st, aa, pos, dimL, B); break;
            }
            HIPC(c, hipGetLastError());
            if (pv_mfma) {   // ... and the weighted sum too (an accumulator element = the reference's chain of one (query, dimension))
                const int qw = pv_mfma_queries(pos + B, kLdsMax);     // 16 queries per workgroup up to ~2500 positions, fewer beyond
                hipLaunchKernelGGL(k_attn_pv_mfma, dim3(c->heads_local, (B + qw - 1) / qw), dim3(256), pv_mfma_lds_bytes(pos + B, qw), st, aa, pos, dim, B, qw);
            } else
                hipLaunchKernelGGL(k_attn_prefill_mq<true>, dim3(c->heads_local, (B + kMqQueries - 1) / kMqQueries), dim3(kAttnBlock), attn_mq_lds_bytes(d.max_seq_len, hs), st, aa, pos, dim, B);
        }
        else if (hs <= 128 && c->use_prefill_mq && mq_fits)      // kMqQueries queries per workgroup share every K/V tile
            hipLaunchKernelGGL(k_attn_prefill_mq<false>, dim3(c->heads_local, (B + kMqQueries - 1) / kMqQueries), dim3(kAttnBlock), attn_mq_lds_bytes(d.max_seq_len, hs), st, aa, pos, dim, B);
        else
            hipLaunchKernelGGL(k_attn_prefill, dim3(c->heads_local, B), dim3(kAttnBlock), attn_lds_bytes(d.max_seq_len, hs), st, aa, pos, dim);
        HIPC(c, hipGetLastError());
        if (tp) { r = exchange(c, st, XK_ATT, nullptr, nullptr, 0); if (r) return r; }
        // x1 += Wo quantize(att)   (transformer.cpp:138-139, 457-466): this rank's rows of Wo = its columns of x1
        RowsArgs rq{c->pf_att, nullptr, c->pf_xq, c->pf_xs, dim, c->pf_xst};
        r = launch_rows<QT, PRO_QUANT>(c, st, rq, B, tp); if (r) return r;
        GemmArgs go{w.o.q, w.o.s, c->pf_xq, c->pf_xs, c->pf_x + col_o, dim, dim, rows_o, B, c->pf_xst, w.o.st};
        peers(go, go.out);
        r = launch_gemm_any<QT, EPI_RESIDUAL>(c, st, go, c->use_mfma, skinny); if (r) return r;
        if (tp) { r = exchange(c, st, XK_X1, nullptr, nullptr, 0); if (r) return r; }
        // hd = swiglu(W1 qx, W3 qx) with qx = quantize(rmsnorm(x1))   (transformer.cpp:144-147, 468-483): this rank's slice of hd
        RowsArgs rf{c->pf_x, w.ffn_norm, c->pf_xq, c->pf_xs, dim, c->pf_xst};
        r = launch_rows<QT, PRO_RMSNORM_QUANT>(c, st, rf, B, tp); if (r) return r;
        if (QT == QT_INT16 || skinny || (c->use_mfma && (tp || c->use_mfma == 3 || (c->use_mfma == 1 && ((hidL + 63) / 64) * ((B + 127) / 128) >= 256)))) {
            // 128 x 128 tiles of 64 gate + 64 up rows: the GEMM's epilogue is the SwiGLU
            GemmArgs g13{w.w13.q, w.w13.s, c->pf_xq, c->pf_xs, c->pf_hd + col_h, hid, dim, hidL, B, c->pf_xst, w.w13.st};
            peers(g13, g13.out);
            r = launch_gemm_any<QT, EPI_SWIGLU>(c, st, g13, c->use_mfma, skinny); if (r) return r;
        } else {
            GemmArgs g13{w.w13.q, w.w13.s, c->pf_xq, c->pf_xs, c->pf_gu, 2 * hidL, dim, 2 * hidL, B, c->pf_xst, w.w13.st};
            r = launch_gemm<QT, EPI_STORE>(c, st, g13, c->use_mfma); if (r) return r;
            SwigluPeers sp{}; { GemmArgs t{}; peers(t, c->pf_hd + col_h); sp.n = t.n_peer; for (int i = 0; i < t.n_peer; ++i) sp.p[i] = t.out_peer[i]; }
            hipLaunchKernelGGL(k_swiglu_rows, dim3(B), dim3(256), 0, st, c->pf_hd + col_h, (const float*)c->pf_gu, hidL, hid, sp);
            HIPC(c, hipGetLastError());
        }
        if (tp) { r = exchange(c, st, XK_HD, nullptr, nullptr, 0); if (r) return r; }
        // x1 += W2 quantize(hd)   (transformer.cpp:149-150, 485-494)
        RowsArgs rh{c->pf_hd, nullptr, c->pf_xq, c->pf_xs, hid, c->pf_xst};
        r = launch_rows<QT, PRO_QUANT>(c, st, rh, B, tp); if (r) return r;
        GemmArgs g2{w.w2.q, w.w2.s, c->pf_xq, c->pf_xs, c->pf_x + col_o, dim, hid, rows_o, B, c->pf_xst, w.w2.st};
        peers(g2, g2.out);
        r = launch_gemm_any<QT, EPI_RESIDUAL>(c, st, g2, c->use_mfma, skinny); if (r) return r;
        if (tp) { r = exchange(c, st, XK_X1, nullptr, nullptr, 0); if (r) return r; }
    }
    return FLM_OK;
}

int launch_gemm_store(flm_ctx* c, hipStream_t st, int qt, const GemmArgs& g, int use_mfma) {
    return qt == FLM_QT_INT8 ? launch_gemm<QT_INT8, EPI_STORE>(c, st, g, use_mfma) : launch_gemm<QT_INT16, EPI_STORE>(c, st, g, use_mfma);
}
int prefill_batched_qt(flm_ctx* c, int B, int pos, bool all_layers, bool skinny, const FanDesc* fan, int row0, const SlotDesc* slots, const SegDesc* segs) {
    if (segs) {   // (in front of the first launch: k_rope_kv_segs writes the rows' cache rows)
        if (c->world != 1 || fan || row0 || pos || B > c->pf_cap || (segs->n_step > 0) != (slots != nullptr) || (slots && slots->n != segs->n_step))
            return fail(c, FLM_ERR_INVALID, "prefill: a ragged pass is one GPU's, not a fan step, at row origin 0, within the batch buffers, its step rows described by a SlotDesc");
        if (const char* why = seg_check(*segs, B, c->d.max_seq_len)) return fail(c, FLM_ERR_INVALID, why);
        for (int r = 0; slots && r < slots->n; ++r)
            if (slots->base[r] != segs->base[r] || slots->rows[r] != segs->rows[r] || slots->pos[r] != segs->pos0[r]) return fail(c, FLM_ERR_INVALID, "prefill: a ragged pass's step rows and its SlotDesc disagree");
        return c->d.quant_type == FLM_QT_INT8 ? prefill_batched<QT_INT8>(c, B, 0, all_layers, skinny, nullptr, 0, slots, segs) : prefill_batched<QT_INT16>(c, B, 0, all_layers, skinny, nullptr, 0, slots, segs);
    }
    if (fan && (c->world != 1 || fan->n != B || pos != fan->S + fan->t)) return fail(c, FLM_ERR_INVALID, "prefill: a fan step is one GPU's batch of fan.n rows at S + t");
    if ((row0 || slots) && (c->world != 1 || fan || row0 < 0 || (slots && (row0 || slots->n != B)) || row0 + pos + (slots ? 0 : B) > c->d.max_seq_len))
        return fail(c, FLM_ERR_INVALID, "prefill: a slot's batch is one GPU's, inside the cache, and not a fan step");
    for (int r = 0; slots && r < slots->n; ++r)      // (in front of the first launch: k_rope_kv_slots writes the rows' cache rows)
        if (slots->n > kBatchMax || slots->base[r] < 0 || slots->rows[r] < 1 || slots->pos[r] < 0 || slots->pos[r] >= slots->rows[r] || (long long)slots->base[r] + slots->rows[r] > c->d.max_seq_len)
            return fail(c, FLM_ERR_INVALID, "prefill: a batch row outside its slot, or a slot outside the cache");
    return c->d.quant_type == FLM_QT_INT8 ? prefill_batched<QT_INT8>(c, B, pos, all_layers, skinny, fan, row0, slots) : prefill_batched<QT_INT16>(c, B, pos, all_layers, skinny, fan, row0, slots);
}
int launch_gemm_skinny_store(flm_ctx* c, hipStream_t st, const GemmArgs& g, int force_nb) { return launch_gemm_skinny<EPI_STORE>(c, st, g, force_nb); }

// ---------------------------------------------------------------------------------------------
// flm_score_tokens: the classifier for a chunk of the batch's rows.  The row prologue is the decode classifier's (rmsnorm with the output norm's weight, quantize), the tiles
// are the prompt path's with the plain store epilogue -- every (row, vocabulary entry) is the chain the token path's classifier GEMV runs -- and k_score_rows reads the staged
// logits.  The chunk is launched as a batch of its own (m rows): the group-major activation scales (pf_xst) are laid out by the launch's row count.
// ---------------------------------------------------------------------------------------------
int launch_score_rows(flm_ctx* c, hipStream_t st, const float* logits, int ld, int n, const int* targets, ScoreRow* out, int rows) {
    {   // a vocabulary's strip can take most of the LDS: raise the kernel's dynamic-LDS limit, once per device
        static std::mutex mu; static bool done[64] = {false};
        int dev = 0; HIPC(c, hipGetDevice(&dev));
        std::lock_guard<std::mutex> lk(mu);
        if (dev >= 0 && dev < 64 && !done[dev]) {
            HIPC(c, hipFuncSetAttribute(reinterpret_cast<const void*>(&k_score_rows), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsMax));
            done[dev] = true;
        }
    }
    const ScoreArgs a{logits, ld, n, targets, out};
    hipLaunchKernelGGL(k_score_rows, dim3(rows), dim3(kSampleBlock), score_lds_bytes(n), st, a);
    HIPC(c, hipGetLastError());
    return FLM_OK;
}
// k_sample_rows on `rows` rows of n logits, ld floats apart: batch rows row0 .. row0 + rows - 1 of a step whose state is `base` (flm_sample.h)
int launch_sample_rows(flm_ctx* c, hipStream_t st, const float* logits, int ld, int n, int row0, int rows, float temperature, float topp, unsigned long long base,
                       unsigned long long* sort_buf, int* out) {
    {   // the strip of a large vocabulary: the dynamic-LDS limit, once per device (flm_ctx_create raises it for the contexts' devices)
        static std::mutex mu; static bool done[64] = {false};
        int dev = 0; HIPC(c, hipGetDevice(&dev));
        std::lock_guard<std::mutex> lk(mu);
        if (dev >= 0 && dev < 64 && !done[dev]) {
            HIPC(c, hipFuncSetAttribute(reinterpret_cast<const void*>(&k_sample_rows), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsMax));
            done[dev] = true;
        }
    }
    if (rows < 1 || row0 < 0 || row0 + rows > kSpecRows) return fail(c, FLM_ERR_INVALID, "sample_rows: rows outside a batch of 16");
    hipLaunchKernelGGL(k_sample_rows, dim3(rows), dim3(kSampleBlock), sample_lds_bytes(n), st, logits, ld, n, row0, temperature, topp, base, sort_buf, out);
    HIPC(c, hipGetLastError());
    return FLM_OK;
}
int launch_entropy_rows(flm_ctx* c, hipStream_t st, const EntropyRowsArgs& a, int rows) {
    {   // the strip of a large vocabulary: the dynamic-LDS limit, once per device
        static std::mutex mu; static bool done[64] = {false};
        int dev = 0; HIPC(c, hipGetDevice(&dev));
        std::lock_guard<std::mutex> lk(mu);
        if (dev >= 0 && dev < 64 && !done[dev]) {
            HIPC(c, hipFuncSetAttribute(reinterpret_cast<const void*>(&k_entropy_rows), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsMax));
            done[dev] = true;
        }
    }
    if (rows < 1 || rows > kSpecRows) return fail(c, FLM_ERR_INVALID, "entropy_rows: rows outside a batch of 16");
    if (a.n < 2 || a.ld < a.n || sample_lds_bytes(a.n) > kLdsMax) return fail(c, FLM_ERR_UNSUPPORTED, "entropy_rows: the row does not fit one workgroup's LDS strip");
    hipLaunchKernelGGL(k_entropy_rows, dim3(rows), dim3(kSampleBlock), sample_lds_bytes(a.n), st, a);
    HIPC(c, hipGetLastError());
    return FLM_OK;
}
int launch_shape_rows(flm_ctx* c, hipStream_t st, const float* logits, int ld, float* out, int ld_out, int n, int row0, int rows, const ShapeParams* p,
                      const int* win, int n_win, const int* drafts, const DfaBlock* dfa, int cstate, int* states_out) {
    if (rows < 1 || row0 < 0 || row0 + rows > kSpecRows) return fail(c, FLM_ERR_INVALID, "shape_rows: rows outside a batch of 16");
    const ShapeRowsArgs a{logits, ld, out, ld_out, n, row0, p, win, n_win, drafts, dfa, dfa ? cstate : -1, states_out};
    hipLaunchKernelGGL(k_shape_rows, dim3(rows), dim3(kSampleBlock), 0, st, a);
    HIPC(c, hipGetLastError());
    return FLM_OK;
}
int launch_logprob_rows(flm_ctx* c, hipStream_t st, const float* rows_dev, int ld, int n, int row0, int rows, const int* chosen, int top_n, LogprobRec* rec, int rec_base, int rec_cap) {
    {   // the strip of a large vocabulary: the dynamic-LDS limit, once per device
        static std::mutex mu; static bool done[64] = {false};
        int dev = 0; HIPC(c, hipGetDevice(&dev));
        std::lock_guard<std::mutex> lk(mu);
        if (dev >= 0 && dev < 64 && !done[dev]) {
            HIPC(c, hipFuncSetAttribute(reinterpret_cast<const void*>(&k_logprob_rows), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsMax));
            done[dev] = true;
        }
    }
    if (rows < 1 || row0 < 0 || row0 + rows > kSpecRows || top_n < 0 || top_n > kLogprobsMax || !rec) return fail(c, FLM_ERR_INVALID, "logprob_rows: rows outside a batch of 16, or top_n outside [0, 20]");
    if (n < 2 || sample_lds_bytes(n) > kLdsMax) return fail(c, FLM_ERR_UNSUPPORTED, "logprob_rows: the row does not fit one workgroup's LDS strip");
    const LogprobRowsArgs a{rows_dev, ld, n, row0, chosen, top_n, rec, rec_base, rec_cap};
    hipLaunchKernelGGL(k_logprob_rows, dim3(rows), dim3(kSampleBlock), logprob_lds_bytes(n), st, a);
    HIPC(c, hipGetLastError());
    return FLM_OK;
}
// the classifier on rows [row0, row0 + m) of the batch's final residual: `stage` [m][vocab] receives their logits
template <int QT>
static int classify_rows_t(flm_ctx* c, int row0, int m, float* stage, bool skinny) {
    const int dim = c->d.dim, V = c->d.vocab_size;
    hipStream_t st = c->stream;
    if (!c->cls_st_ready) {   // once per set of weights, like the layers' copies (no allocation: cls.st came with the matrix)
        const size_t n = (size_t)c->cls.rows * (c->cls.cols / kGroup);
        hipLaunchKernelGGL(k_transpose_scales, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (const float*)c->cls.s, c->cls.st, c->cls.rows, c->cls.cols / kGroup);
        HIPC(c, hipGetLastError());
        c->cls_st_ready = true;
    }
    // logits = Wcls quantize(rmsnorm(x1))   (transformer.cpp:154-160)
    RowsArgs ra{c->pf_x + (size_t)row0 * dim, c->out_norm, c->pf_xq, c->pf_xs, dim, c->pf_xst};
    int r = launch_rows<QT, PRO_RMSNORM_QUANT>(c, st, ra, m); if (r) return r;
    GemmArgs g{c->cls.q, c->cls.s, c->pf_xq, c->pf_xs, stage, V, dim, V, m, c->pf_xst, c->cls.st};
    return launch_gemm_any<QT, EPI_STORE>(c, st, g, c->use_mfma, skinny && m <= kSkinnyTokens);
}
template <int QT>
static int score_classify_t(flm_ctx* c, int row0, int m, float* stage, bool skinny, int* argmax_out, const SpecDraw* draw = nullptr) {
    const int V = c->d.vocab_size;
    hipStream_t st = c->stream;
    int r = classify_rows_t<QT>(c, row0, m, stage, skinny); if (r) return r;
    if (argmax_out) {
        const bool lp = draw && draw->lp_top_n >= 0;          // the context is armed for log-probabilities: a record per row behind the draws (flm_logprob.h)
        float* rows = stage;                                  // what the draw reads
        if (draw && draw->shape) {                            // a control is set: the chunk's rows shaped, each over its own window, in front of the draw -- in place, or into
            if (lp && draw->lp_source == 0) {                 // the side rows where the records want the RAW rows (shape_row copies when S != L); m <= 16: a batch's rows
                if (m > kSpecRows || !c->lp_side) return fail(c, FLM_ERR_INVALID, "logprobs: a verify chunk of more than 16 rows");
                rows = c->lp_side;
            }
            r = launch_shape_rows(c, st, stage, V, rows, V, V, row0, m, draw->shape, draw->win, draw->n_win, c->prompt_dev + 1, c->dfa_blk, draw->cstate); if (r) return r;
        }
        if (draw && draw->temperature != 0.0f && typical_on(draw->typical_p)) {   // flm_entropy_set, typical: stage 5 on every row, in place (a function of the row alone)
            EntropyRowsArgs ea{}; ea.rows = rows; ea.ld = V; ea.n = V; ea.temp = draw->temperature; ea.typical_p = draw->typical_p; ea.sort_buf = c->sort_buf;
            r = launch_entropy_rows(c, st, ea, m); if (r) return r;
        }
        if (draw && draw->temperature != 0.0f) {              // the sampled verify pass: row row0 + i drawn with the (row0 + i + 1)-th coin of the step's state
            r = launch_sample_rows(c, st, rows, V, V, row0, m, draw->temperature, draw->topp, draw->base, c->sort_buf, argmax_out); if (r) return r;
        } else {   // the verify pass: the rows' first maxima only (no softmax, no sum chain, no LDS strip: any vocabulary)
            hipLaunchKernelGGL(k_argmax_rows, dim3(m), dim3(kSampleBlock), 0, st, (const float*)rows, V, V, argmax_out + row0);
            HIPC(c, hipGetLastError());
        }
        if (lp) return launch_logprob_rows(c, st, draw->lp_source ? rows : stage, V, V, row0, m, argmax_out, draw->lp_top_n, c->lp_rec, draw->lp_base, c->d.max_seq_len);
        return FLM_OK;
    }
    return launch_score_rows(c, st, stage, V, V, c->score_tgt + row0, c->score_dev + row0, m);
}
int score_classify(flm_ctx* c, int row0, int m, float* stage) {
    return c->d.quant_type == FLM_QT_INT8 ? score_classify_t<QT_INT8>(c, row0, m, stage, false, nullptr) : score_classify_t<QT_INT16>(c, row0, m, stage, false, nullptr);
}
// k_sample_fan on `rows` rows of n logits, ld floats apart (0: all from one row), batch rows row0 ..; sort_buf [16][2][n] (c may be null)
int launch_sample_fan(flm_ctx* c, hipStream_t st, const float* logits, int ld, int n, int row0, int rows, float temperature, float topp, const FanIn& in,
                      unsigned long long* sort_buf, int* drawn, unsigned long long* after) {
    {   // the strip of a large vocabulary: the dynamic-LDS limit, once per device
        static std::mutex mu; static bool done[64] = {false};
        int dev = 0; HIPC(c, hipGetDevice(&dev));
        std::lock_guard<std::mutex> lk(mu);
        if (dev >= 0 && dev < 64 && !done[dev]) {
            HIPC(c, hipFuncSetAttribute(reinterpret_cast<const void*>(&k_sample_fan), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsMax));
            done[dev] = true;
        }
    }
    if (rows < 1 || row0 < 0 || row0 + rows > kFanMax) return fail(c, FLM_ERR_INVALID, "sample_fan: rows outside a batch of 16");
    if (temperature != 0.0f && (n < 2 || sample_lds_bytes(n) > kLdsMax || !sort_buf)) return fail(c, FLM_ERR_UNSUPPORTED, "sample_fan: the row does not fit one workgroup's LDS strip");
    hipLaunchKernelGGL(k_sample_fan, dim3(rows), dim3(kSampleBlock), temperature != 0.0f ? sample_lds_bytes(n) : 2 * kSampleWaves * sizeof(int), st, logits, ld, n, row0, temperature, topp, in, sort_buf, drawn, after);
    HIPC(c, hipGetLastError());
    return FLM_OK;
}
// a fan step's classifier stage: the chunk through score_classify's prologue and GEMM, then k_sample_fan -- every row with its own state
int fan_classify(flm_ctx* c, int row0, int m, float* stage, bool skinny, float temperature, float topp, const FanIn& in) {
    const int V = c->d.vocab_size;
    int r = c->d.quant_type == FLM_QT_INT8 ? classify_rows_t<QT_INT8>(c, row0, m, stage, skinny) : classify_rows_t<QT_INT16>(c, row0, m, stage, false); if (r) return r;
    return launch_sample_fan(c, c->stream, stage, V, V, row0, m, temperature, topp, in, c->sort_buf, c->fan_drawn, c->fan_after);
}
// k_sample_slots on `rows` rows of n logits, ld floats apart, batch rows row0 ..; sort_buf [16][2][n] (needed where a row of the chunk is sampled)
int launch_sample_slots(flm_ctx* c, hipStream_t st, const float* logits, int ld, int n, int row0, int rows, const SlotIn& in, unsigned long long* sort_buf, int* drawn, unsigned long long* after) {
    {   // the strip of a large vocabulary: the dynamic-LDS limit, once per device
        static std::mutex mu; static bool done[64] = {false};
        int dev = 0; HIPC(c, hipGetDevice(&dev));
        std::lock_guard<std::mutex> lk(mu);
        if (dev >= 0 && dev < 64 && !done[dev]) {
            HIPC(c, hipFuncSetAttribute(reinterpret_cast<const void*>(&k_sample_slots), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsMax));
            done[dev] = true;
        }
    }
    if (rows < 1 || row0 < 0 || row0 + rows > kBatchMax) return fail(c, FLM_ERR_INVALID, "sample_slots: rows outside a batch of 16");
    bool sampled = false;
    for (int r = row0; r < row0 + rows; ++r) sampled = sampled || in.temp[r] != 0.0f;
    if (sampled && (n < 2 || sample_lds_bytes(n) > kLdsMax || !sort_buf)) return fail(c, FLM_ERR_UNSUPPORTED, "sample_slots: the row does not fit one workgroup's LDS strip");
    hipLaunchKernelGGL(k_sample_slots, dim3(rows), dim3(kSampleBlock), sampled ? sample_lds_bytes(n) : 2 * kSampleWaves * sizeof(int), st, logits, ld, n, row0, in, sort_buf, drawn, after);
    HIPC(c, hipGetLastError());
    return FLM_OK;
}
// a batch step's classifier stage, or a join's (src_row0: the batch row the chunk starts at; row0: the SlotIn row its first draw belongs to): the chunk through
// score_classify's prologue and GEMM, then k_sample_slots -- every row with its own parameters and state
int batch_classify(flm_ctx* c, int src_row0, int row0, int m, float* stage, bool skinny, const SlotIn& in) {
    const int V = c->d.vocab_size;
    int r = c->d.quant_type == FLM_QT_INT8 ? classify_rows_t<QT_INT8>(c, src_row0, m, stage, skinny) : classify_rows_t<QT_INT16>(c, src_row0, m, stage, false); if (r) return r;
    return launch_sample_slots(c, c->stream, stage, V, V, row0, m, in, c->sort_buf, c->fan_drawn, c->fan_after);
}
// the verify pass's classifier stage: the same chunk through the same prologue and GEMM (skinny: k_gemm_q8_skinny, int8), then k_argmax_rows into argmax_out[row0 ..]
// (draw given and its temperature > 0: k_sample_rows in place of k_argmax_rows)
int spec_classify(flm_ctx* c, int row0, int m, float* stage, bool skinny, int* argmax_out, const SpecDraw& draw) {
    return c->d.quant_type == FLM_QT_INT8 ? score_classify_t<QT_INT8>(c, row0, m, stage, skinny, argmax_out, &draw) : score_classify_t<QT_INT16>(c, row0, m, stage, false, argmax_out, &draw);
}

} // namespace fh
