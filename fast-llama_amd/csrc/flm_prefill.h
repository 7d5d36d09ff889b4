// flm_prefill.h -- batched prompt processing: row prologues, int8/int16 GEMM tiles (MFMA / v_dot), RoPE + KV rows, SwiGLU rows.
// Part of flm_kernels.h (hand-written gfx950 / CDNA4 kernels of the fast-llama per-token hot path); include that header.
#pragma once
#include "flm_math.h"
#include "flm_gemv.h"
// (bit-exactness hygiene: see flm_math.h -- no implicit FMA contraction in any of these headers)
#pragma clang fp contract(off)

namespace flm {

// ------------------------------------------------------------------------------------------
// Batched prefill (ParallelTransformer::forward with bs > 1, transformer.cpp:105-161).  A prompt's tokens before the
// last one only have to leave their K/V rows in the cache; every (token, row) value is produced by the SAME chain as in
// the single-token kernels (group dots exact, acc = fma(sW*sX, float(dot), acc) with groups ascending; per-row rmsnorm
// chains; per-query attention), so the cache -- and therefore the logits of the last token, which runs through the
// decode kernels -- is bit-identical to feeding the prompt token by token, at a fraction of the time: the weights are
// streamed once per 64 tokens instead of once per token.
//   k_embed_rows        x[b] = embedding[token b]
//   k_rows_prologue     per token row: (rmsnorm,) quantize -> xq[b], xs[b]   (the decode prologue, one workgroup per row)
//   (k_gemm_q, the v_dot4 / v_dot2 tile kernel of round 1, is gone: 256 VGPRs, reachable only through "use_mfma" 0, 3-6x slower than the matrix-core
//    tiles that replaced it; "use_mfma" 0 now selects the 64 x 64 matrix-core tiles)
//   k_rope_kv_rows      RoPE on q and k of every token, K/V rows appended to the cache
//   k_attn_prefill      causal attention: one workgroup per (head, query), the decode attention with T = pos + i + 1
//   k_swiglu_rows       hd[b] = swiglu(gate[b], up[b])
// ------------------------------------------------------------------------------------------
inline __global__ void k_embed_rows(float* x, const void* emb, const float* emb_s, int emb_qt, int dim, const int* tokens) {
    const int tok = tokens[blockIdx.x];
    float* xo = x + (size_t)blockIdx.x * dim;
    for (int e = threadIdx.x; e < dim; e += blockDim.x) {
        float v;
        if (emb_qt == 0) v = reinterpret_cast<const float*>(emb)[(size_t)tok * dim + e];
        else {
            const float s = emb_s[((size_t)tok * dim + e) / kGroup];
            const int q = emb_qt == QT_INT8 ? (int)reinterpret_cast<const int8_t*>(emb)[(size_t)tok * dim + e]
                                            : (int)reinterpret_cast<const int16_t*>(emb)[(size_t)tok * dim + e];
            v = __fmul_rn((float)q, s);                              // dequantize_ quant_operators.cpp:49-65
        }
        xo[e] = v;
    }
}

struct RowsArgs {
    const float* x;          // [B][n]
    const float* norm_w;     // [n] (RMSNORM_QUANT)
    void* xq; float* xs;     // [B][n] quantized, [B][n/64] scales
    int n;
    float* xst;              // the scales once more, group-major [n/64][B] (the matrix-core GEMM tiles read 64 tokens' scales of a group as one 256-byte run); may be null
};
// COH: the rows were (partly) written by peer GPUs (tensor parallel: the exchange regions) -> system-coherent loads
template <int QT, int PRO, int XR, bool COH = false>
__global__ void __launch_bounds__(kGemvBlock) k_rows_prologue(const RowsArgs r) {
    using T = QTraits<QT>;
    extern __shared__ __attribute__((aligned(16))) char lds[];
    GemvArgs a{};
    a.n = r.n; a.x = r.x + (size_t)blockIdx.x * r.n; a.norm_w = r.norm_w;
    a.rows_per_pass = 4; a.cb_shift = 4;                                     // (only the fixed LDS offsets are used)
    float4 xv[XR > 0 ? XR : 1], nv[XR > 0 ? XR : 1];
    gemv_preload<QT, PRO, XR, COH>(a, xv, nv);
    gemv_prologue<QT, PRO, XR, COH>(a, lds, xv, nv, [](int) {});
    const GemvLds L = gemv_lds_layout(r.n, T::kEsz, true, 4, 4, false);
    const int nb16 = r.n * T::kEsz / 16, sn = r.n / kGroup;
    int4* qo = reinterpret_cast<int4*>(reinterpret_cast<char*>(r.xq) + (size_t)blockIdx.x * r.n * T::kEsz);
    for (int c = threadIdx.x; c < nb16; c += kGemvBlock) qo[c] = reinterpret_cast<const int4*>(lds)[c];
    const float* xs = reinterpret_cast<const float*>(lds + L.off_xs);
    for (int g = threadIdx.x; g < sn; g += kGemvBlock) { r.xs[(size_t)blockIdx.x * sn + g] = xs[g]; if (r.xst) r.xst[(size_t)g * gridDim.x + blockIdx.x] = xs[g]; }
}

struct GemmArgs {
    const void* W; const float* sW;      // [rows][n], [rows][n/64]
    const void* Xq; const float* Xs;     // [B][n], [B][n/64]
    float* out; int ldo;                 // out[b * ldo + row]
    int n, rows, B;
    const float* XsT;                    // Xs group-major, [n/64][B] (the matrix-core kernels)
    const float* sWT;                    // sW group-major, [n/64][rows] (the matrix-core kernels; SWIGLU: [n/64][2 rows])
    // EPI_ROPE_KV (the qkv GEMM of k_gemm_q8_mfma): rows [0, dim) = q, [dim, 2 dim) = k, [2 dim, 3 dim) = v of token b at position pos0 + b;
    // RoPE on q and k (rope_v2 pairs), q -> qout[b][dim], k / v -> the layer's cache rows (what k_rope_kv_rows does after a plain store)
    float* qout; float* kcache; float* vcache; const float* rope_cos; const float* rope_sin; int dim, hs, max_seq, pos0;
    // tensor parallel, peer-to-peer (EPI_RESIDUAL / EPI_SWIGLU of k_gemm_q8_mfma): `out` lies in this rank's exchange region (its old value
    // is read coherently) and every result also goes to the same place of every peer's region (system-scope stores), as GemvArgs::out_peer
    float* out_peer[7]; int n_peer;
};
// a result of a batched kernel that the other ranks need: local write-through store + one system-scope store per peer
__device__ __forceinline__ void st_result_tp(float* o, const size_t idx, const float v, float* const (&peer)[7], const int n_peer) {
    if (n_peer == 0) { o[idx] = v; return; }
    st_agent(o + idx, v);
    for (int i = 0; i < n_peer; ++i) __hip_atomic_store(peer[i] + idx, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
// the group-major copy of a weight matrix's scales (made once, when the first prompt is batched)
inline __global__ void k_transpose_scales(const float* s, float* st, int rows, int sn) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < (size_t)rows * sn) { const int r = (int)(i / sn), g = (int)(i - (size_t)r * sn); st[(size_t)g * rows + r] = s[i]; }
}
// The epilogue of the int8 matrix-core GEMMs (k_gemm_q8_mfma, k_gemm_q8_ring): a wave holds acc[j][i] = the finished chain of
// (token tb + (i & 3) + 8 (i >> 2) + 4 (lane >> 5), row rbase + 32 j) -- SWIGLU: j = 0 gate, j = 1 up of the SAME row rbase -- with rbase = the
// lane's row (lane & 31 inside a 32-row fragment).  Store | residual add | SwiGLU | RoPE + KV rows.
template <int EPI, int NB>
__device__ __forceinline__ void gemm_epilogue(const GemmArgs& a, const float (&acc)[NB][16], const int rbase, const int tb, const int lane) {
    constexpr bool TWO = EPI == EPI_SWIGLU;
    const int h = lane >> 5;
    if constexpr (EPI == EPI_ROPE_KV) {
        // a fragment's 32 rows lie inside one of q / k / v (dim is a multiple of 32) and a RoPE pair (rows 2i, 2i + 1) in neighbouring lanes
#pragma unroll
        for (int j = 0; j < NB; ++j) {
            const int row = rbase + j * 32, which = row / a.dim, within = row - which * a.dim, hh = within / a.hs, dd = within - hh * a.hs;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int b = tb + (i & 3) + 8 * (i >> 2) + 4 * h, pos = a.pos0 + b;
                const float mine = acc[j][i], other = __shfl_xor(mine, 1, 64);
                if (row >= a.rows || b >= a.B) continue;
                float v = mine;
                if (which < 2) {
                    const float c = a.rope_cos[(size_t)pos * (a.hs / 2) + dd / 2], sn_ = a.rope_sin[(size_t)pos * (a.hs / 2) + dd / 2];
                    float o0, o1;
                    rope_pair((lane & 1) ? other : mine, (lane & 1) ? mine : other, c, sn_, o0, o1);
                    v = (lane & 1) ? o1 : o0;
                }
                if (which == 0) a.qout[(size_t)b * a.dim + within] = v;
                else (which == 1 ? a.kcache : a.vcache)[((size_t)hh * a.max_seq + pos) * a.hs + dd] = v;
            }
        }
    } else if constexpr (TWO) {
        const int row = rbase;
        if (row < a.rows) {
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int b = tb + (i & 3) + 8 * (i >> 2) + 4 * h;
                if (b < a.B) st_result_tp(a.out, (size_t)b * a.ldo + row, swiglu_elem(acc[0][i], acc[NB - 1][i]), a.out_peer, a.n_peer);
            }
        }
    } else {
#pragma unroll
        for (int j = 0; j < NB; ++j) {
            const int row = rbase + j * 32;
            if (row >= a.rows) continue;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int b = tb + (i & 3) + 8 * (i >> 2) + 4 * h;
                if (b >= a.B) continue;
                const size_t idx = (size_t)b * a.ldo + row;
                if constexpr (EPI == EPI_RESIDUAL) st_result_tp(a.out, idx, __fadd_rn(a.n_peer ? ld_agent(a.out + idx) : a.out[idx], acc[j][i]), a.out_peer, a.n_peer);
                else a.out[idx] = acc[j][i];
            }
        }
    }
}
// The int8 GEMM on the matrix cores (gfx950 v_mfma_i32_32x32x32_i8): a 64 x 64 (rows x tokens) workgroup tile, four waves each owning
// 32 tokens x 32 weight rows.  Per quant group two MFMAs (K = 2 x 32) accumulate the group's 1024 int32 dots exactly (integer sums
// are order-free; A and B use the same byte -> k assignment: lane half h takes bytes 32kk + 16h .. +15 of the group); then every
// lane applies the reference's fp32 chain step to its 16 results: v_cvt, v_mul, v_fma per output -- 48 VALU instructions per group
// against 2 MFMAs, so the VALU (and the LDS that feeds it), not the matrix pipe, bounds the kernel.
// A STAGE is kGPS = 2 consecutive quant groups (128 bytes of every row): one barrier and one pair of LDS buffers per stage.  Inside a
// stage the groups are consumed in ascending order: the chain is the reference's.
// Shaped by the counters (profiles/r02_prefill_gemm_pmc.txt): a first version held 190 registers (124 + 64 accumulation registers
// the compiler parked the MFMA results in, one v_accvgpr_read per element to get them back), so two waves shared a SIMD -- and a
// wave issues a VALU instruction every ~6.5 cycles at best (tools/ubench/valu_rate.hip: 1.4-1.9 cycles per instruction need four
// waves per SIMD; scalar fp32 forms overlap the MFMAs completely, packed forms do not): the SIMDs idled 2/3 of the time.
// Here: <= 128 registers (four waves per SIMD, MFMA results in plain VGPRs), one register slot of prefetch, tokens as the MFMA's
// A operand so that a lane owns ONE weight row (one weight scale per lane and group, coalesced stores: 32 lanes = 128 contiguous
// bytes of an output row), one scale load per thread and stage, five adds of address arithmetic per stage.
// C/D layout: col = lane & 31 (weight row), row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5) (token).
typedef int v16i __attribute__((ext_vector_type(16)));
constexpr int kGPS = 2;
// Tile shapes: WT x WR waves, a wave = 32 tokens x (NB x 32) weight rows (NB fragments of the B operand share one A fragment and
// one set of activation scales).  <2, 2, 1>: 64 tokens x 64 rows, 256 threads, four workgroups per CU.  <4, 2, 2>: 128 x 128, 512
// threads, two per CU: per 32 x 32 x 64 products the LDS moves 36 instead of 62 cycles' worth (operand reads 12 / 16, scale reads
// 10 / 18, stores of the staged tiles 13 / 28) and half the bytes come through the CU's memory pipeline -- and the LDS is what
// bounds the kernel (removing the chain altogether changed nothing, removing the staging stores and loads halved the time:
// profiles/r02_prefill_gemm_pmc.txt).
template <int WT, int WR, int NB>
struct GemmTile {
    static constexpr int TT = 32 * WT, TR = 32 * NB * WR, NT = 64 * WT * WR;
    static constexpr int SB = kGPS * kGroup;      // bytes of a stage in one row
    static constexpr int LS = SB + 16;            // LDS row stride (conflict-free 16-byte reads of 16 consecutive rows)
    static constexpr int kOffX = TR * LS, kOffS = (TR + TT) * LS, kBuf = kOffS + kGPS * (TR + TT) * 4;   // W rows | X rows | scales [W g0][W g1][X g0][X g1]
    static constexpr int NPW = TR * 8 / NT, NPX = TT * 8 / NT;      // 16-byte pieces per thread and stage
    static constexpr int kLds = 2 * kBuf;
    static_assert(kGPS == 2 && NT == kGPS * (TR + TT) && TR % 64 == 0 && TT % 64 == 0, "one scale per thread and stage, wave-uniform (matrix, group)");
    static_assert(TR * 8 % NT == 0 && TT * 8 % NT == 0, "whole pieces per thread");
};
// EPI_SWIGLU (NB == 2): W = [W1 (gate) ; W3 (up)], a.rows rows each; a tile's rows are TR / 2 rows of W1 and the same rows of W3, a
// wave's two B fragments the same 32 rows of both -- gate and up of one (token, row) meet in one lane, and the epilogue stores
// swiglu(gate, up) (o1.swiglu(o3), transformer.cpp:481) instead of both: no [tokens][2 hidden] round trip, no k_swiglu_rows.
template <int EPI, int WT, int WR, int NB>
__global__ void __launch_bounds__(64 * WT * WR, 4) k_gemm_q8_mfma(const GemmArgs a) {
    using G = GemmTile<WT, WR, NB>;
    constexpr bool TWO = EPI == EPI_SWIGLU;
    static_assert(!TWO || NB == 2, "gate and up are the two B fragments of a wave");
    constexpr int TRH = TWO ? G::TR / 2 : G::TR;              // rows of a.rows one tile advances
    constexpr int SB = G::SB, LS = G::LS, TT = G::TT, TR = G::TR, NT = G::NT, kOffX = G::kOffX, kOffS = G::kOffS, kBuf = G::kBuf, NPW = G::NPW, NPX = G::NPX;
    extern __shared__ __attribute__((aligned(16))) char lds[]; char* const sm = lds;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int ntt = (a.B + TT - 1) / TT;
    const int nb = gridDim.x, per = nb >> 3, rem = nb & 7, xcd = blockIdx.x & 7;              // tiles dealt to the XCDs in contiguous runs (token tile fastest: the tiles that share 64 weight rows are neighbours in the LOGICAL order, and workgroup b runs on XCD b mod 8 with its own L2: weight rows are fetched from HBM once per XCD instead of once per token tile)
    const int tile = xcd * per + (xcd < rem ? xcd : rem) + (blockIdx.x >> 3);
    const int r0 = (tile / ntt) * TRH, b0 = (tile % ntt) * TT;
    const int sn = a.n / kGroup, nst = (sn + kGPS - 1) / kGPS;
    const unsigned rowbytes = (unsigned)a.n;
    constexpr unsigned kOOB = 0x80000000u;
    const __amdgpu_buffer_rsrc_t rW = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(a.W), 0, (int)((TWO ? 2u : 1u) * (unsigned)a.rows * rowbytes), 0x00020000);
    // tile row -> row of W (or kOOB-marker -1): SWIGLU tiles hold TRH rows of W1, then the same TRH rows of W3
    auto wrow = [&](int tr) -> int { const int within = TWO ? tr % TRH : tr, r = r0 + within; return r < a.rows ? (TWO ? (tr / TRH) * a.rows + r : r) : -1; };
    const __amdgpu_buffer_rsrc_t rX = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(a.Xq), 0, (int)((unsigned)a.B * rowbytes), 0x00020000);
    // loader: piece k of a thread = 16 bytes at (row (tid >> 3) + (NT / 8) k, chunk tid & 7); rows outside a matrix read as zero
    const int prow = tid >> 3, pch = tid & 7;
    unsigned woff[NPW], xoff[NPX];
#pragma unroll
    for (int k = 0; k < NPW; ++k) { const int r = wrow(prow + (NT / 8) * k); woff[k] = r >= 0 ? (unsigned)r * rowbytes + pch * 16 : kOOB; }
#pragma unroll
    for (int k = 0; k < NPX; ++k) xoff[k] = (b0 + prow + (NT / 8) * k < a.B) ? (unsigned)(b0 + prow + (NT / 8) * k) * rowbytes + pch * 16 : kOOB;
    const unsigned poff = (unsigned)(prow * LS + pch * 16);
    // scales: one per thread and stage, LDS slots [W g0 (TR)][W g1 (TR)][X g0 (TT)][X g1 (TT)]; (matrix, group) is the same for a whole
    // wave.  They come from GROUP-MAJOR copies of both scale arrays (64 rows' or tokens' scales of a group = one 256-byte run): gathered
    // from the row-major arrays -- a cache line per lane -- these loads made twice the line requests of the tile's data and 19 % of
    // the kernel (profiles/r02_prefill_gemm_pmc.txt, section 7).  A group past the end (odd group count) gets scale zero:
    // fma(0 * sx, float(d), acc) = acc (acc is never -0).
    const int s_slot = wave * 64;
    const bool s_x = s_slot >= kGPS * TR;
    const int s_gi = s_x ? (s_slot - kGPS * TR) / TT : s_slot / TR;
    const int s_row = s_x ? (b0 + (s_slot - kGPS * TR) % TT + lane < a.B ? b0 + (s_slot - kGPS * TR) % TT + lane : -1) : wrow(s_slot % TR + lane);
    const unsigned s_rows = s_x ? (unsigned)a.B : (TWO ? 2u : 1u) * (unsigned)a.rows;
    const __amdgpu_buffer_rsrc_t rS = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(s_x ? a.XsT : a.sWT), 0, (int)(s_rows * sn * 4), 0x00020000);
    unsigned soff = s_row >= 0 ? ((unsigned)s_gi * s_rows + s_row) * 4 : kOOB;
    const unsigned sstep = kGPS * s_rows * 4;
    const unsigned spoff = (unsigned)(kOffS + tid * 4);
    v4u wr[NPW], xr[NPX]; unsigned sr;
    auto fetch = [&](int st) {                    // stage st -> the register slot (stages past the end: the offsets have run past the rows; never consumed with a non-zero scale)
#pragma unroll
        for (int k = 0; k < NPW; ++k) { wr[k] = __builtin_amdgcn_raw_buffer_load_b128(rW, (int)woff[k], 0, 0); woff[k] += SB; }
#pragma unroll
        for (int k = 0; k < NPX; ++k) { xr[k] = __builtin_amdgcn_raw_buffer_load_b128(rX, (int)xoff[k], 0, 0); xoff[k] += SB; }
        sr = __builtin_amdgcn_raw_buffer_load_b32(rS, (int)(st * kGPS + s_gi < sn ? soff : kOOB), 0, 0); soff += sstep;
    };
    auto park = [&](int buf) {
        char* base = sm + buf * kBuf;
#pragma unroll
        for (int k = 0; k < NPW; ++k) *reinterpret_cast<v4u*>(base + poff + k * (NT / 8) * LS) = wr[k];
#pragma unroll
        for (int k = 0; k < NPX; ++k) *reinterpret_cast<v4u*>(base + kOffX + poff + k * (NT / 8) * LS) = xr[k];
        *reinterpret_cast<unsigned*>(base + spoff) = sr;
    };
    // this wave's 32 tokens x (NB x 32) weight rows
    // (SWIGLU: fragment j = rows wr0 .. wr0 + 31 of half j, i.e. tile rows j TRH + wr0 ..; otherwise fragment j = tile rows wr0 + 32 j ..)
    const int wt0 = (wave % WT) * 32, wr0 = (wave / WT) * 32 * (TWO ? 1 : NB), l31 = lane & 31, h = lane >> 5;
    constexpr int FS = TWO ? TRH : 32;                            // tile rows between a wave's fragments
    const unsigned offA = (unsigned)(kOffX + (wt0 + l31) * LS + h * 16), offB = (unsigned)((wr0 + l31) * LS + h * 16);
    const unsigned offsw = (unsigned)(kOffS + (wr0 + l31) * 4), offsx = (unsigned)(kOffS + (kGPS * TR + wt0 + 4 * h) * 4);
    float acc[NB][16];
#pragma unroll
    for (int j = 0; j < NB; ++j)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[j][i] = 0.f;
    fetch(0); park(0); fetch(1);
    __syncthreads();
    for (int st = 0; st < nst; ++st) {
        const char* base = sm + (st & 1) * kBuf;
#pragma unroll
        for (int gi = 0; gi < kGPS; ++gi) {
            const v4i a0 = *reinterpret_cast<const v4i*>(base + offA + gi * kGroup), a1 = *reinterpret_cast<const v4i*>(base + offA + gi * kGroup + 32);
            float4 sx[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) sx[q] = *reinterpret_cast<const float4*>(base + offsx + gi * TT * 4 + q * 32);
            v16i d[NB];
#pragma unroll
            for (int j = 0; j < NB; ++j) {
                const v4i b0v = *reinterpret_cast<const v4i*>(base + offB + j * FS * LS + gi * kGroup), b1v = *reinterpret_cast<const v4i*>(base + offB + j * FS * LS + gi * kGroup + 32);
                const v16i z = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
                d[j] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a0, b0v, z, 0, 0, 0);
                d[j] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a1, b1v, d[j], 0, 0, 0);
            }
#pragma unroll
            for (int j = 0; j < NB; ++j) {
                const float sw = *reinterpret_cast<const float*>(base + offsw + (gi * TR + j * FS) * 4);
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    acc[j][4 * q + 0] = __fmaf_rn(__fmul_rn(sw, sx[q].x), (float)d[j][4 * q + 0], acc[j][4 * q + 0]);   // quant_operators.cpp:274
                    acc[j][4 * q + 1] = __fmaf_rn(__fmul_rn(sw, sx[q].y), (float)d[j][4 * q + 1], acc[j][4 * q + 1]);
                    acc[j][4 * q + 2] = __fmaf_rn(__fmul_rn(sw, sx[q].z), (float)d[j][4 * q + 2], acc[j][4 * q + 2]);
                    acc[j][4 * q + 3] = __fmaf_rn(__fmul_rn(sw, sx[q].w), (float)d[j][4 * q + 3], acc[j][4 * q + 3]);
                }
            }
        }
        park((st & 1) ^ 1); fetch(st + 2);        // unconditional: a stage past the end is parked and never read with a non-zero scale
        __syncthreads();
    }
    gemm_epilogue<EPI, NB>(a, acc, r0 + wr0 + l31, b0 + wt0, lane);
}

// The int16 GEMM on the matrix cores.  gfx950 has no int16 MFMA; an int16 value is split EXACTLY into two signed bytes,
//     w = 256 * wh + wl,   wl = (int8)(w & 0xff),   wh = (w - wl) >> 8   (|w| <= 5792: wh in [-23, 23])
// so a quant group's dot product is  65536 * S(wh, xh) + 256 * (S(wh, xl) + S(wl, xh)) + S(wl, xl)  with four int8 MFMA
// accumulations S (each exact in int32; the combination wraps mod 2^32 on the way and lands on the true value, which the reference
// also holds in an int32: 64 * 5792^2 < 2^31, x86_simd.cpp:1524-1552).  Eight v_mfma_i32_32x32x32_i8 per group and wave replace 1024
// the fp32 chain step per group is unchanged (quant_operators.cpp:274).  The split happens
// once per 16-byte piece when it is parked in LDS (byte planes lo / hi per row).
__device__ __forceinline__ void split16(const v4i& v, unsigned (&lo)[2], unsigned (&hi)[2]) {
    const unsigned w0 = (unsigned)v.x, w1 = (unsigned)v.y, w2 = (unsigned)v.z, w3 = (unsigned)v.w;
    lo[0] = __builtin_amdgcn_perm(w1, w0, 0x06040200u); lo[1] = __builtin_amdgcn_perm(w3, w2, 0x06040200u);      // bytes 0, 2 of w0 then of w1
    const unsigned h0 = __builtin_amdgcn_perm(w1, w0, 0x07050301u), h1 = __builtin_amdgcn_perm(w3, w2, 0x07050301u);
    // wh = high byte + (low byte negative as int8 ? 1 : 0), bytewise without carries between bytes
    const unsigned c0 = (lo[0] >> 7) & 0x01010101u, c1 = (lo[1] >> 7) & 0x01010101u;
    hi[0] = ((h0 & 0x7f7f7f7fu) + c0) ^ (h0 & 0x80808080u);
    hi[1] = ((h1 & 0x7f7f7f7fu) + c1) ^ (h1 & 0x80808080u);
}
// Built like k_gemm_q8_mfma (64 tokens x 64 rows, four waves of 32 x 32, tokens as the A operand, results in VGPRs, one register
// slot of prefetch, one scale per thread) with a stage of ONE group (128 bytes of a row = two byte planes of 64): 42 KB of LDS,
// three workgroups per CU.  The four partial sums share ONE accumulator: d = S(hh); d <<= 8; d += S(hl) + S(lh); d <<= 8; d += S(ll)
// (the shifts between the MFMAs; everything mod 2^32) -- 16 registers instead of 48.
struct Gemm16Tile {
    static constexpr int TS = 64, LS = kGroup + 16;                           // tile side; LDS row stride of a byte plane
    static constexpr int kPlane = TS * LS, kOffS = 4 * kPlane, kBuf = kOffS + 2 * TS * 4;   // W lo | W hi | X lo | X hi | scales [W][X]
    static constexpr int kLds = 2 * kBuf;
};
template <int EPI>
__global__ void __launch_bounds__(256, 3) k_gemm_q16_mfma(const GemmArgs a) {
    using G = Gemm16Tile;
    constexpr int GB = kGroup * 2, LS = G::LS, TS = G::TS, kPlane = G::kPlane, kOffS = G::kOffS, kBuf = G::kBuf;
    extern __shared__ __attribute__((aligned(16))) char lds[]; char* const sm = lds;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int ntt = (a.B + TS - 1) / TS;
    const int nb = gridDim.x, per = nb >> 3, rem = nb & 7, xcd = blockIdx.x & 7;              // tiles dealt to the XCDs in contiguous runs (token tile fastest: the tiles that share 64 weight rows are neighbours in the LOGICAL order, and workgroup b runs on XCD b mod 8 with its own L2: weight rows are fetched from HBM once per XCD instead of once per token tile)
    const int tile = xcd * per + (xcd < rem ? xcd : rem) + (blockIdx.x >> 3);
    // EPI_SWIGLU: W = [W1 (gate) ; W3 (up)], a.rows rows each; a tile = 32 rows of W1 (the waves 0, 1) and the SAME 32 rows of W3 (the waves 2, 3): the up halves go
    // through LDS to the lanes that hold the gate halves, the epilogue is the SwiGLU (no [tokens][2 hidden] round trip, no k_swiglu_rows)
    constexpr bool TWO = EPI == EPI_SWIGLU;
    constexpr int TRW = TWO ? TS / 2 : TS;                                                     // rows of (each) matrix per tile
    const int r0 = (tile / ntt) * TRW, b0 = (tile % ntt) * TS;
    const int sn = a.n / kGroup;
    const unsigned rowbytes = (unsigned)a.n * 2;
    constexpr unsigned kOOB = 0x80000000u;
    const __amdgpu_buffer_rsrc_t rW = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(a.W), 0, (int)((unsigned)a.rows * (TWO ? 2u : 1u) * rowbytes), 0x00020000);
    const __amdgpu_buffer_rsrc_t rX = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(a.Xq), 0, (int)((unsigned)a.B * rowbytes), 0x00020000);
    // loader: piece k of a thread = 16 bytes (8 elements) at (row (tid >> 3) + 32 k, chunk tid & 7) of both matrices
    const int prow = tid >> 3, pch = tid & 7;
    unsigned woff[2], xoff[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        if constexpr (TWO) woff[k] = (r0 + prow < a.rows) ? (unsigned)(k * a.rows + r0 + prow) * rowbytes + pch * 16 : kOOB;      // piece 0: W1's row, piece 1: W3's
        else woff[k] = (r0 + prow + 32 * k < a.rows) ? (unsigned)(r0 + prow + 32 * k) * rowbytes + pch * 16 : kOOB;
        xoff[k] = (b0 + prow + 32 * k < a.B)    ? (unsigned)(b0 + prow + 32 * k) * rowbytes + pch * 16 : kOOB;
    }
    const unsigned poff = (unsigned)(prow * LS + pch * 8);
    // scales: wave 0 = the weight rows', wave 1 = the tokens' (lane = row of the tile), from the group-major copies (see k_gemm_q8_mfma);
    // waves 2, 3 load nothing
    const bool s_x = wave == 1;
    const int s_rows = wave < 2 ? (s_x ? a.B : a.rows * (TWO ? 2 : 1)) : 0;
    int s_row = (s_x ? b0 : r0) + lane; bool s_ok = s_row < s_rows;
    if (TWO && !s_x) { s_row = (lane >> 5) * a.rows + r0 + (lane & 31); s_ok = r0 + (lane & 31) < a.rows; }      // (lanes 0..31: W1's rows, 32..63: W3's)
    const __amdgpu_buffer_rsrc_t rS = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(s_x ? a.XsT : a.sWT), 0, (int)((unsigned)s_rows * sn * 4), 0x00020000);
    unsigned soff = s_ok ? (unsigned)s_row * 4 : kOOB;
    const unsigned spoff = (unsigned)(kOffS + (tid & 127) * 4);
    v4u wr[2], xr[2]; unsigned sr;
    auto fetch = [&](int g) {                     // group g -> the register slot (groups past the end: zero scale, never consumed otherwise)
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            wr[k] = __builtin_amdgcn_raw_buffer_load_b128(rW, (int)woff[k], 0, 0); woff[k] += GB;
            xr[k] = __builtin_amdgcn_raw_buffer_load_b128(rX, (int)xoff[k], 0, 0); xoff[k] += GB;
        }
        sr = __builtin_amdgcn_raw_buffer_load_b32(rS, (int)(g < sn ? soff : kOOB), 0, 0); soff += (unsigned)s_rows * 4;
    };
    auto park = [&](int buf) {
        char* base = sm + buf * kBuf;
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            unsigned lo[2], hi[2];
            split16(__builtin_bit_cast(v4i, wr[k]), lo, hi);
            *reinterpret_cast<uint2*>(base + poff + k * 32 * LS) = make_uint2(lo[0], lo[1]); *reinterpret_cast<uint2*>(base + kPlane + poff + k * 32 * LS) = make_uint2(hi[0], hi[1]);
            split16(__builtin_bit_cast(v4i, xr[k]), lo, hi);
            *reinterpret_cast<uint2*>(base + 2 * kPlane + poff + k * 32 * LS) = make_uint2(lo[0], lo[1]); *reinterpret_cast<uint2*>(base + 3 * kPlane + poff + k * 32 * LS) = make_uint2(hi[0], hi[1]);
        }
        if (wave < 2) *reinterpret_cast<unsigned*>(base + spoff) = sr;
    };
    const int wt0 = (wave & 1) * 32, wr0 = (wave >> 1) * 32, l31 = lane & 31, h = lane >> 5;
    const unsigned offX = (unsigned)(2 * kPlane + (wt0 + l31) * LS + h * 16), offW = (unsigned)((wr0 + l31) * LS + h * 16);
    const unsigned offsw = (unsigned)(kOffS + (wr0 + l31) * 4), offsx = (unsigned)(kOffS + (TS + wt0 + 4 * h) * 4);
    float acc[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
    fetch(0); park(0); fetch(1);
    __syncthreads();
    for (int g = 0; g < sn; ++g) {
        const char* base = sm + (g & 1) * kBuf;
        const v4i xl0 = *reinterpret_cast<const v4i*>(base + offX), xl1 = *reinterpret_cast<const v4i*>(base + offX + 32);
        const v4i xh0 = *reinterpret_cast<const v4i*>(base + offX + kPlane), xh1 = *reinterpret_cast<const v4i*>(base + offX + kPlane + 32);
        const v4i wl0 = *reinterpret_cast<const v4i*>(base + offW), wl1 = *reinterpret_cast<const v4i*>(base + offW + 32);
        const v4i wh0 = *reinterpret_cast<const v4i*>(base + offW + kPlane), wh1 = *reinterpret_cast<const v4i*>(base + offW + kPlane + 32);
        const v16i z = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        v16i d = __builtin_amdgcn_mfma_i32_32x32x32_i8(xh0, wh0, z, 0, 0, 0);
        d = __builtin_amdgcn_mfma_i32_32x32x32_i8(xh1, wh1, d, 0, 0, 0);
#pragma unroll
        for (int i = 0; i < 16; ++i) d[i] = (int)((unsigned)d[i] << 8);
        d = __builtin_amdgcn_mfma_i32_32x32x32_i8(xh0, wl0, d, 0, 0, 0);
        d = __builtin_amdgcn_mfma_i32_32x32x32_i8(xh1, wl1, d, 0, 0, 0);
        d = __builtin_amdgcn_mfma_i32_32x32x32_i8(xl0, wh0, d, 0, 0, 0);
        d = __builtin_amdgcn_mfma_i32_32x32x32_i8(xl1, wh1, d, 0, 0, 0);
#pragma unroll
        for (int i = 0; i < 16; ++i) d[i] = (int)((unsigned)d[i] << 8);
        d = __builtin_amdgcn_mfma_i32_32x32x32_i8(xl0, wl0, d, 0, 0, 0);                  // wraps mod 2^32 onto the exact int32 dot
        d = __builtin_amdgcn_mfma_i32_32x32x32_i8(xl1, wl1, d, 0, 0, 0);
        const float sw = *reinterpret_cast<const float*>(base + offsw);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float4 sx = *reinterpret_cast<const float4*>(base + offsx + q * 32);
            acc[4 * q + 0] = __fmaf_rn(__fmul_rn(sw, sx.x), (float)d[4 * q + 0], acc[4 * q + 0]);   // quant_operators.cpp:274
            acc[4 * q + 1] = __fmaf_rn(__fmul_rn(sw, sx.y), (float)d[4 * q + 1], acc[4 * q + 1]);
            acc[4 * q + 2] = __fmaf_rn(__fmul_rn(sw, sx.z), (float)d[4 * q + 2], acc[4 * q + 2]);
            acc[4 * q + 3] = __fmaf_rn(__fmul_rn(sw, sx.w), (float)d[4 * q + 3], acc[4 * q + 3]);
        }
        park((g & 1) ^ 1); fetch(g + 2);          // unconditional: a group past the end is parked and never read with a non-zero scale
        __syncthreads();
    }
    if constexpr (EPI == EPI_ROPE_KV) {
        float accw[1][16];
#pragma unroll
        for (int i = 0; i < 16; ++i) accw[0][i] = acc[i];
        gemm_epilogue<EPI_ROPE_KV, 1>(a, accw, r0 + wr0 + l31, b0 + wt0, lane);
        return;
    }
    if constexpr (TWO) {
        // the up halves (waves 2, 3) to the lanes that hold the gate halves of the same (row, tokens): through LDS (the loop's last barrier has passed: the stages are dead)
        float* xch = reinterpret_cast<float*>(sm);
        if (wave >= 2) {
#pragma unroll
            for (int i = 0; i < 16; ++i) xch[((wave & 1) * 64 + lane) * 17 + i] = acc[i];
        }
        __syncthreads();
        if (wave >= 2) return;
        const int row = r0 + l31;
        if (row < a.rows) {
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int b = b0 + wt0 + (i & 3) + 8 * (i >> 2) + 4 * h;
                if (b < a.B) st_result_tp(a.out, (size_t)b * a.ldo + row, swiglu_elem(acc[i], xch[((wave & 1) * 64 + lane) * 17 + i]), a.out_peer, a.n_peer);   // o1.swiglu(o3) transformer.cpp:481
            }
        }
        return;
    }
    const int row = r0 + wr0 + l31;
    if (row < a.rows) {
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int b = b0 + wt0 + (i & 3) + 8 * (i >> 2) + 4 * h;
            if (b >= a.B) continue;
            const size_t idx = (size_t)b * a.ldo + row;
            if constexpr (EPI == EPI_RESIDUAL) st_result_tp(a.out, idx, __fadd_rn(a.n_peer ? ld_agent(a.out + idx) : a.out[idx], acc[i]), a.out_peer, a.n_peer);   // (peers: tensor parallel, see GemmArgs)
            else a.out[idx] = acc[i];
        }
    }
}

// ------------------------------------------------------------------------------------------
// The skinny int8 GEMM: B <= 16 tokens (the verify pass of flm_verify_greedy / flm_generate_lookup, flm_op_matmul_skinny).  At 5 .. 16 rows three quarters or more of
// every 64-token tile above is padding, the LDS staging that bounds the tiles buys nothing (a weight byte is used once) and Wo has 64 tiles for 256 CUs.  Here:
//   * v_mfma_i32_16x16x64_i8: ONE instruction = 16 tokens x 16 weight rows x one quant group of 64 -- the group's 256 int32 dots, exact.  Tokens are the A operand, weight
//     rows the B operand (as in the tiles): C/D col = lane & 15 = the weight row, row = 4 (lane >> 4) + reg = the token, so a lane owns ONE weight row and four tokens.
//     A and B use the same byte -> k assignment (lane quarter q takes bytes 16 q .. 16 q + 15 of the group), and integer sums are order-free.
//   * weights go from global memory straight into the operand registers: a lane's 16 bytes are contiguous in its row, the four lanes of a row cover the group's 64
//     bytes.  Nothing is staged in LDS; D groups (8, or 6 with two fragments) are in flight per wave in a register ring, every weight byte is read once per pass.
//   * per output the SAME fp32 chain step as k_gemm_q8_mfma: v_cvt, sw * sx, fma, groups ascending -- the bits are the tiles' (and the token path's).
//   * a workgroup is ONE wave and owns 16 rows (NB = 1: Wo and W2 of the 7B shape = 256 workgroups, one per CU) or 32 (NB = 2, where that still gives every CU a
//     workgroup: QKV, the classifier; the two fragments share the activation operand) -- SwiGLU: the same 16 rows of W1 and W3, gate and up meet in one lane.
//   * the <= 16 quantized activation rows are read through L2 (buffer loads; token columns >= B read as zero and are never stored); their scales sit in LDS,
//     [groups][16], zero for idle columns and for the ring's groups past the end: fma(0 * 0, float(0), acc) = acc (acc is never -0).
// INT4 and int16 models have siblings below: k_gemm_q4_skinny on the packed nibbles, k_gemm_q16_skinny on byte planes split in registers.
// ------------------------------------------------------------------------------------------
template <int EPI, int NB>
__device__ __forceinline__ void skinny_epilogue(const GemmArgs& a, const float (&acc)[NB][4], const int rbase, const int lane) {
    const int q = lane >> 4;
    if constexpr (EPI == EPI_ROPE_KV) {
        // a fragment's 16 rows lie inside one of q / k / v (dim is a multiple of 32) and a RoPE pair (rows 2i, 2i + 1) in neighbouring lanes
#pragma unroll
        for (int j = 0; j < NB; ++j) {
            const int row = rbase + j * 16, which = row / a.dim, within = row - which * a.dim, hh = within / a.hs, dd = within - hh * a.hs;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int b = 4 * q + i, pos = a.pos0 + b;
                const float mine = acc[j][i], other = __shfl_xor(mine, 1, 64);
                if (row >= a.rows || b >= a.B) continue;
                float v = mine;
                if (which < 2) {
                    const float c = a.rope_cos[(size_t)pos * (a.hs / 2) + dd / 2], sn_ = a.rope_sin[(size_t)pos * (a.hs / 2) + dd / 2];
                    float o0, o1;
                    rope_pair((lane & 1) ? other : mine, (lane & 1) ? mine : other, c, sn_, o0, o1);
                    v = (lane & 1) ? o1 : o0;
                }
                if (which == 0) a.qout[(size_t)b * a.dim + within] = v;
                else (which == 1 ? a.kcache : a.vcache)[((size_t)hh * a.max_seq + pos) * a.hs + dd] = v;
            }
        }
    } else if constexpr (EPI == EPI_SWIGLU) {
        if (rbase < a.rows) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int b = 4 * q + i;
                if (b < a.B) st_result_tp(a.out, (size_t)b * a.ldo + rbase, swiglu_elem(acc[0][i], acc[NB - 1][i]), a.out_peer, a.n_peer);   // o1.swiglu(o3) transformer.cpp:481
            }
        }
    } else {
#pragma unroll
        for (int j = 0; j < NB; ++j) {
            const int row = rbase + j * 16;
            if (row >= a.rows) continue;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int b = 4 * q + i;
                if (b >= a.B) continue;
                const size_t idx = (size_t)b * a.ldo + row;
                if constexpr (EPI == EPI_RESIDUAL) a.out[idx] = __fadd_rn(a.out[idx], acc[j][i]);
                else a.out[idx] = acc[j][i];
            }
        }
    }
}
constexpr int kSkinnyTokens = 16;
__host__ __device__ constexpr int skinny_depth(int nb) { return nb == 1 ? 8 : 6; }                       // groups in flight per wave
__host__ __device__ inline int skinny_groups_padded(int sn, int nb) { const int d = skinny_depth(nb); return (sn + d - 1) / d * d + d; }
__host__ __device__ inline size_t skinny_lds_bytes(int n, int nb) { return (size_t)skinny_groups_padded(n / kGroup, nb) * kSkinnyTokens * 4; }
// grid: ceil(rows / (16 NB)) workgroups of 64 threads (SWIGLU: ceil(rows / 16), NB = 2); skinny_lds_bytes(n, NB) of dynamic LDS; B <= 16; single GPU (no peers)
template <int EPI, int NB>
__global__ void __launch_bounds__(64) k_gemm_q8_skinny(const GemmArgs a) {
    constexpr bool TWO = EPI == EPI_SWIGLU;
    static_assert(!TWO || NB == 2, "gate and up are the two B fragments of the wave");
    constexpr int D = skinny_depth(NB);
    extern __shared__ __attribute__((aligned(16))) char lds[];
    float* const sxl = reinterpret_cast<float*>(lds);                       // [groups, padded][16 tokens]
    const int lane = threadIdx.x, l15 = lane & 15, q = lane >> 4;
    const int sn = a.n / kGroup, snp = skinny_groups_padded(sn, NB);
    const int r0 = blockIdx.x * (TWO ? 16 : 16 * NB);
    for (int i = lane; i < snp * kSkinnyTokens; i += 64) { const int g = i >> 4, b = i & 15; sxl[i] = (g < sn && b < a.B) ? a.Xs[(size_t)b * sn + g] : 0.0f; }
    __syncthreads();
    const unsigned rowbytes = (unsigned)a.n;
    constexpr unsigned kOOB = 0x80000000u;
    const unsigned s_rows = (TWO ? 2u : 1u) * (unsigned)a.rows;
    const __amdgpu_buffer_rsrc_t rW = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(a.W), 0, (int)(s_rows * rowbytes), 0x00020000);
    const __amdgpu_buffer_rsrc_t rX = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(a.Xq), 0, (int)((unsigned)a.B * rowbytes), 0x00020000);
    const __amdgpu_buffer_rsrc_t rS = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.sWT), 0, (int)(s_rows * (unsigned)sn * 4), 0x00020000);
    // fragment j: rows r0 + 16 j .. (SWIGLU: rows r0 .. of W1 (j = 0) and of W3 (j = 1)); rows past the matrix and groups past the end read as zero
    unsigned woff[NB], soff[NB];
#pragma unroll
    for (int j = 0; j < NB; ++j) {
        const int row = r0 + (TWO ? 0 : 16 * j) + l15;
        const unsigned wrow = (unsigned)(TWO ? j * a.rows + row : row);
        woff[j] = row < a.rows ? wrow * rowbytes + (unsigned)q * 16 : kOOB;
        soff[j] = row < a.rows ? wrow * 4 : kOOB;
    }
    const unsigned xoff = l15 < a.B ? (unsigned)l15 * rowbytes + (unsigned)q * 16 : kOOB;
    const unsigned sstep = s_rows * 4;
    v4u wr[D][NB], xr[D]; unsigned sr[D][NB];
    auto fetch = [&](const int slot, const int g) {                       // group g -> ring slot `slot`
        const bool in = g < sn;
#pragma unroll
        for (int j = 0; j < NB; ++j) {
            wr[slot][j] = __builtin_amdgcn_raw_buffer_load_b128(rW, (int)(in && woff[j] != kOOB ? woff[j] + (unsigned)g * kGroup : kOOB), 0, 0);
            sr[slot][j] = __builtin_amdgcn_raw_buffer_load_b32(rS, (int)(in && soff[j] != kOOB ? soff[j] + (unsigned)g * sstep : kOOB), 0, 0);
        }
        xr[slot] = __builtin_amdgcn_raw_buffer_load_b128(rX, (int)(in && xoff != kOOB ? xoff + (unsigned)g * kGroup : kOOB), 0, 0);
    };
    float acc[NB][4];
#pragma unroll
    for (int j = 0; j < NB; ++j)
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[j][i] = 0.f;
#pragma unroll
    for (int k = 0; k < D; ++k) fetch(k, k);
    for (int g0 = 0; g0 < sn; g0 += D) {
#pragma unroll
        for (int k = 0; k < D; ++k) {
            const int g = g0 + k;                                           // (g >= sn in the last round: zero operands, zero scales)
            const float4 sx = *reinterpret_cast<const float4*>(sxl + g * kSkinnyTokens + 4 * q);
#pragma unroll
            for (int j = 0; j < NB; ++j) {
                const v4i z = {0, 0, 0, 0};
                const v4i d = __builtin_amdgcn_mfma_i32_16x16x64_i8(__builtin_bit_cast(v4i, xr[k]), __builtin_bit_cast(v4i, wr[k][j]), z, 0, 0, 0);
                const float sw = __uint_as_float(sr[k][j]);
                acc[j][0] = __fmaf_rn(__fmul_rn(sw, sx.x), (float)d[0], acc[j][0]);   // quant_operators.cpp:274
                acc[j][1] = __fmaf_rn(__fmul_rn(sw, sx.y), (float)d[1], acc[j][1]);
                acc[j][2] = __fmaf_rn(__fmul_rn(sw, sx.z), (float)d[2], acc[j][2]);
                acc[j][3] = __fmaf_rn(__fmul_rn(sw, sx.w), (float)d[3], acc[j][3]);
            }
            fetch(k, g + D);
        }
    }
    skinny_epilogue<EPI, NB>(a, acc, r0 + l15, lane);
}

// ------------------------------------------------------------------------------------------
// The split-K skinny int8 GEMM ("spec_gemm" 2): k_gemm_q8_skinny's GemmArgs, epilogues, grid rule and bits, with W = 4 waves (one per SIMD) on a workgroup's 16 NB rows.
// One wave per 16 rows keeps D KiB per fragment in flight and three SIMDs of a CU idle where the grid is the CU count (Wo, W2); four waves on the same rows keep the grid
// and carry four rings.
//   * split: wave w owns the quant groups g = w (mod W); a round is W consecutive groups, one per wave, 256 contiguous bytes of a weight row.  Every wave has its own
//     register ring of D groups (weights by b128 buffer loads straight into the B operand, its groups' activation bytes, its groups' weight scales); addresses, descriptors
//     and zero rules are k_gemm_q8_skinny's (rows past the matrix, groups past the end and idle token columns read as zero).
//   * integer part: per group and fragment one v_mfma_i32_16x16x64_i8, tokens = A, weight rows = B.  The 256 int32 dots are exact: which wave made them changes no bit.
//   * ordered chain: acc = fma(sw * sx, float(d), acc) must see the groups ascending, so the dots leave the wave that made them.  A wave parks its group's dots in an LDS
//     slot [W groups][NB][16 tokens][16 rows] int32 (1 KiB per group and fragment) and its 16 weight scales beside them; the activation scales are the [groups][16]
//     table of k_gemm_q8_skinny (sw * sx is formed by the consumer from the parked sw and the table's sx -- not parked as a product, which would double the ring).  The
//     slots are double-buffered, so a round costs ONE barrier: round r + 2 overwrites slot r & 1 only behind barrier r + 1, which every wave reaches after its reads of
//     round r.  After the barrier wave w carries the chains of tokens 4 w .. 4 w + 3: lane (l15, q) = (row, token 4 w + q), ONE output per fragment, W chain steps per
//     round in group order.  A lane carries NB chains where k_gemm_q8_skinny's carries 4 NB, and the chain work of a workgroup runs on four SIMDs.
//   * banks: a producer lane (l15, q) holds tokens 4 q + i; token t lies in row t ^ (t >> 2) of its 16 x 16 block, so that the four lane quarters of one ds_write hit
//     four different 16-bank groups.  A consumer wave's four tokens are a permutation of four neighbouring rows: its reads are 64 consecutive words.
//   * uniform: every wave runs all ceil(groups / W) rounds (a wave without a live group in the last one parks zeros and a zero scale); the barriers sit under
//     conditions on n alone.  No wait on another workgroup.
//   * epilogue: the 16 x 16 NB accumulators meet in LDS and wave 0 reads them in k_gemm_q8_skinny's C layout (lane = row, registers = tokens 4 q + i) and runs
//     skinny_epilogue unchanged -- the RoPE pair in neighbouring lanes, the SwiGLU pairing, the residual add.
// LDS: the sx table (64 bytes per group) + 2 slots x W NB x (1 KiB + 64 B) + NB KiB: 20.5 KiB at n = 11008, NB = 1; the launcher refuses rows whose table does not fit.
// ------------------------------------------------------------------------------------------
constexpr int kSkinnySkWaves = 4;
__host__ __device__ constexpr int skinny_sk_depth(int nb) { return nb == 1 ? 8 : 4; }                    // groups in flight per wave: 32 KiB per workgroup either way (even: a round's slot is its ring index & 1; six groups of two fragments do not fit 128 registers)
__host__ __device__ inline int skinny_sk_rounds(int sn) { return (sn + kSkinnySkWaves - 1) / kSkinnySkWaves; }
__host__ __device__ constexpr int skinny_sk_slot_words(int nb) { return kSkinnySkWaves * nb * (256 + 16); }   // a round's dots and weight scales
__host__ __device__ inline size_t skinny_sk_lds_bytes(int n, int nb) {
    return ((size_t)skinny_sk_rounds(n / kGroup) * kSkinnySkWaves * kSkinnyTokens + 2 * skinny_sk_slot_words(nb) + nb * 256) * 4;
}
// grid: ceil(rows / (16 NB)) workgroups of 256 threads (SWIGLU: ceil(rows / 16), NB = 2); skinny_sk_lds_bytes(n, NB) of dynamic LDS; B <= 16; single GPU (no peers)
// waves_per_eu(4): at most 128 registers to a wave -- two workgroups to a CU where the grid exceeds the CUs -- and the MFMA results in VGPRs (see k_gemm_q4_skinny)
template <int EPI, int NB>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4))) k_gemm_q8_skinny_sk(const GemmArgs a) {
    constexpr bool TWO = EPI == EPI_SWIGLU;
    static_assert(!TWO || NB == 2, "gate and up are the two B fragments of the wave");
    constexpr int W = kSkinnySkWaves, D = skinny_sk_depth(NB), SLOT = skinny_sk_slot_words(NB);
    static_assert(D % 2 == 0, "slot of round r0 + k = k & 1");
    extern __shared__ __attribute__((aligned(16))) char lds[];
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6), lane = threadIdx.x & 63, l15 = lane & 15, q = lane >> 4;
    const int sn = a.n / kGroup, rounds = skinny_sk_rounds(sn);
    float* const sxl = reinterpret_cast<float*>(lds);                       // [rounds W groups][16 tokens]
    int* const ring = reinterpret_cast<int*>(sxl + rounds * W * kSkinnyTokens);   // [2 slots]{[W][NB][16][16] dots, [W][NB][16] weight scales}
    float* const fin = reinterpret_cast<float*>(ring + 2 * SLOT);            // [NB][16 tokens][16 rows]
    const int r0 = blockIdx.x * (TWO ? 16 : 16 * NB);
    for (int i = threadIdx.x; i < rounds * W * kSkinnyTokens; i += 256) { const int g = i >> 4, b = i & 15; sxl[i] = (g < sn && b < a.B) ? a.Xs[(size_t)b * sn + g] : 0.0f; }
    // (no barrier here: the table is first read behind the barrier of round 0)
    const unsigned rowbytes = (unsigned)a.n;
    constexpr unsigned kOOB = 0x80000000u;
    const unsigned s_rows = (TWO ? 2u : 1u) * (unsigned)a.rows;
    const __amdgpu_buffer_rsrc_t rW = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(a.W), 0, (int)(s_rows * rowbytes), 0x00020000);
    const __amdgpu_buffer_rsrc_t rX = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(a.Xq), 0, (int)((unsigned)a.B * rowbytes), 0x00020000);
    const __amdgpu_buffer_rsrc_t rS = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.sWT), 0, (int)(s_rows * (unsigned)sn * 4), 0x00020000);
    unsigned woff[NB], soff[NB];
#pragma unroll
    for (int j = 0; j < NB; ++j) {
        const int row = r0 + (TWO ? 0 : 16 * j) + l15;
        const unsigned wrow = (unsigned)(TWO ? j * a.rows + row : row);
        woff[j] = row < a.rows ? wrow * rowbytes + (unsigned)q * 16 : kOOB;
        soff[j] = row < a.rows ? wrow * 4 : kOOB;
    }
    const unsigned xoff = l15 < a.B ? (unsigned)l15 * rowbytes + (unsigned)q * 16 : kOOB;
    const unsigned sstep = s_rows * 4;
    v4u wr[D][NB], xr[D]; unsigned sr[D][NB];
    auto fetch = [&](const int slot, const int g) {                       // group g -> ring slot `slot`
        const bool in = g < sn;
#pragma unroll
        for (int j = 0; j < NB; ++j) {
            wr[slot][j] = __builtin_amdgcn_raw_buffer_load_b128(rW, (int)(in && woff[j] != kOOB ? woff[j] + (unsigned)g * kGroup : kOOB), 0, 0);
            sr[slot][j] = __builtin_amdgcn_raw_buffer_load_b32(rS, (int)(in && soff[j] != kOOB ? soff[j] + (unsigned)g * sstep : kOOB), 0, 0);
        }
        xr[slot] = __builtin_amdgcn_raw_buffer_load_b128(rX, (int)(in && xoff != kOOB ? xoff + (unsigned)g * kGroup : kOOB), 0, 0);
    };
    // producer: token 4 q + i of this wave's group -> word pofs[i] of the group's block; consumer: (token 4 wave + q, row l15) -> word cofs
    int pofs[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) pofs[i] = (4 * q + (i ^ q)) * 16 + l15;
    const int cofs = (4 * wave + (q ^ wave)) * 16 + l15, ctok = 4 * wave + q;
    float acc[NB];
#pragma unroll
    for (int j = 0; j < NB; ++j) acc[j] = 0.f;
#pragma unroll
    for (int k = 0; k < D; ++k) fetch(k, k * W + wave);
    for (int rb = 0; rb < rounds; rb += D) {
#pragma unroll
        for (int k = 0; k < D; ++k) {
            const int r = rb + k;
            if (r >= rounds) break;                                         // (a condition on n alone: every wave of every workgroup takes it alike)
            int* const dots = ring + (k & 1) * SLOT;
            float* const sws = reinterpret_cast<float*>(dots + W * NB * 256);
#pragma unroll
            for (int j = 0; j < NB; ++j) {                                  // group r W + wave (past the end in the last round: zero operands, a zero scale)
                const v4i z = {0, 0, 0, 0};
                const v4i d = __builtin_amdgcn_mfma_i32_16x16x64_i8(__builtin_bit_cast(v4i, xr[k]), __builtin_bit_cast(v4i, wr[k][j]), z, 0, 0, 0);
                int* const blk = dots + (wave * NB + j) * 256;
                blk[pofs[0]] = d[0]; blk[pofs[1]] = d[1]; blk[pofs[2]] = d[2]; blk[pofs[3]] = d[3];
                if (q == 0) sws[(wave * NB + j) * 16 + l15] = __uint_as_float(sr[k][j]);
            }
            fetch(k, (r + D) * W + wave);
            __syncthreads();
#pragma unroll
            for (int u = 0; u < W; ++u) {                                   // the round's W groups, ascending
                const float sx = sxl[(r * W + u) * kSkinnyTokens + ctok];
#pragma unroll
                for (int j = 0; j < NB; ++j) {
                    const int d = dots[(u * NB + j) * 256 + cofs];
                    const float sw = sws[(u * NB + j) * 16 + l15];
                    acc[j] = __fmaf_rn(__fmul_rn(sw, sx), (float)d, acc[j]);   // quant_operators.cpp:274
                }
            }
        }
    }
#pragma unroll
    for (int j = 0; j < NB; ++j) fin[j * 256 + ctok * 16 + l15] = acc[j];
    __syncthreads();
    if (wave != 0) return;
    float out[NB][4];
#pragma unroll
    for (int j = 0; j < NB; ++j)
#pragma unroll
        for (int i = 0; i < 4; ++i) out[j][i] = fin[j * 256 + (4 * q + i) * 16 + l15];
    skinny_epilogue<EPI, NB>(a, out, r0 + l15, lane);
}

// ------------------------------------------------------------------------------------------
// The skinny W4A8 GEMM: k_gemm_q8_skinny's contract (tokens = A, weight rows = B of v_mfma_i32_16x16x64_i8, C/D col = lane & 15 = the weight row, row = 4 (lane >> 4)
// + reg = the token, one wave per workgroup, activation scales [groups][16] in LDS, the chain step and skinny_epilogue unchanged) on a matrix in the DEVICE nibble layout
// (flm_gemv4.h) -- a.W is [rows][n / 2] packed bytes, nothing is unpacked to memory.
//   * operand: lane (l15, q) owns weights 16 q .. 16 q + 15 of group g of its row = the 8 bytes at row * n / 2 + 32 g + 8 q, ONE 8-byte buffer load.  Its two words are
//     the B operand {w0 & M, (w0 >> 4) & M, w1 & M, (w1 >> 4) & M}, M = 0x0F0F0F0F: the 16 offset nibbles u = q + 8 in column order, byte for byte next to the 16
//     activation bytes the lane loads at 64 g + 16 q.  Six VALU per fragment and group, no per-byte shift, no sign extension.
//   * the offset leaves once per group, exactly: sum (u - 8) x = sum u x - 8 sum x.  One more MFMA per group with B = 0x01010101 gives sum x of every token in the C
//     layout (every column alike); shifted left by 3 and negated (4 VALU, shared by the NB fragments) it is the accumulator INPUT of the fragment MFMAs, whose result is
//     then the exact int32 dot of the sign-extended nibbles (|sum u x| <= 64 * 15 * 127, |8 sum x| <= 8 * 64 * 127).  The float chain behind it is the int8 kernel's.
//   * ring: a fragment's slot is 8 bytes, half of int8's, so the ring holds D = 16 (NB = 1) or 12 (NB = 2) groups.  The activation ring has the SAME depth although
//     its bytes come from L2: a wave's loads return in issue order, so a wait for the activation of group g + 1 from a shallower ring would also wait for every weight
//     load issued before it, and the weight ring's depth would shrink to the activation ring's.  One wave per workgroup and at most a few workgroups per CU: the 112 /
//     120 ring registers limit nothing.
//   * zeros: a zero WORD now means sixteen weights of -8, not 0.  Rows past the matrix: their weight loads are out of range (words 0, dot = -8 sum x) and so are their
//     scale loads -- sw = 0, fma(0 * sx, d, acc) = acc -- and skinny_epilogue masks them at the store.  Groups past the end (the ring's last round) and token columns
//     >= B read zero ACTIVATIONS: sum x = 0 and every product is 0, so d = 0 whatever the weight words are; their sx (LDS) and sw are 0 as well.
//   num_records of the weight descriptor is in BYTES of the packed matrix (SWIGLU: of both halves).
// ------------------------------------------------------------------------------------------
typedef unsigned v2u __attribute__((ext_vector_type(2)));
template <bool T> struct SkinnyTail { static constexpr bool value = T; };
__host__ __device__ constexpr int skinny4_depth(int nb) { return nb == 1 ? 16 : 12; }                    // groups in flight per wave
__host__ __device__ inline int skinny4_groups_padded(int sn, int nb) { const int d = skinny4_depth(nb); return (sn + d - 1) / d * d + d; }
__host__ __device__ inline size_t skinny4_lds_bytes(int n, int nb) { return (size_t)skinny4_groups_padded(n / kGroup, nb) * kSkinnyTokens * 4; }
// grid: ceil(rows / (16 NB)) workgroups of 64 threads (SWIGLU: ceil(rows / 16), NB = 2); skinny4_lds_bytes(n, NB) of dynamic LDS; B <= 16; single GPU (no peers)
// waves_per_eu(2): with at most 256 registers to a wave the compiler keeps the MFMA results in VGPRs; given 512 it puts them into AGPRs and pays 12 v_accvgpr copies per group
template <int EPI, int NB>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2))) k_gemm_q4_skinny(const GemmArgs a) {
    constexpr bool TWO = EPI == EPI_SWIGLU;
    static_assert(!TWO || NB == 2, "gate and up are the two B fragments of the wave");
    constexpr int D = skinny4_depth(NB);
    extern __shared__ __attribute__((aligned(16))) char lds[];
    float* const sxl = reinterpret_cast<float*>(lds);                       // [groups, padded][16 tokens]
    const int lane = threadIdx.x, l15 = lane & 15, q = lane >> 4;
    const int sn = a.n / kGroup, snp = skinny4_groups_padded(sn, NB);
    const int r0 = blockIdx.x * (TWO ? 16 : 16 * NB);
    for (int i = lane; i < snp * kSkinnyTokens; i += 64) { const int g = i >> 4, b = i & 15; sxl[i] = (g < sn && b < a.B) ? a.Xs[(size_t)b * sn + g] : 0.0f; }
    __syncthreads();
    const unsigned xbytes = (unsigned)a.n, wbytes = (unsigned)a.n / 2;      // a row of activations, a row of packed weights
    constexpr unsigned kOOB = 0x80000000u, kWGroup = kGroup / 2, kNib = 0x0F0F0F0Fu;
    const unsigned s_rows = (TWO ? 2u : 1u) * (unsigned)a.rows;
    const __amdgpu_buffer_rsrc_t rW = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(a.W), 0, (int)(s_rows * wbytes), 0x00020000);
    const __amdgpu_buffer_rsrc_t rX = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(a.Xq), 0, (int)((unsigned)a.B * xbytes), 0x00020000);
    const __amdgpu_buffer_rsrc_t rS = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.sWT), 0, (int)(s_rows * (unsigned)sn * 4), 0x00020000);
    // fragment j: rows r0 + 16 j .. (SWIGLU: rows r0 .. of W1 (j = 0) and of W3 (j = 1)).  A dead lane (a row past the matrix, a token column >= B) carries bit 31 in its
    // offsets, a dead group ORs it in: an offset of 2^31 or more is out of range of every descriptor here (the launcher bounds them), and no sum below wraps
    unsigned woff[NB], soff[NB];
#pragma unroll
    for (int j = 0; j < NB; ++j) {
        const int row = r0 + (TWO ? 0 : 16 * j) + l15;
        const unsigned wrow = (unsigned)(TWO ? j * a.rows + row : row);
        woff[j] = row < a.rows ? wrow * wbytes + (unsigned)q * 8 : kOOB;
        soff[j] = row < a.rows ? wrow * 4 : kOOB;
    }
    const unsigned xoff = l15 < a.B ? (unsigned)l15 * xbytes + (unsigned)q * 16 : kOOB;
    const unsigned sstep = s_rows * 4;
    v2u wr[D][NB]; v4u xr[D]; unsigned sr[D][NB];
    // groups gb + k -> ring slot k.  A round's addresses are one VALU add per stream (the step's share is the instruction's immediate offset) plus one per scale load;
    // TAIL: the round may run past the last group -- those loads go out of range and are never issued to memory.  The full rounds carry no test at all
    auto fetch = [&](auto tail, const int k, const int gb, const unsigned (&wb)[NB], const unsigned xb) {
        constexpr bool TAIL = decltype(tail)::value;
        const unsigned dead = TAIL && gb + k >= sn ? kOOB : 0u;           // (uniform: a scalar select)
#pragma unroll
        for (int j = 0; j < NB; ++j) {
            wr[k][j] = __builtin_bit_cast(v2u, __builtin_amdgcn_raw_buffer_load_b64(rW, (int)((wb[j] + (unsigned)k * kWGroup) | dead), 0, 0));
            sr[k][j] = __builtin_amdgcn_raw_buffer_load_b32(rS, (int)((soff[j] + (unsigned)(gb + k) * sstep) | dead), 0, 0);
        }
        xr[k] = __builtin_amdgcn_raw_buffer_load_b128(rX, (int)((xb + (unsigned)k * kGroup) | dead), 0, 0);
    };
    float acc[NB][4];
#pragma unroll
    for (int j = 0; j < NB; ++j)
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[j][i] = 0.f;
#pragma unroll
    for (int k = 0; k < D; ++k) fetch(SkinnyTail<true>{}, k, 0, woff, xoff);
    const v4i ones = {0x01010101, 0x01010101, 0x01010101, 0x01010101}, z = {0, 0, 0, 0};
    auto round = [&](auto tail, const int g0) {                          // consumes groups g0 .. g0 + D - 1, requests g0 + D .. g0 + 2 D - 1 into their slots
        unsigned wb[NB];
#pragma unroll
        for (int j = 0; j < NB; ++j) wb[j] = woff[j] + (unsigned)(g0 + D) * kWGroup;
        const unsigned xb = xoff + (unsigned)(g0 + D) * kGroup;
#pragma unroll
        for (int k = 0; k < D; ++k) {
            const int g = g0 + k;                                           // (g >= sn in the last round: zero activations, zero scales)
            const float4 sx = *reinterpret_cast<const float4*>(sxl + g * kSkinnyTokens + 4 * q);
            const v4i x = __builtin_bit_cast(v4i, xr[k]);
            const v4i sum = __builtin_amdgcn_mfma_i32_16x16x64_i8(x, ones, z, 0, 0, 0);      // sum x of tokens 4 q .. 4 q + 3, in every column
            const v4i off = {__mul24(sum[0], -8), __mul24(sum[1], -8), __mul24(sum[2], -8), __mul24(sum[3], -8)};      // (|sum x| <= 64 * 127: 14 bits)
#pragma unroll
            for (int j = 0; j < NB; ++j) {
                const v2u w = wr[k][j];
                const v4u u = {w[0] & kNib, (w[0] >> 4) & kNib, w[1] & kNib, (w[1] >> 4) & kNib};
                const v4i d = __builtin_amdgcn_mfma_i32_16x16x64_i8(x, __builtin_bit_cast(v4i, u), off, 0, 0, 0);
                const float sw = __uint_as_float(sr[k][j]);
                acc[j][0] = __fmaf_rn(__fmul_rn(sw, sx.x), (float)d[0], acc[j][0]);   // quant_operators.cpp:274
                acc[j][1] = __fmaf_rn(__fmul_rn(sw, sx.y), (float)d[1], acc[j][1]);
                acc[j][2] = __fmaf_rn(__fmul_rn(sw, sx.z), (float)d[2], acc[j][2]);
                acc[j][3] = __fmaf_rn(__fmul_rn(sw, sx.w), (float)d[3], acc[j][3]);
            }
            fetch(tail, k, g0 + D, wb, xb);
        }
    };
    int g0 = 0;
    for (; g0 + 2 * D <= sn; g0 += D) round(SkinnyTail<false>{}, g0);
    for (; g0 < sn; g0 += D) round(SkinnyTail<true>{}, g0);
    skinny_epilogue<EPI, NB>(a, acc, r0 + l15, lane);
}

// ------------------------------------------------------------------------------------------
// The skinny int16 GEMM: k_gemm_q8_skinny's contract once more (tokens = A, weight rows = B of v_mfma_i32_16x16x64_i8, C/D col = lane & 15 = the weight row, row = 4 (lane
// >> 4) + reg = the token, one wave per workgroup, activation scales [groups][16] in LDS, the chain step and skinny_epilogue unchanged) with k_gemm_q16_mfma's arithmetic:
// gfx950 has no int16 MFMA, a value is two signed bytes (split16: w = 256 wh + wl) and a group's dot four int8 products on ONE accumulator.
//   * operand: lane (l15, q) owns elements 16 q .. 16 q + 15 of group g of its row = the 32 bytes at row * 2 n + 128 g + 32 q, two 16-byte buffer loads.  split16 turns each
//     piece, in registers, into 8 low and 8 high bytes; the lane ends with two v4i operands wl and wh whose byte k is element 16 q + k.  The activation side is the same
//     (token l15's 32 bytes -> xl, xh; the split is shared by the NB fragments).  A and B use the same byte -> k assignment, and integer sums are order-free.
//   * four MFMAs per fragment and group: d = S(xh, wh); d <<= 8; d += S(xh, wl) + S(xl, wh); d <<= 8; d += S(xl, wl) -- the accumulator INPUT carries the shifted sum,
//     everything mod 2^32, landing on the true int32 group dot (64 * 5792^2 < 2^31: the reference's own int32).  The shifts are 4 VALU each.
//   * ring: a slot is 8 NB + 8 registers of operands plus NB scales; D groups of all three streams are in flight (equal depths: a wave's loads return in issue order, see
//     k_gemm_q4_skinny).  Nothing but the activation scales is staged in LDS.  The full rounds carry no bounds test.
//   * zeros: a zero word is eight zero weights in both planes.  Rows past the matrix read zero weights and zero scales and are masked at the store; groups past the end
//     (the ring's last round) and token columns >= B read zero activations and zero scales: fma(0 * 0, float(0), acc) = acc.
//   num_records of the weight descriptor is in BYTES: rows * 2 n (SWIGLU: of both halves).
// ------------------------------------------------------------------------------------------
__host__ __device__ constexpr int skinny16_depth(int nb) { return nb == 1 ? 10 : 6; }                    // groups in flight per wave
__host__ __device__ inline int skinny16_groups_padded(int sn, int nb) { const int d = skinny16_depth(nb); return (sn + d - 1) / d * d + d; }
__host__ __device__ inline size_t skinny16_lds_bytes(int n, int nb) { return (size_t)skinny16_groups_padded(n / kGroup, nb) * kSkinnyTokens * 4; }
// grid: ceil(rows / (16 NB)) workgroups of 64 threads (SWIGLU: ceil(rows / 16), NB = 2); skinny16_lds_bytes(n, NB) of dynamic LDS; B <= 16; single GPU (no peers)
// waves_per_eu(2): at most 256 registers to a wave, so that the MFMA results stay in VGPRs (see k_gemm_q4_skinny)
template <int EPI, int NB>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2))) k_gemm_q16_skinny(const GemmArgs a) {
    constexpr bool TWO = EPI == EPI_SWIGLU;
    static_assert(!TWO || NB == 2, "gate and up are the two B fragments of the wave");
    constexpr int D = skinny16_depth(NB);
    extern __shared__ __attribute__((aligned(16))) char lds[];
    float* const sxl = reinterpret_cast<float*>(lds);                       // [groups, padded][16 tokens]
    const int lane = threadIdx.x, l15 = lane & 15, q = lane >> 4;
    const int sn = a.n / kGroup, snp = skinny16_groups_padded(sn, NB);
    const int r0 = blockIdx.x * (TWO ? 16 : 16 * NB);
    for (int i = lane; i < snp * kSkinnyTokens; i += 64) { const int g = i >> 4, b = i & 15; sxl[i] = (g < sn && b < a.B) ? a.Xs[(size_t)b * sn + g] : 0.0f; }
    __syncthreads();
    const unsigned rowbytes = (unsigned)a.n * 2;                            // a row of either side
    constexpr unsigned kOOB = 0x80000000u, kGB = kGroup * 2;
    const unsigned s_rows = (TWO ? 2u : 1u) * (unsigned)a.rows;
    const __amdgpu_buffer_rsrc_t rW = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(a.W), 0, (int)(s_rows * rowbytes), 0x00020000);
    const __amdgpu_buffer_rsrc_t rX = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(a.Xq), 0, (int)((unsigned)a.B * rowbytes), 0x00020000);
    const __amdgpu_buffer_rsrc_t rS = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.sWT), 0, (int)(s_rows * (unsigned)sn * 4), 0x00020000);
    // fragment j: rows r0 + 16 j .. (SWIGLU: rows r0 .. of W1 (j = 0) and of W3 (j = 1)).  A dead lane (a row past the matrix, a token column >= B) carries bit 31 in its
    // offsets, a dead group ORs it in: an offset of 2^31 or more is out of range of every descriptor here (the launcher bounds them), and no sum below wraps
    unsigned woff[NB], soff[NB];
#pragma unroll
    for (int j = 0; j < NB; ++j) {
        const int row = r0 + (TWO ? 0 : 16 * j) + l15;
        const unsigned wrow = (unsigned)(TWO ? j * a.rows + row : row);
        woff[j] = row < a.rows ? wrow * rowbytes + (unsigned)q * 32 : kOOB;
        soff[j] = row < a.rows ? wrow * 4 : kOOB;
    }
    const unsigned xoff = l15 < a.B ? (unsigned)l15 * rowbytes + (unsigned)q * 32 : kOOB;
    const unsigned sstep = s_rows * 4;
    v4u wr[D][NB][2], xr[D][2]; unsigned sr[D][NB];
    // groups gb + k -> ring slot k; TAIL: the round may run past the last group -- those loads go out of range and are never issued to memory
    auto fetch = [&](auto tail, const int k, const int gb, const unsigned (&wb)[NB], const unsigned xb) {
        constexpr bool TAIL = decltype(tail)::value;
        const unsigned dead = TAIL && gb + k >= sn ? kOOB : 0u;           // (uniform: a scalar select)
#pragma unroll
        for (int j = 0; j < NB; ++j) {
            wr[k][j][0] = __builtin_amdgcn_raw_buffer_load_b128(rW, (int)((wb[j] + (unsigned)k * kGB) | dead), 0, 0);
            wr[k][j][1] = __builtin_amdgcn_raw_buffer_load_b128(rW, (int)((wb[j] + (unsigned)k * kGB + 16u) | dead), 0, 0);
            sr[k][j] = __builtin_amdgcn_raw_buffer_load_b32(rS, (int)((soff[j] + (unsigned)(gb + k) * sstep) | dead), 0, 0);
        }
        xr[k][0] = __builtin_amdgcn_raw_buffer_load_b128(rX, (int)((xb + (unsigned)k * kGB) | dead), 0, 0);
        xr[k][1] = __builtin_amdgcn_raw_buffer_load_b128(rX, (int)((xb + (unsigned)k * kGB + 16u) | dead), 0, 0);
    };
    auto planes = [](const v4u (&p)[2], v4i& lo, v4i& hi) {                // 32 bytes = 16 int16 -> their low and their (carry-corrected) high bytes, element order
        unsigned l0[2], h0[2], l1[2], h1[2];
        split16(__builtin_bit_cast(v4i, p[0]), l0, h0); split16(__builtin_bit_cast(v4i, p[1]), l1, h1);
        lo = v4i{(int)l0[0], (int)l0[1], (int)l1[0], (int)l1[1]}; hi = v4i{(int)h0[0], (int)h0[1], (int)h1[0], (int)h1[1]};
    };
    float acc[NB][4];
#pragma unroll
    for (int j = 0; j < NB; ++j)
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[j][i] = 0.f;
#pragma unroll
    for (int k = 0; k < D; ++k) fetch(SkinnyTail<true>{}, k, 0, woff, xoff);
    auto round = [&](auto tail, const int g0) {                          // consumes groups g0 .. g0 + D - 1, requests g0 + D .. g0 + 2 D - 1 into their slots
        unsigned wb[NB];
#pragma unroll
        for (int j = 0; j < NB; ++j) wb[j] = woff[j] + (unsigned)(g0 + D) * kGB;
        const unsigned xb = xoff + (unsigned)(g0 + D) * kGB;
#pragma unroll
        for (int k = 0; k < D; ++k) {
            const int g = g0 + k;                                           // (g >= sn in the last round: zero activations, zero scales)
            const float4 sx = *reinterpret_cast<const float4*>(sxl + g * kSkinnyTokens + 4 * q);
            v4i xl, xh; planes(xr[k], xl, xh);
#pragma unroll
            for (int j = 0; j < NB; ++j) {
                v4i wl, wh; planes(wr[k][j], wl, wh);
                const v4i z = {0, 0, 0, 0};
                v4i d = __builtin_amdgcn_mfma_i32_16x16x64_i8(xh, wh, z, 0, 0, 0);
#pragma unroll
                for (int i = 0; i < 4; ++i) d[i] = (int)((unsigned)d[i] << 8);
                d = __builtin_amdgcn_mfma_i32_16x16x64_i8(xh, wl, d, 0, 0, 0);
                d = __builtin_amdgcn_mfma_i32_16x16x64_i8(xl, wh, d, 0, 0, 0);
#pragma unroll
                for (int i = 0; i < 4; ++i) d[i] = (int)((unsigned)d[i] << 8);
                d = __builtin_amdgcn_mfma_i32_16x16x64_i8(xl, wl, d, 0, 0, 0);                  // wraps mod 2^32 onto the exact int32 dot
                const float sw = __uint_as_float(sr[k][j]);
                acc[j][0] = __fmaf_rn(__fmul_rn(sw, sx.x), (float)d[0], acc[j][0]);   // quant_operators.cpp:274
                acc[j][1] = __fmaf_rn(__fmul_rn(sw, sx.y), (float)d[1], acc[j][1]);
                acc[j][2] = __fmaf_rn(__fmul_rn(sw, sx.z), (float)d[2], acc[j][2]);
                acc[j][3] = __fmaf_rn(__fmul_rn(sw, sx.w), (float)d[3], acc[j][3]);
            }
            fetch(tail, k, g0 + D, wb, xb);
        }
    };
    int g0 = 0;
    for (; g0 + 2 * D <= sn; g0 += D) round(SkinnyTail<false>{}, g0);
    for (; g0 < sn; g0 += D) round(SkinnyTail<true>{}, g0);
    skinny_epilogue<EPI, NB>(a, acc, r0 + l15, lane);
}

// ------------------------------------------------------------------------------------------
// The W4A8 GEMM tiles: k_gemm_q8_mfma's contract (GemmArgs, the tile shapes <2, 2, 1> and <4, 2, 2>, tokens = A of v_mfma_i32_32x32x32_i8 so that a lane owns ONE weight
// row, tiles dealt to the XCDs in contiguous runs, both sides' scales from the group-major copies, the step acc = fma(sw * sx, float(d), acc) with groups ascending,
// gemm_epilogue as it is) on a matrix in the DEVICE nibble layout (flm_gemv4.h) -- a.W is [rows][n / 2] packed bytes (SWIGLU: W3 behind W1); nothing is unpacked to
// memory and nothing is expanded on the way into LDS.  The stored value is, bit for bit, what k_gemm_q8_mfma stores for the sign-extended nibbles.
//   * staging: a stage is still kGPS = 2 groups = 64 PACKED bytes of a weight row: four 16-byte pieces per row, parked as they come -- half the global bytes, half the
//     LDS stores and half the LDS bytes per weight row of the int8 kernel, whose bound is the LDS.  X is staged as there (128 bytes per token and stage).
//     LDS row stride of the packed strip: 80 bytes = 20 banks; the eight lanes one cycle of a 16-byte read serves are eight consecutive rows, starting at banks 20 r mod
//     32 = {0, 20, 8, 28, 16, 4, 24, 12}: four banks each, all 32 once (GemmTile::LS = 144 does the same for 128-byte rows).  The STORES need the loader's row order
//     below.  SQ_LDS_BANK_CONFLICT is 0 with both.
//   * operand: lane (l31, h) reads ONE 16-byte piece per fragment and group: packed bytes 16 h .. 16 h + 15 of group g of its row = weights 32 h .. 32 h + 31.  Its words
//     w0 .. w3 expand as in k_gemm_q4_skinny, M = 0x0F0F0F0F: {w0 & M, (w0 >> 4) & M, w1 & M, (w1 >> 4) & M} = weights 32 h .. 32 h + 15 in column order is the B operand
//     of the group's first MFMA, the same of w2, w3 (weights 32 h + 16 .. 32 h + 31) of the second: 12 VALU per fragment and group, one ds_read_b128 where the int8
//     kernel issues two.  The A side follows (integer group sums are order-free as long as A and B agree): lane half h takes activation bytes 32 h .. 32 h + 15 for the
//     first MFMA and 32 h + 16 .. 32 h + 31 for the second (int8: 16 h .. and 32 + 16 h ..).
//   * the offset leaves once per group, exactly: sum (u - 8) x = sum u x - 8 sum x.  Two MFMAs per group and wave with B = 0x01010101 give sum x of every token in the C
//     layout (every column alike); times -8 (16 VALU, shared by the NB fragments) it is the accumulator INPUT of the fragment MFMAs, whose result is the exact int32 dot
//     of the sign-extended nibbles (|sum u x| <= 64 * 15 * 127).  No table of sum x, nothing folded into the scales (sw * sx stays the int8 kernel's product).
//   * zeros: a zero WORD is now eight weights of -8, not 0.  (1) Rows past the matrix: weight loads out of range (d = -8 sum x) and scale loads too -- sw = 0,
//     fma(0 * sx, float(d), acc) = acc -- and gemm_epilogue masks them at the store.  (2) Token columns >= B: zero ACTIVATIONS, so sum x = 0 and every product is 0:
//     d = 0 whatever the weight words are.  (3) The half stage behind an odd group count (and the stages past the end): whatever bytes lie there, the scale load is
//     refused (sw = 0), as in the int8 kernel.
//   num_records of the weight descriptor is in BYTES of the packed matrix (SWIGLU: of both halves); n_peer is 0 (INT4 is one GPU's).
// ------------------------------------------------------------------------------------------
template <int WT, int WR, int NB>
struct GemmTile4 {
    static constexpr int TT = 32 * WT, TR = 32 * NB * WR, NT = 64 * WT * WR;
    static constexpr int SBX = kGPS * kGroup, SBW = SBX / 2;      // bytes of a stage in one token's row | in one packed weight row
    static constexpr int LSX = SBX + 16, LSW = SBW + 16;          // LDS row strides (conflict-free 16-byte reads of 16 consecutive rows, see above)
    static constexpr int kOffX = TR * LSW, kOffS = kOffX + TT * LSX, kBuf = kOffS + kGPS * (TR + TT) * 4;   // packed W rows | X rows | scales [W g0][W g1][X g0][X g1]
    static constexpr int NPW = TR * 4 / NT, NPX = TT * 8 / NT;    // 16-byte pieces per thread and stage
    static constexpr int kLds = 2 * kBuf;
    static_assert(kGPS == 2 && NT == kGPS * (TR + TT) && TR % 64 == 0 && TT % 64 == 0, "one scale per thread and stage, wave-uniform (matrix, group)");
    static_assert(TR * 4 % NT == 0 && TT * 8 % NT == 0, "whole pieces per thread");
    static_assert(kLds <= 64 * 1024, "both shapes fit the default dynamic-LDS limit (128 x 128: 60 KiB, two workgroups per CU; 64 x 64: 30 KiB, four)");
};
template <int EPI, int WT, int WR, int NB>
__global__ void __launch_bounds__(64 * WT * WR, 4) k_gemm_q4_mfma(const GemmArgs a) {
    using G = GemmTile4<WT, WR, NB>;
    constexpr bool TWO = EPI == EPI_SWIGLU;
    static_assert(!TWO || NB == 2, "gate and up are the two B fragments of a wave");
    constexpr int TRH = TWO ? G::TR / 2 : G::TR;              // rows of a.rows one tile advances
    constexpr int SBX = G::SBX, SBW = G::SBW, LSX = G::LSX, LSW = G::LSW, TT = G::TT, TR = G::TR, NT = G::NT, kOffX = G::kOffX, kOffS = G::kOffS, kBuf = G::kBuf, NPW = G::NPW, NPX = G::NPX;
    constexpr int kWGroup = kGroup / 2;                       // packed bytes of a quant group
    extern __shared__ __attribute__((aligned(16))) char lds[]; char* const sm = lds;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int ntt = (a.B + TT - 1) / TT;
    const int nb = gridDim.x, per = nb >> 3, rem = nb & 7, xcd = blockIdx.x & 7;              // tiles dealt to the XCDs in contiguous runs, token tile fastest (k_gemm_q8_mfma)
    const int tile = xcd * per + (xcd < rem ? xcd : rem) + (blockIdx.x >> 3);
    const int r0 = (tile / ntt) * TRH, b0 = (tile % ntt) * TT;
    const int sn = a.n / kGroup, nst = (sn + kGPS - 1) / kGPS;
    const unsigned xbytes = (unsigned)a.n, wbytes = (unsigned)a.n / 2;      // a row of activations, a row of packed weights
    constexpr unsigned kOOB = 0x80000000u, kNib = 0x0F0F0F0Fu;
    const __amdgpu_buffer_rsrc_t rW = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(a.W), 0, (int)((TWO ? 2u : 1u) * (unsigned)a.rows * wbytes), 0x00020000);
    // tile row -> row of W (or -1): SWIGLU tiles hold TRH rows of W1, then the same TRH rows of W3
    auto wrow = [&](int tr) -> int { const int within = TWO ? tr % TRH : tr, r = r0 + within; return r < a.rows ? (TWO ? (tr / TRH) * a.rows + r : r) : -1; };
    const __amdgpu_buffer_rsrc_t rX = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(a.Xq), 0, (int)((unsigned)a.B * xbytes), 0x00020000);
    // loaders: weight piece k of a thread = 16 packed bytes at (row pwrow + (NT / 4) k, chunk tid & 3); activation piece k = 16 bytes at (token (tid >> 3) + (NT / 8) k,
    // chunk tid & 7); rows outside a matrix read as zero
    // The eight lanes one cycle of a 16-byte LDS store serves write two weight rows' four pieces: 2 x 64 bytes must be all 32 banks once, and rows r, r + 1 at stride 80
    // share four (measured: SQ_LDS_BANK_CONFLICT at 9 % of the active cycles, every one from this store).  Rows r and r + 4 lie 320 = 64 mod 128 bytes apart: inside every
    // eight rows, lane pairs take the rows in the order 0 4 1 5 2 6 3 7.
    const int pwq = tid >> 2, pwrow = (pwq & ~7) | ((pwq & 1) << 2) | ((pwq >> 1) & 3), pwch = tid & 3, pxrow = tid >> 3, pxch = tid & 7;
    unsigned woff[NPW], xoff[NPX];
#pragma unroll
    for (int k = 0; k < NPW; ++k) { const int r = wrow(pwrow + (NT / 4) * k); woff[k] = r >= 0 ? (unsigned)r * wbytes + pwch * 16 : kOOB; }
#pragma unroll
    for (int k = 0; k < NPX; ++k) xoff[k] = (b0 + pxrow + (NT / 8) * k < a.B) ? (unsigned)(b0 + pxrow + (NT / 8) * k) * xbytes + pxch * 16 : kOOB;
    const unsigned pwoff = (unsigned)(pwrow * LSW + pwch * 16), pxoff = (unsigned)(kOffX + pxrow * LSX + pxch * 16);
    // scales: one per thread and stage from the group-major copies, LDS slots [W g0 (TR)][W g1 (TR)][X g0 (TT)][X g1 (TT)], a group past the end gets scale zero (k_gemm_q8_mfma)
    const int s_slot = wave * 64;
    const bool s_x = s_slot >= kGPS * TR;
    const int s_gi = s_x ? (s_slot - kGPS * TR) / TT : s_slot / TR;
    const int s_row = s_x ? (b0 + (s_slot - kGPS * TR) % TT + lane < a.B ? b0 + (s_slot - kGPS * TR) % TT + lane : -1) : wrow(s_slot % TR + lane);
    const unsigned s_rows = s_x ? (unsigned)a.B : (TWO ? 2u : 1u) * (unsigned)a.rows;
    const __amdgpu_buffer_rsrc_t rS = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(s_x ? a.XsT : a.sWT), 0, (int)(s_rows * sn * 4), 0x00020000);
    unsigned soff = s_row >= 0 ? ((unsigned)s_gi * s_rows + s_row) * 4 : kOOB;
    const unsigned sstep = kGPS * s_rows * 4;
    const unsigned spoff = (unsigned)(kOffS + tid * 4);
    v4u wr[NPW], xr[NPX]; unsigned sr;
    auto fetch = [&](int st) {                    // stage st -> the register slot (stages past the end: the offsets have run past the rows; never consumed with a non-zero scale)
#pragma unroll
        for (int k = 0; k < NPW; ++k) { wr[k] = __builtin_amdgcn_raw_buffer_load_b128(rW, (int)woff[k], 0, 0); woff[k] += SBW; }
#pragma unroll
        for (int k = 0; k < NPX; ++k) { xr[k] = __builtin_amdgcn_raw_buffer_load_b128(rX, (int)xoff[k], 0, 0); xoff[k] += SBX; }
        sr = __builtin_amdgcn_raw_buffer_load_b32(rS, (int)(st * kGPS + s_gi < sn ? soff : kOOB), 0, 0); soff += sstep;
    };
    auto park = [&](int buf) {
        char* base = sm + buf * kBuf;
#pragma unroll
        for (int k = 0; k < NPW; ++k) *reinterpret_cast<v4u*>(base + pwoff + k * (NT / 4) * LSW) = wr[k];
#pragma unroll
        for (int k = 0; k < NPX; ++k) *reinterpret_cast<v4u*>(base + pxoff + k * (NT / 8) * LSX) = xr[k];
        *reinterpret_cast<unsigned*>(base + spoff) = sr;
    };
    // this wave's 32 tokens x (NB x 32) weight rows (SWIGLU: fragment j = rows wr0 .. wr0 + 31 of half j; otherwise fragment j = tile rows wr0 + 32 j ..)
    const int wt0 = (wave % WT) * 32, wr0 = (wave / WT) * 32 * (TWO ? 1 : NB), l31 = lane & 31, h = lane >> 5;
    constexpr int FS = TWO ? TRH : 32;                            // tile rows between a wave's fragments
    const unsigned offA = (unsigned)(kOffX + (wt0 + l31) * LSX + h * 32), offB = (unsigned)((wr0 + l31) * LSW + h * 16);
    const unsigned offsw = (unsigned)(kOffS + (wr0 + l31) * 4), offsx = (unsigned)(kOffS + (kGPS * TR + wt0 + 4 * h) * 4);
    float acc[NB][16];
#pragma unroll
    for (int j = 0; j < NB; ++j)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[j][i] = 0.f;
    const v4i ones = {0x01010101, 0x01010101, 0x01010101, 0x01010101};
    fetch(0); park(0); fetch(1);
    __syncthreads();
    for (int st = 0; st < nst; ++st) {
        const char* base = sm + (st & 1) * kBuf;
#pragma unroll
        for (int gi = 0; gi < kGPS; ++gi) {
            const v4i a0 = *reinterpret_cast<const v4i*>(base + offA + gi * kGroup), a1 = *reinterpret_cast<const v4i*>(base + offA + gi * kGroup + 16);
            const v16i z = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
            v16i off = __builtin_amdgcn_mfma_i32_32x32x32_i8(a0, ones, z, 0, 0, 0);      // sum x of the wave's tokens in the C layout, in every column
            off = __builtin_amdgcn_mfma_i32_32x32x32_i8(a1, ones, off, 0, 0, 0);
#pragma unroll
            for (int i = 0; i < 16; ++i) off[i] = __mul24(off[i], -8);                  // (|sum x| <= 64 * 127: 14 bits)
            v16i d[NB];
#pragma unroll
            for (int j = 0; j < NB; ++j) {
                const v4u w = *reinterpret_cast<const v4u*>(base + offB + j * FS * LSW + gi * kWGroup);
                const v4u u0 = {w[0] & kNib, (w[0] >> 4) & kNib, w[1] & kNib, (w[1] >> 4) & kNib}, u1 = {w[2] & kNib, (w[2] >> 4) & kNib, w[3] & kNib, (w[3] >> 4) & kNib};
                d[j] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a0, __builtin_bit_cast(v4i, u0), off, 0, 0, 0);
                d[j] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a1, __builtin_bit_cast(v4i, u1), d[j], 0, 0, 0);
            }
            float4 sx[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) sx[q] = *reinterpret_cast<const float4*>(base + offsx + gi * TT * 4 + q * 32);
#pragma unroll
            for (int j = 0; j < NB; ++j) {
                const float sw = *reinterpret_cast<const float*>(base + offsw + (gi * TR + j * FS) * 4);
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    acc[j][4 * q + 0] = __fmaf_rn(__fmul_rn(sw, sx[q].x), (float)d[j][4 * q + 0], acc[j][4 * q + 0]);   // quant_operators.cpp:274
                    acc[j][4 * q + 1] = __fmaf_rn(__fmul_rn(sw, sx[q].y), (float)d[j][4 * q + 1], acc[j][4 * q + 1]);
                    acc[j][4 * q + 2] = __fmaf_rn(__fmul_rn(sw, sx[q].z), (float)d[j][4 * q + 2], acc[j][4 * q + 2]);
                    acc[j][4 * q + 3] = __fmaf_rn(__fmul_rn(sw, sx[q].w), (float)d[j][4 * q + 3], acc[j][4 * q + 3]);
                }
            }
        }
        park((st & 1) ^ 1); fetch(st + 2);        // unconditional: a stage past the end is parked and never read with a non-zero scale
        __syncthreads();
    }
    gemm_epilogue<EPI, NB>(a, acc, r0 + wr0 + l31, b0 + wt0, lane);
}

// qkv[b] = [q ; k ; v] (dim each) of token b at position pos0 + b: RoPE on q and k (rope_v2 pairs), q -> qout[b], k / v -> cache rows
inline __global__ void k_rope_kv_rows(const float* qkv, float* qout, float* kcache, float* vcache, const float* rope_cos, const float* rope_sin,
                               int dim, int hs, int max_seq, int pos0) {
    const int b = blockIdx.x, pos = pos0 + b;
    const float* in = qkv + (size_t)b * 3 * dim;
    for (int i = threadIdx.x; i < dim / 2; i += blockDim.x) {
        const int row = 2 * i, h = row / hs, d = row - h * hs;
        const float c = rope_cos[(size_t)pos * (hs / 2) + d / 2], s = rope_sin[(size_t)pos * (hs / 2) + d / 2];
        float o0, o1;
        rope_pair(in[row], in[row + 1], c, s, o0, o1);
        qout[(size_t)b * dim + row] = o0; qout[(size_t)b * dim + row + 1] = o1;
        rope_pair(in[dim + row], in[dim + row + 1], c, s, o0, o1);
        float* kp = kcache + ((size_t)h * max_seq + pos) * hs + d; kp[0] = o0; kp[1] = o1;
        float* vp = vcache + ((size_t)h * max_seq + pos) * hs + d; vp[0] = in[2 * dim + row]; vp[1] = in[2 * dim + row + 1];
    }
}

// gu[b] = [gate ; up] (hidden each, this rank's slice) -> hd[b * ldo + i]; tensor parallel: hd = this rank's columns of every rank's [tokens][hidden_dim]
struct SwigluPeers { float* p[7]; int n; };
inline __global__ void k_swiglu_rows(float* hd, const float* gu, int hidden, int ldo, const SwigluPeers peers) {
    const float* g = gu + (size_t)blockIdx.x * 2 * hidden;
    for (int i = threadIdx.x; i < hidden; i += blockDim.x) st_result_tp(hd, (size_t)blockIdx.x * ldo + i, swiglu_elem(g[i], g[hidden + i]), peers.p, peers.n);   // o1.swiglu(o3) transformer.cpp:481
}

} // namespace flm
