// flm_ops.hip -- op-level exports (flm_op_*): 1:1 mirrors of the reference operator seam, host pointers in / out, running the same device code as the token
// path.  Used by the parity tests.
#include "flm_host.h"

namespace {
struct DevBuf {
    void* p = nullptr;
    ~DevBuf() { if (p) hipFree(p); }
    int alloc(size_t n) { return hipMalloc(&p, n ? n : 4) == hipSuccess ? 0 : 1; }
    template <class T> T* as() { return reinterpret_cast<T*>(p); }
};
#define OPC(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) { g_last_error = std::string(#expr " failed: ") + hipGetErrorString(e_); return FLM_ERR_HIP; } } while (0)
}

extern "C" {

// ---------------------------------------------------------------------------------------------
// op-level exports
// ---------------------------------------------------------------------------------------------

int flm_op_quantize(int qt, void* qx, float* qs, const float* x, size_t n, int gs) {
    if (!qx || !qs || !x || gs != kGroup || n % kGroup) return FLM_ERR_INVALID;
    if (qt != FLM_QT_INT8 && qt != FLM_QT_INT16) return FLM_ERR_UNSUPPORTED;
    const int e = esz_of(qt);
    DevBuf dx, dq, ds;
    if (dx.alloc(n * 4) || dq.alloc(n * e) || ds.alloc(n / kGroup * 4)) return FLM_ERR_OOM;
    OPC(hipMemcpy(dx.p, x, n * 4, hipMemcpyHostToDevice));
    if (n <= 16384) {
        // through the fused path's prologue (PRO_QUANT), tapped
        GemvArgs a{}; a.n = (int)n; a.items = 0; a.x = dx.as<float>(); a.dbg_xq = dq.p; a.dbg_xs = ds.as<float>();
        int r = launch_gemv<PRO_QUANT, EPI_STORE>(nullptr, 0, qt, a, 1); if (r) return r;
    } else {
        int r = quantize_flat(nullptr, 0, qt, dq.p, ds.as<float>(), dx.as<float>(), n); if (r) return r;
    }
    OPC(hipDeviceSynchronize());
    OPC(hipMemcpy(qx, dq.p, n * e, hipMemcpyDeviceToHost));
    OPC(hipMemcpy(qs, ds.p, n / kGroup * 4, hipMemcpyDeviceToHost));
    return FLM_OK;
}

// square_sum (x86_simd.cpp:942-960) of x[n], n a multiple of 16: out6 = { speculative wave evaluation (sq_chain_spec), sequential total, the 4 strided lanes }
int flm_op_square_sum(const float* x, size_t n, float* out6) {
    if (!x || !out6 || n % 16 || n == 0 || n > 16384) return FLM_ERR_INVALID;
    DevBuf dx, dout;
    if (dx.alloc(n * 4) || dout.alloc(16 * 4)) return FLM_ERR_OOM;
    OPC(hipMemcpy(dx.p, x, n * 4, hipMemcpyHostToDevice));
    const size_t lds = ((size_t)4 * chain_strip_floats((int)n) + 4 * (n / 4 + 8)) * 4;
    hipLaunchKernelGGL(k_op_square_sum, dim3(1), dim3(256), lds, 0, dout.as<float>(), dx.as<float>(), (int)n);
    OPC(hipGetLastError()); OPC(hipDeviceSynchronize());
    OPC(hipMemcpy(out6, dout.p, 6 * 4, hipMemcpyDeviceToHost));
    if (getenv("FLM_SQ_ITERS")) { float it[6]; hipMemcpy(it, (char*)dout.p + 24, 24, hipMemcpyDeviceToHost); fprintf(stderr, "sq_chain_spec rounds per chain (-1: plain chain): %g %g %g %g; shader-clock ticks: speculative %g, plain %g\n", it[0], it[1], it[2], it[3], it[4], it[5]); }
    return FLM_OK;
}

// the fused launches' publish / poll / coherent-read sequence, `rounds` times on one 256-thread workgroup per CU (k_handoff_litmus, flm_misc.h)
int flm_op_handoff_litmus(int rounds, int* wrong_values, int* timed_out) {
    if (rounds < 1 || !wrong_values || !timed_out) return FLM_ERR_INVALID;
    int dev = 0; OPC(hipGetDevice(&dev));
    hipDeviceProp_t pr; OPC(hipGetDeviceProperties(&pr, dev));
    const int G = pr.multiProcessorCount < 256 ? pr.multiProcessorCount : 256;
    DevBuf pay, fl, er;
    if (pay.alloc((size_t)2 * G * 64 * 4) || fl.alloc((size_t)G * 64) || er.alloc(8)) return FLM_ERR_OOM;
    OPC(hipMemset(pay.p, 0, (size_t)2 * G * 64 * 4)); OPC(hipMemset(fl.p, 0, (size_t)G * 64)); OPC(hipMemset(er.p, 0, 8));
    hipLaunchKernelGGL(k_handoff_litmus, dim3(G), dim3(256), 0, 0, pay.as<float>(), fl.as<unsigned>(), rounds, er.as<int>(), er.as<int>() + 1);
    OPC(hipGetLastError()); OPC(hipDeviceSynchronize());
    int h[2] = {0, 0};
    OPC(hipMemcpy(h, er.p, 8, hipMemcpyDeviceToHost));
    *wrong_values = h[0]; *timed_out = h[1];
    return FLM_OK;
}

int flm_op_rmsnorm(float* o, const float* x, const float* w, size_t n) {
    if (!o || !x || !w || n % kGroup || n > 16384 || n == 0) return FLM_ERR_INVALID;
    DevBuf dx, dw, dn, dq, ds;
    if (dx.alloc(n * 4) || dw.alloc(n * 4) || dn.alloc(n * 4) || dq.alloc(n) || ds.alloc(n / kGroup * 4)) return FLM_ERR_OOM;
    OPC(hipMemcpy(dx.p, x, n * 4, hipMemcpyHostToDevice)); OPC(hipMemcpy(dw.p, w, n * 4, hipMemcpyHostToDevice));
    GemvArgs a{}; a.n = (int)n; a.items = 0; a.x = dx.as<float>(); a.norm_w = dw.as<float>();
    a.dbg_xn = dn.as<float>(); a.dbg_xq = dq.p; a.dbg_xs = ds.as<float>();
    int r = launch_gemv<PRO_RMSNORM_QUANT, EPI_STORE>(nullptr, 0, FLM_QT_INT8, a, 1); if (r) return r;
    OPC(hipDeviceSynchronize());
    OPC(hipMemcpy(o, dn.p, n * 4, hipMemcpyDeviceToHost));
    return FLM_OK;
}

int flm_op_matmul_q(int qt, float* out, const void* W, const float* sW, const void* X, const float* sX, int m, int n, int w, int gs) {
    if (!out || !W || !sW || !X || !sX || m < 1 || n < 1 || w < 1 || gs != kGroup || n % kGroup) return FLM_ERR_INVALID;
    if (qt != FLM_QT_INT8 && qt != FLM_QT_INT16) return FLM_ERR_UNSUPPORTED;
    const size_t e = esz_of(qt), sn = n / kGroup;
    DevBuf dW, dsW, dX, dsX, dsXT, dsWT, dO;
    if (dW.alloc((size_t)m * n * e) || dsW.alloc((size_t)m * sn * 4) || dX.alloc((size_t)w * n * e) || dsX.alloc((size_t)w * sn * 4) || dsXT.alloc((size_t)w * sn * 4 + 64) || dsWT.alloc((size_t)m * sn * 4) || dO.alloc((size_t)w * m * 4)) return FLM_ERR_OOM;
    {   // the activation scales once more, group-major (k_rows_prologue writes both layouts on the prompt path)
        std::vector<float> t((size_t)w * sn);
        for (int b = 0; b < w; ++b) for (size_t g = 0; g < sn; ++g) t[g * w + b] = sX[(size_t)b * sn + g];
        OPC(hipMemcpy(dsXT.p, t.data(), t.size() * 4, hipMemcpyHostToDevice));
        std::vector<float> tw((size_t)m * sn);
        for (int r = 0; r < m; ++r) for (size_t g = 0; g < sn; ++g) tw[g * m + r] = sW[(size_t)r * sn + g];
        OPC(hipMemcpy(dsWT.p, tw.data(), tw.size() * 4, hipMemcpyHostToDevice));
    }
    OPC(hipMemcpy(dW.p, W, (size_t)m * n * e, hipMemcpyHostToDevice)); OPC(hipMemcpy(dsW.p, sW, (size_t)m * sn * 4, hipMemcpyHostToDevice));
    OPC(hipMemcpy(dX.p, X, (size_t)w * n * e, hipMemcpyHostToDevice)); OPC(hipMemcpy(dsX.p, sX, (size_t)w * sn * 4, hipMemcpyHostToDevice));
    int dev = 0, cus = 256; hipGetDevice(&dev); hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    const char* gv = getenv("FLM_OP_GEMM");                     // tests: 0 .. 3 = launch_gemm's use_mfma, "gemv" = a GEMV per batch row
    if (w >= 16 && !(gv && !strcmp(gv, "gemv"))) {
        // the batched path the prompt takes (quant::matmul with w > 1, quant_operators.cpp:252-284): one tile kernel
        GemmArgs g{dW.p, dsW.as<float>(), dX.p, dsX.as<float>(), dO.as<float>(), m, n, m, w, dsXT.as<float>(), dsWT.as<float>()};
        const int um = gv ? atoi(gv) : 1;
        int r = launch_gemm_store(nullptr, 0, qt, g, um);
        if (r) return r;
    } else {
        for (int b = 0; b < w; ++b) {
            GemvArgs a{}; a.W = dW.p; a.sW = dsW.as<float>(); a.n = n; a.items = m;
            a.xq = (const char*)dX.p + (size_t)b * n * e; a.xs = dsX.as<float>() + (size_t)b * sn; a.out = dO.as<float>() + (size_t)b * m;
            int r = launch_gemv<PRO_NONE, EPI_STORE>(nullptr, 0, qt, a, gemv_grid(cus, 1, m, 1)); if (r) return r;
        }
    }
    OPC(hipDeviceSynchronize());
    OPC(hipMemcpy(out, dO.p, (size_t)w * m * 4, hipMemcpyDeviceToHost));
    return FLM_OK;
}

/* quant::matmul for 1 <= w <= 16 batch rows through k_gemm_q8_skinny, the verify pass's int8 GEMM (plain store epilogue): out[w][m] */
int flm_op_matmul_skinny(int qt, float* out, const void* W, const float* sW, const void* X, const float* sX, int m, int n, int w, int gs) {
    if (!out || !W || !sW || !X || !sX || m < 1 || n < 1 || w < 1 || w > kSkinnyTokens || gs != kGroup || n % kGroup) return FLM_ERR_INVALID;
    if (qt != FLM_QT_INT8) return FLM_ERR_UNSUPPORTED;
    const size_t sn = n / kGroup;
    DevBuf dW, dsW, dX, dsX, dsWT, dO;
    if (dW.alloc((size_t)m * n) || dsW.alloc((size_t)m * sn * 4) || dX.alloc((size_t)w * n) || dsX.alloc((size_t)w * sn * 4) || dsWT.alloc((size_t)m * sn * 4) || dO.alloc((size_t)w * m * 4)) return FLM_ERR_OOM;
    {   // the weight scales once more, group-major (k_transpose_scales on the model path)
        std::vector<float> tw((size_t)m * sn);
        for (int r = 0; r < m; ++r) for (size_t g = 0; g < sn; ++g) tw[g * m + r] = sW[(size_t)r * sn + g];
        OPC(hipMemcpy(dsWT.p, tw.data(), tw.size() * 4, hipMemcpyHostToDevice));
    }
    OPC(hipMemcpy(dW.p, W, (size_t)m * n, hipMemcpyHostToDevice)); OPC(hipMemcpy(dsW.p, sW, (size_t)m * sn * 4, hipMemcpyHostToDevice));
    OPC(hipMemcpy(dX.p, X, (size_t)w * n, hipMemcpyHostToDevice)); OPC(hipMemcpy(dsX.p, sX, (size_t)w * sn * 4, hipMemcpyHostToDevice));
    OPC(hipMemset(dO.p, 0xff, (size_t)w * m * 4));                                      // (an output nobody stored reads as NaN)
    GemmArgs g{dW.p, dsW.as<float>(), dX.p, dsX.as<float>(), dO.as<float>(), m, n, m, w, nullptr, dsWT.as<float>()};
    const char* nb = getenv("FLM_OP_SKINNY_NB");                  // tests: 1 / 2 = fragments per wave (by size otherwise: two only from 8192 rows on)
    int r = launch_gemm_skinny_store(nullptr, 0, g, nb ? atoi(nb) : 0); if (r) return r;
    OPC(hipDeviceSynchronize());
    OPC(hipMemcpy(out, dO.p, (size_t)w * m * 4, hipMemcpyDeviceToHost));
    return FLM_OK;
}

/* k_spec_draft -- the prompt-lookup drafter of flm_generate_lookup -- on a caller-supplied history h[n]: d[k] */
int flm_op_spec_draft(const int32_t* h, int n, int k, int ngram_max, int32_t* d) {
    if (!h || !d || n < 1 || n >= (1 << 24) || k < 1 || k > 15 || ngram_max < 1 || ngram_max > 8) return FLM_ERR_INVALID;
    DevBuf dh, db;
    if (dh.alloc((size_t)n * 4) || db.alloc(16 * 4)) return FLM_ERR_OOM;
    OPC(hipMemcpy(dh.p, h, (size_t)n * 4, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_spec_draft, dim3(1), dim3(kSampleBlock), 0, 0, (const int*)dh.as<int>(), n, k, ngram_max, db.as<int>());
    OPC(hipGetLastError()); OPC(hipDeviceSynchronize());
    int32_t b[16];
    OPC(hipMemcpy(b, db.p, 16 * 4, hipMemcpyDeviceToHost));
    if (b[0] != h[n - 1]) return FLM_ERR_HIP;                                           // (row 0 of the batch is the history's last token)
    memcpy(d, b + 1, (size_t)k * 4);
    return FLM_OK;
}

/* the stop rules' matcher (flm_stop.h stop_match, the function the shaped token form runs in front of its last act) on caller-supplied ids: the first index that fires */
int flm_op_stop_match(const flm_stop_rules* r, int32_t stop_token, const int32_t* ids, int n, int* first, int* kind, int* rule) {
    if (!r || !ids || !first || !kind || !rule || n < 1 || n > (1 << 20)) return FLM_ERR_INVALID;
    for (int i = 0; i < n; ++i) if (ids[i] < 0) return FLM_ERR_INVALID;
    if (int rc = flm_stop_validate(r, 0x7fffffff)) return rc;                         // (the op has no model: any non-negative id is inside its vocabulary)
    StopBlock b{};
    b.n_ids = r->n_ids; b.n_seqs = r->n_seqs; b.n_tok = r->n_seqs > 0 ? r->seq_ptr[r->n_seqs] : 0;
    for (int i = 0; i < r->n_ids; ++i) b.ids[i] = r->ids[i];
    for (int s = 0; s <= r->n_seqs && r->n_seqs > 0; ++s) b.seq_ptr[s] = r->seq_ptr[s];
    for (int k = 0; k < b.n_tok; ++k) b.seq_tok[k] = r->seq_tokens[k];
    DevBuf db, di, dr;
    if (db.alloc(sizeof b) || di.alloc((size_t)n * 4) || dr.alloc(4 * 4)) return FLM_ERR_OOM;
    OPC(hipMemcpy(db.p, &b, sizeof b, hipMemcpyHostToDevice));
    OPC(hipMemcpy(di.p, ids, (size_t)n * 4, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_op_stop_match, dim3(1), dim3(1024), 0, 0, (const StopBlock*)db.as<StopBlock>(), (const int*)di.as<int>(), n, stop_token < 0 ? -1 : stop_token, dr.as<int>());
    OPC(hipGetLastError()); OPC(hipDeviceSynchronize());
    int res[3];
    OPC(hipMemcpy(res, dr.p, sizeof res, hipMemcpyDeviceToHost));
    *first = res[0]; *kind = res[1]; *rule = res[2];
    return FLM_OK;
}

/* sample_argmax (sampler.cpp:36-47) as k_argmax_advance evaluates it: first maximum wins */
int flm_op_argmax(const float* logits, int n, int32_t* idx) {
    if (!logits || !idx || n < 1) return FLM_ERR_INVALID;
    DevBuf dl, dst, dout;
    if (dl.alloc((size_t)n * 4) || dst.alloc(sizeof(DecodeState)) || dout.alloc(16)) return FLM_ERR_OOM;
    OPC(hipMemcpy(dl.p, logits, (size_t)n * 4, hipMemcpyHostToDevice));
    OPC(hipMemset(dst.p, 0, sizeof(DecodeState)));
    hipLaunchKernelGGL(k_argmax_advance, dim3(1), dim3(1024), 0, 0, (const float*)dl.as<float>(), n, dst.as<DecodeState>(), dout.as<int>(), 0, 4);
    OPC(hipGetLastError()); OPC(hipDeviceSynchronize());
    OPC(hipMemcpy(idx, dout.p, 4, hipMemcpyDeviceToHost));
    return FLM_OK;
}

/* Sampler::sample (sampler.cpp:113-137) through k_sample_advance -- the kernel the sampled token path launches */
int flm_op_sample(const float* logits, int n, float temperature, float topp, uint64_t* rng_state, int32_t* out) {
    if (!logits || !rng_state || !out || n < 2 || !(temperature >= 0.0f) || topp != topp) return FLM_ERR_INVALID;
    if (sample_lds_bytes(n) > kLdsMax) return FLM_ERR_UNSUPPORTED;
    DevBuf dl, dst, dout, dsp, dsort;
    if (dl.alloc((size_t)n * 4) || dst.alloc(sizeof(DecodeState)) || dout.alloc(16) || dsp.alloc(sizeof(SampleParams)) || dsort.alloc((size_t)2 * n * 8)) return FLM_ERR_OOM;
    const SampleParams sp{temperature, topp, (unsigned long long)*rng_state};
    OPC(hipMemcpy(dl.p, logits, (size_t)n * 4, hipMemcpyHostToDevice));
    OPC(hipMemcpy(dsp.p, &sp, sizeof sp, hipMemcpyHostToDevice));
    OPC(hipMemset(dst.p, 0, sizeof(DecodeState)));
    OPC(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_sample_advance), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsMax));
    SampleArgs a{};
    a.logits = dl.as<float>(); a.n = n; a.sp = dsp.as<SampleParams>(); a.st = dst.as<DecodeState>(); a.out_tokens = dout.as<int>(); a.out_cap = 4; a.advance = 0; a.sort_buf = dsort.as<unsigned long long>();
    hipLaunchKernelGGL(k_sample_advance, dim3(1), dim3(kSampleBlock), sample_lds_bytes(n), 0, a);
    OPC(hipGetLastError()); OPC(hipDeviceSynchronize());
    SampleParams back{};
    OPC(hipMemcpy(out, dout.p, 4, hipMemcpyDeviceToHost));
    OPC(hipMemcpy(&back, dsp.p, sizeof back, hipMemcpyDeviceToHost));
    *rng_state = back.rng;
    return FLM_OK;
}

/* k_sample_rows -- the sampler over the rows of a sampled verify batch -- on caller-supplied logits[rows][ld]: row i drawn with the (i + 1)-th coin of *rng_state */
int flm_op_sample_rows(const float* logits, int rows, int ld, int n, float temperature, float topp, uint64_t* rng_state, int32_t* out) {
    if (!logits || !rng_state || !out || rows < 1 || rows > kSpecRows || n < 2 || ld < n || !(temperature >= 0.0f) || topp != topp) return FLM_ERR_INVALID;
    if (sample_lds_bytes(n) > kLdsMax) return FLM_ERR_UNSUPPORTED;
    DevBuf dl, dout, dsort;
    if (dl.alloc((size_t)rows * ld * 4) || dout.alloc((size_t)kSpecRows * 4) || dsort.alloc((size_t)rows * 2 * n * 8)) return FLM_ERR_OOM;
    OPC(hipMemcpy(dl.p, logits, (size_t)rows * ld * 4, hipMemcpyHostToDevice));
    OPC(hipMemset(dout.p, 0xff, (size_t)kSpecRows * 4));
    int r = launch_sample_rows(nullptr, 0, dl.as<float>(), ld, n, 0, rows, temperature, topp, (unsigned long long)*rng_state, dsort.as<unsigned long long>(), dout.as<int>()); if (r) return r;
    OPC(hipDeviceSynchronize());
    OPC(hipMemcpy(out, dout.p, (size_t)rows * 4, hipMemcpyDeviceToHost));
    if (temperature != 0.0f) { unsigned long long s = *rng_state; for (int i = 0; i < rows; ++i) s = sample_step(s); *rng_state = s; }   // (one coin per row: the state after `rows` draws)
    return FLM_OK;
}

/* k_shape_logits -- the shaping stage of the shaped token form (flm_shape.h) -- on caller-supplied logits and window */
int flm_op_shape_logits(const float* logits, int n, const flm_sampling* sampling, const int32_t* window, int n_window, float* out) {
    if (!logits || !out || n < 2) return FLM_ERR_INVALID;
    ShapeParams sp; bool active = false;
    if (const char* why = shape_fill(sampling, n, window, n_window, false, &sp, &active)) { g_last_error = why; return FLM_ERR_INVALID; }
    DevBuf dl, dout, dp;
    if (dl.alloc((size_t)n * 4) || dout.alloc((size_t)n * 4) || dp.alloc(sizeof sp)) return FLM_ERR_OOM;
    OPC(hipMemcpy(dl.p, logits, (size_t)n * 4, hipMemcpyHostToDevice));
    OPC(hipMemcpy(dp.p, &sp, sizeof sp, hipMemcpyHostToDevice));
    ShapeArgs a{};
    a.logits = dl.as<float>(); a.out = dout.as<float>(); a.n = n; a.p = dp.as<ShapeParams>();
    hipLaunchKernelGGL(k_shape_logits, dim3(1), dim3(kSampleBlock), 0, 0, a);
    OPC(hipGetLastError()); OPC(hipDeviceSynchronize());
    OPC(hipMemcpy(out, dout.p, (size_t)n * 4, hipMemcpyDeviceToHost));
    return FLM_OK;
}

/* k_shape_rows -- the shaper over the rows of a verify batch under the controls (flm_shape.h) -- on caller-supplied rows, window and drafts */
int flm_op_shape_rows(const float* logits, int rows, int ld, int n, const flm_sampling* sampling, const int32_t* window, int n_window, const int32_t* drafts, float* out) {
    if (!logits || !out || rows < 1 || rows > kSpecRows || n < 2 || ld < n || (rows > 1 && !drafts)) return FLM_ERR_INVALID;
    ShapeParams sp; bool active = false;
    if (const char* why = shape_fill(sampling, n, window, n_window, false, &sp, &active)) { g_last_error = why; return FLM_ERR_INVALID; }
    for (int i = 0; i + 1 < rows; ++i) if (drafts[i] < 0 || drafts[i] >= n) { g_last_error = "shape_rows: draft outside [0, n)"; return FLM_ERR_INVALID; }
    const bool pen = sampling->repeat_penalty != 1.0f || sampling->frequency_penalty != 0.0f || sampling->presence_penalty != 0.0f;
    sp.last_n = pen ? sampling->penalty_last_n : 0;
    int32_t d[kSpecRows] = {0};
    for (int i = 0; i + 1 < rows; ++i) d[i] = drafts[i];
    DevBuf dl, dout, dp, dd;
    if (dl.alloc((size_t)rows * ld * 4) || dout.alloc((size_t)rows * n * 4) || dp.alloc(sizeof sp) || dd.alloc(sizeof d)) return FLM_ERR_OOM;
    OPC(hipMemcpy(dl.p, logits, (size_t)rows * ld * 4, hipMemcpyHostToDevice));
    OPC(hipMemcpy(dp.p, &sp, sizeof sp, hipMemcpyHostToDevice));
    OPC(hipMemcpy(dd.p, d, sizeof d, hipMemcpyHostToDevice));
    const ShapeParams* p = dp.as<ShapeParams>();
    int r = launch_shape_rows(nullptr, 0, dl.as<float>(), ld, dout.as<float>(), n, n, 0, rows, p, p->head, sp.n_head, dd.as<int>()); if (r) return r;
    OPC(hipDeviceSynchronize());
    OPC(hipMemcpy(out, dout.p, (size_t)rows * n * 4, hipMemcpyDeviceToHost));
    return FLM_OK;
}

/* k_shape_rows with the constraint's step 0 in front -- the shaper of a verify batch on an armed context -- on caller-supplied rows, window, drafts and automaton */
int flm_op_constrain_rows(const float* logits, int rows, int ld, int n, const flm_sampling* sampling, const int32_t* window, int n_window, const int32_t* drafts,
                          const flm_dfa* dfa, int32_t state, float* out, int32_t* states_out) {
    if (!logits || !out || !states_out || rows < 1 || rows > kSpecRows || n < 2 || ld < n || (rows > 1 && !drafts)) return FLM_ERR_INVALID;
    ShapeParams sp; bool active = false;
    if (const char* why = shape_fill(sampling, n, window, n_window, false, &sp, &active)) { g_last_error = why; return FLM_ERR_INVALID; }
    if (const char* why = dfa_check(dfa, n)) { g_last_error = why; return FLM_ERR_INVALID; }
    if (state < 0 || state >= dfa->n_states) { g_last_error = "constrain_rows: state outside [0, n_states)"; return FLM_ERR_INVALID; }
    for (int i = 0; i + 1 < rows; ++i) if (drafts[i] < 0 || drafts[i] >= n) { g_last_error = "constrain_rows: draft outside [0, n)"; return FLM_ERR_INVALID; }
    const bool pen = sampling->repeat_penalty != 1.0f || sampling->frequency_penalty != 0.0f || sampling->presence_penalty != 0.0f;
    sp.last_n = pen ? sampling->penalty_last_n : 0;
    int32_t d[kSpecRows] = {0};
    for (int i = 0; i + 1 < rows; ++i) d[i] = drafts[i];
    const size_t ns = (size_t)dfa->n_states, ne = (size_t)dfa->n_edges;
    DevBuf dl, dout, dp, dd, da, db, ds;
    if (dl.alloc((size_t)rows * ld * 4) || dout.alloc((size_t)rows * n * 4) || dp.alloc(sizeof sp) || dd.alloc(sizeof d) || da.alloc((ns + 1 + 2 * ne) * 4) ||
        db.alloc(sizeof(DfaBlock)) || ds.alloc((size_t)kSpecRows * 4)) return FLM_ERR_OOM;
    OPC(hipMemcpy(dl.p, logits, (size_t)rows * ld * 4, hipMemcpyHostToDevice));
    OPC(hipMemcpy(dp.p, &sp, sizeof sp, hipMemcpyHostToDevice));
    OPC(hipMemcpy(dd.p, d, sizeof d, hipMemcpyHostToDevice));
    int* arr = da.as<int>();
    OPC(hipMemcpy(arr, dfa->row_ptr, (ns + 1) * 4, hipMemcpyHostToDevice));
    OPC(hipMemcpy(arr + ns + 1, dfa->edge_token, ne * 4, hipMemcpyHostToDevice));
    OPC(hipMemcpy(arr + ns + 1 + ne, dfa->edge_next, ne * 4, hipMemcpyHostToDevice));
    DfaBlock blk{}; blk.row_ptr = arr; blk.edge_token = arr + ns + 1; blk.edge_next = arr + ns + 1 + ne; blk.n_states = dfa->n_states; blk.q = -1;
    OPC(hipMemcpy(db.p, &blk, sizeof blk, hipMemcpyHostToDevice));
    OPC(hipMemset(ds.p, 0xff, (size_t)kSpecRows * 4));
    const ShapeParams* p = dp.as<ShapeParams>();
    int r = launch_shape_rows(nullptr, 0, dl.as<float>(), ld, dout.as<float>(), n, n, 0, rows, p, p->head, sp.n_head, dd.as<int>(), db.as<DfaBlock>(), state, ds.as<int>()); if (r) return r;
    OPC(hipDeviceSynchronize());
    OPC(hipMemcpy(out, dout.p, (size_t)rows * n * 4, hipMemcpyDeviceToHost));
    OPC(hipMemcpy(states_out, ds.p, (size_t)rows * 4, hipMemcpyDeviceToHost));
    return FLM_OK;
}

/* k_score_rows -- the statistics kernel of flm_score_tokens -- on caller-supplied rows of logits */
int flm_op_score_rows(const float* logits, int rows, int n, const int32_t* targets, flm_score* out) {
    if (!logits || !out || rows < 1 || n < 2) return FLM_ERR_INVALID;
    if (sample_lds_bytes(n) > kLdsMax) return FLM_ERR_UNSUPPORTED;
    if (targets) for (int i = 0; i < rows; ++i) if (targets[i] < -1 || targets[i] >= n) return FLM_ERR_INVALID;
    static_assert(sizeof(flm_score) == sizeof(ScoreRow), "flm_score is k_score_rows' ScoreRow");
    DevBuf dl, dt, dout;
    if (dl.alloc((size_t)rows * n * 4) || dt.alloc((size_t)rows * 4) || dout.alloc((size_t)rows * sizeof(ScoreRow))) return FLM_ERR_OOM;
    OPC(hipMemcpy(dl.p, logits, (size_t)rows * n * 4, hipMemcpyHostToDevice));
    if (targets) OPC(hipMemcpy(dt.p, targets, (size_t)rows * 4, hipMemcpyHostToDevice));
    int r = launch_score_rows(nullptr, 0, dl.as<float>(), n, n, targets ? dt.as<int>() : nullptr, dout.as<ScoreRow>(), rows); if (r) return r;
    OPC(hipDeviceSynchronize());
    OPC(hipMemcpy(out, dout.p, (size_t)rows * sizeof(ScoreRow), hipMemcpyDeviceToHost));
    return FLM_OK;
}

/* k_logprob_rows -- the record stage of an armed context's verify batch (flm_logprob.h) -- on caller-supplied rows of logits and drawn ids */
int flm_op_logprob_rows(const float* logits, int rows, int ld, int n, const int32_t* chosen, int top_n, flm_logprob* out) {
    if (!logits || !chosen || !out || rows < 1 || rows > kSpecRows || n < 2 || ld < n || top_n < 0 || top_n > FLM_LOGPROBS_MAX) return FLM_ERR_INVALID;
    if (sample_lds_bytes(n) > kLdsMax) return FLM_ERR_UNSUPPORTED;
    for (int i = 0; i < rows; ++i) if (chosen[i] < 0 || chosen[i] >= n) return FLM_ERR_INVALID;
    static_assert(sizeof(flm_logprob) == sizeof(LogprobRec), "flm_logprob is k_logprob_rows' LogprobRec");
    DevBuf dl, dc, dout;
    if (dl.alloc((size_t)rows * ld * 4) || dc.alloc((size_t)kSpecRows * 4) || dout.alloc((size_t)rows * sizeof(LogprobRec))) return FLM_ERR_OOM;
    OPC(hipMemcpy(dl.p, logits, (size_t)rows * ld * 4, hipMemcpyHostToDevice));
    OPC(hipMemcpy(dc.p, chosen, (size_t)rows * 4, hipMemcpyHostToDevice));
    int r = launch_logprob_rows(nullptr, 0, dl.as<float>(), ld, n, 0, rows, dc.as<int>(), top_n, dout.as<LogprobRec>(), 0, rows); if (r) return r;
    OPC(hipDeviceSynchronize());
    OPC(hipMemcpy(out, dout.p, (size_t)rows * sizeof(LogprobRec), hipMemcpyDeviceToHost));
    return FLM_OK;
}

/* flm_logf as the device evaluates it (csrc/flm_logf.h: the header the host compiles too) */
int flm_op_logf(float* x, size_t n) {
    if (!x || n == 0) return FLM_ERR_INVALID;
    DevBuf d; if (d.alloc(n * 4)) return FLM_ERR_OOM;
    OPC(hipMemcpy(d.p, x, n * 4, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_op_logf, dim3(256), dim3(256), 0, 0, d.as<float>(), n);
    OPC(hipGetLastError()); OPC(hipDeviceSynchronize());
    OPC(hipMemcpy(x, d.p, n * 4, hipMemcpyDeviceToHost));
    return FLM_OK;
}

/* k_entropy_rows -- stage 5 / 6 of flm_entropy_set over the rows of a verify batch (flm_entropy.h) -- on caller-supplied rows, with Mirostat's update for given ids */
int flm_op_entropy_rows(const float* logits, int rows, int ld, int n, float temperature, const flm_entropy* e, const float* mu, const int32_t* chosen,
                        float* out, float* obs_out, float* mu_out) {
    if (!logits || !out || !e || rows < 1 || rows > kSpecRows || n < 2 || ld < n || !(temperature >= 0.0f)) return FLM_ERR_INVALID;
    if (int r = flm_entropy_validate(e)) return r;
    if (e->mirostat == 2 && !mu) { g_last_error = "entropy_rows: Mirostat needs a mu per row"; return FLM_ERR_INVALID; }
    if (chosen) for (int i = 0; i < rows; ++i) if (chosen[i] < 0 || chosen[i] >= n) { g_last_error = "entropy_rows: chosen id outside [0, n)"; return FLM_ERR_INVALID; }
    if (sample_lds_bytes(n) > kLdsMax) return FLM_ERR_UNSUPPORTED;
    DevBuf dl, dm, dc, dobs, dmu, dsort;
    if (dl.alloc((size_t)rows * ld * 4) || dm.alloc((size_t)kSpecRows * 4) || dc.alloc((size_t)kSpecRows * 4) || dobs.alloc((size_t)kSpecRows * 4) || dmu.alloc((size_t)kSpecRows * 4) ||
        dsort.alloc((size_t)rows * 2 * n * sizeof(unsigned long long))) return FLM_ERR_OOM;
    OPC(hipMemcpy(dl.p, logits, (size_t)rows * ld * 4, hipMemcpyHostToDevice));
    if (mu) OPC(hipMemcpy(dm.p, mu, (size_t)rows * 4, hipMemcpyHostToDevice));
    if (chosen) OPC(hipMemcpy(dc.p, chosen, (size_t)rows * 4, hipMemcpyHostToDevice));
    OPC(hipMemset(dobs.p, 0, (size_t)kSpecRows * 4)); OPC(hipMemset(dmu.p, 0, (size_t)kSpecRows * 4));
    EntropyRowsArgs a{};
    a.rows = dl.as<float>(); a.ld = ld; a.n = n; a.temp = temperature; a.typical_p = e->typical_p; a.mirostat = e->mirostat; a.tau = e->tau; a.eta = e->eta;
    a.mu = mu ? dm.as<float>() : nullptr; a.sort_buf = dsort.as<unsigned long long>();
    a.chosen = chosen ? dc.as<int>() : nullptr; a.obs_out = dobs.as<float>(); a.mu_out = dmu.as<float>();
    int r = launch_entropy_rows(nullptr, 0, a, rows); if (r) return r;
    OPC(hipDeviceSynchronize());
    for (int i = 0; i < rows; ++i) OPC(hipMemcpy(out + (size_t)i * n, dl.as<float>() + (size_t)i * ld, (size_t)n * 4, hipMemcpyDeviceToHost));
    if (obs_out) OPC(hipMemcpy(obs_out, dobs.p, (size_t)rows * 4, hipMemcpyDeviceToHost));
    if (mu_out) OPC(hipMemcpy(mu_out, dmu.p, (size_t)rows * 4, hipMemcpyDeviceToHost));
    return FLM_OK;
}

int flm_op_swiglu(float* xo, const float* xr, size_t n) {
    if (!xo || !xr || n == 0) return FLM_ERR_INVALID;
    DevBuf a, b; if (a.alloc(n * 4) || b.alloc(n * 4)) return FLM_ERR_OOM;
    OPC(hipMemcpy(a.p, xo, n * 4, hipMemcpyHostToDevice)); OPC(hipMemcpy(b.p, xr, n * 4, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_op_swiglu, dim3(256), dim3(256), 0, 0, a.as<float>(), (const float*)b.as<float>(), n);
    OPC(hipGetLastError()); OPC(hipDeviceSynchronize());
    OPC(hipMemcpy(xo, a.p, n * 4, hipMemcpyDeviceToHost));
    return FLM_OK;
}

int flm_op_rope(float* o, const float* x, int n_dims, int pos) {
    if (!o || !x || n_dims < 2 || n_dims % 2 || pos < 0) return FLM_ERR_INVALID;
    std::vector<float> cs, sn; build_rope_table(n_dims, pos + 1, cs, sn);
    DevBuf dx, dout, dc, dsn; const size_t h = n_dims / 2;
    if (dx.alloc(n_dims * 4) || dout.alloc(n_dims * 4) || dc.alloc(h * 4) || dsn.alloc(h * 4)) return FLM_ERR_OOM;
    OPC(hipMemcpy(dx.p, x, n_dims * 4, hipMemcpyHostToDevice));
    OPC(hipMemcpy(dc.p, cs.data() + (size_t)pos * h, h * 4, hipMemcpyHostToDevice)); OPC(hipMemcpy(dsn.p, sn.data() + (size_t)pos * h, h * 4, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_op_rope, dim3((unsigned)((h + 63) / 64)), dim3(64), 0, 0, dout.as<float>(), (const float*)dx.as<float>(), n_dims, (const float*)dc.as<float>(), (const float*)dsn.as<float>());
    OPC(hipGetLastError()); OPC(hipDeviceSynchronize());
    OPC(hipMemcpy(o, dout.p, n_dims * 4, hipMemcpyDeviceToHost));
    return FLM_OK;
}

int flm_op_softmax(float* x, int n) {
    if (!x || n < 1) return FLM_ERR_INVALID;
    DevBuf d; if (d.alloc((size_t)n * 4)) return FLM_ERR_OOM;
    OPC(hipMemcpy(d.p, x, (size_t)n * 4, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_op_softmax, dim3(1), dim3(kBlock), 0, 0, d.as<float>(), n);
    OPC(hipGetLastError()); OPC(hipDeviceSynchronize());
    OPC(hipMemcpy(x, d.p, (size_t)n * 4, hipMemcpyDeviceToHost));
    return FLM_OK;
}

int flm_op_attention(float* out, float* kc, float* vc, const float* q, const float* k, const float* v,
                     int n_heads, int hs, int max_seq, int pos) {
    if (!out || !kc || !vc || !q || !k || !v || n_heads < 1 || hs < 32 || hs > 256 || hs % 8 || pos < 0 || pos >= max_seq) return FLM_ERR_INVALID;
    const size_t nd = (size_t)n_heads * hs, nc = (size_t)n_heads * max_seq * hs, h2 = hs / 2;
    std::vector<float> cs, sn; build_rope_table(hs, pos + 1, cs, sn);
    DevBuf dq, dk, dv, dkc, dvc, dout, dc, dsn, dpos;
    if (dq.alloc(nd * 4) || dk.alloc(nd * 4) || dv.alloc(nd * 4) || dkc.alloc(nc * 4) || dvc.alloc(nc * 4) || dout.alloc(nd * 4) ||
        dc.alloc(h2 * 4) || dsn.alloc(h2 * 4) || dpos.alloc(4)) return FLM_ERR_OOM;
    OPC(hipMemcpy(dq.p, q, nd * 4, hipMemcpyHostToDevice)); OPC(hipMemcpy(dk.p, k, nd * 4, hipMemcpyHostToDevice)); OPC(hipMemcpy(dv.p, v, nd * 4, hipMemcpyHostToDevice));
    OPC(hipMemcpy(dkc.p, kc, nc * 4, hipMemcpyHostToDevice)); OPC(hipMemcpy(dvc.p, vc, nc * 4, hipMemcpyHostToDevice));
    OPC(hipMemcpy(dc.p, cs.data() + (size_t)pos * h2, h2 * 4, hipMemcpyHostToDevice)); OPC(hipMemcpy(dsn.p, sn.data() + (size_t)pos * h2, h2 * 4, hipMemcpyHostToDevice));
    OPC(hipMemcpy(dpos.p, &pos, 4, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_op_kv_append, dim3((unsigned)((nd / 2 + 255) / 256)), dim3(256), 0, 0, dq.as<float>(), (const float*)dk.as<float>(), (const float*)dv.as<float>(),
                       dkc.as<float>(), dvc.as<float>(), (const float*)dc.as<float>(), (const float*)dsn.as<float>(), n_heads, hs, max_seq, pos);
    OPC(hipGetLastError());
    AttnArgs a{}; a.q = dq.as<float>(); a.kcache = dkc.as<float>(); a.vcache = dvc.as<float>(); a.pos_ptr = dpos.as<int>(); a.hs = hs; a.max_seq = max_seq;
    a.out = dout.as<float>();
    // tests: FLM_OP_ATTN_PARTS = G spreads every head over G workgroups (the long-context path of the decode loop)
    int G = (getenv("FLM_OP_ATTN_PARTS") && atoi(getenv("FLM_OP_ATTN_PARTS")) > 1) ? hs / kSplitDims : 1;
    if (G < 2 || hs % kSplitDims || hs > 128 || n_heads * G > 256 || max_seq > kSplitMaxSeq) G = 1;
    DevBuf dsc, dfl, derr;
    if (dsc.alloc((size_t)n_heads * max_seq * 4) || dfl.alloc(256 * 64) || derr.alloc(64)) return FLM_ERR_OOM;
    OPC(hipMemset(dfl.p, 0, 256 * 64)); OPC(hipMemset(derr.p, 0, 64));
    a.G = G; a.sc_global = dsc.as<float>(); a.flag_sc = dfl.as<unsigned>(); a.epoch = 1; a.err = derr.as<int>();
    if (G > 1) hipLaunchKernelGGL(k_attn_decode<true>, dim3(n_heads * G), dim3(kAttnBlock), attn_lds_bytes(max_seq, hs, true), 0, a);
    else       hipLaunchKernelGGL(k_attn_decode<false>, dim3(n_heads), dim3(kAttnBlock), attn_lds_bytes(max_seq, hs, false), 0, a);
    OPC(hipGetLastError());
    OPC(hipDeviceSynchronize());
    OPC(hipMemcpy(out, dout.p, nd * 4, hipMemcpyDeviceToHost));
    OPC(hipMemcpy(kc, dkc.p, nc * 4, hipMemcpyDeviceToHost)); OPC(hipMemcpy(vc, dvc.p, nc * 4, hipMemcpyDeviceToHost));
    return FLM_OK;
}

// one flm_generate_n step's RoPE / cache rows / attention on caller-supplied caches: the launches prefill_batched makes with a FanDesc (flm_prompt.hip)
int flm_op_attention_fan(float* out, float* kc, float* vc, const float* q, const float* k, const float* v,
                         int n_heads, int hs, int max_seq, int n, int S, int t, const int32_t* base) {
    if (!out || !kc || !vc || !q || !k || !v || !base || n_heads < 1 || hs < 32 || hs > 128 || hs % 8 || n < 2 || n > FLM_FAN_MAX || S < 1 || t < 0 || max_seq < 1 || S + t + 1 > max_seq) return FLM_ERR_INVALID;
    FanDesc f{}; f.S = S; f.t = t; f.n = n;
    for (int j = 0; j < n; ++j) { if (base[j] < 0 || base[j] + t >= max_seq) return FLM_ERR_INVALID; f.base[j] = base[j]; }
    const int dim = n_heads * hs, pos = S + t;
    const size_t nd = (size_t)n * dim, nc = (size_t)n_heads * max_seq * hs, h2 = hs / 2;
    std::vector<float> cs, sn; build_rope_table(hs, pos + 1, cs, sn);
    std::vector<float> qkv(3 * nd);
    for (int j = 0; j < n; ++j) {
        memcpy(&qkv[(size_t)j * 3 * dim], q + (size_t)j * dim, (size_t)dim * 4); memcpy(&qkv[(size_t)j * 3 * dim + dim], k + (size_t)j * dim, (size_t)dim * 4);
        memcpy(&qkv[(size_t)j * 3 * dim + 2 * dim], v + (size_t)j * dim, (size_t)dim * 4);
    }
    DevBuf dqkv, dq, dkc, dvc, dout, dc, dsn;
    if (dqkv.alloc(3 * nd * 4) || dq.alloc(nd * 4) || dkc.alloc(nc * 4) || dvc.alloc(nc * 4) || dout.alloc(nd * 4) || dc.alloc((pos + 1) * h2 * 4) || dsn.alloc((pos + 1) * h2 * 4)) return FLM_ERR_OOM;
    OPC(hipMemcpy(dqkv.p, qkv.data(), 3 * nd * 4, hipMemcpyHostToDevice));
    OPC(hipMemcpy(dkc.p, kc, nc * 4, hipMemcpyHostToDevice)); OPC(hipMemcpy(dvc.p, vc, nc * 4, hipMemcpyHostToDevice));
    OPC(hipMemcpy(dc.p, cs.data(), (pos + 1) * h2 * 4, hipMemcpyHostToDevice)); OPC(hipMemcpy(dsn.p, sn.data(), (pos + 1) * h2 * 4, hipMemcpyHostToDevice));
    int r = launch_rope_kv_fan(nullptr, 0, dqkv.as<float>(), dq.as<float>(), dkc.as<float>(), dvc.as<float>(), dc.as<float>(), dsn.as<float>(), dim, hs, max_seq, f); if (r) return r;
    AttnArgs a{}; a.q = dq.as<float>(); a.kcache = dkc.as<float>(); a.vcache = dvc.as<float>(); a.out = dout.as<float>(); a.hs = hs; a.max_seq = max_seq;
    r = launch_attn_fan(nullptr, 0, a, f, n_heads, dim); if (r) return r;
    OPC(hipDeviceSynchronize());
    OPC(hipMemcpy(out, dout.p, nd * 4, hipMemcpyDeviceToHost));
    OPC(hipMemcpy(kc, dkc.p, nc * 4, hipMemcpyDeviceToHost)); OPC(hipMemcpy(vc, dvc.p, nc * 4, hipMemcpyDeviceToHost));
    return FLM_OK;
}

// one flm_batch_step's RoPE / cache rows / attention on caller-supplied caches: the launches prefill_batched makes with a SlotDesc (flm_prompt.hip)
int flm_op_attention_slots(float* out, float* kc, float* vc, const float* q, const float* k, const float* v,
                           int n_heads, int hs, int max_seq, int n, const int32_t* base, const int32_t* pos) {
    if (!out || !kc || !vc || !q || !k || !v || !base || !pos || n_heads < 1 || hs < 32 || hs > 256 || hs % 8 || n < 1 || n > FLM_BATCH_MAX || max_seq < 1) return FLM_ERR_INVALID;
    SlotDesc f{}; f.n = n;
    int top = 0;
    for (int r = 0; r < n; ++r) {
        if (base[r] < 0 || pos[r] < 0 || (long long)base[r] + pos[r] >= max_seq) return FLM_ERR_INVALID;
        f.slot[r] = r; f.base[r] = base[r]; f.pos[r] = pos[r]; f.rows[r] = max_seq - base[r];
        top = pos[r] > top ? pos[r] : top;
    }
    const int dim = n_heads * hs;
    const size_t nd = (size_t)n * dim, nc = (size_t)n_heads * max_seq * hs, h2 = hs / 2;
    std::vector<float> cs, sn; build_rope_table(hs, top + 1, cs, sn);
    std::vector<float> qkv(3 * nd);
    for (int j = 0; j < n; ++j) {
        memcpy(&qkv[(size_t)j * 3 * dim], q + (size_t)j * dim, (size_t)dim * 4); memcpy(&qkv[(size_t)j * 3 * dim + dim], k + (size_t)j * dim, (size_t)dim * 4);
        memcpy(&qkv[(size_t)j * 3 * dim + 2 * dim], v + (size_t)j * dim, (size_t)dim * 4);
    }
    DevBuf dqkv, dq, dkc, dvc, dout, dc, dsn, dviews;
    if (dqkv.alloc(3 * nd * 4) || dq.alloc(nd * 4) || dkc.alloc(nc * 4) || dvc.alloc(nc * 4) || dout.alloc(nd * 4) || dc.alloc((top + 1) * h2 * 4) || dsn.alloc((top + 1) * h2 * 4) ||
        dviews.alloc(sizeof(AttnArgs) * kBatchMax)) return FLM_ERR_OOM;
    OPC(hipMemcpy(dqkv.p, qkv.data(), 3 * nd * 4, hipMemcpyHostToDevice));
    OPC(hipMemcpy(dkc.p, kc, nc * 4, hipMemcpyHostToDevice)); OPC(hipMemcpy(dvc.p, vc, nc * 4, hipMemcpyHostToDevice));
    OPC(hipMemcpy(dc.p, cs.data(), (top + 1) * h2 * 4, hipMemcpyHostToDevice)); OPC(hipMemcpy(dsn.p, sn.data(), (top + 1) * h2 * 4, hipMemcpyHostToDevice));
    int r = launch_rope_kv_slots(nullptr, 0, dqkv.as<float>(), dq.as<float>(), dkc.as<float>(), dvc.as<float>(), dc.as<float>(), dsn.as<float>(), dim, hs, max_seq, f); if (r) return r;
    AttnArgs a{}; a.q = dq.as<float>(); a.kcache = dkc.as<float>(); a.vcache = dvc.as<float>(); a.out = dout.as<float>(); a.hs = hs; a.max_seq = max_seq;
    r = launch_attn_slots(nullptr, 0, a, f, n_heads, dim, dviews.as<AttnArgs>()); if (r) return r;
    OPC(hipDeviceSynchronize());
    OPC(hipMemcpy(out, dout.p, nd * 4, hipMemcpyDeviceToHost));
    OPC(hipMemcpy(kc, dkc.p, nc * 4, hipMemcpyDeviceToHost)); OPC(hipMemcpy(vc, dvc.p, nc * 4, hipMemcpyDeviceToHost));
    return FLM_OK;
}

// one flm_batch_pass's RoPE / cache rows / attention on caller-supplied caches: the launches prefill_batched makes with a SegDesc (flm_prompt.hip)
int flm_op_attention_segs(float* out, float* kc, float* vc, const float* q, const float* k, const float* v,
                          int n_heads, int hs, int max_seq, int B, int n_segs, int n_step, const int32_t* base, const int32_t* rows, const int32_t* n, const int32_t* pos0,
                          int one_query) {
    if (!out || !kc || !vc || !q || !k || !v || !base || !rows || !n || !pos0 || n_heads < 1 || hs < 32 || hs > 256 || hs % 8 || max_seq < 1 || B < 1 ||
        n_segs < 1 || n_segs > FLM_BATCH_MAX || n_step < 0 || n_step > n_segs) return FLM_ERR_INVALID;
    SegDesc f{}; f.n_segs = n_segs; f.n_step = n_step;
    SlotDesc fs{}; fs.n = n_step;
    int top = 0;
    for (int s = 0, at = 0; s < n_segs; ++s) {
        f.slot[s] = s; f.row0[s] = at; f.n[s] = n[s]; f.base[s] = base[s]; f.pos0[s] = pos0[s]; f.rows[s] = rows[s];
        if (n[s] < 1 || (long long)at + n[s] > B) return FLM_ERR_INVALID;
        at += n[s];
        if (s < n_step) { fs.slot[s] = s; fs.base[s] = base[s]; fs.pos[s] = pos0[s]; fs.rows[s] = rows[s]; }
        if (pos0[s] >= 0 && (long long)pos0[s] + n[s] <= max_seq) top = pos0[s] + n[s] > top ? pos0[s] + n[s] : top;
    }
    if (seg_check(f, B, max_seq)) return FLM_ERR_INVALID;
    const int dim = n_heads * hs;
    const size_t nd = (size_t)B * dim, nc = (size_t)n_heads * max_seq * hs, h2 = hs / 2;
    std::vector<float> cs, sn; build_rope_table(hs, top, cs, sn);
    std::vector<float> qkv(3 * nd);
    for (int j = 0; j < B; ++j) {
        memcpy(&qkv[(size_t)j * 3 * dim], q + (size_t)j * dim, (size_t)dim * 4); memcpy(&qkv[(size_t)j * 3 * dim + dim], k + (size_t)j * dim, (size_t)dim * 4);
        memcpy(&qkv[(size_t)j * 3 * dim + 2 * dim], v + (size_t)j * dim, (size_t)dim * 4);
    }
    DevBuf dqkv, dq, dkc, dvc, dout, dc, dsn, dviews, dsviews;
    if (dqkv.alloc(3 * nd * 4) || dq.alloc(nd * 4) || dkc.alloc(nc * 4) || dvc.alloc(nc * 4) || dout.alloc(nd * 4) || dc.alloc(top * h2 * 4) || dsn.alloc(top * h2 * 4) ||
        dviews.alloc(sizeof(AttnArgs) * kBatchMax) || dsviews.alloc(sizeof(AttnArgs) * kBatchMax)) return FLM_ERR_OOM;
    OPC(hipMemcpy(dqkv.p, qkv.data(), 3 * nd * 4, hipMemcpyHostToDevice));
    OPC(hipMemcpy(dkc.p, kc, nc * 4, hipMemcpyHostToDevice)); OPC(hipMemcpy(dvc.p, vc, nc * 4, hipMemcpyHostToDevice));
    OPC(hipMemcpy(dc.p, cs.data(), top * h2 * 4, hipMemcpyHostToDevice)); OPC(hipMemcpy(dsn.p, sn.data(), top * h2 * 4, hipMemcpyHostToDevice));
    AttnArgs a{}; a.q = dq.as<float>(); a.kcache = dkc.as<float>(); a.vcache = dvc.as<float>(); a.out = dout.as<float>(); a.hs = hs; a.max_seq = max_seq;
    int r = FLM_OK;
    if (n_step > 0) { r = launch_rope_kv_slots(nullptr, 0, dqkv.as<float>(), dq.as<float>(), dkc.as<float>(), dvc.as<float>(), dc.as<float>(), dsn.as<float>(), dim, hs, max_seq, fs); if (r) return r; }
    if (n_step < n_segs) { r = launch_rope_kv_segs(nullptr, 0, dqkv.as<float>(), dq.as<float>(), dkc.as<float>(), dvc.as<float>(), dc.as<float>(), dsn.as<float>(), dim, hs, max_seq, f, B); if (r) return r; }
    if (n_step > 0) { r = launch_attn_slots(nullptr, 0, a, fs, n_heads, dim, dviews.as<AttnArgs>()); if (r) return r; }
    if (n_step < n_segs) { r = launch_attn_segs(nullptr, 0, a, f, n_heads, dim, dsviews.as<AttnArgs>(), one_query != 0); if (r) return r; }
    OPC(hipDeviceSynchronize());
    OPC(hipMemcpy(out, dout.p, nd * 4, hipMemcpyDeviceToHost));
    OPC(hipMemcpy(kc, dkc.p, nc * 4, hipMemcpyDeviceToHost)); OPC(hipMemcpy(vc, dvc.p, nc * 4, hipMemcpyDeviceToHost));
    return FLM_OK;
}

/* elementary functions exactly as the kernels evaluate them (tests pin them against the host's IEEE results) */
int flm_op_math(int fn, float* x, const float* y, size_t n) {
    if (!x || n == 0 || fn < 0 || fn > 5 || (fn >= 2 && !y)) return FLM_ERR_INVALID;
    DevBuf d, e; if (d.alloc(n * 4) || e.alloc(n * 4)) return FLM_ERR_OOM;
    OPC(hipMemcpy(d.p, x, n * 4, hipMemcpyHostToDevice));
    if (y) OPC(hipMemcpy(e.p, y, n * 4, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_op_math, dim3(1024), dim3(256), 0, 0, fn, d.as<float>(), (const float*)e.as<float>(), n);
    OPC(hipGetLastError()); OPC(hipDeviceSynchronize());
    OPC(hipMemcpy(x, d.p, n * 4, hipMemcpyDeviceToHost));
    return FLM_OK;
}
int flm_op_expf(float* x, size_t n) { return flm_op_math(0, x, nullptr, n); }

} // extern "C"
