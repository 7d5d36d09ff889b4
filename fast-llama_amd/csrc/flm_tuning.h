// flm_tuning.h -- the option table of libflm_gpu.so: ONE row per key that flm_set_option stores and flm_query reads back, with what the code has to know about it.
// (included by flm_host.h behind flm_ctx: the rows hold member pointers.)  flm_gpu.hip walks it; capi.TUNING_KEYS and the option comment of include/flm_gpu.h are checked
// against it (tests/test_capi_host.py).
//
// The rows marked kOptDial are the experiment dials.  They are NOT part of the drop-in boundary (include/flm_gpu.h): a deployment never touches them, their optimum was
// measured and is the default.  flm_set_option refuses these keys (FLM_ERR_INVALID) until the context has been put into tuning mode with flm_set_option(ctx, "tuning", 1)
// -- tools/back_bench.py, tools/stress.py and the parity tests do that (through fast-llama_amd/capi.py) to sweep them and to prove that none of them changes a result bit.
//
//   "wg_per_cu"        workgroups per CU for the stand-alone GEMV launches (1)
//   "use_mfma"         int8 prefill GEMM tile shape on the matrix cores: 1 by problem size, 2 (or 0) always 64 x 64, 3 always 128 x 128 tiles (1)
//   "tok_preq"         k_layers: how many of a workgroup's 16 waves request their first register set of the NEXT layer's [Wq; Wk; Wv] in front of the layer edge's hand-off (by launch: 12 in the one-launch token below 128 positions, else 16)
//   "tok_nstq"         ... and how many LDS stash slots (4.25 KiB each; -1: as many as the LDS holds) it fills with it there (4)
//   "back_nst13"       stash slots a Wo workgroup fills with [W1; W3] under the attention (-1)
//   "back_nst13_head"  ... a head workgroup fills behind its head (-1)
//   "back_nst2"        ... every workgroup fills with W2 behind its rows of hd (0; the arrival-order FFN2 holds W2's whole share anyway)
//   "back_pre13"       waves that request their first register set of [W1; W3] in front of the x1 hand-off (by launch: 8 in the one-launch token below 128 positions, else 16)
//   "back_pre2"        waves that request their first register set of W2 in front of the hd flag round (16; the hand-off in its round-4 form)
//   "back_ao2"         arrival-order FFN2: what of W2 is requested in front of a wave's first look: 1 everything, 2 the first register sets (default), 3 first sets + stash
//   "attn_kpre"        split heads (long contexts) inside the whole-layer launches: a part's first two K tiles are brought into LDS by LDS-DMA under the layer's QKV phase (1) or requested when the
//                      part's attention starts (0)
//   "back_nwo"         arrival-order Wo: how many of a workgroup's 16 waves hold Wo's steps and look for their heads; the others issue the [W1; W3] stash (0 = ceil(steps / 2): 10 at 7B; 16 = every
//                      wave does both, rounds 4-5)
//   "inject_wait_failure" 1 = raise the "a cross-workgroup wait gave up" flag NOW (one shot): the next call's fused launches run through without waiting, the call is re-run on
//                      one kernel per phase and the context stays there for 64 tokens ("fallback" 1, "fallback_active" 1), then takes the census again and returns to the launch
//                      structure it had (maybe_recover) -- the error path of a 20 ms time-out, exercised by tests/test_gpu_model.py without waiting for one.  An action, not a
//                      value: no member, and flm_query does not know it
//   "age_epochs"       value = the 32-bit pattern E: put the context's device state into what a real run would have left with its epoch counters at E -- the one-launch token's
//                      epoch (TailArgs::epoch), the token's epoch base of the tensor-parallel hand-offs (rounded down to a multiple of the token's stride) and k_xchg's four exchange
//                      counters --, every never-cleared flag line and granule tag that counts from one of them holding what the previous token would have left (flm_gpu.hip
//                      age_epochs).  Days of decoding in one call: tests/test_gpu_longlived.py carries contexts across 2^31 and the counters' wrap with it.  Between two calls, and
//                      under tensor parallelism on every rank alike before the next token.  An action like "inject_wait_failure"; flm_query reads the counters back as
//                      "epoch_tail" / "epoch_eng" / "epoch_xchg"
// Numbers behind the defaults: DESIGN.md section 7c / 7d, tools/back_bench.py.
#pragma once
namespace fh {
constexpr unsigned kOptDial = 1;       // an experiment dial: refused until "tuning" is 1
constexpr unsigned kOptResident = 2;   // a non-zero value needs one workgroup per CU resident (the census at flm_ctx_create); zeroed at create where it is not
constexpr unsigned kOptFrozen = 4;     // which prompt kernels a tensor-parallel group runs: refused once flm_p2p_import has agreed on them
constexpr unsigned kOptFallback = 8;   // the launch structure that waits across workgroups: saved and zeroed when a wait gives up (xwg_check), restored by maybe_recover
struct OptionRow { const char* key; int flm_ctx::* member; unsigned flags; };
// Keys whose setter does more than store the value ("wg_per_cu", "tp_fence": clamped; "inject_wait_failure", "age_epochs", "cu_parts", "use_p2p") have their row here -- flags, and the member
// flm_query reports -- and their code in flm_set_option.  "tuning" (a bool) and FLM_ABLATE's "ablate" / "trace" (not queryable) are not rows.
constexpr OptionRow kOptions[] = {
    {"wg_per_cu", &flm_ctx::wg_per_cu, kOptDial},
    {"use_graph", &flm_ctx::use_graph, 0},
    {"graph_chunks", &flm_ctx::graph_chunks, 0},
    {"inject_wait_failure", nullptr, kOptDial},
    {"age_epochs", nullptr, kOptDial},
    {"use_prefill", &flm_ctx::use_prefill, 0},
    {"score_rows", &flm_ctx::score_rows, 0},
    {"spec_gemm", &flm_ctx::spec_gemm, 0},
    {"batch_rows", &flm_ctx::batch_rows, 0},
    {"use_mfma", &flm_ctx::use_mfma, kOptDial | kOptFrozen},
    {"use_pv_mfma", &flm_ctx::use_pv_mfma, kOptFrozen},
    {"use_qk_mfma", &flm_ctx::use_qk_mfma, kOptFrozen},
    {"use_prefill_mq", &flm_ctx::use_prefill_mq, kOptFrozen},
    {"fuse_attn_o", &flm_ctx::fuse_attn_o, kOptResident | kOptFallback},
    {"fuse_ffn", &flm_ctx::fuse_ffn, kOptResident | kOptFallback},
    {"fuse_qkv", &flm_ctx::fuse_qkv, kOptResident | kOptFallback},
    {"fuse_back", &flm_ctx::fuse_back, kOptResident | kOptFallback},
    {"fuse_layer", &flm_ctx::fuse_layer, 0},
    {"fuse_token", &flm_ctx::fuse_token, kOptFallback},
    {"fuse_tail", &flm_ctx::fuse_tail, 0},
    {"tok_nstq", &flm_ctx::tok_nstq, kOptDial},
    {"tok_preq", &flm_ctx::tok_preq, kOptDial},
    {"back_nst13", &flm_ctx::back_nst13, kOptDial},
    {"back_nst13_head", &flm_ctx::back_nst13_head, kOptDial},
    {"back_nst2", &flm_ctx::back_nst2, kOptDial},
    {"back_pre13", &flm_ctx::back_pre13, kOptDial},
    {"back_pre2", &flm_ctx::back_pre2, kOptDial},
    {"back_ao", &flm_ctx::back_ao, 0},
    {"back_ao2", &flm_ctx::back_ao2, kOptDial},
    {"back_nwo", &flm_ctx::back_nwo, kOptDial},
    {"attn_kpre", &flm_ctx::attn_kpre, kOptDial},
    {"gr_edges", &flm_ctx::gr_edges, 0},
    {"attn_split", &flm_ctx::attn_split, kOptResident | kOptFallback},
    {"fold_xchg", &flm_ctx::fold_xchg, 0},
    {"tp_fuse_attn", &flm_ctx::tp_fuse_attn, 0},
    {"tp_fuse_ffn", &flm_ctx::tp_fuse_ffn, 0},
    {"tp_fuse_layers", &flm_ctx::tp_fuse_layers, 0},
    {"tp_fence", &flm_ctx::tp_fence, 0},
    {"tp_trust_fused", &flm_ctx::tp_trust_fused, 0},
    {"force_tp", &flm_ctx::force_tp, 0},
    {"cu_parts", &flm_ctx::cu_parts, 0},
    {"use_p2p", &flm_ctx::p2p, 0},
};
}
