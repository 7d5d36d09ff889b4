// flm_host.h -- what the translation units of libflm_gpu.so share on the HOST side: the context, the launch planning of the GEMV and the entry points of one
// translation unit that another one calls.
//   flm_gpu.hip          the context and everything that outlives a call: create / destroy, upload, residency and fallback, the p2p bootstrap, options and queries, epoch
//                        ageing, the debug taps, the graph cache (run_token / run_tokens / prepare_all), warm_up, flm_prepare
//   flm_calls.hip        what a call does: check_ready, feed, the retry wrapper, the by-value block setters, d2h / h2d, the draw plan (Draw) and the model-level entry
//                        points (forward / decode / generate / score / draft-and-verify / constraint / log-probabilities)
//   flm_token.hip        the per-token launch sequence (enqueue_token: the launch forms it tries come from TokenPlan below), the per-phase and fused decode launches, each
//                        launched in one place, per-kernel timing (flm_kernel_times / _bytes)
//   flm_layerlaunch.hip  the whole-layer launch k_attn_ffn (flm_layer.h) and the layer's argument blocks (plan_layer)
//   flm_layers.hip       all layers of a token / the whole greedy token in one launch (k_layers); flm_layers_tp.hip: its rank-spanning form
//   flm_launch.h         from a run-time choice to one instantiation of a kernel template: the variant lists' dispatch() / for_each_variant()
//   flm_prompt.hip       the batched prompt path (GEMM tiles on the matrix cores, prompt attention; with a FanDesc: one step of flm_generate_n)
//   flm_ops.hip          the op-level exports of the parity tests (flm_op_*)
//   flm_wait.h           (device side, part of flm_kernels.h) every cross-workgroup / cross-rank wait of the fused launches: flag polls, granule pieces, when a wait gives up
//   flm_tuning.h         the option table: one row per flm_set_option / flm_query key (flm_gpu.hip walks it)
#pragma once
#include "flm_gpu.h"
#include "flm_kernels.h"
#include "flm_launch.h"

#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <map>
#include <string>
#include <mutex>
#include <tuple>
#include <vector>

namespace fh {
using namespace flm;
extern thread_local std::string g_last_error;

struct QMat { void* q = nullptr; float* s = nullptr; int rows = 0, cols = 0; float* st = nullptr; /* s group-major [cols / 64][rows]: the prompt path's GEMM tiles */ };
struct LayerW {
    QMat qkv, o, w13, w2;     // w13 = [W1 (gate) ; W3 (up)] back to back: the SwiGLU GEMV walks them as one matrix
    float* att_norm = nullptr; float* ffn_norm = nullptr;
    unsigned got = 0;     // bitmask of uploaded kinds
};

enum KClass { KC_EMBED = 0, KC_QKV, KC_ATTN, KC_ATTN_O, KC_FFN13, KC_FFN2, KC_CLS, KC_ARGMAX, KC_ALLREDUCE, KC_ATTN_WO /* k_attn_o: attention + Wo */, KC_FFN /* k_ffn: FFN13 + FFN2 */, KC_QKV_ATTN_WO /* k_qkv_attn_o */, KC_LAYER /* k_attn_ffn with the QKV GEMV in front: the whole layer */, KC_BACK /* k_attn_ffn: attention + Wo + FFN13 + FFN2 */, KC_LAYERS /* k_layers: all layers of the token in one launch */, KC_TOKEN /* k_layers<.., TAIL>: the whole greedy token in one launch */ };

struct TimedLaunch { int kclass; hipEvent_t e0, e1; };
// owners that release on every exit path (the error macros return from the middle of a function)
struct DevMem { void* p = nullptr; ~DevMem() { if (p) hipFree(p); } };
struct EvPair { hipEvent_t e0 = nullptr, e1 = nullptr; ~EvPair() { if (e0) hipEventDestroy(e0); if (e1) hipEventDestroy(e1); } };
// What a token does behind its layers (enqueue_token):
//   Logits   the classifier's logits stay for the caller, the decode state is left alone
//   Greedy   tok <- the first maximum (k_argmax_advance, or the one-launch token), pos++
//   Prompt   a prompt token in front of the last one: no classifier, the state moves on to the next prompt id
//   Sampled  tok <- k_sample_advance on the logits, pos++
//   Shaped   k_shape_logits, then the sampler (the argmax where the vocabulary is beyond the sampler) on the shaped row, pos++
//   ShapedLp Shaped with k_logprob_token behind the sampler (flm_logprob.h): what the _ex entry points replay while the context is armed with flm_logprobs_arm.  A form of
//            its own, so that the Shaped graphs stay node for node what they were and arming captures nothing
//   ShapedEnt the shaped form with k_entropy_advance as its last launch (flm_entropy.h: stage 5 / 6, the unchanged draw, Mirostat's update, the token's tail): what
//            flm_generate_ex / flm_forward_sample_ex replay while flm_entropy_set is on.  A form of its own for the same reason
enum class TokenForm { Logits, Greedy, Prompt, Sampled, Shaped, ShapedLp, ShapedEnt };
inline bool shaped_form(TokenForm f) { return f == TokenForm::Shaped || f == TokenForm::ShapedLp || f == TokenForm::ShapedEnt; }
// a cached token graph: n token sequences (with_cls, form) for G workgroups per head
using GraphKey = std::tuple<bool, TokenForm, int, int>;


} // namespace fh
using namespace fh;

constexpr size_t kLdsMax = 160 * 1024;                            // LDS of a gfx950 CU = the most one workgroup can have
struct flm_ctx {
    flm_model_desc d{};
    int device = 0, rank = 0, world = 1;
    flm_shard_plan plan{};
    int hs = 0, esz = 1, cu_count = 256, cu_total = 256, n_xcd = 8;   // cu_count: CUs this context's launches are sized for (cu_total / cu_parts)
    int dim_local = 0, hidden_local = 0, heads_local = 0, vocab_slot = 0;    // dim_local = heads_local*hs: q/k/v rows and attention outputs owned
    int drow_begin = 0, drow_count = 0;                                       // rows of Wo / W2 (= slice of the residual stream) owned
    hipStream_t stream = nullptr;
    ncclComm_t comm = nullptr;

    std::vector<LayerW> layers;
    void* emb = nullptr; float* emb_s = nullptr; int emb_qt = 0; bool got_emb = false;
    float* out_norm = nullptr; bool got_out_norm = false;
    QMat cls; bool got_cls = false;

    float *kcache = nullptr, *vcache = nullptr;       // [L][heads_local][kv_rows][hs]
    int kv_rows = 0;                                   // max_seq_len + 8: rows per head in the caches (a head's rows start 4 KiB (hs 128) off the power-of-two stride: DESIGN.md section 7c)
    float *x1 = nullptr, *qbuf = nullptr, *att_out = nullptr, *hd = nullptr;
    float *logits = nullptr;
    float *rope_cos = nullptr, *rope_sin = nullptr;
    DecodeState* state = nullptr; int* prompt_dev = nullptr; int* out_tokens_dev = nullptr;
    int prompt_cap = 0, out_cap = 0;
    // the context's own page-locked bounce buffer: logits, ids and prompt tokens cross the bus through it (allocated at create).  A caller's pageable buffer handed to
    // hipMemcpyAsync is pinned and mapped by the runtime on every call -- ~100 us of host time per call and, the first time an address range is seen, page tables in device memory
    // (2 MiB steps: tools/alloc_diag.py), i.e. an allocation inside flm_forward.
    char* bounce = nullptr; size_t bounce_bytes = 0; int err_word = 0; bool err_word_fresh = false;
    bool warmed = false;                               // flm_gpu.hip warm_up: the runtime's lazily built launch resources were set up at load time

    // options
    bool tuning = false;                               // option "tuning": the experiment dials (the kOptDial rows of flm_tuning.h) may be set
    int wg_per_cu = 1; int use_graph = 1; int ablate = 0;
    int graph_chunks = 1;                              // option "graph_chunks": a greedy decode loop replays graphs of up to 16 tokens (0: one graph launch per token)
    int use_mfma = 1;                                  // option "use_mfma": int8 prefill GEMM tile shape on v_mfma_i32_32x32x32_i8: 1 by size, 2 (0) 64 x 64, 3 128 x 128
    int use_prefill = 1;                               // option "use_prefill": prompts of >= kPrefillMin+1 tokens go through the batched kernels
    int pf_cap = 0;                                    // token capacity of the batched-prefill buffers below
    bool pf_in_xbuf = false;                           // tensor parallel: pf_x / pf_att / pf_hd are regions of the exchange buffer (peers store into them)
    float *pf_x = nullptr, *pf_qkv = nullptr, *pf_q = nullptr, *pf_att = nullptr, *pf_gu = nullptr, *pf_hd = nullptr, *pf_xs = nullptr, *pf_xst = nullptr; void* pf_xq = nullptr;
    int use_prefill_mq = 1;                            // option "use_prefill_mq": batched prefill attention with 8 queries per workgroup (0: one query per workgroup)
    int use_pv_mfma = 1;                               // option "use_pv_mfma": prefill weighted sum (softmax x V) on the matrix cores as well (needs use_qk_mfma), 0: VALU chains
    int use_qk_mfma = 1;                               // option "use_qk_mfma": prefill scores on the matrix cores (fp32 MFMA, bit-identical), 0: VALU chains inside the attention kernel
    float* pf_scores = nullptr;                        // [heads][max_seq][max_seq] prefill scores (k_qk_mfma -> k_attn_prefill_mq<true>)
    int fold_xchg = 1;                                 // option "fold_xchg": tensor parallel, peer to peer: the exchanges' flag rounds inside the consuming GEMV launches
    int ranks_on_device = 1;                           // ranks of the group that live on this context's device (flm_p2p_import): folding needs a CU partition each
    int cu_parts = 1;                                  // option "cu_parts": the ctx's stream is confined to 1 / cu_parts of the device's CUs (rank % cu_parts picks which)
    bool tp_prefill = false;                           // tensor parallel: every rank of the group can (and will) feed prompts through the batched kernels
    int fuse_attn_o = 1;                               // option "fuse_attn_o": attention + Wo GEMV in one launch (k_attn_o; single GPU)
    bool st_ready = false;                             // the layer matrices' group-major scale copies (QMat::st) are up to date
    int fuse_ffn = 1;                                  // option "fuse_ffn": FFN13 + FFN2 in one launch (k_ffn; single GPU)
    int fuse_back = 1;                                 // option "fuse_back": attention + Wo + FFN13 + FFN2 in one launch with [W1; W3] stashed in LDS under the attention (k_attn_ffn; single GPU,
                                                       // head size a multiple of 64, one workgroup per head)
    int fuse_token = 1;                                // option "fuse_token": ALL layers of a token in one launch (k_layers: the edge between two layers is a flag round in front of which [Wq; Wk; Wv] streams)
    int tok_nstq = 4, tok_preq = 99 /* 99: by launch (plan_layer) */;                   // options "tok_nstq" / "tok_preq": its stash slots / early waves of [Wq; Wk; Wv]
    void* la_dev[2] = {nullptr, nullptr}; bool la_valid[2] = {false, false}, la_ok[2] = {false, false}; flm::BackArgs la_p[2]; int la_grid[2] = {0, 0}, la_r2[2] = {0, 0};   // k_layers' argument blocks (flm_layers.hip)
    int fuse_tail = 1;                                 // option "fuse_tail": a greedy decode token is ONE launch (k_layers<.., TAIL>: embedding row, all layers, classifier, argmax + state advance); fp32 embedding tables
    void* tail_dev[2] = {nullptr, nullptr}; bool tail_ok[2] = {false, false};   // its argument block per head split (flm_layers.hip)
    unsigned* tail_mem = nullptr;                      // [0] the epoch base of the one-launch token's flag values, [16 ..) one flag line per classifier workgroup, then their argmax slots
    int fuse_layer = 1;                                // option "fuse_layer": ... with the QKV GEMV in front: the whole layer in one launch
    int back_nst13 = -1, back_nst13_head = -1, back_nst2 = 0, back_pre13 = 99 /* 99: by launch (plan_layer) */, back_pre2 = 16;   // options "back_*": k_attn_ffn's stash slots (-1: as many as the LDS holds) and early register set (flm_layer.h)
    int attn_kpre = 1;                                 // option "attn_kpre" (a dial): split heads' first two K tiles by LDS-DMA under the QKV phase (BackArgs::kpre_off)
    int back_nwo = 0;                                  // option "back_nwo" (a dial): waves that hold the arrival-order Wo's steps (0: ceil(steps / 2); 16: every wave, the stash issued by all)
    int gr_edges = 1;                                  // option "gr_edges" (round 6; public: include/flm_gpu.h): the one-launch token's x / x1 hand-offs as data-tagged granules (flm_gemv.h: granule_t; BackArgs::gr); 0: flag rounds
    granule_t* xg = nullptr; size_t x_gran_off = 0;    // ... the granule vectors [x: dim][x1: dim][att: dim][hd: hidden] (tensor parallel: a region of the exchange buffer, at x_gran_off in every rank's)
    int back_ao = 3, back_ao2 = 2;                     // options "back_ao" (bit 0: Wo, bit 1: FFN2 consume their activation in arrival order, GemvCtx::run_ao) / "back_ao2" (what of W2 is requested in front of the first look)
    int fuse_qkv = 1;                                  // option "fuse_qkv": QKV in front of attention + Wo in the same launch (k_qkv_attn_o; single GPU): 0 never,
                                                       // 1 when a head is spread over several workgroups (long contexts: where it pays), 2 always
    unsigned* flag_lines = nullptr; int* xwg_err = nullptr;   // k_attn_o: one 64-byte flag line per head; "a cross-workgroup wait timed out"
    void* att_q = nullptr; float* att_qs = nullptr;    // k_attn_o: the heads' output already quantized (head_size a multiple of 64)
    // tensor parallel, peer-to-peer: ONE exchange buffer per rank -- [att_out | x1 | hd | logits | flag lines] -- shared with the
    // peers (hipIpc); att_out / x1 / hd / logits point into it.  peer[r] = rank r's buffer mapped here (peer[rank] = xbuf).
    char* xbuf = nullptr; size_t xbuf_bytes = 0, x_flags_off = 0, x_hflags_off = 0; bool xbuf_fine = false;
    int tp_fuse_ffn = 0;                               // option "tp_fuse_ffn": the same for FFN13 + FFN2 (k_ffn across ranks: one line per rank, raised by the rank's last workgroup); off by
                                                       // default: on one GPU under CU masks it is slower at 2-4 ranks and faster at 8 (profiles/r03_tp_onegpu.txt) -- a multi-GPU box has to decide
    unsigned long long* ffn_counter = nullptr;         // (its device counter)
    int tp_fuse_attn = 2;                              // option "tp_fuse_attn": tensor parallel with folded exchanges: 1 = attention + Wo GEMV in one launch across the ranks (k_attn_o),
                                                       // 2 (default) = with the QKV GEMV in front (k_qkv_attn_o: its rows are the rank's own heads), 0 = separate launches
    int tp_fuse_layers = 1;                            // option "tp_fuse_layers" (round 6): ALL layers of a sharded token in one launch that spans the ranks (k_layers<.., TP>: the four hand-offs of a layer are
                                                       // flag rounds between the ranks' workgroups, the next phase's weights requested in front of each, exactly as on one GPU); needs what the
                                                       // rank-spanning launches need (grp_span) and ranks of identical geometry
    int tp_fence = -1;                                 // option "tp_fence" (k_layers<.., TP>): bit 0 a system-scope release fence in front of a cross-rank line, bit 1 an acquire fence behind a cross-rank poll;
                                                       // -1 (default): none where every rank of the group lives on THIS device (one memory system), both between distinct devices
    size_t x_tlines_off = 0;                           // ... its flag region in the exchange buffer: [heads: 256 lines][x1, hd, x, cls: world x 256 lines each]
    char* peer[8] = {nullptr}; bool peer_opened[8] = {false}; int p2p = 0;
    // what the tensor-parallel GROUP runs, agreed at flm_p2p_import from every rank's blob (the ranks' hand-off protocols must match or they wait on flags nobody raises):
    // exchanges folded into the consuming launches / launches that span the ranks / tp_fuse_attn / tp_fuse_ffn / attn_split, each the weakest any rank can do.
    // Options set after the import take effect at the next flm_p2p_export + flm_p2p_import round of the whole group.
    bool grp_fold = false, grp_span = false, grp_can_split = false, grp_tpl = false, grp_gr = false /* every rank has "gr_edges": the rank-spanning launch's vectors are granules */; int grp_tpfa = 0, grp_tpff = 0, grp_split = 0;
    int force_tp = 0;                                  // option "force_tp": a context created with an RCCL id but world == 1 takes the sharded token path (RCCL exchanges over a 1-rank communicator: tests)
    int tp_trust_fused = 0;                            // option "tp_trust_fused": ranks on DISTINCT devices run the folded / rank-spanning launches too (validated only between CU partitions of one GPU)
    unsigned* xepoch = nullptr;                        // [4] exchanges done per kind (att, x1, hd, logits), device memory
    float* att_sc = nullptr;                           // [heads_local][max_seq] scores exchanged between the parts of a split head
    int attn_split = 1;                                // option "attn_split": 1 = spread a head over 4 workgroups from kSplitFrom (128) positions on, 0 = never, >= 2 = always that many
    unsigned* eng_base = nullptr;                      // the token's epoch base (device memory, advanced by k_embed): the tensor-parallel exchanges' flag values count from it
    int resident = 1;                                  // the census at create saw every workgroup of a cu_count-wide launch co-resident
    int fell_back = 0;                                 // how many times a cross-workgroup wait timed out and the context went to one kernel per phase ("fallback")
    bool fb_active = false; int fb_tokens = 0; std::vector<int> fb_saved;   // ... it is there now / tokens since / the launch structure it had (the kOptFallback rows of flm_tuning.h, in row order; restored when the census passes again: maybe_recover)
    int trace_class = -1; unsigned long long* trace = nullptr;   // FLM_ABLATE builds: GEMV timeline of one kernel class
    // the device sampler (flm_sample.h): per-call parameters written at the start of each flm_forward_sample / flm_decode_sample (the token graphs read them), the radix
    // sort's ping-pong buffers [16][2][vocab] (one [2][vocab] slice per row of a sampled verify batch; the token path sorts in slice 0; null where the vocabulary is beyond
    // the sampler: sample_supported), and how many tokens this context sampled on the device ("sampled_tokens")
    flm::SampleParams* sparams = nullptr; unsigned long long* sort_buf = nullptr; long long sampled = 0;
    // the logit shaper (flm_shape.h): its per-call parameter block (controls, bias pairs, the prompt's tail for the penalty window: written at the start of each flm_generate_ex /
    // flm_forward_sample_ex), the shaped row [vocab] the sampler reads in the shaped token form, and how many tokens this context drew through that form ("shaped_tokens")
    flm::ShapeParams* shape_p = nullptr; float* shape_row = nullptr; long long shaped = 0;
    flm::ShapeParams* shape_stage = nullptr;           // ... the block's own page-locked staging copy (the bounce buffer carries the prompt in the same call)
    // constrained decoding (include/flm_gpu.h flm_constraint_set / _arm; the mask: flm_shape.h step 0): the device block the shaped token graphs reach the automaton
    // through (allocated at create; only its contents change), the automaton's three arrays in ONE device allocation made by flm_constraint_set, the host copy the state is
    // folded over after every call, and the armed state (-1: disarmed; "constraint_state")
    flm::DfaBlock* dfa_blk = nullptr; int* dfa_dev = nullptr;
    std::vector<int32_t> dfa_row, dfa_tok, dfa_nxt; int dfa_state = -1;
    // flm_generate (flm_calls.hip): the granule ring [max_seq_len] and the cancel word -- page-locked, mapped, host-coherent memory allocated at create (gen_host; the device's view of it:
    // gen_ring_dev / gen_cancel_dev) --, what set_state writes into the decode state's generate words (gen_stop .. gen_max: -1 / 0 / 0 outside a flm_generate call), the
    // per-attempt sequence number the granules are tagged with, a pageable staging buffer for the ids, and the last call's figures ("gen_tokens" / "gen_streamed")
    unsigned long long* gen_host = nullptr; unsigned long long* gen_ring_dev = nullptr; const int* gen_cancel_dev = nullptr; int gen_cap = 0;
    int gen_stop = -1; unsigned gen_tag = 0; int gen_max = 0; unsigned gen_seq = 0;
    int gen_rules = 0;                                 // ... and DecodeState::stop_rules: 1 while flm_generate_ex enqueues an attempt under installed stop rules, else 0
    std::vector<int32_t> gen_ids; int gen_tokens = 0, gen_streamed = 0;
    // flm_score_tokens (flm_calls.hip; the classifier stage: flm_prompt.hip): the rows' targets and statistics in device memory [max_seq_len] (allocated at create), and the
    // classifier's scales group-major (cls.st) for the GEMM tiles, transposed once per set of weights
    int* score_tgt = nullptr; flm::ScoreRow* score_dev = nullptr; bool cls_st_ready = false;
    // draft-and-verify, greedy, sampled and under the controls (flm_calls.hip verify_impl / generate_lookup_impl; kernels: flm_spec.h, flm_shape.h k_shape_rows): the call's token history [max_seq_len + 32], the batch rows'
    // ids [16] (first maxima or draws) and the step's result block (the accepted ids and the sampler's state behind them, one trip), device memory since create; which GEMM
    // the verify pass runs; the last call's figures ("spec_steps" / "spec_accepted")
    int* spec_hist = nullptr; int* spec_arg = nullptr; flm::SpecOut* spec_res = nullptr;
    int spec_gemm = 0;                                 // option "spec_gemm": 1 = the verify pass's int8 GEMMs through k_gemm_q8_skinny (B <= 16), 0 (default until both forms have been timed: DESIGN.md section 5e) = the 64 x 64 tiles; the new entry points only
    int spec_steps = 0, spec_accepted = 0;
    // the model-based drafter (include/flm_gpu.h flm_draft_set / flm_generate_draft; flm_calls.hip generate_lookup_impl): the paired draft context (not owned; null: none),
    // the two events that order its stream and this one -- [0] recorded here, waited for there, in front of everything the draft enqueues; [1] recorded there, waited for
    // here, behind it -- created by flm_draft_set, and how many tokens the draft computed in the last call ("draft_tokens").  The draft's error word travels to the second
    // word of this context's bounce line (bounce + bounce_bytes + 4), next to its own
    flm_ctx* draft = nullptr; hipEvent_t draft_ev[2] = {nullptr, nullptr}; int draft_tokens = 0;
    // per-token log-probabilities (include/flm_gpu.h flm_logprobs_arm; the stage: flm_logprob.h): the armed setting (top_n -1: off; "logprobs_top_n") and its device block,
    // the records [max_seq_len] with their attempt tags, and the side rows [16][vocab] a verify batch is shaped into when the raw rows must survive -- all device memory
    // since create (null where the context is sharded or the vocabulary is beyond the sampler: arming refuses there).  lp_count: the records the last _ex call left
    // (-1: it ran disarmed, failed, or there was none)
    int lp_top_n = -1, lp_source = 0, lp_count = -1;
    flm::LogprobBlock* lp_blk = nullptr; flm::LogprobRec* lp_rec = nullptr; unsigned* lp_tags = nullptr; float* lp_side = nullptr;
    // stop rules (include/flm_gpu.h flm_stop_set; the matcher: flm_stop.h): the rule block in device memory since create (the shaped token graphs hold the pointer; only its
    // contents change), the host copy the finish reason is computed from (n_ids = n_seqs = 0: none installed; "stop_rules"), and why the last generate-family call ended
    // ("stop_reason" / "stop_rule")
    flm::StopBlock* stop_blk = nullptr; flm::StopBlock stop_host{}; int stop_reason = 0, stop_rule = 0;
    // the entropy-driven samplers (include/flm_gpu.h flm_entropy_set; the stages: flm_entropy.h): the setting's device block since create (null where the context is sharded
    // or the vocabulary is beyond the sampler: the setting refuses there; the entropy token graphs hold the pointer, Draw::arm rewrites its contents from `ent` at the start
    // of every attempt), the host copy -- ent.mu is Mirostat's state behind the ids delivered so far, moved by Draw::commit alone --, the mode (0 off, 1 typical, 2 Mirostat;
    // "entropy") and the state the last attempt's read-back brought along (Draw::fetch; committed only when the attempt is verified)
    flm::EntropyBlock* ent_blk = nullptr; flm_entropy ent{}; int ent_mode = 0; float ent_mu_fetched = 0.0f;
    // parallel sampling (include/flm_gpu.h flm_generate_n / flm_fan_keep; flm_calls.hip; kernels: flm_fan.h): a step's drawn ids [16] and the states behind the draws [16],
    // its result block (one trip per step) -- device memory since create --, and what flm_fan_keep needs of the last call: its layout and every sequence's count
    // (fan_valid: until the next call that writes the cache)
    int* fan_drawn = nullptr; unsigned long long* fan_after = nullptr; flm::FanOut* fan_res = nullptr;
    flm_fan_layout fan_lay{}; int fan_count[FLM_FAN_MAX] = {0}; bool fan_valid = false;
    // cache slots (include/flm_gpu.h flm_batch_*; flm_calls.hip; kernels: flm_batch.h): the open batch's layout, what the host holds of every slot between two steps, and
    // the step's result block in device memory since create (the drawn ids and the states behind the draws share the fan's two arrays).  batch_open: until flm_batch_close
    // or the next call of another entry point that writes the cache
    // A FILLING slot (flm_batch_admit): admitted, its prompt not yet wholly in the cache -- prompt (the CALLER's ids: valid until the slot has delivered its token 0),
    // n_prompt, and fed = the rows flm_batch_pass has verified so far; it turns into a running slot behind the pass that feeds its last row
    struct BatchSlot { bool used = false, live = false; int pos = 0, last = 0, n_out = 0, max_tokens = 0, stop = -1, reason = 0; float temp = 0.0f, topp = 0.0f; unsigned long long rng = 0;
                       bool filling = false; const int32_t* prompt = nullptr; int n_prompt = 0, fed = 0; };
    flm_batch_layout batch_lay{}; BatchSlot batch_slot[FLM_BATCH_MAX]; bool batch_open = false; flm::SlotOut* batch_res = nullptr;
    flm::AttnArgs* batch_views = nullptr;              // ... and the rows' views of the cache for k_attn_slots [FLM_BATCH_MAX], rewritten in front of every layer's attention
    flm::AttnArgs* seg_views = nullptr;                // ... the prompt segments' views for k_attn_segs_mq / k_attn_segs [FLM_BATCH_MAX] (flm_segs.h), device memory since create
    std::vector<int32_t> pass_ids;                     // flm_batch_pass: the pass's prompt rows gathered from the callers' prompts on their way to the device [max_seq_len], sized at create
    int batch_rows = -1;                               // option "batch_rows": flm_generate_batch admits every request and runs flm_batch_pass(batch_rows) (-1: serial joins, then steps)
    int batch_passes = 0;                              // flm_query "batch_passes": weight passes (joins, steps, passes) since the last flm_batch_open
    int score_rows = 0;                                // option "score_rows": rows per classifier chunk of flm_score_tokens (0: as many as the staging holds; < 0: one row at a time through c->logits)
    std::map<GraphKey, hipGraphExec_t> graphs;        // the token graphs captured so far (flm_gpu.hip token_graph)
    std::vector<TimedLaunch>* timing = nullptr;
    std::vector<void*> owned;                          // every device allocation that lives as long as the context (flm_gpu.hip dev_alloc); flm_ctx_destroy frees these
    std::string err;
};
#include "flm_tuning.h"                                           // (the option table: member pointers into flm_ctx)

namespace fh {

#define HIPC(ctx, expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) { \
    char b_[512]; snprintf(b_, sizeof b_, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
    if (ctx) (ctx)->err = b_; g_last_error = b_; return FLM_ERR_HIP; } } while (0)
#define NCCLC(ctx, expr) do { ncclResult_t r_ = (expr); if (r_ != ncclSuccess) { \
    char b_[512]; snprintf(b_, sizeof b_, "%s failed: %s (%s:%d)", #expr, ncclGetErrorString(r_), __FILE__, __LINE__); \
    if (ctx) (ctx)->err = b_; g_last_error = b_; return FLM_ERR_COMM; } } while (0)

int fail(flm_ctx* c, int code, const char* msg);
int esz_of(int qt);
void split_even(int total, int parts, int idx, int* begin, int* count);

// Pass geometry of k_gemv for one launch (flm_token.hip)
struct GemvPlan { int Rm, cb_shift, grid, nbuf; size_t lds; };
GemvPlan gemv_plan(int n, int esz, int rows, bool two, bool pairs, bool norm, int wgs);
// fill the pass geometry of one GEMV into its argument block; returns the LDS bytes and grid it needs
inline int plan_gemv(flm_ctx* c, GemvArgs& a, int esz, int pro, int epi, int wgs, GemvPlan& P) {
    const bool TWO = epi == EPI_SWIGLU, PAIRS = epi == EPI_ROPE_KV;
    const int rows = a.items * (PAIRS ? 2 : 1);
    if ((double)rows * a.n * esz * (TWO ? 2 : 1) >= 2147483648.0) return fail(c, FLM_ERR_UNSUPPORTED, "gemv: matrix of 2 GiB or more");
    P = gemv_plan(a.n, esz, rows, TWO, PAIRS, pro == PRO_RMSNORM_QUANT, wgs);     // (the chain staging area only where an rmsnorm prologue runs)
    if (P.lds > kLdsMax) return fail(c, FLM_ERR_UNSUPPORTED, "gemv: activation vector does not fit LDS");
    a.rows_per_pass = P.Rm; a.cb_shift = P.cb_shift; a.nbuf = P.nbuf;
    return FLM_OK;
}
template <int QT, int PRO, int EPI>
int plan_gemv(flm_ctx* c, GemvArgs& a, int wgs, GemvPlan& P) { return plan_gemv(c, a, QTraits<QT>::kEsz, PRO, EPI, wgs, P); }
// rounds of the activation sweep: every thread of a workgroup takes four elements of the n per round
inline int gemv_rounds(int n) { return (n + kGemvBlock * 4 - 1) / (kGemvBlock * 4); }
// the kernels' rounds template argument (XR / XR2) for a sweep of 1 .. 3 rounds: 1 | 3
inline int rounds_class(int rounds) { return rounds <= 1 ? 1 : 3; }
template <int QT, int PRO, int EPI, bool COH>
int launch_gemv_xr(flm_ctx* c, hipStream_t st, GemvArgs a, int wgs) {
    GemvPlan P;
    int r = plan_gemv<QT, PRO, EPI>(c, a, wgs, P); if (r) return r;
    const int rounds = gemv_rounds(a.n);
    if (PRO == PRO_NONE)   hipLaunchKernelGGL((k_gemv<QT, PRO, EPI, 0, COH>), dim3(P.grid), dim3(kGemvBlock), P.lds, st, a);
    else if (rounds <= 1)  hipLaunchKernelGGL((k_gemv<QT, PRO, EPI, 1, COH>), dim3(P.grid), dim3(kGemvBlock), P.lds, st, a);
    else if (rounds <= 3)  hipLaunchKernelGGL((k_gemv<QT, PRO, EPI, 3, COH>), dim3(P.grid), dim3(kGemvBlock), P.lds, st, a);
    else                   hipLaunchKernelGGL((k_gemv<QT, PRO, EPI, 0, COH>), dim3(P.grid), dim3(kGemvBlock), P.lds, st, a);
    HIPC(c, hipGetLastError());
    return FLM_OK;
}
// coh: the activation a.x holds slices written by peer GPUs (tensor parallel, peer-to-peer) -> system-coherent loads
template <int PRO, int EPI>
int launch_gemv(flm_ctx* c, hipStream_t st, int qt, const GemvArgs& a, int wgs, bool coh = false) {
    if (a.n % kGroup != 0 || a.n <= 0) return fail(c, FLM_ERR_INVALID, "gemv: n must be a positive multiple of 64");
    if (qt != FLM_QT_INT8 && qt != FLM_QT_INT16) return fail(c, FLM_ERR_UNSUPPORTED, "gemv: quant type must be INT8 or INT16");
    if constexpr (PRO != PRO_NONE) {
        if (coh) return qt == FLM_QT_INT8 ? launch_gemv_xr<QT_INT8, PRO, EPI, true>(c, st, a, wgs) : launch_gemv_xr<QT_INT16, PRO, EPI, true>(c, st, a, wgs);
    }
    return qt == FLM_QT_INT8 ? launch_gemv_xr<QT_INT8, PRO, EPI, false>(c, st, a, wgs) : launch_gemv_xr<QT_INT16, PRO, EPI, false>(c, st, a, wgs);
}
// workgroups to spread a GEMV over: wg_per_cu per CU
inline int gemv_grid(int cu_count, int wg_per_cu, int /*items*/, int /*rows_per_item*/) { return cu_count * wg_per_cu; }
int quantize_flat(flm_ctx* c, hipStream_t st, int qt, void* q, float* s, const float* x, size_t n);

// k_attn_o & co. report a cross-workgroup wait that never completed through *xwg_err (flm_gpu.hip)
constexpr int FLM_RETRY = 1;
int xwg_check(flm_ctx* c);

struct Tick {
    flm_ctx* c; hipStream_t st; int kclass; hipEvent_t e0 = nullptr, e1 = nullptr;
    Tick(flm_ctx* c_, hipStream_t st_, int k) : c(c_), st(st_), kclass(k) {
        if (c->timing) { hipEventCreate(&e0); hipEventCreate(&e1); hipEventRecord(e0, st); }
    }
    ~Tick() { if (c->timing) { hipEventRecord(e1, st); c->timing->push_back({kclass, e0, e1}); } }
};

// peer-to-peer tensor parallelism: where `p` (a pointer into this rank's exchange buffer) lies in every peer's buffer
template <class A> void set_peers(flm_ctx* c, A& a, float* p) {
    a.n_peer = 0;
    if (!c->p2p) return;
    const size_t off = (char*)p - c->xbuf;
    for (int r = 0; r < c->world; ++r) if (r != c->rank) a.out_peer[a.n_peer++] = (float*)(c->peer[r] + off);
}
// argument blocks of the five GEMVs and the attention of layer l (flm_token.hip)
GemvArgs args_qkv(flm_ctx* c, int l);
constexpr int kSplitFrom = 128;
constexpr int kTpLinesPerRank = 256;                 // k_layers<.., TP>: flag lines per rank and kind in the exchange buffer's region (one per workgroup of a launch)
int attn_parts(const flm_ctx* c, int T);
AttnArgs args_attn(flm_ctx* c, int l, int G = 1);
GemvArgs args_o(flm_ctx* c, int l);
GemvArgs args_ffn13(flm_ctx* c, int l);
GemvArgs args_ffn2(flm_ctx* c, int l);
GemvArgs args_cls(flm_ctx* c);
void set_fold(flm_ctx* c, GemvArgs& a, int l, int kind);
// the argument blocks, the launch geometry and the stash sizes of layer l for k_attn_ffn / k_layers, by quant type (flm_layerlaunch.hip plan_layer: see there for `tail`)
int plan_layer_qt(flm_ctx* c, int qt, int l, bool with_qkv, int G, LayerArgs& A, BackArgs& p, int& grid, int& r2, TailArgs* tail);
// the whole decoder layer (with_qkv) / attention .. FFN2 of layer l in one launch (flm_layerlaunch.hip); FLM_ERR_UNSUPPORTED when the shape does not allow it
int launch_layer(flm_ctx* c, hipStream_t st, int qt, int l, bool with_qkv, int G = 1);
// all layers of a token in one launch (flm_layers.hip): the argument blocks are built outside any capture
int layers_prepare(flm_ctx* c, int G);
int launch_layers(flm_ctx* c, hipStream_t st, int l0, int l1, int G, bool tail = false);   // G: workgroups per head (attn_parts); tail: the whole greedy token (FLM_ERR_UNSUPPORTED where that launch does not exist)
// one activation exchange between the tensor-parallel ranks (flm_token.hip)
enum XKind { XK_ATT = 0, XK_X1 = 1, XK_HD = 2, XK_LOGITS = 3 };
int exchange(flm_ctx* c, hipStream_t st, int kind, float* full, float* mine, int count);
int enqueue_token(flm_ctx* c, hipStream_t st, bool with_cls, TokenForm form, int G);
int launch_logprob_token(flm_ctx* c, hipStream_t st);                  // (flm_token.hip: the armed form's last launch)
// flm_sampling -> the shaper's parameter block (flm_calls.hip): validates everything include/flm_gpu.h lists (null on success, else what is wrong); window[n_window] becomes the
// block's head; *active: some control is not neutral.  follow: flm_generate_ex's sliding window (penalty_last_n), else the window as given
const char* shape_fill(const flm_sampling* sp, int vocab, const int32_t* window, int n_window, bool follow, flm::ShapeParams* out, bool* active);
int run_token(flm_ctx* c, bool with_cls, TokenForm form, int T);
// the device sampler's LDS fits one workgroup (vocab up to ~36 K); beyond it the sampled entry points refuse (FLM_ERR_UNSUPPORTED) and a caller samples on the host
inline bool sample_supported(const flm_ctx* c) { return c->d.vocab_size >= 2 && sample_lds_bytes(c->d.vocab_size) <= kLdsMax; }
int set_state(flm_ctx* c, int pos, int tok, int step);
// the decode state's latch as the single-GPU token launches receive it (flm_math.h DecodeState::halt); the tensor-parallel launch forms get none and run unconditionally
// this context runs the sharded (tensor-parallel) token path; a 1-rank communicator takes it only on request ("force_tp")
inline bool sharded(const flm_ctx* c) { return c->world > 1 || (c->comm != nullptr && c->force_tp); }
// per-token log-probabilities can be armed: one GPU, the vocabulary within the sampler's LDS strip (the sum chain's bound; flm_score_tokens has the same)
inline bool logprobs_supported(const flm_ctx* c) { return !sharded(c) && sample_supported(c); }
// the entropy-driven samplers can be set: the same bound (the stage runs on the sampler's strip), and the block exists
inline bool entropy_supported(const flm_ctx* c) { return !sharded(c) && sample_supported(c) && c->ent_blk != nullptr; }
inline const int* halt_ptr(const flm_ctx* c) { return sharded(c) ? nullptr : &c->state->halt; }

// The token's launch plan: which launch forms a token of this context may take, decided in ONE place.  enqueue_token tries the forms that run() in its order of
// preference (a form answers FLM_ERR_UNSUPPORTED where the shape does not allow it: the next one is tried), flm_kernel_times times the forms the options allow and
// flm_query("token_path") reports them.  DESIGN.md section 5: the table of forms.
// In enqueue_token's order of preference: the whole greedy token (k_layers<.., TAIL>), all layers (k_layers), ... in one launch per rank that spans the ranks (k_layers<.., TP>),
// the whole layer (k_attn_ffn<.., QKV>), QKV + attention + Wo (k_qkv_attn_o), attention + Wo + FFN13 + FFN2 (k_attn_ffn), attention + Wo (k_attn_o), FFN13 + FFN2 (k_ffn)
enum Launch { LF_TOKEN = 0, LF_LAYERS, LF_LAYERS_TP, LF_LAYER, LF_QKV_ATTN_O, LF_BACK, LF_ATTN_O, LF_FFN, kLaunchForms };
// What instrumentation takes away.  Timing (flm_kernel_times across ranks: one event pair per phase) leaves no fused form.  A trace (FLM_ABLATE builds, option "trace")
// stamps the timeline of ONE kernel class: the form that class belongs to still runs, every other one steps aside.  -1: the form runs under no trace
constexpr int trace_admits(Launch f) { return f == LF_TOKEN || f == LF_LAYERS ? 103 : f == LF_LAYER || f == LF_BACK ? 102 : f == LF_ATTN_O ? 101 : -1; }
// "fuse_token": the all-layers forms are wanted (token_plan; layers_prepare / launch_layers and plan_layer build for them on this alone: their checks are the shape's)
inline bool wants_layers(const flm_ctx* c) { return c->fuse_token != 0; }
struct TokenPlan {
    bool opt[kLaunchForms];                        // what the OPTIONS allow on one GPU, whatever this context is: each form its own option and the forms it is made of (flm_kernel_times, "token_path")
    int qkv;                                       // "fuse_qkv" where attention + Wo is fused at all: 0 never in front of it, 1 with split heads, >= 2 always
    bool tp, coh, fold, span; int tpfa, tpff;      // sharded; peers store into the activations; flag rounds folded into the consuming launches; launches span the ranks, as agreed for "tp_fuse_attn" / "tp_fuse_ffn"
    bool use[kLaunchForms];                        // what THIS CONTEXT's token may try (enqueue_token, through runs()): one GPU: opt; sharded: none but the rank-spanning forms the group agreed on
    bool timing; int trace_class;
    bool runs(Launch f) const { return use[f] && !timing && (trace_class < 0 || trace_class == trace_admits(f)); }
};
inline TokenPlan token_plan(const flm_ctx* c, int G) {   // G: workgroups per head (attn_parts)
    TokenPlan P{};
    bool* o = P.opt;
    o[LF_ATTN_O] = c->fuse_attn_o != 0;
    o[LF_FFN] = c->fuse_ffn != 0;
    P.qkv = o[LF_ATTN_O] ? c->fuse_qkv : 0;
    o[LF_QKV_ATTN_O] = P.qkv >= 2 || (P.qkv && G > 1);
    o[LF_BACK] = c->fuse_back && o[LF_ATTN_O] && o[LF_FFN];
    o[LF_LAYER] = c->fuse_layer && o[LF_BACK];
    o[LF_LAYERS] = wants_layers(c) && o[LF_LAYER];
    o[LF_TOKEN] = c->fuse_tail && o[LF_LAYERS];
    o[LF_LAYERS_TP] = wants_layers(c);
    P.tp = sharded(c); P.coh = P.tp && c->p2p;
    P.fold = P.tp && c->p2p && c->world > 1 && c->grp_fold;          // (agreed by the group at flm_p2p_import)
    P.span = P.fold && c->grp_span;                                   // (they wait across workgroups of one launch too: only where the census found one workgroup per CU resident)
    P.tpfa = P.span ? c->grp_tpfa : 0; P.tpff = P.span ? c->grp_tpff : 0;
    for (int f = 0; f < kLaunchForms; ++f) P.use[f] = !P.tp && o[f];
    P.use[LF_LAYERS_TP] = P.span && c->grp_tpl && o[LF_LAYERS_TP];
    P.use[LF_QKV_ATTN_O] |= P.tpfa >= 2; P.use[LF_ATTN_O] |= P.tpfa != 0; P.use[LF_FFN] |= P.tpff != 0;
    P.timing = c->timing != nullptr; P.trace_class = c->trace_class;
    return P;
}

// the quant types and rounds classes the fused kernels' variant lists are made of (flm_launch.h)
using VQuant = Variants<Variant<QT_INT8>, Variant<QT_INT16>>;
using VRounds = Variants<Variant<1>, Variant<3>>;
inline int quant_variant(int qt) { return qt == FLM_QT_INT8 ? QT_INT8 : QT_INT16; }
// a launch that stashes weights takes the CU's whole LDS: raise the dynamic-LDS limit of EVERY instantiation in the list the launch dispatches over, once per device
// (kernel_of: a list entry -> the kernel's address; the launch goes through the same function)
template <class List, class KernelOf> int raise_lds_limit(flm_ctx* c, KernelOf kernel_of) {
    static std::mutex mu; static bool done[64] = {false};
    std::lock_guard<std::mutex> lk(mu);
    if (c->device >= 0 && c->device < 64 && !done[c->device]) {
        std::vector<const void*> fns;
        for_each_variant(List{}, [&](auto v) { fns.push_back((const void*)kernel_of(v)); });
        for (const void* f : fns) HIPC(c, hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsMax));
        done[c->device] = true;
    }
    return FLM_OK;
}
// ids[0 .. n) lie in [0, vocab)
inline bool ids_in_vocab(const flm_ctx* c, const int32_t* ids, int n) {
    for (int i = 0; i < n; ++i) if (ids[i] < 0 || ids[i] >= c->d.vocab_size) return false;
    return true;
}
struct SpecDraw;
// How a call draws its tokens, resolved ONCE at the entry point (flm_calls.hip: the plain entry points construct it, the _ex ones go through draw_resolve) and the only
// thing an implementation receives about drawing.  An implementation asks for the form, arms its attempts and commits; which of a control, an armed constraint or a context
// armed for log-probabilities made the form shaped it cannot tell and need not know.
struct Draw {
    float temperature, topp; uint64_t* rng_state;
    TokenForm form;                                               // Greedy / Sampled by temperature (sampler: Sampled whatever the temperature -- flm_forward_sample / flm_decode_sample); shape_by: Shaped / ShapedLp
    flm::ShapeParams block;                                       // the shaper's parameter block (shaped forms only)
    int cstate = -1;                                              // the constraint's state at the call's first token (-1: none; only with the block: an armed constraint counts as a control)
    bool lp = false;                                              // the context is armed for log-probabilities: the form is ShapedLp, record i is the call's i-th id's
    bool rules = false;                                           // stop rules are installed and this entry point honours them (flm_generate_ex / flm_generate_lookup_ex; only with the block)
    int ent = 0; float typical_p = 0.0f;                          // flm_entropy_set is on (1 typical, 2 Mirostat): the form is ShapedEnt; a verify batch's rows get stage 5 (typical only)
    Draw(float t = 0.0f, float p = 0.0f, uint64_t* st = nullptr, bool sampler = false) { plain(t, p, st, sampler); }
    void plain(float t, float p, uint64_t* st, bool sampler = false) { temperature = t; topp = p; rng_state = st; form = t != 0.0f || sampler ? TokenForm::Sampled : TokenForm::Greedy; }
    void shape_by(int cq, bool armed, int entropy = 0, float tp = 0.0f) {                                                   // `block` is filled: the shaped form runs
        form = entropy ? TokenForm::ShapedEnt : armed ? TokenForm::ShapedLp : TokenForm::Shaped; cstate = cq; lp = armed; ent = entropy; typical_p = entropy == 1 ? tp : 0.0f;
    }
    bool mu_moves() const { return ent == 2 && temperature != 0.0f; }   // Mirostat's state is read back and committed
    bool shaped() const { return shaped_form(form); }
    bool coins() const { return form == TokenForm::Sampled || (shaped() && temperature != 0.0f); }   // the caller's state is read and moved on
    // an attempt's start: the shaper's block, the constraint's {state, 0}, the record stage's base, then the sampler's parameters FROM THE CALLER'S STATE -- a retried attempt draws nothing twice
    int arm(flm_ctx* c) const { return arm_with(c, block, coins() ? (unsigned long long)*rng_state : 0ull, cstate, 0); }       // (rng_state may be null where no coin is drawn)
    // a later single-token step of a call that holds its running copies on the host (generate_lookup_impl): the sampler's state, the constraint's state and the record base
    // as they stand behind the n_hist = n_prompt + n_drawn ids so far; the block's head is the window as given, the last min(last_n, n_hist) ids of prompt ++ drawn
    int arm_step(flm_ctx* c, unsigned long long rng, int q, int rec_base, const int32_t* prompt, int n_prompt, const int32_t* drawn, int n_drawn) const;
    int arm_block(flm_ctx* c) const;       // a verify batch's attempt: the block alone (the rows' draws take everything else as launch arguments: batch)
    // the batch form of this plan for one verify step: what varies per step is the xorshift state its rows' coins count from, the window in device memory
    // (win[0 .. n_win) ++ the drafts in front of a row; win null: the block's own head, as the last arm_block left it), the constraint's state at row 0 and the record index of row 0
    SpecDraw batch(const flm_ctx* c, unsigned long long base, const int* win, int n_win, int q, int rec_base) const;
    int fetch(flm_ctx* c, unsigned long long* after) const;       // an attempt's end: the state behind its draws comes back (and Mirostat's, into flm_ctx::ent_mu_fetched)
    // a verified attempt that delivered ids[0 .. n) and left the sampler's state `after`: the ONE place that writes the caller's state, "sampled_tokens" / "shaped_tokens",
    // "constraint_state" (folded over the ids; q_after: the caller folded step by step), the count of records flm_last_logprobs hands out and Mirostat's mu
    void commit(flm_ctx* c, const int32_t* ids, int n, unsigned long long after) const;
    void commit(flm_ctx* c, int n, unsigned long long after, int q_after) const;
private:
    int arm_with(flm_ctx* c, const flm::ShapeParams& blk, unsigned long long rng, int q, int rec_base) const;
};
int check_ready(flm_ctx* c, int n, int pos);
// what flm_calls.hip calls of flm_gpu.hip (the context's state and the graph cache), then what flm_gpu.hip calls of a call's plumbing (warm_up, flm_debug_read)
bool model_complete(const flm_ctx* c);
int run_tokens(flm_ctx* c, int pos, int n, TokenForm form);
int maybe_recover(flm_ctx* c, int tokens);
int feed(flm_ctx* c, const int32_t* tokens, int n, int pos, TokenForm last);
int d2h(flm_ctx* c, void* dst, const void* src_dev, size_t bytes);
float* score_stage(const flm_ctx* c, int* chunk);
constexpr int kPrefillMin = 4;
int prefill_batched_qt(flm_ctx* c, int B, int pos, bool all_layers = false, bool skinny = false, const flm::FanDesc* fan = nullptr, int row0 = 0, const flm::SlotDesc* slots = nullptr, const flm::SegDesc* segs = nullptr);      // (flm_prompt.hip; by the model's quant type.  all_layers: the last layer is completed too -- flm_score_tokens needs every row's final residual; skinny: int8 and B <= 16: every GEMM through k_gemm_q8_skinny -- the verify pass under "spec_gemm" 1; fan: the rows are a fan step's -- flm_generate_n; row0: the batch is a prompt entering the cache slot that starts at physical row row0 -- flm_batch_join; slots: the rows are a batch step's -- flm_batch_step; segs: a ragged pass -- flm_batch_pass: rows [0, n_step) are a step's (slots, where n_step > 0), the rest prompt segments)
// a fan step's pieces (flm_prompt.hip; kernels: flm_fan.h).  fan_classify: rows [row0, row0 + m) through score_classify's prologue and GEMM into `stage`, then k_sample_fan
// into fan_drawn / fan_after, row j with in.rng[j].  The launchers take c == null from the op-level mirror (flm_op_attention_fan)
int fan_classify(flm_ctx* c, int row0, int m, float* stage, bool skinny, float temperature, float topp, const flm::FanIn& in);
int launch_sample_fan(flm_ctx* c, hipStream_t st, const float* logits, int ld, int n, int row0, int rows, float temperature, float topp, const flm::FanIn& in,
                      unsigned long long* sort_buf, int* drawn, unsigned long long* after);
// a batch step's pieces (flm_prompt.hip; kernels: flm_batch.h).  batch_classify: batch rows [src_row0, src_row0 + m) through score_classify's prologue and GEMM into `stage`,
// then k_sample_slots into fan_drawn / fan_after, chunk row i with the parameters and state of in's row row0 + i.  The launchers take c == null from flm_op_attention_slots
int batch_classify(flm_ctx* c, int src_row0, int row0, int m, float* stage, bool skinny, const flm::SlotIn& in);
int launch_attn_slots(flm_ctx* c, hipStream_t st, const flm::AttnArgs& aa, const flm::SlotDesc& f, int heads, int row_stride, flm::AttnArgs* views);
int launch_rope_kv_slots(flm_ctx* c, hipStream_t st, const float* qkv, float* qout, float* kcache, float* vcache, const float* rope_cos, const float* rope_sin, int dim, int hs, int kv_rows, const flm::SlotDesc& f);
// a ragged pass's pieces (flm_prompt.hip; kernels: flm_segs.h) for the prompt segments [n_step, n_segs) of f; q / out / qkv are the WHOLE batch's (the views move them);
// one_query: k_attn_segs although the multi-query form would fit; views: device memory for 16 AttnArgs.  seg_check: null, or what is wrong with f as a pass of B rows
// over a cache of max_seq rows.  c may be null (flm_op_attention_segs)
const char* seg_check(const flm::SegDesc& f, int B, int max_seq);
int launch_attn_segs(flm_ctx* c, hipStream_t st, const flm::AttnArgs& aa, const flm::SegDesc& f, int heads, int row_stride, flm::AttnArgs* views, bool one_query);
int launch_rope_kv_segs(flm_ctx* c, hipStream_t st, const float* qkv, float* qout, float* kcache, float* vcache, const float* rope_cos, const float* rope_sin, int dim, int hs, int kv_rows, const flm::SegDesc& f, int B);
int launch_attn_fan(flm_ctx* c, hipStream_t st, const flm::AttnArgs& aa, const flm::FanDesc& f, int heads, int row_stride);
int launch_rope_kv_fan(flm_ctx* c, hipStream_t st, const float* qkv, float* qout, float* kcache, float* vcache, const float* rope_cos, const float* rope_sin, int dim, int hs, int kv_rows, const flm::FanDesc& f);
// flm_score_tokens' classifier stage (flm_prompt.hip): rows [row0, row0 + m) of the batch's final residual (pf_x) -> output norm, quantize, the classifier GEMM tiles into
// `stage` [m][vocab], k_score_rows into score_dev[row0 ..]
int score_classify(flm_ctx* c, int row0, int m, float* stage);
// the verify pass's classifier stage (flm_prompt.hip): score_classify's prologue and GEMM (skinny: k_gemm_q8_skinny), then k_argmax_rows into argmax_out[row0 ..]
// (draw: temperature, top-p and the step's xorshift state: k_sample_rows draws row row0 + i with that state's (row0 + i + 1)-th coin; temperature 0: k_argmax_rows)
// shape (the device block) given: k_shape_rows shapes the chunk's rows in place in front of the draw, row i over the last min(last_n, n_win + i) ids of
// win[0 .. n_win) ++ the batch's drafts in front of it (prompt_dev + 1); null: no shape kernel runs.  Filled by Draw::batch and by nobody else
struct SpecDraw { float temperature, topp; unsigned long long base; const flm::ShapeParams* shape = nullptr; const int* win = nullptr; int n_win = 0; int cstate = -1 /* the batch's base constraint state; -1: none */;
                  float typical_p = 0.0f /* flm_entropy_set, typical: k_entropy_rows between the shaper and the rows' draws; otherwise 0 */;
                  int lp_top_n = -1 /* the context is armed: k_logprob_rows behind the rows' draws, records from lp_base on; -1: not */, lp_source = 0, lp_base = 0; };
// k_shape_rows on `rows` rows (batch rows row0 ..) of n logits, ld floats apart -> out, ld_out apart (out == logits: in place); c may be null: flm_op_shape_rows
int launch_shape_rows(flm_ctx* c, hipStream_t st, const float* logits, int ld, float* out, int ld_out, int n, int row0, int rows, const flm::ShapeParams* p,
                      const int* win, int n_win, const int* drafts, const flm::DfaBlock* dfa = nullptr, int cstate = -1, int* states_out = nullptr);
// stop rules are installed (flm_stop_set refuses where the shaped form could not honour them)
inline bool stop_installed(const flm_ctx* c) { return c->stop_blk != nullptr && (c->stop_host.n_ids | c->stop_host.n_seqs) != 0; }
// delta folded over ids[0 .. n) from state q on the context's host copy of the automaton (flm_calls.hip; q in [0, n_states))
int dfa_fold(const flm_ctx* c, int q, const int32_t* ids, int n);
// the rules of flm_dfa_validate (flm_calls.hip): null, or which one failed
const char* dfa_check(const flm_dfa* dfa, int vocab);
int spec_classify(flm_ctx* c, int row0, int m, float* stage, bool skinny, int* argmax_out, const SpecDraw& draw);
// k_logprob_rows on `rows` <= 16 rows of n logits, ld floats apart, batch rows row0 ..: chosen[row0 + r] the row's drawn id, its record rec[rec_base + row0 + r]
// (flm_prompt.hip; c may be null: flm_op_logprob_rows)
int launch_logprob_rows(flm_ctx* c, hipStream_t st, const float* rows_dev, int ld, int n, int row0, int rows, const int* chosen, int top_n, flm::LogprobRec* rec, int rec_base, int rec_cap);
// k_entropy_rows on `rows` <= 16 rows of n logits, ld floats apart, in place; sort_buf [rows][2][n] (flm_prompt.hip; c may be null: flm_op_entropy_rows)
int launch_entropy_rows(flm_ctx* c, hipStream_t st, const flm::EntropyRowsArgs& a, int rows);
// k_sample_rows on `rows` <= 16 rows of n logits, ld floats apart, batch rows row0 ..; sort_buf [rows][2][n] (flm_prompt.hip; c may be null: flm_op_sample_rows)
int launch_sample_rows(flm_ctx* c, hipStream_t st, const float* logits, int ld, int n, int row0, int rows, float temperature, float topp, unsigned long long base,
                       unsigned long long* sort_buf, int* out);
int launch_gemm_skinny_store(flm_ctx* c, hipStream_t st, const GemmArgs& g, int force_nb = 0);   // (flm_prompt.hip: k_gemm_q8_skinny, plain store epilogue: flm_op_matmul_skinny; c may be null; force_nb 1 / 2: that many 16-row fragments per wave, 0: by size)
// k_score_rows on `rows` rows of n logits, ld floats apart (c may be null: flm_op_score_rows)
int launch_score_rows(flm_ctx* c, hipStream_t st, const float* logits, int ld, int n, const int* targets, flm::ScoreRow* out, int rows);
int launch_gemm_store(flm_ctx* c, hipStream_t st, int qt, const GemmArgs& g, int use_mfma);   // (flm_prompt.hip: one GEMM tile launch, plain store epilogue: flm_op_matmul_q)
void build_rope_table(int hs, int max_seq, std::vector<float>& cs, std::vector<float>& sn);  // (flm_gpu.hip)

} // namespace fh
