/* flm_gpu.h -- C ABI of the MI355X (gfx950) implementation of fast-llama's per-token hot path.
 *
 * The reference (CoderLSF/fast-llama) has no plugin/FFI seam; its path sits behind the C++ class
 * ParallelTransformer (src/transformer/transformer.h:76-99) and the raw-pointer operator set
 * cpuft::quant::* (src/blas/quant_operators.h:37-82) / cpuft::simd::* (src/platforms/arch/simd.h:13-63).
 * This header is the boundary a maintainer would bind instead: one device-resident forward per
 * token (model level) plus 1:1 mirrors of the operator seam (op level, used by the parity tests).
 * Plain pointers and sizes only; no C++/torch types; no exceptions cross it.  Every entry point
 * cites the reference interface it replaces (paths relative to the reference repo root).
 *
 * Threading: one caller thread per ctx at a time (as ParallelTransformer::forward, single caller,
 * transformer.h:101-110).  Independent ctxs (replicas / tensor-parallel ranks) are independent.
 * Ownership: the caller owns every host pointer (copied during the call); the ctx owns all device
 * memory, ALL of it allocated at flm_ctx_create / flm_upload_tensor time (prompt, output-id and batched-prefill buffers are
 * sized by max_seq_len; the launches' argument blocks and every token graph the entry points replay are built when the model's
 * last tensor arrives, at flm_p2p_import, or by flm_prepare) -- nothing is allocated inside flm_forward* / flm_decode_* / flm_generate (the
 * reference's zero-allocation contract, transformer.cpp:110-130; tests/test_gpu_configs.py brackets the first calls with
 * hipMemGetInfo and a hipMalloc interposer).  Exceptions, both off the steady path: after flm_set_option the graphs are
 * re-instantiated by the next call (or by flm_prepare), and so they are when a context returns from a fallback.
 * Robustness: the fused launches hand data between workgroups of one kernel; if a hand-off ever times out (a workgroup not
 * resident because another process holds CUs) the call re-runs its work on one kernel per phase and still returns FLM_OK with
 * correct results; the context stays on that path for 64 tokens, then takes the census again and, if every workgroup is
 * resident, returns to the launch structure it had ("fallback" counts the episodes, "fallback_active" = on that path now).
 */
#ifndef FLM_GPU_H
#define FLM_GPU_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* status codes (reference: bool + printf, src/utils/log.h; here: int + flm_last_error) */
#define FLM_OK               0
#define FLM_ERR_INVALID     -1   /* bad argument / shape */
#define FLM_ERR_UNSUPPORTED -2   /* e.g. n_kv_heads != n_heads (reference GQA path is broken, transformer.cpp:449) */
#define FLM_ERR_HIP         -3   /* HIP runtime error, see flm_last_error */
#define FLM_ERR_OOM         -4
#define FLM_ERR_STATE       -5   /* e.g. forward before all tensors were uploaded */
#define FLM_ERR_COMM        -6   /* RCCL error */

/* QuantType numbering == cpuft::quant::QuantType (src/blas/quant_operators.h:18-25) */
#define FLM_QT_NONE  0
#define FLM_QT_INT16 1
#define FLM_QT_INT8  2

/* tensor kinds == .flm TensorType (src/model_loaders/flm_loader.cpp:50-67) */
#define FLM_T_TOKEN_EMBD  1
#define FLM_T_OUTPUT_NORM 2
#define FLM_T_CLASSIFIER  3
#define FLM_T_INPUT_NORM 17
#define FLM_T_ATTN_Q     18
#define FLM_T_ATTN_K     19
#define FLM_T_ATTN_V     20
#define FLM_T_ATTN_O     21
#define FLM_T_MLP_GATE   22   /* ffn_1 */
#define FLM_T_MLP_UP     23   /* ffn_3 */
#define FLM_T_MLP_DOWN   24   /* ffn_2 */
#define FLM_T_POST_NORM  25

typedef struct flm_ctx flm_ctx;

/* == TransformerConfig (src/model_loaders/model_loader.h:46-68), the fields the path uses.
 * rope_freq_base / rms_norm_eps are NOT here on purpose: the reference ops hard-code 10000 and
 * 1e-5 (tf_operators.cpp:353, x86_simd.cpp:1755) and ignore the file's values. */
typedef struct flm_model_desc {
    int32_t dim;
    int32_t hidden_dim;
    int32_t n_layers;
    int32_t n_heads;
    int32_t n_kv_heads;       /* must equal n_heads (see FLM_ERR_UNSUPPORTED) */
    int32_t vocab_size;
    int32_t max_seq_len;      /* reference clamps to 1024 (transformer.cpp:32); here any length whose scores (4 bytes per position) fit the
                               * LDS beside a head's K/V tiles: ~22 000 positions at head size 128 (FLM_ERR_UNSUPPORTED beyond) */
    int32_t quant_type;       /* FLM_QT_INT8 | FLM_QT_INT16: type of the linear layers and activations */
    int32_t quant_group_size; /* 64 */
} flm_model_desc;

/* ---- lifecycle: replaces ParallelTransformer::load (transformer.cpp:23-42) + parallel_*_init
 *      (transformer.cpp:209-384).  device_id = HIP ordinal.  rank/world/comm_id: tensor-parallel
 *      group.  comm_id = 128 bytes from flm_comm_unique_id() on rank 0, distributed by the caller (RCCL all-gathers, the
 *      fallback exchange), or NULL: then the ranks must be connected peer to peer (flm_p2p_export / flm_p2p_import). */
int  flm_comm_unique_id(void* out128);
int  flm_ctx_create(const flm_model_desc* desc, int device_id, int rank, int world,
                    const void* comm_id, flm_ctx** out);
void flm_ctx_destroy(flm_ctx* ctx);
/* Tensor parallel, peer to peer (world > 1): every rank exports a blob describing its exchange buffer, the caller gathers all
 * ranks' blobs in rank order (any transport) and imports them on every rank; activation slices then travel as direct stores
 * over xGMI plus a flag round instead of RCCL all-gathers, and comm_id may be NULL at create.  The reference's threads share
 * these vectors in memory (transformer.cpp:394,465,482,493,504); this is the same picture across GPUs. */
#define FLM_P2P_BLOB_BYTES 128
int  flm_p2p_export(flm_ctx* ctx, void* blob128);
int  flm_p2p_import(flm_ctx* ctx, const void* blobs /* [world][128] */, int world);
const char* flm_last_error(const flm_ctx* ctx);   /* ctx may be NULL: last create error */

/* Hand one tensor (one layer of it) to the device: what load_tensor (flm_loader.cpp:493-559) +
 * copy_layers (transformer.cpp:289-304) do for the CPU threads.  `values` is row-major
 * [rows][cols] of src_qtype (fp32 when FLM_QT_NONE) with fp32 `scales` [rows][cols/gs] when
 * quantized.  fp32 linear-layer tensors are quantized on the device with the reference's
 * quantizer (A13).  Under tensor parallelism the FULL tensor is passed on every rank; the ctx
 * keeps its row shard. */
int  flm_upload_tensor(flm_ctx* ctx, int kind, int layer, int src_qtype,
                       const void* values, const float* scales, int rows, int cols);
/* Build everything the token entry points use beyond the buffers -- the launches' argument blocks and the hipGraphs of every token form (parallel_thread_init's
 * arena carving, transformer.cpp:110-130,253-384) -- so that the calls below allocate nothing.  Done automatically when the last tensor arrives and at flm_p2p_import;
 * call it after flm_set_option if the next forward must not pay for it.  FLM_ERR_STATE before the model is complete. */
int  flm_prepare(flm_ctx* ctx);

/* ---- the hot path: replaces ParallelTransformer::forward (transformer.h:99, transformer.cpp:105-161).
 * tokens[n] enter at absolute position pos (pos = tokens already in the KV cache);
 * logits_host[vocab] = logits of the LAST token.  n > 5: the first n-1 tokens are evaluated as one batch (MFMA int8 GEMM,
 * causal attention per query) that leaves the same cache rows as feeding them one by one -- bit-identical results. */
int  flm_forward(flm_ctx* ctx, const int32_t* tokens, int n, int pos, float* logits_host);
/* same + sample_argmax (src/transformer/sampler.cpp:36-47, first maximum wins) on the device */
int  flm_forward_argmax(flm_ctx* ctx, const int32_t* tokens, int n, int pos, int32_t* next_token);
/* Device-resident greedy loop == the body of ParallelTransformer::generate (transformer.cpp:92-101)
 * at temperature 0: feeds `first_token` at `pos`, then n_steps-1 further argmax tokens, no host
 * round trip between tokens.  out_tokens[n_steps] receives every sampled token.  Does not stop
 * on token 0: all n_steps tokens are computed (a caller that wants the reference's loop -- stop on a token, per-token
 * callback -- calls flm_generate below; truncating this call's output is the other way). */
int  flm_decode_greedy(flm_ctx* ctx, int32_t first_token, int pos, int n_steps, int32_t* out_tokens);
/* Same loop, nothing copied back; *ms = device time of the n_steps tokens measured with HIP events
 * on the ctx's stream (bench.py's timed region; call flm_sync afterwards is not needed). */
int  flm_decode_timed(flm_ctx* ctx, int32_t first_token, int pos, int n_steps, float* ms);
/* the same with an event after every token: ms_each[n_steps] (medians; the events cost a few us per token) */
int  flm_decode_timed_each(flm_ctx* ctx, int32_t first_token, int pos, int n_steps, float* ms_each);
/* Sampler::sample (sampler.cpp:113-137) on the device, bit for bit: temperature == 0 is the argmax (the state untouched); otherwise logits / temperature, the
 * clipped softmax (tf_operators.cpp:188-209), one xorshift* coin per token, then multinomial (topp <= 0 or >= 1) or top-p.  *rng_state in: the sampler's
 * xorshift state, out: the state after the call's draws (the reference CLI's seed 0 keeps it 0).  The parameters live in a device block written at the start
 * of each call: changing them re-captures no graph and allocates nothing.  A call that retries behind a timed-out cross-workgroup wait restarts from the
 * caller's state.  FLM_ERR_UNSUPPORTED where the vocabulary does not fit one workgroup's LDS (above ~36 K entries): sample on the host there. */
int  flm_forward_sample(flm_ctx* ctx, const int32_t* tokens, int n, int pos, float temperature, float topp, uint64_t* rng_state, int32_t* next_token);
/* the device-resident loop of flm_decode_greedy with the argmax replaced by the sampler: out_tokens[n_steps], one draw per token; no stop on token 0
 * (flm_generate stops on the device) */
int  flm_decode_sample(flm_ctx* ctx, int32_t first_token, int pos, int n_steps, float temperature, float topp, uint64_t* rng_state, int32_t* out_tokens);
/* ParallelTransformer::generate (transformer.cpp:76-103) as one call: forward, sample, call back per token, stop on a token -- the whole loop on the device's stream.
 * The prompt enters at `pos` exactly as in flm_forward* (more than 5 tokens: the batched path).  Token `index` 0 is drawn from the prompt's last logits, every further one from
 * the previous token fed at the next position: the argmax when temperature == 0 (rng_state may be NULL then), otherwise the device sampler with flm_decode_sample's state contract.
 * The loop ends after max_tokens tokens, at the first token equal to stop_token (-1: none; the reference's loop: 0), or one or more tokens behind a callback's non-zero return
 * (cancel: how far the device runs ahead of the callback is not bounded here).  The stop token is delivered and counted, with last = 1; it is NOT fed: it gets no K/V row and
 * draws nothing further.  *n_out = tokens delivered, out_tokens[0 .. *n_out) = their ids, *rng_state = the state after exactly *n_out draws; afterwards the KV cache holds
 * pos + n_prompt + *n_out - 1 rows and the caller may continue from there with any entry point.  cb (may be NULL) is called on the calling thread, in index order, as the tokens
 * appear -- while the device is still computing the next ones --, `last` set on the final token only; after it has returned non-zero it is not called again (the tokens the device
 * had drawn by then are still counted in *n_out and written to out_tokens).
 * How: every token's last act on the device (the argmax / sampler thread that advances the decode state) publishes {token | last << 31, call tag} as ONE aligned 8-byte store into
 * a ring in page-locked host-coherent memory and sets a latch when the token is the stop token or the host's cancel word is set; every launch of a token looks at the latch first
 * and returns if it is set, so the launches still queued behind a stop touch nothing.  The prompt and all max_tokens - 1 decode tokens are enqueued at once (the token graphs of
 * flm_decode_*: nothing new is captured) with no host synchronisation between them; the host polls the ring, then synchronises and delivers whatever it has not seen yet.
 * Nothing is allocated in the call (the ring, max_seq_len entries, and the cancel word exist since flm_ctx_create).  A call that retries behind a timed-out cross-workgroup wait
 * restarts from the caller's state, produces the same ids, and does not deliver again what the first attempt delivered (a cancel raised in the first attempt takes effect in the
 * re-run only behind the tokens the callback has already received: *n_out never falls below them).
 * FLM_ERR_INVALID if pos + n_prompt + max_tokens - 1 > max_seq_len (nothing is launched); FLM_ERR_UNSUPPORTED for temperature > 0 where flm_decode_sample refuses, and for
 * world > 1 (before anything is launched: halting and cancelling across ranks is not built). */
typedef int (*flm_token_cb)(void* user, int index, int32_t token, int last);   /* non-zero return: cancel */
int  flm_generate(flm_ctx* ctx, const int32_t* prompt, int n_prompt, int pos, int max_tokens,
                  float temperature, float topp, uint64_t* rng_state /* NULL allowed iff temperature == 0 */,
                  int32_t stop_token /* -1: none; the reference's loop: 0 */,
                  flm_token_cb cb /* may be NULL */, void* user,
                  int32_t* out_tokens /* [max_tokens], may be NULL */, int* n_out);
/* Score a sequence in ONE batched pass: per position the greedy id and the probability the model gives a target token -- what perplexity and draft-and-verify schemes need,
 * without one flm_forward call and 4 * vocab bytes of logits per token.  Row i describes the logits after feeding tokens[0..i] at positions pos .. pos + i: exactly the logits
 * flm_forward(tokens, i + 1, pos) returns, bit for bit (logits_all[i][vocab] receives them when it is not NULL).
 *   argmax                 sample_argmax (sampler.cpp:36-47): the first maximum wins
 *   max_logit, sum, prob   the reference sampler's softmax (tf_operators.cpp:188-209) at temperature 1 on that row, read at the row's target: d = x - max; e = d < -15 ? 0 : expf(d);
 *                          sum = the sequential fp32 chain of the e in index order; prob = e_target * (float)(1.0 / sum)
 *   target_logit           the target's raw fp32 logit
 * so that the UNCLIPPED log-probability is (target_logit - max_logit) - log(sum), evaluated by the caller in double from bit-exact ingredients (a clipped target has prob 0 and
 * a finite loss).  targets[n]: the index read in row i, -1 = none; NULL: tokens[i + 1], none for the last row.  A row without a target has target_logit = prob = 0.
 * Afterwards the KV cache holds rows pos .. pos + n - 1 and the decode state is what flm_forward with the same arguments leaves: the caller may continue from pos + n with any
 * entry point, or rewind by passing a smaller pos.
 * How: the first n - 1 tokens run through the batched prompt kernels with the last layer completed, their final rows through the output norm and the classifier on the GEMM tiles
 * in chunks of as many rows as the staging holds (the prefill scores' memory, free by then; without it one row at a time through the logits vector; option "score_rows" caps the
 * chunk), one 1024-thread workgroup per row reduces a chunk's logits to its flm_score; the last token runs through the decode kernels as in flm_forward.  n < 5 (and
 * "use_prefill" 0): token by token, each with its classifier.  Nothing is allocated in the call (the classifier's group-major scales, the targets and the results' device
 * memory exist since flm_ctx_create); the n structs come back in one trip through the bounce buffer, logits_all row by row.
 * Errors, with nothing launched: FLM_ERR_INVALID for n < 1, pos + n > max_seq_len, a token or a target outside [0, vocab) other than a target of -1, out == NULL;
 * FLM_ERR_UNSUPPORTED for world > 1 and where the vocabulary does not fit the statistics kernel's LDS strip (flm_forward_sample's bound, ~36 K entries); FLM_ERR_STATE before the
 * model is complete.  Not built: tensor-parallel scoring, temperatures other than 1. */
typedef struct flm_score { int32_t argmax; float target_logit, max_logit, sum, prob; } flm_score;
int  flm_score_tokens(flm_ctx* ctx, const int32_t* tokens, int n, int pos,
                      const int32_t* targets /* [n], NULL: tokens[i + 1], none for the last */,
                      flm_score* out /* [n] */, float* logits_all /* [n][vocab], may be NULL */);
/* Greedy draft-and-verify: several ids per pass over the weights, the ids of flm_decode_greedy element for element.
 * flm_verify_greedy is the primitive, for callers with a drafter of their own: first_token and drafts[0 .. k) run as ONE batch of k + 1 rows at positions pos .. pos + k through
 * the batched prompt kernels (every row, the last layer and the classifier included: no token goes through the decode kernels); a[i] = the first maximum of row i's logits
 * (sample_argmax); on the device m = the first i with a[i] != drafts[i] (k if there is none).  *n_out = m + 1 and out_tokens[0 .. m] = a[0 .. m]: exactly what the decode loop
 * started with first_token at pos returns for m + 1 steps -- a batched row's logits are flm_forward's bit for bit and the argmax is pinned, so this is equality, not a tolerance.
 * Afterwards the K/V rows pos .. pos + m are valid and are the token path's bits; the rows behind them are stale (every entry point writes a row before it reads it); the caller
 * continues at pos + m + 1 with token out_tokens[m], through any entry point.  4 <= k <= 15 (batches of 5 .. 16 rows).  Errors, with nothing launched: FLM_ERR_INVALID for k
 * outside 4 .. 15, pos + k + 1 > max_seq_len, ids outside [0, vocab); FLM_ERR_UNSUPPORTED for world > 1; FLM_ERR_STATE before the model is complete.  No vocabulary bound (an
 * argmax needs no LDS strip).  Nothing is allocated in the call; the m + 1 ids come back in one trip.
 * The weight pass: option "spec_gemm" 1 = int8 models run every GEMM of the batch through the skinny kernel (v_mfma_i32_16x16x64_i8, 16 tokens x 16 rows x one quant group per
 * instruction, weights from global memory straight into the operand registers, one wave per 16 or 32 rows so that every matrix of the 7B shape fills 256 CUs); 0 = the 64 x 64
 * tiles of the prompt path.  int16 models always run the hi / lo-plane tiles here: correct, not fast. */
int  flm_verify_greedy(flm_ctx* ctx, int32_t first_token, const int32_t* drafts, int k, int pos,
                       int32_t* out_tokens /* [k + 1] */, int* n_out);
/* The loop on top of it, with a built-in prompt-lookup drafter: flm_generate's contract at temperature 0 for *n_out, out_tokens and cb (the stop token is delivered and counted
 * with last = 1 and not fed; the loop ends after max_tokens or behind a callback's non-zero return; cb runs on the calling thread in index order, for all accepted ids of a step).
 * The prompt enters exactly as in flm_forward_argmax.  A step = draft -> a batch of draft_len + 1 rows -> row argmax -> accept, all on the device:
 *   drafter   over the call's history h[0 .. n) (the prompt and every accepted id, in device memory): for g = min(ngram_max, n - 1) down to 1 the LARGEST j with j + g <= n - 1 and
 *             h[j .. j + g) == h[n - g .. n); the first g with a match wins, period p = n - g - j; d[i] = h[n - p + i] for i < p, else d[i - p]; no match: d[i] = h[n - 1].
 *             The choice is a maximum over the matching positions, independent of the order in which waves finish
 *   accept    the verified run is cut behind the first stop token and at max_tokens, appended to the history, and left with m where the host reads both in one trip
 * The batched kernels take the position as a launch argument, so the host learns m before it enqueues the next step: ONE host synchronisation per step (a device-resident or
 * graph-captured loop is not built).  Where pos + draft_len + 1 would pass max_seq_len, or fewer than 2 ids are still wanted, the step is an ordinary one-launch greedy token; the
 * ids are the same.  FLM_ERR_INVALID if pos + n_prompt + max_tokens - 1 > max_seq_len, draft_len outside 4 .. 15 or ngram_max outside 1 .. 8; FLM_ERR_UNSUPPORTED for world > 1.
 * Temperature > 0: flm_generate_lookup_sample below.  flm_query: "spec_steps" / "spec_accepted" = the last call's verify passes / drafted ids accepted in them. */
int  flm_generate_lookup(flm_ctx* ctx, const int32_t* prompt, int n_prompt, int pos, int max_tokens,
                         int32_t stop_token /* -1: none */, int draft_len /* 4..15 */, int ngram_max /* 1..8 */,
                         flm_token_cb cb /* may be NULL */, void* user,
                         int32_t* out_tokens /* [max_tokens], may be NULL */, int* n_out);
/* Sampled draft-and-verify: the ids of flm_decode_sample element for element, several per pass over the weights.  The sampler is a function of a row's logits and one coin, and
 * token i of a sampled decode loop is drawn with the i-th coin of its xorshift state; so row i of a verify batch is drawn with the (i + 1)-th coin of the step's state
 * (k_sample_rows: one 1024-thread workgroup per row, every row the draw flm_forward_sample makes -- the IEEE division by the temperature, the clipped expf, the sequential sum
 * chain, multinomial or top-p behind the stable radix sort; the two kernels share that code), and the batch is cut at the first draw that differs from its draft.  This is
 * equality, not rejection sampling: no id is re-drawn and no tolerance is involved; a call consumes exactly as many coins as it returns ids.
 * flm_verify_sample is flm_verify_greedy's contract with the row argmax replaced by the row draw: s[i] = row i drawn with the (i + 1)-th coin of *rng_state, m = the first i with
 * s[i] != drafts[i] (k if none), out_tokens[0 .. m] = s[0 .. m], *n_out = m + 1, *rng_state = the state after m + 1 draws -- what flm_decode_sample(first_token, pos, m + 1,
 * temperature, topp, the same state) returns and leaves; the K/V rows pos .. pos + m are the token path's bits.  temperature == 0: flm_verify_greedy's result, the state
 * untouched (rng_state may be NULL; no vocabulary bound).  Errors as in flm_verify_greedy, and FLM_ERR_INVALID for a NULL rng_state at temperature != 0, a negative or NaN
 * temperature, a NaN top-p; FLM_ERR_UNSUPPORTED at temperature != 0 where flm_decode_sample refuses (the vocabulary bound).  Nothing is launched on any error; nothing is
 * allocated in the call (the rows sort in slices of a [16][2][vocab] buffer that exists since flm_ctx_create); the ids and the state come back in one trip. */
int  flm_verify_sample(flm_ctx* ctx, int32_t first_token, const int32_t* drafts, int k, int pos,
                       float temperature, float topp, uint64_t* rng_state /* NULL allowed iff temperature == 0 */,
                       int32_t* out_tokens /* [k + 1] */, int* n_out);
/* flm_generate's contract at ANY temperature through draft-and-verify steps with flm_generate_lookup's drafter: the same ids, *n_out, callbacks and final state as flm_generate
 * with the same arguments (a callback's cancel ends the call behind the step that delivered it; *rng_state is then the state after *n_out draws all the same).  Token 0 is drawn
 * from the prompt's last logits with the first coin, as flm_forward_sample does it; every step is draft -> the batch -> the rows' draws -> accept, and the accept step leaves, next
 * to m and the ids, the state after exactly as many draws as ids it delivers (a run cut by the stop token or max_tokens counts only the ids in front of the cut).  The step's
 * state is a launch argument from the host, so a step that is re-run (the retry path) draws the same coins and delivers nothing twice.  Where fewer than 2 ids are still wanted,
 * or the batch would pass max_seq_len, the step is one ordinary sampled token.  *rng_state on return: the state after *n_out draws (untouched at temperature 0, where the call is
 * flm_generate_lookup).  Errors as in flm_generate_lookup and flm_generate; one GPU only.  "spec_steps" / "spec_accepted" as there; the ids count in "sampled_tokens". */
int  flm_generate_lookup_sample(flm_ctx* ctx, const int32_t* prompt, int n_prompt, int pos, int max_tokens,
                                float temperature, float topp, uint64_t* rng_state /* NULL allowed iff temperature == 0 */,
                                int32_t stop_token /* -1: none */, int draft_len /* 4..15 */, int ngram_max /* 1..8 */,
                                flm_token_cb cb /* may be NULL */, void* user,
                                int32_t* out_tokens /* [max_tokens], may be NULL */, int* n_out);
/* Sampling controls on the device: top-k, min-p, repetition / frequency / presence penalties over a window of recent ids, and a logit bias (-inf: a ban).  No reference
 * counterpart (the reference samples with temperature and top-p only).  A shaping stage (k_shape_logits, csrc/flm_shape.h: one 1024-thread workgroup, no vocabulary bound) runs
 * between the classifier and the sampler above, which is not changed and reads the shaped row S instead of the raw row L.  The definition, all of it fp32 round-to-nearest:
 *   1 bias       S = L; S[id] = S[id] + b for each of the n_bias pairs (ids distinct; b finite or -inf)
 *   2 penalties  window W[0 .. w), w > 0: for every DISTINCT id t of W with c occurrences (each id once): x = S[t]; repeat_penalty != 1: x = x > 0 ? x / repeat_penalty
 *                : x * repeat_penalty; frequency_penalty or presence_penalty != 0: x = x - ((float)c * frequency_penalty + presence_penalty); S[t] = x
 *   3 top-k      0 < top_k < n: the top_k entries first in "larger value, equal values by lower index" (float comparison: -0.0 ties +0.0) stay, all others become -inf
 *   4 min-p      min_p > 0 and temperature != 0: y[i] = S[i] / temperature over the entries that are not -inf, mx = max y; S[i] = -inf where y[i] - mx < logf(min_p) (the
 *                logarithm is taken once on the host, glibc's): the entries whose probability is below min_p times the largest one
 *   5 the sampler  on S with (temperature, topp), unchanged -- its top-p cutoff keeps using the full n; temperature 0: the first maximum of S
 * A stage whose control is neutral (n_bias 0; repeat_penalty 1; frequency_penalty = presence_penalty = 0, or an empty window; top_k 0 or >= n; min_p 0) writes nothing: with
 * every control neutral S is L bit for bit and the _ex entry points run the launches of their plain forms.  The host restatement is host/sampler.cpp shape_logits; the device
 * equals it bit for bit, so ids under controls are a host loop's ids (flm_forward, shape_logits, Sampler::sample) element for element.  NaN logits are outside the contract.
 * The controls live in a device block written at the start of each call (like the sampler's parameters): no graph is re-captured, nothing is allocated.
 * Spec decoding takes the controls through flm_verify_sample_ex / flm_generate_lookup_ex below: every row of a verify batch is shaped over a window of its own. */
#define FLM_PENALTY_WINDOW_MAX 1024
#define FLM_BIAS_MAX 256
typedef struct flm_sampling {
    float temperature, topp;          /* as flm_generate */
    int32_t top_k;                    /* 0: off */
    float min_p;                      /* 0: off */
    float repeat_penalty;             /* 1: off */
    float frequency_penalty, presence_penalty;   /* 0: off */
    int32_t penalty_last_n;           /* 0 .. FLM_PENALTY_WINDOW_MAX; 0: penalties off */
    int32_t n_bias;                   /* 0 .. FLM_BIAS_MAX */
    const int32_t* bias_ids; const float* bias_values;
} flm_sampling;
/* flm_generate with the controls: its contract in every other respect (the stop token, cancel, streaming, *n_out, *rng_state after exactly *n_out draws, the KV rows,
 * FLM_ERR_UNSUPPORTED for world > 1; a retried call re-runs from the caller's state and delivers nothing twice).  The penalty window at generated token s is the last
 * min(penalty_last_n, n_prompt + s) ids of THIS call's prompt followed by the ids this call has drawn so far, assembled on the device; ids that were in the KV cache before the
 * call (pos > 0) are not part of it.  A token is classifier -> k_shape_logits -> the sampler, replayed as a graph built at flm_prepare next to the sampled one; at temperature 0
 * with a control set the same form runs (the sampler's own first-maximum branch), not the one-launch greedy token.  Vocabulary: the shaper has no bound; at temperature != 0 the
 * sampler's FLM_ERR_UNSUPPORTED above ~36 K entries stays; at temperature 0 there is none.  rng_state may be NULL iff temperature == 0.
 * FLM_ERR_INVALID, with nothing launched: a NULL struct, top_k < 0, min_p outside [0, 1) or NaN, repeat_penalty <= 0 or NaN, a NaN frequency or presence penalty,
 * penalty_last_n / n_window / n_bias out of range, a bias id outside [0, vocab) or listed twice, a bias that is NaN or +inf, a window id outside [0, vocab). */
int  flm_generate_ex(flm_ctx* ctx, const int32_t* prompt, int n_prompt, int pos, int max_tokens, const flm_sampling* sampling,
                     uint64_t* rng_state, int32_t stop_token, flm_token_cb cb, void* user, int32_t* out_tokens, int* n_out);
/* flm_forward_sample with the controls, for callers with a loop of their own: the window is the caller's, window[0 .. n_window), 0 <= n_window <= FLM_PENALTY_WINDOW_MAX, used
 * as given (penalty_last_n is only range-checked here; n_window == 0: penalties off).  One GPU only when a control is set. */
int  flm_forward_sample_ex(flm_ctx* ctx, const int32_t* tokens, int n, int pos, const flm_sampling* sampling,
                           const int32_t* window, int n_window, uint64_t* rng_state, int32_t* next_token);
/* Draft-and-verify under the controls.  In a flm_generate_ex loop the window of generated token s is the last min(penalty_last_n, n_prompt + s) ids of prompt ++ drawn[0 .. s).
 * Row r of a verify batch fed with {last id, d[0 .. k)} matters only if d[0 .. r) were the ids drawn for rows 0 .. r - 1 -- exactly when the accept step keeps row r -- and then
 * the loop's window for that token is the last min(penalty_last_n, n_hist + r) ids of hist[0 .. n_hist) ++ d[0 .. r): both parts are in device memory before the batch runs.
 * The shaped row is a function of (raw row, window, controls) and the draw a function of (shaped row, coin r + 1), so shaping row r with that window (k_shape_rows,
 * csrc/flm_shape.h: one 1024-thread workgroup per row, the definition above through the same device function as k_shape_logits, in place in the classifier's staging, no
 * vocabulary bound) and drawing it with the verify pass's row sampler (the row argmax at temperature 0) gives the id the shaped token loop draws.  Rows behind the first
 * mismatch used windows the loop never sees; they are discarded anyway.  Equality, not rejection sampling.
 * flm_verify_sample_ex: flm_verify_sample's contract with row r shaped over the last min(penalty_last_n, n_window + r) ids of window ++ drafts[0 .. r); n_window <=
 * penalty_last_n is required (row 0 then uses the window exactly as given; penalty_last_n == 0: penalties off).  The ids, *n_out, the state and the K/V rows pos .. pos + m are
 * those of *n_out successive flm_forward_sample_ex calls by a caller who keeps that sliding window.
 * flm_generate_lookup_ex: flm_generate_ex's contract (ids, *n_out, callbacks, stop, cancel as in flm_generate_lookup_sample, the final state, the K/V rows) through
 * draft-and-verify steps: token 0 is the shaped token behind the prompt, a batch step's base window is the call's history, a single-token step (fewer than 2 ids wanted, or
 * the batch would pass max_seq_len) is the shaped token with its window written from the ids the host holds.
 * Both: every control neutral = the launches of flm_verify_sample / flm_generate_lookup_sample (no shape kernel); FLM_ERR_INVALID as in flm_generate_ex /
 * flm_forward_sample_ex and in the plain forms (nothing launched); FLM_ERR_UNSUPPORTED for world > 1 and, at temperature != 0, above the sampler's vocabulary bound (none at
 * temperature 0); nothing is allocated in a call; a re-run step delivers nothing twice.  The ids delivered with a control set count in "shaped_tokens". */
int  flm_verify_sample_ex(flm_ctx* ctx, int32_t first_token, const int32_t* drafts, int k, int pos,
                          const flm_sampling* sampling, const int32_t* window, int n_window,
                          uint64_t* rng_state /* NULL allowed iff temperature == 0 */, int32_t* out_tokens /* [k + 1] */, int* n_out);
int  flm_generate_lookup_ex(flm_ctx* ctx, const int32_t* prompt, int n_prompt, int pos, int max_tokens,
                            const flm_sampling* sampling, uint64_t* rng_state /* NULL allowed iff temperature == 0 */,
                            int32_t stop_token /* -1: none */, int draft_len /* 4..15 */, int ngram_max /* 1..8 */,
                            flm_token_cb cb /* may be NULL */, void* user,
                            int32_t* out_tokens /* [max_tokens], may be NULL */, int* n_out);
/* Draft-and-verify with a small DRAFT MODEL of the same vocabulary as the drafter, instead of the prompt lookup: the drafter every engine pairs a big model with, and the
 * one that pays on text that does not repeat its history.  The verify contract is equality with the plain loop, not rejection sampling, so the ids cannot depend on the
 * drafter: a bad draft model costs acceptance, never an id.
 * flm_draft_set pairs a target context with a draft context (NULL: detach).  FLM_ERR_INVALID when draft == ctx or the vocabulary sizes differ; FLM_ERR_UNSUPPORTED when
 * either context has world > 1 or the two sit on different devices; FLM_ERR_STATE before both models are complete.  Everything the pairing needs is created here (the two
 * events that order the two contexts' streams; the hand-off reads the draft's ids where its decode loop leaves them and brings its error word along in the target's own
 * page-locked line), so the generate call below allocates nothing; no graph of either context is re-captured by attaching, re-attaching or detaching.  The target does NOT
 * own the draft: the caller detaches before destroying either context.  Every other entry point of both contexts behaves as it does unpaired; the caller must not run
 * calls on the draft context from another thread while the generate call below runs on the target.
 * flm_generate_draft is flm_generate_lookup_ex's signature without ngram_max, and its contract: ids, *n_out, *rng_state, the callback sequence, the target's K/V rows,
 * "constraint_state", the log-probability records and "stop_reason" / "stop_rule" equal flm_generate_ex's with the same arguments, element for element.  sampling may be NULL
 * (every control neutral at temperature 0) or neutral: the plain forms; temperature 0 needs no rng_state.  4 <= draft_len <= 15.  FLM_ERR_STATE when no draft is attached; argument
 * errors as in flm_generate_lookup_ex, and FLM_ERR_INVALID when pos + n_prompt + max_tokens - 1 passes the DRAFT's max_seq_len; nothing is launched on an error.
 *   token 0   the target's prompt feed as there; the draft feeds the same prompt at the same pos, its own draw discarded
 *   a step    the draft context runs its device-resident token loop for draft_len tokens from {the last id, its position}: greedy at temperature 0, else its plain sampled
 *             form with the step's base state and the call's temperature / top-p -- draft i is drawn with the (i + 1)-th coin, the coin the verify batch uses for row i
 *             (common random numbers: where the two models agree on a row they draw the same id).  The controls, the constraint, the stop rules and the log-probabilities act
 *             on the target's rows only; the draft drafts from its raw logits.  k_spec_take_drafts (csrc/flm_spec.h), on the target's stream behind the draft's event, makes
 *             the draft's ids the batch (an id outside [0, vocab) is replaced by the last id); everything behind it is the lookup loop's.  No draft id travels to the host:
 *             a step still has ONE host synchronisation.  The two contexts' launches never overlap on the device (the one-launch token waits on co-resident workgroups).
 *   catch-up  after a step that accepted every draft the draft context lacks one row (the last draft was never fed): it feeds that token at the head of its next step.
 *             Single-token steps (fewer than 2 ids wanted, or the batch would pass either max_seq_len) run on the target alone; the draft feeds what it lacks once, before
 *             the call returns.
 *   re-run    a step's inputs stay host-held (the history's length, the room, the state, the draft's row count): a timed-out wait in EITHER context re-runs the whole step,
 *             nothing is delivered twice; each context falls back and recovers by its own policy.
 * Precondition: both caches hold rows for the same pos tokens.  Postcondition: both hold pos + n_prompt + *n_out - 1 rows of the same sequence (the draft is caught up before
 * the call returns), so a following call at that position, on either entry point, is valid.  Beyond that the draft's decode state and sampler block are unspecified.
 * flm_query: "spec_steps" / "spec_accepted" as for the lookup loop, "draft_tokens" = tokens the draft context computed in the last call. */
int  flm_draft_set(flm_ctx* ctx, flm_ctx* draft /* NULL: detach */);
int  flm_generate_draft(flm_ctx* ctx, const int32_t* prompt, int n_prompt, int pos, int max_tokens,
                        const flm_sampling* sampling /* may be NULL */, uint64_t* rng_state /* NULL allowed iff temperature == 0 */,
                        int32_t stop_token /* -1: none */, int draft_len /* 4..15 */,
                        flm_token_cb cb /* may be NULL */, void* user,
                        int32_t* out_tokens /* [max_tokens], may be NULL */, int* n_out);
/* Parallel sampling: n completions of ONE prompt, all n drawn per pass over the weights -- what the API parameter n / best_of, self-consistency voting and reranking ask
 * for, without n sequential flm_generate calls.  One context, one cache, one shared prompt; no reference counterpart (the reference generates one sequence).
 * Contract, for every j < n: out_tokens[j * max_tokens + 0 .. n_out[j]), n_out[j] and rng_states[j] afterwards are exactly what
 *     flm_generate(ctx, prompt, n_prompt, pos, max_tokens, temperature, topp, &rng_states[j], stop_token, ...)
 * delivers on a context whose cache holds the same pos rows: the ids element for element, the states as 64-bit integers.  The stop token is delivered, counted and not fed;
 * a finished sequence's state stays at the state after its last delivered draw; the others go on.  temperature == 0 is allowed: every row is the greedy run, rng_states may be
 * NULL and no state is touched.  Like plain flm_generate the call IGNORES installed stop rules, the constraint, armed log-probabilities and flm_entropy_set.
 *   layout    S = pos + n_prompt cache rows are shared by all sequences.  Sequence j's fed tokens (at most max_tokens - 1 of them) live in the physical rows base[j] + i,
 *             base[j] = S + j * (max_tokens - 1); token i of a tail is at LOGICAL position S + i -- for RoPE and for the attention's order -- whatever its physical row.  The
 *             call needs S + n * (max_tokens - 1) <= max_seq_len and no cache memory of its own.  flm_fan_layout_for computes and checks this without a device (pure host
 *             arithmetic, like flm_plan_shards); the entry point uses the same function.
 *   a step    the prompt enters as in flm_generate (flm_forward's rows); token 0 of every sequence is drawn from the one row of logits it leaves, each with its own first
 *             coin.  Then one step per token: the n last ids run as ONE batch of n rows through the batched kernels (the verify pass's: every row's logits are flm_forward's
 *             bits), the attention of row j over the shared rows followed by tail j in the logical order (k_attn_fan, csrc/flm_fan.h: a workgroup brings a shared K / V tile to
 *             LDS once for up to 8 rows), row j drawn by the unchanged sampler with state j.  ONE host synchronisation per step (the result block: ids, live mask, states);
 *             finished sequences stay in the batch, their outputs dropped.  A step's inputs are launch arguments from what the host holds, so a step that retries behind a
 *             timed-out cross-workgroup wait (the prompt's token launches can have one) enqueues the same work.
 *   cb        the flm_fan_cb receives (user, seq, index, token, last): called on the calling thread, per step in sequence order; `last` on a sequence's final token.  A non-zero return
 *             cancels the WHOLE call: the callback is not called again, the ids of the step in flight are still counted (n_out covers what was delivered).
 *   after     rows [0, S) are untouched: the prompt's rows bit-equal what flm_forward leaves; rows behind S are unspecified.  flm_fan_keep(ctx, j), valid until the next call
 *             that writes the cache (and once), moves tail j to rows [S, S + n_out[j] - 1) with one copy kernel over all layers and heads (source and destination cannot
 *             overlap for j > 0; j = 0 is in place): the cache is then bit for bit what sequence j's own flm_generate would have left, and any entry point continues from
 *             pos + n_prompt + n_out[j] - 1.
 * Errors, with nothing launched and the cache untouched: FLM_ERR_INVALID for n outside 2 .. FLM_FAN_MAX, S + n * (max_tokens - 1) > max_seq_len, max_tokens < 1, a NULL prompt /
 * out_tokens / n_out, a NULL rng_states at temperature != 0, ids outside [0, vocab), stop_token >= vocab; for flm_fan_keep without a preceding flm_generate_n or with seq outside
 * [0, n).  FLM_ERR_UNSUPPORTED for world > 1, for temperature > 0 where flm_decode_sample refuses (the vocabulary bound), and for head sizes above 128 (the multi-query attention's
 * bound).  flm_query "stop_reason" describes the WHOLE call: cancel; else length where any sequence ran to max_tokens; else the stop token ("stop_rule" 0).
 * Nothing is allocated in the call: the drawn ids, the states and the result block (a few hundred bytes) exist since flm_ctx_create. */
#define FLM_FAN_MAX 16
typedef struct flm_fan_layout { int32_t shared_rows, tail_rows, n; int32_t base[FLM_FAN_MAX]; } flm_fan_layout;
int  flm_fan_layout_for(int pos, int n_prompt, int max_tokens, int n, int max_seq_len, flm_fan_layout* out);
typedef int (*flm_fan_cb)(void* user, int seq, int index, int32_t token, int last);   /* non-zero return: cancel the whole call */
int  flm_generate_n(flm_ctx* ctx, const int32_t* prompt, int n_prompt, int pos, int max_tokens, int n,
                    float temperature, float topp, uint64_t* rng_states /* [n]; NULL allowed iff temperature == 0 */,
                    int32_t stop_token /* -1: none */, flm_fan_cb cb /* may be NULL */, void* user,
                    int32_t* out_tokens /* [n][max_tokens] */, int* n_out /* [n] */);
int  flm_fan_keep(flm_ctx* ctx, int seq);
/* Cache slots: up to FLM_BATCH_MAX INDEPENDENT sequences -- each its own prompt, length, sampler parameters and state -- served per pass over the weights, at step
 * granularity, so that a sequence can join while others are in flight (continuous batching).  One context, one cache; no reference counterpart.
 * Contract, for every request, in any slot, whatever else shares the pass, joins or finishes around it: the ids delivered from flm_batch_join through the flm_batch_steps,
 * their count and the final sampler state are exactly what
 *     flm_generate(ctx, prompt, n_prompt, 0, max_tokens, temperature, topp, &rng_state, stop_token, ...)
 * delivers on a fresh context, the ids element for element, the state as a 64-bit integer; and the slot's rows [base, base + n_prompt + n_out - 1) of every layer's K and V
 * are that context's rows [0, ...), bit for bit.  The stop token is delivered, counted and not fed.  temperature == 0 is the greedy run: the state passes through.  Like plain
 * flm_generate these calls IGNORE installed sampling controls, stop rules, the constraint, armed log-probabilities and flm_entropy_set (per-slot forms of them are follow-ups).
 *   layout    no cache memory of its own: the context's rows [0, max_seq_len) are divided into n_slots regions, slot s owning the physical rows [base[s], base[s] + rows[s]),
 *             base the prefix sum of rows.  A sequence in slot s keeps LOGICAL position p -- for RoPE and for the attention's order -- in physical row base[s] + p.
 *             flm_batch_layout_for computes and checks this without a device (pure host arithmetic, like flm_fan_layout_for) and is the one place the capacity condition
 *             sum(rows) <= max_seq_len is written: FLM_ERR_INVALID for n_slots outside 1 .. FLM_BATCH_MAX, a rows[s] < 1, or a layout that does not fit.
 *   open      records the layout (it must be what flm_batch_layout_for gives for this context's max_seq_len) and empties all slots.  Launches nothing, allocates nothing.  Any
 *             other entry point that writes the cache ends the batch: join, step, state and close(keep) then answer FLM_ERR_STATE.
 *   join      needs an empty slot (a slot whose sequence finished is empty again; its flm_batch_state stays readable until the next join into it), n_prompt >= 1,
 *             max_tokens >= 1, n_prompt + max_tokens - 1 <= rows[slot], and flm_generate_n's checks on ids, temperature, top-p, stop token and the sampler's vocabulary bound.
 *             The prompt enters at logical positions [0, n_prompt) of the slot as ONE batch through the batched kernels with the last layer completed (a verify pass's route:
 *             every row's logits are flm_forward's bits; no token launch, the decode state and the captured graphs untouched); token 0 is drawn from its last row with the
 *             request's first coin and returned in *first_token.  *live = 0 if token 0 was the stop token or max_tokens == 1.  Other slots' rows and state are untouched.
 *   step      ONE pass over the weights for all live slots: each feeds its last id at its own position (k_rope_kv_slots, k_attn_slots -- csrc/flm_batch.h: workgroup
 *             (head, row) narrows the cache to the row's slot and runs the one-query attention), one id is drawn per slot with its own state, temperature and top-p.  A
 *             finished or empty slot is not in the batch and costs nothing.  A slot leaves the live set when it draws its stop token or has delivered max_tokens ids.  ONE
 *             host synchronisation (the result block); a step's inputs are launch arguments, so a step that retries enqueues the same work.  No live slot: FLM_OK, live = 0,
 *             nothing launched.
 *   state     the sampler state behind exactly the delivered ids, their count, and FLM_STOP_TOKEN / FLM_STOP_LENGTH (0 while the slot runs).
 *   close     ends the batch.  keep_slot >= 0: that slot's rows move to [0, len), len = n_prompt + n_out - 1, and any entry point continues the conversation from pos = len, as
 *             after flm_fan_keep (where source and destination overlap, base < len, the move runs as successive copies of at most base rows, ascending).
 *   flm_generate_batch  the loop on top: rows[j] = n_prompt[j] + max_tokens[j] - 1, open, join every request in order, step until nobody is live, close(-1).  Request j's
 *             ids go to out_tokens[j * stride ..) (stride >= every max_tokens), n_out[j], rng_out[j].  cb(user, seq, index, token, last) runs on the calling thread in
 *             (step, slot) order; a non-zero return ends the call behind that step ("stop_reason": cancel; else length where any sequence ran to max_tokens; else token).
 * Errors, with nothing launched and the cache untouched: FLM_ERR_INVALID for the checks above, a slot outside the layout, a join into a live slot; FLM_ERR_STATE without an open
 * batch; FLM_ERR_UNSUPPORTED for world > 1, for head sizes whose one-query attention does not fit the LDS, and for temperature > 0 where flm_decode_sample refuses.
 * Nothing is allocated in any of these calls: the result block exists since flm_ctx_create.
 *
 * Ragged passes: requests enter INSIDE the steps' pass.  Between empty and running a slot can be FILLING: admitted, its prompt not yet wholly in the cache.
 *   admit     join's checks (an empty slot -- neither running nor filling --, the lengths against the slot's rows, ids in the vocabulary, the sampler's bounds), then the
 *             request is recorded and the slot is filling.  No launch, no allocation, nothing is copied: req->prompt MUST STAY VALID until the slot has delivered its
 *             token 0 (req itself may go).
 *   pass      ONE pass over the weights for a plan of at most 16 segments {slot, row0, n, pos0, draws}, at most one per slot: first every running slot's one step row
 *             (a step's rows and kernels), then, in ascending slot order, a chunk of every filling slot's prompt -- min(pending, what is left of prompt_rows_max) rows
 *             each, entering at the slot's logical position pos0 = the rows fed so far (csrc/flm_segs.h: k_rope_kv_segs, and k_attn_segs_mq, where eight consecutive
 *             queries of ONE sequence share every K / V tile of that sequence's slot; head sizes above 128 and "use_prefill_mq" 0: one query per workgroup).
 *             prompt_rows_max 0: no bound -- every filling slot's whole remainder.  A slot whose prompt completes draws its token 0 from the chunk's last row in the same
 *             pass, runs from the next pass on, and is finished at once if token 0 is its stop token or max_tokens == 1.  ids[s]: the next id of a running slot, token 0
 *             of a slot whose prompt completed in this pass, -1 otherwise; live: the running slots behind the pass; filling: the slots still filling; finished as in a
 *             step.  Nobody running or filling: FLM_OK, nothing launched.  ONE host synchronisation; what the pass reads is launch arguments and ids uploaded inside the
 *             retried region; the host's copy of a slot moves only behind a verified pass.  "spec_gemm" 1 and at most 16 rows in the pass: the skinny GEMM, as in a step.
 *   flm_batch_plan_for  the scheduling rule above, pure host arithmetic and the one place it is written (flm_batch_pass calls it): fed[s] = the rows slot s has in the
 *             cache (a running slot's position, a filling slot's rows fed so far), pending[s] = the prompt rows a filling slot still lacks (0: not filling), running =
 *             the mask of running slots.  FLM_ERR_INVALID for n_slots outside 1 .. FLM_BATCH_MAX, a negative budget, negative counts, a slot both running and pending.
 *   The contract is the one above, unchanged, whatever the budget is, however a prompt was cut into chunks, and whatever else ran, joined, filled or finished in the same
 *   passes.  The calls mix: step leaves filling slots alone; join or admit into a filling or running slot, and close(keep) of a filling slot, answer FLM_ERR_INVALID;
 *   flm_batch_state of a filling slot answers n_out 0, reason 0; a negative budget answers FLM_ERR_INVALID; FLM_ERR_STATE / FLM_ERR_UNSUPPORTED as for step.
 *   flm_generate_batch under option "batch_rows" b >= 0: every request is admitted, then flm_batch_pass(b) until nobody runs or fills.  The results are the default's;
 *   the callbacks come in (pass, slot) order -- with a bounded budget a slot can deliver its token 1 before a later slot delivers its token 0.
 *   flm_query "batch_passes": the weight passes (joins, steps, passes) since the last flm_batch_open. */
#define FLM_BATCH_MAX 16
typedef struct flm_batch_layout { int32_t n_slots; int32_t base[FLM_BATCH_MAX], rows[FLM_BATCH_MAX]; } flm_batch_layout;
typedef struct flm_batch_req { const int32_t* prompt; int32_t n_prompt, max_tokens; float temperature, topp;
                               uint64_t rng_state; int32_t stop_token /* -1: none */; } flm_batch_req;
typedef struct flm_batch_out { int32_t ids[FLM_BATCH_MAX];      /* -1: the slot delivered nothing in this step */
                               uint32_t live;                   /* slots still running behind this step */
                               uint32_t finished; } flm_batch_out; /* slots whose LAST id is in this step */
int  flm_batch_layout_for(int n_slots, const int32_t* rows, int max_seq_len, flm_batch_layout* out);
int  flm_batch_open(flm_ctx* ctx, const flm_batch_layout* layout);
int  flm_batch_join(flm_ctx* ctx, int slot, const flm_batch_req* req, int32_t* first_token, int* live);
int  flm_batch_step(flm_ctx* ctx, flm_batch_out* out);
int  flm_batch_state(flm_ctx* ctx, int slot, uint64_t* rng_state, int* n_out, int* stop_reason);
int  flm_batch_close(flm_ctx* ctx, int keep_slot /* -1: none */);
typedef struct flm_batch_seg  { int32_t slot, row0 /* first batch row */, n /* rows */, pos0 /* logical position of its first row */, draws /* 1: its last row is drawn from */; } flm_batch_seg;
typedef struct flm_batch_plan { int32_t n_segs, n_rows, n_step, n_draws; flm_batch_seg seg[FLM_BATCH_MAX]; } flm_batch_plan;
typedef struct flm_batch_pass_out { int32_t ids[FLM_BATCH_MAX]; uint32_t live, finished, filling; } flm_batch_pass_out;
int  flm_batch_plan_for(int n_slots, const int32_t* fed, const int32_t* pending, uint32_t running, int prompt_rows_max /* 0: no bound */, flm_batch_plan* out);
int  flm_batch_admit(flm_ctx* ctx, int slot, const flm_batch_req* req);
int  flm_batch_pass(flm_ctx* ctx, int prompt_rows_max /* 0: no bound */, flm_batch_pass_out* out);
int  flm_generate_batch(flm_ctx* ctx, const flm_batch_req* reqs, int n, flm_fan_cb cb /* may be NULL */, void* user,
                        int32_t* out_tokens /* [n][stride] */, int stride, int* n_out /* [n] */, uint64_t* rng_out /* [n], may be NULL */);
/* Constrained decoding: a token-level deterministic automaton masks the logits in front of the controls -- what "one of these strings", a JSON shape or a regular expression
 * reduce to.  No reference counterpart.  The automaton is CSR: the edges of state q are [row_ptr[q], row_ptr[q + 1]).
 *   delta(q, t)  the edge_next of t's edge in state q, or q ITSELF when t has no edge there.  The no-edge case is reachable only through the multinomial branch's last-index
 *                fallback of Sampler::sample (sampler.cpp `return _n - 1`: the coin lies beyond the accumulated probabilities), which can name a masked id.
 *   step 0       with the context armed at state q the shaping definition at flm_sampling gains a step in front of the bias: S = L; S[i] = -inf for every i without an edge
 *                in q.  A masked entry stays -inf under steps 1 - 4 (-inf + b = -inf for every allowed bias), so step 0 followed by those steps is the whole definition; the
 *                host restatement is host/sampler.cpp constrain_logits followed by shape_logits.  Every state has an edge: the mask alone never bans a whole row.
 * flm_dfa_validate (pure host arithmetic, like flm_plan_shards): FLM_OK, or FLM_ERR_INVALID with flm_last_error(NULL) naming the rule -- n_states in [1, FLM_DFA_STATES_MAX] and
 * n_edges in [1, FLM_DFA_EDGES_MAX]; row_ptr[0] = 0, non-decreasing, row_ptr[n_states] = n_edges; tokens strictly ascending inside a state and in [0, vocab); edge_next in
 * [0, n_states); every state has at least one edge.
 * flm_constraint_set installs or replaces the automaton (NULL: removes it): validated against the model's vocabulary, copied to device memory allocated HERE, off the steady
 * path like flm_upload_tensor (the previous automaton's memory is released), with a host copy kept; afterwards the constraint is disarmed.  FLM_ERR_UNSUPPORTED on a sharded
 * context, FLM_ERR_STATE before the model is complete.  No graph is re-captured: the shaped token graphs reach the automaton through a device block that exists since
 * flm_ctx_create and whose contents are rewritten.
 * flm_constraint_arm sets the state (-1: disarms); FLM_ERR_INVALID for a state outside [0, n_states) or with no automaton installed.  Allocates nothing, re-captures nothing.
 * flm_query "constraint_state" reads the state (-1: disarmed).  (Not an option: flm_set_option drops the graphs.)
 * While armed, the four _ex entry points apply it -- flm_generate_ex, flm_forward_sample_ex, flm_verify_sample_ex, flm_generate_lookup_ex -- and an armed constraint counts as
 * a control that is set: with every flm_sampling control neutral the shaped form still runs, masking only, and the delivered ids count in "shaped_tokens".  After a call that
 * delivers ids t[0 .. n) the state is delta folded over them from the state the context was armed at, the stop token included when delivered (the host folds its own copy of
 * the automaton over the ids it delivered: nothing extra is read back).  Row r of a verify batch is masked in delta folded over drafts[0 .. r): the loop's state for that token
 * exactly when the accept step keeps the row.  A retried call restarts from the state it was armed at and delivers nothing twice; on any error nothing is launched and the
 * state does not move.  Every other rule of the _ex forms stays.  The PLAIN entry points (flm_forward*, flm_decode_*, flm_generate, flm_verify_greedy / _sample,
 * flm_generate_lookup / _sample, flm_score_tokens) ignore the constraint and leave its state alone. */
#define FLM_DFA_STATES_MAX 65536
#define FLM_DFA_EDGES_MAX  (1 << 24)
typedef struct flm_dfa {            /* CSR: the edges of state q are [row_ptr[q], row_ptr[q + 1]) */
    int32_t n_states, n_edges;
    const int32_t* row_ptr;         /* [n_states + 1], row_ptr[0] = 0, non-decreasing, row_ptr[n_states] = n_edges */
    const int32_t* edge_token;      /* [n_edges], STRICTLY ascending inside a state, in [0, vocab) */
    const int32_t* edge_next;       /* [n_edges], in [0, n_states) */
} flm_dfa;
int  flm_dfa_validate(const flm_dfa* dfa, int vocab);
int  flm_constraint_set(flm_ctx* ctx, const flm_dfa* dfa);
int  flm_constraint_arm(flm_ctx* ctx, int32_t state);
/* Per-token log-probabilities and top-N alternatives from the device loop: how sure the model was of each id it delivered, and what the alternatives were (OpenAI-style
 * logprobs / top_logprobs, llama.cpp's n_probs).  No reference counterpart.  One small stage (k_logprob_token / k_logprob_rows, csrc/flm_logprob.h: one 1024-thread workgroup
 * per row) runs behind the draw, on the row that is still in device memory.  The record of ONE token drawn from a row R[0 .. n) with drawn id t, top_n in 0 .. FLM_LOGPROBS_MAX:
 *   token, logit     t and R[t].  R[t] may be -inf: the multinomial branch's last-index fallback can name a masked id (see delta at flm_dfa)
 *   max_logit, sum   exactly flm_score's fields on R at temperature 1: max_logit = the first maximum's value; e_i = (R[i] - max) < -15 ? 0 : expf(R[i] - max); sum = the
 *                    sequential fp32 chain of the e_i in index order
 *   n_top, top_id, top_logit   n_top = min(top_n, n); top_id[0 .. n_top) = the first n_top indices in the order "larger value, equal values by lower index, -0.0 ties +0.0"
 *                    (step 3's order at flm_sampling), listed in that order; -inf entries take part, so a row with fewer than n_top finite entries lists its -inf entries by
 *                    index; top_logit[j] = R[top_id[j]]; the entries at and beyond n_top are 0
 * No logarithm is taken on the device: the caller evaluates (logit - max_logit) - log(sum) in double from bit-exact ingredients, flm_score's rule.  Rows with a NaN, or whose
 * maximum is -inf, are outside the contract.  The host restatement is host/sampler.cpp logprob_row; the device equals it element for element.
 * source selects R: FLM_LOGPROBS_RAW = the classifier's row L, the model's own distribution; FLM_LOGPROBS_SHAPED = the row S the sampler reads, after steps 0 - 4 (mask, bias,
 * penalties, top-k, min-p).  Both are evaluated at temperature 1.  NOT built: dividing by the sampler's temperature, top-p renormalisation, records through the streaming
 * callback (flm_token_cb is unchanged), tensor-parallel contexts, vocabularies beyond the sampler's bound, prompt tokens (that is flm_score_tokens).
 * flm_logprobs_arm is a context setting like flm_constraint_arm (top_n -1: off).  It allocates nothing and re-captures nothing: top_n and source live in a device block that
 * exists since flm_ctx_create (its contents are rewritten), like the record buffer of max_seq_len records, and the armed token graphs are built at flm_prepare next to the
 * shaped ones.  flm_query "logprobs_top_n" reads the setting (-1: off).  (Not an option: flm_set_option drops the graphs.)  FLM_ERR_INVALID for top_n outside -1 .. 20 or a
 * source other than 0 / 1; FLM_ERR_UNSUPPORTED on a sharded context and where the vocabulary is beyond the device sampler's LDS strip (the sum chain's bound, as in
 * flm_score_tokens); FLM_ERR_STATE before the model is complete.
 * While armed, the four _ex entry points -- flm_generate_ex, flm_forward_sample_ex, flm_verify_sample_ex, flm_generate_lookup_ex -- write one record per delivered id, record i
 * for out_tokens[i] (flm_forward_sample_ex: one record per call).  An armed context counts as a control that is set: with every flm_sampling control neutral the shaped form
 * still runs, the ids count in "shaped_tokens", and S is L bit for bit.  Arming changes no result: the ids, *n_out, *rng_state, the callbacks, the K/V rows and
 * "constraint_state" equal the disarmed call's.  A stop token that is delivered has its record; the launches queued behind it write nothing.  Under source = raw with a control
 * or a constraint set, a verify batch is shaped into side rows ([16][vocab], there since flm_ctx_create) so that the raw rows survive.  A retried call rewrites its records.
 * The plain entry points ignore the setting.  On any error nothing is launched.
 * flm_last_logprobs copies records [first, first + n) of the last _ex call to the host, through the bounce buffer (in pieces if need be): the only place records cross the
 * bus -- an armed _ex call itself reads back nothing extra.  FLM_ERR_INVALID if first + n passes that call's *n_out (or n < 1); FLM_ERR_STATE if the last _ex call ran
 * disarmed or failed, or there was none. */
#define FLM_LOGPROBS_MAX 20
#define FLM_LOGPROBS_RAW 0
#define FLM_LOGPROBS_SHAPED 1
typedef struct flm_logprob { int32_t token; float logit, max_logit, sum; int32_t n_top;
                             int32_t top_id[FLM_LOGPROBS_MAX]; float top_logit[FLM_LOGPROBS_MAX]; int32_t pad_[3]; } flm_logprob; /* 192 bytes */
int  flm_logprobs_arm(flm_ctx* ctx, int top_n /* -1: off; 0 .. FLM_LOGPROBS_MAX */, int source);
int  flm_last_logprobs(flm_ctx* ctx, int first, int n, flm_logprob* out /* [n] */);
/* measurement tap (tools/sample_bench.py --logprobs), in the manner of flm_kernel_times: the mean duration in microseconds of ONE launch of the token form's stage, `iters`
 * launches enqueued back to back between one pair of HIP events, on the rows and the decode state the last armed _ex call left (each launch rewrites that call's last record
 * with the same bytes).  FLM_ERR_STATE unless the context is armed and its last _ex call delivered ids. */
int  flm_logprob_stage_time(flm_ctx* ctx, int iters, float* avg_us);
/* The entropy-driven samplers: locally typical sampling (llama-family `--typical P`) and Mirostat v2 (`--mirostat 2`, target entropy tau, learning rate eta, running state
 * mu).  No reference counterpart.  Two more stages, 5 and 6, behind steps 0 - 4 of flm_sampling, on the row R the sampler is about to read (the shaped row S; with every plain
 * control neutral: the classifier's row).  They act at temperature != 0 only: at temperature 0 both are neutral and mu does not move.  All arithmetic fp32 round-to-nearest
 * without contraction; the logarithm is flm_logf -- csrc/flm_logf.h: a fixed sequence of IEEE double operations, one function for host and device; within 1 ulp of libm.
 *   statistics   y = R / T, mx = max y, d = y - mx, e = d < -15 ? 0 : expf(d) (the sampler's clip), sum = the sequential fp32 chain of e in index order,
 *                p = e * (float)(1.0 / sum), ls = flm_logf of sum, surprise a = ls - d (nats).  Entries with e == 0 are DEAD: never candidates, left untouched
 *   5 typical    0 < typical_p < 1: H = the sequential chain in index order of h = p * a (dead: 0); key = fabsf(a - H); the live entries ordered by key ascending, equal
 *                keys by ascending index; c = c + p along that order from 0: the kept set ends with the first entry at which c > typical_p (included; none: all stay);
 *                every other live entry becomes -inf
 *   6 mirostat   mirostat == 2: a live entry stays iff a * 1.44269504f <= mu; the first maximum always stays; the others become -inf.  The unchanged sampler then draws id
 *                t at the call's temperature with topp = 1.0 (multinomial: flm_sampling's topp is ignored).  sum' = the sequential chain over the masked row,
 *                obs = (flm_logf of sum' - d[t]) * 1.44269504f, then in three operations mu = mu - eta * (obs - tau)
 * The host restatement is host/sampler.cpp entropy_logits / mirostat_update; the device (csrc/flm_entropy.h) equals it bit for bit.
 * flm_entropy_validate (pure host arithmetic): FLM_OK, or FLM_ERR_INVALID with flm_last_error(NULL) naming the rule -- typical_p a number, mirostat 0 or 2, tau, eta and mu
 * finite where mirostat is set, never both stages.
 * flm_entropy_set is a context setting like flm_logprobs_arm (NULL, or a struct with both stages off: off).  It allocates nothing and re-captures nothing: the parameters
 * and mu live in a device block that exists since flm_ctx_create, rewritten from the host's copy at the start of every attempt (a retried attempt updates nothing twice), and
 * the token form -- classifier, k_shape_logits, k_entropy_advance (the stage, the unchanged draw, mu's update, the token's last act: one launch) -- has its graphs built at
 * flm_prepare next to the shaped ones.  FLM_ERR_UNSUPPORTED on a sharded context and where the vocabulary is beyond the device sampler's LDS strip; FLM_ERR_STATE before
 * the model is complete.  flm_query "entropy": 0 off, 1 typical, 2 Mirostat.
 * While set, flm_generate_ex and flm_forward_sample_ex apply the stages; the setting counts as a control that is set (the ids count in "shaped_tokens").  With only
 * typical_p set, flm_verify_sample_ex, flm_generate_lookup_ex and flm_generate_draft apply stage 5 to every row of a verify batch (k_entropy_rows between the shaper and the
 * rows' draws): the stage is a function of the row alone, so the ids are flm_generate_ex's.  flm_entropy_mu: the state behind exactly the ids delivered so far, the halting
 * id's update included (moved by nothing but a verified attempt's commit).  The plain entry points ignore the setting.
 * NOT built (FLM_ERR_UNSUPPORTED, nothing launched): Mirostat through the draft-and-verify entry points (row r's mu depends on the draws in front of it); this setting on
 * a context armed for log-probabilities; Mirostat v1; tensor-parallel contexts. */
typedef struct flm_entropy { float typical_p;      /* <= 0 or >= 1: off */
                             int32_t mirostat;     /* 0: off, 2: v2 */
                             float tau, eta, mu;   /* mu: the starting state (callers usually pass 2 * tau) */ } flm_entropy;
int  flm_entropy_validate(const flm_entropy* e);
int  flm_entropy_set(flm_ctx* ctx, const flm_entropy* e /* NULL: off */);
int  flm_entropy_mu(flm_ctx* ctx, float* mu);
/* Stop rules on the device: a set of stop ids and up to 16 short stop sequences, next to the entry point's one stop token -- several end ids (a vocabulary's eos, a chat
 * model's end-of-turn id) and the `stop` strings of the serving APIs, token level.  No reference counterpart (its loop ends on token 0 only).  The decision is taken on the
 * device in the token's last act, so a call that ends on a rule is as exact about where it ends as one that ends on the stop token; a callback's cancel is not (it lands one
 * or more tokens behind).
 *   when a rule fires   take t[0 .. n), the ids THIS call has delivered (the prompt and the ids of earlier calls take no part).  Index i fires when
 *                 kind 1  t[i] == stop_token, the entry point's own argument;
 *                 kind 2  t[i] is one of ids; rule = its lowest position in ids;
 *                 kind 3  some sequence s of length L <= i + 1 has t[i - L + 1 .. i] == seq_s; rule = the lowest such s.
 *               Several at one index: preferred in that order.  The call ends at the first firing index (and at max_tokens, and behind a cancel, as before).
 *   the final id  is treated exactly as the stop token: delivered and counted with last = 1, NOT fed -- no K/V row, no further draw.  The earlier ids of a fired sequence
 *               were ordinary tokens and have their rows: the cache holds pos + n_prompt + *n_out - 1 rows, *rng_state is the state after exactly *n_out draws,
 *               "constraint_state" is folded over the delivered ids, there is one log-probability record per delivered id.
 * flm_stop_validate (pure host arithmetic, like flm_dfa_validate): FLM_OK, or FLM_ERR_INVALID with flm_last_error(NULL) naming the rule -- n_ids in [0, FLM_STOP_IDS_MAX],
 * n_seqs in [0, FLM_STOP_SEQS_MAX]; ids distinct and in [0, vocab); seq_ptr[0] = 0, not decreasing, every length in [1, FLM_STOP_SEQ_LEN_MAX]; sequence tokens in [0, vocab).
 * flm_stop_match (pure host arithmetic; r may be NULL, stop_token -1: none; the rules are taken as valid): the first index of ids[0 .. n) that fires, with its *kind and
 * *rule, or n with *kind = FLM_STOP_LENGTH.  The host restatement of the definition (host/stop_rules.h: a direct suffix comparison per index), which the device equals index
 * for index.
 * flm_stop_set installs or replaces the rules (NULL, or a set with no id and no sequence: removes them), validated against the model's vocabulary.  A context setting like
 * flm_constraint_set, but it allocates nothing and re-captures nothing: the rule block has a fixed size (at most 64 + 17 + 512 words and its counts), exists in device memory
 * since flm_ctx_create, and the shaped token graphs reach it through a pointer captured at flm_prepare; only its contents are rewritten, and a host copy is kept.
 * FLM_ERR_UNSUPPORTED on a sharded context and where the vocabulary is beyond the device sampler's LDS strip (the shaped form ends in the plain argmax there, which takes no
 * rules); FLM_ERR_STATE before the model is complete; FLM_ERR_INVALID as flm_stop_validate reports it.  On an error nothing is launched and the installed rules stay.
 * Where the rules apply: in flm_generate_ex and flm_generate_lookup_ex ONLY.  An installed non-empty rule set counts as a control that is set: with every flm_sampling control
 * neutral the shaped form still runs and the ids count in "shaped_tokens".  In a draft-and-verify step the accept step cuts the verified run behind the first firing index,
 * evaluated against the ids the call has delivered followed by the run.  The PLAIN entry points ignore the rules, and so do flm_forward_sample_ex and flm_verify_sample_ex:
 * their callers hold the ids and call flm_stop_match themselves.
 * flm_query: "stop_rules" = 1 when rules are installed; "stop_reason" / "stop_rule" describe the last generate-family call (flm_generate, flm_generate_ex, flm_generate_lookup
 * and its _sample / _ex forms): the host runs flm_stop_match's rule at the last delivered index -- a rule fires there: its kind and rule; otherwise *n_out < max_tokens: cancel;
 * otherwise length (nothing extra is read back, as for "constraint_state").  The plain forms report reasons 0, 1 and 4.
 * flm_op_stop_match (op level): flm_stop_match's result through the device function the token form runs (csrc/flm_stop.h), on caller-supplied ids: *first, *kind, *rule.
 * NOT built: text-level matching across tokenisations, withholding the ids of a partially matched sequence from the callback, min_tokens, tensor-parallel contexts, rules in
 * the plain entry points or in the one-launch greedy token. */
#define FLM_STOP_IDS_MAX     64
#define FLM_STOP_SEQS_MAX    16
#define FLM_STOP_SEQ_LEN_MAX 32
typedef struct flm_stop_rules {
    int32_t n_ids;  const int32_t* ids;            /* distinct, in [0, vocab) */
    int32_t n_seqs; const int32_t* seq_ptr;        /* [n_seqs + 1], seq_ptr[0] = 0; sequence s = seq_tokens[seq_ptr[s] .. seq_ptr[s + 1]), length 1 .. FLM_STOP_SEQ_LEN_MAX */
    const int32_t* seq_tokens;                     /* ids in [0, vocab) */
} flm_stop_rules;
#define FLM_STOP_LENGTH 0   /* max_tokens reached */
#define FLM_STOP_TOKEN  1   /* the entry point's stop_token */
#define FLM_STOP_ID     2   /* one of the rules' ids */
#define FLM_STOP_SEQ    3   /* one of the rules' sequences */
#define FLM_STOP_CANCEL 4   /* behind a callback's non-zero return */
int  flm_stop_validate(const flm_stop_rules* r, int vocab);
int  flm_stop_match(const flm_stop_rules* r /* may be NULL */, int32_t stop_token, const int32_t* ids, int n, int* kind, int* rule);
int  flm_stop_set(flm_ctx* ctx, const flm_stop_rules* r /* NULL: remove */);
int  flm_op_stop_match(const flm_stop_rules* r, int32_t stop_token, const int32_t* ids, int n, int* first, int* kind, int* rule);
/* the ids generated by the last flm_decode_greedy / flm_decode_sample / flm_decode_timed* call: out[n] (n <= its n_steps) */
int  flm_last_tokens(flm_ctx* ctx, int n, int32_t* out);
int  flm_reset_kv(flm_ctx* ctx);
int  flm_sync(flm_ctx* ctx);

/* Per-kernel timing at position pos with HIP events on the ctx's stream, averaged over `iters` rounds.
 * Classes: 0 embed, 1 qkv, 2 attn, 3 attn_o, 4 ffn13, 5 ffn2, 6 cls, 7 argmax, 8 allreduce (tensor parallel), and the two fused launches
 * the single-GPU token path runs instead of (2, 3) and (4, 5): 9 attn_wo (attention + Wo), 10 ffn (FFN13 + FFN2); count 0 = not in use.
 * 11 qkv_attn_wo: QKV + attention + Wo in one launch, what the token path runs instead of (1, 9) at long contexts ("fuse_qkv").
 * 12 layer: the whole decoder layer in one launch (k_attn_ffn: QKV, attention, Wo, FFN13, FFN2 -- what the token path runs instead of (1, 9, 10) where a head is
 * one workgroup and the head size a multiple of 64; option "fuse_layer"), 13 back: the same without the QKV GEMV ("fuse_layer" 0: instead of (9, 10)).
 * 14 layers: ALL layers of the token in one launch (k_layers: what the token path runs instead of L launches of class 12; option "fuse_token"): ONE launch per token,
 * avg_us = the duration of that launch, flm_kernel_bytes = L layers' bytes.
 * 15 token: a greedy decode token as ONE launch (k_layers<.., TAIL>: the embedding row read by the first layer, the L layers, the classifier, the argmax and the state's advance;
 * option "fuse_tail"; what flm_decode_* runs instead of (0, 14, 6, 7) for fp32 embedding tables where the arrival-order launch runs); bytes = the layers' + the classifier's.
 * avg_us[c] = mean duration of ONE launch of class c (single GPU: the class's launches of one token are
 * enqueued back to back between one pair of events, so the figure is launch duration + dispatch gap and
 * agrees with a rocprofv3 kernel trace), count[c] = launches of that class per token.
 * Side effect: the KV cache is cleared and the decode state is undefined afterwards. */
#define FLM_KCLASSES 16
int  flm_kernel_times(flm_ctx* ctx, int pos, int iters, float* avg_us, int32_t* count);
/* weight + scale bytes one launch of class c streams (the algorithmic bytes of DESIGN.md) */
int  flm_kernel_bytes(flm_ctx* ctx, int kclass, int pos, double* bytes);

/* debugging tap for the parity tests: copy an internal fp32 device buffer to the host.
 * what: 0 residual x1[dim], 1 q[dim], 2 attention output[dim], 3 hd[hidden], 4 K cache of `layer`
 * [heads][max_seq][hs], 5 V cache of `layer`, 6 logits; 11 / 12 the never-cleared flag lines / granule tags that
 * count from the epoch counters, as raw 32-bit words (the long-lived-context tests); 13 flm_generate's granule ring as the last call left it, two raw 32-bit
 * words per entry: {token | last << 31, the call's tag}; 14 the per-token log-probability records as the device holds them (the slots behind the last call's *n_out
 * included), 48 raw 32-bit words per record. */
int  flm_debug_read(flm_ctx* ctx, int what, int layer, float* out, size_t n);

/* Structure switches: which launches a token runs.  None of them changes a result bit; the defaults are what was measured fastest.
 *   "use_graph"      0 = launches enqueued eagerly (default 1: a token is one hipGraph replay)
 *   "graph_chunks"   0 = one graph launch per greedy token (default 1: flm_decode_* replay graphs of up to 16 tokens -- the device idles ~10 us between two graph launches, ~1.5 between two nodes)
 *   "fuse_attn_o"    0 = attention and the Wo GEMV as two launches (default 1: one launch, single GPU)
 *   "fuse_ffn"       0 = FFN13 and FFN2 as two launches (default 1)
 *   "fuse_qkv"       QKV in the same launch as attention + Wo: 0 never, 1 (default) where a head is spread over several workgroups, 2 always
 *   "fuse_back"      0 = attention + Wo and FFN13 + FFN2 as two launches (k_attn_o, k_ffn) instead of one (k_attn_ffn; default 1)
 *   "fuse_layer"     0 = the QKV GEMV as its own launch in front of k_attn_ffn (default 1: the whole decoder layer in one launch)
 *   "fuse_token"     0 = one launch per layer instead of one for all layers (k_layers; default 1: the edge between two layers is a flag round)
 *   "fuse_tail"      0 = a greedy decode token as four launches (embedding row, k_layers, classifier, argmax) instead of one (default 1)
 *   "back_ao"        0 = inside k_layers, Wo and FFN2 wait for ALL producers of their activation (round 4); default 3: consumed in arrival order (a wave waits
 *                    for the producers of its own steps' column blocks only)
 *   "attn_split"     0 = one workgroup per head at every context length (default 1: hs / 32 workgroups per head from 128 positions on; n >= 2: always n)
 *   "use_prefill"    0 = prompts token by token (default 1: batched; under tensor parallelism once the peers are mapped with flm_p2p_import)
 *   "score_rows"     n = flm_score_tokens runs its classifier on chunks of at most n rows (default 0: as many rows as the staging holds; < 0: one row at a time through the logits vector, the staging of a context without prefill scores)
 *   "spec_gemm"      1 = flm_verify_greedy / flm_generate_lookup and their sampled forms run the verify batch's int8 GEMMs on the skinny kernel for <= 16 rows (default 0: the prompt path's 64 x 64
 *                    tiles, until both forms have been timed on the device: DESIGN.md section 5e); the same bits; no other entry point looks at it
 *   "batch_rows"     b >= 0 = flm_generate_batch admits every request and runs ragged passes with a budget of b prompt rows each (0: no bound); default -1: serial joins, then
 *                    steps; the same results; read per call
 *   "use_prefill_mq" 0 = batched attention with one query per workgroup (default 1: eight)
 *   "use_qk_mfma" / "use_pv_mfma"  0 = prefill scores / softmax x V on VALU chains (default 1: v_mfma_f32_16x16x4_f32, the same bits)
 * Tensor parallel (set on every rank alike, before flm_p2p_export where noted):
 *   "use_p2p"        0 = exchanges by RCCL all-gathers although the peers are mapped (1: peer to peer again)
 *   "fold_xchg"      0 = every peer-to-peer exchange's flag round as a launch of its own (k_xchg); default 1: inside the launch that consumes the vector
 *   "tp_fuse_attn"   folded exchanges: 1 = attention + Wo in ONE launch across the ranks, 2 (default) = with the QKV GEMV in front, 0 = separate launches
 *   "tp_fuse_ffn"    the same for FFN13 + FFN2 (default 0)
 *   "tp_fuse_layers" 1 (default) = ALL layers of a sharded token in one launch per rank that spans the ranks (k_layers<.., TP>: the single-GPU persistent launch with the
 *                    reference's row split across the ranks; the four hand-offs of a layer are flag rounds between the ranks' workgroups); where the group can span
 *                    (folded exchanges, every rank's workgroups resident, identical geometry), else the per-layer launches above; before flm_p2p_export
 *   "tp_fence"       that launch's system-scope fences: bit 0 release in front of a cross-rank flag line, bit 1 acquire behind a cross-rank poll; -1 (default) = none between
 *                    ranks of ONE device, both between distinct devices (every cross-rank access is itself a system-scope atomic or a coherent load: the fences are belt and braces,
 *                    and cost ~20 us per hand-off)
 *   "gr_edges"       1 (default) = inside the one-launch token (one GPU) and inside the rank-spanning launch (tensor parallel, where every rank says so; before flm_p2p_export) the
 *                    vectors that cross workgroups / ranks -- the residual stream behind Wo and behind FFN2; across ranks also the heads' output and FFN13's hd -- travel as
 *                    8-byte {value, tag} granules: ONE aligned store per element, the tag = the hand-off's flag value.  The data is its own flag: no drained stores, no flag
 *                    line, no fence, nothing inferred from the ORDER of stores (over xGMI a granule is one write); the consumers re-read their own granules until the tags
 *                    match.  0 = flag rounds (rounds 4-5).  Same results bit for bit
 *   "tp_trust_fused" 1 = between DISTINCT devices too, run the folded exchanges / rank-spanning launches (default 0: the k_xchg launches; before flm_p2p_export)
 *   "cu_parts"       n = confine the context's stream to 1/n of the device's CUs (part rank % n): several ranks on ONE GPU (tests)
 *   "force_tp"       1 = a context created with an RCCL id and world == 1 takes the sharded token path (RCCL exchanges over a 1-rank communicator; tests)
 * Not part of the boundary: the experiment dials whose optimum was measured and fixed (stash slots, early register sets, tile shapes: the rows marked kOptDial in the option table, csrc/flm_tuning.h) are refused
 * until "tuning" 1 has been set; switches that skip work ("ablate", "trace") exist only in -DFLM_ABLATE=1 builds.  Unknown key: FLM_ERR_INVALID. */
int  flm_set_option(flm_ctx* ctx, const char* key, int value);
/* What the context actually runs (bench.py reports it; a caller can see that a fused launch was given up).  Keys: every flm_set_option key
 * (its current value; the dials of csrc/flm_tuning.h too), "tuning", and
 *   "resident"  1 = the census at flm_ctx_create saw one 1024-thread workgroup per CU co-resident (the fused launches wait across workgroups;
 *               0 = they were switched off up front: a masked / partitioned device),
 *   "fallback"  how many times a cross-workgroup wait timed out during a call and the context fell back to one kernel per phase (flm_gpu.hip
 *               xwg_check; the call itself was re-run and returned correct results), "fallback_active" 1 = it is on that path now (after 64 tokens the census
 *               runs again and a context whose workgroups are all resident returns to the launch structure it had),
 *   "token_path" bit 0 attention + Wo fused, bit 1 FFN13 + FFN2 fused, bit 2 QKV joins the attention's launch at long contexts, bit 3 the same
 *               at every context, bit 6 heads split over workgroups at long contexts, bit 7 attention .. FFN2 in one launch (k_attn_ffn), bit 8 with the QKV GEMV in front
 *               (the whole layer in one launch), bit 9 all layers of the token in one launch (k_layers), bit 10 a greedy decode token is ONE launch (embedding row, layers,
 *               classifier, argmax in k_layers<.., TAIL>),
 *   "ao_active" which hand-offs of that launch are consumed in arrival order: bit 0 Wo, bit 1 FFN2 (-1: the launch has not been planned yet),
 *   "sampled_tokens" how many tokens this context sampled on the device (flm_forward_sample / flm_decode_sample / flm_generate / flm_verify_sample / flm_generate_lookup_sample at temperature > 0),
 *   "shaped_tokens" how many tokens this context drew under the controls (flm_generate_ex / flm_forward_sample_ex / flm_verify_sample_ex / flm_generate_lookup_ex with a control set or a constraint armed),
   "constraint_state" the automaton state the context is armed at (flm_constraint_arm; moved on by every _ex call over the ids it delivers), -1: disarmed,
 *   "entropy" the entropy-driven sampler the context is set to (flm_entropy_set): 0 off, 1 locally typical, 2 Mirostat v2,
 *   "logprobs_top_n" the top_n the context is armed with for per-token log-probabilities (flm_logprobs_arm), -1: off,
 *   "stop_rules" 1 = stop rules are installed (flm_stop_set), "stop_reason" / "stop_rule" why the last generate-family call ended (FLM_STOP_LENGTH .. FLM_STOP_CANCEL) and, for
 *               an id or a sequence, which one,
 *   "spec_steps" / "spec_accepted" the last flm_generate_lookup / flm_generate_lookup_sample call: verify passes run / drafted ids accepted in them,
 *   "draft_tokens" the last flm_generate_draft call: tokens the draft context computed (its prompt feed, its drafts, its catch-up feeds),
 *   "gen_tokens" / "gen_streamed" the last flm_generate call: tokens delivered / how many of them were delivered while hipStreamQuery still said the stream was busy,
 *   "epoch_tail" / "epoch_eng" / "epoch_xchg" the epoch counters the cross-workgroup waits count from (device memory; the 32-bit pattern): the one-launch token's, the
 *               tensor-parallel token's epoch base, k_xchg's logits exchanges (the long-lived-context tests).
 * Unknown key: FLM_ERR_INVALID. */
int  flm_query(flm_ctx* ctx, const char* key, int* value);

/* ---- op level: 1:1 mirrors of the reference operator seam, host pointers in / out, running the
 *      same device code as the fused path.  Used by the parity tests. ----------------------- */
/* quant::quantize (quant_operators.cpp:78-97) */
int  flm_op_quantize(int qt, void* qx, float* qs, const float* x, size_t n, int gs);
/* quant::matmul (quant_operators.cpp:571-591), same argument order: out[w][m].  w < 16: one GEMV per batch row (the decode
 * kernel); w >= 16: the tile kernels of the batched prompt path (int8 and int16 on the int8 matrix cores; FLM_OP_GEMM=1|2|3: the tile shape) */
int  flm_op_matmul_q(int qt, float* out, const void* mat1, const float* scales1,
                     const void* mat2, const float* scales2, int m, int n, int w, int gs);
/* the same product for 1 <= w <= 16 batch rows through the skinny int8 kernel of the verify pass (k_gemm_q8_skinny); FLM_QT_INT8 only
 * (FLM_OP_SKINNY_NB=1|2: 16-row fragments per wave; by size otherwise) */
int  flm_op_matmul_skinny(int qt, float* out, const void* mat1, const float* scales1,
                          const void* mat2, const float* scales2, int m, int n, int w, int gs);
/* the prompt-lookup drafter of flm_generate_lookup (k_spec_draft) on a caller-supplied history h[n]: d[k], 1 <= k <= 15, 1 <= ngram_max <= 8 */
int  flm_op_spec_draft(const int32_t* h, int n, int k, int ngram_max, int32_t* d);
/* simd::rmsnorm(o,x,w,n) (x86_simd.cpp:1754-1764) */
int  flm_op_rmsnorm(float* o, const float* x, const float* w, size_t n);
/* simd::square_sum (x86_simd.cpp:942-960), n % 16 == 0, n <= 16384: out6 = { total from the speculative wave evaluation the
 * rmsnorm prologue uses, total from the plain sequential chains, the 4 strided partial sums }; the two totals must be the same bits */
int  flm_op_square_sum(const float* x, size_t n, float* out6);
/* sample_argmax (sampler.cpp:36-47): first maximum wins */
int  flm_op_argmax(const float* logits, int n, int32_t* idx);
/* Sampler::sample (sampler.cpp:113-137) through k_sample_advance, the kernel of flm_forward_sample / flm_decode_sample: logits[n] are not modified;
 * *rng_state in / out as there.  n >= 2. */
int  flm_op_sample(const float* logits, int n, float temperature, float topp, uint64_t* rng_state, int32_t* out);
/* the sampler of flm_verify_sample (k_sample_rows) on caller-supplied logits[rows][ld], n entries per row, 1 <= rows <= 16, ld >= n >= 2: out[i] = row i drawn with the
 * (i + 1)-th coin of *rng_state, i.e. what `rows` successive flm_op_sample calls on the rows return; *rng_state out: the state after `rows` draws (temperature 0: untouched) */
int  flm_op_sample_rows(const float* logits, int rows, int ld, int n, float temperature, float topp, uint64_t* rng_state, int32_t* out);
/* the shaping stage of flm_generate_ex (k_shape_logits) on caller-supplied logits[n], n >= 2, and window[n_window] used as given: out[n] = the shaped row (steps 1 - 4 of the
 * definition at flm_sampling; sampling->temperature is min-p's divisor, topp is not used).  No bound on n.  Errors as there. */
int  flm_op_shape_logits(const float* logits, int n, const flm_sampling* sampling, const int32_t* window, int n_window, float* out);
/* the shaper of flm_verify_sample_ex (k_shape_rows) on caller-supplied logits[rows][ld], n entries per row, 1 <= rows <= 16, ld >= n >= 2: out[r][0 .. n) = row r shaped over
 * the last min(penalty_last_n, n_window + r) ids of window ++ drafts[0 .. r) -- flm_op_shape_logits on row r with that window.  drafts: rows - 1 ids in [0, n) (may be NULL
 * for rows == 1).  No bound on n.  Errors as there. */
int  flm_op_shape_rows(const float* logits, int rows, int ld, int n, const flm_sampling* sampling, const int32_t* window, int n_window,
                       const int32_t* drafts /* [rows - 1] */, float* out /* [rows][n] */);
/* flm_op_shape_rows with the automaton added (k_shape_rows with its step 0): row r is masked in delta folded over drafts[0 .. r) from `state`, then shaped as there;
 * states_out[r] receives that state.  dfa is validated against n; state in [0, n_states).  Drafts without an edge leave the state where it is. */
int  flm_op_constrain_rows(const float* logits, int rows, int ld, int n, const flm_sampling* sampling, const int32_t* window, int n_window,
                           const int32_t* drafts /* [rows - 1] */, const flm_dfa* dfa, int32_t state, float* out /* [rows][n] */, int32_t* states_out /* [rows] */);
/* flm_score_tokens' statistics kernel (k_score_rows) on caller-supplied logits[rows][n]: out[rows]; targets[rows] as there (NULL: none).  2 <= n, n within the LDS bound. */
int  flm_op_score_rows(const float* logits, int rows, int n, const int32_t* targets, flm_score* out);
/* the record stage of flm_logprobs_arm (k_logprob_rows) on caller-supplied logits[rows][ld], n entries per row, 1 <= rows <= 16, ld >= n >= 2, n within the LDS bound:
 * out[r] = the flm_logprob of row r with drawn id chosen[r] in [0, n) and top_n in [0, FLM_LOGPROBS_MAX]. */
int  flm_op_logprob_rows(const float* logits, int rows, int ld, int n, const int32_t* chosen /* [rows] */, int top_n, flm_logprob* out /* [rows] */);
/* csrc/flm_logf.h's flm_logf as the device evaluates it, in place over n positive normal floats: the tests pin it to the host's compilation of the same header */
int  flm_op_logf(float* x, size_t n);
/* the entropy-driven stages of flm_entropy_set (k_entropy_rows) on caller-supplied logits[rows][ld], n entries per row, 1 <= rows <= 16, ld >= n >= 2, n within the LDS
 * bound: out[r][0 .. n) = row r after stage 5 (e->typical_p) or stage 6 at mu[r] (e->mirostat == 2; mu: [rows], e->mu is not used), at `temperature`.  chosen given
 * ([rows], ids in [0, n); Mirostat only): obs_out[r] / mu_out[r] = the observed surprise of chosen[r] on the masked row and the updated state (e->tau, e->eta). */
int  flm_op_entropy_rows(const float* logits, int rows, int ld, int n, float temperature, const flm_entropy* e, const float* mu /* [rows] or NULL */,
                         const int32_t* chosen /* [rows] or NULL */, float* out /* [rows][n] */, float* obs_out /* [rows] or NULL */, float* mu_out /* [rows] or NULL */);
/* simd::swiglu(xo,xr,n) (x86_simd.cpp:1766-1770) */
int  flm_op_swiglu(float* xo, const float* xr, size_t n);
/* rope_v2 (tf_operators.cpp:352-402): one head row of n_dims at position pos */
int  flm_op_rope(float* o, const float* x, int n_dims, int pos);
/* softmax_sisd over the first n entries (tf_operators.cpp:176-186) */
int  flm_op_softmax(float* x, int n);
/* the ATTN task (execute_attn, transformer.cpp:397-455) for n_heads heads of one new token at
 * position pos: q,k,v are [n_heads*hs]; kc,vc are [n_heads][max_seq][hs] caches (updated);
 * out [n_heads*hs]. */
int  flm_op_attention(float* out, float* kc, float* vc, const float* q, const float* k, const float* v,
                      int n_heads, int hs, int max_seq, int pos);
/* the same task for the n rows of one flm_generate_n step (k_rope_kv_fan + k_attn_fan, csrc/flm_fan.h): q, k, v are [n][n_heads*hs], all at logical position S + t; row j's
 * k / v go to cache row base[j] + t and its query attends rows 0 .. S - 1 followed by base[j] .. base[j] + t.  kc, vc as above (updated); out [n][n_heads*hs].
 * 2 <= n <= FLM_FAN_MAX, hs <= 128, S >= 1, S + t + 1 <= max_seq and every base[j] + t < max_seq (FLM_ERR_INVALID otherwise). */
int  flm_op_attention_fan(float* out, float* kc, float* vc, const float* q, const float* k, const float* v,
                          int n_heads, int hs, int max_seq, int n, int S, int t, const int32_t* base);
/* the same task for the n rows of one flm_batch_step (k_rope_kv_slots + k_attn_slots, csrc/flm_batch.h): q, k, v are [n][n_heads*hs]; row r is at ITS logical position pos[r]
 * of the slot that starts at cache row base[r] (and reaches to max_seq): its k / v go to cache row base[r] + pos[r], its query attends rows base[r] .. base[r] + pos[r].
 * kc, vc as above (updated); out [n][n_heads*hs].  1 <= n <= FLM_BATCH_MAX, pos[r] >= 0, base[r] >= 0, base[r] + pos[r] < max_seq (FLM_ERR_INVALID otherwise). */
int  flm_op_attention_slots(float* out, float* kc, float* vc, const float* q, const float* k, const float* v,
                            int n_heads, int hs, int max_seq, int n, const int32_t* base, const int32_t* pos);
/* the same task for the B rows of one flm_batch_pass (csrc/flm_segs.h): n_segs <= FLM_BATCH_MAX segments whose rows follow one another in q, k, v [B][n_heads*hs], B = the
 * sum of n[s].  Segment s lies in the slot [base[s], base[s] + rows[s]) and enters at logical position pos0[s]: row i of it is rotated at pos0[s] + i, its k / v go to cache
 * row base[s] + pos0[s] + i, its query attends the slot's rows 0 .. pos0[s] + i.  The first n_step segments are step rows (n[s] = 1: k_rope_kv_slots + k_attn_slots), the
 * rest prompt segments (k_rope_kv_segs + k_seg_views + k_attn_segs_mq; one_query != 0, head sizes above 128 or a multi-query LDS that does not fit: k_attn_segs).
 * FLM_ERR_INVALID, with nothing launched, for more than FLM_BATCH_MAX segments, a segment outside its slot, a slot outside the cache, or a sum of n[s] other than B. */
int  flm_op_attention_segs(float* out, float* kc, float* vc, const float* q, const float* k, const float* v,
                           int n_heads, int hs, int max_seq, int B, int n_segs, int n_step, const int32_t* base, const int32_t* rows, const int32_t* n, const int32_t* pos0,
                           int one_query);
/* libm expf as the device evaluates it (the reference calls glibc expf in softmax_sisd and swiglu);
 * in place over n floats.  Lets the tests pin the device routine against glibc bit for bit. */
int  flm_op_expf(float* x, size_t n);
/* elementary fp32 functions as the kernels evaluate them, in place over x[n]:
 * fn 0 expf(x), 1 sqrtf(x), 2 x / y, 3 rmsnorm scale 1/sqrtf(x/n + 1e-5) with n = (int)y[i],
 * 4 / 5 quant::quantize's element step q(x) = (T)(x / y) (quant_operators.cpp:26-47) the way the prologues evaluate it (4: the group's four divisions share one refined
 *       reciprocal) and as a plain IEEE division (5): x[i] <- q(x) - 1024 q(-x); the two must agree on every input. */
int  flm_op_math(int fn, float* x, const float* y, size_t n);
/* the hand-off protocol of the fused launches on its own (no reference counterpart: it replaces the reference's thread-pool task barrier,
 * src/components/threadparallel.hpp, inside one GPU launch): `rounds` publish -> flag -> poll -> coherent-read rounds between one workgroup per CU,
 * every value read checked.  *wrong_values / *timed_out must both come back 0. */
int  flm_op_handoff_litmus(int rounds, int* wrong_values, int* timed_out);

/* ---- tensor-parallel shard plan (pure host arithmetic, no GPU needed).
 * Every matmul is split by OUTPUT ROWS, as the reference splits them over its worker threads
 * (split_rows, transformer.cpp:264-287): each output row is reduced on one rank in the reference's
 * order, so a sharded run is bit-identical to the single-GPU / CPU run.  Ranks exchange activation
 * slices with all-gathers (attention outputs, the residual stream twice, the FFN hidden vector, the
 * logits), which is why every split is an equal contiguous slice. */
typedef struct flm_shard_plan {
    int32_t head_begin, head_count;        /* attention heads owned: q,k,v rows, KV cache, attention */
    int32_t hidden_begin, hidden_count;    /* rows of W1/W3 owned (slice of the FFN hidden vector) */
    int32_t dim_begin, dim_count;          /* rows of Wo and W2 owned (slice of the residual stream) */
    int32_t vocab_begin, vocab_count;      /* classifier rows */
} flm_shard_plan;
int  flm_plan_shards(const flm_model_desc* desc, int rank, int world, flm_shard_plan* out);

#ifdef __cplusplus
}
#endif
#endif
