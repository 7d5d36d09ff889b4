// engine.h -- the MI355X counterpart of ParallelTransformer (src/transformer/transformer.h:76-96): same public
// surface (load / encode / decode / generate / get_quant_type), the per-token forward runs on the GPU through
// the C ABI in include/flm_gpu.h.
#pragma once
#include <functional>
#include <string>
#include <vector>

#include "flm_gpu.h"
#include "model_file.h"
#include "sampler.h"
#include "tokenizer.h"

namespace flmhost {

// "title[ a,  b, ...]" with every number right-aligned to the widest one, like the reference's print_vector
void print_vector(const char* title, const std::vector<int>& vec);

class GpuTransformer {
public:
    explicit GpuTransformer(bool debug) : _debug(debug) {}
    ~GpuTransformer();
    // load(ckpt, tokenizer, file type, -q quant type, devices): transformer.cpp:23-42.  More than one device = the reference's parallel width
    // (main.cpp:30,78 `-j`, split_rows transformer.cpp:264-287) on GPUs: ONE sequence, every matmul split by output rows over the devices, one host
    // thread per device (a tensor-parallel rank of the C ABI), activation slices exchanged peer to peer.  A device may be named more than once
    // (ranks sharing a GPU: how the 1-GPU test box exercises the path).
    bool load(const std::string& ckpt, const std::string& tknr, FileType ft, int qtype, const std::vector<int>& devices, uint64_t seed = 0);
    bool load(const std::string& ckpt, const std::string& tknr, FileType ft, int qtype, int device, uint64_t seed = 0) { return load(ckpt, tknr, ft, qtype, std::vector<int>{device}, seed); }
    std::vector<int> encode(const char* prompt) const;
    std::string decode(const std::vector<int>& tokens) const { return _tok.decode(tokens); }
    // generate(prompt, cb(text, n_input, n_output, ended), max_new_tokens, temperature, topp): transformer.cpp:54-103
    bool generate(const char* prompt, const std::function<bool(const char*, int, int, bool)>& cb, int max_new_tokens, float temperature, float topp);
    // --samples N (this build only; one device, none of the other extras): N completions of the prompt, all N drawn per pass over the weights (flm_generate_n; N == 1:
    // flm_generate).  Sample j's sampler state is seed + j -- here --seed counts, where the plain run keeps the reference's state 0 --, every sample stops on token 0 by
    // itself and max_new_tokens is cut to what the N tails leave room for.  texts[j]: sample j's pieces as generate() would have streamed them
    bool generate_samples(const char* prompt, int n, uint64_t seed, int max_new_tokens, float temperature, float topp, std::vector<std::string>& texts);
    // --prompts FILE (this build only; one device, none of the other extras): 1 .. 16 INDEPENDENT prompts served together, one batch per pass over the weights
    // (flm_generate_batch).  Prompt j's sampler state is seed + j, every completion stops on token 0 by itself, and max_new_tokens is cut to an equal share of the cache.
    // texts[j]: what generate_samples(prompts[j], 1, seed + j, ...) gives
    // batch_rows >= 0 (--batch-rows): option "batch_rows" -- the prompts are admitted and enter inside the steps' passes (flm_batch_pass); the same texts
    bool generate_prompts(const std::vector<std::string>& prompts, uint64_t seed, int max_new_tokens, float temperature, float topp, std::vector<std::string>& texts, int batch_rows = -1);
    // --mode score (this build only): the prompt's tokens through flm_score_tokens in one call; one line per position (index, token id, argmax id, the probability of the
    // next token), then a summary line (token count, mean natural-log loss, perplexity, ms)
    bool score(const char* prompt);
    // --lookup K[,G] (this build only): temperature-0 generation on one device runs through flm_generate_lookup (draft-and-verify with the prompt-lookup drafter: the same ids,
    // several per pass over the weights); lookup_steps / lookup_accepted: verify passes run / drafted ids accepted, summed over the generate calls
    void set_lookup(int draft_len, int ngram_max) { _lookup_k = draft_len; _lookup_g = ngram_max; }
    // --draft K[,G] (this build only): the same at whatever temperature the run has: at 0 flm_generate_lookup, otherwise flm_generate_lookup_sample with the Sampler's state (written
    // back afterwards) -- the same ids as the sampled loop's; where the library refuses (FLM_ERR_UNSUPPORTED) the run is what it is without the flag.  Counted in lookup_steps / _accepted
    void set_draft(int draft_len, int ngram_max) { _draft_k = draft_len; _draft_g = ngram_max; }
    // --draft-model FILE (this build only; one device, after load): a second, small model of the same vocabulary on the same device (the quantisation: the file's own or -q),
    // paired with the model through flm_draft_set.  Generation then runs through flm_generate_draft -- draft-and-verify with that model as the drafter, draft length --draft K
    // (7 without the flag), at any temperature and under every control flag: the same ids and text as the run without the flag; where the library refuses the call as
    // unsupported the run is what it is without the flag.  Counted in lookup_steps / _accepted.  A missing or malformed file, another vocabulary size: false, error() says why
    bool load_draft(const std::string& ckpt, const std::string& tknr, FileType ft, int qtype, int device);
    // --top-k / --min-p / --repeat-penalty / --repeat-last-n / --presence-penalty / --frequency-penalty / --logit-bias (this build only): the sampling controls of flm_sampling.
    // One device: the whole loop is flm_generate_ex (the shaping stage on the device); where the engine samples on the host (a vocabulary beyond the device sampler, several
    // devices) it calls shape_logits in front of the host sampler: the same ids.  --lookup / --draft: flm_generate_lookup_ex, the same ids through draft-and-verify steps.
    // Not called: nothing changes.
    void set_sampling(const ShapeControls& c, int penalty_last_n, const std::vector<int32_t>& bias_ids, const std::vector<float>& bias_values) {
        _shape = c; _shape_last_n = penalty_last_n; _bias_ids = bias_ids; _bias_values = bias_values;
        _shape.n_bias = (int)_bias_ids.size(); _shape.bias_ids = _bias_ids.data(); _shape.bias_values = _bias_values.data();
        _shape_set = true;
    }
    // --constraint FILE (this build only): a token-level DFA (flm_dfa; the text format of capi.Dfa.save) masks every generated token's logits.  One device: installed with
    // flm_constraint_set, armed at state 0 before every generate; the run is flm_generate_ex / flm_generate_lookup_ex (neutral controls where no control flag was given).
    // Where the engine samples on the host (the library refuses, several devices) it calls constrain_logits and dfa_next itself: the same ids.
    void set_constraint(std::vector<int32_t> row_ptr, std::vector<int32_t> edge_token, std::vector<int32_t> edge_next) {
        _dfa_row = std::move(row_ptr); _dfa_tok = std::move(edge_token); _dfa_nxt = std::move(edge_next); _dfa_set = true; _dfa_installed = false;
    }
    // --logprobs N[,shaped] (this build only): the context is armed with flm_logprobs_arm before every generate on one device, the run takes the _ex path as an armed
    // constraint does, and the records of the last generate are kept for the caller: one flm_logprob per delivered token
    void set_logprobs(int top_n, bool shaped) { _lp_top_n = top_n; _lp_shaped = shaped; }
    // --typical / --mirostat: flm_entropy_set before every generate (Mirostat's state starts at e.mu each time); the run is flm_generate_ex (with --draft / --lookup and
    // typical: flm_generate_lookup_ex); where the loop is the host's, entropy_logits / mirostat_update behind shape_logits: the same ids.  Not together with --logprobs
    void set_entropy(const flm_entropy& e) { _ent = e; _ent_set = e.mirostat == 2 || (e.typical_p > 0.0f && e.typical_p < 1.0f); }
    const std::vector<flm_logprob>& logprobs() const { return _lp; }
    // --stop-ids / --stop-seq / --stop (this build only, one device): stop rules next to the loop's own stop on token 0 (flm_stop_rules).  ids: the stop ids; seqs: id
    // sequences; strs: strings, each tokenised ONCE by this tokenizer without BOS when the model is loaded and matched token by token on that one tokenisation (text that
    // tokenises differently in context does not match).  Installed with flm_stop_set before the first generate; the run is flm_generate_ex / flm_generate_lookup_ex
    // (neutral controls where no control flag was given): the device ends the call at the first index flm_stop_match names.  Refused by the library: an error
    void set_stop(std::vector<int32_t> ids, std::vector<std::vector<int32_t>> seqs, std::vector<std::string> strs) {
        _stop_ids = std::move(ids); _stop_seqs = std::move(seqs); _stop_strs = std::move(strs); _stop_set = true; _stop_installed = false;
    }
    // why the last generate on one device ended: FLM_STOP_LENGTH .. FLM_STOP_CANCEL and the rule (flm_query "stop_reason" / "stop_rule"); -1 where no call ran
    int stop_reason() const { return _stop_reason; }
    int stop_rule() const { return _stop_rule; }
    int lookup_steps() const { return _lookup_steps; }
    int lookup_accepted() const { return _lookup_accepted; }
    int get_quant_type() const { return _cfg.quant_type; }
    const std::string& error() const { return _err; }
    // more than one device: which launch structure of the sharded token load() settled on (calibrate_structure), for --detail
    const std::string& tp_structure() const { return _tp_structure; }
private:
    // Sharded over several devices: time ONE token under the conservative launch structure (exchange flag rounds as launches of their own between distinct devices), then
    // under each faster one ("tp_trust_fused" 1; + "tp_fuse_ffn" 1), and keep the fastest whose logits are the conservative structure's bit for bit -- nothing is trusted
    // that was not verified on THIS machine; a structure that gives up or differs is dropped and the group put back.
    bool connect_ranks();
    bool calibrate_structure();
    std::string _tp_structure;
    bool _debug;
    Config _cfg;
    Tokenizer _tok;
    Sampler _sampler;
    std::vector<flm_ctx*> _ctxs;                    // rank r's context (rank 0's results are the ones reported)
    // run f(rank) on every rank at once (the ranks wait for each other's slices inside the launches); first non-zero status wins
    int on_all(const std::function<int(int)>& f);
    std::string _err;
    int _lookup_k = 0, _lookup_g = 3, _lookup_steps = 0, _lookup_accepted = 0;
    int _draft_k = 0, _draft_g = 3;
    flm_ctx* _draft_ctx = nullptr;                  // --draft-model: the draft model's context (owned here; the target context only refers to it)
    int _lp_top_n = -1; bool _lp_shaped = false; std::vector<flm_logprob> _lp;
    bool _stop_set = false, _stop_installed = false; std::vector<int32_t> _stop_ids; std::vector<std::vector<int32_t>> _stop_seqs; std::vector<std::string> _stop_strs;
    int _stop_reason = -1, _stop_rule = 0;
    bool _dfa_set = false, _dfa_installed = false; std::vector<int32_t> _dfa_row, _dfa_tok, _dfa_nxt;
    bool _ent_set = false; flm_entropy _ent{};
    bool _shape_set = false; ShapeControls _shape; int _shape_last_n = 0; std::vector<int32_t> _bias_ids; std::vector<float> _bias_values;
};

} // namespace flmhost
