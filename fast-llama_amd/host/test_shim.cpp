// test_shim.cpp -- C entry points over the host-side classes so that tests/ can drive them through ctypes
// (no GPU needed).  Built as lib/libflm_host.so next to the CLI; the CLI itself does not use it.
#include <math.h>
#include <stdint.h>
#include <stddef.h>
#include <string.h>

#include <string>

#include "flm_gpu.h"

#include "model_file.h"
#include "sampler.h"
#include "spec_draft.h"
#include "tokenizer.h"
#include "../csrc/flm_logf.h"

using namespace flmhost;

namespace { struct Handle { ModelFile mf; Tokenizer tok; Vocab vocab_copy; std::string err; }; thread_local std::string g_err; }

extern "C" {

const char* fh_last_error() { return g_err.c_str(); }

void* fh_open(const char* ckpt, const char* tknr, int file_type, int tokenizer_only) {
    Handle* h = new Handle();
    if (!load_model_file(ckpt ? ckpt : "", tknr ? tknr : "", (FileType)file_type, tokenizer_only != 0, false, h->mf, g_err)) { delete h; return nullptr; }
    h->tok.set_vocab(h->mf.vocab);
    return h;
}
void fh_close(void* p) { delete (Handle*)p; }

int fh_detect(const char* path) { return (int)detect_file_type(path, g_err); }

// dim, hidden_dim, n_layers, n_heads, n_kv_heads, vocab_size, max_seq_len, quant_type, quant_group_size
void fh_config(void* p, int* out9) {
    const Config& c = ((Handle*)p)->mf.cfg;
    int v[9] = {c.dim, c.hidden_dim, c.n_layers, c.n_heads, c.n_kv_heads, c.vocab_size, c.max_seq_len, c.quant_type, c.quant_group_size};
    memcpy(out9, v, sizeof(v));
}
int fh_n_tensors(void* p) { return (int)((Handle*)p)->mf.tensors.size(); }
// kind, layer, qtype, rows, cols
void fh_tensor(void* p, int i, int* out5, const void** values, const float** scales) {
    const HostTensor& t = ((Handle*)p)->mf.tensors[i];
    int v[5] = {t.kind, t.layer, t.qtype, t.rows, t.cols};
    memcpy(out5, v, sizeof(v)); *values = t.values; *scales = t.scales;
}
int fh_vocab_size(void* p) { return ((Handle*)p)->tok.vocab_size(); }
int fh_encode(void* p, const char* text, int add_bos, int* out, int cap) {
    auto v = ((Handle*)p)->tok.encode(text, add_bos != 0);
    int n = (int)v.size() < cap ? (int)v.size() : cap;
    memcpy(out, v.data(), n * sizeof(int));
    return (int)v.size();
}
int fh_decode(void* p, const int* toks, int n, char* out, int cap) {
    std::string s = ((Handle*)p)->tok.decode(std::vector<int>(toks, toks + n));
    int m = (int)s.size() < cap - 1 ? (int)s.size() : cap - 1;
    memcpy(out, s.data(), m); out[m] = 0;
    return (int)s.size();
}
int fh_decode_one(void* p, int tok, int prev, char* out, int cap) {
    std::string s = ((Handle*)p)->tok.decode(tok, prev);
    int m = (int)s.size() < cap - 1 ? (int)s.size() : cap - 1;
    memcpy(out, s.data(), m); out[m] = 0;
    return (int)s.size();
}
// n_draws samples from the same logits (copied per draw) with one sampler state
void fh_sample(int vocab, unsigned long long seed, const float* logits, float temperature, float topp, int n_draws, int* out) {
    Sampler s; s.build(vocab, seed);
    std::vector<float> l(vocab);
    for (int i = 0; i < n_draws; ++i) { memcpy(l.data(), logits, vocab * sizeof(float)); out[i] = s.sample(l.data(), temperature, topp); }
}
// one draw with the sampler state carried by the caller: *state in / out (the device sampler's contract)
int fh_sample_state(int vocab, unsigned long long* state, const float* logits, float temperature, float topp) {
    Sampler s; s.build(vocab, *state);
    std::vector<float> l(logits, logits + vocab);
    const int tok = s.sample(l.data(), temperature, topp);
    *state = s.state();
    return tok;
}
// the logit-shaping stage (sampler.h shape_logits) on one row: out[n]; the expected value of the device's k_shape_logits
void fh_shape(const float* logits, int n, float temperature, int top_k, float min_p, float repeat_penalty, float frequency_penalty, float presence_penalty,
              int n_bias, const int32_t* bias_ids, const float* bias_values, const int32_t* window, int n_window, float* out) {
    ShapeControls c;
    c.top_k = top_k; c.min_p = min_p; c.repeat_penalty = repeat_penalty; c.frequency_penalty = frequency_penalty; c.presence_penalty = presence_penalty;
    c.n_bias = n_bias; c.bias_ids = bias_ids; c.bias_values = bias_values;
    shape_logits(logits, n, temperature, c, window, n_window, out);
}
// step 0 of the shaping definition (sampler.h constrain_logits) on one row: out[n]; the expected value of the device's mask
void fh_constrain(const float* logits, int n, const int32_t* tokens, int count, float* out) { constrain_logits(logits, n, tokens, count, out); }
// the automaton's transition (sampler.h dfa_next)
int fh_dfa_next(const int32_t* row_ptr, const int32_t* edge_token, const int32_t* edge_next, int q, int t) { return dfa_next(row_ptr, edge_token, edge_next, q, t); }
// flm_score (include/flm_gpu.h) of one row of logits, in plain C++: sample_argmax (sampler.cpp:36-47) and the sampler's clipped softmax (tf_operators.cpp:188-209) at
// temperature 1, read at `target` (-1: none) -- libm expf, a sequential fp32 sum in index order, prob = e_target * (float)(1.0 / sum).  out5: {argmax, target_logit,
// max_logit, sum, prob} as 32-bit words (the struct's layout).  The expected value of the device's k_score_rows.
void fh_score_row(const float* x, int n, int target, void* out5) {
    int arg = 0; float mx = x[0];
    for (int i = 1; i < n; ++i) if (x[i] > mx) { mx = x[i]; arg = i; }
    float sum = 0.0f, et = 0.0f;
    for (int i = 0; i < n; ++i) {
        const float d = x[i] - mx;
        const float e = d < -15 ? 0.0f : expf(d);
        if (!(d < -15)) sum += e;
        if (i == target) et = e;
    }
    struct { int32_t argmax; float target_logit, max_logit, sum, prob; } r{arg, 0.0f, mx, sum, 0.0f};
    if (target >= 0 && target < n) { r.target_logit = x[target]; r.prob = et * (float)(1. / sum); }
    memcpy(out5, &r, sizeof r);
}
// flm_logprob (include/flm_gpu.h) of one row with drawn id `chosen` (sampler.h logprob_row): out = the 192-byte struct; the expected value of the device's k_logprob_rows
void fh_logprob_row(const float* x, int n, int chosen, int top_n, void* out) {
    LogprobRecord r; logprob_row(x, n, chosen, top_n, &r);
    memcpy(out, &r, sizeof r);
}
// the C struct's layout as the compiler sees it (include/flm_gpu.h): {sizeof, offsets of token, logit, max_logit, sum, n_top, top_id, top_logit, pad_}
void fh_logprob_layout(int* out9) {
    const int v[9] = {(int)sizeof(flm_logprob), (int)offsetof(flm_logprob, token), (int)offsetof(flm_logprob, logit), (int)offsetof(flm_logprob, max_logit), (int)offsetof(flm_logprob, sum),
                      (int)offsetof(flm_logprob, n_top), (int)offsetof(flm_logprob, top_id), (int)offsetof(flm_logprob, top_logit), (int)offsetof(flm_logprob, pad_)};
    memcpy(out9, v, sizeof v);
}
// flm_logf (csrc/flm_logf.h) as the host compiles it: x[n] in place; the expected value of the device's flm_op_logf
void fh_logf(float* x, size_t n) { for (size_t i = 0; i < n; ++i) x[i] = flm_logf(x[i]); }
// the entropy-driven stages (sampler.h entropy_logits) on one row: out[n], returns how many live entries were dropped; the expected value of the device's entropy_row
int fh_entropy(const float* logits, int n, float temperature, float typical_p, int mirostat, float mu, float* out) {
    return entropy_logits(logits, n, temperature, typical_p, mirostat, mu, out);
}
// Mirostat's update behind the draw of id t from the masked row (sampler.h mirostat_update): returns the new mu, *obs the observed surprise
float fh_mirostat_update(const float* masked, int n, float temperature, int t, float tau, float eta, float mu, float* obs) {
    return mirostat_update(masked, n, temperature, t, tau, eta, mu, obs);
}
// the prompt-lookup drafter of flm_generate_lookup (spec_draft.h): h[n] -> d[k]; the expected value of the device's k_spec_draft
void fh_spec_draft(const int32_t* h, int n, int k, int ngram_max, int32_t* d) { spec_draft(h, n, k, ngram_max, d); }
void fh_quantize(const float* x, size_t n, int qtype, void* q, float* scales) { quantize_groups(x, n, qtype, q, scales); }

}
