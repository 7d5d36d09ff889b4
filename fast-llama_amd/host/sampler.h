// sampler.h -- llama2.c style sampler with the reference's exact arithmetic (src/transformer/sampler.cpp):
// argmax at temperature 0, otherwise temperature scaling, the reference's clipped softmax
// (src/blas/tf_operators.cpp:188-209), xorshift* coin and multinomial / top-p selection.
#pragma once
#include <stdint.h>

#include <vector>

namespace flmhost {

class Sampler {
public:
    void build(int vocab_size, uint64_t seed) { _n = vocab_size; _state = seed; _idx.resize(vocab_size); }
    int sample(float* logits, float temperature, float topp);     // modifies logits in place, like the reference
    // the xorshift state: the device sampler (flm_forward_sample / flm_decode_sample) draws from it and hands it back
    uint64_t state() const { return _state; }
    void set_state(uint64_t s) { _state = s; }
private:
    struct PI { float prob; int index; };
    float coin();
    int _n = 0;
    uint64_t _state = 0;      // seed 0 (the CLI default, transformer.cpp:40) keeps the state at 0: coin == 0 forever
    std::vector<PI> _idx;
};

// The logit-shaping stage in front of Sampler::sample (include/flm_gpu.h, flm_sampling): a plain sequential restatement of its definition -- bias, penalties over the
// DISTINCT ids of the window, top-k (larger value first, equal values by lower index), min-p in the logit domain with glibc's logf -- that the device's k_shape_logits
// (csrc/flm_shape.h) equals bit for bit.  S[n] <- the shaped L[n]; a stage whose control is neutral writes nothing.  The arguments are taken as valid: the C ABI checks them, and so does GpuTransformer::generate before its host loop calls this.
struct ShapeControls {
    int top_k = 0; float min_p = 0.f;
    float repeat_penalty = 1.f, frequency_penalty = 0.f, presence_penalty = 0.f;
    int n_bias = 0; const int32_t* bias_ids = nullptr; const float* bias_values = nullptr;
    bool neutral() const { return top_k <= 0 && min_p <= 0.f && repeat_penalty == 1.f && frequency_penalty == 0.f && presence_penalty == 0.f && n_bias == 0; }
};
void shape_logits(const float* L, int n, float temperature, const ShapeControls& c, const int32_t* window, int n_window, float* S);

// Constrained decoding (include/flm_gpu.h, flm_dfa): step 0 of the shaping definition and the automaton's transition, restated sequentially; the device's mask
// (csrc/flm_shape.h) equals constrain_logits bit for bit.
// S[n] <- L[n] with -inf at every index that is not one of tokens[0 .. count) (the edge list of the armed state: ascending ids in [0, n)).  S may be L
void constrain_logits(const float* L, int n, const int32_t* tokens, int count, float* S);
// delta(q, t) over a CSR automaton: the edge_next of t's edge in state q, or q itself when t has no edge there (reachable only through Sampler::sample's last-index
// fallback, `return _n - 1` in its multinomial branch, which can name a masked id)
int dfa_next(const int32_t* row_ptr, const int32_t* edge_token, const int32_t* edge_next, int q, int t);

// The record of one drawn token (include/flm_gpu.h, flm_logprob): a plain sequential restatement of its definition that the device's logprob_row (csrc/flm_logprob.h)
// equals element for element.  R[n], n >= 2, chosen in [0, n), top_n in [0, kLogprobsMax]; the struct is flm_logprob's layout, 192 bytes
constexpr int kLogprobsMax = 20;
struct LogprobRecord { int32_t token; float logit, max_logit, sum; int32_t n_top; int32_t top_id[kLogprobsMax]; float top_logit[kLogprobsMax]; int32_t pad_[3]; };
static_assert(sizeof(LogprobRecord) == 192, "flm_logprob is 192 bytes");
void logprob_row(const float* R, int n, int chosen, int top_n, LogprobRecord* out);

// The entropy-driven stages behind the shaping stage (include/flm_gpu.h, flm_entropy): a plain sequential restatement of their definition that the
// device's entropy_row (csrc/flm_entropy.h) equals bit for bit.  R[n] is the row the sampler is about to read, S[n] <- R with -inf at every live entry the stage drops
// (S may be R).  Statistics: y = R / T, d = y - max y, e = d < -15 ? 0 : expf(d), sum and H sequential in index order, p = e * (float)(1. / sum), surprise a = flm_logf(sum) - d
// (csrc/flm_logf.h).  Dead entries (e == 0) are never candidates and stay as they are.
//   typical_p in (0, 1): stage 5 -- the live entries ordered by |a - H| ascending (equal keys by index), kept up to and including the first at which the running sum of p
//                        passes typical_p
//   mirostat == 2:       stage 6 -- a live entry stays iff a * 1.44269504f <= mu; the first maximum always stays
// T == 0, or neither set: S = R.  Returns how many live entries were dropped.  The arguments are taken as valid (never both stages): the C ABI checks them
int entropy_logits(const float* R, int n, float temperature, float typical_p, int mirostat, float mu, float* S);
// Mirostat's state behind the draw of id t from the MASKED row S (at topp = 1): obs = (flm_logf(sum') - d[t]) * 1.44269504f with sum' the sequential sum over the masked
// row, then mu - eta * (obs - tau) in three operations.  *obs_out (may be null): obs
float mirostat_update(const float* S, int n, float temperature, int t, float tau, float eta, float mu, float* obs_out);

} // namespace flmhost
