#include "sampler.h"
#include "../csrc/flm_logf.h"

#include <math.h>
#include <stdlib.h>

#include <algorithm>
#include <numeric>

namespace flmhost {

float Sampler::coin() {
    _state ^= _state >> 12; _state ^= _state << 25; _state ^= _state >> 27;
    const uint32_t r = (uint32_t)((_state * 0x2545F4914F6CDD1Dull) >> 32);
    return (r >> 8) / 16777216.0f;
}

static int argmax(const float* p, int n) {
    int bi = 0; float bv = p[0];
    for (int i = 1; i < n; ++i) if (p[i] > bv) { bv = p[i]; bi = i; }
    return bi;
}

// cpuft::softmax (tf_operators.cpp:188-209): exp(x - max) with x - max < -15 clamped to 0, then scaled by 1/sum
static void clipped_softmax(float* x, int n) {
    float mx = x[0];
    for (int i = 1; i < n; ++i) if (x[i] > mx) mx = x[i];
    float sum = 0.f;
    for (int i = 0; i < n; ++i) {
        const float d = x[i] - mx;
        if (d < -15) x[i] = 0.f; else { x[i] = expf(d); sum += x[i]; }      // d <= 0 always, so the d >= 6 table branch never fires
    }
    const float inv = (float)(1. / sum);
    for (int i = 0; i < n; ++i) x[i] *= inv;
}

int Sampler::sample(float* logits, float temperature, float topp) {
    if (temperature == 0.0f) return argmax(logits, _n);
    for (int i = 0; i < _n; ++i) logits[i] /= temperature;
    clipped_softmax(logits, _n);
    const float c = coin();
    if (topp <= 0 || topp >= 1) {
        float cdf = 0.f;
        for (int i = 0; i < _n; ++i) { cdf += logits[i]; if (c < cdf) return i; }
        return _n - 1;
    }
    int n0 = 0;
    const float cutoff = (1.0f - topp) / (_n - 1);
    for (int i = 0; i < _n; ++i) if (logits[i] >= cutoff) { _idx[n0].index = i; _idx[n0].prob = logits[i]; ++n0; }
    qsort(_idx.data(), n0, sizeof(PI), [](const void* a, const void* b) {
        const float pa = ((const PI*)a)->prob, pb = ((const PI*)b)->prob; return pa > pb ? -1 : pa < pb ? 1 : 0; });
    float cum = 0.f; int last = n0 - 1;
    for (int i = 0; i < n0; ++i) { cum += _idx[i].prob; if (cum > topp) { last = i; break; } }
    const float r = c * cum;
    float cdf = 0.f;
    for (int i = 0; i <= last; ++i) { cdf += _idx[i].prob; if (r < cdf) return _idx[i].index; }
    return _idx[last].index;
}

void shape_logits(const float* L, int n, float temperature, const ShapeControls& c, const int32_t* window, int n_window, float* S) {
    for (int i = 0; i < n; ++i) S[i] = L[i];
    // 1: bias
    for (int i = 0; i < c.n_bias; ++i) S[c.bias_ids[i]] = S[c.bias_ids[i]] + c.bias_values[i];
    // 2: penalties, once per distinct id of the window
    const bool rep = c.repeat_penalty != 1.0f, fpp = c.frequency_penalty != 0.0f || c.presence_penalty != 0.0f;
    if (n_window > 0 && (rep || fpp)) {
        for (int j = 0; j < n_window; ++j) {
            const int t = window[j];
            int count = 0; bool first = true;
            for (int k = 0; k < n_window; ++k) if (window[k] == t) { ++count; if (k < j) first = false; }
            if (!first) continue;
            float x = S[t];
            if (rep) x = x > 0.0f ? x / c.repeat_penalty : x * c.repeat_penalty;
            if (fpp) x = x - ((float)count * c.frequency_penalty + c.presence_penalty);
            S[t] = x;
        }
    }
    // 3: top-k
    if (c.top_k > 0 && c.top_k < n) {
        std::vector<int> idx(n);
        std::iota(idx.begin(), idx.end(), 0);
        std::stable_sort(idx.begin(), idx.end(), [&](int a, int b) { return S[a] > S[b]; });
        for (int r = c.top_k; r < n; ++r) S[idx[r]] = -INFINITY;
    }
    // 4: min-p
    if (c.min_p > 0.0f && temperature != 0.0f) {
        const float lt = logf(c.min_p);
        float mx = -INFINITY;
        for (int i = 0; i < n; ++i) if (S[i] != -INFINITY) { const float y = S[i] / temperature; if (y > mx) mx = y; }
        for (int i = 0; i < n; ++i) if (S[i] != -INFINITY) { const float y = S[i] / temperature; if (y - mx < lt) S[i] = -INFINITY; }
    }
}

void constrain_logits(const float* L, int n, const int32_t* tokens, int count, float* S) {
    int e = 0;
    for (int i = 0; i < n; ++i) {
        while (e < count && tokens[e] < i) ++e;
        S[i] = (e < count && tokens[e] == i) ? L[i] : -INFINITY;
    }
}

int dfa_next(const int32_t* row_ptr, const int32_t* edge_token, const int32_t* edge_next, int q, int t) {
    for (int e = row_ptr[q]; e < row_ptr[q + 1]; ++e) if (edge_token[e] == t) return edge_next[e];
    return q;
}

void logprob_row(const float* R, int n, int chosen, int top_n, LogprobRecord* out) {
    LogprobRecord r{};
    // flm_score's statistics at temperature 1: the first maximum, the clipped exponentials (libm expf), their sequential sum in index order
    float mx = R[0];
    for (int i = 1; i < n; ++i) if (R[i] > mx) mx = R[i];
    float sum = 0.0f;
    for (int i = 0; i < n; ++i) {
        const float d = R[i] - mx;
        if (!(d < -15)) sum += expf(d);
    }
    r.token = chosen; r.logit = R[chosen]; r.max_logit = mx; r.sum = sum;
    // the first n_top indices in "larger value, equal values by lower index" (float comparison: -0.0 ties +0.0; -inf takes part): a stable selection -- the indices arrive in
    // ascending order, and one enters the list only in front of strictly smaller values
    const int K = std::min(std::min(std::max(top_n, 0), kLogprobsMax), n);
    int m = 0;
    for (int i = 0; i < n && K > 0; ++i) {
        const float x = R[i];
        if (m == K && !(x > R[r.top_id[K - 1]])) continue;
        int j = m < K ? m : K - 1;                      // the slot that opens: the list's end, or its last entry falls out
        while (j > 0 && x > R[r.top_id[j - 1]]) { r.top_id[j] = r.top_id[j - 1]; --j; }
        r.top_id[j] = i;
        if (m < K) ++m;
    }
    r.n_top = K;
    for (int j = 0; j < K; ++j) r.top_logit[j] = R[r.top_id[j]];
    *out = r;
}

namespace {
// the statistics of a row at temperature T: d[n], e[n]; returns the sequential sum
struct RowStats { std::vector<float> d, e; float sum = 0.f; int first_max = 0; };
void row_stats(const float* R, int n, float T, RowStats& s) {
    s.d.resize(n); s.e.resize(n);
    for (int i = 0; i < n; ++i) s.d[i] = R[i] / T;
    float mx = s.d[0]; s.first_max = 0;
    for (int i = 1; i < n; ++i) if (s.d[i] > mx) { mx = s.d[i]; s.first_max = i; }
    float sum = 0.f;
    for (int i = 0; i < n; ++i) {
        const float d = s.d[i] - mx;
        s.d[i] = d;
        s.e[i] = d < -15 ? 0.f : expf(d);
        sum += s.e[i];
    }
    s.sum = sum;
}
}

int entropy_logits(const float* R, int n, float T, float typical_p, int mirostat, float mu, float* S) {
    if (S != R) for (int i = 0; i < n; ++i) S[i] = R[i];
    const bool typ = typical_p > 0.0f && typical_p < 1.0f, miro = mirostat == 2;
    if (T == 0.0f || !(typ || miro)) return 0;
    RowStats st; row_stats(R, n, T, st);
    const float ls = flm_logf(st.sum);
    int dropped = 0;
    if (miro) {
        for (int i = 0; i < n; ++i) {
            if (st.e[i] == 0.f || i == st.first_max) continue;
            const float a = ls - st.d[i];
            if (!(a * 1.44269504f <= mu)) { S[i] = -INFINITY; ++dropped; }
        }
        return dropped;
    }
    const float inv = (float)(1. / st.sum);
    std::vector<float> p(n), key(n);
    float H = 0.f;
    for (int i = 0; i < n; ++i) {
        p[i] = st.e[i] * inv;
        const float h = st.e[i] == 0.f ? 0.f : p[i] * (ls - st.d[i]);
        H += h;
    }
    std::vector<int> idx;
    for (int i = 0; i < n; ++i) if (st.e[i] != 0.f) { key[i] = fabsf((ls - st.d[i]) - H); idx.push_back(i); }
    std::stable_sort(idx.begin(), idx.end(), [&](int a, int b) { return key[a] < key[b]; });
    float c = 0.f; size_t last = idx.size();
    for (size_t j = 0; j < idx.size(); ++j) { c += p[idx[j]]; if (c > typical_p) { last = j; break; } }
    for (size_t j = last + 1; j < idx.size(); ++j) { S[idx[j]] = -INFINITY; ++dropped; }
    return dropped;
}

float mirostat_update(const float* S, int n, float T, int t, float tau, float eta, float mu, float* obs_out) {
    RowStats st; row_stats(S, n, T, st);
    const float obs = (flm_logf(st.sum) - st.d[t]) * 1.44269504f;
    if (obs_out) *obs_out = obs;
    const float err = obs - tau;
    const float step = eta * err;
    return mu - step;
}

} // namespace flmhost
