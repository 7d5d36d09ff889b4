// stop_rules.h -- the stop rules of include/flm_gpu.h (flm_stop_rules) in plain C++, written as the definition reads: the ONE host implementation behind flm_stop_match /
// flm_stop_validate and flm_query "stop_reason" (csrc/flm_calls.hip includes this file).  The device's matcher (csrc/flm_stop.h) equals stop_fires_at index for index.
// It stands next to sampler.cpp's other restatements (constrain_logits, dfa_next) as a header, because the library does not link host/sampler.cpp.  The CLI does not call
// it: bin/main runs rules on the device path only and reads the finish reason through flm_query; a caller with a loop of its own reaches it through flm_stop_match.
#pragma once
#include <stdint.h>

#include "flm_gpu.h"

namespace flmhost {

// the rules of flm_stop_validate: null, or which one is broken
inline const char* stop_check(const flm_stop_rules* r, int vocab) {
    if (!r) return "stop: null struct";
    if (vocab < 1) return "stop: vocab < 1";
    if (r->n_ids < 0 || r->n_ids > FLM_STOP_IDS_MAX) return "stop: n_ids outside [0, FLM_STOP_IDS_MAX]";
    if (r->n_seqs < 0 || r->n_seqs > FLM_STOP_SEQS_MAX) return "stop: n_seqs outside [0, FLM_STOP_SEQS_MAX]";
    if (r->n_ids > 0 && !r->ids) return "stop: null ids";
    if (r->n_seqs > 0 && (!r->seq_ptr || !r->seq_tokens)) return "stop: null seq_ptr or seq_tokens";
    for (int i = 0; i < r->n_ids; ++i) {
        if (r->ids[i] < 0 || r->ids[i] >= vocab) return "stop: id outside [0, vocab)";
        for (int k = 0; k < i; ++k) if (r->ids[k] == r->ids[i]) return "stop: an id is listed twice";
    }
    if (r->n_seqs > 0 && r->seq_ptr[0] != 0) return "stop: seq_ptr must start at 0";
    for (int s = 0; s < r->n_seqs; ++s) {
        const int L = r->seq_ptr[s + 1] - r->seq_ptr[s];
        if (L < 0) return "stop: seq_ptr is decreasing";
        if (L < 1 || L > FLM_STOP_SEQ_LEN_MAX) return "stop: sequence length outside [1, FLM_STOP_SEQ_LEN_MAX]";
    }
    for (int k = 0; r->n_seqs > 0 && k < r->seq_ptr[r->n_seqs]; ++k)
        if (r->seq_tokens[k] < 0 || r->seq_tokens[k] >= vocab) return "stop: sequence token outside [0, vocab)";
    return nullptr;
}

// does index i of t[0 .. n) fire (i < n)?  *kind: FLM_STOP_TOKEN (t[i] == stop_token, -1: none), FLM_STOP_ID (*rule: the lowest position in ids), FLM_STOP_SEQ (a direct
// suffix comparison per sequence, no automaton: sequence s of length L <= i + 1 with t[i - L + 1 .. i] == seq_s; *rule: the lowest such s), preferred in that order.
// r may be null; valid rules are the caller's business
inline bool stop_fires_at(const flm_stop_rules* r, int32_t stop_token, const int32_t* t, int i, int* kind, int* rule) {
    if (stop_token >= 0 && t[i] == stop_token) { *kind = FLM_STOP_TOKEN; *rule = 0; return true; }
    if (!r) return false;
    for (int p = 0; p < r->n_ids; ++p) if (r->ids[p] == t[i]) { *kind = FLM_STOP_ID; *rule = p; return true; }
    for (int s = 0; s < r->n_seqs; ++s) {
        const int b = r->seq_ptr[s], L = r->seq_ptr[s + 1] - b;
        if (L > i + 1) continue;
        bool same = true;
        for (int j = 0; j < L && same; ++j) same = r->seq_tokens[b + j] == t[i - L + 1 + j];
        if (same) { *kind = FLM_STOP_SEQ; *rule = s; return true; }
    }
    return false;
}

// the first index of t[0 .. n) that fires, or n (then *kind = FLM_STOP_LENGTH, *rule = 0)
inline int stop_match(const flm_stop_rules* r, int32_t stop_token, const int32_t* t, int n, int* kind, int* rule) {
    for (int i = 0; i < n; ++i) if (stop_fires_at(r, stop_token, t, i, kind, rule)) return i;
    *kind = FLM_STOP_LENGTH; *rule = 0;
    return n;
}

} // namespace flmhost
