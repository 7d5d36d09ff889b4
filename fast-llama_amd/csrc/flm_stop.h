// flm_stop.h -- stop rules on the device (include/flm_gpu.h flm_stop_rules): does the id a token's last act is about to publish end the call?  Part of
// flm_kernels.h; include that header.  No reference counterpart (the reference's loop ends on one id).  The host restatement is host/stop_rules.h stop_fires_at, which this
// equals index for index.
//
// The definition, over t[0 .. i], the ids THIS call has delivered up to and including the one just drawn (t[i] = tok): index i fires by id when tok is one of ids[0 .. n_ids)
// (rule: its lowest position), by sequence when some sequence s of length L <= i + 1 equals t[i - L + 1 .. i] (rule: the lowest such s); the id wins over the sequence.  The
// entry point's own stop token (kind 1) is not evaluated here: gen_last_act and the accept step compare it as they always have, and it wins over both.
//
// One function, stop_match, for the three places that ask: the token form (k_sample_advance, t[0 .. i) = out_tokens), the accept step of draft-and-verify
// (k_spec_accept_rules, t = the call's history behind the prompt followed by the verified run) and flm_op_stop_match.  It runs over the whole 1024-thread workgroup:
//   wave 0         lane p < n_ids compares ids[p] with tok; the wave's ballot is the id result, its lowest set bit the rule -- no memory involved
//   waves 1 .. 8   thread k of them owns sequence token k (at most 16 x 32 = 512): it finds its sequence s by a search over seq_ptr (17 words), and compares seq_tokens[k]
//                  with tok (the sequence's last position) or with t[i - L + 1 + j] (position j in front of it); a sequence with L > i + 1 reads nothing and counts as a
//                  mismatch.  A mismatch sets the thread's bit in its wave's 64-bit word in LDS (one ballot, one store per wave: nothing to initialise)
//   one barrier
//   wave 0         lane s < n_seqs reads the (at most two) words its sequence's bits [seq_ptr[s], seq_ptr[s + 1]) lie in: the sequence fires when they are all clear; the
//                  ballot's lowest set bit is the rule.  Every lane of wave 0 -- thread 0, which performs the last act, among them -- holds the result
// so the critical path of a token gains two loads, one barrier and a handful of scalar-rate instructions, not a serial scan of up to 576 words.  An empty block is one
// uniform load and a branch (stop_armed), a null pointer not even the load.
#pragma once
#include "flm_math.h"

namespace flm {

constexpr int kStopIdsMax = 64, kStopSeqsMax = 16, kStopSeqLenMax = 32;
constexpr int kStopTokMax = kStopSeqsMax * kStopSeqLenMax;
// the rule block in device memory (there since flm_ctx_create; flm_stop_set rewrites its contents): n_tok = seq_ptr[n_seqs]
struct StopBlock { int n_ids, n_seqs, n_tok, pad; int ids[kStopIdsMax]; int seq_ptr[kStopSeqsMax + 1]; int seq_tok[kStopTokMax]; };
constexpr int kStopLdsWords = 2 * (kStopTokMax / 64);       // the mismatch words of waves 1 .. 8, 64 bits each
struct StopHit { int kind; int rule; };                     // kind: 0 none, 2 an id, 3 a sequence (FLM_STOP_ID / FLM_STOP_SEQ)

// a uniform load through the constant address space and a scalar branch, like the latch (flm_math.h halted): the block is rewritten by flm_stop_set only, behind a
// synchronise and in front of the next call's first launch
__device__ __forceinline__ bool stop_armed(const StopBlock* sb) {
    typedef const int __attribute__((address_space(4))) CInt;
    if (sb == nullptr) return false;
    const CInt* w = (const CInt*)(unsigned long long)sb;
    return (w[0] | w[1]) != 0;
}

// Called by ALL threads of a 1024-thread workgroup with uniform arguments; contains one __syncthreads.  hist(j), 0 <= j < i: t[j] (called only for such j; the caller's
// accessor keeps the read inside its buffer).  lds: kStopLdsWords words that nobody else touches until the caller's next barrier.  The result is valid in wave 0.
template <class H>
__device__ __forceinline__ StopHit stop_match(const StopBlock* sb, int tok, H hist, int i, unsigned* lds) {
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int n_ids = sb->n_ids, n_seqs = sb->n_seqs, n_tok = sb->n_tok;
    unsigned long long idm = 0ull;
    if (w == 0) idm = __ballot(lane < n_ids && lane < kStopIdsMax && sb->ids[lane] == tok);
    else if (w <= kStopTokMax / 64) {
        const int k = t - 64;
        bool miss = false;
        if (k < n_tok) {
            int s = 0;                                                    // the sequence that owns token k: seq_ptr[s] <= k < seq_ptr[s + 1]
#pragma unroll
            for (int b = kStopSeqsMax / 2; b > 0; b >>= 1) if (s + b < n_seqs && sb->seq_ptr[s + b] <= k) s += b;
            const int b0 = sb->seq_ptr[s], L = sb->seq_ptr[s + 1] - b0, j = k - b0;
            if (L > i + 1) miss = true;
            else {
                const int at = i - L + 1 + j;                             // in [0, i]
                miss = sb->seq_tok[k] != (at == i ? tok : hist(at));
            }
        }
        const unsigned long long m = __ballot(miss);
        if (lane == 0) { lds[2 * (w - 1)] = (unsigned)m; lds[2 * (w - 1) + 1] = (unsigned)(m >> 32); }
    }
    __syncthreads();
    StopHit hit{0, 0};
    if (w == 0) {
        bool fires = false;
        if (lane < n_seqs && lane < kStopSeqsMax) {
            const int b0 = sb->seq_ptr[lane], e0 = sb->seq_ptr[lane + 1], L = e0 - b0;       // 1 <= L <= 32: the bits span at most two words
            const int w0 = b0 >> 6, w1 = (e0 - 1) >> 6;
            const unsigned long long m0 = (unsigned long long)lds[2 * w0] | ((unsigned long long)lds[2 * w0 + 1] << 32);
            unsigned long long bits = m0 >> (b0 & 63);
            if (w1 != w0) {
                const unsigned long long m1 = (unsigned long long)lds[2 * w1] | ((unsigned long long)lds[2 * w1 + 1] << 32);
                bits |= m1 << (64 - (b0 & 63));
            }
            fires = (bits & ((1ull << L) - 1ull)) == 0ull;
        }
        const unsigned long long sm = __ballot(fires);
        if (idm) { hit.kind = 2; hit.rule = __ffsll((long long)idm) - 1; }
        else if (sm) { hit.kind = 3; hit.rule = __ffsll((long long)sm) - 1; }
    }
    return hit;
}

// flm_op_stop_match: the first index of ids[0 .. n) that fires, by the function above index after index.  res = {first, kind, rule}; first = n, kind = rule = 0 if none.
// stop_tok: the entry point's own stop token (-1: none), kind 1, which wins.  One workgroup of 1024 threads.  The mismatch words alternate between two sets, so one
// barrier per index suffices (a set is rewritten two barriers after it was read)
inline __global__ void __launch_bounds__(1024) k_op_stop_match(const StopBlock* sb, const int* __restrict__ ids, int n, int stop_tok, int* res) {
    __shared__ unsigned lds[2][kStopLdsWords];
    int first = n, kind = 0, rule = 0;
    const bool armed = stop_armed(sb);
    for (int i = 0; i < n; ++i) {
        const int tok = ids[i];
        StopHit h{0, 0};
        if (armed) h = stop_match(sb, tok, [&](int j) { return ids[j]; }, i, lds[i & 1]);
        if (tok == stop_tok) { h.kind = 1; h.rule = 0; }
        if (first == n && h.kind != 0) { first = i; kind = h.kind; rule = h.rule; }       // (valid in wave 0; thread 0 writes)
    }
    if (threadIdx.x == 0) { res[0] = first; res[1] = kind; res[2] = rule; }
}

} // namespace flm
