// flm_wait.h -- everything a cross-workgroup / cross-rank wait is made of (part of flm_kernels.h; included by flm_gemv.h behind flm_math.h): when a flag line or a granule tag
// has reached its target, how long a wait is patient and what it does when it gives up, the one flag-line poll, the granule pieces.  What is polled, what is requested in front
// of a wait and the fences around it stay with the caller.
#pragma once
#include "flm_math.h"
#pragma clang fp contract(off)

namespace flm {

// ------------------------------------------------------------------------------------------
// Every cross-workgroup / cross-rank wait compares a flag line's value f with a target that counts from an epoch in device memory (TailArgs::epoch, the token's epoch base
// advanced by k_embed, k_xchg's per-kind counters) or, in the k_embed-era launches, with layer + 1 against lines k_embed cleared.  A line has reached its target when
// f - target (mod 2^32) lies in [0, kEpochWindow): values a producer of the SAME launch may already have moved on to lie a few hundred above the target at most, and everything
// stale -- the previous token's value (just below), a line k_embed cleared (0) or a k_embed-era launch left at layer + 1, a value from the counter's previous lap -- lies
// outside the window as long as the epochs stay inside [kEpochFirst, kEpochWrap + a token's stride): targets keep kEpochWindow away from both ends of the 32-bit range, and
// the counters go back to their first value at kEpochWrap (tail_phase, k_embed).  The signed form this replaces, (int)(f - target) >= 0, let a cleared line pass every target
// above 2^31 (tests/test_gpu_longlived.py ages a context there).  Granule tags compare by equality: a tag repeats after a whole lap of its counter, and every granule is
// rewritten every token.
// FLM_WAIT_FORM (experiment builds: the teeth of tests/test_gpu_longlived.py): 1 = the signed difference again, 2 = plain f >= target and tag >= target.
// ------------------------------------------------------------------------------------------
#ifndef FLM_WAIT_FORM
#define FLM_WAIT_FORM 0
#endif
constexpr unsigned kEpochWindow = 1u << 20;
constexpr unsigned kEpochFirst = 4096u;          // the one-launch token's first epoch: above anything a k_embed-era launch leaves in a line (layer + 1)
constexpr unsigned kEpochWrap = 0xFFE00000u;     // a counter that reaches this goes back to its first value: no target comes within kEpochWindow of 2^32
__device__ __forceinline__ bool flag_reached(const unsigned f, const unsigned target) {
#if FLM_WAIT_FORM == 1
    return (int)(f - target) >= 0;
#elif FLM_WAIT_FORM == 2
    return f >= target;
#else
    return f - target < kEpochWindow;
#endif
}
__device__ __forceinline__ bool tag_is(const unsigned t, const unsigned tag) {
#if FLM_WAIT_FORM == 2
    return t >= tag;
#else
    return t == tag;
#endif
}

constexpr int kFlagStride = 16;                  // dwords: one 64-byte flag line per producer
constexpr int kXchgSlots = 8;                    // tensor parallel, the exchange flags: slots 0..3 k_xchg's kinds (att, x1, hd, logits), 4..6 the folded exchanges (att, x1, hd)
constexpr int kXchgAbortLine = kXchgSlots * 8;   // flag line behind the [slot][8 ranks] lines: non-zero = some rank gave up, nobody waits any more

// ------------------------------------------------------------------------------------------
// The give-up policy.  All workgroups of a fused launch are resident (the census of flm_ctx_create), so a wait normally ends within microseconds; one that does not must end
// all the same.  Two patiences, in ticks of the 100 MHz real-time clock:
//   kPatienceLocal   20 ms, one GPU: *err = 1, the host re-runs the call on one kernel per phase
//   kPatienceRanks   20 s, across tensor-parallel ranks (they start seconds apart: module loading, graph capture): *err = 2, a group error (FLM_ERR_COMM; nothing is
//                    re-run on one rank alone) -- and where the group has an abort line, everybody leaves as soon as ANY rank has given up
// INVARIANT (why a token computed on garbage cannot be published, gen_last_act in flm_math.h): garbage exists only behind a wait that gave up, and the wave that gives up
// stores the error word -- at system scope: the host reads it -- BEFORE it leaves the wait and produces anything from what it failed to wait for.  Whatever it produces reaches
// the token's last act only through the later hand-offs of the token (flag rounds / granules / a kernel boundary), each of them an agent-scope store -> load chain behind that
// error store.  These two functions are the only stores to an error word.
// A single-GPU wait also looks at *err when it starts and runs through once another wait of the launch has given up: the host re-runs the call in either case, and a failed
// launch does not spend 20 ms per layer.  (The per-phase fused kernels k_attn_o / k_qkv_attn_o / k_ffn and the split heads' score exchange did not do that before they took
// poll_wave; results are the same, a failed launch ends sooner.)
// ------------------------------------------------------------------------------------------
constexpr unsigned long long kPatienceLocal = 2000000ull;
constexpr unsigned long long kPatienceRanks = 2000000000ull;
__device__ __forceinline__ bool give_up_local(const unsigned long long t0, int* err) {
    if (__builtin_amdgcn_s_memrealtime() - t0 <= kPatienceLocal) return false;
    __hip_atomic_store(err, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    return true;
}
// ab: the group's abort line as the caller's layout has it -- aborted(): has anybody given up?  raise(): tell every rank.  kEvery: a power of two, the looks between two checks
template <class Abort>
__device__ __forceinline__ bool give_up_ranks(const unsigned long long t0, int* err, const Abort& ab) {
    if (!ab.aborted() && __builtin_amdgcn_s_memrealtime() - t0 <= kPatienceRanks) return false;
    __hip_atomic_store(err, 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    ab.raise();
    return true;
}
struct NoAbortLine {                             // the per-phase kernels' heads / hd lines across ranks: patient, nobody to tell
    static constexpr unsigned kEvery = 1;
    __device__ __forceinline__ bool aborted() const { return false; }
    __device__ __forceinline__ void raise() const {}
};
// BackArgs::Tp (flm_layer.h, the rank-spanning k_layers): peer[r] + abort_off, looked at every 256 looks together with this rank's own error word; one lane raises all ranks' lines
template <class Args>
struct TpAbortLine {
    const Args& p;
    static constexpr unsigned kEvery = 256;
    __device__ __forceinline__ bool aborted() const {
        return __hip_atomic_load(p.tp.peer[p.tp.rank] + p.tp.abort_off, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) != 0 || __hip_atomic_load(p.err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0;
    }
    __device__ __forceinline__ void raise() const { for (int r = 0; r < p.tp.world; ++r) __hip_atomic_store(p.tp.peer[r] + p.tp.abort_off, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM); }
};
// GemvArgs::XchgFold / XchgArgs (xchg_fold, k_xchg): line kXchgAbortLine of the exchange flags, looked at every look; the thread whose line is rank r's raises rank r's abort line
template <class Args>
struct XchgAbortLine {
    const Args& x; const int r;
    static constexpr unsigned kEvery = 1;
    __device__ __forceinline__ bool aborted() const { return __hip_atomic_load(x.local_flags + kXchgAbortLine * kFlagStride, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) != 0; }
    __device__ __forceinline__ void raise() const { if (r < x.world) __hip_atomic_store(x.peer_flags[r] + kXchgAbortLine * kFlagStride, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM); }
};

// ------------------------------------------------------------------------------------------
// The flag-line poll: one wave's look at its lines (lane i: `line`, if `mine`) until all have reached `target`.  A look is a round trip to memory (the lines are written and read
// across XCDs); one look is in flight at a time (three in flight took 0.2 .. 0.3 us off a short-context layer and added 1.6 us to a long-context one, tools/variants.sh).
// SCOPE of the look: agent on one GPU, system where peer GPUs write the lines.  RANKS: the patience (above).  NAP: s_sleep units (64 cycles) between two looks across ranks.
// ------------------------------------------------------------------------------------------
template <int SCOPE = __HIP_MEMORY_SCOPE_AGENT, bool RANKS = false, int NAP = 0, class Abort = NoAbortLine>
__device__ __forceinline__ void poll_wave(const unsigned* line, bool mine, unsigned target, int* err, const Abort& ab = Abort()) {
    const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
    auto look = [&]() -> unsigned { return mine ? __hip_atomic_load(line, __ATOMIC_RELAXED, SCOPE) : target; };
    if constexpr (!RANKS) {
        // (a wait of this launch has already given up: the host re-runs the call anyway; do not spend another 20 ms here -- the look at *err flies beside the first look at the lines;
        //  the clock is read while the next look is in flight)
        const int gave_up = __hip_atomic_load(err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        unsigned f = look();
        if (gave_up) return;
        while (true) {
            if (__all(flag_reached(f, target))) break;
            f = look();
            if (give_up_local(t0, err)) break;
        }
    } else {
        // (nothing hurries here: the abort line and the clock are looked at between two looks, then the nap)
        unsigned looks = 0;
        while (true) {
            if (__all(flag_reached(look(), target))) break;
            if (Abort::kEvery == 1 || (++looks & (Abort::kEvery - 1)) == 0u) { if (give_up_ranks(t0, err, ab)) break; }
            if constexpr (NAP > 0) __builtin_amdgcn_s_sleep(NAP);
        }
    }
}
// lane i (of the first 256 threads) polls line i of `n` lines until all have reached `target`
__device__ __forceinline__ void poll_lines(const unsigned* flag, int n, unsigned target, int* err) {
    if ((int)(threadIdx.x & ~63u) < n) poll_wave(flag + threadIdx.x * kFlagStride, (int)threadIdx.x < n, target, err);
}
// ---- the same across tensor-parallel ranks (layer_body<.., TP>; p: BackArgs): the lines are written by peer GPUs (system-scope stores into this rank's region)
template <class Args>
__device__ __forceinline__ void poll_wave_tp(const unsigned* line, bool mine, unsigned target, const Args& p) {
    poll_wave<__HIP_MEMORY_SCOPE_SYSTEM, true, 0>(line, mine, target, p.err, TpAbortLine<Args>{p});
}
// every thread takes the lines tid, tid + 1024, ... of `n` (<= 8 ranks x 256 workgroups); the caller's barrier follows
template <bool TP, class Args>
__device__ __forceinline__ void poll_lines_t(const unsigned* flag, int n, unsigned target, const Args& p) {
    if constexpr (!TP) poll_lines(flag, n, target, p.err);
    else {
        for (int b = 0; b < n; b += kGemvBlock) {
            const int i = b + (int)threadIdx.x;
            if ((i & ~63) < n) poll_wave_tp(flag + (size_t)i * kFlagStride, i < n, target, p);
        }
        if (p.tp.fence & 2) __atomic_thread_fence(__ATOMIC_ACQUIRE);
    }
}
// a producer workgroup's line goes up (its stores have completed: wait_stores_done + barrier in front): one local store, or one store into every rank's array
template <bool TP, class Args>
__device__ __forceinline__ void raise_line(const Args& p, unsigned* local, unsigned off, unsigned line, unsigned target) {
    if constexpr (!TP) { if (threadIdx.x == 0) __hip_atomic_store(local + line * kFlagStride, target, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    else if (threadIdx.x == 0) {
        if (p.tp.fence & 1) __atomic_thread_fence(__ATOMIC_RELEASE);
        for (int r = 0; r < p.tp.world; ++r) __hip_atomic_store(p.tp.peer[r] + off + line * kFlagStride, target, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// lane i of the QKV -> heads hand-off (layer_body's qwait, k_qkv_attn_o): does workgroup i of the nq that run [Wq; Wk; Wv] reduce a row of head h's q, k or v?
// (pass p = rows [p Rm, (p + 1) Rm) of the matrix, workgroup p mod nq; the head's rows start at h hs, dim + h hs, dim + kv_dim + h hs)
__device__ __forceinline__ bool qkv_line_needed(const unsigned i, const unsigned nq, const unsigned Rm, const unsigned hs, const unsigned h, const unsigned dim, const unsigned kv_dim) {
    bool need = false;
    if (i < nq) {
#pragma unroll
        for (int m = 0; m < 3; ++m) {
            const unsigned r0 = (m == 0 ? 0u : m == 1 ? dim : dim + kv_dim) + h * hs;
            const unsigned pa = r0 / Rm, pb = (r0 + hs - 1) / Rm;
            need |= (i + nq - pa % nq) % nq <= pb - pa;
        }
    }
    return need;
}

// ---- granule pieces (flm_gemv.h: granule_t = {value, tag}, 8 bytes): four consecutive granules = two 16-byte coherent loads (A, C) = {v0, t0, v1, t1}, {v2, t2, v3, t3}
typedef float v4f __attribute__((ext_vector_type(4)));
typedef unsigned v4u32 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void granules4_load(const __amdgpu_buffer_rsrc_t r, const int byte_off, v4u32& A, v4u32& C) {
    A = __builtin_bit_cast(v4u32, __builtin_amdgcn_raw_buffer_load_b128(r, byte_off, 0, kAuxCoherent));
    C = __builtin_bit_cast(v4u32, __builtin_amdgcn_raw_buffer_load_b128(r, byte_off + 16, 0, kAuxCoherent));
}
__device__ __forceinline__ bool granules4_tagged(const v4u32& A, const v4u32& C, const unsigned tag) { return tag_is(A.y, tag) && tag_is(A.w, tag) && tag_is(C.y, tag) && tag_is(C.w, tag); }
__device__ __forceinline__ v4f granules4_values(const v4u32& A, const v4u32& C) { return v4f{__uint_as_float(A.x), __uint_as_float(A.z), __uint_as_float(C.x), __uint_as_float(C.z)}; }

} // namespace flm
