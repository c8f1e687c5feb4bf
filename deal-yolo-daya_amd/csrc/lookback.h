// lookback.h — the decoupled look-back of the single-pass scans: K7's three tile kernels and K8's two banded-resolve passes.
//
// state[0] = ticket counter, state[1] = error word, state[2 + t] = look-back word of tile t: flag in bits 62..63, value below.
// A workgroup takes its tile from the ticket counter, so every tile before it is held by a running or finished workgroup
// whatever order the hardware dispatches workgroups in; a tile publishes its own aggregate without waiting for anything, so
// waiting for the words of the tiles before it cannot deadlock.  The words are written and polled with agent-scope relaxed
// atomics: a word carries its whole message, nothing else is read on the strength of it.
#pragma once

#include "dyd_common.h"

namespace dyd {

constexpr unsigned long long LB_AGG = 1ull << 62;        // the word holds the tile's own aggregate
constexpr unsigned long long LB_PFX = 2ull << 62;        // the word holds the inclusive prefix up to this tile
constexpr unsigned long long LB_VALUE = (1ull << 62) - 1;
constexpr int LB_SPIN_LIMIT = 1 << 22;                   // polls before a tile gives up (sets the error word)

// tile t's word: flag | value, value < 2^62 (tile 0 publishes its aggregate as LB_PFX: it is its own prefix)
__device__ __forceinline__ void lookback_publish(unsigned long long *state, int64_t tile, unsigned long long flag,
                                                 unsigned long long value) {
    __hip_atomic_store(&state[2 + tile], flag | value, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Called by the workgroup's first wave: the sum of the aggregates of every tile before `tile`, the same in all lanes.  Lane l
// polls the word of tile look - l; the nearest lane that holds a prefix ends the walk.  A spin that times out sets the error
// word to 1 (lane 0) and gives 0.
__device__ __forceinline__ unsigned long long lookback_sum(unsigned long long *state, int64_t tile, int lane) {
    const unsigned long long *words = state + 2;
    unsigned long long base = 0;
    int64_t look = tile - 1;      // nearest tile not yet accounted for
    bool failed = false;
    while (look >= 0) {
        const int64_t t = look - lane;
        unsigned long long wv = LB_PFX;   // lanes before tile 0 read as an empty prefix
        if (t >= 0) {
            int spins = 0;
            do {
                wv = __hip_atomic_load(&words[t], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if ((wv >> 62) == 0 && ++spins > LB_SPIN_LIMIT) {
                    failed = true;
                    break;
                }
                if ((wv >> 62) == 0) __builtin_amdgcn_s_sleep(1);
            } while ((wv >> 62) == 0);
        }
        if (__any(failed)) {
            failed = true;
            break;
        }
        const unsigned long long has_pfx = __ballot((wv >> 62) == 2);
        const int first = has_pfx ? __ffsll((long long)has_pfx) - 1 : kWave;   // nearest lane holding a prefix
        unsigned long long part = (lane <= first) ? (wv & LB_VALUE) : 0ull;
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) part += __shfl_xor(part, d);
        base += part;
        if (has_pfx) break;
        look -= kWave;
    }
    if (failed) {
        if (lane == 0) atomicExch(&state[1], 1ull);
        base = 0;
    }
    return base;
}

}  // namespace dyd
