// Placement helpers shared by the greedy constructive population (tt_greedy.hip)
// and the guided crossover (tt_cx.hip): one wave per individual, lane t = slot t.
#pragma once
#include <climits>

#include "tt_common.h"

namespace ttga {

constexpr int kGreedyRegWords = 7;      // E <= 448: a slot's event bitset is 7 x 64 bits of its lane's registers
constexpr int kGreedyWaves = 4;         // individuals (waves) per workgroup on that path

// Full-wave minimum (every lane active), the DPP pattern of wave_sum: a lane
// without a source keeps its own value.
__device__ __forceinline__ int wave_min(int v) {
    v = min(v, __builtin_amdgcn_update_dpp(v, v, 0x111, 0xf, 0xf, false));   // row_shr:1
    v = min(v, __builtin_amdgcn_update_dpp(v, v, 0x112, 0xf, 0xf, false));   // row_shr:2
    v = min(v, __builtin_amdgcn_update_dpp(v, v, 0x114, 0xf, 0xf, false));   // row_shr:4
    v = min(v, __builtin_amdgcn_update_dpp(v, v, 0x118, 0xf, 0xf, false));   // row_shr:8
    v = min(v, __builtin_amdgcn_update_dpp(v, v, 0x142, 0xa, 0xf, false));   // row_bcast:15 (rows 1, 3)
    v = min(v, __builtin_amdgcn_update_dpp(v, v, 0x143, 0xc, 0xf, false));   // row_bcast:31 (rows 2, 3)
    return __builtin_amdgcn_readlane(v, 63);
}

// this wave's LDS writes are visible to its own later reads
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// The draws of one individual, 64 at a time: they do not depend on the
// placement, draw j is state * 16807^(j+1). The first step is pm_next's own (an
// out-of-range seed); lane l of batch b then holds the state of draw 64 b + l.
struct GreedyDraws {
    uint32_t base, lane_pow, pow64, st, last;
    __device__ __forceinline__ void init(int64_t seed, int lane) {
        pm_next(seed);
        base = (uint64_t)seed < (uint64_t)kPmM ? (uint32_t)seed : 0u;     // pm_mulmod needs < 2^31 - 1
        lane_pow = pm_pow(lane);
        pow64 = pm_pow(64);
        st = last = base;
    }
    // before draw j with j % 64 == 0
    __device__ __forceinline__ void next_batch() {
        st = pm_mulmod(base, lane_pow);
        base = pm_mulmod(base, pow64);
    }
    // (int)(next() * n) of draw j, as pm_pick: wave-uniform
    __device__ __forceinline__ int pick(int j, int n) {
        last = (uint32_t)__builtin_amdgcn_readlane((int)st, j & 63);
        const double u = __dmul_rn(1.0 / 2147483647.0, (double)last);
        const int k = (int)__dmul_rn(u, (double)n);
        return (unsigned)k < (unsigned)n ? k : 0;
    }
};

// Lane t (< 45) holds cost(t) = c; the slot of the event: T = the lanes at the
// minimum, the draw picks T[k]. Returns the slot (wave-uniform) and whether this
// lane is it.
__device__ __forceinline__ int greedy_choose(int c, int lane, GreedyDraws& d, int j, bool& mine) {
    if (lane >= kSlots) c = INT_MAX;
    const int m = wave_min(c);
    const bool tie = c == m;
    const uint64_t T = ballot(tie);
    const int k = d.pick(j, __popcll(T));
    mine = tie && __popcll(T & ((1ull << lane) - 1)) == k;
    return __builtin_ctzll(ballot(mine));
}

}  // namespace ttga
