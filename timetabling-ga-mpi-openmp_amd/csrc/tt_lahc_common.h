// Device helpers shared by the late-acceptance kernels (tt_lahc.hip, tt_lahc_kempe.hip).
#pragma once
#include "tt_common.h"

namespace ttga {

constexpr int kStatusLahcBadGene = 256;     // tt_device_status bit 8
constexpr size_t kLahcMaxLds = 64 * 1024;

// one day's cost of a student: last slot of the day, windows of three, single class
__device__ __forceinline__ int lahc_day_cost(uint64_t m, int day) {
    const uint32_t d = (uint32_t)(m >> (9 * day)) & 0x1FFu;
    return (int)(d >> 8) + __popc(d & (d >> 1) & (d >> 2)) + (__popc(d) == 1);
}

// cost(m ^ flip) - cost(m) where flip has bits on days da and db only
__device__ __forceinline__ int lahc_mask_delta(uint64_t m, uint64_t flip, int da, int db) {
    const uint64_t n = m ^ flip;
    int d = lahc_day_cost(n, da) - lahc_day_cost(m, da);
    if (db != da) d += lahc_day_cost(n, db) - lahc_day_cost(m, db);
    return d;
}

__device__ __forceinline__ int lahc_uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }

}  // namespace ttga
