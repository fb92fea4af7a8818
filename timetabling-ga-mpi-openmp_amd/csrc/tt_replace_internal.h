// What tt_ga.hip's replacement shares with a replacement of another kind
// (tt_unique.hip): the u64 key sorts, the survivors-in-order check, the layout
// of the work buffer and the row movers. The kernels live in tt_ga.hip; this
// header declares their host launchers and holds the small device helpers
// both files inline.
#pragma once
#include "tt_internal.h"

namespace ttga {

constexpr int kSortTile = 8192;      // keys one workgroup sorts in LDS / registers
constexpr int kRankTile = 256;       // tile of the tiles + ranks sort
constexpr int kPrepBlocks = 64;      // workgroups checking the survivors' order

inline int pow2_at_least(int n) {
    int p = 1;
    while (p < n) p <<= 1;
    return p;
}

inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

// (penalty, position) as one u64; penalties compare as unsigned, so the -1 of an
// invalid genome (tt_eval's sentinel; valid penalties are >= 0) sorts last
__device__ __forceinline__ uint64_t sort_key(int32_t penalty, int pos) {
    return ((uint64_t)(uint32_t)penalty << 32) | (uint32_t)pos;
}

// every workgroup's flag set (call with blockDim >= kPrepBlocks, every thread)
__device__ __forceinline__ bool survivors_sorted(const int32_t* flag) {
    return __syncthreads_and(threadIdx.x < kPrepBlocks ? flag[threadIdx.x] != 0 : true);
}

// full bitonic sort of keys[0..NP) (NP a power of two) by one workgroup in global
// memory (keys, 8 B each, stay L2-resident); every thread calls it, behind a
// barrier that made the keys visible, and leaves behind one
__device__ __forceinline__ void bitonic_global(uint64_t* __restrict__ keys, int NP) {
    for (int k = 2; k <= NP; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int q = threadIdx.x; q < NP / 2; q += blockDim.x) {
                const int i = ((q & ~(j - 1)) << 1) | (q & (j - 1)), l = i + j;
                const uint64_t x = keys[i], y = keys[l];
                if ((x > y) == ((i & k) == 0)) { keys[i] = y; keys[l] = x; }
            }
            __threadfence_block();
            __syncthreads();
        }
}

// copy two rows of E bytes (slot and room), 512 bytes per lane block with all
// loads in flight before the stores
__device__ __forceinline__ void copy_rows2(uint8_t* __restrict__ d0, const uint8_t* __restrict__ s0,
                                           uint8_t* __restrict__ d1, const uint8_t* __restrict__ s1, int E,
                                           int lane) {
    for (int e0 = 0; e0 < E; e0 += 512) {
        uint8_t a[8], b[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int e = e0 + 64 * k + lane;
            a[k] = e < E ? s0[e] : 0;
            b[k] = e < E ? s1[e] : 0;
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int e = e0 + 64 * k + lane;
            if (e < E) { d0[e] = a[k]; d1[e] = b[k]; }
        }
    }
}

// ascending sort of NP (a power of two) u64 keys on stream st, in place
void sort_keys(uint64_t* keys, int NP, hipStream_t st);
// NP keys in [2*kRankTile, kSortTile]: sorted by tiles + ranks, in two steps:
// sort_rank_tiles sorts the tiles in place, then a kernel that counts every
// key's rank writes the result (rank_scatter: the sorted copy `out`)
bool use_rank_sort(int NP);
void sort_rank_tiles(uint64_t* keys, int NP, hipStream_t st);
void rank_scatter(const uint64_t* keys, int NP, uint64_t* out, hipStream_t st);

// The parts of tt_ga_replace's work buffer (tt_ga_work_bytes(N, E)) that a
// replacement of another kind shares: sort keys [pow2(N)], the gathered rows
// and meta, the source word (tt_ga_work_source_offset) and the merged keys [N]
struct GaWork {
    uint64_t* keys;
    uint8_t *ws, *wr;
    int32_t *wm, *source;
    uint64_t* mkeys;
};
GaWork ga_work_layout(void* work, int N, int E);

// the work rows and meta (GaWork ws, wr, wm) back into the population, N workgroups
void replace_scatter(int E, int N, const GaWork& w, uint8_t* ps, uint8_t* pr, int32_t* ph, int32_t* psc, uint8_t* pf,
                     int32_t* pp, hipStream_t st);

}  // namespace ttga
