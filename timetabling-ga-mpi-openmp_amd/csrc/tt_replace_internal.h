// What tt_ga_replace (tt_ga.hip) and tt_ga_replace_unique (tt_unique.hip) share:
// the u64 key sorts, the merge form (order check, merge path, fallback sort), the
// row movers and the carve of the work buffer. The kernels live in tt_ga.hip, once;
// the two callers differ in two data items, the child count (ChildCount) and the
// base of a child key's low word. This header declares the host launchers and
// holds the small device helpers of these steps.
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

// How many children a replacement merges in: a host value, or (word non-null) a
// device word written earlier on the stream (tt_ga_replace_unique's n_kept)
struct ChildCount {
    int value;
    const int32_t* word;
};
__device__ __forceinline__ int child_count(const ChildCount& c) { return c.word ? *c.word : c.value; }

// key i of the merged population: the survivors' (positions < k) and, behind them, ckeys
__device__ __forceinline__ uint64_t merged_key(const int32_t* __restrict__ pen, const uint64_t* __restrict__ ckeys,
                                               int N, int k, int i) {
    return i >= N ? ~0ull : i < k ? sort_key(pen[i], i) : ckeys[i - k];
}

// child keys are padded with ~0 to a power of two >= 2
inline int padded(int n) { return pow2_at_least(n > 2 ? n : 2); }

// Consecutive regions of a work buffer; with a null buffer only the offsets count
struct Carve {
    uint8_t* base;
    size_t off = 0;
    template <class T>
    T* take(size_t bytes) {
        T* p = base ? (T*)(base + off) : nullptr;
        off += bytes;
        return p;
    }
};

// The child side of the merge form: the child keys (padded), their sorted copy
// when the tiles + ranks sort runs, and the survivors-in-order flags
struct ChildWork {
    uint64_t *keys, *sorted;
    int32_t* flag;
};

// tt_ga_replace's work buffer: sort keys [pow2(N)], the gathered rows and meta, the
// source word, the merged keys [N], and the child side of its merge form, of kSortTile
// keys (tt_ga_replace_unique brings its own, of pow2(C) keys).
// bytes = tt_ga_work_bytes(N, E), source_offset = tt_ga_work_source_offset
struct GaWork {
    uint64_t* keys;
    uint8_t *ws, *wr;
    int32_t *wm, *source;
    uint64_t* mkeys;
    ChildWork child;
    size_t source_offset, bytes;
};
GaWork ga_work_layout(void* work, int N, int E);

// ascending sort of NP (a power of two) u64 keys on stream st, in place
void sort_keys(uint64_t* keys, int NP, hipStream_t st);
// the same, by whichever sort is fastest for NP; returns where the sorted keys are:
// `keys`, or `other` (NP keys) when the tiles + ranks sort ran (2*kRankTile <= NP <= kSortTile)
const uint64_t* sort_any(uint64_t* keys, uint64_t* other, int NP, hipStream_t st);

// The merge form for 0 < C <= kSortTile: the survivors' order checked, the `count`
// child keys (cw.keys, padded to CP; made here from cpen as sort_key(cpen[c], base + c)
// when cpen is given) sorted, merged with the survivors or, those out of order, all
// keys sorted by one workgroup (in w.keys). Returns the merged population's sorted
// keys (w.mkeys).
const uint64_t* merge_sorted_keys(const int32_t* pen, int N, ChildCount count, const int32_t* cpen, int base, int CP,
                                  const ChildWork& cw, const GaWork& w, hipStream_t st);

// Rows and meta in the order of `sorted` (a key's low word: a member's position
// < base, or base + c for child c) through the work rows back into the population,
// and the new pop[0]'s low word into the source word; 2 launches of N workgroups
void replace_move_rows(int E, int N, int base, const uint64_t* sorted, uint8_t* ps, uint8_t* pr, int32_t* ph,
                       int32_t* psc, uint8_t* pf, int32_t* pp, const uint8_t* cs, const uint8_t* cr, const int32_t* ch,
                       const int32_t* csc, const uint8_t* cf, const int32_t* cp, const GaWork& w, hipStream_t st);

}  // namespace ttga
