// Duplicate-free replacement and the first occurrence of every genome
// (include/ttga_unique.h). A genome is a slot row followed by a room row,
// 2*E bytes; a 32-bit hash of it nominates candidates and every equality is
// confirmed by comparing the rows in full.
//
//   hash_rows     16 lanes per row, four rows per wave: h = sum over byte
//                 positions q (slot bytes q = e, room bytes q = E + e) of
//                 mix(q, byte) mod 2^32, so the hash depends on every gene's
//                 position and on the row it is in, and not on how a row is
//                 aligned (rows start at byte i*E: up to 3 head bytes, aligned
//                 4-byte words, four of them in flight per lane, up to 3 tail
//                 bytes). The rows of the set that is searched (children, or
//                 the population of tt_genome_first) leave a key hash << 32 |
//                 index; these keys are sorted with tt_ga.hip's sorts.
//   unique_probe  one lane per item, candidates compared by the whole wave:
//                 a population member binary-searches its hash in the sorted
//                 child keys and clears the keep flag of the first child of
//                 that run of equal hashes whose rows equal its own (the later
//                 ones equal that child and drop themselves); the child at
//                 sorted position s scans its run from the start up to s and
//                 stops at the first equal row, which is the lowest index
//                 (keys sort by hash, then index): a run of identical genomes
//                 costs one comparison per row.
//   keep_scan     one workgroup: prefix sum over child_keep -> D = n_kept and
//                 the kept children's penalty keys sort_key(penalty, N + c) in
//                 child order, padded with ~0 to a power of two.
//   then tt_ga_replace's own steps (tt_ga.hip's kernels through
//   merge_sorted_keys and replace_move_rows, tt_replace_internal.h) with the two
//   things that differ passed as data: the child count is the device word n_kept
//   (the kernels that need k = N - D load it) and the base of a child key's low
//   word is N, so the source word of a child is N + c. Only the key fill of the
//   full sort for C > kSortTile is this file's own (unique_keys).
#include "../../include/ttga_unique.h"
#include "tt_replace_internal.h"

namespace ttga {

__device__ __forceinline__ uint32_t byte_mix(uint32_t q, uint32_t b) {
    uint32_t x = ((q << 8) | b) * 0x9E3779B1u + 0x7F4A7C15u;
    x ^= x >> 15;
    x *= 0x85EBCA77u;
    x ^= x >> 13;
    return x;
}

constexpr int kHashLanes = 16;        // lanes that share a row
constexpr int kHashRows = 256 / kHashLanes;

__device__ __forceinline__ uint32_t word_mix(uint32_t q, uint32_t v) {
    return byte_mix(q, v & 0xFFu) + byte_mix(q + 1, (v >> 8) & 0xFFu) + byte_mix(q + 2, (v >> 16) & 0xFFu) +
           byte_mix(q + 3, v >> 24);
}

// this lane's share (lane `sub` of the row's kHashLanes) of the hash of the E
// bytes at p, whose positions are q0..q0+E-1
__device__ __forceinline__ uint32_t row_hash_part(const uint8_t* __restrict__ p, int E, uint32_t q0, int sub) {
    uint32_t h = 0;
    const int head = min(E, (int)((4u - (uint32_t)((uintptr_t)p & 3u)) & 3u));
    if (sub < head) h += byte_mix(q0 + sub, p[sub]);
    const int nw = (E - head) >> 2;
    const uint32_t* __restrict__ w = (const uint32_t*)(p + head);
    for (int i0 = sub; i0 < nw; i0 += 4 * kHashLanes) {
        uint32_t v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int i = i0 + k * kHashLanes;
            v[k] = i < nw ? w[i] : 0u;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int i = i0 + k * kHashLanes;
            if (i < nw) h += word_mix(q0 + head + 4 * i, v[k]);
        }
    }
    const int done = head + 4 * nw;
    if (sub < E - done) h += byte_mix(q0 + done + sub, p[done + sub]);
    return h;
}

// Rows 0..n0-1 of (s0, r0) leave their hash in hash0; rows 0..n1-1 of (s1, r1)
// leave the key hash << 32 | index in keys1 (padded with ~0 to NP1 keys) and,
// with keep, keep[index] = 1. kHashLanes lanes per row.
__global__ __launch_bounds__(256) void hash_rows_kernel(int E, const uint8_t* __restrict__ s0,
                                                        const uint8_t* __restrict__ r0, int n0,
                                                        const uint8_t* __restrict__ s1,
                                                        const uint8_t* __restrict__ r1, int n1, uint32_t mask,
                                                        uint32_t* __restrict__ hash0, uint64_t* __restrict__ keys1,
                                                        int NP1, uint8_t* __restrict__ keep) {
    // (long: the grid has kHashLanes threads a row, so n1 + gt passes 2^31 from 1.3 * 10^8 rows on)
    const long gt = (long)blockIdx.x * 256 + threadIdx.x;
    for (long i = n1 + gt; i < NP1; i += (long)gridDim.x * 256) keys1[i] = ~0ull;
    const int sub = threadIdx.x & (kHashLanes - 1);
    const long row = (long)blockIdx.x * kHashRows + (threadIdx.x / kHashLanes);
    if (row >= (long)n0 + n1) return;                          // uniform over the row's lanes
    const bool first_set = row < n0;
    const long r = first_set ? row : row - n0;
    const uint8_t* ps = (first_set ? s0 : s1) + r * E;
    const uint8_t* pr = (first_set ? r0 : r1) + r * E;
    uint32_t h = row_hash_part(ps, E, 0u, sub) + row_hash_part(pr, E, (uint32_t)E, sub);
    for (int o = 1; o < kHashLanes; o <<= 1) h += __shfl_xor(h, o, 64);     // partners within the row's lanes
    h &= mask;
    if (sub == 0) {
        if (first_set) {
            hash0[r] = h;
        } else {
            keys1[r] = ((uint64_t)h << 32) | (uint32_t)r;
            if (keep) keep[r] = 1;
        }
    }
}

// first index in sorted[0..n) with sorted[index] >= x
__device__ __forceinline__ int lower_bound(const uint64_t* __restrict__ sorted, int n, uint64_t x) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (sorted[mid] < x) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// the rows (as, ar) and (bs, br) of E bytes each are equal; the whole wave calls it
__device__ __forceinline__ bool rows_equal(const uint8_t* __restrict__ as, const uint8_t* __restrict__ ar,
                                           const uint8_t* __restrict__ bs, const uint8_t* __restrict__ br, int E,
                                           int lane) {
    uint32_t d = 0;
    for (int e = lane; e < E; e += 64) d |= (uint32_t)(as[e] ^ bs[e]) | (uint32_t)(ar[e] ^ br[e]);
    return !wave_any(d != 0u);
}

// Item g < N is population member g, item N + s the child whose key is at
// sorted position s (sorted: the C child keys hash << 32 | index, ascending).
// A member drops the first child of its hash's run that equals it; a child
// looks for the first equal child before it in its run and, if there is one,
// drops itself (keep) and reports it (first; first[c] = c otherwise). Each lane
// searches its item's run; the wave then compares the candidates of one lane
// after the other, rows spread over its lanes.
__global__ __launch_bounds__(256) void unique_probe_kernel(int E, const uint8_t* __restrict__ ps,
                                                           const uint8_t* __restrict__ pr,
                                                           const uint32_t* __restrict__ phash, int N,
                                                           const uint8_t* __restrict__ cs,
                                                           const uint8_t* __restrict__ cr,
                                                           const uint64_t* __restrict__ sorted, int C,
                                                           uint8_t* __restrict__ keep, int32_t* __restrict__ first) {
    const int lane = threadIdx.x & 63;
    const long g = (long)blockIdx.x * 256 + threadIdx.x;
    const bool member = g < N, child = !member && g - N < C;
    int cur = 0, hi = 0, me = 0;
    if (member) {
        const uint64_t h = (uint64_t)phash[g] << 32;
        me = (int)g;
        cur = lower_bound(sorted, C, h);
        hi = lower_bound(sorted, C, h | 0xFFFFFFFFull);
    } else if (child) {
        const int s = (int)(g - N);
        const uint64_t key = sorted[s];
        me = (int)(uint32_t)key;
        cur = lower_bound(sorted, s, key & 0xFFFFFFFF00000000ull);
        hi = s;
    }
    int found = -1;
    for (;;) {
        const uint64_t todo = ballot(cur < hi);
        if (!todo) break;                                      // wave-uniform
        const int leader = __ffsll((unsigned long long)todo) - 1;
        const int a = __shfl(me, leader, 64), at = __shfl(cur, leader, 64);
        const bool a_member = __shfl((int)member, leader, 64) != 0;
        const int b = (int)(uint32_t)sorted[at];
        const uint8_t* as = (a_member ? ps : cs) + (long)a * E;
        const uint8_t* ar = (a_member ? pr : cr) + (long)a * E;
        const bool eq = rows_equal(as, ar, cs + (long)b * E, cr + (long)b * E, E, lane);
        if (lane == leader) {
            if (eq) { found = b; cur = hi; }
            else ++cur;
        }
    }
    if (member) {
        if (found >= 0) keep[found] = 0;
    } else if (child) {
        if (keep && found >= 0) keep[me] = 0;
        if (first) first[me] = found >= 0 ? found : me;
    }
}

// One workgroup: rank of every kept child = the kept children before it, D =
// their number; ckeys[rank] = sort_key(penalty, N + c), ckeys[D..CP) = ~0.
__global__ __launch_bounds__(1024) void keep_scan_kernel(const uint8_t* __restrict__ keep,
                                                         const int32_t* __restrict__ cpen, int N, int C, int CP,
                                                         uint64_t* __restrict__ ckeys, int32_t* __restrict__ n_kept) {
    __shared__ int wsum[16];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const int per = (C + 1023) / 1024, c0 = t * per, c1 = min(C, c0 + per);
    int cnt = 0;
    for (int c = c0; c < c1; ++c) cnt += keep[c] != 0;
    int inc = cnt;                                             // inclusive scan over the wave
    for (int o = 1; o < 64; o <<= 1) {
        const int v = __shfl_up(inc, o, 64);
        if (lane >= o) inc += v;
    }
    if (lane == 63) wsum[wv] = inc;
    __syncthreads();
    int before = 0, D = 0;
    for (int w = 0; w < 16; ++w) {
        if (w < wv) before += wsum[w];
        D += wsum[w];
    }
    int r = before + inc - cnt;
    for (int c = c0; c < c1; ++c)
        if (keep[c]) ckeys[r++] = sort_key(cpen[c], N + c);
    for (int i = D + t; i < CP; i += 1024) ckeys[i] = ~0ull;
    if (t == 0) *n_kept = D;
}

// C > kSortTile: the keys of a full sort. The one step not shared with tt_ga_replace,
// which has no child-key array of that size and fills its keys from the penalties
__global__ void unique_keys_kernel(const int32_t* __restrict__ pen, const uint64_t* __restrict__ ckeys,
                                   const int32_t* __restrict__ n_kept, int N, int NP, uint64_t* __restrict__ keys) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < NP) keys[i] = merged_key(pen, ckeys, N, N - *n_kept, i);
}

static bool hash_bits_ok(int hash_bits) { return hash_bits >= 0 && hash_bits <= 31; }
static uint32_t hash_mask(int hash_bits) { return hash_bits == 0 ? 0xFFFFFFFFu : (1u << hash_bits) - 1u; }

// work of tt_ga_replace_unique behind tt_ga_replace's: child hash keys [CP] u64 |
// their sorted copy [CP] | kept penalty keys [CP] | their sorted copy [CP] |
// member hashes [N] u32 | survivors-in-order flags (256 B)
// (bytes: all of tt_ga_unique_work_bytes(N, C, E))
struct UniqueWork {
    uint64_t *hkeys, *hsorted;
    ChildWork child;
    uint32_t* phash;
    size_t bytes;
};
static UniqueWork unique_work_layout(void* work, int N, int C, int E) {
    const size_t kb = align256(8 * (size_t)padded(C));
    Carve c{(uint8_t*)work, ga_work_layout(nullptr, N, E).bytes};
    UniqueWork u;
    u.hkeys = c.take<uint64_t>(kb);
    u.hsorted = c.take<uint64_t>(kb);
    u.child.keys = c.take<uint64_t>(kb);
    u.child.sorted = c.take<uint64_t>(kb);
    u.phash = c.take<uint32_t>(align256(4 * (size_t)N));
    u.child.flag = c.take<int32_t>(256);
    u.bytes = c.off;
    return u;
}

// work of tt_genome_first: the P hash keys, padded | their sorted copy
struct GenomeWork {
    uint64_t *keys, *other;
    size_t bytes;
};
static GenomeWork genome_work_layout(void* work, int P) {
    const size_t kb = align256(8 * (size_t)padded(P));
    Carve c{(uint8_t*)work};
    GenomeWork g;
    g.keys = c.take<uint64_t>(kb);
    g.other = c.take<uint64_t>(kb);
    g.bytes = c.off;
    return g;
}

}  // namespace ttga

using namespace ttga;

extern "C" size_t tt_genome_work_bytes(int P, int E) {
    if (P < 1 || E < 1) return 0;
    return genome_work_layout(nullptr, P).bytes;
}

extern "C" int tt_genome_first(const tt_problem* p, const uint8_t* slot, const uint8_t* room, int P, int32_t* first,
                               int hash_bits, void* work, void* stream) {
    int rc = check_pop_args(p, P, slot, room);
    if (rc) return rc;
    if (P > 0 && (!first || !work)) { set_error("null output or work buffer"); return TT_ERR_INVALID; }
    if (!hash_bits_ok(hash_bits)) { set_error("hash_bits must be 0..31"); return TT_ERR_INVALID; }
    if (P == 0) return TT_OK;
    if ((rc = check_grid("tt_genome_first", ((long long)P + kHashRows - 1) / kHashRows, 256))) return rc;
    if ((rc = use_device(p))) return rc;
    hipStream_t st = (hipStream_t)stream;
    const int E = p->E, PP = padded(P);
    const GenomeWork gw = genome_work_layout(work, P);
    hipLaunchKernelGGL(hash_rows_kernel, dim3((P + kHashRows - 1) / kHashRows), dim3(256), 0, st, E, (const uint8_t*)nullptr,
                       (const uint8_t*)nullptr, 0, slot, room, P, hash_mask(hash_bits), (uint32_t*)nullptr, gw.keys, PP,
                       (uint8_t*)nullptr);
    const uint64_t* sorted = sort_any(gw.keys, gw.other, PP, st);
    hipLaunchKernelGGL(unique_probe_kernel, dim3((P + 255) / 256), dim3(256), 0, st, E, (const uint8_t*)nullptr,
                       (const uint8_t*)nullptr, (const uint32_t*)nullptr, 0, slot, room, sorted, P, (uint8_t*)nullptr,
                       first);
    return check_hip(hipGetLastError(), "tt_genome_first launch");
}

extern "C" size_t tt_ga_unique_work_bytes(int N, int C, int E) {
    if (N < 1 || C < 0 || E < 1) return 0;
    return unique_work_layout(nullptr, N, C, E).bytes;
}

extern "C" int tt_ga_replace_unique(const tt_problem* p, uint8_t* pop_slot, uint8_t* pop_room, int32_t* pop_hcv,
                                    int32_t* pop_scv, uint8_t* pop_feasible, int32_t* pop_penalty, int N,
                                    const uint8_t* child_slot, const uint8_t* child_room, const int32_t* child_hcv,
                                    const int32_t* child_scv, const uint8_t* child_feasible,
                                    const int32_t* child_penalty, int C, uint8_t* child_keep, int32_t* n_kept,
                                    int hash_bits, void* work, void* stream) {
    if (!p) { set_error("null tt_problem"); return TT_ERR_INVALID; }
    if (N < 1 || C < 0 || C > N || !work || !pop_slot || !pop_room || !pop_hcv || !pop_scv || !pop_feasible ||
        !pop_penalty || (C > 0 && (!child_slot || !child_room || !child_hcv || !child_scv || !child_feasible ||
                                   !child_penalty || !child_keep || !n_kept))) {
        set_error("tt_ga_replace_unique: bad arguments");
        return TT_ERR_INVALID;
    }
    if (!hash_bits_ok(hash_bits)) { set_error("hash_bits must be 0..31"); return TT_ERR_INVALID; }
    hipStream_t st = (hipStream_t)stream;
    if (C == 0) {
        int rc = tt_ga_replace(p, pop_slot, pop_room, pop_hcv, pop_scv, pop_feasible, pop_penalty, N, pop_slot, pop_room,
                               pop_hcv, pop_scv, pop_feasible, pop_penalty, 0, work, stream);
        if (rc) return rc;
        if (n_kept) TT_HIP(hipMemsetAsync(n_kept, 0, sizeof(int32_t), st));
        return TT_OK;
    }
    int rc = check_rows_grid("tt_ga_replace_unique", p, N, false);
    if (rc) return rc;
    if ((rc = use_device(p))) return rc;
    const int E = p->E, NP = pow2_at_least(N), CP = padded(C);
    const GaWork gw = ga_work_layout(work, N, E);
    const UniqueWork uw = unique_work_layout(work, N, C, E);
    // which children are kept
    hipLaunchKernelGGL(hash_rows_kernel, dim3((N + C + kHashRows - 1) / kHashRows), dim3(256), 0, st, E, (const uint8_t*)pop_slot,
                       (const uint8_t*)pop_room, N, child_slot, child_room, C, hash_mask(hash_bits), uw.phash, uw.hkeys,
                       CP, child_keep);
    const uint64_t* hsorted = sort_any(uw.hkeys, uw.hsorted, CP, st);
    hipLaunchKernelGGL(unique_probe_kernel, dim3((N + C + 255) / 256), dim3(256), 0, st, E, (const uint8_t*)pop_slot,
                       (const uint8_t*)pop_room, (const uint32_t*)uw.phash, N, child_slot, child_room, hsorted, C,
                       child_keep, (int32_t*)nullptr);
    hipLaunchKernelGGL(keep_scan_kernel, dim3(1), dim3(1024), 0, st, (const uint8_t*)child_keep, child_penalty, N, C, CP,
                       uw.child.keys, n_kept);
    // tt_ga_replace's steps with the D = *n_kept kept children, their keys' low words N + c
    const uint64_t* sorted = gw.keys;
    if (C <= kSortTile) {
        sorted = merge_sorted_keys(pop_penalty, N, ChildCount{0, n_kept}, nullptr, N, CP, uw.child, gw, st);
    } else {
        hipLaunchKernelGGL(unique_keys_kernel, dim3((NP + 255) / 256), dim3(256), 0, st, (const int32_t*)pop_penalty,
                           (const uint64_t*)uw.child.keys, (const int32_t*)n_kept, N, NP, gw.keys);
        sort_keys(gw.keys, NP, st);
    }
    replace_move_rows(E, N, N, sorted, pop_slot, pop_room, pop_hcv, pop_scv, pop_feasible, pop_penalty, child_slot,
                      child_room, child_hcv, child_scv, child_feasible, child_penalty, gw, st);
    return check_hip(hipGetLastError(), "tt_ga_replace_unique launch");
}
