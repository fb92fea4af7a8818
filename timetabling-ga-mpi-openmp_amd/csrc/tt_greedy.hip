// Greedy constructive initial population (include/ttga_greedy.h):
//   tt_greedy_order  the events by 128 * degree + (64 - possible rooms), descending
//   tt_greedy_init   per individual, the events in that order into a slot of
//                    least conflict, ties drawn from its Random stream; then
//                    assignRooms on every slot (tt_rooms.hip)
// No counterpart in the reference; replaces RandomInitialSolution (ga.cpp:431) only.
#include <climits>

#include "tt_internal.h"
#include "tt_match.h"
#include "tt_place.h"

namespace ttga {

// tt_ga.hip: ascending bitonic sort of NP (a power of two) u64 keys on stream st
void sort_keys(uint64_t* keys, int NP, hipStream_t st);
// tt_rooms.hip
int launch_assign_masked(const tt_problem* p, const uint8_t* slot, uint8_t* room, int P, const uint8_t* mask,
                         uint8_t bit, hipStream_t st);

constexpr int kStatusBadOrder = 32;     // tt_device_status bit 5

static int order_keys(int E) {
    int np = 8;
    while (np < E) np <<= 1;
    return np;
}

// ---------------------------------------------------------------- order
// larger key first, ties by event index; padding keys sort after all
__global__ __launch_bounds__(256) void greedy_keys_kernel(DevProblem pb, int NP, uint64_t* __restrict__ keys) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= NP) return;
    if (e >= pb.E) { keys[e] = ~0ull; return; }
    const uint64_t* row = pb.corr64 + (size_t)e * pb.EW64;
    int deg = 0;
    for (int w = 0; w < pb.EW64; ++w) deg += __popcll(row[w]);
    deg -= (int)((row[e >> 6] >> (e & 63)) & 1);                      // the diagonal is not a neighbour
    const int key = 128 * deg + (64 - __popcll(pb.poss[e]));
    keys[e] = ((uint64_t)(uint32_t)(0x7FFFFFFF - key) << 32) | (uint32_t)e;
}

__global__ __launch_bounds__(256) void greedy_order_kernel(const uint64_t* __restrict__ keys, int E,
                                                           int32_t* __restrict__ order) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < E) order[i] = (int32_t)(uint32_t)keys[i];
}

// ---------------------------------------------------------------- placement (helpers: tt_place.h)
// E <= 448. One wave per individual, lane t = slot t: the slot's events as a
// bitset in the lane's registers, cost(t) = popcount(correlation row & bitset);
// the correlation row is wave-uniform (scalar loads). The slot row is collected
// in LDS and written out coalesced.
__global__ __launch_bounds__(64 * kGreedyWaves) void greedy_place_reg_kernel(DevProblem pb,
                                                                             const int32_t* __restrict__ order,
                                                                             int64_t* __restrict__ rng,
                                                                             uint8_t* __restrict__ slot, int P, int SP) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    const int E = pb.E, EW64 = pb.EW64, R = pb.R, lane = threadIdx.x & 63;
    const long p = (long)blockIdx.x * kGreedyWaves + wave_id();
    if (p >= P) return;
    uint8_t* row = lds + wave_id() * SP;
    for (int e = lane; e < E; e += 64) row[e] = 0xFF;
    wave_lds_sync();
    GreedyDraws d;
    d.init(rng[p], lane);
    uint64_t bits[kGreedyRegWords];
#pragma unroll
    for (int w = 0; w < kGreedyRegWords; ++w) bits[w] = 0;
    int cnt = 0, ord = 0;
    bool bad = false;
    for (int j = 0; j < E; ++j) {
        if ((j & 63) == 0) {
            d.next_batch();
            ord = j + lane < E ? order[j + lane] : 0;
        }
        const int e = __builtin_amdgcn_readlane(ord, j & 63);
        if ((unsigned)e >= (unsigned)E) {            // not a permutation: skip the entry, keep the draw
            bad = true;
            d.pick(j, 1);
            continue;
        }
        const uint64_t* cr = pb.corr64 + (size_t)e * EW64;
        int c = cnt >= R;
#pragma unroll
        for (int w = 0; w < kGreedyRegWords; ++w)
            if (w < EW64) c += __popcll(cr[w] & bits[w]);
        bool mine;
        const int t = greedy_choose(c, lane, d, j, mine);
        cnt += mine;
        const int ew = e >> 6;
        const uint64_t eb = 1ull << (e & 63);
#pragma unroll
        for (int w = 0; w < kGreedyRegWords; ++w) bits[w] |= (mine && w == ew) ? eb : 0ull;
        if (lane == 0) row[e] = (uint8_t)t;
    }
    wave_lds_sync();
    uint8_t* dst = slot + p * E;
    for (int e = lane; e < E; e += 64) dst[e] = row[e];
    if (lane == 0) {
        rng[p] = (int64_t)d.last;
        if (bad) atomicOr(pb.status, kStatusBadOrder);
    }
}

// Any E. One wave (workgroup) per individual; the slot row so far lives in LDS
// (255 = not placed). The lanes share the words of the event's correlation row
// and count every placed neighbour into its slot's counter (LDS atomics): the
// work follows the event's degree, and the LDS is E bytes whatever E is.
//   LDS: cost[64] i32 | row[64 * EW64] u8
__global__ __launch_bounds__(64) void greedy_place_row_kernel(DevProblem pb, const int32_t* __restrict__ order,
                                                              int64_t* __restrict__ rng, uint8_t* __restrict__ slot,
                                                              int P) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    const int E = pb.E, EW64 = pb.EW64, R = pb.R, lane = threadIdx.x;
    const long p = blockIdx.x;
    int* cost = (int*)lds;
    uint8_t* row = lds + 256;
    for (int e = lane; e < 64 * EW64; e += 64) row[e] = 0xFF;
    cost[lane] = 0;
    wave_lds_sync();
    GreedyDraws d;
    d.init(rng[p], lane);
    int cnt = 0, ord = 0;
    bool bad = false;
    for (int j = 0; j < E; ++j) {
        if ((j & 63) == 0) {
            d.next_batch();
            ord = j + lane < E ? order[j + lane] : 0;
        }
        const int e = __builtin_amdgcn_readlane(ord, j & 63);
        if ((unsigned)e >= (unsigned)E) {
            bad = true;
            d.pick(j, 1);
            continue;
        }
        const uint64_t* cr = pb.corr64 + (size_t)e * EW64;
        for (int w = lane; w < EW64; w += 64) {
            uint64_t x = cr[w];
            while (x) {
                const int n = 64 * w + __builtin_ctzll(x);
                x &= x - 1;
                const int tn = row[n];
                if (tn < kSlots) atomicAdd(&cost[tn], 1);
            }
        }
        wave_lds_sync();
        const int c = cost[lane] + (cnt >= R);
        cost[lane] = 0;
        bool mine;
        const int t = greedy_choose(c, lane, d, j, mine);
        cnt += mine;
        if (lane == 0) row[e] = (uint8_t)t;
        wave_lds_sync();
    }
    uint8_t* dst = slot + p * E;
    for (int e = lane; e < E; e += 64) dst[e] = row[e];
    if (lane == 0) {
        rng[p] = (int64_t)d.last;
        if (bad) atomicOr(pb.status, kStatusBadOrder);
    }
}

}  // namespace ttga

using namespace ttga;

extern "C" size_t tt_greedy_work_bytes(const tt_problem* p) { return p ? 8 * (size_t)order_keys(p->E) : 0; }

extern "C" int tt_greedy_order(const tt_problem* p, int32_t* order, void* work, void* stream) {
    if (!p) { set_error("null tt_problem"); return TT_ERR_INVALID; }
    if (!order || !work) { set_error("tt_greedy_order: null buffer"); return TT_ERR_INVALID; }
    int rc = use_device(p);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    const int E = p->E, NP = order_keys(E);
    uint64_t* keys = (uint64_t*)work;
    hipLaunchKernelGGL(greedy_keys_kernel, dim3((NP + 255) / 256), dim3(256), 0, st, p->dev, NP, keys);
    sort_keys(keys, NP, st);
    hipLaunchKernelGGL(greedy_order_kernel, dim3((E + 255) / 256), dim3(256), 0, st, keys, E, order);
    return check_hip(hipGetLastError(), "tt_greedy_order launch");
}

extern "C" int tt_greedy_init(const tt_problem* p, const int32_t* order, int64_t* rng, uint8_t* slot, uint8_t* room,
                              int P, void* stream) {
    int rc = check_pop_args(p, P, slot, room);
    if (rc || P == 0) return rc;
    if (!order || !rng) { set_error("tt_greedy_init: null order or rng buffer"); return TT_ERR_INVALID; }
    // the rooms come from the matcher: its limit is checked before anything is launched
    if (match_scratch_bytes(p->E, p->R, match_wide(p->R) ? kWideWaves : 1) > 160 * 1024) {
        set_error("instance too large for the matcher");
        return TT_ERR_LIMIT;
    }
    if ((rc = check_rows_grid("tt_greedy_init", p, P, true))) return rc;
    if ((rc = use_device(p))) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (p->dev.EW64 <= kGreedyRegWords) {
        const int SP = (p->E + 15) & ~15;
        hipLaunchKernelGGL(greedy_place_reg_kernel, dim3((P + kGreedyWaves - 1) / kGreedyWaves),
                           dim3(64 * kGreedyWaves), (size_t)kGreedyWaves * SP, st, p->dev, order, rng, slot, P, SP);
    } else {
        hipLaunchKernelGGL(greedy_place_row_kernel, dim3(P), dim3(64), 256 + (size_t)64 * p->dev.EW64, st, p->dev,
                           order, rng, slot, P);
    }
    if ((rc = check_hip(hipGetLastError(), "greedy placement launch"))) return rc;
    return launch_assign_masked(p, slot, room, P, nullptr, 0, st);
}
