// Conflict-guided crossover (include/ttga_cx.h):
//   tt_crossover_guided  per individual, the events in `order`, each into the
//                        parent's slot that costs less among what the child has
//                        placed so far (the coin between equals; with repair, a
//                        slot of least cost where both parents' clash); then
//                        assignRooms on every slot (tt_rooms.hip)
//   tt_ga_breed_guided   tt_ga_breed (tt_ga.hip) with that crossover
// No counterpart in the reference; replaces Solution::crossover (ga.cpp:562-566) only.
#include "tt_internal.h"
#include "tt_match.h"
#include "tt_place.h"

namespace ttga {

// tt_rooms.hip
int launch_assign_masked(const tt_problem* p, const uint8_t* slot, uint8_t* room, int P, const uint8_t* mask,
                         uint8_t bit, hipStream_t st);
int launch_mutation_masked(const tt_problem* p, uint8_t* slot, uint8_t* room, int64_t* rng, int P,
                           const uint8_t* mask, uint8_t bit, hipStream_t st);

constexpr uint8_t kFlagCross = 1, kFlagMutate = 2;      // tt_ga.hip's
constexpr int kStatusBadCxOrder = 512;                  // tt_device_status bit 9

// What one launch works on. pen == nullptr: tt_crossover_guided, individual i
// crosses pa[i] and pb[i]. Otherwise tt_ga_breed_guided: pa = pop_slot,
// pb = pop_room, and breed_kernel's prologue picks the two parents.
struct CxArgs {
    const uint8_t *pa, *pb;
    const int32_t* pen;
    int N;
    double p_cross, p_mut;
    int skip_init;
    uint32_t jump_skip;
    const int32_t* order;
    int64_t* rng;
    uint8_t *slot, *room, *flags;
    int P, repair;
    int32_t *cost, *repaired;
};

// breed_kernel's draws up to the crossover draw (tt_ga.hip): every lane replays them
__device__ __forceinline__ bool cx_breed_prologue(const CxArgs& a, int E, int64_t& s, int best[2]) {
    if (a.skip_init) {
        pm_next(s);
        if ((uint64_t)s < kPmM)
            s = pm_mulmod((uint32_t)s, a.jump_skip);
        else
            for (int k = 1; k < 3 * E; ++k) pm_next(s);
    }
    for (int q = 0; q < 2; ++q) {                     // selection5 (ga.cpp:129-145)
        int b = pm_pick(s, a.N);
        for (int i = 1; i < 5; ++i) {
            const int t = pm_pick(s, a.N);
            if ((uint32_t)a.pen[t] < (uint32_t)a.pen[b]) b = t;
        }
        best[q] = b;
    }
    return pm_next(s) < a.p_cross;
}

// The running sums of one child (wave-uniform)
struct CxSums {
    int cost = 0, repaired = 0;
    bool invalid = false, bad = false;
};

// Lane t (< 45) holds cost(t) = c; a, b the parents' genes of the event (wave-
// uniform); draw j decides as ttga_cx.h's step 4. Returns the slot.
__device__ __forceinline__ int cx_choose(int c, int lane, GreedyDraws& d, int j, int a, int b, int repair,
                                         CxSums& sums) {
    if (lane >= kSlots) c = INT_MAX;
    const int ca = a < kSlots ? __builtin_amdgcn_readlane(c, a) : INT_MAX;
    const int cb = b < kSlots ? __builtin_amdgcn_readlane(c, b) : INT_MAX;
    int t;
    if (repair && min(ca, cb) > 0) {
        const bool tie = c == wave_min(c);
        const uint64_t T = ballot(tie);
        const int k = d.pick(j, __popcll(T));
        t = __builtin_ctzll(ballot(tie && __popcll(T & ((1ull << lane) - 1)) == k));
        ++sums.repaired;
    } else {
        d.pick(j, 1);                                  // the draw is taken whatever follows
        const bool coin_a = __dmul_rn(1.0 / 2147483647.0, (double)d.last) < 0.5;
        t = ca < cb ? a : cb < ca ? b : coin_a ? a : b;
    }
    if (t < kSlots)
        sums.cost += __builtin_amdgcn_readlane(c, t);
    else
        sums.invalid = true;
    return t;
}

// a not-crossed child: the copy of the first parent's rows
__device__ __forceinline__ void cx_copy_parent(const CxArgs& a, int E, long ch, int parent, int lane) {
    const uint8_t* sa = a.pa + (long)parent * E;
    const uint8_t* ra = a.pb + (long)parent * E;
    uint8_t* cs = a.slot + ch * E;
    uint8_t* cr = a.room + ch * E;
    for (int e = lane; e < E; e += 64) { cs[e] = sa[e]; cr[e] = ra[e]; }
}

__device__ __forceinline__ void cx_finish(const CxArgs& a, const DevProblem& pb, long ch, bool crossed, int64_t s,
                                          const CxSums& sums) {
    uint8_t f = crossed ? kFlagCross : 0;
    if (a.pen) {
        if (pm_next(s) < a.p_mut) f |= kFlagMutate;
        a.flags[ch] = f;
    }
    a.rng[ch] = s;
    if (a.cost) a.cost[ch] = !crossed ? 0 : sums.invalid ? -1 : sums.cost;
    if (a.repaired) a.repaired[ch] = crossed ? sums.repaired : 0;
    if (sums.bad) atomicOr(pb.status, kStatusBadCxOrder);
}

// E <= 448. One wave per child, lane t = slot t: the slot's events as a bitset
// in the lane's registers, cost(t) = popcount(correlation row & bitset); the
// correlation row is wave-uniform (scalar loads). The order entries, their
// draws and the parents' genes of 64 entries are fetched at a time. The slot
// row is collected in LDS and written out coalesced.
__global__ __launch_bounds__(64 * kGreedyWaves) void cx_reg_kernel(DevProblem pb, CxArgs a, int SP) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    const int E = pb.E, EW64 = pb.EW64, R = pb.R, lane = threadIdx.x & 63;
    const long ch = (long)blockIdx.x * kGreedyWaves + wave_id();
    if (ch >= a.P) return;                            // wave-uniform; the waves never meet at a barrier
    int64_t s = a.rng[ch];
    const uint8_t *sa = a.pa + ch * E, *sb = a.pb + ch * E;
    bool crossed = true;
    if (a.pen) {
        int best[2];
        crossed = cx_breed_prologue(a, E, s, best);
        sa = a.pa + (long)best[0] * E;
        sb = a.pa + (long)best[1] * E;
        if (!crossed) cx_copy_parent(a, E, ch, best[0], lane);
    }
    CxSums sums;
    if (crossed) {
        uint8_t* row = lds + wave_id() * SP;
        for (int e = lane; e < E; e += 64) row[e] = 0xFF;
        wave_lds_sync();
        GreedyDraws d;
        d.init(s, lane);
        uint64_t bits[kGreedyRegWords];
#pragma unroll
        for (int w = 0; w < kGreedyRegWords; ++w) bits[w] = 0;
        int cnt = 0, ord = 0, ga = 0xFF, gb = 0xFF;
        for (int j = 0; j < E; ++j) {
            if ((j & 63) == 0) {
                d.next_batch();
                ord = j + lane < E ? a.order[j + lane] : -1;
                const bool ok = (unsigned)ord < (unsigned)E;
                ga = ok ? sa[ord] : 0xFF;
                gb = ok ? sb[ord] : 0xFF;
            }
            const int e = __builtin_amdgcn_readlane(ord, j & 63);
            if ((unsigned)e >= (unsigned)E) {            // not a permutation: skip the entry, keep the draw
                sums.bad = true;
                d.pick(j, 1);
                continue;
            }
            const uint64_t* cr = pb.corr64 + (size_t)e * EW64;
            int c = cnt >= R;
#pragma unroll
            for (int w = 0; w < kGreedyRegWords; ++w)
                if (w < EW64) c += __popcll(cr[w] & bits[w]);
            const int t = cx_choose(c, lane, d, j, __builtin_amdgcn_readlane(ga, j & 63),
                                    __builtin_amdgcn_readlane(gb, j & 63), a.repair, sums);
            const bool mine = lane == t;
            cnt += mine;
            const int ew = e >> 6;
            const uint64_t eb = 1ull << (e & 63);
#pragma unroll
            for (int w = 0; w < kGreedyRegWords; ++w) bits[w] |= (mine && w == ew) ? eb : 0ull;
            if (lane == 0) row[e] = (uint8_t)t;
        }
        wave_lds_sync();
        uint8_t* dst = a.slot + ch * E;
        for (int e = lane; e < E; e += 64) dst[e] = row[e];
        s = (int64_t)d.last;
    }
    if (lane == 0) cx_finish(a, pb, ch, crossed, s, sums);
}

// Any E. One wave (workgroup) per child; the slot row so far lives in LDS
// (255 = not placed). The lanes share the words of the event's correlation row
// and count every placed neighbour into its slot's counter (LDS atomics), as
// greedy_place_row_kernel does.
//   LDS: cost[64] i32 | row[64 * EW64] u8
__global__ __launch_bounds__(64) void cx_row_kernel(DevProblem pb, CxArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    const int E = pb.E, EW64 = pb.EW64, R = pb.R, lane = threadIdx.x;
    const long ch = blockIdx.x;
    int64_t s = a.rng[ch];
    const uint8_t *sa = a.pa + ch * E, *sb = a.pb + ch * E;
    bool crossed = true;
    if (a.pen) {
        int best[2];
        crossed = cx_breed_prologue(a, E, s, best);
        sa = a.pa + (long)best[0] * E;
        sb = a.pa + (long)best[1] * E;
        if (!crossed) cx_copy_parent(a, E, ch, best[0], lane);
    }
    CxSums sums;
    if (crossed) {
        int* cost = (int*)lds;
        uint8_t* row = lds + 256;
        for (int e = lane; e < 64 * EW64; e += 64) row[e] = 0xFF;
        cost[lane] = 0;
        wave_lds_sync();
        GreedyDraws d;
        d.init(s, lane);
        int cnt = 0, ord = 0, ga = 0xFF, gb = 0xFF;
        for (int j = 0; j < E; ++j) {
            if ((j & 63) == 0) {
                d.next_batch();
                ord = j + lane < E ? a.order[j + lane] : -1;
                const bool ok = (unsigned)ord < (unsigned)E;
                ga = ok ? sa[ord] : 0xFF;
                gb = ok ? sb[ord] : 0xFF;
            }
            const int e = __builtin_amdgcn_readlane(ord, j & 63);
            if ((unsigned)e >= (unsigned)E) {
                sums.bad = true;
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
            const int t = cx_choose(c, lane, d, j, __builtin_amdgcn_readlane(ga, j & 63),
                                    __builtin_amdgcn_readlane(gb, j & 63), a.repair, sums);
            cnt += lane == t;
            if (lane == 0) row[e] = (uint8_t)t;
            wave_lds_sync();
        }
        uint8_t* dst = a.slot + ch * E;
        for (int e = lane; e < E; e += 64) dst[e] = row[e];
        s = (int64_t)d.last;
    }
    if (lane == 0) cx_finish(a, pb, ch, crossed, s, sums);
}

// 16807^n mod (2^31 - 1) on the host (the jump over the discarded draws)
static uint32_t cx_host_pm_pow(long n) {
    uint64_t r = 1, b = 16807;
    for (; n > 0; n >>= 1) {
        if (n & 1) r = r * b % 2147483647ull;
        b = b * b % 2147483647ull;
    }
    return (uint32_t)r;
}

// the rooms come from the matcher: its limit is checked before anything is launched
static int cx_check_limit(const char* fn, const tt_problem* p, int rows) {
    if (match_scratch_bytes(p->E, p->R, match_wide(p->R) ? kWideWaves : 1) > 160 * 1024) {
        set_error("instance too large for the matcher");
        return TT_ERR_LIMIT;
    }
    return check_rows_grid(fn, p, rows, true);
}

static int cx_launch(const tt_problem* p, const CxArgs& a, hipStream_t st) {
    if (p->dev.EW64 <= kGreedyRegWords) {
        const int SP = (p->E + 15) & ~15;
        hipLaunchKernelGGL(cx_reg_kernel, dim3((a.P + kGreedyWaves - 1) / kGreedyWaves), dim3(64 * kGreedyWaves),
                           (size_t)kGreedyWaves * SP, st, p->dev, a, SP);
    } else {
        hipLaunchKernelGGL(cx_row_kernel, dim3(a.P), dim3(64), 256 + (size_t)64 * p->dev.EW64, st, p->dev, a);
    }
    return check_hip(hipGetLastError(), "guided crossover launch");
}

}  // namespace ttga

using namespace ttga;

extern "C" int tt_crossover_guided(const tt_problem* p, const uint8_t* slot1, const uint8_t* slot2,
                                   const int32_t* order, int64_t* rng, uint8_t* slot, uint8_t* room, int P, int repair,
                                   int32_t* cost, int32_t* repaired, void* stream) {
    if (!p) { set_error("null tt_problem"); return TT_ERR_INVALID; }
    if (P < 0) { set_error("negative population size"); return TT_ERR_INVALID; }
    if (P == 0) return TT_OK;
    if (!slot1 || !slot2 || !slot || !room) { set_error("tt_crossover_guided: null population buffer"); return TT_ERR_INVALID; }
    if (!order || !rng) { set_error("tt_crossover_guided: null order or rng buffer"); return TT_ERR_INVALID; }
    int rc = cx_check_limit("tt_crossover_guided", p, P);
    if (rc) return rc;
    if ((rc = use_device(p))) return rc;
    hipStream_t st = (hipStream_t)stream;
    CxArgs a{slot1, slot2, nullptr, 0, 0.0, 0.0, 0, 0u, order, rng, slot, room, nullptr, P, repair, cost, repaired};
    if ((rc = cx_launch(p, a, st))) return rc;
    return launch_assign_masked(p, slot, room, P, nullptr, 0, st);
}

extern "C" int tt_ga_breed_guided(const tt_problem* p, const uint8_t* pop_slot, const uint8_t* pop_room,
                                  const int32_t* pop_penalty, int N, const int32_t* order, int64_t* rng, int C,
                                  double p_cross, double p_mut, int skip_init_draws, int repair, uint8_t* child_slot,
                                  uint8_t* child_room, uint8_t* child_flags, int32_t* child_cost,
                                  int32_t* child_repaired, void* stream) {
    int rc = check_pop_args(p, C, child_slot, child_room);
    if (rc) return rc;
    if (N < 1 || !pop_slot || !pop_room || !pop_penalty || (C > 0 && (!rng || !child_flags))) {
        set_error("tt_ga_breed_guided: bad population arguments");
        return TT_ERR_INVALID;
    }
    if (C == 0) return TT_OK;
    if (!order) { set_error("tt_ga_breed_guided: null order buffer"); return TT_ERR_INVALID; }
    if ((rc = cx_check_limit("tt_ga_breed_guided", p, C))) return rc;
    if ((rc = use_device(p))) return rc;
    hipStream_t st = (hipStream_t)stream;
    CxArgs a{pop_slot, pop_room, pop_penalty, N, p_cross, p_mut, skip_init_draws, cx_host_pm_pow(3L * p->E - 1), order,
             rng, child_slot, child_room, child_flags, C, repair, child_cost, child_repaired};
    if ((rc = cx_launch(p, a, st))) return rc;
    if ((rc = launch_assign_masked(p, child_slot, child_room, C, child_flags, kFlagCross, st))) return rc;
    return launch_mutation_masked(p, child_slot, child_room, rng, C, child_flags, kFlagMutate, st);
}
