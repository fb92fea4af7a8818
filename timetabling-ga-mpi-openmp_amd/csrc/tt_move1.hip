// The full single-event neighbourhood of a feasible row (include/ttga/move1.h):
//   tt_move1_scan     per individual, for every event e and slot t what "e goes to t" does
//                     to scv and which room it would take, and a summary of the table
//   tt_move1_descent  steepest descent on that table: the feasible move of least delta is
//                     applied while it lowers scv
// No counterpart in the reference; the descent's call site would follow ga.cpp:574-575,
// after the walk. One wave (workgroup) per individual. The entry is the walk's
// (tt_lahc_walk.h: lahc_enter builds the 45 event bitsets, the room occupancy, one
// attendance mask per student and the hcv gate), on the walk's LDS image without the
// history and the best row.
//
// One pass over the table is a wave-uniform loop over the events with lane = target slot
// (45 of 64 lanes busy): the clash test ANDs the event's correlation words (one address
// for the wave) with the lane's slot bitset, the room test is poss[e] & ~occ[t], and the
// change of scv is a loop over the students of e, 64 of their masks fetched at a time (lane
// = student) and handed round with readlane. A lane needs that loop only where its move is
// feasible or the caller asked for the d_scv table; an event with no such lane skips it.
// Every pass of the descent recomputes the whole table.
#include "tt_lahc_walk.h"
#include "../../include/ttga/move1.h"

namespace ttga {

constexpr int kStatusMove1BadGene = 1024;   // tt_device_status bit 10
constexpr long long kMove1NoKey = 0x7fffffffffffffffll;

// set[45][EW64] u64 | occ[45] u64 | mask[S] u64 | sl[E] rr[E] u8: lahc_carve(kLahcPlain)'s
// order without hist, bsl and brr, which stay null (lahc_enter with L = 0 touches none of them)
__host__ __device__ constexpr LahcLds move1_carve(uint8_t* base, int E, int EW64, int S) {
    LahcLds m{};
    size_t off = 0;
    m.set = lahc_take<uint64_t>(base, off, (size_t)kSlots * EW64);
    m.occ = lahc_take<uint64_t>(base, off, kSlots);
    m.mask = lahc_take<uint64_t>(base, off, S);
    m.sl = lahc_take<uint8_t>(base, off, E);
    m.rr = lahc_take<uint8_t>(base, off, E);
    m.bytes = off;
    return m;
}

__host__ __device__ constexpr size_t move1_lds_bytes(int E, int S) {
    return move1_carve(nullptr, E, (E + 63) / 64, S).bytes;
}

// the limit that include/ttga/move1.h documents: 8 (45 EW64 + 45 + S) + 2 E
static_assert(move1_lds_bytes(100, 80) == 1920, "sm");
static_assert(move1_lds_bytes(400, 200) == 5280, "med");
static_assert(move1_lds_bytes(2000, 5000) == 55880, "syn");
static_assert(move1_lds_bytes(100, 80) + 2 * 100 == lahc_lds_bytes(kLahcPlain, 100, 80, 0), "the walk's less the best row");
static_assert(move1_lds_bytes(40, 8200) > kLahcMaxLds, "8,200 students: the masks alone pass 64 KB");

// windows of three set bits + [exactly one bit] of one day's nine bits: lahc_day_cost
// without the last slot, which Solution::computeScv counts per event (studentNumber) and
// not per attended slot, so that the two differ where a student has two events in a slot
__device__ __forceinline__ int move1_day_cost(uint32_t d) { return __popc(d & (d >> 1) & (d >> 2)) + (__popc(d) == 1); }

__device__ __forceinline__ uint32_t move1_day(uint64_t m, int day) { return (uint32_t)(m >> (kSlotsPerDay * day)) & 0x1FFu; }

// what one pass finds: the wave's counts and the least key (delta, event, slot) over the
// feasible moves, kMove1NoKey when there is none; the same in every lane
struct Move1Sum {
    int feasible, improving;
    long long key;
};
__device__ __forceinline__ int move1_key_delta(long long key) { return (int)(key >> 32); }
__device__ __forceinline__ int move1_key_event(long long key) { return (int)((uint32_t)key >> 6); }
__device__ __forceinline__ int move1_key_slot(long long key) { return (int)((uint32_t)key & 63u); }

// One pass over the row in `m`: lane = target slot t. dl and tr (either may be null): the
// row's d_scv and to_room tables, [E][45]. Reads the image only; no barrier inside.
// Loop bounds: E events, each over EW64 correlation words and, where some lane wants the
// delta, over the event's students in blocks of 64.
__device__ __forceinline__ Move1Sum move1_pass(const DevProblem& pb, const LahcLds& m, int lane, int32_t* dl,
                                               uint8_t* tr) {
    const int E = pb.E, EW64 = pb.EW64;
    const bool live = lane < kSlots;
    const int t = live ? lane : kSlots - 1;             // the idle lanes read slot 44's words and write nothing
    const int dt = t / kSlotsPerDay;
    const uint32_t tbit = 1u << (t % kSlotsPerDay);
    const int last_t = t % kSlotsPerDay == kSlotsPerDay - 1;
    const uint64_t free_t = ~m.occ[t];
    const uint64_t* set_t = m.set + (size_t)t * EW64;
    int n_feas = 0, n_imp = 0;
    long long best = kMove1NoKey;
    for (int e = 0; e < E; ++e) {
        const int a = lahc_uniform((int)m.sl[e]);
        const uint64_t* cr = pb.corr64 + (size_t)e * EW64;
        bool clash = false;
        for (int w = 0; w < EW64; ++w) clash |= (cr[w] & set_t[w]) != 0ull;
        const uint64_t f = pb.poss[e] & free_t;
        const bool here = t == a;
        const int code = here ? (int)m.rr[e]
                         : clash ? TT_MOVE1_CLASH
                         : f == 0ull ? TT_MOVE1_NO_ROOM
                                     : __ffsll((unsigned long long)f) - 1;
        const bool feas = live && !here && code < kMaxRooms;
        int d = 0;
        if (wave_any(feas || (dl != nullptr && live))) {
            const int da = a / kSlotsPerDay;
            const uint32_t abit = 1u << (a % kSlotsPerDay);
            const bool same_day = dt == da;
            const int b = pb.ev_off[e], end = pb.ev_off[e + 1];
            for (int i0 = b; i0 < end; i0 += 64) {
                const int i = i0 + lane;
                const uint64_t mine = i < end ? m.mask[pb.ev_stu[i]] : 0ull;
                const int n = min(64, end - i0);
                for (int j = 0; j < n; ++j) {
                    const uint64_t mm = lahc_lane64(mine, j);
                    // the student leaves slot a (nobody has a second event there, the row being
                    // feasible) and attends slot t, which may hold another event of theirs
                    const uint32_t old_a = move1_day(mm, da), new_a = old_a & ~abit;
                    const uint32_t x = same_day ? new_a : move1_day(mm, dt);
                    const int base = same_day ? move1_day_cost(old_a)
                                              : move1_day_cost(x) + move1_day_cost(old_a) - move1_day_cost(new_a);
                    d += move1_day_cost(x | tbit) - base;
                }
            }
            d += pb.sn[e] * (last_t - (int)(a % kSlotsPerDay == kSlotsPerDay - 1));
        }
        if (live) {
            if (dl) dl[(size_t)e * kSlots + t] = d;
            if (tr) tr[(size_t)e * kSlots + t] = (uint8_t)code;
        }
        if (feas) {
            ++n_feas;
            n_imp += d < 0;
            const long long key = (long long)d * (1ll << 32) + (long long)(e * 64 + t);
            best = key < best ? key : best;
        }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const long long other = __shfl_xor(best, o);
        best = other < best ? other : best;
    }
    return {wave_sum(n_feas), wave_sum(n_imp), best};
}

// a row that is not scanned: the status bit of a bad gene
__device__ __forceinline__ void move1_flag(const DevProblem& pb, LahcEntry in, int lane) {
    if (in.bad_gene && lane == 0) atomicOr(pb.status, kStatusMove1BadGene);
}

__global__ __launch_bounds__(64) void move1_scan_kernel(DevProblem pb, const uint8_t* __restrict__ slot,
                                                        const uint8_t* __restrict__ room, int P,
                                                        int32_t* __restrict__ summary, int32_t* __restrict__ d_scv,
                                                        uint8_t* __restrict__ to_room) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    const int lane = threadIdx.x;
    const long p = blockIdx.x;
    if (p >= P) return;
    const LahcLds m = move1_carve(lds, pb.E, pb.EW64, pb.S);
    const LahcEntry in = lahc_enter(pb, m, slot, room, p, 1, 0, lane);
    const size_t cells = (size_t)pb.E * kSlots, base = (size_t)p * cells;
    int32_t* dl = d_scv ? d_scv + base : nullptr;
    uint8_t* tr = to_room ? to_room + base : nullptr;
    int32_t* sm = summary ? summary + (size_t)p * 6 : nullptr;
    if (in.closed) {
        for (size_t c = lane; c < cells; c += 64) {
            if (dl) dl[c] = TT_MOVE1_NONE;
            if (tr) tr[c] = TT_MOVE1_UNSCANNED;
        }
        if (sm && lane < 6) sm[lane] = lane < 4 ? 0 : -1;
        return move1_flag(pb, in, lane);
    }
    const Move1Sum s = move1_pass(pb, m, lane, dl, tr);
    if (sm && lane == 0) {
        const bool any = s.key != kMove1NoKey;
        sm[0] = 1;
        sm[1] = s.feasible;
        sm[2] = s.improving;
        sm[3] = any ? move1_key_delta(s.key) : 0;
        sm[4] = any ? move1_key_event(s.key) : -1;
        sm[5] = any ? move1_key_slot(s.key) : -1;
    }
}

// Lane roles of an applied move: the bitsets, occ and the two genes are written by every
// lane alike (each lane reads back what it wrote itself); the student masks are written by
// one lane (lane = student of the event) and read by another in the next pass: the barrier
// at the end of the pass covers them.
// Loop bounds: at most max_passes passes, and at most the row's scv, which falls with each.
__global__ __launch_bounds__(64) void move1_descent_kernel(DevProblem pb, uint8_t* __restrict__ slot,
                                                           uint8_t* __restrict__ room, int P, int max_passes,
                                                           int32_t* __restrict__ scv, int32_t* __restrict__ penalty,
                                                           int32_t* __restrict__ gain, int32_t* __restrict__ passes) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    const int E = pb.E, EW64 = pb.EW64, lane = threadIdx.x;
    const long p = blockIdx.x;
    if (p >= P) return;
    const LahcLds m = move1_carve(lds, E, EW64, pb.S);
    const LahcEntry in = lahc_enter(pb, m, slot, room, p, 1, 0, lane);
    if (in.closed) {
        if (lane == 0) {
            if (gain) gain[p] = 0;
            if (passes) passes[p] = 0;
        }
        return move1_flag(pb, in, lane);
    }
    int total = 0, applied = 0;
    while (applied < max_passes) {
        const Move1Sum s = move1_pass(pb, m, lane, nullptr, nullptr);
        if (s.key == kMove1NoKey) break;
        const int d = lahc_uniform(move1_key_delta(s.key));
        if (d >= 0) break;
        const int e = lahc_uniform(move1_key_event(s.key)), t = lahc_uniform(move1_key_slot(s.key));
        const int a = lahc_uniform((int)m.sl[e]), ro = lahc_uniform((int)m.rr[e]);
        const int r = lahc_uniform(__ffsll((unsigned long long)(pb.poss[e] & ~m.occ[t])) - 1);    // the pass's to_room
        const uint64_t abit = 1ull << a, tbit = 1ull << t;
        for (int i = pb.ev_off[e] + lane; i < pb.ev_off[e + 1]; i += 64) {
            const int s_ = pb.ev_stu[i];
            m.mask[s_] = (m.mask[s_] & ~abit) | tbit;
        }
        const uint64_t ebit = 1ull << (e & 63);
        m.set[(size_t)a * EW64 + (e >> 6)] &= ~ebit;
        m.set[(size_t)t * EW64 + (e >> 6)] |= ebit;
        m.occ[a] &= ~(1ull << ro);
        m.occ[t] |= 1ull << r;
        m.sl[e] = (uint8_t)t;
        m.rr[e] = (uint8_t)r;
        total -= d;
        ++applied;
        __syncthreads();
    }
    if (applied)
        for (int e = lane; e < E; e += 64) {
            slot[p * E + e] = m.sl[e];
            room[p * E + e] = m.rr[e];
        }
    if (lane == 0) {
        if (gain) gain[p] = total;
        if (passes) passes[p] = applied;
        lahc_credit(scv, penalty, p, total);
    }
}

// the arguments both entry points share; *lds: the launch's LDS size, set for P > 0
inline int move1_check(const std::string& fn, const tt_problem* p, int P, const uint8_t* slot, const uint8_t* room,
                       int max_passes, size_t* lds) {
    if (!p) { set_error("null tt_problem"); return TT_ERR_INVALID; }
    if (P < 0) { set_error("negative population size"); return TT_ERR_INVALID; }
    if (!slot || !room) { set_error(fn + ": null population buffer"); return TT_ERR_INVALID; }
    if (max_passes < 1) { set_error(fn + ": max_passes must be at least 1"); return TT_ERR_INVALID; }
    if (P == 0) return TT_OK;
    *lds = move1_lds_bytes(p->E, p->S);
    if (*lds > kLahcMaxLds) {
        set_error("instance too large for the single-event neighbourhood");
        return TT_ERR_LIMIT;
    }
    return check_rows_grid(fn.c_str(), p, P, false);
}

}  // namespace ttga

using namespace ttga;

extern "C" int tt_move1_scan(const tt_problem* p, const uint8_t* slot, const uint8_t* room, int P, int32_t* summary,
                             int32_t* d_scv, uint8_t* to_room, void* stream) {
    size_t lds = 0;
    int rc = move1_check("tt_move1_scan", p, P, slot, room, 1, &lds);
    if (rc || P == 0 || (!summary && !d_scv && !to_room)) return rc;
    if ((rc = use_device(p))) return rc;
    hipLaunchKernelGGL(move1_scan_kernel, dim3(P), dim3(64), lds, (hipStream_t)stream, p->dev, slot, room, P, summary,
                       d_scv, to_room);
    return check_hip(hipGetLastError(), "move1 scan launch");
}

extern "C" int tt_move1_descent(const tt_problem* p, uint8_t* slot, uint8_t* room, int P, int max_passes, int32_t* scv,
                                int32_t* penalty, int32_t* gain, int32_t* passes, void* stream) {
    size_t lds = 0;
    int rc = move1_check("tt_move1_descent", p, P, slot, room, max_passes, &lds);
    if (rc || P == 0) return rc;
    if ((rc = use_device(p))) return rc;
    hipLaunchKernelGGL(move1_descent_kernel, dim3(P), dim3(64), lds, (hipStream_t)stream, p->dev, slot, room, P,
                       max_passes, scv, penalty, gain, passes);
    return check_hip(hipGetLastError(), "move1 descent launch");
}
