// Late-acceptance hill climbing on feasible rows (include/ttga_lahc.h):
//   tt_lahc  per individual, a walk of Move1 / Move2 candidates that keep hcv 0; a
//            candidate is accepted when it is no worse than the current row or than
//            the row `history` steps ago; the best row seen comes back
// No counterpart in the reference; its call site would follow ga.cpp:574-575.
//
// On a feasible row a student attends at most one event per slot, so scv is a sum over
// the students of a function of the 45-bit attendance mask m: per 9-bit day,
// [bit 8] + the windows of three set bits + [exactly one bit]. A move of event e from
// slot a to slot t turns m into m ^ bit a ^ bit t for the students of e and for nobody
// else, and only the days of a and t change their cost. The feasibility of a candidate
// is one AND of the event's correlation row with the target slot's event bitset and
// one AND of its possible rooms with the slot's free rooms; no matcher runs.
#include "../../include/ttga_lahc.h"
#include "tt_internal.h"
#include "tt_lahc_common.h"

namespace ttga {

// LDS of one wave: set[45][EW64] u64 | occ[45] u64 | mask[S] u64 | hist[L] i32 |
//                  sl[E] | rr[E] | bsl[E] | brr[E]  (u8)
__host__ __device__ inline size_t lahc_lds_bytes(int E, int S, int L) {
    return 8 * ((size_t)kSlots * (size_t)((E + 63) / 64) + kSlots + (size_t)S) + 4 * (size_t)L + 4 * (size_t)E;
}

// One wave (workgroup) per individual. Everything that decides a step is wave-uniform:
// every lane draws the same three numbers from its own copy of the state, and the
// words that all lanes update (set, occ, the two genes, hist) are written by every
// lane with the same value to the same address, so each lane later reads what it
// wrote itself. Only the student masks are written by one lane and read by another:
// a barrier follows every applied move. Lane roles: entry = event / student per lane;
// correlation test = bitset word per lane; delta and apply = student of the moved
// event(s) per lane.
// Loop bounds: `steps` steps; inside a step, ceil(EW64 / 64) words and
// ceil(students of the one or two events / 64) students per lane.
__global__ __launch_bounds__(64) void lahc_kernel(DevProblem pb, uint8_t* __restrict__ slot, uint8_t* __restrict__ room,
                                                  int64_t* __restrict__ rng, int P, int steps, int L, double p_swap,
                                                  int32_t* __restrict__ scv, int32_t* __restrict__ penalty,
                                                  int32_t* __restrict__ gain, int32_t* __restrict__ accepted,
                                                  int32_t* __restrict__ best_step) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    const int E = pb.E, R = pb.R, S = pb.S, EW64 = pb.EW64, lane = threadIdx.x;
    const long p = blockIdx.x;
    if (p >= P) return;
    uint64_t* set = (uint64_t*)lds;
    uint64_t* occ = set + (size_t)kSlots * EW64;
    uint64_t* mask = occ + kSlots;
    int32_t* hist = (int32_t*)(mask + S);
    uint8_t* sl = (uint8_t*)(hist + L);
    uint8_t* rr = sl + E;
    uint8_t* bsl = rr + E;
    uint8_t* brr = bsl + E;

    // ---- entry: the row, validity, the bitsets and the hcv gate
    bool bad = false;
    for (int e = lane; e < E; e += 64) {
        const uint8_t s = slot[p * E + e], r = room[p * E + e];
        sl[e] = s;
        rr[e] = r;
        bad |= s >= kSlots || r >= R;
    }
    for (int i = lane; i < kSlots * EW64 + kSlots; i += 64) set[i] = 0ull;      // set and occ are adjacent
    for (int i = lane; i < L; i += 64) hist[i] = 0;                             // costs are kept relative to scv0
    __syncthreads();
    if (wave_any(bad)) {
        if (lane == 0) {
            if (gain) gain[p] = 0;
            if (accepted) accepted[p] = 0;
            if (best_step) best_step[p] = 0;
            atomicOr(pb.status, kStatusLahcBadGene);
        }
        return;
    }
    bool hard = false;                                  // a hard-constraint violation seen by this lane
    for (int e = lane; e < E; e += 64) {
        const int s = sl[e], r = rr[e];
        atomicOr((unsigned long long*)&set[(size_t)s * EW64 + (e >> 6)], 1ull << (e & 63));
        const unsigned long long old = atomicOr((unsigned long long*)&occ[s], 1ull << r);
        hard |= ((old >> r) & 1ull) != 0ull;            // two events in one room of one slot
        hard |= ((pb.poss[e] >> r) & 1ull) == 0ull;     // a room that is not possible
    }
    // two correlated events share a student: they are in one slot exactly if some
    // student's events cover fewer slots than the student has events
    for (int s = lane; s < S; s += 64) {
        const int b = pb.stu_off[s], end = pb.stu_off[s + 1];
        uint64_t m = 0ull;
        for (int i = b; i < end; ++i) m |= 1ull << sl[pb.stu_ev[i]];
        mask[s] = m;
        hard |= __popcll(m) != end - b;
    }
    __syncthreads();
    if (wave_any(hard) || steps == 0) {
        if (lane == 0) {
            if (gain) gain[p] = 0;
            if (accepted) accepted[p] = 0;
            if (best_step) best_step[p] = 0;
        }
        return;
    }

    // ---- the walk (cur and best relative to scv0)
    int64_t st = rng[p];
    int cur = 0, best = 0, n_acc = 0, b_step = 0;
    bool live_is_best = true;                           // the best row is the row in sl / rr
    int v = 0;
    for (int k = 0; k < steps; ++k) {
        const int e1 = min(max(lahc_uniform(pm_pick(st, E)), 0), E - 1);
        const double u = pm_next(st), x = pm_next(st);
        const bool swap = E >= 2 && lahc_uniform((int)(u < p_swap)) != 0;
        const int a = lahc_uniform((int)sl[e1]);
        const int off1 = pb.ev_off[e1], n1 = pb.ev_off[e1 + 1] - off1;
        int e2 = e1, b, r1, r2 = 0, off2 = 0, n2 = 0;
        bool feas;
        if (swap) {
            e2 = lahc_uniform((int)__dmul_rn(x, (double)(E - 1)));
            e2 += e2 >= e1;
            e2 = min(max(e2, 0), E - 1);
            b = lahc_uniform((int)sl[e2]);
            off2 = pb.ev_off[e2];
            n2 = pb.ev_off[e2 + 1] - off2;
            bool clash = false;
            for (int w = lane; w < EW64; w += 64) {
                uint64_t sb = set[(size_t)b * EW64 + w], sa = set[(size_t)a * EW64 + w];
                if (w == (e2 >> 6)) sb &= ~(1ull << (e2 & 63));
                if (w == (e1 >> 6)) sa &= ~(1ull << (e1 & 63));
                clash |= ((pb.corr64[(size_t)e1 * EW64 + w] & sb) | (pb.corr64[(size_t)e2 * EW64 + w] & sa)) != 0ull;
            }
            const uint64_t f1 = pb.poss[e1] & ~(occ[b] & ~(1ull << rr[e2]));
            const uint64_t f2 = pb.poss[e2] & ~(occ[a] & ~(1ull << rr[e1]));
            r1 = lahc_uniform(__ffsll((unsigned long long)f1) - 1);
            r2 = lahc_uniform(__ffsll((unsigned long long)f2) - 1);
            feas = a != b && r1 >= 0 && r2 >= 0 && !wave_any(clash);
        } else {
            b = lahc_uniform((int)__dmul_rn(x, (double)(kSlots - 1)));
            b += b >= a;
            b = min(max(b, 0), kSlots - 1);
            bool clash = false;
            for (int w = lane; w < EW64; w += 64)
                clash |= (pb.corr64[(size_t)e1 * EW64 + w] & set[(size_t)b * EW64 + w]) != 0ull;
            const uint64_t f1 = pb.poss[e1] & ~occ[b];
            r1 = lahc_uniform(__ffsll((unsigned long long)f1) - 1);
            feas = r1 >= 0 && !wave_any(clash);
        }
        if (feas) {
            // the students of e1, then (Move2) of e2; one who attends both keeps the mask:
            // the other slot's bit is set for nobody else, the candidate being feasible
            const uint64_t flip = (1ull << a) | (1ull << b);
            const int da = a / kSlotsPerDay, db = b / kSlotsPerDay, n = n1 + n2;
            int d = 0;
            for (int i = lane; i < n; i += 64) {
                const bool first = i < n1;
                const uint64_t m = mask[pb.ev_stu[first ? off1 + i : off2 + i - n1]];
                if (!swap || ((m >> (first ? b : a)) & 1ull) == 0ull) d += lahc_mask_delta(m, flip, da, db);
            }
            const int cand = cur + wave_sum(d);
            if (cand <= cur || cand <= lahc_uniform(hist[v])) {
                if (live_is_best && cand >= cur) {      // the row is about to leave the best one
                    for (int e = lane; e < E; e += 64) { bsl[e] = sl[e]; brr[e] = rr[e]; }
                    live_is_best = false;
                }
                for (int i = lane; i < n; i += 64) {
                    const bool first = i < n1;
                    const int s = pb.ev_stu[first ? off1 + i : off2 + i - n1];
                    const uint64_t m = mask[s];
                    if (!swap || ((m >> (first ? b : a)) & 1ull) == 0ull) mask[s] = m ^ flip;
                }
                const uint64_t bit1 = 1ull << (e1 & 63);
                uint64_t* wa1 = &set[(size_t)a * EW64 + (e1 >> 6)];
                uint64_t* wb1 = &set[(size_t)b * EW64 + (e1 >> 6)];
                *wa1 &= ~bit1;
                *wb1 |= bit1;
                const int ro1 = rr[e1];
                if (swap) {
                    const uint64_t bit2 = 1ull << (e2 & 63);
                    uint64_t* wb2 = &set[(size_t)b * EW64 + (e2 >> 6)];
                    uint64_t* wa2 = &set[(size_t)a * EW64 + (e2 >> 6)];
                    *wb2 &= ~bit2;
                    *wa2 |= bit2;
                    const int ro2 = rr[e2];
                    occ[a] = (occ[a] & ~(1ull << ro1)) | (1ull << r2);
                    occ[b] = (occ[b] & ~(1ull << ro2)) | (1ull << r1);
                    sl[e2] = (uint8_t)a;
                    rr[e2] = (uint8_t)r2;
                } else {
                    occ[a] &= ~(1ull << ro1);
                    occ[b] |= 1ull << r1;
                }
                sl[e1] = (uint8_t)b;
                rr[e1] = (uint8_t)r1;
                cur = cand;
                ++n_acc;
                if (cur < best) {
                    best = cur;
                    b_step = k + 1;
                    live_is_best = true;
                }
                __syncthreads();                        // the masks: written by one lane, read by another
            }
        }
        hist[v] = cur;
        v = v + 1 == L ? 0 : v + 1;
    }

    // ---- exit: the best row
    if (b_step > 0) {
        const uint8_t* os = live_is_best ? sl : bsl;
        const uint8_t* orr = live_is_best ? rr : brr;
        for (int e = lane; e < E; e += 64) {
            slot[p * E + e] = os[e];
            room[p * E + e] = orr[e];
        }
    }
    if (lane == 0) {
        rng[p] = st;
        const int g = -best;
        if (gain) gain[p] = g;
        if (accepted) accepted[p] = n_acc;
        if (best_step) best_step[p] = b_step;
        if (scv) scv[p] -= g;
        if (penalty) {
            const int pen = penalty[p];
            if (pen >= 0 && pen < 1000000) penalty[p] = pen - g;
        }
    }
}

}  // namespace ttga

using namespace ttga;

extern "C" int tt_lahc(const tt_problem* p, uint8_t* slot, uint8_t* room, int64_t* rng, int P, int steps, int history,
                       double p_swap, int32_t* scv, int32_t* penalty, int32_t* gain, int32_t* accepted,
                       int32_t* best_step, void* stream) {
    int rc = check_pop_args(p, P, slot, room);
    if (rc) return rc;
    if (!rng) { set_error("tt_lahc: null rng buffer"); return TT_ERR_INVALID; }
    if (steps < 0) { set_error("tt_lahc: negative steps"); return TT_ERR_INVALID; }
    if (history < 1) { set_error("tt_lahc: history must be at least 1"); return TT_ERR_INVALID; }
    if (!(p_swap >= 0.0 && p_swap <= 1.0)) { set_error("tt_lahc: p_swap outside [0, 1]"); return TT_ERR_INVALID; }
    if (P == 0) return TT_OK;
    const size_t lds = lahc_lds_bytes(p->E, p->S, history);
    if (lds > kLahcMaxLds) {
        set_error("instance or history too large for the late-acceptance search");
        return TT_ERR_LIMIT;
    }
    if ((rc = use_device(p))) return rc;
    hipLaunchKernelGGL(lahc_kernel, dim3(P), dim3(64), lds, (hipStream_t)stream, p->dev, slot, room, rng, P, steps,
                       history, p_swap, scv, penalty, gain, accepted, best_step);
    return check_hip(hipGetLastError(), "lahc launch");
}
