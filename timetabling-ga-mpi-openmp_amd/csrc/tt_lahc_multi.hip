// Parallel walkers for the late-acceptance walk (include/ttga_lahc_multi.h):
//   tt_lahc_multi             K walks of tt_lahc_kempe_aug from every row, each on its own
//                             stretch of the row's stream; the best of them comes back
//   tt_lahc_multi_work_bytes  the size of its work buffer
// No counterpart in the reference; its call site is tt_lahc's.
//
// Two launches on the caller's stream. lahc_multi_walk_kernel: P * K waves, wave q is walker
// q % K of row q / K, tt_lahc_walk.h's lahc_chain_walk with kAug and kMulti. It reads the row
// and rng[p] and writes nothing but its own part of `work` (and the status bit of a bad gene).
// lahc_multi_commit_kernel, behind it: one wave per row takes the lowest-index maximum of
// the K gains, copies the winner's row and numbers out of `work` and moves rng[p] on. The
// stream orders the two, so a walker never sees a committed row and the commit sees every
// walker's writes. With K = 1 the call is tt_lahc_kempe_aug itself (lahc_kempe_aug_kernel,
// no work buffer) and a fill of winner and walker_gain.
#include "../../include/ttga_lahc_multi.h"
#include "tt_lahc_walk.h"
#include "tt_place.h"

namespace ttga {

constexpr int kLmMaxWalkers = 1024;

__global__ __launch_bounds__(64) void lahc_multi_walk_kernel(DevProblem pb, const uint8_t* __restrict__ slot,
                                                             const uint8_t* __restrict__ room,
                                                             const int64_t* __restrict__ rng, int P, int walkers,
                                                             int steps, int L, double p_swap, double p_kempe,
                                                             double kempe_from, int max_chain, int room_rule,
                                                             void* __restrict__ work) {
    // the walk's pointers are not const: under kMulti it stores through none of them
    lahc_chain_walk<true, true>(pb, const_cast<uint8_t*>(slot), const_cast<uint8_t*>(room), const_cast<int64_t*>(rng),
                                P, steps, L, p_swap, p_kempe, kempe_from, max_chain, room_rule, nullptr, nullptr,
                                nullptr, nullptr, nullptr, nullptr, walkers, work);
}

// One wave per row. Lane l looks at walkers l, l + 64, ...: ascending, so `>` keeps the
// lowest index of its maximum; across lanes the maximum, then the lowest index that has it.
// Gains are >= 0, a lane without a walker holds -1. Loop bounds: K / 64 <= 16 walkers a
// lane, E / 64 genes a lane.
__global__ __launch_bounds__(64) void lahc_multi_commit_kernel(int E, int P, int K, void* __restrict__ work,
                                                               uint8_t* __restrict__ slot, uint8_t* __restrict__ room,
                                                               int64_t* __restrict__ rng, int32_t* __restrict__ scv,
                                                               int32_t* __restrict__ penalty,
                                                               int32_t* __restrict__ gain,
                                                               int32_t* __restrict__ accepted,
                                                               int32_t* __restrict__ best_step,
                                                               int32_t* __restrict__ kstats,
                                                               int32_t* __restrict__ winner,
                                                               int32_t* __restrict__ walker_gain) {
    const long p = blockIdx.x;
    const int lane = threadIdx.x;
    if (p >= P) return;
    const LahcMultiWork mw = lahc_multi_work(work, P, K, E);
    const int32_t* nm = mw.nums + p * K * kLmNums;
    int bg = -1, bw = 0;
    for (int w = lane; w < K; w += 64) {
        const int g = nm[w * kLmNums + kLmGain];
        if (walker_gain) walker_gain[p * K + w] = g;
        if (g > bg) {
            bg = g;
            bw = w;
        }
    }
    const int top = -wave_min(-bg);
    const int win = wave_min(bg == top ? bw : INT_MAX);
    const bool walked = lahc_uniform(nm[kLmWalked]) != 0;       // walker 0's flag is every walker's
    if (!walked || win < 0 || win >= K) {                       // a closed row (or steps 0): zeros, nothing moves
        if (lane == 0) {
            if (gain) gain[p] = 0;
            if (accepted) accepted[p] = 0;
            if (best_step) best_step[p] = 0;
            if (winner) winner[p] = 0;
        }
        if (kstats && lane < 7) kstats[p * 7 + lane] = 0;
        return;
    }
    const long q = p * K + win;
    const int32_t* src = mw.nums + q * kLmNums;
    if (top > 0) {                                              // the winner improved: it wrote its row
        const uint8_t* row = mw.rows + (size_t)q * 2 * (size_t)E;
        for (int e = lane; e < E; e += 64) {
            slot[p * E + e] = row[e];
            room[p * E + e] = row[E + e];
        }
    }
    if (kstats && lane < 7) kstats[p * 7 + lane] = src[kLmStats + lane];
    if (lane == 0) {
        rng[p] = mw.state[p];
        if (gain) gain[p] = top;
        if (accepted) accepted[p] = src[kLmAccepted];
        if (best_step) best_step[p] = src[kLmBestStep];
        if (winner) winner[p] = win;
        lahc_credit(scv, penalty, p, top);
    }
}

// walkers == 1, behind tt_lahc_kempe_aug: the winner is walker 0 and its gain the row's
__global__ __launch_bounds__(256) void lahc_multi_single_kernel(int P, const int32_t* __restrict__ gain,
                                                                int32_t* __restrict__ winner,
                                                                int32_t* __restrict__ walker_gain) {
    const long p = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= P) return;
    if (winner) winner[p] = 0;
    if (walker_gain && gain != walker_gain) walker_gain[p] = gain[p];
}

}  // namespace ttga

using namespace ttga;

extern "C" size_t tt_lahc_multi_work_bytes(const tt_problem* p, int P, int walkers) {
    if (!p || P < 0 || walkers < 1 || walkers > kLmMaxWalkers) return 0;
    if ((long long)P * walkers > (long long)INT_MAX) return 0;
    return lahc_multi_work_size(P, walkers, p->E);
}

extern "C" int tt_lahc_multi(const tt_problem* p, uint8_t* slot, uint8_t* room, int64_t* rng, int P, int walkers,
                             int steps, int history, double p_swap, double p_kempe, int max_chain, int room_rule,
                             int32_t* scv, int32_t* penalty, int32_t* gain, int32_t* accepted, int32_t* best_step,
                             int32_t* kempe_stats, int32_t* winner, int32_t* walker_gain, void* work, void* stream) {
    const char* fn = "tt_lahc_multi";
    int rc = lahc_check_rows(fn, p, P, slot, room, rng);
    if (rc) return rc;
    if (walkers < 1 || walkers > kLmMaxWalkers) { set_error("tt_lahc_multi: walkers outside 1 .. 1024"); return TT_ERR_INVALID; }
    if ((rc = lahc_check_walk(fn, kLahcAug, steps, history, p_swap, p_kempe, max_chain, room_rule))) return rc;
    if (walkers > 1 && (!work || ((uintptr_t)work & 7u) != 0)) {
        set_error("tt_lahc_multi: work must be an 8-byte aligned buffer when walkers > 1");
        return TT_ERR_INVALID;
    }
    if (P == 0) return TT_OK;
    size_t lds = 0;
    if ((rc = lahc_check_lds(kLahcAug, p, history, &lds))) return rc;
    if ((long long)P * walkers > (long long)INT_MAX) {
        set_error("tt_lahc_multi: P * walkers above 2^31 - 1");
        return TT_ERR_LIMIT;
    }
    if ((rc = check_grid(fn, (long long)P * walkers, 64))) return rc;     // one wave per walker
    if (walkers == 1) {
        int32_t* g = gain ? gain : walker_gain;
        if ((rc = tt_lahc_kempe_aug(p, slot, room, rng, P, steps, history, p_swap, p_kempe, max_chain, room_rule, scv,
                                    penalty, g, accepted, best_step, kempe_stats, stream)))
            return rc;
        if (winner || (walker_gain && g != walker_gain)) {
            hipLaunchKernelGGL(lahc_multi_single_kernel, dim3((P + 255) / 256), dim3(256), 0, (hipStream_t)stream, P, g,
                               winner, walker_gain);
            return check_hip(hipGetLastError(), "lahc_multi fill launch");
        }
        return TT_OK;
    }
    if ((rc = use_device(p))) return rc;
    hipLaunchKernelGGL(lahc_multi_walk_kernel, dim3((unsigned)(P * walkers)), dim3(64), lds, (hipStream_t)stream, p->dev,
                       slot, room, rng, P, walkers, steps, history, p_swap, p_kempe, 1.0 - p_kempe, max_chain,
                       room_rule, work);
    if ((rc = check_hip(hipGetLastError(), "lahc_multi walk launch"))) return rc;
    hipLaunchKernelGGL(lahc_multi_commit_kernel, dim3(P), dim3(64), 0, (hipStream_t)stream, p->E, P, walkers, work, slot,
                       room, rng, scv, penalty, gain, accepted, best_step, kempe_stats, winner, walker_gain);
    return check_hip(hipGetLastError(), "lahc_multi commit launch");
}
