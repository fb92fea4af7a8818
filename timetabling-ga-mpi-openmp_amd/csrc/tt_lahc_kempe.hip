// Late-acceptance hill climbing with Kempe-chain candidates (include/ttga_lahc_kempe.h):
//   tt_lahc_kempe  tt_lahc's walk with a third kind of candidate: the connected
//                  component of e1 in the conflict graph of its slot and a second slot
//                  changes sides as a whole, its rooms chosen directly
// No counterpart in the reference; its call site is tt_lahc's. The walk itself is
// tt_lahc_kempe_walk.h's, which tt_lahc_kempe_aug.hip shares.
#include "tt_lahc_kempe_walk.h"

namespace ttga {

__global__ __launch_bounds__(64) void lahc_kempe_kernel(DevProblem pb, uint8_t* __restrict__ slot,
                                                        uint8_t* __restrict__ room, int64_t* __restrict__ rng, int P,
                                                        int steps, int L, double p_swap, double p_kempe,
                                                        double kempe_from, int max_chain, int32_t* __restrict__ scv,
                                                        int32_t* __restrict__ penalty, int32_t* __restrict__ gain,
                                                        int32_t* __restrict__ accepted, int32_t* __restrict__ best_step,
                                                        int32_t* __restrict__ kstats) {
    lahc_kempe_walk<false>(pb, slot, room, rng, P, steps, L, p_swap, p_kempe, kempe_from, max_chain, 0, scv, penalty, gain,
                           accepted, best_step, kstats);
}

}  // namespace ttga

using namespace ttga;

extern "C" int tt_lahc_kempe(const tt_problem* p, uint8_t* slot, uint8_t* room, int64_t* rng, int P, int steps,
                             int history, double p_swap, double p_kempe, int max_chain, int32_t* scv, int32_t* penalty,
                             int32_t* gain, int32_t* accepted, int32_t* best_step, int32_t* kempe_stats, void* stream) {
    int rc = check_pop_args(p, P, slot, room);
    if (rc) return rc;
    if (!rng) { set_error("tt_lahc_kempe: null rng buffer"); return TT_ERR_INVALID; }
    if (steps < 0) { set_error("tt_lahc_kempe: negative steps"); return TT_ERR_INVALID; }
    if (history < 1) { set_error("tt_lahc_kempe: history must be at least 1"); return TT_ERR_INVALID; }
    if (!(p_swap >= 0.0 && p_swap <= 1.0)) { set_error("tt_lahc_kempe: p_swap outside [0, 1]"); return TT_ERR_INVALID; }
    if (!(p_kempe >= 0.0 && p_kempe <= 1.0)) { set_error("tt_lahc_kempe: p_kempe outside [0, 1]"); return TT_ERR_INVALID; }
    if (max_chain < 0) { set_error("tt_lahc_kempe: negative max_chain"); return TT_ERR_INVALID; }
    const double kempe_from = 1.0 - p_kempe;
    if (!(p_swap <= kempe_from)) { set_error("tt_lahc_kempe: p_swap above 1 - p_kempe"); return TT_ERR_INVALID; }
    if (P == 0) return TT_OK;
    const size_t lds = lahc_kempe_lds_bytes(p->E, p->S, history);
    if (lds > kLahcMaxLds || p->dev.EW64 > 64 * kLkLaneWords) {
        set_error("instance or history too large for the late-acceptance search with Kempe chains");
        return TT_ERR_LIMIT;
    }
    if ((rc = use_device(p))) return rc;
    hipLaunchKernelGGL(lahc_kempe_kernel, dim3(P), dim3(64), lds, (hipStream_t)stream, p->dev, slot, room, rng, P, steps,
                       history, p_swap, p_kempe, kempe_from, max_chain, scv, penalty, gain, accepted, best_step,
                       kempe_stats);
    return check_hip(hipGetLastError(), "lahc_kempe launch");
}
