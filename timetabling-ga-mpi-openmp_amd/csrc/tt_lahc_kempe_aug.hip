// Augmenting-path rooms for the Kempe candidates of the late-acceptance walk
// (include/ttga_lahc_kempe_aug.h):
//   tt_lahc_kempe_aug  tt_lahc_kempe with a room_rule: where a chain event finds no free
//                      possible room, a breadth-first search over the target slot's holders
//                      moves them along an augmenting path
// No counterpart in the reference; its call site is tt_lahc's. The walk is
// tt_lahc_walk.h's lahc_chain_walk with kAug, in a translation unit of its own like
// lahc_kempe_kernel.
#include "tt_lahc_walk.h"

namespace ttga {

__global__ __launch_bounds__(64) void lahc_kempe_aug_kernel(DevProblem pb, uint8_t* __restrict__ slot,
                                                            uint8_t* __restrict__ room, int64_t* __restrict__ rng,
                                                            int P, int steps, int L, double p_swap, double p_kempe,
                                                            double kempe_from, int max_chain, int room_rule,
                                                            int32_t* __restrict__ scv, int32_t* __restrict__ penalty,
                                                            int32_t* __restrict__ gain, int32_t* __restrict__ accepted,
                                                            int32_t* __restrict__ best_step,
                                                            int32_t* __restrict__ kstats) {
    lahc_chain_walk<true>(pb, slot, room, rng, P, steps, L, p_swap, p_kempe, kempe_from, max_chain, room_rule, scv,
                          penalty, gain, accepted, best_step, kstats);
}

}  // namespace ttga

using namespace ttga;

extern "C" int tt_lahc_kempe_aug(const tt_problem* p, uint8_t* slot, uint8_t* room, int64_t* rng, int P, int steps,
                                 int history, double p_swap, double p_kempe, int max_chain, int room_rule, int32_t* scv,
                                 int32_t* penalty, int32_t* gain, int32_t* accepted, int32_t* best_step,
                                 int32_t* kempe_stats, void* stream) {
    size_t lds = 0;
    int rc = lahc_check_args("tt_lahc_kempe_aug", kLahcAug, p, P, slot, room, rng, steps, history, p_swap, p_kempe,
                             max_chain, room_rule, &lds);
    if (rc || P == 0) return rc;
    if ((rc = use_device(p))) return rc;
    hipLaunchKernelGGL(lahc_kempe_aug_kernel, dim3(P), dim3(64), lds, (hipStream_t)stream, p->dev, slot, room, rng, P,
                       steps, history, p_swap, p_kempe, 1.0 - p_kempe, max_chain, room_rule, scv, penalty, gain,
                       accepted, best_step, kempe_stats);
    return check_hip(hipGetLastError(), "lahc_kempe_aug launch");
}
