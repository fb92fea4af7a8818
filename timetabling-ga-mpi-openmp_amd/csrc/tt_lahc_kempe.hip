// Late-acceptance hill climbing with Kempe-chain candidates (include/ttga_lahc_kempe.h):
//   tt_lahc_kempe  tt_lahc's walk with a third kind of candidate: the connected
//                  component of e1 in the conflict graph of its slot and a second slot
//                  changes sides as a whole, its rooms chosen directly
// No counterpart in the reference; its call site is tt_lahc's. The walk is
// tt_lahc_walk.h's lahc_chain_walk with the direct room rule. The kernel has a translation
// unit of its own: next to lahc_kernel its branch labels would carry another number.
#include "tt_lahc_walk.h"

namespace ttga {

__global__ __launch_bounds__(64) void lahc_kempe_kernel(DevProblem pb, uint8_t* __restrict__ slot,
                                                        uint8_t* __restrict__ room, int64_t* __restrict__ rng, int P,
                                                        int steps, int L, double p_swap, double p_kempe,
                                                        double kempe_from, int max_chain, int32_t* __restrict__ scv,
                                                        int32_t* __restrict__ penalty, int32_t* __restrict__ gain,
                                                        int32_t* __restrict__ accepted, int32_t* __restrict__ best_step,
                                                        int32_t* __restrict__ kstats) {
    lahc_chain_walk<false>(pb, slot, room, rng, P, steps, L, p_swap, p_kempe, kempe_from, max_chain, 0, scv, penalty, gain,
                           accepted, best_step, kstats);
}

}  // namespace ttga

using namespace ttga;

extern "C" int tt_lahc_kempe(const tt_problem* p, uint8_t* slot, uint8_t* room, int64_t* rng, int P, int steps,
                             int history, double p_swap, double p_kempe, int max_chain, int32_t* scv, int32_t* penalty,
                             int32_t* gain, int32_t* accepted, int32_t* best_step, int32_t* kempe_stats, void* stream) {
    size_t lds = 0;
    int rc = lahc_check_args("tt_lahc_kempe", kLahcChain, p, P, slot, room, rng, steps, history, p_swap, p_kempe,
                             max_chain, 0, &lds);
    if (rc || P == 0) return rc;
    if ((rc = use_device(p))) return rc;
    hipLaunchKernelGGL(lahc_kempe_kernel, dim3(P), dim3(64), lds, (hipStream_t)stream, p->dev, slot, room, rng, P, steps,
                       history, p_swap, p_kempe, 1.0 - p_kempe, max_chain, scv, penalty, gain, accepted, best_step,
                       kempe_stats);
    return check_hip(hipGetLastError(), "lahc_kempe launch");
}
