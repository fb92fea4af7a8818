// Late-acceptance hill climbing on feasible rows (include/ttga_lahc.h):
//   tt_lahc  per individual, a walk of Move1 / Move2 candidates that keep hcv 0; a
//            candidate is accepted when it is no worse than the current row or than
//            the row `history` steps ago; the best row seen comes back
// No counterpart in the reference; its call site would follow ga.cpp:574-575. One wave
// (workgroup) per individual; the kernel composes the pieces of tt_lahc_walk.h.
#include "tt_lahc_walk.h"

namespace ttga {

// the plain walk: no chain step and none of the chain's LDS
__global__ __launch_bounds__(64) void lahc_kernel(DevProblem pb, uint8_t* __restrict__ slot, uint8_t* __restrict__ room,
                                                  int64_t* __restrict__ rng, int P, int steps, int L, double p_swap,
                                                  int32_t* __restrict__ scv, int32_t* __restrict__ penalty,
                                                  int32_t* __restrict__ gain, int32_t* __restrict__ accepted,
                                                  int32_t* __restrict__ best_step) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    const int lane = threadIdx.x;
    const long p = blockIdx.x;
    if (p >= P) return;
    const LahcLds m = lahc_carve(kLahcPlain, lds, pb.E, pb.EW64, pb.S, L);
    const LahcOut out{scv, penalty, gain, accepted, best_step, nullptr};
    const LahcEntry in = lahc_enter(pb, m, slot, room, p, steps, L, lane);
    if (in.closed) return lahc_exit_closed(pb, out, 0, p, in, lane);
    LahcWalk w{rng[p]};
    for (int k = 0; k < steps; ++k) {
        lahc_plain_step(pb, m, w, lahc_draw(pb, m, w, p_swap), k, lane);
        lahc_remember(m, w, L);
    }
    lahc_exit_row(m, w, out, slot, room, rng, p, pb.E, lane);
}

}  // namespace ttga

using namespace ttga;

extern "C" int tt_lahc(const tt_problem* p, uint8_t* slot, uint8_t* room, int64_t* rng, int P, int steps, int history,
                       double p_swap, int32_t* scv, int32_t* penalty, int32_t* gain, int32_t* accepted,
                       int32_t* best_step, void* stream) {
    size_t lds = 0;
    int rc = lahc_check_args("tt_lahc", kLahcPlain, p, P, slot, room, rng, steps, history, p_swap, 0.0, 0, 0, &lds);
    if (rc || P == 0) return rc;
    if ((rc = use_device(p))) return rc;
    hipLaunchKernelGGL(lahc_kernel, dim3(P), dim3(64), lds, (hipStream_t)stream, p->dev, slot, room, rng, P, steps,
                       history, p_swap, scv, penalty, gain, accepted, best_step);
    return check_hip(hipGetLastError(), "lahc launch");
}
