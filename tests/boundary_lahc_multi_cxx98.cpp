// A consumer of tt_lahc_multi and tt_lahc_multi_work_bytes (include/ttga_lahc_multi.h,
// through ttga_lahc.h) written as the reference's own code is: C++98 with the reference's
// flags (g++ -Wall -ansi -O3). tests/test_lahc_multi_cpu.py builds it warning-free, links
// it against libttga.so and runs it: without a GPU tt_problem_create stops at
// TT_ERR_DEVICE and the null-handle checks run; with one, the argument checks
// against a live handle (the device path is exercised by the GPU tests).
#include <cstdio>

#include "ttga_lahc.h"
#include "boundary_common_cxx98.h"

namespace {

// one call with the arguments that vary; every output goes to `out`
int call(const tt_problem* tp, uint8_t* slot, uint8_t* room, int64_t* rng, int P, int walkers, int steps, int history,
         double p_swap, double p_kempe, int max_chain, int room_rule, int32_t* out, void* work) {
    return tt_lahc_multi(tp, slot, room, rng, P, walkers, steps, history, p_swap, p_kempe, max_chain, room_rule, out,
                         out, out, out, out, out, out, out, work, NULL);
}

}  // namespace

int main() {
    Instance in = make_instance();
    int bad = 0;
    tt_problem* tp = NULL;
    int rc = tt_problem_create(in.E, in.R, in.F, in.S, &in.roomSize[0], &in.studentEvents[0], &in.roomFeatures[0],
                               &in.eventFeatures[0], /*device=*/0, &tp);
    uint8_t genes[8] = {0};
    int64_t rng[8] = {1};
    int32_t out[8] = {0};
    int64_t work[8] = {0};
    if (rc == TT_ERR_DEVICE) {
        std::printf("tt_problem_create TT_ERR_DEVICE: %s\n", tt_last_error());
        bad += call(NULL, genes, genes, rng, 1, 4, 10, 5, 0.25, 0.5, 0, 1, out, work) != TT_ERR_INVALID;
        bad += call(NULL, NULL, NULL, NULL, -1, 0, -1, 0, 2.0, 0.5, 0, 1, NULL, NULL) != TT_ERR_INVALID;
        bad += tt_lahc_multi_work_bytes(NULL, 1, 4) != 0;
        std::printf("null-handle checks: %d wrong\n", bad);
        return bad ? 10 : TT_ERR_DEVICE;
    }
    if (rc != TT_OK) return fail("tt_problem_create", rc);
    // the work buffer: 8 P + (48 + 2 E) P walkers bytes, 0 for arguments the call refuses
    bad += tt_lahc_multi_work_bytes(tp, 3, 4) != (size_t)(8 * 3 + (48 + 2 * in.E) * 3 * 4);
    bad += tt_lahc_multi_work_bytes(tp, 0, 4) != 0;
    bad += tt_lahc_multi_work_bytes(tp, -1, 4) != 0;
    bad += tt_lahc_multi_work_bytes(tp, 3, 0) != 0;
    bad += tt_lahc_multi_work_bytes(tp, 3, 1025) != 0;
    bad += tt_lahc_multi_work_bytes(tp, 2147483647, 2) != 0;
    bad += tt_lahc_multi_work_bytes(NULL, 3, 4) != 0;
    // bad arguments with a live handle are rejected before any launch
    bad += call(tp, NULL, genes, rng, 1, 4, 10, 5, 0.25, 0.5, 0, 1, out, work) != TT_ERR_INVALID;
    bad += call(tp, genes, NULL, rng, 1, 4, 10, 5, 0.25, 0.5, 0, 1, out, work) != TT_ERR_INVALID;
    bad += call(tp, genes, genes, NULL, 1, 4, 10, 5, 0.25, 0.5, 0, 1, out, work) != TT_ERR_INVALID;
    bad += call(tp, genes, genes, rng, -1, 4, 10, 5, 0.25, 0.5, 0, 1, out, work) != TT_ERR_INVALID;
    bad += call(tp, genes, genes, rng, 1, 0, 10, 5, 0.25, 0.5, 0, 1, out, work) != TT_ERR_INVALID;
    bad += call(tp, genes, genes, rng, 1, -3, 10, 5, 0.25, 0.5, 0, 1, out, work) != TT_ERR_INVALID;
    bad += call(tp, genes, genes, rng, 1, 1025, 10, 5, 0.25, 0.5, 0, 1, out, work) != TT_ERR_INVALID;
    bad += call(tp, genes, genes, rng, 1, 4, 10, 5, 0.25, 0.5, 0, 1, out, NULL) != TT_ERR_INVALID;
    bad += call(tp, genes, genes, rng, 1, 4, -1, 5, 0.25, 0.5, 0, 1, out, work) != TT_ERR_INVALID;
    bad += call(tp, genes, genes, rng, 1, 4, 10, 0, 0.25, 0.5, 0, 1, out, work) != TT_ERR_INVALID;
    bad += call(tp, genes, genes, rng, 1, 4, 10, 5, 1.5, 0.5, 0, 1, out, work) != TT_ERR_INVALID;
    bad += call(tp, genes, genes, rng, 1, 4, 10, 5, 0.25, -0.5, 0, 1, out, work) != TT_ERR_INVALID;
    bad += call(tp, genes, genes, rng, 1, 4, 10, 5, 0.25, 0.5, -1, 1, out, work) != TT_ERR_INVALID;
    bad += call(tp, genes, genes, rng, 1, 4, 10, 5, 0.75, 0.5, 0, 1, out, work) != TT_ERR_INVALID;
    bad += call(tp, genes, genes, rng, 1, 4, 10, 5, 0.25, 0.5, 0, 2, out, work) != TT_ERR_INVALID;
    bad += call(tp, genes, genes, rng, 0, 4, 10, 5, 0.25, 0.5, 0, -1, NULL, work) != TT_ERR_INVALID;
    bad += call(tp, genes, genes, rng, 1, 4, 10, 20000, 0.25, 0.5, 0, 1, out, work) != TT_ERR_LIMIT;
    bad += call(tp, genes, genes, rng, 2147483647, 2, 10, 5, 0.25, 0.5, 0, 1, out, work) != TT_ERR_LIMIT;
    bad += call(tp, genes, genes, rng, 0, 4, 10, 5, 0.25, 0.5, 0, 1, NULL, work) != TT_OK;
    bad += call(tp, genes, genes, rng, 0, 1, 10, 5, 0.25, 0.5, 0, 0, NULL, NULL) != TT_OK;
    std::printf("null-buffer checks: %d wrong\n", bad);
    tt_problem_destroy(tp);
    return bad ? 10 : TT_OK;
}
