// A consumer of include/ttga_greedy.h written as the reference's own code is:
// C++98 with the reference's flags (g++ -Wall -ansi -O3), calling every entry
// point of the header. tests/test_greedy_cpu.py builds it warning-free, links
// it against libttga.so and runs it: without a GPU tt_problem_create stops at
// TT_ERR_DEVICE and the null-handle checks run; with one, the argument checks
// against a live handle (the device path is exercised by the GPU tests).
#include <cstdio>

#include "ttga_greedy.h"
#include "boundary_common_cxx98.h"

int main() {
    Instance in = make_instance();
    int bad = 0;
    bad += tt_greedy_work_bytes(NULL) != 0;
    tt_problem* tp = NULL;
    int rc = tt_problem_create(in.E, in.R, in.F, in.S, &in.roomSize[0], &in.studentEvents[0], &in.roomFeatures[0],
                               &in.eventFeatures[0], /*device=*/0, &tp);
    uint8_t genes[8] = {0};
    int32_t order[8] = {0};
    int64_t rng[8] = {0};
    if (rc == TT_ERR_DEVICE) {
        std::printf("tt_problem_create TT_ERR_DEVICE: %s\n", tt_last_error());
        bad += tt_greedy_order(NULL, order, genes, NULL) != TT_ERR_INVALID;
        bad += tt_greedy_init(NULL, order, rng, genes, genes, 1, NULL) != TT_ERR_INVALID;
        std::printf("null-handle checks: %d wrong\n", bad);
        return bad ? 10 : TT_ERR_DEVICE;
    }
    if (rc != TT_OK) return fail("tt_problem_create", rc);
    // bad arguments with a live handle are rejected before any launch
    bad += tt_greedy_work_bytes(tp) < 8 * 70;
    bad += tt_greedy_order(tp, NULL, genes, NULL) != TT_ERR_INVALID;
    bad += tt_greedy_order(tp, order, NULL, NULL) != TT_ERR_INVALID;
    bad += tt_greedy_init(tp, NULL, rng, genes, genes, 1, NULL) != TT_ERR_INVALID;
    bad += tt_greedy_init(tp, order, NULL, genes, genes, 1, NULL) != TT_ERR_INVALID;
    bad += tt_greedy_init(tp, order, rng, NULL, genes, 1, NULL) != TT_ERR_INVALID;
    bad += tt_greedy_init(tp, order, rng, genes, NULL, 1, NULL) != TT_ERR_INVALID;
    bad += tt_greedy_init(tp, order, rng, genes, genes, -1, NULL) != TT_ERR_INVALID;
    bad += tt_greedy_init(tp, order, rng, genes, genes, 0, NULL) != TT_OK;
    std::printf("null-buffer checks: %d wrong\n", bad);
    tt_problem_destroy(tp);
    return bad ? 10 : TT_OK;
}
