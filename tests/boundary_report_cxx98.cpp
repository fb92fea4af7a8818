// A consumer of include/ttga_report.h written as the reference's own code is:
// C++98 with the reference's flags (g++ -Wall -ansi -O3), calling both report
// entry points. tests/test_report_cpu.py builds it warning-free, links it
// against libttga.so and runs it: without a GPU tt_problem_create stops at
// TT_ERR_DEVICE and the null-handle checks run; with one, the null-buffer
// checks against a live handle (the device path is exercised by the GPU tests).
#include <cstdio>

#include "ttga_report.h"
#include "boundary_common_cxx98.h"

int main() {
    Instance in = make_instance();
    tt_problem* tp = NULL;
    int rc = tt_problem_create(in.E, in.R, in.F, in.S, &in.roomSize[0], &in.studentEvents[0], &in.roomFeatures[0],
                               &in.eventFeatures[0], /*device=*/0, &tp);
    if (rc == TT_ERR_DEVICE) {
        std::printf("tt_problem_create TT_ERR_DEVICE: %s\n", tt_last_error());
        int bad = 0;
        bad += tt_eval_parts(NULL, NULL, NULL, 1, NULL, NULL, NULL) != TT_ERR_INVALID;
        bad += tt_slot_histogram(NULL, NULL, 1, NULL, NULL) != TT_ERR_INVALID;
        std::printf("null-handle checks: %d wrong\n", bad);
        return bad ? 10 : TT_ERR_DEVICE;
    }
    if (rc != TT_OK) return fail("tt_problem_create", rc);
    // null buffers with a live handle are rejected before any launch
    int bad = 0;
    int32_t dummy[TT_NUM_PARTS];
    uint8_t genes[1] = {0};
    bad += tt_eval_parts(tp, NULL, genes, 1, dummy, NULL, NULL) != TT_ERR_INVALID;
    bad += tt_eval_parts(tp, genes, NULL, 1, dummy, NULL, NULL) != TT_ERR_INVALID;
    bad += tt_eval_parts(tp, genes, genes, 1, NULL, NULL, NULL) != TT_ERR_INVALID;
    bad += tt_eval_parts(tp, genes, genes, -1, dummy, NULL, NULL) != TT_ERR_INVALID;
    bad += tt_eval_parts(tp, NULL, NULL, 0, NULL, NULL, NULL) != TT_OK;
    bad += tt_slot_histogram(tp, NULL, 1, dummy, NULL) != TT_ERR_INVALID;
    bad += tt_slot_histogram(tp, genes, 1, NULL, NULL) != TT_ERR_INVALID;
    bad += tt_slot_histogram(tp, genes, -1, dummy, NULL) != TT_ERR_INVALID;
    std::printf("null-buffer checks: %d wrong, %d parts (%d..%d)\n", bad, TT_NUM_PARTS, TT_PART_ROOM_PAIRS,
                TT_PART_SINGLE_CLASS);
    tt_problem_destroy(tp);
    return bad ? 10 : TT_OK;
}
