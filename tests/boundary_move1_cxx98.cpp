// A consumer of include/ttga/move1.h written as the reference's own code is:
// C++98 with the reference's flags (g++ -Wall -ansi -O3), calling every entry
// point of the header. tests/test_move1_cpu.py builds it warning-free, links
// it against libttga.so and runs it: without a GPU tt_problem_create stops at
// TT_ERR_DEVICE and the null-handle checks run; with one, the argument checks
// against a live handle (the device path is exercised by the GPU tests).
#include <cstdio>

#include "ttga/move1.h"
#include "boundary_common_cxx98.h"

int main() {
    Instance in = make_instance();
    int bad = 0;
    tt_problem* tp = NULL;
    int rc = tt_problem_create(in.E, in.R, in.F, in.S, &in.roomSize[0], &in.studentEvents[0], &in.roomFeatures[0],
                               &in.eventFeatures[0], /*device=*/0, &tp);
    uint8_t genes[8] = {0};
    int32_t out[8] = {0};
    if (rc == TT_ERR_DEVICE) {
        std::printf("tt_problem_create TT_ERR_DEVICE: %s\n", tt_last_error());
        bad += tt_move1_scan(NULL, genes, genes, 1, out, out, genes, NULL) != TT_ERR_INVALID;
        bad += tt_move1_scan(NULL, NULL, NULL, -1, NULL, NULL, NULL, NULL) != TT_ERR_INVALID;
        bad += tt_move1_descent(NULL, genes, genes, 1, 1, out, out, out, out, NULL) != TT_ERR_INVALID;
        bad += tt_move1_descent(NULL, NULL, NULL, -1, 0, NULL, NULL, NULL, NULL, NULL) != TT_ERR_INVALID;
        std::printf("null-handle checks: %d wrong\n", bad);
        return bad ? 10 : TT_ERR_DEVICE;
    }
    if (rc != TT_OK) return fail("tt_problem_create", rc);
    // bad arguments with a live handle are rejected before any launch
    bad += tt_move1_scan(tp, NULL, genes, 1, out, out, genes, NULL) != TT_ERR_INVALID;
    bad += tt_move1_scan(tp, genes, NULL, 1, out, out, genes, NULL) != TT_ERR_INVALID;
    bad += tt_move1_scan(tp, genes, genes, -1, out, out, genes, NULL) != TT_ERR_INVALID;
    bad += tt_move1_scan(tp, genes, genes, 0, NULL, NULL, NULL, NULL) != TT_OK;
    bad += tt_move1_scan(tp, genes, genes, 1, NULL, NULL, NULL, NULL) != TT_OK;      // no output: no launch
    bad += tt_move1_descent(tp, NULL, genes, 1, 1, out, out, out, out, NULL) != TT_ERR_INVALID;
    bad += tt_move1_descent(tp, genes, NULL, 1, 1, out, out, out, out, NULL) != TT_ERR_INVALID;
    bad += tt_move1_descent(tp, genes, genes, -1, 1, out, out, out, out, NULL) != TT_ERR_INVALID;
    bad += tt_move1_descent(tp, genes, genes, 1, 0, out, out, out, out, NULL) != TT_ERR_INVALID;
    bad += tt_move1_descent(tp, genes, genes, 1, -1, out, out, out, out, NULL) != TT_ERR_INVALID;
    bad += tt_move1_descent(tp, genes, genes, 0, 1, NULL, NULL, NULL, NULL, NULL) != TT_OK;
    std::printf("null-buffer checks: %d wrong\n", bad);
    tt_problem_destroy(tp);
    return bad ? 10 : TT_OK;
}
