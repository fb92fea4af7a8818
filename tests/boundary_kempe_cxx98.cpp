// A consumer of include/ttga_kempe.h written as the reference's own code is:
// C++98 with the reference's flags (g++ -Wall -ansi -O3), calling every entry
// point of the header. tests/test_kempe_cpu.py builds it warning-free, links
// it against libttga.so and runs it: without a GPU tt_problem_create stops at
// TT_ERR_DEVICE and the null-handle checks run; with one, the argument checks
// against a live handle (the device path is exercised by the GPU tests).
#include <cstdio>

#include "ttga_kempe.h"
#include "boundary_common_cxx98.h"

int main() {
    Instance in = make_instance();
    int bad = 0;
    tt_problem* tp = NULL;
    int rc = tt_problem_create(in.E, in.R, in.F, in.S, &in.roomSize[0], &in.studentEvents[0], &in.roomFeatures[0],
                               &in.eventFeatures[0], /*device=*/0, &tp);
    uint8_t genes[8] = {0};
    int64_t rng[8] = {0};
    int32_t len[8] = {0};
    if (rc == TT_ERR_DEVICE) {
        std::printf("tt_problem_create TT_ERR_DEVICE: %s\n", tt_last_error());
        bad += tt_kempe_move(NULL, genes, genes, rng, 1, 0.5, 0, len, NULL) != TT_ERR_INVALID;
        bad += tt_kempe_move(NULL, NULL, NULL, NULL, -1, 2.0, -1, NULL, NULL) != TT_ERR_INVALID;
        std::printf("null-handle checks: %d wrong\n", bad);
        return bad ? 10 : TT_ERR_DEVICE;
    }
    if (rc != TT_OK) return fail("tt_problem_create", rc);
    // bad arguments with a live handle are rejected before any launch
    bad += tt_kempe_move(tp, NULL, genes, rng, 1, 0.5, 0, len, NULL) != TT_ERR_INVALID;
    bad += tt_kempe_move(tp, genes, NULL, rng, 1, 0.5, 0, len, NULL) != TT_ERR_INVALID;
    bad += tt_kempe_move(tp, genes, genes, NULL, 1, 0.5, 0, len, NULL) != TT_ERR_INVALID;
    bad += tt_kempe_move(tp, genes, genes, rng, -1, 0.5, 0, len, NULL) != TT_ERR_INVALID;
    bad += tt_kempe_move(tp, genes, genes, rng, 1, 0.5, -1, len, NULL) != TT_ERR_INVALID;
    bad += tt_kempe_move(tp, genes, genes, rng, 1, -0.1, 0, len, NULL) != TT_ERR_INVALID;
    bad += tt_kempe_move(tp, genes, genes, rng, 1, 1.5, 0, len, NULL) != TT_ERR_INVALID;
    bad += tt_kempe_move(tp, genes, genes, rng, 0, 0.5, 0, NULL, NULL) != TT_OK;
    std::printf("null-buffer checks: %d wrong\n", bad);
    tt_problem_destroy(tp);
    return bad ? 10 : TT_OK;
}
