// A consumer of include/ttga_cx.h written as the reference's own code is:
// C++98 with the reference's flags (g++ -Wall -ansi -O3), calling every entry
// point of the header. tests/test_cx_cpu.py builds it warning-free, links it
// against libttga.so and runs it: without a GPU tt_problem_create stops at
// TT_ERR_DEVICE and the null-handle checks run; with one, the argument checks
// against a live handle (the device path is exercised by the GPU tests).
#include <cstdio>

#include "ttga_cx.h"
#include "boundary_common_cxx98.h"

int main() {
    Instance in = make_instance();
    int bad = 0;
    tt_problem* tp = NULL;
    int rc = tt_problem_create(in.E, in.R, in.F, in.S, &in.roomSize[0], &in.studentEvents[0], &in.roomFeatures[0],
                               &in.eventFeatures[0], /*device=*/0, &tp);
    uint8_t g[8] = {0};
    int64_t rng[8] = {1};
    int32_t o[8] = {0};
    if (rc == TT_ERR_DEVICE) {
        std::printf("tt_problem_create TT_ERR_DEVICE: %s\n", tt_last_error());
        bad += tt_crossover_guided(NULL, g, g, o, rng, g, g, 1, 0, o, o, NULL) != TT_ERR_INVALID;
        bad += tt_crossover_guided(NULL, NULL, NULL, NULL, NULL, NULL, NULL, -1, 1, NULL, NULL, NULL) != TT_ERR_INVALID;
        bad += tt_ga_breed_guided(NULL, g, g, o, 1, o, rng, 1, 0.8, 0.5, 1, 0, g, g, g, o, o, NULL) != TT_ERR_INVALID;
        bad += tt_ga_breed_guided(NULL, NULL, NULL, NULL, 0, NULL, NULL, -1, 0.8, 0.5, 1, 1, NULL, NULL, NULL, NULL, NULL,
                                  NULL) != TT_ERR_INVALID;
        std::printf("null-handle checks: %d wrong\n", bad);
        return bad ? 10 : TT_ERR_DEVICE;
    }
    if (rc != TT_OK) return fail("tt_problem_create", rc);
    // bad arguments with a live handle are rejected before any launch
    bad += tt_crossover_guided(tp, NULL, g, o, rng, g, g, 1, 0, o, o, NULL) != TT_ERR_INVALID;
    bad += tt_crossover_guided(tp, g, NULL, o, rng, g, g, 1, 0, o, o, NULL) != TT_ERR_INVALID;
    bad += tt_crossover_guided(tp, g, g, NULL, rng, g, g, 1, 0, o, o, NULL) != TT_ERR_INVALID;
    bad += tt_crossover_guided(tp, g, g, o, NULL, g, g, 1, 0, o, o, NULL) != TT_ERR_INVALID;
    bad += tt_crossover_guided(tp, g, g, o, rng, NULL, g, 1, 0, o, o, NULL) != TT_ERR_INVALID;
    bad += tt_crossover_guided(tp, g, g, o, rng, g, NULL, 1, 0, o, o, NULL) != TT_ERR_INVALID;
    bad += tt_crossover_guided(tp, g, g, o, rng, g, g, -1, 0, o, o, NULL) != TT_ERR_INVALID;
    bad += tt_crossover_guided(tp, g, g, o, rng, g, g, 0, 1, NULL, NULL, NULL) != TT_OK;
    bad += tt_ga_breed_guided(tp, NULL, g, o, 1, o, rng, 1, 0.8, 0.5, 1, 0, g, g, g, o, o, NULL) != TT_ERR_INVALID;
    bad += tt_ga_breed_guided(tp, g, g, NULL, 1, o, rng, 1, 0.8, 0.5, 1, 0, g, g, g, o, o, NULL) != TT_ERR_INVALID;
    bad += tt_ga_breed_guided(tp, g, g, o, 0, o, rng, 1, 0.8, 0.5, 1, 0, g, g, g, o, o, NULL) != TT_ERR_INVALID;
    bad += tt_ga_breed_guided(tp, g, g, o, 1, NULL, rng, 1, 0.8, 0.5, 1, 0, g, g, g, o, o, NULL) != TT_ERR_INVALID;
    bad += tt_ga_breed_guided(tp, g, g, o, 1, o, NULL, 1, 0.8, 0.5, 1, 0, g, g, g, o, o, NULL) != TT_ERR_INVALID;
    bad += tt_ga_breed_guided(tp, g, g, o, 1, o, rng, 1, 0.8, 0.5, 1, 0, NULL, g, g, o, o, NULL) != TT_ERR_INVALID;
    bad += tt_ga_breed_guided(tp, g, g, o, 1, o, rng, 1, 0.8, 0.5, 1, 0, g, g, NULL, o, o, NULL) != TT_ERR_INVALID;
    bad += tt_ga_breed_guided(tp, g, g, o, 1, o, rng, -1, 0.8, 0.5, 1, 0, g, g, g, o, o, NULL) != TT_ERR_INVALID;
    bad += tt_ga_breed_guided(tp, g, g, o, 1, o, rng, 0, 0.8, 0.5, 1, 1, g, g, g, NULL, NULL, NULL) != TT_OK;
    std::printf("null-buffer checks: %d wrong\n", bad);
    tt_problem_destroy(tp);
    return bad ? 10 : TT_OK;
}
