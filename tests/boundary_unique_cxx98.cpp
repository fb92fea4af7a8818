// A consumer of include/ttga_unique.h written as the reference's own code is:
// C++98 with the reference's flags (g++ -Wall -ansi -O3), calling every entry
// point of the header. tests/test_unique_cpu.py builds it warning-free, links
// it against libttga.so and runs it: without a GPU tt_problem_create stops at
// TT_ERR_DEVICE and the null-handle checks run; with one, the argument checks
// against a live handle (the device path is exercised by the GPU tests).
#include <cstdio>

#include "ttga_unique.h"
#include "boundary_common_cxx98.h"

namespace {

// tt_ga_replace_unique with one buffer for every pointer argument (none is
// touched: the calls below are rejected before any device call)
int replace_unique(const tt_problem* tp, uint8_t* g, int32_t* m, int N, int C, int hash_bits, void* work) {
    return tt_ga_replace_unique(tp, g, g, m, m, g, m, N, g, g, m, m, g, m, C, g, m, hash_bits, work, NULL);
}

}  // namespace

int main() {
    Instance in = make_instance();
    int bad = 0;
    bad += tt_genome_work_bytes(0, 70) != 0;
    bad += tt_genome_work_bytes(5, 0) != 0;
    bad += tt_genome_work_bytes(5, 70) == 0;
    bad += tt_ga_unique_work_bytes(0, 0, 70) != 0;
    bad += tt_ga_unique_work_bytes(10, -1, 70) != 0;
    bad += tt_ga_unique_work_bytes(10, 2, 70) < tt_ga_work_bytes(10, 70);
    tt_problem* tp = NULL;
    int rc = tt_problem_create(in.E, in.R, in.F, in.S, &in.roomSize[0], &in.studentEvents[0], &in.roomFeatures[0],
                               &in.eventFeatures[0], /*device=*/0, &tp);
    uint8_t genes[8] = {0};
    int32_t meta[8] = {0};
    if (rc == TT_ERR_DEVICE) {
        std::printf("tt_problem_create TT_ERR_DEVICE: %s\n", tt_last_error());
        bad += tt_genome_first(NULL, genes, genes, 1, meta, 0, genes, NULL) != TT_ERR_INVALID;
        bad += replace_unique(NULL, genes, meta, 1, 1, 0, genes) != TT_ERR_INVALID;
        std::printf("null-handle checks: %d wrong\n", bad);
        return bad ? 10 : TT_ERR_DEVICE;
    }
    if (rc != TT_OK) return fail("tt_problem_create", rc);
    // bad arguments with a live handle are rejected before any launch
    bad += tt_genome_first(tp, NULL, genes, 1, meta, 0, genes, NULL) != TT_ERR_INVALID;
    bad += tt_genome_first(tp, genes, genes, 1, NULL, 0, genes, NULL) != TT_ERR_INVALID;
    bad += tt_genome_first(tp, genes, genes, 1, meta, 0, NULL, NULL) != TT_ERR_INVALID;
    bad += tt_genome_first(tp, genes, genes, -1, meta, 0, genes, NULL) != TT_ERR_INVALID;
    bad += tt_genome_first(tp, genes, genes, 1, meta, 32, genes, NULL) != TT_ERR_INVALID;
    bad += tt_genome_first(tp, genes, genes, 1, meta, -1, genes, NULL) != TT_ERR_INVALID;
    bad += tt_genome_first(tp, NULL, NULL, 0, NULL, 0, NULL, NULL) != TT_OK;
    bad += replace_unique(tp, genes, meta, 0, 0, 0, genes) != TT_ERR_INVALID;
    bad += replace_unique(tp, genes, meta, 1, 2, 0, genes) != TT_ERR_INVALID;
    bad += replace_unique(tp, genes, meta, 1, -1, 0, genes) != TT_ERR_INVALID;
    bad += replace_unique(tp, genes, meta, 1, 1, 32, genes) != TT_ERR_INVALID;
    bad += replace_unique(tp, genes, meta, 1, 1, 0, NULL) != TT_ERR_INVALID;
    std::printf("null-buffer checks: %d wrong\n", bad);
    tt_problem_destroy(tp);
    return bad ? 10 : TT_OK;
}
