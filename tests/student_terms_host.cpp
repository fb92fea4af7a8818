// Host check of eval_tile5's per-student terms (mask_scv_shift5, csrc/tt_common.h: the
// function the kernel's lane phase calls, compiled here for the host) against the
// mask_scv formula: built and run by tests/test_student_terms_cpu.py (host code only).
// A student's 45-bit attendance mask m goes in as the kernel builds it, every slot s as
// kShift5One << s, so m << 5; the sentinel column's slot byte 63 shifts out of the word.
#include <cstdint>
#include <cstdio>

#include "tt_common.h"

using namespace ttga;

// mask_scv (tt_common.h, device only) restated for the host
static int formula(uint64_t m) {
    int sc = __builtin_popcountll(m & (m >> 1) & (m >> 2) & kTripleMask);
    for (int d = 0; d < 5; ++d) sc += __builtin_popcount((uint32_t)(m >> (9 * d)) & 0x1FFu) == 1;
    return sc;
}

// the kernel's mask of the slots in m (bit 63: the sentinel column's byte)
static uint64_t shifted(uint64_t m) {
    uint64_t r = 0;
    for (int s = 0; s < 64; ++s)
        if ((m >> s) & 1) r |= kShift5One << s;
    return r;
}

static long checked = 0, failed = 0;
static void check(uint64_t m) {
    ++checked;
    const int got = mask_scv_shift5(shifted(m)), want = formula(m & ((1ull << 45) - 1));
    if (got != want && ++failed <= 8) std::printf("mask %016llx: word form %d formula %d\n", (unsigned long long)m, got, want);
}

int main() {
    // every field in every day position: the other days empty, then full, each with the
    // sentinel's bit 63 clear and set
    const uint64_t all45 = (1ull << 45) - 1;
    for (int d = 0; d < 5; ++d)
        for (uint64_t f = 0; f < 512; ++f) {
            const uint64_t day = 0x1FFull << (9 * d), m0 = f << (9 * d), m1 = (all45 & ~day) | m0;
            check(m0); check(m1); check(m0 | 1ull << 63); check(m1 | 1ull << 63);
        }
    // seeded random 45-bit masks, dense and sparse, bit 63 clear and set
    uint64_t s = 0x9E3779B97F4A7C15ull;
    auto next = [&s]() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s; };
    for (int i = 0; i < 120000; ++i) {
        const uint64_t r = next(), m = (i & 1 ? r : r & next() & next()) & all45;
        check(m); check(m | 1ull << 63);
    }
    std::printf("checked %ld masks, %ld failed\n", checked, failed);
    return failed ? 1 : 0;
}
