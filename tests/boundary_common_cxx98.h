// What the stage consumers (tests/boundary_*_cxx98.cpp) share: the instance
// they hand to tt_problem_create and the report of a call that failed. C++98,
// clean under g++ -Wall -ansi -O3 -pedantic -Werror. The functions are inline,
// so a consumer that calls only one of them still builds warning-free.
#ifndef TTGA_TESTS_BOUNDARY_COMMON_CXX98_H
#define TTGA_TESTS_BOUNDARY_COMMON_CXX98_H

#include <cstdio>
#include <vector>

#include "ttga.h"

struct Instance {
    int E, R, F, S;
    std::vector<int32_t> roomSize, studentEvents, roomFeatures, eventFeatures;
};

inline Instance make_instance() {
    Instance in;
    in.E = 70; in.R = 3; in.F = 2; in.S = 40;
    in.roomSize.assign(in.R, 40);
    in.studentEvents.resize(in.S * in.E);
    in.roomFeatures.assign(in.R * in.F, 1);
    in.eventFeatures.assign(in.E * in.F, 0);
    for (int s = 0; s < in.S; ++s)
        for (int e = 0; e < in.E; ++e) in.studentEvents[s * in.E + e] = (s * 7 + e * 3) % 11 == 0;
    return in;
}

inline int fail(const char* what, int rc) {
    std::printf("%s rc=%d: %s\n", what, rc, tt_last_error());
    return rc ? rc : 10;
}

#endif
