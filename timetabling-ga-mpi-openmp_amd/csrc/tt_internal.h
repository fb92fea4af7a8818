// Host-side internals shared by the C-ABI translation units.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <atomic>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/ttga.h"
#include "tt_common.h"

struct tt_problem {
    int E, R, F, S, device, num_cus;
    // host copies (tt_problem_derived, validation)
    std::vector<int32_t> student_number;
    std::vector<uint64_t> poss_bits;
    std::vector<uint32_t> corr_bits;
    int nnz_students;
    // device allocations
    void* dev_block;
    ttga::DevProblem dev;
    // local search redo lists, one per stream (count, done counter, entries):
    // zeroed once when allocated, reset on the device by the redo launch;
    // ls_mu is held while a call enqueues its launches, so two host threads on
    // one stream cannot interleave their first and redo launches
    struct LsRedo {
        void* stream;
        int32_t* list;
        int cap;
        // phase-2 steps and all steps of the stream's local-search calls: counted
        // on the device (ph_dev), copied after call k into pinned host memory
        // ph_host[2 (k & 1) ..] with event ev[k & 1] recorded behind the copy;
        // call k + 2 waits for that event and decides the phase-2 student masks'
        // launch from those counts (tt_ls.hip), so a launch's shape depends only
        // on the sequence of calls, never on host/device timing
        unsigned long long* ph_dev = nullptr;
        volatile unsigned long long* ph_host = nullptr;
        hipEvent_t ev[2] = {nullptr, nullptr};
        long calls = 0;
        int sms_last = 0;        // students with masks in the last call's first launch
    };
    std::vector<LsRedo> ls_redo;
    std::mutex ls_mu;
    // students with phase-2 masks in the local search, per matcher-task cap
    // (full, small); -1 until the first call decides (tt_ls.hip ls_mask_students)
    std::atomic<int> ls_smask[2] = {-1, -1};
    // eval_tile5 launch decisions, per wave count (4, 8) and tile buffers (1, 2):
    // workgroups per CU, -1 until the first launch asks (tt_eval.hip); and the
    // largest studentNumber (packing choice), set at creation
    std::atomic<int> t5_occ[2][2] = {{-1, -1}, {-1, -1}};
    int max_sn = 0;
};

namespace ttga {

void set_error(const std::string& msg);

// Returns TT_OK or records the HIP error and returns TT_ERR_DEVICE.
int check_hip(hipError_t e, const char* what);

#define TT_HIP(call)                                         \
    do {                                                     \
        int _rc = ::ttga::check_hip((call), #call);          \
        if (_rc != TT_OK) return _rc;                        \
    } while (0)

// Workgroups of `lds_bytes` of LDS each that one gfx950 CU actually keeps
// resident: LDS is allocated in blocks of 1,280 B (160 KB / 128), which
// hipOccupancyMaxActiveBlocksPerMultiprocessor does not model (it divides
// 160 KB by the size rounded to 256 B: 20 against the real 18 at 8,032 B).
// Measured by tools/occ_probe.hip (profiles/r05_occ_sweep.jsonl).
inline int lds_resident_limit(size_t lds_bytes) {
    const size_t blocks = (lds_bytes + 1279) / 1280;
    return blocks == 0 ? 1 << 30 : (int)(128 / blocks);
}

// HIP runs no launch whose gridDim.x * blockDim.x passes 2^32 - 1 in full: an
// exact multiple of 2^32 is refused (hipErrorInvalidConfiguration), anything
// else is accepted with hipSuccess and runs the product modulo 2^32 threads
// (2^24 + 3 workgroups of 256: three of them), a silent wrong result. An entry
// point whose grid grows with the population therefore asks before its first launch:
// TT_OK, or TT_ERR_LIMIT with nothing launched and every buffer untouched
// (include/ttga.h, "Population size").
constexpr long long kMaxGridThreads = 0xFFFFFFFFll;
inline int check_grid(const char* fn, long long blocks, int threads) {
    if (blocks * threads <= kMaxGridThreads) return TT_OK;
    set_error(std::string(fn) + ": population too large for one launch (" + std::to_string(blocks) +
              " workgroups of " + std::to_string(threads) + " threads; at most " +
              std::to_string(kMaxGridThreads / threads) + ")");
    return TT_ERR_LIMIT;
}

// check_grid for a call that gives every one of `rows` rows a workgroup of one
// wave, and with `rooms` also one of assign_rooms_kernel's, which has
// kAssignWideThreads threads in the matcher's wide layout (R > 16, tt_match.h;
// tt_rooms.hip asserts both).
constexpr int kAssignWideThreads = 256;
inline int check_rows_grid(const char* fn, const tt_problem* p, long long rows, bool rooms) {
    return check_grid(fn, rows, rooms && p->R > 16 ? kAssignWideThreads : 64);
}

// Common argument checks for population entry points.
int check_pop_args(const tt_problem* p, int P, const void* a, const void* b);

// Makes the handle's device current for the calling thread.
int use_device(const tt_problem* p);

// Bit image of the attendance matrix for the device derivation: Ep = E rounded
// up to 64 event rows of SW u32 words, Sp = S rounded up to 128 students (one
// 16-B load per lane per chunk).
struct DeriveLayout {
    int Ep, Sp, SW;
};
inline DeriveLayout derive_layout(int E, int S) {
    DeriveLayout L;
    L.Ep = (E + 63) & ~63;
    L.Sp = (S + 127) & ~127;
    L.SW = L.Sp / 32;
    return L;
}

// studentNumber, eventCorrelations (corr, corr64, cupT) and possibleRooms of
// the image, derived on the handle's (current) device from the attendance bit
// rows atb[Ep][SW] (derive_layout; csrc/tt_derive.hip); synchronous.
int derive_on_device(const tt_problem* p, const uint32_t* atb, const int32_t* room_size, const uint64_t* efw,
                     const uint64_t* rfw, int FW);

// eval_tile5's packing of possibleRooms and studentNumber (its PK template
// argument), fixed per problem: 1 = one u32 per event (R <= 16 and every
// studentNumber < 65536), 2 = u32 room mask (R <= 32), 0 = u64 room mask.
inline int t5_pk(int R, int max_sn) { return (R <= 16 && max_sn <= 0xFFFF) ? 1 : R <= 32 ? 2 : 0; }

// eval_tile5's invariant image (DevProblem::t5_img, EW64 <= 7 only): what every
// lane of the kernel keeps in registers for a whole launch, laid out so that a
// wave reads each register's 64 values as one contiguous row, with no bounds
// test and no index arithmetic. EWC = EW64, e = 64 r + lane:
//  * correlation rows, 512 B each, r-major then w (r <= w < F; F = EWC at TP 1,
//    EWC - 1 with a packed tail, t5_tp in tt_common.h):
//      row (r, w)[lane] = cupT[w * E + e], 0 for e >= E;
//  * packed tail rows (TP > 1), 512 B each, k = 0..ceil(EWC/TP)-1, in place of the
//    rows (r, EWC-1): with j = 64 (EWC-1) + (lane & (64/TP - 1)) and
//    wd = lane / (64/TP) + TP k,
//      row k[lane] bit i = corr(j, 64 wd + i) for wd < EWC-1,
//                          corr(j, 64 wd + i) and i > j - 64 (EWC-1) for wd = EWC-1
//                          (the diagonal block), 0 for j >= E or wd >= EWC;
//  * per-event rows of the problem's PK form (t5_pk), event word r = 0..EWC-1:
//      PK 1: u32 rows   (~possibleRooms & 0xFFFF) | studentNumber << 16, 0 for e >= E;
//      PK 2: u32 rows   possibleRooms (all ones for e >= E),
//            then i32 rows studentNumber (0 for e >= E);
//      PK 0: u64 rows   possibleRooms (all ones for e >= E), then i32 rows studentNumber.
// t5_img_bytes(EWC, PK, TP) bytes (13,568 at E = 400, R = 10), a multiple of 256. The
// image lives in the handle's device block, is written once by build_t5_image
// after derive_on_device (cupT, possibleRooms and studentNumber are
// device-derived) and is immutable afterwards. Synchronous.
int build_t5_image(tt_problem* p);

}  // namespace ttga
