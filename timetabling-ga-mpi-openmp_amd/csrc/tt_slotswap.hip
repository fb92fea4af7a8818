// Timeslot-swap descent (include/ttga_slotswap.h):
//   tt_slot_swap  per individual, steepest descent over the 990 pairs of
//                 timeslots: the pair whose exchange lowers scv most trades
//                 its events, until no pair lowers it
// No counterpart in the reference; its call site would follow ga.cpp:574-575.
//
// delta(a, b) over a student's 45-bit attendance mask m, with h(m9) = the >2-in-a-row
// windows plus [exactly one class] of one day's 9 bits:
//   D[s][a]  = h(m_d | bit k) - h(m_d & ~bit k), a = 9d + k: what the day of a pays for
//              student s being in a against not being there (-1..3, an int8)
//   T        = att^T . D  (45 x 45, contracted over the students, att[s][t] = bit t of m_s)
//   a, b on different days: delta = T[b][a] - T[a][a] + T[a][b] - T[b][b] + last-slot term
//   a, b on one day: the day keeps its number of classes, so only its windows of three
//              change, and of those only the ones that hold exactly one of the two
//              positions: there the position's bit is replaced by the other's. With
//              N3[d][t][c] = the students in position t of day d and in both positions
//              of pair column c (columns 0..7: positions i, i + 1; 8..14: i, i + 2),
//              delta = the sum over those windows of N3[other][rest] - N3[own][rest].
//              N3 = att_d^T . Q_d per day, a second contraction over the students
//   last-slot term: (W[b] - W[a]) * ([a % 9 == 8] - [b % 9 == 8]), W[t] = the sum of
//              studentNumber over the events of slot t
// T is an int8 MFMA contraction (v_mfma_i32_32x32x32_i8, 2 x 2 output tiles, operand and
// accumulator layout as derive_corr_kernel's, csrc/tt_derive.hip), N3 five more
// (v_mfma_i32_16x16x64_i8, one 9 x 15 block per day, K = the 64 students of a chunk); every
// pass recomputes the masks, D, T and N3 from the row in LDS.
#include "../../include/ttga_slotswap.h"
#include "tt_internal.h"

namespace ttga {

constexpr int kStatusBadSlotGene = 128;   // tt_device_status bit 7
constexpr int kTStride = 46;              // ints per row of T in LDS
// LDS: attw[48] u64 | pairw[80] u64 | Dt[45][64] i8 | T[45][46] i32 | W[48] i32 | N3[45][16] i32 | slot row
constexpr int kOffPairw = 384, kOffDt = 1024, kOffT = 3904, kOffW = 12184, kOffN3 = 12376, kSwapFixedLds = 15264;
constexpr int kSwapMaxLds = 64 * 1024;

typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v16i __attribute__((ext_vector_type(16)));

// 16 bits -> 16 bytes of 0/1, byte j = bit j (tt_derive.hip)
__device__ __forceinline__ v4i swap_bits_to_bytes(uint32_t h16) {
    v4i v;
#pragma unroll
    for (int d = 0; d < 4; d++) v[d] = (int)((__builtin_amdgcn_ubfe(h16, 4 * d, 4) * 0x00204081u) & 0x01010101u);
    return v;
}

// The windows of day d that hold position k and not `other`, with k's bit replaced by
// other's: window w = k - j holds k, and its other two positions are pair column k + 1
// (j = 0), 7 + k (j = 1: k - 1 and k + 1) or k - 2 (j = 2).
__device__ __forceinline__ int moved_windows(const int32_t* N3, int d, int k, int other) {
    int v = 0;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const int w = k - j;
        const bool on = w >= 0 && w <= 6 && !(other >= w && other <= w + 2);
        const int c = on ? (j == 0 ? k + 1 : j == 1 ? 7 + k : k - 2) : 0;
        const int dv = N3[(9 * d + other) * 16 + c] - N3[(9 * d + k) * 16 + c];
        v += on ? dv : 0;
    }
    return v;
}

__device__ __forceinline__ int is_last(int t) { return (int)((kLastSlotMask >> t) & 1ull); }

// One wave (workgroup) per individual. Lane roles by phase:
//   masks, D     lane = student of the 64-student chunk
//   MFMA         lane (r, h) = row/column r of a 32-wide tile, students 16h.. of a 32-student step
//   same day     MFMA lane (r, g) = row/column r of a day's 16-wide tile, students 16g.. of the chunk;
//                then lane = pair (three rounds of 64 over the 180 pairs) on N3
//   argmin       lane = b - a - 1 for a = 0..43, then the same-day pairs
// Loop bounds: a pass is applied only with delta < 0, so scv falls by at least 1 per
// pass and the descent ends after at most the initial scv passes (or max_passes).
// Two waves per SIMD: without the bound the compiler takes 288 registers and one wave runs
// per SIMD (measured 2 x slower); at three it spills and is slower than at two.
__global__ __launch_bounds__(64, 2) void slot_swap_kernel(DevProblem pb, uint8_t* __restrict__ slot, int P, int max_passes,
                                                       int32_t* __restrict__ scv, int32_t* __restrict__ penalty,
                                                       int32_t* __restrict__ gain, int32_t* __restrict__ passes,
                                                       uint8_t* __restrict__ perm) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    uint64_t* attw = (uint64_t*)lds;
    uint64_t* pairw = (uint64_t*)(lds + kOffPairw);
    int8_t* Dt = (int8_t*)(lds + kOffDt);
    int32_t* T = (int32_t*)(lds + kOffT);
    int32_t* W = (int32_t*)(lds + kOffW);
    int32_t* N3 = (int32_t*)(lds + kOffN3);
    uint8_t* sl = lds + kSwapFixedLds;
    const int E = pb.E, S = pb.S, lane = threadIdx.x;
    const long p = blockIdx.x;
    if (p >= P) return;
    bool bad = false;
    for (int e = lane; e < E; e += 64) {
        const uint8_t v = slot[p * E + e];
        sl[e] = v;
        bad |= v >= kSlots;
    }
    if (lane < 48) W[lane] = 0;
    __syncthreads();
    if (wave_any(bad)) {                               // the row stays as it is
        if (lane == 0) {
            if (gain) gain[p] = 0;
            if (passes) passes[p] = 0;
            atomicOr(pb.status, kStatusBadSlotGene);
        }
        if (perm && lane < kSlots) perm[p * kSlots + lane] = (uint8_t)lane;
        return;
    }
    for (int e = lane; e < E; e += 64) atomicAdd(&W[sl[e]], pb.sn[e]);
    // the same-day pairs of this lane: pair 64 r + lane of 180 = 5 days x 36 (ka < kb)
    int sd_pair[3];                                    // 256 d + 16 ka + kb, -1: no pair
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const int idx = 64 * r + lane, d = idx / 36;
        int ka = 0, rem = idx - 36 * d;
        while (rem >= 8 - ka) { rem -= 8 - ka; ++ka; }
        sd_pair[r] = idx < 180 ? 256 * d + 16 * ka + ka + 1 + rem : -1;
    }
    const int r32 = lane & 31, h = lane >> 5, r16 = lane & 15, g16 = lane >> 4;
    int my_perm = lane, total = 0, applied = 0;
    __syncthreads();
    for (;;) {
        v16i acc[2][2] = {};
        v4i acc3[5] = {};
        for (int s0 = 0; s0 < S; s0 += 64) {
            // attendance mask of student s0 + lane (students past S: 0), four event ids in flight
            const int s = s0 + lane;
            uint64_t m = 0ull;
            if (s < S) {
                const int end = pb.stu_off[s + 1];
                int i = pb.stu_off[s];
                for (; i + 4 <= end; i += 4) {
                    const int e0 = pb.stu_ev[i], e1 = pb.stu_ev[i + 1], e2 = pb.stu_ev[i + 2], e3 = pb.stu_ev[i + 3];
                    m |= (1ull << sl[e0]) | (1ull << sl[e1]) | (1ull << sl[e2]) | (1ull << sl[e3]);
                }
                for (; i < end; ++i) m |= 1ull << sl[pb.stu_ev[i]];
            }
            // bit t of the 64 masks as one word over the students
#pragma unroll
            for (int t = 0; t < kSlots; ++t) {
                const uint64_t w = ballot((m >> t) & 1ull);
                if (lane == t) attw[t] = w;
            }
            // the pair columns: positions i and i + 1 (adj), i and i + 2 (skp) of one day
            const uint64_t adj = m & (m >> 1), skp = m & (m >> 2);
#pragma unroll
            for (int d = 0; d < 5; ++d) {
#pragma unroll
                for (int i = 0; i < 15; ++i) {
                    const uint64_t w = ballot(((i < 8 ? adj >> (9 * d + i) : skp >> (9 * d + i - 8)) & 1ull) != 0ull);
                    if (lane == ((15 * d + i) & 63)) pairw[15 * d + i] = w;
                }
            }
            // D over all 45 positions at once. The windows of three that hold position k with
            // their other two positions attended: k first, k in the middle, k last. The single
            // class: with n = the day's classes without k, [n == 0] - [n == 1].
            const uint64_t t1 = (adj >> 1) & kTripleMask, t2 = (skp & kTripleMask) << 1, t3 = (adj & kTripleMask) << 2;
            uint64_t z = 0ull, o = 0ull, tw = 0ull;              // the days with 0, 1, 2 classes
#pragma unroll
            for (int d = 0; d < 5; ++d) {
                const int cnt = __popc((uint32_t)(m >> (9 * d)) & 0x1FFu);
                const uint64_t day = 0x1FFull << (9 * d);
                z |= cnt == 0 ? day : 0ull;
                o |= cnt == 1 ? day : 0ull;
                tw |= cnt == 2 ? day : 0ull;
            }
            const uint64_t pos = (~m & z) | (m & o), neg = (~m & o) | (m & tw);
#pragma unroll
            for (int a = 0; a < kSlots; ++a)
                Dt[a * 64 + lane] = (int8_t)((int)((t1 >> a) & 1ull) + (int)((t2 >> a) & 1ull) + (int)((t3 >> a) & 1ull) +
                                             (int)((pos >> a) & 1ull) - (int)((neg >> a) & 1ull));
            __syncthreads();
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                if (s0 + 32 * q >= S) break;
                const int sh = 32 * q + 16 * h;
                v4i a_op[2], b_op[2];
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    const int x = 32 * t + r32;
                    const uint64_t w = x < kSlots ? attw[x] : 0ull;
                    a_op[t] = swap_bits_to_bytes((uint32_t)(w >> sh));
                    b_op[t] = x < kSlots ? *(const v4i*)(Dt + x * 64 + sh) : v4i{};
                }
#pragma unroll
                for (int bt = 0; bt < 2; ++bt)
#pragma unroll
                    for (int at = 0; at < 2; ++at)
                        acc[bt][at] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a_op[bt], b_op[at], acc[bt][at], 0, 0, 0);
            }
#pragma unroll
            for (int d = 0; d < 5; ++d) {
                const uint64_t wa = r16 < 9 ? attw[9 * d + r16] : 0ull;
                const uint64_t wb = r16 < 15 ? pairw[15 * d + r16] : 0ull;
                acc3[d] = __builtin_amdgcn_mfma_i32_16x16x64_i8(swap_bits_to_bytes((uint32_t)(wa >> (16 * g16))),
                                                                swap_bits_to_bytes((uint32_t)(wb >> (16 * g16))),
                                                                acc3[d], 0, 0, 0);
            }
            __syncthreads();                            // attw, pairw and Dt are rewritten by the next chunk
        }
        // accumulator register g of lane (r32, h) holds row (g & 3) + 8 (g >> 2) + 4 h, column r32
#pragma unroll
        for (int bt = 0; bt < 2; ++bt)
#pragma unroll
            for (int at = 0; at < 2; ++at)
#pragma unroll
                for (int g = 0; g < 16; ++g) {
                    const int row = 32 * bt + (g & 3) + 8 * (g >> 2) + 4 * h, col = 32 * at + r32;
                    if (row < kSlots && col < kSlots) T[row * kTStride + col] = acc[bt][at][g];
                }
        // 16 x 16 tiles: register g of lane (r16, g16) holds row 4 g16 + g, column r16
#pragma unroll
        for (int d = 0; d < 5; ++d)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int row = 4 * g16 + g;
                if (row < 9 && r16 < 15) N3[(9 * d + row) * 16 + r16] = acc3[d][g];
            }
        __syncthreads();
        // the least (delta, a, b): key = delta * 4096 + 64 a + b
        long long best = 0x7FFFFFFFFFFFFFFFll;
        for (int a = 0; a < kSlots - 1; ++a) {
            const int b = a + 1 + lane;
            if (b < kSlots && b / 9 != a / 9) {
                const int dl = T[b * kTStride + a] + T[a * kTStride + b] - T[a * kTStride + a] - T[b * kTStride + b] +
                               (W[b] - W[a]) * (is_last(a) - is_last(b));
                const long long key = (long long)dl * 4096 + (64 * a + b);
                best = key < best ? key : best;
            }
        }
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            if (sd_pair[r] >= 0) {
                const int d = sd_pair[r] >> 8, ka = (sd_pair[r] >> 4) & 15, kb = sd_pair[r] & 15;
                const int a = 9 * d + ka, b = 9 * d + kb;
                const int dl = moved_windows(N3, d, ka, kb) + moved_windows(N3, d, kb, ka) +
                               (W[b] - W[a]) * (is_last(a) - is_last(b));
                const long long key = (long long)dl * 4096 + (64 * a + b);
                best = key < best ? key : best;
            }
        }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
            const long long other = __shfl_xor(best, o);
            best = other < best ? other : best;
        }
        const int dl = (int)(best >> 12);
        if (dl >= 0) break;
        const int a = (int)(best >> 6) & 63, b = (int)best & 63;
        for (int e = lane; e < E; e += 64) {
            const uint8_t v = sl[e];
            sl[e] = v == a ? (uint8_t)b : v == b ? (uint8_t)a : v;
        }
        if (lane == 0) { const int wa = W[a]; W[a] = W[b]; W[b] = wa; }
        my_perm = my_perm == a ? b : my_perm == b ? a : my_perm;
        total -= dl;
        ++applied;
        __syncthreads();
        if (applied >= max_passes) break;
    }
    if (applied)
        for (int e = lane; e < E; e += 64) slot[p * E + e] = sl[e];
    if (perm && lane < kSlots) perm[p * kSlots + lane] = (uint8_t)my_perm;
    if (lane == 0) {
        if (gain) gain[p] = total;
        if (passes) passes[p] = applied;
        if (scv) scv[p] -= total;
        if (penalty) {
            const int pen = penalty[p];
            if (pen >= 0 && pen < 1000000) penalty[p] = pen - total;
        }
    }
}

}  // namespace ttga

using namespace ttga;

extern "C" int tt_slot_swap(const tt_problem* p, uint8_t* slot, int P, int max_passes, int32_t* scv, int32_t* penalty,
                            int32_t* gain, int32_t* passes, uint8_t* perm, void* stream) {
    int rc = check_pop_args(p, P, slot, slot);
    if (rc) return rc;
    if (max_passes < 1) { set_error("tt_slot_swap: max_passes must be at least 1"); return TT_ERR_INVALID; }
    if (P == 0) return TT_OK;
    const size_t lds = (size_t)kSwapFixedLds + (size_t)p->E;
    if (lds > (size_t)kSwapMaxLds) {
        set_error("instance too large for the timeslot swap");
        return TT_ERR_LIMIT;
    }
    if ((rc = check_rows_grid("tt_slot_swap", p, P, false))) return rc;
    if ((rc = use_device(p))) return rc;
    hipLaunchKernelGGL(slot_swap_kernel, dim3(P), dim3(64), lds, (hipStream_t)stream, p->dev, slot, P, max_passes, scv,
                       penalty, gain, passes, perm);
    return check_hip(hipGetLastError(), "slot swap launch");
}
