// Population report (include/ttga_report.h): the six constraint parts of every
// individual (the terms tt_eval adds up into hcv and scv, kept apart), the
// per-event conflict count Solution::eventHcv (Solution.cpp:173-191) and the
// per-event histogram of slot assignments over a population.
//
//   hard parts (Solution.cpp:140-170)
//     room_pairs   = sum over (slot, room) cells of C(n_cell, 2)
//     corr_pairs   = #{i<j : slot_i == slot_j, corr_ij}
//     unsuitable   = #{e : room_e not in possibleRooms[e]}
//   soft parts (Solution.cpp:86-138)
//     last_slot    = sum_e [slot_e % 9 == 8] * studentNumber[e]
//     consecutive  = sum_s popcount(m_s & m_s>>1 & m_s>>2 & triple-window)
//     single_class = sum_s sum_d [popcount(m_s day d) == 1]
//   eventHcv(e)    = (n_cell(e) - 1) + #{j != e : slot_j == slot_e, corr_ej}
//
// Kernels, one 256-thread workgroup per individual (tt_eval_parts chooses):
//  * parts_bits<W> (E <= 448, W = EW64 <= 7 words per event bitset): the 45
//    per-slot event bitsets are built in LDS (ds_or_b64), and an event's
//    correlated same-slot events are popcount(corr64[e] & bits[slot_e]) over
//    the W words of its full correlation row, minus its own bit where the
//    diagonal is set (studentNumber[e] > 0). That count is the correlated term
//    of eventHcv(e); its sum over e is twice corr_pairs. Three barriers.
//  * parts_bucket (E > 448): eval_block's form. Events are grouped by slot
//    into buckets and the correlation bits tested inside a bucket: pairs i < j
//    for corr_pairs alone, every j != i when eventHcv is asked for (the sum is
//    then twice corr_pairs).
// (slot, room) cell counters are 32-bit: a cell can hold all E events.
// An individual with a gene out of range gets -1 throughout.
//
// slot_hist: workgroup (b, c) counts events [64 b, 64 b + 64) over chunk c of
// the individuals in LDS (lane = event, waves stride over the rows: a wave
// reads 64 consecutive bytes of a row), then adds its non-zero counts to the
// zeroed output: one global atomic per (event, slot, chunk), none per gene.
#include <algorithm>

#include "../../include/ttga_report.h"
#include "tt_internal.h"

namespace ttga {

constexpr int kPartsThreads = 256;
constexpr int kHistThreads = 256;
constexpr int kHistEvents = 64;

// Sums the six per-thread parts over the workgroup into acc[0..5] (LDS, zeroed
// before the last barrier) and stores them; v[1] is twice corr_pairs when
// `halve`. Every thread of the workgroup calls it.
__device__ __forceinline__ void store_parts(int (&v)[TT_NUM_PARTS], int32_t* acc, bool halve, int32_t* out) {
#pragma unroll
    for (int k = 0; k < TT_NUM_PARTS; ++k) {
        const int s = wave_sum(v[k]);
        if ((threadIdx.x & 63) == 0 && s) atomicAdd(&acc[k], s);
    }
    __syncthreads();
    if (threadIdx.x < TT_NUM_PARTS) {
        const int x = acc[threadIdx.x];
        out[threadIdx.x] = (halve && threadIdx.x == TT_PART_CORR_PAIRS) ? x >> 1 : x;
    }
}

// -1 in the parts and the eventHcv row of an individual with an invalid gene.
__device__ __forceinline__ void store_invalid(int E, int32_t* out, int32_t* eh) {
    if (threadIdx.x < TT_NUM_PARTS) out[threadIdx.x] = -1;
    if (eh)
        for (int e = threadIdx.x; e < E; e += kPartsThreads) eh[e] = -1;
}

// >2 in a row and single class of the students tid, tid + 256, ... from the
// slot row sl in LDS. PADDED: the student's events come from the lists padded
// to multiples of 8 with the sentinel column E (sl[E] = 63, a bit no term
// looks at), eight ids in two 16-B loads and eight LDS reads in flight at a
// time; the plain CSR walk is one dependent global load + LDS read per event.
template <bool PADDED>
__device__ __forceinline__ void student_parts(const DevProblem& pb, const uint8_t* sl, int& consecutive, int& single) {
    for (int st = threadIdx.x; st < pb.S; st += kPartsThreads) {
        uint64_t m = 0;
        if constexpr (PADDED) {
            const int c1 = pb.stc_off[st + 1];
            for (int c = pb.stc_off[st]; c < c1; c += 8) {
                const int4 a = *(const int4*)(pb.stc_ev + c), b = *(const int4*)(pb.stc_ev + c + 4);
                m |= 1ull << sl[a.x] | 1ull << sl[a.y] | 1ull << sl[a.z] | 1ull << sl[a.w] | 1ull << sl[b.x] |
                     1ull << sl[b.y] | 1ull << sl[b.z] | 1ull << sl[b.w];
            }
        } else {
            for (int k = pb.stu_off[st]; k < pb.stu_off[st + 1]; ++k) m |= 1ull << sl[pb.stu_ev[k]];
        }
        consecutive += __popcll(m & (m >> 1) & (m >> 2) & kTripleMask);
#pragma unroll
        for (int d = 0; d < 5; ++d) single += (__popc((uint32_t)(m >> (9 * d)) & 0x1FFu) == 1);
    }
}

// ---------------------------------------------------------------- parts_bits
template <int W>
__global__ __launch_bounds__(kPartsThreads) void parts_bits_kernel(DevProblem pb, const uint8_t* __restrict__ slot,
                                                                   const uint8_t* __restrict__ room,
                                                                   int32_t* __restrict__ parts,
                                                                   int32_t* __restrict__ event_hcv) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    const int E = pb.E, R = pb.R;
    const int tid = threadIdx.x;
    const long p = blockIdx.x;
    const int cells = kSlots * R;
    unsigned long long* bits = (unsigned long long*)lds;  // [45][W] events of each slot
    uint32_t* cnt = (uint32_t*)(bits + kSlots * W);        // [cells]
    int32_t* red = (int32_t*)(cnt + cells);                // [8]: the six parts, [6] invalid gene
    uint8_t* sl = (uint8_t*)(red + 8);                     // [E + 1]: sl[E] = 63, the sentinel column

    const uint8_t* gs = slot + p * E;
    const uint8_t* gr = room + p * E;
    int32_t* eh = event_hcv ? event_hcv + p * E : nullptr;
    if (tid == 0) sl[E] = 63;
    for (int c = tid; c < kSlots * W; c += kPartsThreads) bits[c] = 0ull;
    for (int c = tid; c < cells; c += kPartsThreads) cnt[c] = 0u;
    if (tid < 8) red[tid] = 0;
    __syncthreads();

    int v[TT_NUM_PARTS] = {0, 0, 0, 0, 0, 0};
    bool bad = false;
    for (int e = tid; e < E; e += kPartsThreads) {
        const int s = gs[e], r = gr[e];
        sl[e] = (uint8_t)s;
        if (s >= kSlots || r >= R) { bad = true; continue; }
        v[TT_PART_ROOM_PAIRS] += (int)atomicAdd(&cnt[s * R + r], 1u);
        v[TT_PART_UNSUITABLE] += ((pb.poss[e] >> r) & 1ull) ? 0 : 1;
        v[TT_PART_LAST_SLOT] += ((kLastSlotMask >> s) & 1ull) ? pb.sn[e] : 0;
        atomicOr(&bits[s * W + (e >> 6)], 1ull << (e & 63));
    }
    if (bad) atomicOr(&red[6], 1);
    __syncthreads();
    if (red[6]) {                                          // uniform over the workgroup
        store_invalid(E, parts + p * TT_NUM_PARTS, eh);
        return;
    }
    for (int e = tid; e < E; e += kPartsThreads) {
        const int s = sl[e];
        const uint64_t* row = pb.corr64 + (size_t)e * W;
        uint64_t cw[W];
#pragma unroll
        for (int w = 0; w < W; ++w) cw[w] = row[w];
        int c = 0;
#pragma unroll
        for (int w = 0; w < W; ++w) {
            if (w == (e >> 6)) c -= (int)((cw[w] >> (e & 63)) & 1ull);      // e itself, where the diagonal is set
            c += __popcll(cw[w] & bits[s * W + w]);
        }
        v[TT_PART_CORR_PAIRS] += c;
        if (eh) eh[e] = c + (int)cnt[s * R + gr[e]] - 1;
    }
    student_parts<true>(pb, sl, v[TT_PART_CONSECUTIVE], v[TT_PART_SINGLE_CLASS]);
    store_parts(v, red, true, parts + p * TT_NUM_PARTS);
}

static size_t bits_lds_bytes(int E, int R, int W) {
    return 8 * (size_t)(kSlots * W) + 4 * (size_t)(kSlots * R + 8) + (size_t)E + 1;
}

// -------------------------------------------------------------- parts_bucket
// LDS as eval_block's (the same instances fit); the part sums reuse the bucket
// cursors once the buckets are filled.
__global__ __launch_bounds__(kPartsThreads) void parts_bucket_kernel(DevProblem pb, const uint8_t* __restrict__ slot,
                                                                     const uint8_t* __restrict__ room,
                                                                     int32_t* __restrict__ parts,
                                                                     int32_t* __restrict__ event_hcv) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    const int E = pb.E, R = pb.R, EW = pb.EW;
    const int tid = threadIdx.x;
    const long p = blockIdx.x;
    const int cells = kSlots * R;
    uint32_t* cnt = (uint32_t*)lds;                       // [cells]
    uint32_t* bcnt = cnt + cells;                         // [45] events per slot
    uint32_t* bstart = bcnt + kSlots;                     // [45]
    uint32_t* bcur = bstart + kSlots;                     // [45] fill cursors, then the part sums
    int32_t* red = (int32_t*)(bcur + kSlots);             // [4]: [2] invalid gene
    uint16_t* bucket = (uint16_t*)(red + 4);              // [E]
    uint8_t* sl = (uint8_t*)(bucket + ((E + 1) & ~1));    // [E]

    const uint8_t* gs = slot + p * E;
    const uint8_t* gr = room + p * E;
    int32_t* eh = event_hcv ? event_hcv + p * E : nullptr;
    for (int c = tid; c < cells; c += kPartsThreads) cnt[c] = 0u;
    for (int c = tid; c < kSlots; c += kPartsThreads) { bcnt[c] = 0u; bcur[c] = 0u; }
    if (tid < 4) red[tid] = 0;
    __syncthreads();

    int v[TT_NUM_PARTS] = {0, 0, 0, 0, 0, 0};
    bool bad = false;
    for (int e = tid; e < E; e += kPartsThreads) {
        const int s = gs[e], r = gr[e];
        sl[e] = (uint8_t)s;
        if (s >= kSlots || r >= R) { bad = true; continue; }
        v[TT_PART_ROOM_PAIRS] += (int)atomicAdd(&cnt[s * R + r], 1u);
        v[TT_PART_UNSUITABLE] += ((pb.poss[e] >> r) & 1ull) ? 0 : 1;
        v[TT_PART_LAST_SLOT] += ((kLastSlotMask >> s) & 1ull) ? pb.sn[e] : 0;
        atomicAdd(&bcnt[s], 1u);
    }
    if (bad) atomicOr(&red[2], 1);
    __syncthreads();
    if (red[2]) {                                          // uniform over the workgroup
        store_invalid(E, parts + p * TT_NUM_PARTS, eh);
        return;
    }
    if (tid == 0) {
        uint32_t acc = 0;
        for (int t = 0; t < kSlots; ++t) { bstart[t] = acc; acc += bcnt[t]; }
    }
    __syncthreads();
    for (int e = tid; e < E; e += kPartsThreads) {
        const int s = sl[e];
        bucket[bstart[s] + atomicAdd(&bcur[s], 1u)] = (uint16_t)e;
    }
    __syncthreads();
    if (tid < TT_NUM_PARTS) bcur[tid] = 0u;                // the cursors are done with
    const bool all = eh != nullptr;
    for (int i = tid; i < E; i += kPartsThreads) {
        const int s = sl[i];
        const uint32_t* row = pb.corr + (size_t)i * EW;
        const uint32_t b0 = bstart[s], b1 = b0 + bcnt[s];
        int c = 0;
        for (uint32_t b = b0; b < b1; ++b) {
            const int j = bucket[b];
            if (all ? j != i : j > i) c += (int)((row[j >> 5] >> (j & 31)) & 1u);
        }
        v[TT_PART_CORR_PAIRS] += c;
        if (all) eh[i] = c + (int)cnt[s * R + gr[i]] - 1;
    }
    student_parts<false>(pb, sl, v[TT_PART_CONSECUTIVE], v[TT_PART_SINGLE_CLASS]);
    __syncthreads();                                       // bcur[0..5] zeroed above
    store_parts(v, (int32_t*)bcur, all, parts + p * TT_NUM_PARTS);
}

static size_t bucket_lds_bytes(int E, int R) {
    return 4 * (size_t)(kSlots * R + 3 * kSlots + 4) + 2 * (size_t)((E + 1) & ~1) + (size_t)E;
}

// ----------------------------------------------------------------- slot_hist
__global__ __launch_bounds__(kHistThreads) void slot_hist_kernel(int E, const uint8_t* __restrict__ slot, int P,
                                                                 int rows_per_chunk, int32_t* __restrict__ hist) {
    __shared__ uint32_t cnt[kHistEvents * kSlots];
    const int tid = threadIdx.x;
    const int e0 = blockIdx.x * kHistEvents;
    const int e = e0 + (tid & 63);
    for (int c = tid; c < kHistEvents * kSlots; c += kHistThreads) cnt[c] = 0u;
    __syncthreads();
    const long r0 = (long)blockIdx.y * rows_per_chunk;
    const long r1 = r0 + rows_per_chunk < (long)P ? r0 + rows_per_chunk : (long)P;
    if (e < E) {
        uint32_t* mine = cnt + (tid & 63) * kSlots;
        for (long i = r0 + (tid >> 6); i < r1; i += kHistThreads / 64) {
            const int s = slot[i * E + e];
            if (s < kSlots) atomicAdd(&mine[s], 1u);
        }
    }
    __syncthreads();
    const int n = (E - e0 < kHistEvents ? E - e0 : kHistEvents) * kSlots;
    int32_t* out = hist + (size_t)e0 * kSlots;
    for (int c = tid; c < n; c += kHistThreads)
        if (cnt[c]) atomicAdd(&out[c], (int32_t)cnt[c]);
}

}  // namespace ttga

using namespace ttga;

extern "C" int tt_eval_parts(const tt_problem* p, const uint8_t* slot, const uint8_t* room, int P, int32_t* parts,
                             int32_t* event_hcv, void* stream) {
    int rc = check_pop_args(p, P, slot, room);
    if (rc) return rc;
    if (P > 0 && !parts) { set_error("null output buffer"); return TT_ERR_INVALID; }
    if (P == 0) return TT_OK;
    rc = use_device(p);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    const int E = p->E, R = p->R, W = p->dev.EW64;
    if ((rc = check_grid("tt_eval_parts", P, kPartsThreads))) return rc;
    if (W <= 7) {
        const size_t lds = bits_lds_bytes(E, R, W);
#define TT_BITS(WC)                                                                                              \
    case WC:                                                                                                     \
        hipLaunchKernelGGL(parts_bits_kernel<WC>, dim3(P), dim3(kPartsThreads), lds, st, p->dev, slot, room,     \
                           parts, event_hcv);                                                                    \
        break;
        switch (W) {
            TT_BITS(1) TT_BITS(2) TT_BITS(3) TT_BITS(4) TT_BITS(5) TT_BITS(6) TT_BITS(7)
            default: set_error("bad event bitset width"); return TT_ERR_LIMIT;
        }
#undef TT_BITS
    } else {
        const size_t lds = bucket_lds_bytes(E, R);
        if (lds > 160 * 1024) { set_error("instance too large for the parts kernel"); return TT_ERR_LIMIT; }
        hipLaunchKernelGGL(parts_bucket_kernel, dim3(P), dim3(kPartsThreads), lds, st, p->dev, slot, room, parts,
                           event_hcv);
    }
    return check_hip(hipGetLastError(), "tt_eval_parts launch");
}

extern "C" int tt_slot_histogram(const tt_problem* p, const uint8_t* slot, int P, int32_t* hist, void* stream) {
    if (!p) { set_error("null tt_problem"); return TT_ERR_INVALID; }
    if (P < 0) { set_error("negative population size"); return TT_ERR_INVALID; }
    if (!hist || (P > 0 && !slot)) { set_error("null population or output buffer"); return TT_ERR_INVALID; }
    int rc = use_device(p);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    const int E = p->E;
    TT_HIP(hipMemsetAsync(hist, 0, sizeof(int32_t) * (size_t)E * kSlots, st));
    if (P == 0) return TT_OK;
    // chunks of individuals: enough workgroups for two per CU, each with at
    // least 256 rows (a chunk costs up to 64 x 45 global atomics)
    const int eb = (E + kHistEvents - 1) / kHistEvents;
    const int want = (2 * std::max(1, p->num_cus) + eb - 1) / eb;
    const int chunks = std::max(1, std::min({want, (P + 255) / 256, 65535}));
    const int rows = (P + chunks - 1) / chunks;
    hipLaunchKernelGGL(slot_hist_kernel, dim3(eb, (P + rows - 1) / rows), dim3(kHistThreads), 0, st, E, slot, P, rows,
                       hist);
    return check_hip(hipGetLastError(), "tt_slot_histogram launch");
}
