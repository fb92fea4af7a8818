// Kempe-chain interchange (include/ttga_kempe.h):
//   tt_kempe_move  per individual, the connected component of one event in the
//                  conflict graph of two timeslots changes sides; the two slots
//                  are then re-matched as tt_mutation re-matches its touched
//                  slots (tt_match.h)
// No counterpart in the reference; its call site would follow the mutation of ga.cpp:571.
#include "../../include/ttga_kempe.h"
#include "tt_internal.h"
#include "tt_match.h"

namespace ttga {

constexpr int kStatusBadGene = 64;      // tt_device_status bit 6
// correlation-row words a lane accumulates (words l, l + 64, ...): 640 words = 40,960
// events, past anything the matcher's scratch admits
constexpr int kKempeLaneWords = 10;

// the three bitsets follow the matcher's scratch
__host__ __device__ inline size_t kempe_lds_bytes(int E, int R) {
    return match_scratch_bytes(E, R) + 3 * 8 * (size_t)((E + 63) / 64);
}

// One wave (workgroup) per individual.
//   LDS: MatchScratch | U[EW64] | K[EW64] | F[EW64]   (u64 words)
// U = the events of slots t1 and t2, K = the chain so far, F = the frontier: the
// events that joined K in the last round. A round ORs the correlation rows of
// the frontier's events (lane l: words l, l + 64, ...) and keeps what lies in
// U \ K. The rows carry the diagonal wherever an event has a student
// (tt_common.h: corr64, "diagonal included"); it does not matter here, e is in
// K from the start and K is masked out of every round's result.
// Loop bounds: a round that adds nothing ends the search and every other round
// adds at least one of the E events to K, so at most E rounds; a round visits
// each of the EW64 frontier words once and at most 64 bits of each.
__global__ __launch_bounds__(64) void kempe_kernel(DevProblem pb, uint8_t* __restrict__ slot,
                                                   uint8_t* __restrict__ room, int64_t* __restrict__ rng, int P,
                                                   double prob, int max_chain, int32_t* __restrict__ chain_len,
                                                   unsigned bits_off) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    const int E = pb.E, R = pb.R, EW64 = pb.EW64, lane = threadIdx.x;
    const long p = blockIdx.x;
    if (p >= P) return;
    MatchScratch m = carve_match_scratch(lds, E, R);
    uint64_t* U = (uint64_t*)(lds + bits_off);
    uint64_t* K = U + EW64;
    uint64_t* F = K + EW64;
    for (int e0 = 0; e0 < E; e0 += 512) {               // eight loads of each row in flight (tt_rooms.hip load_row)
        uint8_t vs[8], vr[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int e = e0 + 64 * k + lane;
            vs[k] = e < E ? slot[p * E + e] : 0;
            vr[k] = e < E ? room[p * E + e] : 0;
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int e = e0 + 64 * k + lane;
            if (e < E) { m.sl[e] = vs[k]; m.rr[e] = vr[k]; }
        }
    }
    __syncthreads();
    // validity: an invalid row is left as it is, its stream included
    bool bad = false;
    for (int e = lane; e < E; e += 64) bad |= m.sl[e] >= kSlots || m.rr[e] >= R;
    if (wave_any(bad)) {
        if (lane == 0) {
            if (chain_len) chain_len[p] = 0;
            atomicOr(pb.status, kStatusBadGene);
        }
        return;
    }
    // gate and choice: lane 0 draws, the wave reads the result from LDS
    if (lane == 0) {
        int64_t s = rng[p];
        uint32_t go = pm_next(s) < prob, e = 0, t1 = 0, t2 = 0;
        if (go) {
            e = (uint32_t)pm_pick(s, E);
            t1 = m.sl[e];
            t2 = (uint32_t)pm_pick(s, kSlots - 1);
            if (t2 >= t1) t2 += 1;
        }
        rng[p] = s;
        m.flags[0] = go; m.flags[1] = e; m.flags[2] = t1; m.flags[3] = t2;
    }
    __syncthreads();
    if (!m.flags[0]) {
        if (lane == 0 && chain_len) chain_len[p] = 0;
        return;
    }
    const int e0 = (int)m.flags[1], t1 = (int)m.flags[2], t2 = (int)m.flags[3];
    for (int w = 0; w < EW64; ++w) {
        const int e = 64 * w + lane;
        const int s = e < E ? m.sl[e] : 0xFF;            // the tail of the last word stays out of U
        const uint64_t u = ballot(s == t1 || s == t2);
        if (lane == (w & 63)) {
            const uint64_t k0 = w == (e0 >> 6) ? 1ull << (e0 & 63) : 0ull;
            U[w] = u; K[w] = k0; F[w] = k0;
        }
    }
    __syncthreads();
    for (int round = 0; round < E; ++round) {
        uint64_t acc[kKempeLaneWords];
#pragma unroll
        for (int k = 0; k < kKempeLaneWords; ++k) acc[k] = 0ull;
        for (int fw = 0; fw < EW64; ++fw) {
            const uint64_t xv = F[fw];                  // one address for the wave: wave-uniform
            uint64_t x = ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(xv >> 32)) << 32) |
                         (uint32_t)__builtin_amdgcn_readfirstlane((int)xv);
            for (int g = 0; g < 64 && x; ++g) {
                const int f = 64 * fw + (__ffsll((unsigned long long)x) - 1);
                x &= x - 1;
                const uint64_t* cr = pb.corr64 + (size_t)f * EW64;
#pragma unroll
                for (int k = 0; k < kKempeLaneWords; ++k)
                    if (64 * k < EW64 && 64 * k + lane < EW64) acc[k] |= cr[64 * k + lane];
            }
        }
        __syncthreads();                                // every lane has read the frontier
        bool grew = false;
#pragma unroll
        for (int k = 0; k < kKempeLaneWords; ++k) {
            const int w = 64 * k + lane;
            if (w < EW64) {
                const uint64_t nw = acc[k] & U[w] & ~K[w];
                K[w] |= nw;
                F[w] = nw;
                grew |= nw != 0ull;
            }
        }
        const bool go_on = wave_any(grew);
        __syncthreads();
        if (!go_on) break;
    }
    int cnt = 0;
    for (int w = lane; w < EW64; w += 64) cnt += __popcll(K[w]);
    cnt = wave_sum(cnt);
    if (max_chain > 0 && cnt > max_chain) {             // the cap: the row stays, three draws are gone
        if (lane == 0 && chain_len) chain_len[p] = -cnt;
        return;
    }
    for (int e = lane; e < E; e += 64)
        if ((K[e >> 6] >> (e & 63)) & 1ull) m.sl[e] = (uint8_t)(t1 + t2 - m.sl[e]);
    __syncthreads();
    build_buckets(pb, m, lane);
    assign_touched(pb, m, (1ull << t1) | (1ull << t2), lane);
    for (int e = lane; e < E; e += 64) {
        slot[p * E + e] = m.sl[e];
        room[p * E + e] = m.rr[e];
    }
    if (lane == 0 && chain_len) chain_len[p] = cnt;
}

}  // namespace ttga

using namespace ttga;

extern "C" int tt_kempe_move(const tt_problem* p, uint8_t* slot, uint8_t* room, int64_t* rng, int P, double prob,
                             int max_chain, int32_t* chain_len, void* stream) {
    int rc = check_pop_args(p, P, slot, room);
    if (rc) return rc;
    if (max_chain < 0) { set_error("tt_kempe_move: negative max_chain"); return TT_ERR_INVALID; }
    if (!(prob >= 0.0 && prob <= 1.0)) { set_error("tt_kempe_move: prob outside [0, 1]"); return TT_ERR_INVALID; }
    if (P == 0) return TT_OK;
    if (!rng) { set_error("tt_kempe_move: null rng buffer"); return TT_ERR_INVALID; }
    const size_t lds = kempe_lds_bytes(p->E, p->R);
    if (lds > 160 * 1024 || p->dev.EW64 > 64 * kKempeLaneWords) {
        set_error("instance too large for the Kempe move");
        return TT_ERR_LIMIT;
    }
    if ((rc = check_rows_grid("tt_kempe_move", p, P, false))) return rc;
    if ((rc = use_device(p))) return rc;
    hipLaunchKernelGGL(kempe_kernel, dim3(P), dim3(64), lds, (hipStream_t)stream, p->dev, slot, room, rng, P, prob,
                       max_chain, chain_len, (unsigned)match_scratch_bytes(p->E, p->R));
    return check_hip(hipGetLastError(), "kempe launch");
}
