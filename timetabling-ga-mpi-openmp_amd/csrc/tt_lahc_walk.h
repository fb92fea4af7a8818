// The late-acceptance walk on feasible rows (include/ttga_lahc*.h), shared by tt_lahc.hip,
// tt_lahc_kempe.hip, tt_lahc_kempe_aug.hip and tt_lahc_multi.hip: the LDS image and its one
// carve, the pieces that lahc_kernel composes (entry, the walk's running state, the
// acceptance rule and its bookkeeping, the plain step, the exits), the walk with chains
// (lahc_chain_walk, one body for lahc_kempe_kernel, lahc_kempe_aug_kernel and
// lahc_multi_walk_kernel), and the host's argument checks.
//
// On a feasible row a student attends at most one event per slot, so scv is a sum over
// the students of a function of the 45-bit attendance mask m: per 9-bit day,
// [bit 8] + the windows of three set bits + [exactly one bit]. A move of event e from
// slot a to slot t turns m into m ^ bit a ^ bit t for the students of e and for nobody
// else, and only the days of a and t change their cost. The feasibility of a candidate
// is one AND of the event's correlation row with the target slot's event bitset and
// one AND of its possible rooms with the slot's free rooms; no matcher runs.
//
// One wave (workgroup) per walk. Everything that decides a step is wave-uniform: every
// lane draws the same three numbers from its own copy of the state, and the words that
// all lanes update (set and occ outside a chain, the two genes of Move1 / Move2, hist,
// klist, koff, kroom) are written by every lane with the same value to the same address,
// so each lane later reads what it wrote itself. What one lane writes and another reads
// is named at the piece that writes it, with the barrier that covers it.
#pragma once
#include "../../include/ttga_lahc.h"
#include "tt_internal.h"

namespace ttga {

constexpr int kStatusLahcBadGene = 256;     // tt_device_status bit 8
constexpr size_t kLahcMaxLds = 64 * 1024;
constexpr int kChainMax = 2 * kMaxRooms;    // the events of two slots of a feasible row
// correlation-row words a lane accumulates (words l, l + 64): 128 words = 8,192 events;
// the LDS formula admits no more than 101 words (47 bitset words and 256 gene bytes a word)
constexpr int kLkLaneWords = 2;
constexpr int kLkRoot = 0xFF;               // qpar of a room of poss[e]: the event itself takes it

// ---- the LDS image
// What a kernel's walk keeps in LDS: the plain walk, the walk with chains, or the walk
// with chains and the augmenting search's tables.
enum LahcKind { kLahcPlain, kLahcChain, kLahcAug };

// set[45][EW64] u64 | occ[45] u64 | K[EW64] F[EW64] u64 (chains) | mask[S] u64 | hist[L] i32 |
// klist[128] koff[128 + 4] i32 (chains) | sl[E] rr[E] bsl[E] brr[E] u8 | kroom[128] u8 (chains) |
// hold[2][64] i16 (room -> event, -1: free; the table of slot a, then of slot t), qpar[64]
// queue[64] u8 (augment). A pointer the kind does not have is null.
struct LahcLds {
    uint64_t *set, *occ, *K, *F, *mask;
    int32_t *hist, *klist, *koff;
    uint8_t *sl, *rr, *bsl, *brr, *kroom;
    int16_t* hold;
    uint8_t *qpar, *queue;
    size_t bytes;                           // of the whole image
};

// the next n elements of type T: counted in `off`, and in a kernel taken at `base`, which
// moves on; the host and the compiler only count
template <class T>
__host__ __device__ constexpr T* lahc_take(uint8_t*& base, size_t& off, size_t n) {
    off += n * sizeof(T);
#ifdef __HIP_DEVICE_COMPILE__
    if (!__builtin_is_constant_evaluated()) {
        T* at = (T*)base;
        base = (uint8_t*)(at + n);
        return at;
    }
#endif
    return nullptr;
}

// The one carve: a kernel calls it with its LDS, the host with a null base for `bytes`.
__host__ __device__ constexpr LahcLds lahc_carve(LahcKind kind, uint8_t* base, int E, int EW64, int S, int L) {
    LahcLds m{};
    size_t off = 0;
    m.set = lahc_take<uint64_t>(base, off, (size_t)kSlots * EW64);
    m.occ = lahc_take<uint64_t>(base, off, kSlots);
    if (kind != kLahcPlain) {
        m.K = lahc_take<uint64_t>(base, off, EW64);
        m.F = lahc_take<uint64_t>(base, off, EW64);
    }
    m.mask = lahc_take<uint64_t>(base, off, S);
    m.hist = lahc_take<int32_t>(base, off, L);
    if (kind != kLahcPlain) {
        m.klist = lahc_take<int32_t>(base, off, kChainMax);
        m.koff = lahc_take<int32_t>(base, off, kChainMax + 4);
    }
    m.sl = lahc_take<uint8_t>(base, off, E);
    m.rr = lahc_take<uint8_t>(base, off, E);
    m.bsl = lahc_take<uint8_t>(base, off, E);
    m.brr = lahc_take<uint8_t>(base, off, E);
    if (kind != kLahcPlain) m.kroom = lahc_take<uint8_t>(base, off, kChainMax);
    if (kind == kLahcAug) {
        m.hold = lahc_take<int16_t>(base, off, 2 * kMaxRooms);
        m.qpar = lahc_take<uint8_t>(base, off, kMaxRooms);
        m.queue = lahc_take<uint8_t>(base, off, kMaxRooms);
    }
    m.bytes = off;
    return m;
}

__host__ __device__ constexpr size_t lahc_lds_bytes(LahcKind kind, int E, int S, int L) {
    return lahc_carve(kind, nullptr, E, (E + 63) / 64, S, L).bytes;
}

// the limits that include/ttga_lahc*.h document: 8 (45 EW64 + 45 + S) + 4 L + 4 E plain;
// 8 (47 EW64 + 45 + S) + 4 L + 4 E + 1,168 with chains; 384 more with the tables
static_assert(lahc_lds_bytes(kLahcPlain, 100, 80, 0) == 2120, "sm without the history");
static_assert(lahc_lds_bytes(kLahcChain, 400, 200, 500) == 9360, "med with chains");
static_assert(lahc_lds_bytes(kLahcChain, 2000, 5000, 100) == 61960, "syn with chains");
static_assert(lahc_lds_bytes(kLahcAug, 400, 200, 500) == 9360 + 384, "med with the tables");
static_assert(lahc_lds_bytes(kLahcAug, 2000, 5000, 100) == 61960 + 384, "syn with the tables");

// ---- small helpers
// one day's cost of a student: last slot of the day, windows of three, single class
__device__ __forceinline__ int lahc_day_cost(uint64_t m, int day) {
    const uint32_t d = (uint32_t)(m >> (9 * day)) & 0x1FFu;
    return (int)(d >> 8) + __popc(d & (d >> 1) & (d >> 2)) + (__popc(d) == 1);
}

// cost(m ^ flip) - cost(m) where flip has bits on days da and db only
__device__ __forceinline__ int lahc_mask_delta(uint64_t m, uint64_t flip, int da, int db) {
    const uint64_t n = m ^ flip;
    int d = lahc_day_cost(n, da) - lahc_day_cost(m, da);
    if (db != da) d += lahc_day_cost(n, db) - lahc_day_cost(m, db);
    return d;
}

__device__ __forceinline__ int lahc_uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }

// lane r's 64-bit value, r the same in every lane
__device__ __forceinline__ uint64_t lahc_lane64(uint64_t v, int r) {
    return ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(v >> 32), r) << 32) |
           (uint32_t)__builtin_amdgcn_readlane((int)v, r);
}

// what a finished walk does to the row's scv and penalty: the penalty of a feasible row is
// its scv, anything else (an infeasible row's 1000000 + hcv) stays
__device__ __forceinline__ void lahc_credit(int32_t* scv, int32_t* penalty, long p, int g) {
    if (scv) scv[p] -= g;
    if (penalty) {
        const int pen = penalty[p];
        if (pen >= 0 && pen < 1000000) penalty[p] = pen - g;
    }
}

// ---- entry: the row, validity, the bitsets, the student masks and the hcv gate
struct LahcEntry {
    bool closed;                            // the row does not walk: a bad gene, hcv > 0 or steps == 0
    bool bad_gene;                          // a gene out of range: nothing but sl / rr was built
};

// Lane roles: event per lane (genes, bitsets), then student per lane (masks). set and occ
// are built with LDS atomics; the barrier at the end covers them, the masks and hist, so
// the walk starts on an image every lane sees. What a closed row writes is the caller's exit.
// Loop bounds: ceil(E / 64) events, ceil((45 EW64 + 45) / 64) words, ceil(L / 64) history
// entries and ceil(S / 64) students per lane, each student over its own events.
__device__ __forceinline__ LahcEntry lahc_enter(const DevProblem& pb, const LahcLds& lds, const uint8_t* slot,
                                                const uint8_t* room, long p, int steps, int L, int lane) {
    const int E = pb.E, R = pb.R, S = pb.S, EW64 = pb.EW64;
    bool bad = false;
    for (int e = lane; e < E; e += 64) {
        const uint8_t s = slot[p * E + e], r = room[p * E + e];
        lds.sl[e] = s;
        lds.rr[e] = r;
        bad |= s >= kSlots || r >= R;
    }
    for (int i = lane; i < kSlots * EW64 + kSlots; i += 64) lds.set[i] = 0ull;    // set and occ are adjacent
    for (int i = lane; i < L; i += 64) lds.hist[i] = 0;                           // costs are kept relative to scv0
    __syncthreads();
    const bool bad_row = wave_any(bad);
    bool hard = false;                                  // a hard-constraint violation seen by this lane
    if (!bad_row) {
        for (int e = lane; e < E; e += 64) {
            const int s = lds.sl[e], r = lds.rr[e];
            atomicOr((unsigned long long*)&lds.set[(size_t)s * EW64 + (e >> 6)], 1ull << (e & 63));
            const unsigned long long old = atomicOr((unsigned long long*)&lds.occ[s], 1ull << r);
            hard |= ((old >> r) & 1ull) != 0ull;            // two events in one room of one slot
            hard |= ((pb.poss[e] >> r) & 1ull) == 0ull;     // a room that is not possible
        }
        // two correlated events share a student: they are in one slot exactly if some
        // student's events cover fewer slots than the student has events
        for (int s = lane; s < S; s += 64) {
            const int b = pb.stu_off[s], end = pb.stu_off[s + 1];
            uint64_t m = 0ull;
            for (int i = b; i < end; ++i) m |= 1ull << lds.sl[pb.stu_ev[i]];
            lds.mask[s] = m;
            hard |= __popcll(m) != end - b;
        }
        __syncthreads();
    }
    return {bad_row || wave_any(hard) || steps == 0, bad_row};
}

// ---- the walk's running state; cur and best are relative to the row's scv at entry
struct LahcWalk {
    int64_t st;                             // the stream
    int cur = 0, best = 0, n_acc = 0, b_step = 0;
    bool live_is_best = true;               // the best row is the row in sl / rr
    int v = 0;                              // the history entry this step reads and writes
};

// A step's three draws, the same in every lane: the event, Move1 or Move2, and the number x
// that picks the second slot or event.
struct LahcDraw {
    int e1, a;                              // the event and its slot
    double x;
    bool swap;
};
__device__ __forceinline__ LahcDraw lahc_draw(const DevProblem& pb, const LahcLds& m, LahcWalk& w, double p_swap) {
    const int E = pb.E;
    LahcDraw c;
    c.e1 = min(max(lahc_uniform(pm_pick(w.st, E)), 0), E - 1);
    const double u = pm_next(w.st);
    c.x = pm_next(w.st);
    c.swap = E >= 2 && lahc_uniform((int)(u < p_swap)) != 0;
    c.a = lahc_uniform((int)m.sl[c.e1]);
    return c;
}

// the second slot of Move1: one of the 44 others
__device__ __forceinline__ int lahc_other_slot(double x, int a) {
    int b = lahc_uniform((int)__dmul_rn(x, (double)(kSlots - 1)));
    b += b >= a;
    return min(max(b, 0), kSlots - 1);
}

// ---- the acceptance rule and its bookkeeping, for the plain step and the chain step alike
__device__ __forceinline__ bool lahc_accepts(const LahcLds& m, const LahcWalk& w, int cand) {
    return cand <= w.cur || cand <= lahc_uniform(m.hist[w.v]);
}

// Before an accepted candidate is applied: if the row in sl / rr is the best one and is
// about to get worse (or stay level), it goes to bsl / brr. Lane = event; the barrier
// stands between these reads of sl / rr and the writes of the move that follows, which
// other lanes make (the chain's genes) or every lane makes (Move1 / Move2). ceil(E / 64)
// events per lane.
__device__ __forceinline__ void lahc_leave_best(const LahcLds& m, LahcWalk& w, int cand, int E, int lane) {
    const bool leaves = w.live_is_best && cand >= w.cur;
    if (leaves) {
        for (int e = lane; e < E; e += 64) { m.bsl[e] = m.sl[e]; m.brr[e] = m.rr[e]; }
        __syncthreads();
    }
    w.live_is_best = w.live_is_best && !leaves;
}

// after step k's candidate is applied
__device__ __forceinline__ void lahc_accepted(LahcWalk& w, int cand, int k) {
    const bool better = cand < w.best;
    w.cur = cand;
    ++w.n_acc;
    if (better) {
        w.best = cand;
        w.b_step = k + 1;
    }
    w.live_is_best = w.live_is_best || better;
}

// the end of every step, accepted or not; every lane writes the one entry
__device__ __forceinline__ void lahc_remember(const LahcLds& m, LahcWalk& w, int L) {
    m.hist[w.v] = w.cur;
    w.v = w.v + 1 == L ? 0 : w.v + 1;
}

// ---- the plain step: Move1 (e1 to another slot) or Move2 (e1 and e2 trade slots)
// Lane roles: correlation test = bitset word per lane; delta and apply = student of the
// moved event(s) per lane. The bitsets, occ and the one or two genes are written by every
// lane alike; the student masks are written by one lane and read by another: the barrier
// at the end of an applied move covers them.
// Loop bounds: ceil(EW64 / 64) words and ceil(students of the one or two events / 64)
// students per lane.
__device__ __forceinline__ void lahc_plain_step(const DevProblem& pb, const LahcLds& m, LahcWalk& wk,
                                                const LahcDraw& c, int k, int lane) {
    const int E = pb.E, EW64 = pb.EW64, e1 = c.e1, a = c.a;
    const bool swap = c.swap;
    const int off1 = pb.ev_off[e1], n1 = pb.ev_off[e1 + 1] - off1;
    int e2 = e1, b, r1, r2 = 0, off2 = 0, n2 = 0;
    bool feas;
    if (swap) {
        e2 = lahc_uniform((int)__dmul_rn(c.x, (double)(E - 1)));
        e2 += e2 >= e1;
        e2 = min(max(e2, 0), E - 1);
        b = lahc_uniform((int)m.sl[e2]);
        off2 = pb.ev_off[e2];
        n2 = pb.ev_off[e2 + 1] - off2;
        bool clash = false;
        for (int w = lane; w < EW64; w += 64) {
            uint64_t sb = m.set[(size_t)b * EW64 + w], sa = m.set[(size_t)a * EW64 + w];
            if (w == (e2 >> 6)) sb &= ~(1ull << (e2 & 63));
            if (w == (e1 >> 6)) sa &= ~(1ull << (e1 & 63));
            clash |= ((pb.corr64[(size_t)e1 * EW64 + w] & sb) | (pb.corr64[(size_t)e2 * EW64 + w] & sa)) != 0ull;
        }
        const uint64_t f1 = pb.poss[e1] & ~(m.occ[b] & ~(1ull << m.rr[e2]));
        const uint64_t f2 = pb.poss[e2] & ~(m.occ[a] & ~(1ull << m.rr[e1]));
        r1 = lahc_uniform(__ffsll((unsigned long long)f1) - 1);
        r2 = lahc_uniform(__ffsll((unsigned long long)f2) - 1);
        feas = a != b && r1 >= 0 && r2 >= 0 && !wave_any(clash);
    } else {
        b = lahc_other_slot(c.x, a);
        bool clash = false;
        for (int w = lane; w < EW64; w += 64)
            clash |= (pb.corr64[(size_t)e1 * EW64 + w] & m.set[(size_t)b * EW64 + w]) != 0ull;
        const uint64_t f1 = pb.poss[e1] & ~m.occ[b];
        r1 = lahc_uniform(__ffsll((unsigned long long)f1) - 1);
        feas = r1 >= 0 && !wave_any(clash);
    }
    if (!feas) return;
    // the students of e1, then (Move2) of e2; one who attends both keeps the mask:
    // the other slot's bit is set for nobody else, the candidate being feasible
    const uint64_t flip = (1ull << a) | (1ull << b);
    const int da = a / kSlotsPerDay, db = b / kSlotsPerDay, n = n1 + n2;
    int d = 0;
    for (int i = lane; i < n; i += 64) {
        const bool first = i < n1;
        const uint64_t mm = m.mask[pb.ev_stu[first ? off1 + i : off2 + i - n1]];
        if (!swap || ((mm >> (first ? b : a)) & 1ull) == 0ull) d += lahc_mask_delta(mm, flip, da, db);
    }
    const int cand = wk.cur + wave_sum(d);
    if (!lahc_accepts(m, wk, cand)) return;
    lahc_leave_best(m, wk, cand, E, lane);
    for (int i = lane; i < n; i += 64) {
        const bool first = i < n1;
        const int s = pb.ev_stu[first ? off1 + i : off2 + i - n1];
        const uint64_t mm = m.mask[s];
        if (!swap || ((mm >> (first ? b : a)) & 1ull) == 0ull) m.mask[s] = mm ^ flip;
    }
    const uint64_t bit1 = 1ull << (e1 & 63);
    uint64_t* wa1 = &m.set[(size_t)a * EW64 + (e1 >> 6)];
    uint64_t* wb1 = &m.set[(size_t)b * EW64 + (e1 >> 6)];
    *wa1 &= ~bit1;
    *wb1 |= bit1;
    const int ro1 = m.rr[e1];
    if (swap) {
        const uint64_t bit2 = 1ull << (e2 & 63);
        uint64_t* wb2 = &m.set[(size_t)b * EW64 + (e2 >> 6)];
        uint64_t* wa2 = &m.set[(size_t)a * EW64 + (e2 >> 6)];
        *wb2 &= ~bit2;
        *wa2 |= bit2;
        const int ro2 = m.rr[e2];
        m.occ[a] = (m.occ[a] & ~(1ull << ro1)) | (1ull << r2);
        m.occ[b] = (m.occ[b] & ~(1ull << ro2)) | (1ull << r1);
        m.sl[e2] = (uint8_t)a;
        m.rr[e2] = (uint8_t)r2;
    } else {
        m.occ[a] &= ~(1ull << ro1);
        m.occ[b] |= 1ull << r1;
    }
    m.sl[e1] = (uint8_t)b;
    m.rr[e1] = (uint8_t)r1;
    lahc_accepted(wk, cand, k);
    __syncthreads();                        // the masks: written by one lane, read by another
}

// ---- the single-row exits
// the optional per-row outputs of the three single-walk entry points; kstats: n_stats a row
struct LahcOut {
    int32_t *scv, *penalty, *gain, *accepted, *best_step, *kstats;
};

// a row that did not walk: zeros, and the status bit of a bad gene
__device__ __forceinline__ void lahc_exit_closed(const DevProblem& pb, const LahcOut& o, int n_stats, long p,
                                                 LahcEntry in, int lane) {
    if (lane == 0) {
        if (o.gain) o.gain[p] = 0;
        if (o.accepted) o.accepted[p] = 0;
        if (o.best_step) o.best_step[p] = 0;
        if (in.bad_gene) atomicOr(pb.status, kStatusLahcBadGene);
    }
    if (o.kstats && lane < n_stats) o.kstats[p * n_stats + lane] = 0;
}

// The best row seen goes back if a step improved on the entry row (lane = event,
// ceil(E / 64) per lane; the last applied move's barrier covers sl / rr, lahc_leave_best's
// bsl / brr); lane 0 writes the stream and the row's numbers.
__device__ __forceinline__ void lahc_exit_row(const LahcLds& m, const LahcWalk& w, const LahcOut& o, uint8_t* slot,
                                              uint8_t* room, int64_t* rng, long p, int E, int lane) {
    if (w.b_step > 0) {
        const uint8_t* os = w.live_is_best ? m.sl : m.bsl;
        const uint8_t* orr = w.live_is_best ? m.rr : m.brr;
        for (int e = lane; e < E; e += 64) {
            slot[p * E + e] = os[e];
            room[p * E + e] = orr[e];
        }
    }
    if (lane == 0) {
        rng[p] = w.st;
        const int g = -w.best;
        if (o.gain) o.gain[p] = g;
        if (o.accepted) o.accepted[p] = w.n_acc;
        if (o.best_step) o.best_step[p] = w.b_step;
        lahc_credit(o.scv, o.penalty, p, g);
    }
}

// ---- the walk with chains
// One body, as it was before lahc_kernel was taken apart into the pieces above. The three
// kernels it serves are held to the instructions they had, and they lose them as soon as
// the body calls one of those pieces (the entry, the plain step, the acceptance helpers, the
// row exit, even the carve: each was tried, and each moves at least a few instructions). So
// the body keeps its own pointer chain over the LDS image, in lahc_carve's order, its own
// entry and its own Move1 / Move2 path, which are lahc_enter's and lahc_plain_step's line for
// line; a change to one is made to the other. Of the pieces it shares lahc_exit_closed.
//
// tt_lahc_multi's work buffer for P rows of K walkers, wave q = row * K + walker:
//   state[P] i64      the row's stream state behind all K walks (the last walker writes it)
//   nums[P K][12] i32 walker q's gain, accepted, best_step, the seven counts, walked (0: the
//                     row is closed or steps is 0: nothing else of q is written), a pad
//   rows[P K][2][E] u8 walker q's exit slot and room genes, written only if best_step > 0
constexpr int kLmNums = 12, kLmGain = 0, kLmAccepted = 1, kLmBestStep = 2, kLmStats = 3, kLmWalked = 10;
struct LahcMultiWork {
    int64_t* state;
    int32_t* nums;
    uint8_t* rows;
};
__host__ __device__ inline LahcMultiWork lahc_multi_work(void* work, long P, long K, int E) {
    uint8_t* w = (uint8_t*)work;
    return {(int64_t*)w, (int32_t*)(w + 8 * (size_t)P), w + 8 * (size_t)P + 4 * (size_t)kLmNums * (size_t)(P * K)};
}
__host__ __device__ inline size_t lahc_multi_work_size(long P, long K, int E) {
    return 8 * (size_t)P + (4 * (size_t)kLmNums + 2 * (size_t)E) * (size_t)(P * K);
}

// Walker w's stream state: s after 3 * steps * w draws. The product form of pm_mulmod holds
// for a state below 2^31 - 1 only, and rng[] may hold any 64-bit seed: draws are taken with
// pm_next until the state is in range (at least one; a 64-bit state shrinks by a factor of
// 45 a draw, so a dozen at the most), the rest is one jump. 16807 has an order that divides
// 2^31 - 2, so the exponent is reduced by it.
__device__ __forceinline__ int64_t lahc_multi_start(int64_t s, int steps, int w) {
    int64_t n = 3ll * steps * w;
    for (int g = 0; g < 64 && n > 0 && (g == 0 || (uint64_t)s >= (uint64_t)kPmM); ++g, --n) pm_next(s);
    if (n > 0 && (uint64_t)s < (uint64_t)kPmM) s = pm_mulmod((uint32_t)s, pm_pow((int)(n % (int64_t)(kPmM - 1))));
    return s;
}

// One wave (workgroup) per individual; the rules of lahc_enter and lahc_plain_step on who
// writes what hold for the entry and for Move1 and Move2. A Kempe candidate adds words that one lane writes and another reads:
// K and F during the component search (a barrier after every round's reads and after
// every round's writes, as kempe_kernel), and on an applied chain the two slots' event
// bitsets (lane = word), the genes of the chain's events (lane = event of K) and the
// student masks (lane = (event of K, student) pair): the barrier after every applied
// move covers all three. klist, koff, kroom and occ are written by every lane with the
// same value.
// Loop bounds: `steps` steps. A Kempe step: at most |K| <= 128 rounds of the search, each
// over the EW64 frontier words and the frontier's events; two passes over the at most
// 128 events of K; ceil(pairs / 64) (event, student) pairs per lane, each with a binary
// search of 7 steps in koff.
//
// kAug with room_rule 1 (include/ttga_lahc_kempe_aug.h): the first event of K with no free
// possible room builds the two holder tables, hold[0] for slot a and hold[1] for slot t:
// lanes 0..63 clear them, a barrier, lane = word files the bystanders (set[s] & ~K, at most
// 64 a slot) and lane = index the chain events placed so far, a barrier; lane r then keeps
// poss[hold[s][r]] in a register for either table. From there on every placement writes
// hold, qpar and queue from every lane with the same value, as klist, and a lane reads
// back only what it wrote itself; after a path every lane reloads its word of the target's
// table. An accepted chain with tables writes sl / rr from them (lane = room: the chain's
// events and the displaced bystanders), covered by the barrier after every applied move.
// Loop bounds: one search queues every room at most once (V), so it pops at most R <= 64
// rooms and queues at most 64; a path has at most 64 rooms; a chain runs at most 128
// searches.
//
// kMulti (tt_lahc_multi.hip, include/ttga_lahc_multi.h): wave q of the launch is walker
// q % walkers of row q / walkers. It reads the row and rng[p] like any other walk, jumps to
// its own stretch of the stream, and writes to `work` only: its numbers, its exit row when
// it improved, and (the last walker) the stream state behind all of them. Everything it
// needs stands under `if constexpr (kMulti)`, so the other kernels compile to the
// instructions they had.
template <bool kAug, bool kMulti = false>
__device__ __forceinline__ void lahc_chain_walk(const DevProblem& pb, uint8_t* __restrict__ slot,
                                                uint8_t* __restrict__ room, int64_t* __restrict__ rng, int P, int steps,
                                                int L, double p_swap, double p_kempe, double kempe_from, int max_chain,
                                                int room_rule, int32_t* __restrict__ scv, int32_t* __restrict__ penalty,
                                                int32_t* __restrict__ gain, int32_t* __restrict__ accepted,
                                                int32_t* __restrict__ best_step, int32_t* __restrict__ kstats,
                                                int walkers = 1, void* work = nullptr) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    constexpr int kStats = kAug ? 7 : 5;
    const int E = pb.E, R = pb.R, S = pb.S, EW64 = pb.EW64, lane = threadIdx.x;
    const long q = blockIdx.x;                          // the launch's wave
    const long p = kMulti ? q / walkers : q;            // its row
    if (p >= P) return;
    uint64_t* set = (uint64_t*)lds;
    uint64_t* occ = set + (size_t)kSlots * EW64;
    uint64_t* K = occ + kSlots;
    uint64_t* F = K + EW64;
    uint64_t* mask = F + EW64;
    int32_t* hist = (int32_t*)(mask + S);
    int32_t* klist = hist + L;
    int32_t* koff = klist + kChainMax;
    uint8_t* sl = (uint8_t*)(koff + kChainMax + 4);
    uint8_t* rr = sl + E;
    uint8_t* bsl = rr + E;
    uint8_t* brr = bsl + E;
    uint8_t* kroom = brr + E;
    [[maybe_unused]] int16_t* hold = (int16_t*)(kroom + kChainMax);
    [[maybe_unused]] uint8_t* qpar = (uint8_t*)(hold + 2 * kMaxRooms);
    [[maybe_unused]] uint8_t* queue = qpar + kMaxRooms;

    // ---- entry: the row, validity, the bitsets and the hcv gate
    bool bad = false;
    for (int e = lane; e < E; e += 64) {
        const uint8_t s = slot[p * E + e], r = room[p * E + e];
        sl[e] = s;
        rr[e] = r;
        bad |= s >= kSlots || r >= R;
    }
    for (int i = lane; i < kSlots * EW64 + kSlots; i += 64) set[i] = 0ull;      // set and occ are adjacent
    for (int i = lane; i < L; i += 64) hist[i] = 0;                             // costs are kept relative to scv0
    __syncthreads();
    const bool bad_row = wave_any(bad);
    bool hard = false;                                  // a hard-constraint violation seen by this lane
    if (!bad_row) {
        for (int e = lane; e < E; e += 64) {
            const int s = sl[e], r = rr[e];
            atomicOr((unsigned long long*)&set[(size_t)s * EW64 + (e >> 6)], 1ull << (e & 63));
            const unsigned long long old = atomicOr((unsigned long long*)&occ[s], 1ull << r);
            hard |= ((old >> r) & 1ull) != 0ull;            // two events in one room of one slot
            hard |= ((pb.poss[e] >> r) & 1ull) == 0ull;     // a room that is not possible
        }
        // two correlated events share a student: they are in one slot exactly if some
        // student's events cover fewer slots than the student has events
        for (int s = lane; s < S; s += 64) {
            const int b = pb.stu_off[s], end = pb.stu_off[s + 1];
            uint64_t m = 0ull;
            for (int i = b; i < end; ++i) m |= 1ull << sl[pb.stu_ev[i]];
            mask[s] = m;
            hard |= __popcll(m) != end - b;
        }
        __syncthreads();
    }
    const LahcEntry in{bad_row || wave_any(hard) || steps == 0, bad_row};
    if (in.closed) {
        if constexpr (kMulti) {                         // a closed row: zeros, the flag among them
            if (lane < kLmNums) lahc_multi_work(work, P, walkers, E).nums[q * kLmNums + lane] = 0;
            if (in.bad_gene && lane == 0) atomicOr(pb.status, kStatusLahcBadGene);
            return;
        }
        return lahc_exit_closed(pb, {scv, penalty, gain, accepted, best_step, kstats}, kStats, p, in, lane);
    }

    // ---- the walk (cur and best relative to scv0)
    int64_t st = rng[p];
    if constexpr (kMulti) st = lahc_multi_start(st, steps, (int)(q - p * walkers));
    int cur = 0, best = 0, n_acc = 0, b_step = 0;
    int k_tried = 0, k_capped = 0, k_noroom = 0, k_acc = 0, k_events = 0;
    [[maybe_unused]] int k_rescued = 0, k_displaced = 0;
    bool live_is_best = true;                           // the best row is the row in sl / rr
    int v = 0;
    for (int k = 0; k < steps; ++k) {
        const int e1 = min(max(lahc_uniform(pm_pick(st, E)), 0), E - 1);
        const double u = pm_next(st), x = pm_next(st);
        const bool kempe = p_kempe > 0.0 && lahc_uniform((int)(u >= kempe_from)) != 0;
        const bool swap = !kempe && E >= 2 && lahc_uniform((int)(u < p_swap)) != 0;
        const int a = lahc_uniform((int)sl[e1]);
        if (kempe) {
            int b = lahc_uniform((int)__dmul_rn(x, (double)(kSlots - 1)));
            b += b >= a;
            b = min(max(b, 0), kSlots - 1);
            ++k_tried;
            // ---- the component of e1 in the events of slots a and b
            for (int w = lane; w < EW64; w += 64) {
                const uint64_t k0 = w == (e1 >> 6) ? 1ull << (e1 & 63) : 0ull;
                K[w] = k0;
                F[w] = k0;
            }
            __syncthreads();
            for (int round = 0; round < kChainMax; ++round) {
                uint64_t acc[kLkLaneWords];
#pragma unroll
                for (int j = 0; j < kLkLaneWords; ++j) acc[j] = 0ull;
                for (int fw = 0; fw < EW64; ++fw) {
                    uint64_t xw = wave_uniform64(F[fw]);        // one address for the wave
                    for (int g = 0; g < 64 && xw; ++g) {
                        const int f = 64 * fw + (__ffsll((unsigned long long)xw) - 1);
                        xw &= xw - 1;
                        const uint64_t* cr = pb.corr64 + (size_t)f * EW64;
#pragma unroll
                        for (int j = 0; j < kLkLaneWords; ++j)
                            if (64 * j + lane < EW64) acc[j] |= cr[64 * j + lane];
                    }
                }
                __syncthreads();                            // every lane has read the frontier
                bool grew = false;
#pragma unroll
                for (int j = 0; j < kLkLaneWords; ++j) {
                    const int w = 64 * j + lane;
                    if (w < EW64) {
                        const uint64_t nw = acc[j] & (set[(size_t)a * EW64 + w] | set[(size_t)b * EW64 + w]) & ~K[w];
                        K[w] |= nw;
                        F[w] = nw;
                        grew |= nw != 0ull;
                    }
                }
                const bool go_on = wave_any(grew);
                __syncthreads();
                if (!go_on) break;
                if (max_chain > 0) {                        // a part of K above the cap: K is, too
                    int part = 0;
                    for (int w = lane; w < EW64; w += 64) part += __popcll(K[w]);
                    if (wave_sum(part) > max_chain) break;
                }
            }
            int cnt = 0;
            for (int w = lane; w < EW64; w += 64) cnt += __popcll(K[w]);
            cnt = wave_sum(cnt);
            bool feas = cnt <= kChainMax;
            if (max_chain > 0 && cnt > max_chain) {
                ++k_capped;
                feas = false;
            }
            // ---- the rooms: the chain leaves its own, then takes new ones in ascending order
            uint64_t oa = occ[a], ob = occ[b];
            oa = wave_uniform64(oa);
            ob = wave_uniform64(ob);
            int n = 0, pairs = 0;
            [[maybe_unused]] bool built = false, augmented = false;     // the holder tables stand; a path was used
            [[maybe_unused]] uint64_t pwa = 0ull, pwb = 0ull;           // lane r: poss of the holder of room r in a, in t
            if (feas) {
                for (int w = 0; w < EW64; ++w) {
                    uint64_t xw = wave_uniform64(K[w]);
                    for (int g = 0; g < 64 && xw && n < kChainMax; ++g) {
                        const int e = 64 * w + (__ffsll((unsigned long long)xw) - 1);
                        xw &= xw - 1;
                        const uint64_t rbit = 1ull << lahc_uniform((int)rr[e]);
                        if (lahc_uniform((int)sl[e]) == a) oa &= ~rbit; else ob &= ~rbit;
                        klist[n] = e;
                        koff[n] = pairs;
                        pairs += pb.ev_off[e + 1] - pb.ev_off[e];
                        ++n;
                    }
                }
                koff[n] = pairs;
                if constexpr (!kAug) {
                    for (int i = 0; i < n; ++i) {
                        const int e = klist[i];
                        const bool to_b = lahc_uniform((int)sl[e]) == a;
                        const uint64_t f = wave_uniform64(pb.poss[e] & ~(to_b ? ob : oa));
                        if (f == 0ull) { feas = false; break; }
                        const int r = __ffsll((unsigned long long)f) - 1;
                        if (to_b) ob |= 1ull << r; else oa |= 1ull << r;
                        kroom[i] = (uint8_t)r;
                    }
                } else {
                    for (int i = 0; i < n; ++i) {
                        const int e = klist[i];
                        const bool to_b = lahc_uniform((int)sl[e]) == a;
                        const uint64_t pe = wave_uniform64(pb.poss[e]);
                        const uint64_t oc = to_b ? ob : oa;
                        int16_t* hd = hold + (to_b ? kMaxRooms : 0);        // the target slot's table
                        int r;
                        if ((pe & ~oc) != 0ull) {                           // step 1: the lowest free possible room
                            r = __ffsll((unsigned long long)(pe & ~oc)) - 1;
                            kroom[i] = (uint8_t)r;
                            if (built) {
                                hd[r] = (int16_t)e;
                                if (lane == r) { if (to_b) pwb = pe; else pwa = pe; }
                            }
                        } else {                                            // step 2: an augmenting path
                            if (room_rule == 0) { feas = false; break; }
                            if (!built) {
                                for (int q = lane; q < 2 * kMaxRooms; q += 64) hold[q] = -1;
                                __syncthreads();
                                for (int w = lane; w < EW64; w += 64) {
                                    const uint64_t kw = K[w];
                                    uint64_t xa = set[(size_t)a * EW64 + w] & ~kw, xb = set[(size_t)b * EW64 + w] & ~kw;
                                    for (int g = 0; g < 64 && xa; ++g) {
                                        const int h = 64 * w + (__ffsll((unsigned long long)xa) - 1);
                                        xa &= xa - 1;
                                        hold[rr[h]] = (int16_t)h;
                                    }
                                    for (int g = 0; g < 64 && xb; ++g) {
                                        const int h = 64 * w + (__ffsll((unsigned long long)xb) - 1);
                                        xb &= xb - 1;
                                        hold[kMaxRooms + rr[h]] = (int16_t)h;
                                    }
                                }
                                for (int j = lane; j < i; j += 64) {        // the chain events placed so far
                                    const int h = klist[j];
                                    hold[(sl[h] == a ? kMaxRooms : 0) + kroom[j]] = (int16_t)h;
                                }
                                __syncthreads();
                                const int ha = hold[lane], hb = hold[kMaxRooms + lane];
                                pwa = ha >= 0 ? pb.poss[ha] : 0ull;
                                pwb = hb >= 0 ? pb.poss[hb] : 0ull;
                                built = true;
                            }
                            const uint64_t pwt = to_b ? pwb : pwa;
                            uint64_t V = pe, xq = pe;
                            int head = 0, tail = 0;
                            r = -1;
                            for (int g = 0; g < kMaxRooms && xq; ++g) {
                                const int q = __ffsll((unsigned long long)xq) - 1;
                                xq &= xq - 1;
                                queue[tail++] = (uint8_t)q;
                                qpar[q] = (uint8_t)kLkRoot;
                            }
                            for (int pop = 0; pop < kMaxRooms && head < tail; ++pop) {
                                const int q = lahc_uniform((int)queue[head++]);
                                const uint64_t nw = lahc_lane64(pwt, q) & ~V;   // poss of q's holder, rooms not yet seen
                                if ((nw & ~oc) != 0ull) {
                                    r = __ffsll((unsigned long long)(nw & ~oc)) - 1;
                                    qpar[r] = (uint8_t)q;
                                    break;
                                }
                                uint64_t xn = nw;
                                for (int g = 0; g < kMaxRooms && xn && tail < kMaxRooms; ++g) {
                                    const int q2 = __ffsll((unsigned long long)xn) - 1;
                                    xn &= xn - 1;
                                    queue[tail++] = (uint8_t)q2;
                                    qpar[q2] = (uint8_t)q;
                                }
                                V |= nw;
                            }
                            if (r < 0) { feas = false; break; }
                            int q = r;                                      // every holder on the path moves up one room
                            for (int g = 0; g < kMaxRooms; ++g) {
                                const int par = lahc_uniform((int)qpar[q]);
                                if (par == kLkRoot) { hd[q] = (int16_t)e; break; }
                                hd[q] = hd[par];
                                q = par;
                            }
                            const int ht = hd[lane];
                            const uint64_t pw = ht >= 0 ? pb.poss[ht] : 0ull;
                            if (to_b) pwb = pw; else pwa = pw;
                            augmented = true;
                        }
                        if (to_b) ob |= 1ull << r; else oa |= 1ull << r;
                    }
                    if (feas && augmented) ++k_rescued;
                }
                if (!feas) ++k_noroom;
            }
            if (feas) {
                const uint64_t flip = (1ull << a) | (1ull << b);
                const int da = a / kSlotsPerDay, db = b / kSlotsPerDay;
                int d = 0;
                for (int i = lane; i < pairs; i += 64) {
                    int lo = 0, hi = n - 1;                 // the event of pair i: the last koff <= i
                    while (lo < hi) {
                        const int mid = (lo + hi + 1) >> 1;
                        if (koff[mid] <= i) lo = mid; else hi = mid - 1;
                    }
                    const uint64_t m = mask[pb.ev_stu[pb.ev_off[klist[lo]] + i - koff[lo]]];
                    if ((m & flip) != flip) d += lahc_mask_delta(m, flip, da, db);
                }
                const int cand = cur + wave_sum(d);
                if (cand <= cur || cand <= lahc_uniform(hist[v])) {
                    if (live_is_best && cand >= cur) {      // the row is about to leave the best one
                        for (int e = lane; e < E; e += 64) { bsl[e] = sl[e]; brr[e] = rr[e]; }
                        live_is_best = false;
                        __syncthreads();                    // other lanes write these genes below
                    }
                    for (int i = lane; i < pairs; i += 64) {
                        int lo = 0, hi = n - 1;
                        while (lo < hi) {
                            const int mid = (lo + hi + 1) >> 1;
                            if (koff[mid] <= i) lo = mid; else hi = mid - 1;
                        }
                        const int s = pb.ev_stu[pb.ev_off[klist[lo]] + i - koff[lo]];
                        const uint64_t m = mask[s];
                        if ((m & flip) != flip) mask[s] = m ^ flip;
                    }
                    for (int w = lane; w < EW64; w += 64) {
                        const uint64_t kw = K[w], sa = set[(size_t)a * EW64 + w], sb = set[(size_t)b * EW64 + w];
                        set[(size_t)a * EW64 + w] = (sa & ~kw) | (sb & kw);
                        set[(size_t)b * EW64 + w] = (sb & ~kw) | (sa & kw);
                    }
                    bool from_list = true;
                    if constexpr (kAug) {
                        if (built) {                            // lane = room: the chain's events and the displaced
                            int moved = 0;
                            for (int tb = 0; tb < 2; ++tb) {
                                const int h = hold[tb * kMaxRooms + lane];
                                if (h >= 0) {
                                    const bool in_k = ((K[h >> 6] >> (h & 63)) & 1ull) != 0ull;
                                    moved += !in_k && rr[h] != lane;
                                    sl[h] = (uint8_t)(tb ? b : a);
                                    rr[h] = (uint8_t)lane;
                                }
                            }
                            k_displaced += wave_sum(moved);
                            from_list = false;
                        }
                    }
                    if (from_list) {
                        for (int i = lane; i < n; i += 64) {
                            const int e = klist[i];
                            sl[e] = (uint8_t)(a + b - sl[e]);
                            rr[e] = kroom[i];
                        }
                    }
                    occ[a] = oa;
                    occ[b] = ob;
                    cur = cand;
                    ++n_acc;
                    ++k_acc;
                    k_events += n;
                    if (cur < best) {
                        best = cur;
                        b_step = k + 1;
                        live_is_best = true;
                    }
                    __syncthreads();                        // masks, bitsets, genes: one lane writes, another reads
                }
            }
            hist[v] = cur;
            v = v + 1 == L ? 0 : v + 1;
            continue;
        }
        const int off1 = pb.ev_off[e1], n1 = pb.ev_off[e1 + 1] - off1;
        int e2 = e1, b, r1, r2 = 0, off2 = 0, n2 = 0;
        bool feas;
        if (swap) {
            e2 = lahc_uniform((int)__dmul_rn(x, (double)(E - 1)));
            e2 += e2 >= e1;
            e2 = min(max(e2, 0), E - 1);
            b = lahc_uniform((int)sl[e2]);
            off2 = pb.ev_off[e2];
            n2 = pb.ev_off[e2 + 1] - off2;
            bool clash = false;
            for (int w = lane; w < EW64; w += 64) {
                uint64_t sb = set[(size_t)b * EW64 + w], sa = set[(size_t)a * EW64 + w];
                if (w == (e2 >> 6)) sb &= ~(1ull << (e2 & 63));
                if (w == (e1 >> 6)) sa &= ~(1ull << (e1 & 63));
                clash |= ((pb.corr64[(size_t)e1 * EW64 + w] & sb) | (pb.corr64[(size_t)e2 * EW64 + w] & sa)) != 0ull;
            }
            const uint64_t f1 = pb.poss[e1] & ~(occ[b] & ~(1ull << rr[e2]));
            const uint64_t f2 = pb.poss[e2] & ~(occ[a] & ~(1ull << rr[e1]));
            r1 = lahc_uniform(__ffsll((unsigned long long)f1) - 1);
            r2 = lahc_uniform(__ffsll((unsigned long long)f2) - 1);
            feas = a != b && r1 >= 0 && r2 >= 0 && !wave_any(clash);
        } else {
            b = lahc_uniform((int)__dmul_rn(x, (double)(kSlots - 1)));
            b += b >= a;
            b = min(max(b, 0), kSlots - 1);
            bool clash = false;
            for (int w = lane; w < EW64; w += 64)
                clash |= (pb.corr64[(size_t)e1 * EW64 + w] & set[(size_t)b * EW64 + w]) != 0ull;
            const uint64_t f1 = pb.poss[e1] & ~occ[b];
            r1 = lahc_uniform(__ffsll((unsigned long long)f1) - 1);
            feas = r1 >= 0 && !wave_any(clash);
        }
        if (feas) {
            // the students of e1, then (Move2) of e2; one who attends both keeps the mask:
            // the other slot's bit is set for nobody else, the candidate being feasible
            const uint64_t flip = (1ull << a) | (1ull << b);
            const int da = a / kSlotsPerDay, db = b / kSlotsPerDay, n = n1 + n2;
            int d = 0;
            for (int i = lane; i < n; i += 64) {
                const bool first = i < n1;
                const uint64_t m = mask[pb.ev_stu[first ? off1 + i : off2 + i - n1]];
                if (!swap || ((m >> (first ? b : a)) & 1ull) == 0ull) d += lahc_mask_delta(m, flip, da, db);
            }
            const int cand = cur + wave_sum(d);
            if (cand <= cur || cand <= lahc_uniform(hist[v])) {
                if (live_is_best && cand >= cur) {      // the row is about to leave the best one
                    for (int e = lane; e < E; e += 64) { bsl[e] = sl[e]; brr[e] = rr[e]; }
                    live_is_best = false;
                    __syncthreads();                    // every lane writes the moved genes below
                }
                for (int i = lane; i < n; i += 64) {
                    const bool first = i < n1;
                    const int s = pb.ev_stu[first ? off1 + i : off2 + i - n1];
                    const uint64_t m = mask[s];
                    if (!swap || ((m >> (first ? b : a)) & 1ull) == 0ull) mask[s] = m ^ flip;
                }
                const uint64_t bit1 = 1ull << (e1 & 63);
                uint64_t* wa1 = &set[(size_t)a * EW64 + (e1 >> 6)];
                uint64_t* wb1 = &set[(size_t)b * EW64 + (e1 >> 6)];
                *wa1 &= ~bit1;
                *wb1 |= bit1;
                const int ro1 = rr[e1];
                if (swap) {
                    const uint64_t bit2 = 1ull << (e2 & 63);
                    uint64_t* wb2 = &set[(size_t)b * EW64 + (e2 >> 6)];
                    uint64_t* wa2 = &set[(size_t)a * EW64 + (e2 >> 6)];
                    *wb2 &= ~bit2;
                    *wa2 |= bit2;
                    const int ro2 = rr[e2];
                    occ[a] = (occ[a] & ~(1ull << ro1)) | (1ull << r2);
                    occ[b] = (occ[b] & ~(1ull << ro2)) | (1ull << r1);
                    sl[e2] = (uint8_t)a;
                    rr[e2] = (uint8_t)r2;
                } else {
                    occ[a] &= ~(1ull << ro1);
                    occ[b] |= 1ull << r1;
                }
                sl[e1] = (uint8_t)b;
                rr[e1] = (uint8_t)r1;
                cur = cand;
                ++n_acc;
                if (cur < best) {
                    best = cur;
                    b_step = k + 1;
                    live_is_best = true;
                }
                __syncthreads();                        // the masks: written by one lane, read by another
            }
        }
        hist[v] = cur;
        v = v + 1 == L ? 0 : v + 1;
    }

    // ---- exit: the best row
    if constexpr (kMulti) {
        const LahcMultiWork mw = lahc_multi_work(work, P, walkers, E);
        if (b_step > 0) {
            const uint8_t* os = live_is_best ? sl : bsl;
            const uint8_t* orr = live_is_best ? rr : brr;
            uint8_t* row = mw.rows + (size_t)q * 2 * (size_t)E;
            for (int e = lane; e < E; e += 64) {
                row[e] = os[e];
                row[E + e] = orr[e];
            }
        }
        if (lane == 0) {
            int32_t* nm = mw.nums + q * kLmNums;
            nm[kLmGain] = -best;
            nm[kLmAccepted] = n_acc;
            nm[kLmBestStep] = b_step;
            nm[kLmStats + 0] = k_tried;
            nm[kLmStats + 1] = k_capped;
            nm[kLmStats + 2] = k_noroom;
            nm[kLmStats + 3] = k_acc;
            nm[kLmStats + 4] = k_events;
            if constexpr (kAug) {
                nm[kLmStats + 5] = k_rescued;
                nm[kLmStats + 6] = k_displaced;
            }
            nm[kLmWalked] = 1;
            nm[kLmWalked + 1] = 0;
            if (q - p * walkers == walkers - 1) mw.state[p] = st;     // s_K: the row's stream behind every walker
        }
        return;
    }
    if (b_step > 0) {
        const uint8_t* os = live_is_best ? sl : bsl;
        const uint8_t* orr = live_is_best ? rr : brr;
        for (int e = lane; e < E; e += 64) {
            slot[p * E + e] = os[e];
            room[p * E + e] = orr[e];
        }
    }
    if (lane == 0) {
        rng[p] = st;
        const int g = -best;
        if (gain) gain[p] = g;
        if (accepted) accepted[p] = n_acc;
        if (best_step) best_step[p] = b_step;
        if (scv) scv[p] -= g;
        if (penalty) {
            const int pen = penalty[p];
            if (pen >= 0 && pen < 1000000) penalty[p] = pen - g;
        }
        if (kstats) {
            kstats[p * kStats + 0] = k_tried;
            kstats[p * kStats + 1] = k_capped;
            kstats[p * kStats + 2] = k_noroom;
            kstats[p * kStats + 3] = k_acc;
            kstats[p * kStats + 4] = k_events;
            if constexpr (kAug) {
                kstats[p * kStats + 5] = k_rescued;
                kstats[p * kStats + 6] = k_displaced;
            }
        }
    }
}

// ---- the host's argument checks, shared by tt_lahc, tt_lahc_kempe, tt_lahc_kempe_aug and
// tt_lahc_multi (`fn`: the name in the messages), in three stages in the order the entry
// points have always made them; tt_lahc_multi makes its own checks between the stages.
// `kind` says which arguments the entry point has: p_kempe and max_chain come with the
// chains, room_rule with the tables.

// the population and the streams
inline int lahc_check_rows(const std::string& fn, const tt_problem* p, int P, const uint8_t* slot,
                           const uint8_t* room, const int64_t* rng) {
    const int rc = check_pop_args(p, P, slot, room);
    if (rc) return rc;
    if (!rng) { set_error(fn + ": null rng buffer"); return TT_ERR_INVALID; }
    return TT_OK;
}

// the walk's parameters
inline int lahc_check_walk(const std::string& fn, LahcKind kind, int steps, int history, double p_swap, double p_kempe,
                           int max_chain, int room_rule) {
    if (steps < 0) { set_error(fn + ": negative steps"); return TT_ERR_INVALID; }
    if (history < 1) { set_error(fn + ": history must be at least 1"); return TT_ERR_INVALID; }
    if (!(p_swap >= 0.0 && p_swap <= 1.0)) { set_error(fn + ": p_swap outside [0, 1]"); return TT_ERR_INVALID; }
    if (kind == kLahcPlain) return TT_OK;
    if (!(p_kempe >= 0.0 && p_kempe <= 1.0)) { set_error(fn + ": p_kempe outside [0, 1]"); return TT_ERR_INVALID; }
    if (max_chain < 0) { set_error(fn + ": negative max_chain"); return TT_ERR_INVALID; }
    if (kind == kLahcAug && room_rule != 0 && room_rule != 1) {
        set_error(fn + ": room_rule must be 0 or 1");
        return TT_ERR_INVALID;
    }
    if (!(p_swap <= 1.0 - p_kempe)) { set_error(fn + ": p_swap above 1 - p_kempe"); return TT_ERR_INVALID; }
    return TT_OK;
}

// the launch's LDS size into *lds, within the limit; made for P > 0 only
inline int lahc_check_lds(LahcKind kind, const tt_problem* p, int history, size_t* lds) {
    *lds = lahc_lds_bytes(kind, p->E, p->S, history);
    if (*lds > kLahcMaxLds || (kind != kLahcPlain && p->dev.EW64 > 64 * kLkLaneWords)) {
        const char* with[] = {"", " with Kempe chains", " with augmenting Kempe chains"};
        set_error(std::string("instance or history too large for the late-acceptance search") + with[kind]);
        return TT_ERR_LIMIT;
    }
    return TT_OK;
}

// the three stages of a single walk's entry point; TT_OK with P == 0 means there is nothing to do
inline int lahc_check_args(const char* fn, LahcKind kind, const tt_problem* p, int P, const uint8_t* slot,
                           const uint8_t* room, const int64_t* rng, int steps, int history, double p_swap,
                           double p_kempe, int max_chain, int room_rule, size_t* lds) {
    int rc = lahc_check_rows(fn, p, P, slot, room, rng);
    if (!rc) rc = lahc_check_walk(fn, kind, steps, history, p_swap, p_kempe, max_chain, room_rule);
    if (rc || P == 0) return rc;
    if ((rc = lahc_check_lds(kind, p, history, lds))) return rc;
    return check_rows_grid(fn, p, P, false);
}

}  // namespace ttga
