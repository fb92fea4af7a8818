/* ttga_slotswap.h -- the timeslot-swap descent on top of ttga.h: the contents
 * of two whole timeslots trade places, steepest descent over all 990 pairs.
 *
 * An addition with no counterpart in the reference, whose only perturbations
 * are Move1, Move2 and Move3 (Solution.cpp:357-439). The three soft
 * constraints of Solution::computeScv (Solution.cpp:86-139) depend only on
 * where in the week each slot's set of events sits, the hard constraints only
 * on which events share a slot: an exchange of two slots' contents changes
 * scv and nothing else. Its call site would follow the local search and the
 * penalty of ga.cpp:574-575.
 *
 * Conventions as in ttga.h: TT_OK or a TT_ERR_* code, never an exception;
 * asynchronous on the caller's stream (no device-to-host copy and no
 * synchronisation inside a call); device buffers owned by the caller; no CPU
 * fallback.
 */
#ifndef TTGA_SLOTSWAP_H
#define TTGA_SLOTSWAP_H

#include "ttga.h"

#ifdef __cplusplus
extern "C" {
#endif

/* In place on slot[P][E]; per individual i:
 *
 *  1. Validity: a row with a slot gene >= 45 is left untouched; gain[i] = 0,
 *     passes[i] = 0, perm[i] = the identity and tt_device_status bit 7 (128)
 *     is set; scv[i] and penalty[i] keep their value. Rooms are not an
 *     argument: the move never touches them.
 *  2. One pass: for every pair a < b of the 45 timeslots, delta(a, b) = the
 *     scv (exactly Solution::computeScv) of the row with the events of slots
 *     a and b exchanged, minus the scv of the row. The pair of least delta is
 *     taken, among equal deltas the least a, then the least b. If that delta
 *     is >= 0 the descent stops. Otherwise the exchange is applied (every
 *     event in a goes to b and every event in b to a), -delta is added to
 *     the gain and the pass counts as applied. The descent also stops once
 *     max_passes passes have been applied. Empty slots take part like any
 *     other.
 *  3. Outputs: gain[i] >= 0 = scv before - scv after; passes[i] = the applied
 *     swaps; perm[i][45] = the composed permutation, new slot[e] =
 *     perm[i][old slot[e]]. If scv is given, scv[i] -= gain[i]. If penalty is
 *     given and 0 <= penalty[i] < 1000000 (a feasible row, whose penalty is
 *     its scv), penalty[i] -= gain[i]; infeasible rows and the -1 sentinels
 *     keep their penalty.
 *
 * Invariants: the multiset of events per slot is only relabelled, so
 * TT_PART_ROOM_PAIRS, TT_PART_CORR_PAIRS, TT_PART_UNSUITABLE (ttga_report.h)
 * and every room stay exactly as they were, for any row, feasible or not. scv
 * strictly falls with each pass, so the descent ends without a cap after at
 * most the initial scv passes. No random numbers are drawn.
 *
 * scv, penalty (device int32 [P], in/out), gain, passes (device int32 [P],
 * out) and perm (device uint8 [P][45], out) may each be NULL. P == 0 is TT_OK
 * with no launch. TT_ERR_INVALID (a null handle named first): P < 0, a null
 * handle, a null slot, max_passes < 1.
 *
 * Limit: one wave per individual keeps the slot row and 15,264 bytes of
 * tables in LDS, against 64 KB: E + 15,264 <= 65,536, i.e. E <= 50,272. The
 * students are processed 64 at a time, so S has no limit. A larger instance
 * returns TT_ERR_LIMIT and launches nothing (every buffer untouched). */
int tt_slot_swap(const tt_problem* p, uint8_t* slot, int P, int max_passes, int32_t* scv, int32_t* penalty,
                 int32_t* gain, int32_t* passes, uint8_t* perm, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* TTGA_SLOTSWAP_H */
