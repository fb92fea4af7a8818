/* ttga_kempe.h -- the Kempe-chain interchange on top of ttga.h: one event, a
 * second timeslot, and the connected component of the event in the conflict
 * graph of the two slots changes sides as a whole.
 *
 * An addition with no counterpart in the reference, whose only perturbations
 * are Move1, Move2 and Move3 (Solution.cpp:357-439). Its call site would
 * follow the mutation of ga.cpp:571, before the local search of ga.cpp:574.
 *
 * Conventions as in ttga.h: TT_OK or a TT_ERR_* code, never an exception;
 * asynchronous on the caller's stream (no device-to-host copy and no
 * synchronisation inside a call); device buffers owned by the caller; no CPU
 * fallback.
 */
#ifndef TTGA_KEMPE_H
#define TTGA_KEMPE_H

#include "ttga.h"

#ifdef __cplusplus
extern "C" {
#endif

/* In place on slot[P][E], room[P][E]; individual i uses its own stream rng[i]
 * (next() and (int)(next() * n) as everywhere in ttga.h).
 *
 *  1. Validity: a row with a slot gene >= 45 or a room gene >= R is left
 *     untouched, rng[i] included; chain_len[i] = 0 and tt_device_status bit 6
 *     (64) is set.
 *  2. Gate: u = next(). Unless u < prob: chain_len[i] = 0, the row is unchanged
 *     and one draw is gone. prob 1.0 moves every valid individual, 0.0 none.
 *  3. Choice: e = (int)(next() * E), t1 = slot[i][e], t2 = (int)(next() * 44),
 *     t2 += 1 if t2 >= t1. An individual past the gate consumes exactly three
 *     draws, whatever follows.
 *  4. Chain: U = the events whose slot is t1 or t2; K = the connected
 *     component of e in the graph on U whose edges are ALL correlated pairs
 *     a != b, eventCorrelations[a][b] > 0, pairs inside one slot included.
 *  5. Cap: if max_chain > 0 and |K| > max_chain the row is unchanged and
 *     chain_len[i] = -|K|. max_chain == 0: no cap.
 *  6. Apply: every event of K gets slot t1 + t2 - slot; chain_len[i] = |K|.
 *     Slots t1 and t2 are then re-matched as tt_mutation re-matches the slots
 *     it touched: the reference's assignRooms rule, the limit of 256 events
 *     per slot and status bit 0 as in tt_assign_rooms. Rooms of events in any
 *     other slot keep their value.
 *
 * Invariant: K is a whole component, so no event of K is correlated with an
 * event of U \ K. Both events of a correlated pair inside K change sides, so
 * the pair shares a slot after the move exactly if it did before; a pair
 * inside U \ K does not move; and no correlated pair joins K to U \ K or
 * involves another slot's events differently than before. The correlated-pairs
 * part of hcv (ttga_report.h TT_PART_CORR_PAIRS) is therefore exactly the same
 * before and after, for any row, feasible or not, however many events move.
 *
 * chain_len (device int32 [P]) may be NULL. P == 0 is TT_OK with no launch.
 * TT_ERR_INVALID (a null handle named first): P < 0, a null handle, slot,
 * room or rng, max_chain < 0, prob outside [0, 1] or NaN.
 *
 * Limit: one wave per individual keeps the matcher's scratch (tt_mutation's:
 * about 13 E + 90 R bytes for R <= 16 rooms, 4 E + 8 R + 9 KB for R > 16) and
 * three event bitsets of 8 * ceil(E / 64) bytes each in LDS, against 160 KB:
 * E <= 12,108 at R = 10 and E <= 36,688 at R = 17 (from the formula). A larger
 * instance returns TT_ERR_LIMIT and launches nothing (every buffer untouched). */
int tt_kempe_move(const tt_problem* p, uint8_t* slot, uint8_t* room, int64_t* rng, int P, double prob, int max_chain,
                  int32_t* chain_len, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* TTGA_KEMPE_H */
