/* ttga_lahc.h -- late-acceptance hill climbing (LAHC, Burke and Bykov) on top
 * of ttga.h: a walk of single-event moves over feasible timetables that
 * accepts a candidate when it is no worse than the current timetable or than
 * the one `history` steps ago, and returns the best timetable it has seen.
 *
 * An addition with no counterpart in the reference, whose only search that
 * lowers scv event by event is the first-improvement descent of phase 2 of
 * Solution::localSearch (Solution.cpp:471-769). The moves are the reference's
 * Move1 and Move2 (Solution.cpp:357-400), restricted to candidates that keep
 * every hard constraint and with the room chosen directly instead of by the
 * matcher. Its call site would follow the local search and the penalty of
 * ga.cpp:574-575.
 *
 * Conventions as in ttga.h: TT_OK or a TT_ERR_* code, never an exception;
 * asynchronous on the caller's stream (no device-to-host copy and no
 * synchronisation inside a call); device buffers owned by the caller; no CPU
 * fallback.
 */
#ifndef TTGA_LAHC_H
#define TTGA_LAHC_H

#include "ttga.h"

#ifdef __cplusplus
extern "C" {
#endif

/* In place on slot[P][E], room[P][E]; individual i uses its own stream rng[i]
 * (next() and (int)(next() * n) as everywhere in ttga.h). "Correlated" is
 * eventCorrelations[a][b] > 0, "possible" is possibleRooms[e][r] > 0, and a
 * room is occupied in a slot when some event of that slot has it as its room.
 * scv(.) is exactly Solution::computeScv. Per individual i:
 *
 *  1. Validity: a row with a slot gene >= 45 or a room gene >= R is left
 *     untouched, rng[i] included; gain[i] = accepted[i] = best_step[i] = 0 and
 *     tt_device_status bit 8 (256) is set; scv[i] and penalty[i] keep their
 *     value.
 *  2. Feasibility gate: the call computes the row's hcv itself, exactly as
 *     tt_eval defines it (two events in one room of one slot, correlated
 *     events in one slot, an event in a room that is not possible for it), and
 *     does not look at penalty[i]. A row with hcv != 0 is left untouched,
 *     rng[i] included; gain[i] = accepted[i] = best_step[i] = 0; scv[i] and
 *     penalty[i] keep their value. No status bit is set.
 *  3. State: scv0 = scv(row); cur = best = scv0; hist[0 .. L-1] = scv0 with
 *     L = history; the best row = the row; accepted = 0; best_step = 0.
 *  4. Step k = 0 .. steps-1, with v = k mod L. Every step draws exactly three
 *     numbers, whatever follows: e1 = (int)(next() * E); u = next();
 *     x = next().
 *       Move2 if E >= 2 and u < p_swap: e2 = (int)(x * (E - 1)), then
 *         e2 += 1 if e2 >= e1. Let a = slot[e1] and b = slot[e2]. The
 *         candidate is infeasible if a == b; if e1 is correlated with an event
 *         of slot b other than e2; or if e2 is correlated with an event of
 *         slot a other than e1. r1 = the lowest-numbered room that is possible
 *         for e1 and not occupied in slot b by an event other than e2; r2 =
 *         the lowest-numbered room that is possible for e2 and not occupied in
 *         slot a by an event other than e1. The candidate is infeasible if
 *         either room does not exist. Otherwise the candidate row is the row
 *         with e1 at (b, r1) and e2 at (a, r2).
 *       Move1 otherwise: t = (int)(x * 44), then t += 1 if t >= slot[e1]. The
 *         candidate is infeasible if e1 is correlated with any event of slot
 *         t, or if no room possible for e1 is unoccupied in slot t. Otherwise
 *         the candidate row is the row with e1 at (t, the lowest-numbered such
 *         room).
 *     For a feasible candidate, cand = cur + (scv(candidate row) - scv(row)).
 *     It is accepted iff cand <= cur or cand <= hist[v]. On acceptance the row
 *     becomes the candidate row, cur = cand and accepted += 1; if then
 *     cur < best: best = cur, the best row = the row and best_step = k + 1.
 *     An infeasible candidate is not accepted. In every case the step ends
 *     with hist[v] = cur.
 *  5. Exit: slot[i] and room[i] become the best row, i.e. the first row that
 *     reached the least cost of the walk, not the last current row.
 *     gain[i] = scv0 - best >= 0, accepted[i] = accepted, best_step[i] =
 *     best_step (0: the row is unchanged). If scv is given, scv[i] -= gain[i].
 *     If penalty is given and 0 <= penalty[i] < 1000000 (a feasible row, whose
 *     penalty is its scv), penalty[i] -= gain[i]. rng[i] has advanced by
 *     exactly 3 * steps draws.
 *
 * Invariants: every accepted candidate has hcv 0, so hcv stays 0; scv never
 * rises (the exit row is the best seen, at worst the row itself); no matcher
 * runs; the rooms of events that the walk never moved keep their values.
 *
 * scv, penalty (device int32 [P], in/out), gain, accepted and best_step
 * (device int32 [P], out) may each be NULL. P == 0 is TT_OK with no launch.
 * steps == 0 is valid and changes nothing (the outputs are 0). TT_ERR_INVALID
 * (a null handle named first): P < 0, a null handle, slot, room or rng,
 * steps < 0, history < 1, p_swap outside [0, 1] or NaN.
 *
 * Limit: one wave per individual keeps in LDS the slot row, the room row and
 * the best row (4 E bytes), 45 event bitsets of ceil(E / 64) 64-bit words,
 * 45 room-occupancy words, one 64-bit attendance mask per student and the
 * history:
 *     8 * (45 * ceil(E / 64) + 45 + S) + 4 * history + 4 * E  <=  65,536.
 * med (E 400, S 200) with history 500 takes 8,080 bytes; syn (E 2000, S 5000)
 * fits up to history 1,414. Anything larger returns TT_ERR_LIMIT and launches
 * nothing (every buffer untouched). */
int tt_lahc(const tt_problem* p, uint8_t* slot, uint8_t* room, int64_t* rng, int P, int steps, int history,
            double p_swap, int32_t* scv, int32_t* penalty, int32_t* gain, int32_t* accepted, int32_t* best_step,
            void* stream);

#ifdef __cplusplus
}
#endif

/* The same walk with Kempe-chain candidates as a third kind of move is
 * declared in ttga_lahc_kempe.h, which this header brings in. */
#include "ttga_lahc_kempe.h"

/* And that walk with the chains' rooms found by augmenting paths is declared
 * in ttga_lahc_kempe_aug.h. */
#include "ttga_lahc_kempe_aug.h"

/* And K such walks from every row at once, the best of them kept, are declared
 * in ttga_lahc_multi.h. */
#include "ttga_lahc_multi.h"

#endif /* TTGA_LAHC_H */
