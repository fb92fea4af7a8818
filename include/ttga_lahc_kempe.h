/* ttga_lahc_kempe.h -- Kempe-chain candidates in the late-acceptance walk of
 * ttga_lahc.h, which includes this header: include that one.
 *
 * An addition with no counterpart in the reference; its call site is tt_lahc's,
 * behind the local search and the penalty of ga.cpp:574-575.
 *
 * Conventions as in ttga.h: TT_OK or a TT_ERR_* code, never an exception;
 * asynchronous on the caller's stream (no device-to-host copy and no
 * synchronisation inside a call); device buffers owned by the caller; no CPU
 * fallback.
 */
#ifndef TTGA_LAHC_KEMPE_H
#define TTGA_LAHC_KEMPE_H

#include "ttga.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ttga_lahc.h's tt_lahc with a third kind of candidate, the Kempe-chain
 * interchange of ttga_kempe.h inside the cost-controlled walk: where Move1 is refused because
 * of a correlated event in the target slot, the chain moves the clash along.
 * Everything tt_lahc's comment says holds unchanged -- validity, the
 * feasibility gate, the state, three draws per step, the acceptance rule,
 * hist[v] = cur at the end of every step, the exit with the best row, the
 * in-place scv / penalty update, 3 * steps draws -- except step 4's choice of
 * move. With a = slot[e1] and the threshold 1.0 - p_kempe computed once in
 * double:
 *
 *   Kempe if p_kempe > 0 and u >= 1.0 - p_kempe (tested first):
 *     t = (int)(x * 44), then t += 1 if t >= a (Move1's target). U = the events
 *     of slots a and t; K = the connected component of e1 in the graph on U
 *     whose edges are all correlated pairs (ttga_kempe.h step 4). If
 *     max_chain > 0 and |K| > max_chain the candidate is infeasible (capped).
 *     Otherwise the rooms are chosen with no matcher: occ'[a] = the rooms
 *     occupied in a by events of a outside K, occ'[t] likewise; the events of K
 *     are taken in ascending event number, and event e with target
 *     s' = a + t - slot[e] gets the lowest-numbered room that is possible for e
 *     and not in occ'[s'], which then joins occ'[s']. If an event finds no room
 *     the candidate is infeasible (no room). The candidate row is the row with
 *     every event of K at its target slot and that room; events outside K keep
 *     slot and room.
 *   Move2 if E >= 2 and u < p_swap, exactly as in tt_lahc.
 *   Move1 otherwise, exactly as in tt_lahc.
 *
 * cand = cur + (scv(candidate row) - scv(row)) and the acceptance rule are
 * tt_lahc's. K is a whole component, so no event of K is correlated with an
 * event of U \ K and the candidate keeps hcv 0 whenever every event finds a
 * room. A student of an event of K attends either one event of U, and then
 * changes sides with it, or one event on each side, both in K, and then attends
 * both slots before and after.
 *
 * kempe_stats (device int32 [P][5], out, may be NULL) receives per individual:
 * the Kempe candidates drawn, those capped, those with no room, those accepted,
 * and the sum of |K| over the accepted ones. A row that is invalid or fails the
 * gate gets five zeros.
 *
 * Invariants: hcv stays 0; scv never rises; the rooms of events that never
 * moved keep their values; accepted[i] counts all three kinds of move. With
 * p_kempe == 0 the call is tt_lahc, bit for bit, in every output and stream
 * state (and kempe_stats is all 0).
 *
 * Arguments as tt_lahc. TT_ERR_INVALID in addition: p_kempe outside [0, 1] or
 * NaN, max_chain < 0, or not p_swap <= 1.0 - p_kempe.
 *
 * Limit: tt_lahc's LDS image plus two event bitsets (the chain and the
 * frontier of its search; U is read off the two slots' bitsets) and the list
 * of K, which on a feasible row has at most 2 R <= 128 events (1,168 bytes:
 * 128 events, 132 offsets, 128 rooms):
 *     8 * (47 * ceil(E / 64) + 45 + S) + 4 * history + 4 * E + 1,168  <=  65,536.
 * sm (E 100, S 80) takes 3,320 bytes without the history; syn's E and S (2000,
 * 5000) fit up to history 994. Anything larger returns TT_ERR_LIMIT and
 * launches nothing (every buffer untouched). */
int tt_lahc_kempe(const tt_problem* p, uint8_t* slot, uint8_t* room, int64_t* rng, int P, int steps, int history,
                  double p_swap, double p_kempe, int max_chain, int32_t* scv, int32_t* penalty, int32_t* gain,
                  int32_t* accepted, int32_t* best_step, int32_t* kempe_stats, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* TTGA_LAHC_KEMPE_H */
