/* ttga_lahc_kempe_aug.h -- rooms by augmenting paths for the Kempe-chain
 * candidates of the late-acceptance walk of ttga_lahc.h, which includes this
 * header: include that one.
 *
 * An addition with no counterpart in the reference; its call site is tt_lahc's,
 * behind the local search and the penalty of ga.cpp:574-575.
 *
 * Conventions as in ttga.h: TT_OK or a TT_ERR_* code, never an exception;
 * asynchronous on the caller's stream (no device-to-host copy and no
 * synchronisation inside a call); device buffers owned by the caller; no CPU
 * fallback.
 */
#ifndef TTGA_LAHC_KEMPE_AUG_H
#define TTGA_LAHC_KEMPE_AUG_H

#include "ttga.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ttga_lahc_kempe.h's tt_lahc_kempe with one more argument, room_rule, and
 * wider statistics. Only the room part of a Kempe candidate differs: the draws,
 * the component K, the cap, the change of scv, the acceptance rule, the
 * history, the exit with the best row and the in-place scv / penalty update are
 * tt_lahc_kempe's.
 *
 * room_rule 0 (direct) is tt_lahc_kempe's rule. room_rule 1 (augment): with
 * a = slot[e1] and t the second slot, hold[s] for each s of the two maps a room
 * to the event that holds it and starts with the events of s outside K at their
 * present rooms (the row is feasible: at most one event a room). The events of
 * K are taken in ascending event number; event e with target
 * s' = a + t - slot[e]:
 *
 *   1. Direct. If poss[e] has a room not held in hold[s'], e takes the lowest
 *      one (tt_lahc_kempe's rule).
 *   2. Augment. Otherwise V = poss[e], every room of which is held. A queue
 *      starts with the rooms of V, ascending, each with parent "e". Pop the
 *      front room r and let h = hold[s'][r], a bystander or an event of K
 *      placed earlier in this candidate, and new = poss[h] & ~V. If new has a
 *      room not held in hold[s'], take the lowest such room r* with parent r
 *      and stop; otherwise append the rooms of new to the queue, ascending,
 *      each with parent r, set V |= new and go on. On stopping at r*, walk the
 *      parents back: the holder of each room's parent moves into that room, and
 *      e takes the root room. If the queue empties the candidate is infeasible
 *      (no room) and nothing changes. Every room is queued at most once, so one
 *      search pops at most R <= 64 rooms.
 *
 * The candidate row is the row with every event of K at its target slot and
 * the room hold gives it; every bystander of a or t whose room in hold differs
 * from its present one goes to that room (a bystander may be displaced more
 * than once within a candidate); all other events keep slot and room. Rooms do
 * not enter scv, so the change of scv is the one tt_lahc_kempe computes.
 *
 * Consequences: where step 2 never runs the candidate is tt_lahc_kempe's, bit
 * for bit. With room_rule 0 the whole call is tt_lahc_kempe, bit for bit, in
 * every output and stream state, and the two new counts are 0. By Berge's
 * theorem "no room" is exact under room_rule 1: a candidate is refused for
 * rooms only if the events that slot a or slot t would hold have no complete
 * assignment to possible rooms at all, in any order. hcv stays 0 and scv never
 * rises. An event keeps its room unless it was in an accepted chain or was a
 * bystander of an accepted chain's two slots that a path displaced.
 *
 * kempe_stats (device int32 [P][7], out, may be NULL) receives per individual
 * the five counts of tt_lahc_kempe, then `rescued`: the Kempe candidates,
 * accepted or not, in which every event found a room and at least one needed
 * step 2, and `displaced`: summed over the accepted chains, the bystanders
 * whose room changed. A row that is invalid or fails the gate gets seven zeros.
 *
 * Arguments as tt_lahc_kempe. TT_ERR_INVALID in addition: room_rule other than
 * 0 or 1. An invalid call launches nothing and touches no buffer.
 *
 * Limit: tt_lahc_kempe's LDS image plus the search's state, 384 bytes: two
 * holder tables of 64 rooms (int16 events, 256 bytes) and the parents and the
 * queue of one search (64 bytes each):
 *     8 * (47 * ceil(E / 64) + 45 + S) + 4 * history + 4 * E + 1,552  <=  65,536.
 * sm (E 100, S 80) takes 3,704 bytes without the history; syn's E and S (2000,
 * 5000) fit up to history 898. Anything larger returns TT_ERR_LIMIT and
 * launches nothing (every buffer untouched). */
int tt_lahc_kempe_aug(const tt_problem* p, uint8_t* slot, uint8_t* room, int64_t* rng, int P, int steps, int history,
                      double p_swap, double p_kempe, int max_chain, int room_rule, int32_t* scv, int32_t* penalty,
                      int32_t* gain, int32_t* accepted, int32_t* best_step, int32_t* kempe_stats, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* TTGA_LAHC_KEMPE_AUG_H */
