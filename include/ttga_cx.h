/* ttga_cx.h -- a conflict-guided crossover on top of ttga.h: the child takes
 * every event's timeslot from one of its two parents, as the uniform crossover
 * does, but looks at what it has already placed: the parent's slot that brings
 * fewer clashes wins, the coin decides only between equals, and optionally an
 * event that clashes in both parents' slots is repaired into a slot of least
 * cost.
 *
 * An addition with no counterpart in the reference. Its call site would be the
 * crossover of ga.cpp:562-566 (Solution::crossover, Solution.cpp:893-910).
 *
 * Conventions as in ttga.h: TT_OK or a TT_ERR_* code, never an exception;
 * asynchronous on the caller's stream (no device-to-host copy and no
 * synchronisation inside a call); device buffers owned by the caller; no CPU
 * fallback.
 */
#ifndef TTGA_CX_H
#define TTGA_CX_H

#include "ttga.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Guided counterpart of tt_crossover, same buffers plus `order` (device int32
 * [E], from ttga_greedy.h's tt_greedy_order or the caller's own permutation),
 * `repair`, and two optional outputs `cost` and `repaired` (device int32 [P],
 * either may be NULL).
 *
 * Per individual i, with parents A = slot1[i], B = slot2[i] and its own stream
 * rng[i], the child's timeslots start empty. Then for j = 0 .. E-1, e = order[j]:
 *   1. u = next(): exactly one draw per entry, whatever follows, so rng[i]
 *      advances by exactly E draws, as tt_crossover's does.
 *   2. cost(t), 0 <= t < 45, as tt_greedy_init's: the number of events already
 *      placed in the child's slot t that are correlated with e
 *      (eventCorrelations[e][f] > 0, f != e), + 1 if slot t already holds >= R
 *      events.
 *   3. a = A[e], b = B[e]; ca = cost(a) if a < 45, else a value greater than
 *      every cost; cb likewise.
 *   4. if repair != 0 and min(ca, cb) > 0: T = the slots of minimum cost among
 *      0..44, ascending; t = T[(int)(u * |T|)]; repaired += 1;
 *      else if ca < cb: t = a; else if cb < ca: t = b;
 *      else t = (u < 0.5) ? a : b      (the reference's pick).
 *   5. child[e] = t. If t < 45, e joins slot t and cost_sum += cost(t). With
 *      repair != 0, t is always < 45; with repair == 0, t >= 45 happens only
 *      where both parents' genes are >= 45, and such an event is placed
 *      nowhere and counts for nothing.
 * Then the rooms are exactly what tt_assign_rooms writes for the child's slot
 * row (an event in a slot >= 45 keeps room 255). cost[i] = cost_sum, or -1 if
 * some event ended in a slot >= 45; repaired[i] = the events that took the
 * fallback of step 4 (0 when repair == 0). No status bit is set for parents'
 * genes.
 *
 * Consequences: with repair == 0 every child gene is A[e] or B[e]. On an
 * instance where every cost is 0 (no correlations and fewer than R events in
 * every slot), with order = 0..E-1, the result is tt_crossover's, bit for bit:
 * slot, room and rng.
 *
 * `order` is trusted to be a permutation of 0..E-1, handled as in
 * tt_greedy_init: entry j outside 0..E-1 is skipped (draw j is still consumed)
 * and tt_device_status bit 9 (512) is set; an event that no entry names keeps
 * slot 255 and room 255; an event named twice keeps the later slot (not
 * detected, result otherwise undefined).
 *
 * Limit: exactly tt_assign_rooms's own, as in tt_greedy_init: what does not fit
 * returns TT_ERR_LIMIT with nothing launched and nothing written. The placement
 * itself fits any E. P < 0 or a null slot1, slot2, order, rng, slot or room is
 * TT_ERR_INVALID (a null handle named first); P == 0 is TT_OK with no launch,
 * the buffers not looked at, as in tt_crossover. */
int tt_crossover_guided(const tt_problem* p, const uint8_t* slot1, const uint8_t* slot2, const int32_t* order,
                        int64_t* rng, uint8_t* slot, uint8_t* room, int P, int repair,
                        int32_t* cost, int32_t* repaired, void* stream);

/* tt_ga_breed with the guided crossover. Per child c, on rng[c], the same
 * sequence of draws as tt_ga_breed: the optional 3 E discarded draws, two
 * selection5 tournaments, the crossover draw. If the child crosses, the E
 * draws of the guided crossover above, of the two parents' slot rows, are
 * taken in order-entry sequence; otherwise the child is the copy of the first
 * parent's slot and room rows. The mutation draw and tt_mutation's move follow,
 * unchanged.
 *
 * Consequences: child_flags equal tt_ga_breed's for the same inputs; with
 * p_mut == 0, rng equals tt_ga_breed's; a child that did not cross is
 * identical to tt_ga_breed's child.
 *
 * child_cost[c] and child_repaired[c] (device int32 [C], either may be NULL)
 * are as defined above for a crossed child and 0 for a child that did not
 * cross. Argument checks are tt_ga_breed's, plus a null `order`; the limit is
 * tt_crossover_guided's (TT_ERR_LIMIT, nothing launched); C == 0 is TT_OK
 * with no launch, `order` not looked at. */
int tt_ga_breed_guided(const tt_problem* p, const uint8_t* pop_slot, const uint8_t* pop_room,
                       const int32_t* pop_penalty, int N, const int32_t* order, int64_t* rng, int C,
                       double p_cross, double p_mut, int skip_init_draws, int repair,
                       uint8_t* child_slot, uint8_t* child_room, uint8_t* child_flags,
                       int32_t* child_cost, int32_t* child_repaired, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* TTGA_CX_H */
