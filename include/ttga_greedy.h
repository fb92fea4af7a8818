/* ttga_greedy.h -- a greedy constructive initial population on top of ttga.h:
 * the events ordered hardest first, and every individual built by placing
 * them in that order into a timeslot of least conflict, ties drawn from the
 * individual's own Random stream.
 *
 * An addition with no counterpart in the reference. Its call site would be the
 * RandomInitialSolution of ga.cpp:431 (the initial population); the three
 * discarded RandomInitialSolution calls of ga.cpp:543-548 are draws, not
 * solutions, and stay as they are (tt_ga_breed's skip_init_draws).
 *
 * Conventions as in ttga.h: TT_OK or a TT_ERR_* code, never an exception;
 * asynchronous on the caller's stream (no device-to-host copy and no
 * synchronisation inside a call); device buffers owned by the caller; no CPU
 * fallback.
 */
#ifndef TTGA_GREEDY_H
#define TTGA_GREEDY_H

#include "ttga.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of device work memory tt_greedy_order needs: 8 bytes per event, the
 * events rounded up to a power of two (at least 8). Depends on the instance
 * only; 0 for a null handle. */
size_t tt_greedy_work_bytes(const tt_problem* p);

/* order[0..E-1] (device int32): the events, hardest first.
 *   key[e] = 128 * deg(e) + (64 - |possibleRooms(e)|),
 *   deg(e) = the number of OTHER events correlated with e (eventCorrelations
 *   row, diagonal excluded); key descending, ties by event index ascending.
 * work: device scratch of tt_greedy_work_bytes(p) bytes. */
int tt_greedy_order(const tt_problem* p, int32_t* order, void* work, void* stream);

/* Greedy constructive counterpart of tt_random_init, same buffers plus `order`
 * (device int32 [E], from tt_greedy_order or the caller's own permutation).
 * Per individual i, with its own stream rng[i], the events are placed in
 * order[0], order[1], ...:
 *   cost(t) = the number of events already placed in slot t that are
 *             correlated with e, + 1 if slot t already holds >= R events;
 *   T = the slots of minimum cost, ascending; n = |T|;
 *   e goes to T[(int)(next() * n)]: exactly one draw per event, also when
 *   n == 1, so rng[i] advances by exactly E draws, as tt_random_init's does.
 * Then assignRooms on every slot (tt_assign_rooms). Writes slot[P][E], room[P][E].
 *
 * `order` is trusted to be a permutation of 0..E-1. If it is not, nothing is
 * written outside the rows: entry j outside 0..E-1 is skipped (draw j is still
 * consumed, so rng[i] advances by E all the same) and tt_device_status bit 5
 * (32) is set; an event that no entry names keeps slot 255 and room 255, an
 * invalid genome that tt_eval reports as -1; an event named twice is placed
 * twice and keeps the later slot (not detected, result otherwise undefined).
 *
 * Limit: exactly tt_assign_rooms's own, since the rooms come from it. An
 * instance whose matcher scratch does not fit the LDS returns TT_ERR_LIMIT and
 * launches nothing (rng, slot and room untouched). The scratch is about
 * 13 E + 90 R bytes for R <= 16 rooms and 4 E + 8 R + 9 KB for R > 16, against
 * 160 KB: E <= 12,521 at R = 1, 12,459 at R = 10, 12,417 at R = 16; E <= 38,380
 * at R = 17, 38,286 at R = 64. The placement itself fits any E.
 * P < 0 or a null pointer is TT_ERR_INVALID (a null handle named first);
 * P == 0 is TT_OK with no launch. */
int tt_greedy_init(const tt_problem* p, const int32_t* order, int64_t* rng, uint8_t* slot, uint8_t* room, int P,
                   void* stream);

#ifdef __cplusplus
}
#endif

#endif /* TTGA_GREEDY_H */
