/* ttga/move1.h -- the full single-event neighbourhood of a feasible timetable
 * on top of ttga.h: for every event and every timeslot, what the move "this
 * event goes to that slot" does to scv and which room it would take
 * (tt_move1_scan), and the steepest descent built on that table
 * (tt_move1_descent).
 *
 * An addition with no counterpart in the reference, whose searches only sample
 * this neighbourhood: phase 2 of Solution::localSearch (Solution.cpp:471-769)
 * takes the first improving move it meets. The move is the reference's Move1
 * (Solution.cpp:357-370), restricted as in ttga_lahc.h to candidates that keep
 * every hard constraint and with the room chosen directly instead of by the
 * matcher. The descent's call site would follow the local search and the
 * penalty of ga.cpp:574-575, after the walk of ttga_lahc.h.
 *
 * This header sits in include/ttga/ and not beside the ttga_*.h additions; a
 * consumer includes "ttga/move1.h" with the same -I include (DESIGN.md says
 * why).
 *
 * Conventions as in ttga.h: TT_OK or a TT_ERR_* code, never an exception;
 * asynchronous on the caller's stream (no device-to-host copy and no
 * synchronisation inside a call); device buffers owned by the caller; no CPU
 * fallback.
 */
#ifndef TTGA_MOVE1_H
#define TTGA_MOVE1_H

#include "../ttga.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TT_MOVE1_CLASH     255   /* to_room: a correlated event sits in slot t            */
#define TT_MOVE1_NO_ROOM   254   /* to_room: no clash, but no possible room is free in t  */
#define TT_MOVE1_UNSCANNED 253   /* to_room of a row that was not scanned                 */
#define TT_MOVE1_NONE 0x7fffffff /* d_scv of a row that was not scanned                   */

/* Reads slot[P][E] and room[P][E]. "Correlated" is eventCorrelations[a][b] > 0,
 * "possible" is possibleRooms[e][r] > 0, and a room is occupied in a slot when
 * some event of that slot has it as its room, as in ttga_lahc.h. scv(.) is
 * exactly Solution::computeScv. Per individual i:
 *
 *  1. Validity: a row with a slot gene >= 45 or a room gene >= R is not
 *     scanned, and tt_device_status bit 10 (1024) is set.
 *  2. Feasibility gate: the call computes the row's hcv itself, exactly as
 *     tt_lahc's step 2 does, from the row alone. A row with hcv != 0 is not
 *     scanned. No status bit is set.
 *  3. A row that is not scanned: summary[i] = {0, 0, 0, 0, -1, -1}, every
 *     d_scv[i][e][t] = TT_MOVE1_NONE and every to_room[i][e][t] =
 *     TT_MOVE1_UNSCANNED.
 *  4. A scanned row, for every event e and every slot t = 0 .. 44:
 *       d_scv[i][e][t] = scv(the row with slot[e] = t) - scv(the row), for
 *         every t, whether or not that row keeps hcv 0 (scv does not depend on
 *         the rooms). It is 0 at t == slot[e].
 *       to_room[i][e][t] = room[e] at t == slot[e]; else TT_MOVE1_CLASH if e is
 *         correlated with any event of slot t; else the lowest-numbered room
 *         that is possible for e and not occupied in slot t, or
 *         TT_MOVE1_NO_ROOM if there is none. This is tt_lahc's Move1 rule.
 *     An entry with to_room < 64 and t != slot[e] is a feasible move: the row
 *     with e at (t, that room) has hcv 0 and its scv differs by d_scv.
 *  5. Summary of a scanned row: summary[i] = {1, the feasible moves, the
 *     feasible moves with d_scv < 0, the least d_scv over the feasible moves,
 *     its event, its slot}; among equal d_scv the least event, then the least
 *     slot. With no feasible move it is {1, 0, 0, 0, -1, -1}.
 *
 * summary (device int32 [P][6]), d_scv (device int32 [P][E][45]) and to_room
 * (device uint8 [P][E][45]), all out, may each be NULL; with all three NULL
 * the call is TT_OK and launches nothing. P == 0 is TT_OK with no launch.
 * TT_ERR_INVALID (a null handle named first): P < 0, a null handle, a null
 * slot or room (also with P == 0). The scan draws no random numbers and writes neither input.
 * Placement as in ttga.h: the int32 buffers 4-byte aligned, the uint8 buffers
 * at any byte. Every offset is 64-bit: i * E * 45 may pass 2^32 elements, and
 * d_scv 2^32 bytes from P * E >= 23.9 million on. The largest P is 67,108,863
 * (one wave a row); more returns TT_ERR_LIMIT with nothing launched.
 *
 * Limit: one wave per individual keeps in LDS the slot row and the room row
 * (2 E bytes), 45 event bitsets of ceil(E / 64) 64-bit words, 45
 * room-occupancy words and one 64-bit attendance mask per student -- tt_lahc's
 * image without the history and the best row:
 *     8 * (45 * ceil(E / 64) + 45 + S) + 2 * E  <=  65,536.
 * sm (E 100, S 80) takes 1,920 bytes, med (E 400, S 200) 5,280, syn (E 2000,
 * S 5000) 55,880. Anything larger returns TT_ERR_LIMIT and launches nothing
 * (every buffer untouched). The call keeps no state on the handle: several
 * host threads may call it on streams of their own. */
int tt_move1_scan(const tt_problem* p, const uint8_t* slot, const uint8_t* room, int P, int32_t* summary,
                  int32_t* d_scv, uint8_t* to_room, void* stream);

/* Steepest descent over that neighbourhood, in place on slot[P][E] and
 * room[P][E]. Per individual i:
 *
 *  1. Validity and the feasibility gate are tt_move1_scan's, the status bit
 *     included. A row that is not scanned is left untouched; gain[i] =
 *     passes[i] = 0; scv[i] and penalty[i] keep their value.
 *  2. One pass takes tt_move1_scan's summary of the current row. If it has no
 *     feasible move, or its least d_scv is >= 0, the descent stops. Otherwise
 *     that move is applied: the event goes to the slot and to the to_room
 *     room; -d_scv is added to the gain and the pass counts as applied. The
 *     descent also stops once max_passes passes have been applied.
 *  3. Outputs: gain[i] >= 0 = scv before - scv after; passes[i] = the applied
 *     moves. If scv is given, scv[i] -= gain[i]. If penalty is given and
 *     0 <= penalty[i] < 1000000 (a feasible row, whose penalty is its scv),
 *     penalty[i] -= gain[i]: tt_lahc's step 5.
 *
 * Invariants: hcv stays 0 and scv strictly falls with each pass, so the
 * descent ends without a cap after at most the initial scv passes; the rooms
 * of events that no pass moved keep their values; no random numbers are drawn;
 * a descent that returns passes[i] < max_passes leaves a row whose scan has no
 * improving move (summary[i][2] == 0); the call equals max_passes rounds of
 * "tt_move1_scan, apply the summary's move" made by the host. Every pass
 * recomputes the whole table.
 *
 * scv, penalty (device int32 [P], in/out), gain and passes (device int32 [P],
 * out) may each be NULL. P == 0 is TT_OK with no launch. TT_ERR_INVALID (a
 * null handle named first): P < 0, a null handle, a null slot or room,
 * max_passes < 1. The LDS limit and the largest P are tt_move1_scan's. */
int tt_move1_descent(const tt_problem* p, uint8_t* slot, uint8_t* room, int P, int max_passes, int32_t* scv,
                     int32_t* penalty, int32_t* gain, int32_t* passes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* TTGA_MOVE1_H */
