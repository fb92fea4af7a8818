/* ttga_lahc_multi.h -- parallel walkers for the late-acceptance walk of
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
#ifndef TTGA_LAHC_MULTI_H
#define TTGA_LAHC_MULTI_H

#include "ttga.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The bytes of tt_lahc_multi's `work` for a population of P rows and `walkers`
 * walkers a row: 8 P + (48 + 2 E) P walkers. 0 for invalid arguments: a NULL
 * problem, P < 0, walkers outside 1 .. 1024, or P * walkers past 2^31 - 1.
 * (The formula holds up to there; the call itself takes at most 67,108,863
 * walkers in all, see below, and refuses a larger product whatever `work` is.) */
size_t tt_lahc_multi_work_bytes(const tt_problem* p, int P, int walkers);

/* K = `walkers` independent walks of ttga_lahc_kempe_aug.h's tt_lahc_kempe_aug
 * from every row, each on its own stretch of the row's random stream; the best
 * of them comes back. The acceptance rule, the three kinds of candidate, the
 * history and the room rules are tt_lahc_kempe_aug's: a walker is one such
 * walk. For row i:
 *
 * Closed rows. An invalid row (a slot gene >= 45 or a room gene >= R) and a
 * row with hcv != 0 are as in tt_lahc_kempe_aug: untouched, rng[i] included,
 * and every per-row output is 0, winner[i] and the K entries of
 * walker_gain[i] among them. tt_device_status bit 8 is set for bad genes only.
 *
 * Walkers. Otherwise walker w = 0 .. K - 1 is tt_lahc_kempe_aug with the same
 * steps, history, p_swap, p_kempe, max_chain and room_rule, applied to a copy
 * of the entry row with stream state s_w: s_0 = rng[i], and s_(w+1) is s_w
 * after 3 * steps draws (every step draws exactly three numbers). So the call
 * equals K consecutive calls of tt_lahc_kempe_aug on fresh copies of the same
 * entry row, with the row's stream running on from one to the next.
 * walker_gain[i][w] is walker w's gain.
 *
 * Winner. The walker with the largest gain wins; ties go to the lowest w, so
 * if no walker improves the winner is 0 and the row is unchanged. slot[i] and
 * room[i] become the winner's exit row; gain[i], accepted[i], best_step[i] and
 * the seven kempe_stats are the winner's; scv[i] and penalty[i] are lowered by
 * gain[i] under tt_lahc's rule; winner[i] = w.
 *
 * Stream state. rng[i] becomes s_K, the state 3 * steps * K draws on, whatever
 * the winner. steps == 0 changes nothing (every output of every row is 0).
 *
 * Equivalences. With walkers == 1 the call is tt_lahc_kempe_aug, bit for bit,
 * in every buffer (winner 0, walker_gain = gain); `work` may then be NULL. So
 * with p_kempe 0 and room_rule 0 it is also tt_lahc, and with room_rule 0
 * tt_lahc_kempe. hcv stays 0 and scv never rises.
 *
 * walkers: 1 .. 1024. winner (device int32 [P], out) and walker_gain (device
 * int32 [P][walkers], out) may be NULL, as may scv, penalty, gain, accepted,
 * best_step and kempe_stats (device int32 [P][7]). work: device memory of
 * tt_lahc_multi_work_bytes(p, P, walkers) bytes, 8-byte aligned, the call's
 * own until it has finished on the stream: two calls that may overlap (two
 * streams) take two buffers. Its contents are unspecified before and after.
 * No walker writes slot, room, rng, scv or penalty: walkers write to `work`
 * only, and a second launch behind them on the same stream picks the winner
 * and commits the row.
 *
 * The other arguments as tt_lahc_kempe_aug. TT_ERR_INVALID: everything
 * tt_lahc_kempe_aug refuses; walkers outside 1 .. 1024; a NULL or misaligned
 * work with walkers > 1. TT_ERR_LIMIT: tt_lahc_kempe_aug's limit, for every
 * set of arguments (the walk that runs is always the one with augmenting
 * rooms, whatever p_kempe and room_rule):
 *     8 * (47 * ceil(E / 64) + 45 + S) + 4 * history + 4 * E + 1,552  <=  65,536,
 * or P * walkers past 67,108,863: every walker is a workgroup of one wave, and
 * a launch holds at most 2^32 - 1 threads (ttga.h, "Population size"). Either
 * launches nothing and touches no buffer. */
int tt_lahc_multi(const tt_problem* p, uint8_t* slot, uint8_t* room, int64_t* rng, int P, int walkers, int steps,
                  int history, double p_swap, double p_kempe, int max_chain, int room_rule, int32_t* scv,
                  int32_t* penalty, int32_t* gain, int32_t* accepted, int32_t* best_step, int32_t* kempe_stats,
                  int32_t* winner, int32_t* walker_gain, void* work, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* TTGA_LAHC_MULTI_H */
