/* ttga_report.h -- population report on top of ttga.h: which constraint an
 * individual violates, which events are in conflict, and how different the
 * individuals of a population still are.
 *
 * An addition with no call site in ga.cpp. The nearest reference code is
 * Solution::eventHcv (Solution.cpp:173-191) and the loops of computeHcv /
 * computeScv (Solution.cpp:86-170), whose terms tt_eval adds up and the
 * entry points below keep apart.
 *
 * Conventions as in ttga.h: TT_OK or a TT_ERR_* code, never an exception;
 * asynchronous on the caller's stream; device buffers owned by the caller; no
 * CPU fallback.
 */
#ifndef TTGA_REPORT_H
#define TTGA_REPORT_H

#include "ttga.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TT_NUM_PARTS 6
/* order of the parts; the names are ttga/validate.py's keys */
#define TT_PART_ROOM_PAIRS   0  /* pairs i<j sharing slot and room            Solution.cpp:148-150 */
#define TT_PART_CORR_PAIRS   1  /* pairs i<j sharing a slot and a student     :151-153 */
#define TT_PART_UNSUITABLE   2  /* events in a room not in possibleRooms      :155-156 */
#define TT_PART_LAST_SLOT    3  /* sum of studentNumber over slot % 9 == 8    :93-96  */
#define TT_PART_CONSECUTIVE  4  /* student-day runs, each class beyond two    :98-117 */
#define TT_PART_SINGLE_CLASS 5  /* (student, day) with exactly one class      :119-137 */

/* The six constraint parts of every individual: parts[i][0..2] add up to
 * tt_eval's hcv[i], parts[i][3..5] to its scv[i]. With event_hcv != NULL also
 * Solution::eventHcv of every event: event_hcv[i][e] = the other events in e's
 * slot that share its room + the other events in e's slot correlated with it
 * (room suitability is not part of it, as in the reference), so a row sums to
 * 2 * (parts[i][0] + parts[i][1]). An individual with slot >= 45 or room >= R
 * gets -1 in all six parts and in its whole event_hcv row.
 *   parts[P][6], event_hcv[P][E] or NULL (device, int32). */
int tt_eval_parts(const tt_problem* p, const uint8_t* slot, const uint8_t* room, int P, int32_t* parts,
                  int32_t* event_hcv, void* stream);

/* hist[e][t] = the number of individuals i with slot[i][e] == t; genes >= 45
 * are counted nowhere. The output is overwritten (all zero for P = 0).
 *   hist[E][45] (device, int32). */
int tt_slot_histogram(const tt_problem* p, const uint8_t* slot, int P, int32_t* hist, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* TTGA_REPORT_H */
