/* ttga_unique.h -- duplicate-free replacement on top of ttga.h: drop the
 * children of a generation that are already in the population, and find the
 * first occurrence of every genome of a population.
 *
 * An addition with no counterpart in ga.cpp. Its call site would be next to
 * pop[popSize-1]->copy(child) (ga.cpp:582): skip the copy when the child is
 * already in pop.
 *
 * A genome is an individual's slot row followed by its room row, 2*E bytes;
 * two individuals are duplicates when these bytes are equal (penalties play
 * no part). A 32-bit hash of the row only nominates candidates: every
 * equality reported is a full comparison of the 2*E bytes.
 *
 * hash_bits (both entry points): 0 uses the whole hash, 1..31 only that many
 * low bits of it -- more candidates, the same results (a test and profiling
 * knob, as tt_eval_variant's variants); any other value is TT_ERR_INVALID.
 *
 * Conventions as in ttga.h: TT_OK or a TT_ERR_* code, never an exception;
 * asynchronous on the caller's stream (no device-to-host copy and no
 * synchronisation inside a call); device buffers owned by the caller; no CPU
 * fallback.
 */
#ifndef TTGA_UNIQUE_H
#define TTGA_UNIQUE_H

#include "ttga.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of device work memory tt_genome_first needs for P individuals (0 for
 * P < 1 or E < 1). */
size_t tt_genome_work_bytes(int P, int E);

/* first[i] = the lowest j <= i whose genome equals i's: first[i] == i exactly
 * for the first individual of each kind, so the number of such i is the
 * number of distinct genomes.
 *   slot, room: [P][E] (device, uint8); first[P] (device, int32);
 *   work: tt_genome_work_bytes(P, E) bytes (device). */
int tt_genome_first(const tt_problem* p, const uint8_t* slot, const uint8_t* room, int P, int32_t* first,
                    int hash_bits, void* work, void* stream);

/* Bytes of device work memory tt_ga_replace_unique needs (0 for N < 1, C < 0
 * or E < 1); at least tt_ga_work_bytes of (N, E), and the source word is at
 * tt_ga_work_source_offset of (N, E) as in tt_ga_replace's buffer. */
size_t tt_ga_unique_work_bytes(int N, int C, int E);

/* tt_ga_replace without duplicates. Child c is dropped when its genome equals
 * the genome of any of the N population members (one at a position about to
 * be overwritten counts too) or of a child with a lower index; otherwise it is
 * kept. With D kept children the result is exactly tt_ga_replace's for the
 * same population and the kept children, in child order, as its C = D
 * children: they overwrite positions N-D..N-1, and the population is sorted by
 * penalty (as unsigned), ties in position order. D = 0 only sorts. A
 * population of pairwise distinct genomes stays pairwise distinct.
 *   child_keep[C] (device, uint8): 1 kept, 0 dropped;
 *   n_kept[1] (device, int32): D, which the host never reads inside the call;
 *   the int32 at tt_ga_work_source_offset of (N, E) in work: where the new pop[0]
 *   came from, its old position p < N for a member, N + c for child c (c the
 *   index among all C children);
 *   work: tt_ga_unique_work_bytes(N, C, E) bytes (device).
 * C = 0 is tt_ga_replace with C = 0 (child_keep unused; n_kept, if given, 0). */
int tt_ga_replace_unique(const tt_problem* p, uint8_t* pop_slot, uint8_t* pop_room, int32_t* pop_hcv,
                         int32_t* pop_scv, uint8_t* pop_feasible, int32_t* pop_penalty, int N,
                         const uint8_t* child_slot, const uint8_t* child_room, const int32_t* child_hcv,
                         const int32_t* child_scv, const uint8_t* child_feasible, const int32_t* child_penalty,
                         int C, uint8_t* child_keep, int32_t* n_kept, int hash_bits, void* work, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* TTGA_UNIQUE_H */
