"""Pure-Python statement of tt_lahc_kempe (include/ttga_lahc.h), written from
the header on top of tests/lahc_model.py: the chain as a connected component
on Python-int bitsets, the rooms by the header's ascending rule, the change of
scv by recomputing the scv of the whole candidate row (scv_of), the draws from
ttga.rng.ParkMiller."""
import numpy as np

import lahc_model as lm
from lahc_model import SLOTS
from ttga.rng import ParkMiller

STAT_NAMES = ("tried", "capped", "no_room", "accepted", "chain_events")


def _events(bits):
    """The set bits of a Python int, ascending."""
    out = []
    while bits:
        low = bits & -bits
        out.append(low.bit_length() - 1)
        bits ^= low
    return out


def _lowest(bits):
    return (bits & -bits).bit_length() - 1


class Model(lm.Model):
    def component(self, u, e1):
        """The connected component of e1 in the graph on the events of bitset u
        whose edges are all correlated pairs (ttga_kempe.h step 4), as a bitset."""
        k = frontier = 1 << e1
        while frontier:
            reach = 0
            for f in _events(frontier):
                reach |= self.corr[f]
            frontier = reach & u & ~k
            k |= frontier
        return k

    def chain_rooms(self, slot, room, occ, k, a, t, descending=False):
        """The header's room rule for chain k between slots a and t:
        [(e, target, room)] in ascending event number, or None (no room)."""
        free = {a: occ[a], t: occ[t]}
        for e in _events(k):
            free[int(slot[e])] &= ~(1 << int(room[e]))
        out = []
        for e in sorted(_events(k), reverse=descending):
            target = a + t - int(slot[e])
            f = self.poss[e] & ~free[target]
            if not f:
                return None
            r = _lowest(f)
            free[target] |= 1 << r
            out.append((e, target, r))
        return sorted(out)

    def lahc_kempe(self, slot, room, seed, steps, history, p_swap=0.5, p_kempe=0.0, max_chain=0, on_accept=None,
                   info=None):
        """(slot, room, rng state, gain, accepted, best_step, the five counts) of
        one row. on_accept(k, slot, room, cur) is called after every accepted
        step. info (a dict) receives scv0, the final current row and its cost,
        the kinds of accepted moves, and of the accepted Kempe steps: `chains`
        (their lengths), `two_sided` (chains with a student who attends an
        event on each side), `order_matters` (taking K in descending order
        would have changed the rooms or the verdict) and `left_room` (chains of
        two events in which each takes the room the other leaves)."""
        slot, room = np.array(slot, np.uint8), np.array(room, np.uint8)
        E, L = self.E, int(history)
        zeros = (0, 0, 0, 0, 0)
        if not self.valid(slot, room) or self.hcv_of(slot, room) != 0:
            return slot, room, int(seed), 0, 0, 0, zeros
        rng = ParkMiller(seed)
        sets = self.slot_sets(slot)
        occ = [0] * SLOTS
        for e in range(E):
            occ[int(slot[e])] |= 1 << int(room[e])
        scv0 = row_scv = self.scv_of(slot)
        cur = best = scv0
        hist = [scv0] * L
        best_rows = (slot.copy(), room.copy())
        accepted = best_step = 0
        kempe_from = 1.0 - p_kempe
        stats = dict.fromkeys(STAT_NAMES, 0)
        kinds = {"move1": 0, "move2": 0, "kempe": 0, "chains": [], "two_sided": 0, "order_matters": 0, "left_room": 0}
        for k in range(steps):
            v = k % L
            e1 = int(rng.next() * E)
            u = rng.next()
            x = rng.next()
            cand, kind, kbits = None, None, 0
            a = int(slot[e1])
            if p_kempe > 0 and u >= kempe_from:
                kind = "kempe"
                stats["tried"] += 1
                t = int(x * (SLOTS - 1))
                if t >= a:
                    t += 1
                kbits = self.component(sets[a] | sets[t], e1)
                if max_chain > 0 and bin(kbits).count("1") > max_chain:
                    stats["capped"] += 1
                else:
                    cand = self.chain_rooms(slot, room, occ, kbits, a, t)
                    if cand is None:
                        stats["no_room"] += 1
            elif E >= 2 and u < p_swap:
                kind = "move2"
                e2 = int(x * (E - 1))
                if e2 >= e1:
                    e2 += 1
                b = int(slot[e2])
                if a != b and not (self.corr[e1] & sets[b] & ~(1 << e2)) and not (self.corr[e2] & sets[a] & ~(1 << e1)):
                    f1 = self.poss[e1] & ~(occ[b] & ~(1 << int(room[e2])))
                    f2 = self.poss[e2] & ~(occ[a] & ~(1 << int(room[e1])))
                    if f1 and f2:
                        cand = [(e1, b, _lowest(f1)), (e2, a, _lowest(f2))]
            else:
                kind = "move1"
                t = int(x * (SLOTS - 1))
                if t >= a:
                    t += 1
                if not (self.corr[e1] & sets[t]):
                    f = self.poss[e1] & ~occ[t]
                    if f:
                        cand = [(e1, t, _lowest(f))]
            if cand is not None:
                new_slot = slot.copy()
                for e, s, _ in cand:
                    new_slot[e] = s
                new_scv = self.scv_of(new_slot)
                c = cur + (new_scv - row_scv)
                if c <= cur or c <= hist[v]:
                    kinds[kind] += 1
                    if kind == "kempe":
                        stats["accepted"] += 1
                        stats["chain_events"] += len(cand)
                        kinds["chains"].append(len(cand))
                        in_a = in_t = 0                              # students of K's events on either side
                        for e, s, _ in cand:
                            if s == t:
                                in_a |= self.students[e]
                            else:
                                in_t |= self.students[e]
                        kinds["two_sided"] += bool(in_a & in_t)
                        kinds["order_matters"] += self.chain_rooms(slot, room, occ, kbits, a, t, descending=True) != cand
                        kinds["left_room"] += (len(cand) == 2 and cand[0][2] == int(room[cand[1][0]])
                                               and cand[1][2] == int(room[cand[0][0]]))
                    for e, _, _ in cand:
                        sets[int(slot[e])] &= ~(1 << e)
                        occ[int(slot[e])] &= ~(1 << int(room[e]))
                    for e, s, r in cand:
                        sets[s] |= 1 << e
                        occ[s] |= 1 << r
                        slot[e], room[e] = s, r
                    cur, row_scv = c, new_scv
                    accepted += 1
                    if cur < best:
                        best, best_step = cur, k + 1
                        best_rows = (slot.copy(), room.copy())
                    if on_accept is not None:
                        on_accept(k, slot, room, cur)
            hist[v] = cur
        if info is not None:
            info.update(scv0=scv0, cur=cur, cur_slot=slot.copy(), cur_room=room.copy(), **kinds)
        return (best_rows[0], best_rows[1], rng.seed, scv0 - best, accepted, best_step,
                tuple(stats[n] for n in STAT_NAMES))

    @property
    def students(self):
        """students[e]: the students of event e as a bitset."""
        if not hasattr(self, "_students"):
            A = self.inst.student_events
            self._students = [lm._bits(A[:, e]) for e in range(self.E)]
        return self._students

    def lahc_kempe_rows(self, slot, room, seeds, steps, history, p_swap=0.5, p_kempe=0.0, max_chain=0, infos=None):
        """The whole population: (slot, room, rng, gain, accepted, best_step,
        stats [P, 5]) as arrays."""
        out = []
        for i in range(len(slot)):
            info = {} if infos is not None else None
            out.append(self.lahc_kempe(slot[i], room[i], int(seeds[i]), steps, history, p_swap, p_kempe, max_chain,
                                       info=info))
            if infos is not None:
                infos.append(info)
        return (np.stack([o[0] for o in out]), np.stack([o[1] for o in out]), np.array([o[2] for o in out], np.int64),
                np.array([o[3] for o in out], np.int32), np.array([o[4] for o in out], np.int32),
                np.array([o[5] for o in out], np.int32), np.array([o[6] for o in out], np.int32).reshape(len(out), 5))
