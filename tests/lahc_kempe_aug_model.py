"""Pure-Python statement of tt_lahc_kempe_aug (include/ttga_lahc_kempe_aug.h),
written from the header on top of tests/lahc_kempe_model.py: the walk is that
model's, the rooms of a chain come from chain_rooms below (the direct rule,
then a breadth-first search for an augmenting path over the target slot's
holders), and a candidate carries the displaced bystanders next to the chain's
events."""
import numpy as np

import lahc_kempe_model as km
from lahc_kempe_model import _events, _lowest
from lahc_model import SLOTS
from ttga.rng import ParkMiller

STAT_NAMES = km.STAT_NAMES + ("rescued", "displaced")


class Model(km.Model):
    def chain_rooms(self, slot, room, occ, k, a, t, room_rule=1, descending=False):
        """The header's room rule for chain k between slots a and t. Returns
        None (no room) or (chain, displaced, paths): chain = [(e, target,
        room)] in ascending event number, displaced = [(h, slot, room)] for the
        bystanders whose room changed, paths = [(holders moved, whether one of
        them was an event of k, the rooms on the path)] per search that
        succeeded. room_rule 0 and `descending` are lahc_kempe_model's."""
        if room_rule == 0 or descending:
            direct = km.Model.chain_rooms(self, slot, room, occ, k, a, t, descending)
            return None if direct is None else (direct, [], [])
        chain = _events(k)
        hold = {a: {}, t: {}}
        for e in range(self.E):
            if int(slot[e]) in hold and not (k >> e) & 1:
                hold[int(slot[e])][int(room[e])] = e
        paths = []
        for e in chain:
            tab = hold[a + t - int(slot[e])]
            held = sum(1 << r for r in tab)
            free = self.poss[e] & ~held
            if free:                                                 # step 1
                tab[_lowest(free)] = e
                continue
            seen = self.poss[e]                                      # step 2
            queue = _events(seen)
            parent = dict.fromkeys(queue)                            # None: e itself
            last = None
            while queue and last is None:
                r = queue.pop(0)
                new = self.poss[tab[r]] & ~seen
                if new & ~held:
                    last = _lowest(new & ~held)
                    parent[last] = r
                else:
                    for q in _events(new):
                        parent[q] = r
                        queue.append(q)
                    seen |= new
            if last is None:
                return None
            rooms, moved_k, q = [last], False, last
            while parent[q] is not None:
                tab[q] = tab[parent[q]]
                moved_k |= bool((k >> tab[q]) & 1)
                q = parent[q]
                rooms.append(q)
            tab[q] = e
            paths.append((len(rooms) - 1, moved_k, rooms))
        out, displaced = [], []
        for s in (a, t):
            for r, e in hold[s].items():
                if (k >> e) & 1:
                    out.append((e, s, r))
                elif int(room[e]) != r:
                    displaced.append((e, s, r))
        return sorted(out), sorted(displaced), paths

    def lahc_kempe_aug(self, slot, room, seed, steps, history, p_swap=0.5, p_kempe=0.0, max_chain=0, room_rule=1,
                       on_accept=None, on_kempe=None, info=None):
        """(slot, room, rng state, gain, accepted, best_step, the seven counts)
        of one row. on_accept(k, slot, room, cur) is called after every accepted
        step, on_kempe(slot, room, kbits, a, t, result) for every Kempe
        candidate that reaches the room rule, before it is judged. info (a
        dict) receives scv0, the kinds of accepted moves and, of the accepted
        chains, `chains` (their lengths), `longest_path` (the most holders one
        path moved), `moved_chain_event` (chains in which a path displaced an
        event of K placed earlier) and `high_room` (the highest room on a
        path)."""
        slot, room = np.array(slot, np.uint8), np.array(room, np.uint8)
        E, L = self.E, int(history)
        zeros = (0,) * 7
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
        kinds = {"move1": 0, "move2": 0, "kempe": 0, "chains": [], "longest_path": 0, "moved_chain_event": 0,
                 "high_room": -1}
        for k in range(steps):
            v = k % L
            e1 = int(rng.next() * E)
            u = rng.next()
            x = rng.next()
            cand, kind, displaced, paths = None, None, [], []
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
                    res = self.chain_rooms(slot, room, occ, kbits, a, t, room_rule)
                    if on_kempe is not None:
                        on_kempe(slot, room, kbits, a, t, res)
                    if res is None:
                        stats["no_room"] += 1
                    else:
                        cand, displaced, paths = res
                        stats["rescued"] += bool(paths)
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
                        stats["displaced"] += len(displaced)
                        kinds["chains"].append(len(cand))
                        kinds["longest_path"] = max([kinds["longest_path"]] + [p[0] for p in paths])
                        kinds["moved_chain_event"] += any(p[1] for p in paths)
                        kinds["high_room"] = max([kinds["high_room"]] + [r for p in paths for r in p[2]])
                    moves = cand + displaced
                    for e, _, _ in moves:
                        sets[int(slot[e])] &= ~(1 << e)
                        occ[int(slot[e])] &= ~(1 << int(room[e]))
                    for e, s, r in moves:
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
            info.update(scv0=scv0, cur=cur, **kinds)
        return (best_rows[0], best_rows[1], rng.seed, scv0 - best, accepted, best_step,
                tuple(stats[n] for n in STAT_NAMES))

    def lahc_kempe_aug_rows(self, slot, room, seeds, steps, history, p_swap=0.5, p_kempe=0.0, max_chain=0, room_rule=1,
                            infos=None):
        """The whole population: (slot, room, rng, gain, accepted, best_step,
        stats [P, 7]) as arrays."""
        out = []
        for i in range(len(slot)):
            info = {} if infos is not None else None
            out.append(self.lahc_kempe_aug(slot[i], room[i], int(seeds[i]), steps, history, p_swap, p_kempe, max_chain,
                                           room_rule, info=info))
            if infos is not None:
                infos.append(info)
        return (np.stack([o[0] for o in out]), np.stack([o[1] for o in out]), np.array([o[2] for o in out], np.int64),
                np.array([o[3] for o in out], np.int32), np.array([o[4] for o in out], np.int32),
                np.array([o[5] for o in out], np.int32), np.array([o[6] for o in out], np.int32).reshape(len(out), 7))
