"""Pure-Python statement of tt_lahc (include/ttga_lahc.h), written from the
header: the feasibility of a candidate from the definitions on Python-int
bitsets, the change of scv by recomputing the scv of the whole candidate row
(scv_of: Solution::computeScv from the row alone, no running state), the
draws from ttga.rng.ParkMiller.

feasible_rows() is a CPU constructor of rows that are feasible at entry."""
import numpy as np

from ttga.rng import ParkMiller

SLOTS, PER_DAY, DAYS = 45, 9, 5

_i = np.arange(1 << PER_DAY)
# windows of three classes in a row + [exactly one class] of one day's nine bits
DAY_LUT = (np.array([bin(v & (v >> 1) & (v >> 2)).count("1") for v in _i])
           + np.array([bin(v).count("1") == 1 for v in _i])).astype(np.int64)


def _bits(row):
    """A 0/1 vector as a Python int, bit j = row[j]."""
    return int.from_bytes(np.packbits(np.asarray(row) != 0, bitorder="little").tobytes(), "little")


class Model:
    def __init__(self, inst):
        self.inst, self.E, self.R, self.S = inst, inst.E, inst.R, inst.S
        A = inst.student_events.astype(np.int64)
        self.sn = A.sum(axis=0)
        Af = A.astype(np.float32)                                     # counts <= S: exact
        corr = (Af.T @ Af) > 0
        poss = inst.possible_rooms()
        self.corr = [_bits(corr[e]) for e in range(self.E)]           # bit f: e and f share a student
        self.poss = [_bits(poss[e]) for e in range(self.E)]           # bit r: room r is possible for e
        stu, ev = np.nonzero(A)                                       # student-major
        self.stu_of, self.ev_of = stu, ev

    # -- the cost of a row, from the row alone
    def scv_of(self, slot):
        slot = np.asarray(slot, np.int64)
        last = int(self.sn[slot % PER_DAY == PER_DAY - 1].sum())
        att = np.zeros((self.S, SLOTS), bool)
        att[self.stu_of, slot[self.ev_of]] = True
        idx = att.reshape(self.S, DAYS, PER_DAY) @ (1 << np.arange(PER_DAY))
        return last + int(DAY_LUT[idx].sum())

    def hcv_of(self, slot, room):
        """Room pairs + correlated pairs + unsuitable rooms, as tt_eval defines them."""
        slot, room = np.asarray(slot, np.int64), np.asarray(room, np.int64)
        cells = np.bincount(slot * self.R + room, minlength=SLOTS * self.R)
        h = int((cells * (cells - 1) // 2).sum())
        sets = self.slot_sets(slot)
        h += sum(bin(self.corr[e] & sets[slot[e]] & ~(1 << e)).count("1") for e in range(self.E)) // 2
        return h + sum(1 for e in range(self.E) if not (self.poss[e] >> int(room[e])) & 1)

    def slot_sets(self, slot):
        sets = [0] * SLOTS
        for e, t in enumerate(slot):
            sets[int(t)] |= 1 << e
        return sets

    def valid(self, slot, room):
        return int(np.max(slot, initial=0)) < SLOTS and int(np.max(room, initial=0)) < self.R

    # -- one individual
    def lahc(self, slot, room, seed, steps, history, p_swap=0.5, on_accept=None, info=None):
        """(slot, room, rng state, gain, accepted, best_step) of one row.
        on_accept(k, slot, room, cur) is called after every accepted step;
        info (a dict) receives scv0, the final current row and its cost, and
        the kinds of accepted moves."""
        slot, room = np.array(slot, np.uint8), np.array(room, np.uint8)
        E, L = self.E, int(history)
        untouched = (slot, room, int(seed), 0, 0, 0)
        if not self.valid(slot, room) or self.hcv_of(slot, room) != 0:
            return untouched
        rng = ParkMiller(seed)
        sets = self.slot_sets(slot)
        occ = [0] * SLOTS
        for e in range(E):
            occ[int(slot[e])] |= 1 << int(room[e])
        scv0 = row_scv = self.scv_of(slot)                           # row_scv: scv_of(the current row)
        cur = best = scv0
        hist = [scv0] * L
        best_rows = (slot.copy(), room.copy())
        accepted = best_step = 0
        kinds = {"move1": 0, "move2": 0, "both": 0, "own_room": 0}
        for k in range(steps):
            v = k % L
            e1 = int(rng.next() * E)
            u = rng.next()
            x = rng.next()
            cand = None
            a = int(slot[e1])
            if E >= 2 and u < p_swap:
                e2 = int(x * (E - 1))
                if e2 >= e1:
                    e2 += 1
                b = int(slot[e2])
                if a != b and not (self.corr[e1] & sets[b] & ~(1 << e2)) and not (self.corr[e2] & sets[a] & ~(1 << e1)):
                    f1 = self.poss[e1] & ~(occ[b] & ~(1 << int(room[e2])))
                    f2 = self.poss[e2] & ~(occ[a] & ~(1 << int(room[e1])))
                    if f1 and f2:
                        r1, r2 = (f1 & -f1).bit_length() - 1, (f2 & -f2).bit_length() - 1
                        cand = [(e1, b, r1), (e2, a, r2)]
            else:
                t = int(x * (SLOTS - 1))
                if t >= a:
                    t += 1
                if not (self.corr[e1] & sets[t]):
                    f = self.poss[e1] & ~occ[t]
                    if f:
                        cand = [(e1, t, (f & -f).bit_length() - 1)]
            if cand is not None:
                new_slot = slot.copy()
                for e, t, _ in cand:
                    new_slot[e] = t
                new_scv = self.scv_of(new_slot)
                c = cur + (new_scv - row_scv)
                if c <= cur or c <= hist[v]:
                    if len(cand) == 2:
                        kinds["move2"] += 1
                        kinds["both"] += bool((self.corr[cand[0][0]] >> cand[1][0]) & 1)
                        # e1's new room is the one e2 leaves, and no other room was there for it
                        kinds["own_room"] += (cand[0][2] == int(room[cand[1][0]])
                                              and not self.poss[cand[0][0]] & ~occ[cand[0][1]])
                    else:
                        kinds["move1"] += 1
                    for e, _, _ in cand:
                        sets[int(slot[e])] &= ~(1 << e)
                        occ[int(slot[e])] &= ~(1 << int(room[e]))
                    for e, t, r in cand:
                        sets[t] |= 1 << e
                        occ[t] |= 1 << r
                        slot[e], room[e] = t, r
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
        return best_rows[0], best_rows[1], rng.seed, scv0 - best, accepted, best_step

    def lahc_rows(self, slot, room, seeds, steps, history, p_swap=0.5, infos=None):
        """The whole population: (slot, room, rng, gain, accepted, best_step) as arrays."""
        out = []
        for i in range(len(slot)):
            info = {} if infos is not None else None
            out.append(self.lahc(slot[i], room[i], int(seeds[i]), steps, history, p_swap, info=info))
            if infos is not None:
                infos.append(info)
        return (np.stack([o[0] for o in out]), np.stack([o[1] for o in out]), np.array([o[2] for o in out], np.int64),
                np.array([o[3] for o in out], np.int32), np.array([o[4] for o in out], np.int32),
                np.array([o[5] for o in out], np.int32))


def feasible_rows(inst, P, seed, model=None):
    """(slot, room) uint8 [P, E]. Per row, the event with the fewest slots left
    goes next, ties in a seeded random order; it goes to a seeded random slot
    among those with no correlated event and a free possible room, and takes
    the lowest such room. (A plain seeded random order of the events, with the
    same slot and room rule, leaves 0 of 40 rows of med and 12 of 40 of sm
    feasible.) A row in which some event finds no slot is finished with random
    genes: that event then breaks a hard constraint wherever it lands, so the
    row stays infeasible."""
    m = model or Model(inst)
    E, R = inst.E, inst.R
    A = inst.student_events.astype(np.float32)
    corr = (A.T @ A) > 0
    np.fill_diagonal(corr, False)
    poss = inst.possible_rooms().astype(bool)                        # [E, R]
    slot = np.zeros((P, E), np.uint8)
    room = np.zeros((P, E), np.uint8)
    for i in range(P):
        g = np.random.default_rng([int(seed), i])
        tie = g.permutation(E)
        avail = np.repeat(poss.any(axis=1)[:, None], SLOTS, axis=1)  # [E, 45]: the slot is open to the event
        free = np.ones((SLOTS, R), bool)
        left = np.ones(E, bool)
        for _ in range(E):
            key = np.where(left, avail.sum(axis=1) * E + tie, SLOTS * E + E)
            e = int(np.argmin(key))
            ok = np.flatnonzero(avail[e])
            if ok.size == 0:
                rest = np.flatnonzero(left)
                slot[i, rest] = g.integers(0, SLOTS, size=rest.size)
                room[i, rest] = g.integers(0, R, size=rest.size)
                break
            t = int(ok[int(g.integers(0, ok.size))])
            r = int(np.flatnonzero(poss[e] & free[t])[0])
            slot[i, e], room[i, e] = t, r
            left[e] = False
            free[t, r] = False
            avail[:, t] &= ~corr[e] & (poss & free[t]).any(axis=1)
    return slot, room


# ---------------------------------------------------------------- the shapes of tests/test_gpu_lahc.py
def load_golden(name):
    """The instance of tests/golden/<name>.npz."""
    import pathlib

    import ttga
    z = np.load(pathlib.Path(__file__).resolve().parent / "golden" / f"{name}.npz")
    E, R, F, S = (int(x) for x in z["dims"])
    return ttga.Instance(E, R, F, S, z["room_size"], z["student_events"], z["room_features"], z["event_features"])


def _variant(inst, student_events=None, room_size=None, room_features=None, event_features=None):
    import ttga
    A = inst.student_events if student_events is None else student_events
    rf = inst.room_features if room_features is None else room_features
    ef = inst.event_features if event_features is None else event_features
    return ttga.Instance(inst.E, inst.R, rf.shape[1], A.shape[0], inst.room_size if room_size is None else room_size,
                         A, rf, ef)


def _tight_rooms():
    """tests/golden/tight.npz with every room made possible for every event (27
    of its events have no possible room: no row of it is feasible)."""
    inst = load_golden("tight")
    return _variant(inst, room_size=np.full(inst.R, int(inst.student_number().max()), np.int32),
                    room_features=np.ones_like(inst.room_features))


def _room63():
    """R 64; event 0 needs a feature that only room 63 has."""
    import ttga
    inst = ttga.generate(40, 64, 2, 30, seed=17)
    rf = np.concatenate([inst.room_features, np.zeros((64, 1), np.int32)], axis=1)
    ef = np.concatenate([inst.event_features, np.zeros((40, 1), np.int32)], axis=1)
    rf[63, 2], ef[0, 2] = 1, 1
    rf[63, :2] |= inst.event_features[0]
    size = inst.room_size.copy()
    size[63] = max(int(size[63]), int(inst.student_number()[0]))
    out = _variant(inst, room_size=size, room_features=rf, event_features=ef)
    assert out.possible_rooms()[0].tolist() == [0] * 63 + [1]
    return out


def _extremes():
    """Two added students: one attends nothing, one attends 45 of the 60 events,
    which a feasible row spreads over all 45 slots (a full mask)."""
    import ttga
    inst = ttga.generate(60, 5, 3, 30, seed=5)
    A = np.concatenate([inst.student_events, np.zeros((2, 60), np.int32)], axis=0)
    A[31, :45] = 1
    size = np.maximum(inst.room_size, int(A.sum(axis=0).max()))
    return _variant(inst, student_events=A, room_size=size)


def _gen(*a, **k):
    import ttga
    return lambda: ttga.generate(*a, **k)


def _cfg(name):
    import ttga
    return lambda: ttga.config_instance(name)


SHAPES = {
    "sm": _cfg("sm"), "med": _cfg("med"),
    "tight": lambda: load_golden("tight"),              # no feasible row exists: the gate only
    "tight_rooms": _tight_rooms,
    "E1": _gen(1, 2, 2, 5, seed=3, min_att=1, max_att=1),
    "E2": _gen(2, 2, 2, 6, seed=4, min_att=1, max_att=1),
    "E3": _gen(3, 2, 2, 8, seed=5, min_att=1, max_att=2),
    "E63": _gen(63, 5, 3, 40, seed=14), "E64": _gen(64, 5, 3, 40, seed=13), "E65": _gen(65, 5, 3, 40, seed=15),
    "R1": _gen(30, 1, 2, 20, seed=16),
    "R64": _room63,
    "S0": _gen(30, 3, 2, 0, seed=18),
    "extremes": _extremes,
    "syn": _cfg("syn"),                                 # 2000 events, 45 x 40 cells: the gate only
    # syn's E and S (the same LDS image) with 64 rooms and 2 to 6 events per student
    "syn_sparse": _gen(2000, 64, 10, 5000, seed=19, min_att=2, max_att=6),
}
NO_FEASIBLE_ROW = ("tight", "syn")

# id: (shape, P, steps, history, p_swap)
CASES = {
    "sm-L50": ("sm", 67, 2000, 50, 0.5), "sm-L500": ("sm", 67, 2000, 500, 0.5),
    "med-L50": ("med", 67, 2000, 50, 0.5), "med-L500": ("med", 67, 2000, 500, 0.5),
    "tight-L50": ("tight", 67, 2000, 50, 0.5), "tight-L500": ("tight", 67, 2000, 500, 0.5),
    "tight_rooms-L50": ("tight_rooms", 67, 2000, 50, 0.5), "tight_rooms-L500": ("tight_rooms", 67, 2000, 500, 0.5),
    "E1": ("E1", 67, 2000, 50, 1.0), "E2": ("E2", 67, 2000, 50, 0.5), "E3": ("E3", 67, 2000, 50, 0.5),
    "E63": ("E63", 67, 2000, 50, 0.5), "E64": ("E64", 67, 2000, 50, 0.5), "E65": ("E65", 67, 2000, 50, 0.5),
    "R1": ("R1", 67, 2000, 50, 0.5), "R64": ("R64", 67, 2000, 50, 0.5), "S0": ("S0", 67, 2000, 50, 0.5),
    "extremes": ("extremes", 67, 2000, 50, 0.5),
    "p_swap0": ("sm", 67, 2000, 50, 0.0), "p_swap1": ("sm", 67, 2000, 50, 1.0),
    "L1": ("sm", 67, 2000, 1, 0.5), "L3000": ("sm", 67, 2000, 3000, 0.5),
    "steps0": ("sm", 67, 0, 50, 0.5), "steps1": ("sm", 67, 1, 50, 0.5),
    "P1": ("sm", 1, 2000, 50, 0.5), "P65": ("sm", 65, 2000, 50, 0.5),
    "syn": ("syn", 4, 300, 100, 0.5), "syn_sparse": ("syn_sparse", 4, 300, 100, 0.5),
}
ROW_SEED, RNG_SEED = 7, 90001


def population(inst, P, model=None):
    """The rows of a case: feasible_rows with every fifth row (2, 7, ...) spoiled
    by putting event 1 into event 0's slot and room, and one in-range rng state
    per row. (slot, room, seeds)."""
    slot, room = feasible_rows(inst, P, ROW_SEED, model)
    if inst.E >= 2:
        slot[2::5, 1], room[2::5, 1] = slot[2::5, 0], room[2::5, 0]
    return slot, room, (np.arange(P, dtype=np.int64) * 7919 + RNG_SEED)
