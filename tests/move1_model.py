"""Numpy / Python-int statement of tt_move1_scan and tt_move1_descent
(include/ttga/move1.h), written from the header: to_room from the correlation
and possible-room matrices, d_scv from the attendance of the
students of each event -- for every (student, event) pair the nine bits of
each day with the event's slot cleared, then what setting the target slot adds
to its day, all 45 targets at once -- and the last-slot term from studentNumber. The descent is rounds of
"scan, apply the summary's move".

`defect` plants what tests/test_move1_cpu.py shows the GPU comparison can see."""
import numpy as np

import lahc_model as lm
from lahc_model import DAY_LUT, DAYS, PER_DAY, SLOTS

CLASH, NO_ROOM, UNSCANNED, NONE = 255, 254, 253, 0x7FFFFFFF
UNSCANNED_SUMMARY = (0, 0, 0, 0, -1, -1)
DEFECTS = ("tie_larger_event", "highest_room", "clash_as_no_room")

_T = np.arange(SLOTS)
_LAST = (_T % PER_DAY == PER_DAY - 1).astype(np.int64)


class Model(lm.Model):
    def __init__(self, inst):
        super().__init__(inst)
        A = inst.student_events.astype(np.float32)                                    # counts <= S: exact
        self.corr_m = ((A.T @ A) > 0).astype(np.float32)                              # the diagonal included
        self.poss_m = inst.possible_rooms().astype(bool)                              # [E, R]
        # the (student, event) pairs event by event: their order, the events that have any, where each begins
        self.pair_order = np.argsort(self.ev_of, kind="stable")
        self.pair_events, self.pair_starts = np.unique(self.ev_of[self.pair_order], return_index=True)

    def scanned(self, slot, room):
        """The header's steps 1 and 2: the row is valid and has hcv 0."""
        return self.valid(slot, room) and self.hcv_of(slot, room) == 0

    def d_scv(self, slot):
        """int64 [E, 45]: scv(the row with slot[e] = t) - scv(the row), from the
        attendance bits alone; the row is feasible, so a student's bit of
        slot[e] belongs to e and to no other event."""
        slot = np.asarray(slot, np.int64)
        att = np.zeros((self.S, SLOTS), bool)
        att[self.stu_of, slot[self.ev_of]] = True
        days = att.reshape(self.S, DAYS, PER_DAY) @ (1 << np.arange(PER_DAY))        # [S, 5] nine-bit words
        s, e = self.stu_of, self.ev_of                                                # the (student, event) pairs
        a = slot[e]
        rows = days[s]                                                                # [n, 5]
        left = rows.copy()
        left[np.arange(len(s)), a // PER_DAY] &= ~(1 << (a % PER_DAY))                # the student leaves slot a
        day_t = left[:, _T // PER_DAY]                                                # [n, 45]: the day of slot t, before
        into = DAY_LUT[day_t | (1 << (_T % PER_DAY))] - DAY_LUT[day_t]                # ... and what attending t adds to it
        delta = into + (DAY_LUT[left].sum(axis=1) - DAY_LUT[rows].sum(axis=1))[:, None]
        d = np.zeros((self.E, SLOTS), np.int64)
        if len(s):
            d[self.pair_events] = np.add.reduceat(delta[self.pair_order], self.pair_starts, axis=0)
        return d + self.sn[:, None] * (_LAST[None, :] - _LAST[slot][:, None])

    def to_room(self, slot, room, defect=None):
        """int64 [E, 45]: the header's step 4, from the correlation and
        possible-room matrices."""
        slot, room = np.asarray(slot, np.int64), np.asarray(room, np.int64)
        there = np.zeros((self.E, SLOTS), np.float32)
        there[np.arange(self.E), slot] = 1
        clash = (self.corr_m @ there) > 0                                             # [E, 45]: a correlated event in t
        occ = np.zeros((SLOTS, self.R), bool)
        occ[slot, room] = True
        free = self.poss_m[:, None, :] & ~occ[None, :, :]                             # [E, 45, R]
        lowest = free.argmax(axis=2)
        if defect == "highest_room":
            lowest = self.R - 1 - free[:, :, ::-1].argmax(axis=2)
        out = np.where(free.any(axis=2), lowest, NO_ROOM)
        out = np.where(clash, NO_ROOM if defect == "clash_as_no_room" else CLASH, out)
        out[np.arange(self.E), slot] = room
        return out

    def summary(self, slot, d, tr, defect=None):
        """The header's step 5 from the two tables of a scanned row."""
        feas = (tr < 64) & (_T[None, :] != np.asarray(slot, np.int64)[:, None])
        if not feas.any():
            return (1, 0, 0, 0, -1, -1)
        least = int(d[feas].min())
        ee, tt = np.nonzero(feas & (d == least))                                      # event-major: least e, then least t
        k = 0 if defect != "tie_larger_event" else int(np.flatnonzero(ee == ee.max())[0])
        return (1, int(feas.sum()), int((feas & (d < 0)).sum()), least, int(ee[k]), int(tt[k]))

    def scan(self, slot, room, defect=None, gate=True):
        """(summary int32 [6], d_scv int32 [E, 45], to_room uint8 [E, 45]) of one row."""
        if gate and not self.scanned(slot, room):
            return (np.array(UNSCANNED_SUMMARY, np.int32), np.full((self.E, SLOTS), NONE, np.int32),
                    np.full((self.E, SLOTS), UNSCANNED, np.uint8))
        d, tr = self.d_scv(slot), self.to_room(slot, room, defect)
        return np.array(self.summary(slot, d, tr, defect), np.int32), d.astype(np.int32), tr.astype(np.uint8)

    def scan_rows(self, slot, room):
        out = [self.scan(slot[i], room[i]) for i in range(len(slot))]
        return tuple(np.stack([o[k] for o in out]) if out else np.zeros((0,), np.int32) for k in range(3))

    def descent(self, slot, room, max_passes, ties=None):
        """(slot, room, gain, passes) of one row. ties (a list): receives, per
        applied pass, how many feasible moves shared the least delta."""
        slot, room = np.array(slot, np.uint8), np.array(room, np.uint8)
        gain = passes = 0
        if not self.scanned(slot, room):
            return slot, room, 0, 0
        while passes < max_passes:
            d, tr = self.d_scv(slot), self.to_room(slot, room)
            sm = self.summary(slot, d, tr)
            if sm[1] == 0 or sm[3] >= 0:
                break
            if ties is not None:
                feas = (tr < 64) & (_T[None, :] != slot.astype(np.int64)[:, None])
                ties.append(int((feas & (d == sm[3])).sum()))
            e, t = sm[4], sm[5]
            slot[e], room[e] = t, tr[e, t]
            gain -= sm[3]
            passes += 1
        return slot, room, gain, passes

    def descent_rows(self, slot, room, max_passes, ties=None):
        """(slot, room, gain int32 [P], passes int32 [P])."""
        out = [self.descent(slot[i], room[i], max_passes, ties) for i in range(len(slot))]
        return (np.stack([o[0] for o in out]), np.stack([o[1] for o in out]), np.array([o[2] for o in out], np.int32),
                np.array([o[3] for o in out], np.int32))


def credit(scv, penalty, gain):
    """tt_lahc's step 5 on int arrays: scv -= gain; a feasible row's penalty too."""
    scv, penalty, gain = np.asarray(scv, np.int64), np.asarray(penalty, np.int64), np.asarray(gain, np.int64)
    return ((scv - gain).astype(np.int32),
            np.where((penalty >= 0) & (penalty < 1000000), penalty - gain, penalty).astype(np.int32))


def population(inst, P, model=None):
    """lahc_model.population's rows (every fifth spoiled): (slot, room)."""
    slot, room, _ = lm.population(inst, P, model)
    return slot, room
