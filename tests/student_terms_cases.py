"""Populations that put chosen students on the edges of eval_tile5's per-student
scv terms (the lane phase's word form), shared by the CPU and the GPU test
of it, and a plain restatement of those terms (Solution.cpp:99-137) to say
what each crafted row must give.

A student's terms depend only on the set of slots it attends: per day, the
windows of three consecutive slots all attended (the window stays inside the
day) plus one if exactly one slot of the day is attended. A pattern below maps
the student's k events onto a fixed slot list (event j to list[j % len]), so
with k >= len the attended set is the list, whatever else the row holds.
"""
import numpy as np

import ttga

DAYS, PER_DAY = 5, 9

# name -> (slot list, terms of a student that attends exactly these slots)
PATTERNS = {
    # every slot of day 2 (18..26: the field that ends at the day-3 straddle): 7 triples,
    # and no event on the four other days
    "full_day": (list(range(18, 27)), 7),
    # a run across a day boundary: 7, 8 | 9, 10 -- no window may cross, two slots per day
    "across_days": ([7, 8, 9, 10], 0),
    # the straddling day and the 32-bit word boundary: 26 alone in day 2 (single class),
    # 27, 28 and 31, 32, 33 in day 3 (one triple, bits 31 | 32 | 33)
    "straddle": ([26, 27, 28, 31, 32, 33], 2),
    # the last slot alone: single class of day 4
    "slot_44": ([44], 1),
    # the last three slots: one triple, the window ending at bit 44
    "last_three": ([42, 43, 44], 1),
    # exactly one event on each day, at a day's first and last slots and at bit 32
    "one_per_day": ([0, 17, 22, 32, 44], 5),
    # every event of the student in one slot (two and more events in the same slot)
    "same_slot": ([13], 1),
}


def student_terms(slots_of_student):
    """>2 in a row + single class of one student, from the slots of its events."""
    att = np.zeros(DAYS * PER_DAY, dtype=bool)
    att[np.asarray(slots_of_student, dtype=np.int64)] = True
    total = 0
    for d in range(DAYS):
        day = att[PER_DAY * d:PER_DAY * (d + 1)]
        total += int(np.sum(day[:-2] & day[1:-1] & day[2:])) + int(day.sum() == 1)
    return total


def scv_model(inst, slots):
    """scv of every row: the students' terms plus the last-slot-of-day term (Solution.cpp:93-96)."""
    sn = inst.student_number().astype(np.int64)
    events = [np.flatnonzero(inst.student_events[s]) for s in range(inst.S)]
    out = np.zeros(len(slots), dtype=np.int64)
    for p, row in enumerate(slots):
        out[p] = int(sn[row % PER_DAY == PER_DAY - 1].sum()) + sum(student_terms(row[ev]) for ev in events)
    return out.astype(np.int32)


def pick_students(inst, big_min=9):
    """(big, odd): the student with the most events (>= big_min, so that every pattern's
    list is covered), and one with an odd number >= 5 of events, none shared with big's --
    its id list ends in the sentinel column."""
    k = inst.student_events.sum(axis=1)
    big = int(np.argmax(k))
    assert k[big] >= big_min
    for s in np.argsort(k, kind="stable"):
        if k[s] >= 5 and k[s] % 2 == 1 and not np.any(inst.student_events[s] & inst.student_events[big]):
            return big, int(s)
    raise AssertionError("no odd-sized student disjoint from the largest")


def craft(inst, P, seed, rows):
    """Random slots [P, E] with one pattern per entry of `rows` ((pattern name, row) pairs)
    applied to the big student and, rotated by one pattern, to the odd one. Returns slots
    and the list of (row, student, pattern name, intended terms)."""
    slots, _ = ttga.random_slots(ttga.population_seeds(seed, P), inst.E)
    big, odd = pick_students(inst)
    names = list(PATTERNS)
    intended = []
    for name, row in rows:
        for student, pat in ((big, name), (odd, names[(names.index(name) + 1) % len(names)])):
            lst, want = PATTERNS[pat]
            ev = np.flatnonzero(inst.student_events[student])
            slots[row, ev] = [lst[j % len(lst)] for j in range(len(ev))]
            if len(ev) < len(lst):                    # the odd student covers a prefix of the list
                want = student_terms(lst[:len(ev)])
            intended.append((row, student, pat, want))
    return slots, intended


def spread_rows(P):
    """(pattern, row) pairs: the first tile's first and last lanes and both sides of its
    32-lane half, the population's last row (the short last tile), and with more than two
    tiles the same lanes of the second tile and the last tile's first row."""
    at = [0, 31, 32, 63, P - 1, 62, 17]
    if P > 128:
        at += [64, 95, 96, 127, 128, 126, 81]
    assert len(set(at)) == len(at) and max(at) < P
    return list(zip(list(PATTERNS) * 2, at))


def golden_instance(golden_dir, name):
    z = np.load(golden_dir / f"{name}.npz")
    E, R, F, S = (int(x) for x in z["dims"])
    return ttga.Instance(E, R, F, S, z["room_size"], z["student_events"], z["room_features"], z["event_features"])


def with_long_student(inst, n_events=40):
    """inst with student 0 attending n_events events (more than the 32 ids of the unrolled
    lane-phase runs: the plain loop serves it), spread over the event range."""
    se = inst.student_events.copy()
    se[0] = 0
    se[0, np.linspace(0, inst.E - 1, n_events).astype(np.int64)] = 1
    assert se[0].sum() == n_events
    return ttga.Instance(inst.E, inst.R, inst.F, inst.S, inst.room_size, se, inst.room_features, inst.event_features)
