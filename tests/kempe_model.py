"""A numpy model of tt_kempe_move (include/ttga_kempe.h) for one row: the six
steps of the header with ttga.rng for the draws and a plain breadth-first
search on Instance.correlations() with the diagonal cleared. Rooms are not
modelled: the expected rooms of the two touched slots are the oracle's
assign_rooms of the new slot row restricted to those slots (assignRooms works
slot by slot), every other event keeps the room it had (expected_rooms)."""
import collections

import numpy as np

from ttga.rng import ParkMiller, step

SLOTS = 45


def neighbours(inst) -> np.ndarray:
    """eventCorrelations > 0 with the diagonal cleared, as a bool matrix."""
    nb = inst.correlations() > 0
    np.fill_diagonal(nb, False)
    return nb


def advanced(state: int, draws: int) -> int:
    s = int(state)
    for _ in range(draws):
        s = step(s)
    return s


def component(nb, members, e) -> np.ndarray:
    """The connected component of e in the graph nb restricted to `members`
    (a bool vector over the events), as a sorted index array."""
    seen = {int(e)}
    todo = collections.deque(seen)
    while todo:
        a = todo.popleft()
        for b in np.flatnonzero(nb[a] & members):
            if int(b) not in seen:
                seen.add(int(b))
                todo.append(int(b))
    return np.array(sorted(seen), np.int64)


def kempe_row(inst, nb, slot, state, prob, max_chain=0, room=None):
    """-> (new slot row, new rng state, chain_len, (t1, t2) or None)."""
    slot = np.asarray(slot, np.uint8)
    if slot.max() >= SLOTS or (room is not None and np.asarray(room).max() >= inst.R):
        return slot.copy(), int(state), 0, None                       # 1. validity
    g = ParkMiller(int(state))
    if not g.next() < prob:                                           # 2. gate
        return slot.copy(), g.seed, 0, None
    e = g.pick(inst.E)                                                # 3. choice
    t1 = int(slot[e])
    t2 = g.pick(SLOTS - 1)
    if t2 >= t1:
        t2 += 1
    K = component(nb, (slot == t1) | (slot == t2), e)                 # 4. chain
    if max_chain > 0 and len(K) > max_chain:                          # 5. cap
        return slot.copy(), g.seed, -len(K), (t1, t2)
    new = slot.copy()                                                 # 6. apply
    new[K] = (t1 + t2 - slot[K].astype(np.int64)).astype(np.uint8)
    return new, g.seed, len(K), (t1, t2)


def kempe_rows(inst, slot, states, prob, max_chain=0, room=None, nb=None):
    """kempe_row for every row -> (slot rows, states int64, chain_len int32, [(t1, t2) | None])."""
    nb = neighbours(inst) if nb is None else nb
    out = [kempe_row(inst, nb, slot[i], states[i], prob, max_chain, None if room is None else room[i])
           for i in range(len(slot))]
    return (np.stack([o[0] for o in out]), np.array([o[1] for o in out], np.int64),
            np.array([o[2] for o in out], np.int32), [o[3] for o in out])


def expected_rooms(orc_problem, new_slot, old_room, chain_len, pairs) -> np.ndarray:
    """The rooms after the move: for an applied row the oracle's assign_rooms of
    the new slot row on the events now in t1 or t2, the old room elsewhere."""
    want = np.array(old_room, np.uint8, copy=True)
    rows = [i for i in range(len(new_slot)) if chain_len[i] > 0]
    if rows:
        full = orc_problem.assign_rooms(new_slot[rows])
        for k, i in enumerate(rows):
            t1, t2 = pairs[i]
            touched = (new_slot[i] == t1) | (new_slot[i] == t2)
            want[i, touched] = full[k, touched]
    return want
