"""CPU model of the greedy constructive initial population (include/ttga_greedy.h),
written from the header's text and independent of the kernels: the event order,
the slot rows with their Random draws, and a replay checker that needs no RNG.
Rooms are not its business (the oracle's assign_rooms gives them)."""
import numpy as np

from ttga.rng import ParkMiller, step

NUM_SLOTS = 45


def _neighbours(inst):
    """eventCorrelations without the diagonal, as a bool [E, E] matrix."""
    c = inst.correlations().astype(bool)
    np.fill_diagonal(c, False)
    return c


def greedy_keys(inst) -> np.ndarray:
    """key[e] = 128 * deg(e) + (64 - |possibleRooms(e)|)."""
    deg = _neighbours(inst).sum(axis=1).astype(np.int64)
    return 128 * deg + (64 - inst.possible_rooms().astype(bool).sum(axis=1).astype(np.int64))


def greedy_order(inst) -> np.ndarray:
    """The events by key descending, ties by event index ascending (int32 [E])."""
    key = greedy_keys(inst)
    return np.lexsort((np.arange(inst.E), -key)).astype(np.int32)


def greedy_slots(inst, order, seeds):
    """The slot rows [P, E] (uint8) of the individuals with Random(seeds[i]) and
    their final states (int64 [P]): exactly one draw per event."""
    E, R = inst.E, inst.R
    nb = _neighbours(inst)
    P = len(seeds)
    rngs = [ParkMiller(int(s)) for s in seeds]
    slot = np.full((P, E), 255, np.uint8)
    # conf[i, e, t]: the events placed in slot t of individual i that are correlated with e
    conf = np.zeros((P, E, NUM_SLOTS), np.int32)
    count = np.zeros((P, NUM_SLOTS), np.int32)
    rows = np.arange(P)
    for e in order:
        e = int(e)
        cost = conf[:, e, :] + (count >= R)
        tie = cost == cost.min(axis=1, keepdims=True)
        n = tie.sum(axis=1)
        k = np.array([g.pick(int(m)) for g, m in zip(rngs, n)])
        t = np.argmax(tie & (np.cumsum(tie, axis=1) == (k + 1)[:, None]), axis=1)      # T[k], T ascending
        slot[:, e] = t
        count[rows, t] += 1
        conf[rows, :, t] += nb[e].astype(np.int32)[None, :]
    return slot, np.array([g.seed for g in rngs], np.int64)


def advanced(seed: int, draws: int) -> int:
    """The Random state after `draws` draws from `seed`."""
    s = int(seed)
    for _ in range(draws):
        s = step(s)
    return s


def replay_check(inst, order, row) -> None:
    """Asserts that `row` (one finished slot row) can come from placing the
    events in `order`: every event's slot had minimum cost among the 45 at the
    moment it was placed. No RNG."""
    E, R = inst.E, inst.R
    nb = _neighbours(inst)
    assert sorted(int(e) for e in order) == list(range(E)), "order is not a permutation"
    placed = np.zeros((NUM_SLOTS, E), bool)
    count = np.zeros(NUM_SLOTS, np.int64)
    for e in order:
        e = int(e)
        t = int(row[e])
        assert 0 <= t < NUM_SLOTS, (e, t)
        cost = (placed & nb[e][None, :]).sum(axis=1) + (count >= R)
        assert cost[t] == cost.min(), f"event {e} in slot {t} at cost {cost[t]}, minimum {cost.min()}"
        placed[t, e] = True
        count[t] += 1
