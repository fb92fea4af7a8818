"""A plain-Python model of tt_mutation (include/ttga.h) for one row: the block
that lane 0 of mutation_kernel runs (csrc/tt_rooms.hip), with ttga.rng for the
draws, and of the draws tt_ga_breed makes before it. It follows the kernel
where the reference's randomMove (Solution.cpp:441-469) never returns: a
rejection loop gives up after `bound` further draws (the kernel's
kMaxRejections, 2^20) and the move is applied with the coinciding events, in
the kernel's order of slot writes. A loop that cannot end -- every event is
already taken: any loop at E 1, the third event's at E 2 -- is not replayed
draw by draw: the state jumps by 16807^bound mod (2^31 - 1), which is what
`bound` Schrage steps give for a state in [1, 2^31 - 2].

Rooms are not modelled. tt_mutation re-assigns the touched slots, and
assignRooms works slot by slot, so from rows whose rooms are the oracle's
assign_rooms of the old slots the expected rooms are the oracle's assign_rooms
of the new slots (expected_rooms)."""
import numpy as np

from ttga.rng import AM, IA, IM, ParkMiller

SLOTS = 45
BOUND = 1 << 20


def spread_seeds(n: int, base: int = 1) -> np.ndarray:
    """n states in [1, 2^31 - 2] whose first draws spread over [0, 1): small
    consecutive seeds all draw about seed * 16807 / 2^31, i.e. move type 1."""
    k = np.arange(base, base + n, dtype=np.int64)
    return (k * np.int64(0x9E3779B1) % np.int64(IM - 1) + 1).astype(np.int64)


def move_type(state: int) -> int:
    """The move type (1, 2 or 3) a row with this stream state draws first."""
    return ParkMiller(int(state)).pick(3) + 1


def _last_pick(g: ParkMiller, n: int) -> int:
    return int(AM * g.seed * n)


def _reject(g: ParkMiller, E: int, taken: tuple, bound: int) -> int:
    """e = pick(E); then up to `bound` more picks while e is one of `taken`."""
    e = g.pick(E)
    if set(taken) >= set(range(E)):                   # the loop cannot end: skip its draws in one step
        assert 0 < g.seed < IM
        g.seed = g.seed * pow(IA, bound, IM) % IM
        return _last_pick(g, E)
    n = 0
    while e in taken and n < bound:
        e = g.pick(E)
        n += 1
    return e


def mutation_row(slot, state: int, bound: int = BOUND):
    """-> (new slot row, new rng state, move type, the events drawn)."""
    new = np.array(slot, np.uint8, copy=True)
    E = new.size
    g = ParkMiller(int(state))
    kind = g.pick(3) + 1
    assert 0 < g.seed < IM, "the stream is in range after its first draw"
    e1 = g.pick(E)
    if kind == 1:
        t = g.pick(SLOTS)
        new[e1] = t
        events = (e1,)
    elif kind == 2:
        e2 = _reject(g, E, (e1,), bound)
        t = new[e1]
        new[e1] = new[e2]
        new[e2] = t
        events = (e1, e2)
    else:
        e2 = _reject(g, E, (e1,), bound)
        e3 = _reject(g, E, (e1, e2), bound)
        t = new[e1]                                   # at e3 == e1 the third write lands on the first
        new[e1] = new[e2]
        new[e2] = new[e3]
        new[e3] = t
        events = (e1, e2, e3)
    return new, g.seed, kind, events


def mutation_rows(slot, states, bound: int = BOUND):
    """mutation_row for every row -> (slot rows, states int64, move types, [events])."""
    out = [mutation_row(slot[i], states[i], bound) for i in range(len(slot))]
    return (np.stack([o[0] for o in out]), np.array([o[1] for o in out], np.int64),
            np.array([o[2] for o in out], np.int64), [o[3] for o in out])


def breed_row(pop_slot, penalty, state: int, p_cross: float, p_mut: float, skip_init_draws: bool,
              bound: int = BOUND):
    """tt_ga_breed's draws for one child, then the mutation's: the 3E discarded
    draws (skip_init_draws), the ten selection5 picks over `penalty` (compared
    as unsigned), the crossover draw (and its E picks), the mutation draw (and
    mutation_row). -> (child slot row, new state, flags, first parent, move type or 0)."""
    pop_slot = np.asarray(pop_slot, np.uint8)
    N, E = pop_slot.shape
    pen = np.asarray(penalty).astype(np.uint32)
    g = ParkMiller(int(state))
    if skip_init_draws:
        for _ in range(3 * E):
            g.next()
    par = []
    for _ in range(2):
        best = g.pick(N)
        for _ in range(4):
            t = g.pick(N)
            if pen[t] < pen[best]:
                best = t
        par.append(best)
    flags = 0
    if g.next() < p_cross:
        flags |= 1
        child = np.array([pop_slot[par[0] if g.next() < 0.5 else par[1], e] for e in range(E)], np.uint8)
    else:
        child = pop_slot[par[0]].copy()
    kind = 0
    if g.next() < p_mut:
        flags |= 2
        child, g.seed, kind, _ = mutation_row(child, g.seed, bound)
    return child, g.seed, flags, par[0], kind


def breed_rows(pop_slot, penalty, states, p_cross, p_mut, skip_init_draws, bound: int = BOUND):
    """breed_row for every stream -> (child rows, states int64, flags uint8, first parents, move types)."""
    out = [breed_row(pop_slot, penalty, s, p_cross, p_mut, skip_init_draws, bound) for s in states]
    return (np.stack([o[0] for o in out]), np.array([o[1] for o in out], np.int64),
            np.array([o[2] for o in out], np.uint8), np.array([o[3] for o in out], np.int64),
            np.array([o[4] for o in out], np.int64))


def expected_rooms(orc_problem, new_slot) -> np.ndarray:
    """The rooms after a mutation of rows that had the oracle's assign_rooms of
    their old slots: untouched slots keep those rooms, touched ones get them."""
    return orc_problem.assign_rooms(new_slot)
