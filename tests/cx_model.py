"""CPU model of the conflict-guided crossover (include/ttga_cx.h), written from
the header's text and independent of the kernels: the guided slot rows with
their Random draws, the breed sequence around them, and a replay checker that
needs no RNG. Rooms and the mutation move are the oracle's (assign_rooms,
mutation)."""
import numpy as np

from ttga.rng import ParkMiller

NUM_SLOTS = 45
BIG = 1 << 30                      # "a value greater than every cost"
FLAG_CROSS, FLAG_MUTATE = 1, 2


def _neighbours(inst):
    """eventCorrelations without the diagonal, as an int32 [E, E] 0/1 matrix."""
    c = (inst.correlations() > 0).astype(np.int32)
    np.fill_diagonal(c, 0)
    return c


def guided_row(nb, R, order, A, B, g, repair, stats=None):
    """One child: parents' slot rows A, B, the stream g (a ParkMiller, advanced
    by one draw per order entry). Returns (slot row uint8 [E], cost, repaired).
    stats (optional dict) counts the events by branch: "fallback", "cost", "coin"."""
    E = nb.shape[0]
    row = np.full(E, 255, np.uint8)
    conf = np.zeros((E, NUM_SLOTS), np.int64)       # conf[f, t]: events placed in t correlated with f
    count = np.zeros(NUM_SLOTS, np.int64)
    cost_sum, repaired, invalid = 0, 0, False
    for e in order:
        e = int(e)
        u = g.next()                                 # one draw per entry, whatever follows
        if not 0 <= e < E:
            continue
        cost = conf[e] + (count >= R)
        a, b = int(A[e]), int(B[e])
        ca = int(cost[a]) if a < NUM_SLOTS else BIG
        cb = int(cost[b]) if b < NUM_SLOTS else BIG
        if repair and min(ca, cb) > 0:
            T = np.flatnonzero(cost == cost.min())
            t = int(T[int(u * len(T))])
            repaired += 1
            branch = "fallback"
        elif ca < cb:
            t, branch = a, "cost"
        elif cb < ca:
            t, branch = b, "cost"
        else:
            t, branch = (a if u < 0.5 else b), "coin"
        if stats is not None:
            stats[branch] = stats.get(branch, 0) + 1
        row[e] = t
        if t < NUM_SLOTS:
            cost_sum += int(cost[t])
            count[t] += 1
            conf[:, t] += nb[e]
        else:
            invalid = True
    return row, (-1 if invalid else cost_sum), repaired


def guided_slots(inst, order, A, B, seeds, repair, stats=None):
    """The slot rows [P, E] (uint8) of the children of A[i] x B[i] on
    Random(seeds[i]), their final states (int64 [P]), cost and repaired
    (int32 [P])."""
    nb = _neighbours(inst)
    P = len(seeds)
    slot = np.zeros((P, inst.E), np.uint8)
    state, cost, rep = np.zeros(P, np.int64), np.zeros(P, np.int32), np.zeros(P, np.int32)
    for i in range(P):
        g = ParkMiller(int(seeds[i]))
        slot[i], cost[i], rep[i] = guided_row(nb, inst.R, order, A[i], B[i], g, repair, stats)
        state[i] = g.seed
    return slot, state, cost, rep


def breed(inst, o, order, pop_slot, pop_room, pen, seeds, p_cross, p_mut, skip_init, repair):
    """tt_ga_breed_guided on the host: per child c on Random(seeds[c]) the 3 E
    discarded draws (skip_init), two selection5 tournaments (strict unsigned
    compare: the first pick wins ties), the crossover draw, the guided rows or
    the copy of the first parent, the mutation draw and the oracle's mutation.
    `o` is the oracle's problem handle. Returns (slot, room, flags, rng, cost,
    repaired)."""
    nb = _neighbours(inst)
    E, N, C = inst.E, len(pop_slot), len(seeds)
    upen = np.asarray(pen, np.int32).astype(np.int64) & 0xFFFFFFFF
    cs, cr = np.zeros((C, E), np.uint8), np.zeros((C, E), np.uint8)
    flags, rng = np.zeros(C, np.uint8), np.zeros(C, np.int64)
    cost, rep = np.zeros(C, np.int32), np.zeros(C, np.int32)
    for c in range(C):
        g = ParkMiller(int(seeds[c]))
        if skip_init:
            for _ in range(3 * E):
                g.next()
        best = []
        for _ in range(2):
            b = g.pick(N)
            for _ in range(4):
                t = g.pick(N)
                if upen[t] < upen[b]:
                    b = t
            best.append(b)
        if g.next() < p_cross:
            flags[c] |= FLAG_CROSS
            cs[c], cost[c], rep[c] = guided_row(nb, inst.R, order, pop_slot[best[0]], pop_slot[best[1]], g, repair)
            cr[c] = o.assign_rooms(cs[c:c + 1])[0]
        else:
            cs[c], cr[c] = pop_slot[best[0]], pop_room[best[0]]
        if g.next() < p_mut:
            flags[c] |= FLAG_MUTATE
            s, r, st = o.mutation(cs[c:c + 1], cr[c:c + 1], np.array([g.seed], np.int64))
            cs[c], cr[c], g.seed = s[0], r[0], int(st[0])
        rng[c] = g.seed
    return cs, cr, flags, rng, cost, rep


def replay_check(inst, order, A, B, row, repair, cost, repaired) -> None:
    """Asserts that `row` (one finished child slot row) obeys the rule given
    what was placed before each event, and that cost and repaired are the sums
    the header defines. No RNG. `order` must be a permutation."""
    E, R = inst.E, inst.R
    nb = _neighbours(inst)
    assert sorted(int(e) for e in order) == list(range(E)), "order is not a permutation"
    conf = np.zeros((E, NUM_SLOTS), np.int64)
    count = np.zeros(NUM_SLOTS, np.int64)
    cost_sum, rep, invalid = 0, 0, False
    for e in order:
        e = int(e)
        c = conf[e] + (count >= R)
        a, b, t = int(A[e]), int(B[e]), int(row[e])
        ca = int(c[a]) if a < NUM_SLOTS else BIG
        cb = int(c[b]) if b < NUM_SLOTS else BIG
        if repair and min(ca, cb) > 0:
            assert t < NUM_SLOTS and c[t] == c.min(), f"event {e} repaired into slot {t} at cost {c[t]}, minimum {c.min()}"
            rep += 1
        elif ca < cb:
            assert t == a, f"event {e}: slot {t}, parent 1's {a} costs {ca} < {cb}"
        elif cb < ca:
            assert t == b, f"event {e}: slot {t}, parent 2's {b} costs {cb} < {ca}"
        else:
            assert t in (a, b), f"event {e}: slot {t} is neither parent's ({a}, {b})"
        if t < NUM_SLOTS:
            cost_sum += int(c[t])
            count[t] += 1
            conf[:, t] += nb[e]
        else:
            invalid = True
    assert int(cost) == (-1 if invalid else cost_sum), (int(cost), cost_sum, invalid)
    assert int(repaired) == rep, (int(repaired), rep)


def shared_pairs(inst, rows) -> np.ndarray:
    """Per row, the pairs of correlated events that share a timeslot (< 45)."""
    nb = _neighbours(inst)
    out = np.zeros(len(rows), np.int64)
    for i, row in enumerate(rows):
        row = np.asarray(row).astype(np.int64)
        same = (row[:, None] == row[None, :]) & (row[:, None] < NUM_SLOTS)
        out[i] = int((nb * same).sum()) // 2
    return out
