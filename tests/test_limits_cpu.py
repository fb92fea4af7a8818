"""Host-side half of the tests at the documented limits of E, R, S and F
(tests/test_gpu_limits.py is the device half and imports the instances and
populations built here): the mutation model (tests/mutation_model.py) against
the oracle wherever the reference's randomMove returns, the seed choice of the
E < 3 mutation test, and what the oracle says about the inputs of the device
tests -- so that a badly chosen input shows here, before any device runs it."""
import functools

import numpy as np
import pytest

import mutation_model as mm
import ttga
from oracle_lib import oracle
from ttga.ga import stream_seeds
from ttga.rng import IM, ParkMiller

# (E, R, F, S): one, two and three events (Move2 needs two, Move3 three); 44..46 around the
# 45 timeslots; 63..65 around the 64-bit event word and the local search's small-task limit;
# R 1 and 64; no students; no features
SHAPES = [(1, 1, 0, 0), (1, 1, 1, 1), (1, 2, 2, 3), (2, 1, 1, 3), (2, 3, 0, 5), (3, 2, 2, 5), (44, 3, 2, 30),
          (45, 3, 2, 30), (46, 3, 0, 30), (63, 5, 3, 0), (64, 64, 3, 40), (65, 1, 3, 40)]
# 65 events in one room and 45 slots: no timetable is feasible
NEVER_FEASIBLE = {(65, 1, 3, 40)}
P_ROWS = 67                                            # one full 64-row tile and three rows


def shape_id(d):
    return "E%dR%dF%dS%d" % d


@functools.lru_cache(maxsize=None)
def instance(dims):
    E, R, F, S = dims
    if S > 0 and F > 0:
        return ttga.generate(E, R, F, S, seed=E + S, min_att=1, max_att=min(E, 9))
    rng = np.random.default_rng(E + S)
    A = np.zeros((S, E), np.int32)
    for s in range(S):                                  # 1..min(E, 9) events per student
        A[s, rng.choice(E, size=int(rng.integers(1, min(E, 9) + 1)), replace=False)] = 1
    top = int(A.sum(axis=0).max(initial=0))
    sizes = rng.integers(1, top + 2, size=R)
    sizes[0] = max(top, 1)                              # every event has a possible room
    rf = rng.random((R, F)) < 0.6
    rf[0] = True
    return ttga.Instance(E, R, F, S, sizes, A, rf, rng.random((E, F)) < 0.2)


@functools.lru_cache(maxsize=None)
def orc():
    return oracle()


@functools.lru_cache(maxsize=None)
def problem(dims):
    return orc().problem(instance(dims))


def init_seeds(dims, n=P_ROWS):
    return stream_seeds(dims[0] + dims[3], 0, n)


LS_SMALL_ROWS = 24
LS_PROBS = [(1, 1, 0), (1, 1, 1), (0.7, 0.4, 0.5)]


@functools.lru_cache(maxsize=None)
def small_ls_case(dims, probs):
    """The first 24 random-init rows and the oracle's local search of them with
    the move probabilities `probs`: {0, 1, 200: steps from the start, "chain":
    1000 more steps on the rows after 200} -> ((slots, rooms, streams), evaluation)."""
    o = problem(dims)
    start = o.random_init(init_seeds(dims, LS_SMALL_ROWS))
    out = {}
    for steps in (0, 1, 200):
        res = o.local_search(*start, steps, *probs)
        out[steps] = (res, o.eval(res[0], res[1]))
    res = o.local_search(*out[200][0], 1000, *probs)
    out["chain"] = (res, o.eval(res[0], res[1]))
    return start, out


def small_rows(dims, n, seed):
    """n random slot rows with the oracle's rooms."""
    o = problem(dims)
    slots = np.random.default_rng(seed).integers(0, 45, size=(n, dims[0]), dtype=np.uint8)
    return slots, o.assign_rooms(slots)


def breed_case_below_three(dims, skip):
    """Eight members, eight streams and the model's children for tt_ga_breed
    with p_cross 0 and p_mut 1 at E < 3: (slots, rooms, penalty, seeds, model)."""
    o = problem(dims)
    slots, rooms = small_rows(dims, 8, 21)
    pen = o.eval(slots, rooms)[3]
    seeds = mm.spread_seeds(8, 40)
    return slots, rooms, pen, seeds, mm.breed_rows(slots, pen, seeds, 0.0, 1.0, bool(skip))


def eval_population(o, inst, slots, rooms):
    """The 67 rows of the evaluation tests from `slots`, `rooms` (random-init
    rows): rows 40..59 get random rooms, row 60 has every event in slot 0, room
    0, row 61 every event in slot 44, room R-1; rows 62..64 are invalid (slot
    45 at event 0, slot 255 at event E-1, room R at event E//2). Returns slots,
    rooms and the expected (hcv, scv, feasible, penalty): the oracle's on the
    valid rows, the -1 / -1 / 0 / -1 sentinels on the invalid ones."""
    E, R = inst.E, inst.R
    s, r = slots.copy(), rooms.copy()
    assert s.shape == (P_ROWS, E)
    r[40:60] = np.random.default_rng(E + R).integers(0, R, size=(20, E), dtype=np.uint8)
    s[60], r[60] = 0, 0
    s[61], r[61] = 44, R - 1
    s[62, 0] = 45
    s[63, E - 1] = 255
    r[64, E // 2] = R
    ok = np.ones(P_ROWS, bool)
    ok[62:65] = False
    want = [np.full(P_ROWS, -1, np.int32), np.full(P_ROWS, -1, np.int32), np.zeros(P_ROWS, np.uint8),
            np.full(P_ROWS, -1, np.int32)]
    for w, v in zip(want, o.eval(s[ok], r[ok])):
        w[ok] = v
    return s, r, tuple(want)


# ---------------------------------------------------------------- more than 65,535 students
BIG_E, BIG_F, BIG_S = 40, 3, 66000
BIG_CASES = [(5, BIG_S), (16, BIG_S), (17, BIG_S), (40, BIG_S), (5, 65535)]


def big_id(c):
    return "R%dS%d" % c


@functools.lru_cache(maxsize=None)
def big_matrices():
    """student_events [66000, 40]: event 0 has all 66,000 students, event 1 the
    first 65,535 and event 2 the first 65,536; the others Bernoulli(0.08)."""
    rng = np.random.default_rng(1)
    A = (rng.random((BIG_S, BIG_E)) < 0.08).astype(np.int32)
    A[:, 0] = 1
    A[:, 1] = np.arange(BIG_S) < 65535
    A[:, 2] = np.arange(BIG_S) < 65536
    ef = (rng.random((BIG_E, BIG_F)) < 0.2).astype(np.int32)
    return A, ef


@functools.lru_cache(maxsize=None)
def big_instance(case):
    """R rooms of 20,000..70,000 seats; room 0 has 70,000, rooms 1 and 2 have
    65,535 and 65,536 (uniform sizes hardly ever fall between the three big
    events' 65,535, 65,536 and 66,000 students), all three with every feature,
    so the three big events differ in their possible rooms. S 65,535 keeps the
    first 65,535 students: the largest studentNumber is then exactly 0xFFFF."""
    R, S = case
    A, ef = big_matrices()
    rng = np.random.default_rng(R)
    sizes = rng.integers(20000, 70001, size=R)
    sizes[:3] = 70000, 65535, 65536
    rf = (rng.random((R, BIG_F)) < 0.6).astype(np.int32)
    rf[:3] = 1
    return ttga.Instance(BIG_E, R, BIG_F, S, sizes, A[:S], rf, ef)


@functools.lru_cache(maxsize=None)
def big_problem(case):
    return orc().problem(big_instance(case))


@functools.lru_cache(maxsize=None)
def big_eval_case(case):
    """(slots, rooms, expected evaluation) of the 67 evaluation rows of a big instance."""
    inst, o = big_instance(case), big_problem(case)
    s, r, _ = o.random_init(stream_seeds(case[0], 0, P_ROWS))
    return eval_population(o, inst, s, r)


# ---------------------------------------------------------------- the local search's layout edges
LS_EDGES = [(E, 5, 3, S) for E in (64, 65) for S in (128, 129, 512, 513)]
LS_ROWS = 24


@functools.lru_cache(maxsize=None)
def ls_edge_case(dims):
    """Random-init rows and the oracle's local search of them, 300 steps and
    then 3000 more: (inst, o, (slots, rooms, seeds), after 300, after 3000)."""
    # 2..4 events per student: with the generator's default 5..20 no row becomes feasible
    inst = ttga.generate(*dims, seed=dims[0] + dims[3], min_att=2, max_att=4)
    o = orc().problem(inst)
    start = o.random_init(stream_seeds(dims[0] + dims[3], 0, LS_ROWS))
    first = o.local_search(*start, 300)
    second = o.local_search(*first, 3000)
    return inst, o, start, first, second


# ---------------------------------------------------------------- tests
def test_rejection_skip_equals_the_draws():
    """The one-step skip of a loop that cannot end is what the loop's draws give."""
    for E, taken in ((1, (0,)), (2, (0, 1)), (2, (1, 0))):
        for seed in mm.spread_seeds(6, 3):
            a, b = ParkMiller(int(seed)), ParkMiller(int(seed))
            a.next(), b.next()
            e = mm._reject(a, E, taken, 1000)
            x = b.pick(E)
            for _ in range(1000):
                x = b.pick(E)
            assert (e, a.seed) == (x, b.seed) and 0 < a.seed < IM


@pytest.mark.parametrize("dims", [(3, 2, 2, 5), (45, 3, 2, 30), (65, 1, 3, 40)], ids=shape_id)
def test_mutation_model_vs_oracle(dims):
    o = problem(dims)
    slots, rooms = small_rows(dims, 64, 5)
    seeds = mm.spread_seeds(64)
    ws, wg, kinds, _ = mm.mutation_rows(slots, seeds)
    es, er, eg = o.mutation(slots, rooms, seeds)
    assert np.array_equal(ws, es) and np.array_equal(wg, eg)
    assert np.array_equal(mm.expected_rooms(o, ws), er)
    assert all((kinds == k).sum() >= 8 for k in (1, 2, 3))


@pytest.mark.parametrize("dims", [d for d in SHAPES if d[0] < 3], ids=shape_id)
def test_mutation_model_vs_oracle_below_three_events(dims):
    """Only the rows whose move the reference finishes go to the oracle: type 1
    at E 1, types 1 and 2 at E 2 (on the others it never returns)."""
    E = dims[0]
    o = problem(dims)
    slots, rooms = small_rows(dims, 64, 6)
    seeds = mm.spread_seeds(64)
    kinds = np.array([mm.move_type(s) for s in seeds])
    ends = kinds <= (1 if E == 1 else 2)
    assert ends.sum() >= 16 and (~ends).sum() >= 16
    ws, wg, wk, _ = mm.mutation_rows(slots[ends], seeds[ends])
    assert np.array_equal(wk, kinds[ends])
    es, er, eg = o.mutation(slots[ends], rooms[ends], seeds[ends])
    assert np.array_equal(ws, es) and np.array_equal(wg, eg)
    assert np.array_equal(mm.expected_rooms(o, ws), er)


def test_mutation_model_with_coinciding_events():
    """What the bounded loops leave: at E 1 every move but Move1 keeps the row;
    at E 2 Move3 keeps the row where e3 == e1 (the third write lands on the
    first and undoes it) and swaps the two events where e3 == e2; a loop gives
    up after `bound` further draws, and the stream has advanced by them."""
    for seed in mm.spread_seeds(24, 11):
        seed = int(seed)
        row, state, kind, ev = mm.mutation_row(np.array([7], np.uint8), seed, bound=50)
        g = ParkMiller(seed)
        for _ in range({1: 3, 2: 2 + 51, 3: 2 + 51 + 51}[kind]):
            g.next()
        assert state == g.seed and (kind == 1 or row[0] == 7) and set(ev) == {0}
        row, state, kind, ev = mm.mutation_row(np.array([3, 9], np.uint8), seed, bound=50)
        if kind == 3:
            e1, e2, e3 = ev
            assert e1 != e2 and e3 in (e1, e2)
            assert row.tolist() == ([3, 9] if e3 == e1 else [9, 3])


def test_mutation_seeds_cover_the_move_types():
    """The E < 3 device test's eight streams: every move type at least twice.
    (ttga.population_seeds(13, 8) would not do: all eight draw type 1.)"""
    kinds = [mm.move_type(s) for s in mm.spread_seeds(8)]
    assert all(kinds.count(k) >= 2 for k in (1, 2, 3)), kinds
    assert {mm.move_type(s) for s in ttga.population_seeds(13, 8)} == {1}


@pytest.mark.parametrize("dims", [(3, 2, 2, 5), (45, 3, 2, 30)], ids=shape_id)
@pytest.mark.parametrize("skip", [0, 1])
def test_breed_model_vs_oracle(dims, skip):
    o = problem(dims)
    slots, rooms = small_rows(dims, 9, 7)
    pen = np.random.default_rng(8).integers(0, 30, 9).astype(np.int32)
    pen[4] = -1
    seeds = mm.spread_seeds(32, 100)
    cs, cr, fl, rng = o.ga_breed(slots, rooms, pen, seeds, 32, 0.8, 0.5, skip)
    ws, wg, wf, _, _ = mm.breed_rows(slots, pen, seeds, 0.8, 0.5, bool(skip))
    assert np.array_equal(ws, cs) and np.array_equal(wg, rng) and np.array_equal(wf, fl)
    assert np.array_equal(mm.expected_rooms(o, ws), cr)
    assert {0, 1, 2, 3} == set(fl.tolist())


@pytest.mark.parametrize("dims", [d for d in SHAPES if d[0] < 3], ids=shape_id)
def test_breed_streams_below_three_events_cover_the_move_types(dims):
    for skip in (0, 1):
        child, states, flags, parents, kinds = breed_case_below_three(dims, skip)[4]
        assert (flags == 2).all() and all((kinds == k).any() for k in (1, 2, 3)), kinds


@pytest.mark.parametrize("dims", SHAPES, ids=shape_id)
def test_smallest_instances_on_the_oracle(dims):
    """The oracle's local search ends on every shape, and makes at least half
    the rows feasible in 200 steps wherever a feasible timetable exists (the
    1000 steps chained behind them then start in phase 2)."""
    inst = instance(dims)
    assert (inst.E, inst.R, inst.F, inst.S) == dims
    for probs in LS_PROBS:
        start, out = small_ls_case(dims, probs)
        feas = out[200][1][2]
        assert (2 * feas.sum() >= LS_SMALL_ROWS) == (dims not in NEVER_FEASIBLE), (probs, int(feas.sum()))
        assert out["chain"][1][2].sum() >= feas.sum()


def test_slotswap_table_form_vs_the_other_forms():
    """slotswap_model.deltas_lut, which the 66,000-student test descends with,
    against the model's three other forms (sm and a crowded row) and against
    deltas_windows at 66,000 students."""
    import slotswap_model as sm
    inst = ttga.config_instance("sm")
    for seed in range(3):
        row = np.random.default_rng(seed).integers(0, 45, inst.E).astype(np.uint8)
        want = sm.deltas_table(inst, row)
        assert np.array_equal(sm.deltas_lut(inst, row), want) and np.array_equal(sm.deltas_windows(inst, row), want)
    row = (row % 3 * 9 + 8).astype(np.uint8)
    assert np.array_equal(sm.deltas_lut(inst, row), sm.deltas_brute(inst, row))
    none = instance((63, 5, 3, 0))
    assert np.array_equal(sm.deltas_lut(none, row[:63]), sm.deltas_table(none, row[:63]))
    big = big_instance(BIG_CASES[0])
    row = big_eval_case(BIG_CASES[0])[0][0]
    assert np.array_equal(sm.deltas_lut(big, row), sm.deltas_windows(big, row))


@pytest.mark.parametrize("case", BIG_CASES, ids=big_id)
def test_big_instances_on_the_oracle(case):
    """studentNumber on both sides of 0xFFFF, scv beyond 16 bits, rows that differ in hcv."""
    inst = big_instance(case)
    sn, _, poss = big_problem(case).derived()
    assert sn[:3].tolist() == ([66000, 65535, 65536] if case[1] == BIG_S else [65535] * 3)
    assert sn.max() == (66000 if case[1] == BIG_S else 0xFFFF) and sn[3:].max() < 0xFFFF
    assert poss.any(axis=1).all() and not poss[:3].all() and 0 < poss.sum() < poss.size
    if case[1] == BIG_S:
        assert poss[:3, :3].tolist() == [[1, 0, 0], [1, 1, 1], [1, 0, 1]]
    _, _, (hcv, scv, feas, pen) = big_eval_case(case)
    assert scv.max() > 65535 and len(set(hcv[:62].tolist())) > 1
    assert inst.student_events.nbytes == 4 * case[1] * BIG_E


@pytest.mark.parametrize("dims", LS_EDGES, ids=shape_id)
def test_ls_edge_rows_meet_both_phases(dims):
    """Every row starts infeasible (phase 1 has work) and the oracle makes
    every row feasible within the first 300 steps (phase 2 runs in both calls)."""
    inst, o, start, first, second = ls_edge_case(dims)
    assert (o.eval(start[0], start[1])[0] > 0).all()
    assert o.eval(first[0], first[1])[2].all() and o.eval(second[0], second[1])[2].all()
    assert not np.array_equal(start[0], first[0]) and not np.array_equal(first[0], second[0])
