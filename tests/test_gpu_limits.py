"""The kernels that replace the reference's own calls -- tt_eval (every variant),
tt_assign_rooms, tt_random_init, tt_crossover, tt_mutation, tt_local_search*
and tt_ga_breed / tt_ga_replace -- at the documented limits of include/ttga.h:
E 1..3, 44..46 and 63..65, R 1 and 64, no students, no features, more than
65,535 students, the local search's LDS layout edges (S 128/129, 512/513 at
E 64/65) and tt_ga_breed on streams that start out of range. Everything is
compared bit for bit with the CPU oracle; where the reference's randomMove
never returns (E < 3) with tests/mutation_model.py. The instances, populations
and the oracle's results come from tests/test_limits_cpu.py, which checks them
on the host."""
import time
import types

import numpy as np
import pytest

import mutation_model as mm
import slotswap_model as sm
import test_limits_cpu as L
import ttga
from helpers import dev, host, oracle_generations, oracle_population
from oracle_lib import split_rows
from ttga import validate

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
from ttga import native  # noqa: E402
from ttga.ga import Island, stream_seeds  # noqa: E402
from ttga.rng import IM, step  # noqa: E402

KEYS = ("slot", "room", "hcv", "scv", "feasible", "penalty")
EVAL_NAMES = ("hcv", "scv", "feasible", "penalty")
P = L.P_ROWS


def empty_rows(n, E):
    return torch.empty((n, E), dtype=torch.uint8, device="cuda")


def eval_outputs(n):
    """Four output tensors holding values no evaluation gives."""
    i32 = lambda: torch.full((n,), -77, dtype=torch.int32, device="cuda")    # noqa: E731
    return i32(), i32(), torch.full((n,), 77, dtype=torch.uint8, device="cuda"), i32()


def assert_rows(got, want, what):
    """(slot, room, rng) device tensors against the oracle's arrays."""
    for name, g, w in zip(("slots", "rooms", "streams"), got, want):
        assert np.array_equal(host(g), w), f"{what}: {name} differ"


def assert_eval(got, want, what):
    for name, g, w in zip(EVAL_NAMES, got, want):
        g = host(g)
        bad = np.flatnonzero(g != w)[:8]
        assert bad.size == 0, f"{what}: {name} differ at rows {bad}: {g[bad]} != {w[bad]}"


def check_eval_variants(dp, slots, rooms, want, what):
    """Variants 0, 2, 7 and 8 must run and agree with `want`; the wide path (13)
    may refuse the shape with TT_ERR_LIMIT and nothing else."""
    auto = dp.eval_variant()
    assert auto in (7, 8), auto                        # ttga.h: 8 or 7 for E <= 448
    ds, dr = dev(slots), dev(rooms)
    for v in (0, 2, 7, 8):
        assert_eval(dp.eval(ds, dr, variant=v, out=eval_outputs(len(slots))), want, f"{what} variant {v}")
    try:
        got = dp.eval(ds, dr, variant=13, out=eval_outputs(len(slots)))
    except native.TTError as e:
        assert e.code == native.TT_ERR_LIMIT, e
        print(f"{what}: tt_eval_variant 13 refused the shape (TT_ERR_LIMIT)")
    else:
        assert_eval(got, want, f"{what} variant 13")


# ================================================================ A. the smallest instances
@pytest.fixture(scope="module")
def small():
    cache = {}

    def get(dims):
        if dims not in cache:
            inst, o = L.instance(dims), L.problem(dims)
            cache[dims] = types.SimpleNamespace(inst=inst, o=o, dp=native.DeviceProblem(inst),
                                                init=o.random_init(L.init_seeds(dims)))
        return cache[dims]
    return get


small_shapes = pytest.mark.parametrize("dims", L.SHAPES, ids=L.shape_id)


@small_shapes
def test_small_derived_and_random_init(small, dims):
    c = small(dims)
    for got, want, what in zip(c.dp.derived(), c.o.derived(), ("studentNumber", "eventCorrelations", "possibleRooms")):
        assert np.array_equal(got, want), what
    s, r, g = empty_rows(P, c.inst.E), empty_rows(P, c.inst.E), dev(L.init_seeds(dims))
    c.dp.random_init(g, s, r)
    assert_rows((s, r, g), c.init, "random init")


@small_shapes
def test_small_eval_variants(small, dims):
    c = small(dims)
    slots, rooms, want = L.eval_population(c.o, c.inst, c.init[0], c.init[1])
    assert (want[0][62:65] == -1).all() and (want[0][:62] >= 0).all()
    check_eval_variants(c.dp, slots, rooms, want, L.shape_id(dims))


@small_shapes
def test_small_rooms_and_crossover(small, dims):
    c = small(dims)
    slots = L.eval_population(c.o, c.inst, c.init[0], c.init[1])[0]
    slots = np.delete(slots, [62, 63], axis=0)          # the oracle takes no slot >= 45
    assert np.array_equal(host(c.dp.assign_rooms(dev(slots))), c.o.assign_rooms(slots))
    a, b, seeds = c.init[0][:33], c.init[0][33:66], mm.spread_seeds(33, 7)
    s, r, g = empty_rows(33, c.inst.E), empty_rows(33, c.inst.E), dev(seeds)
    c.dp.crossover(dev(a), dev(b), g, s, r)
    assert_rows((s, r, g), c.o.crossover(a, b, seeds), "crossover")


@pytest.mark.parametrize("probs", L.LS_PROBS, ids=lambda p: "p%g_%g_%g" % p)
@small_shapes
def test_small_local_search_eval(small, dims, probs):
    c = small(dims)
    start, want = L.small_ls_case(dims, probs)
    if dims not in L.NEVER_FEASIBLE:
        assert 2 * want[200][1][2].sum() >= L.LS_SMALL_ROWS       # the chained call starts in phase 2
    for steps in (0, 1, 200):
        s, r, g = (dev(x) for x in start)
        out = eval_outputs(L.LS_SMALL_ROWS)
        c.dp.local_search(s, r, g, steps, *probs, out=out)
        assert_rows((s, r, g), want[steps][0], f"{steps} steps")
        assert_eval(out, want[steps][1], f"{steps} steps")
    out = eval_outputs(L.LS_SMALL_ROWS)
    c.dp.local_search(s, r, g, 1000, *probs, out=out)
    assert_rows((s, r, g), want["chain"][0], "200 + 1000 steps")
    assert_eval(out, want["chain"][1], "200 + 1000 steps")
    assert c.dp.status() == 0


@small_shapes
def test_small_breed_and_replace(small, dims):
    c = small(dims)
    E = c.inst.E
    p_mut = 0.5 if E >= 3 else 0.0                      # E < 3: test_mutation_below_three_events
    for N, C in ((1, 1), (5, 1), (5, 5)):
        pop = oracle_population(c.o, N, 3 + N, 50)
        for skip in (0, 1):
            seeds = mm.spread_seeds(C, 10 * N + C + skip)
            cs, cr, fl, rng = c.o.ga_breed(pop["slot"], pop["room"], pop["penalty"], seeds, C, 0.8, p_mut, skip)
            gs, gr, gf, grng = empty_rows(C, E), empty_rows(C, E), dev(np.zeros(C, np.uint8)), dev(seeds)
            c.dp.ga_breed(dev(pop["slot"]), dev(pop["room"]), dev(pop["penalty"]), grng, gs, gr, gf, 0.8, p_mut,
                          bool(skip))
            assert np.array_equal(host(gf), fl), (N, C, skip)
            assert_rows((gs, gr, grng), (cs, cr, rng), f"breed N {N} C {C} skip {skip}")
            h, sc, f, p = c.o.eval(cs, cr)
            child = dict(slot=cs, room=cr, hcv=h, scv=sc, feasible=f, penalty=p)
            want = c.o.ga_replace(pop, child)
            gpop = {k: dev(v) for k, v in pop.items()}
            c.dp.ga_replace(gpop, {k: dev(v) for k, v in child.items()}, c.dp.ga_work(N))
            for k in KEYS:
                assert np.array_equal(host(gpop[k]), want[k]), (k, N, C, skip)


@pytest.mark.parametrize("dims", [(3, 2, 2, 5), (45, 3, 2, 30)], ids=L.shape_id)
def test_small_island_generations(small, dims):
    c = small(dims)
    N, C, gens, steps, seed = 6, 3, 5, 50, 17
    isl = Island(c.dp, pop_size=N, children=C, max_steps=steps, seed=seed)
    isl.initialize()
    for _ in range(gens):
        isl.step()
    pop = oracle_population(c.o, N, seed, steps)
    pop, rng = oracle_generations(c.o, pop, stream_seeds(seed, N, C), C, gens, steps)
    for k in KEYS:
        assert np.array_equal(host(isl.pop[k]), pop[k]), k
    assert np.array_equal(host(isl.rng_child), rng)
    assert c.dp.status() == 0
    isl.close()


@pytest.mark.parametrize("dims", [d for d in L.SHAPES if d[0] >= 3], ids=L.shape_id)
def test_small_mutation(small, dims):
    c = small(dims)
    seeds = mm.spread_seeds(P)
    assert {mm.move_type(x) for x in seeds} == {1, 2, 3}
    s, r, g = dev(c.init[0]), dev(c.init[1]), dev(seeds)
    c.dp.mutation(s, r, g)
    assert_rows((s, r, g), c.o.mutation(c.init[0], c.init[1], seeds), "mutation")


# ================================================================ B. tt_mutation below three events
below_three = pytest.mark.parametrize("dims", [d for d in L.SHAPES if d[0] < 3], ids=L.shape_id)


@below_three
def test_mutation_below_three_events(small, dims):
    """Move2 at E 1 and Move3 at E <= 2: every rejection loop gives up after 2^20
    draws and the move is applied with the coinciding events (ttga.h); eight
    rows, every move type at least twice. A launch takes about 0.2 s at E 1
    (Move3: 2^21 draws on one lane) and 0.12 s at E 2 on an MI355X."""
    c = small(dims)
    slots, rooms = L.small_rows(dims, 8, 21)
    seeds = mm.spread_seeds(8)
    kinds = [mm.move_type(x) for x in seeds]
    assert all(kinds.count(k) >= 2 for k in (1, 2, 3)), kinds
    ws, wg, wk, _ = mm.mutation_rows(slots, seeds)
    assert wk.tolist() == kinds
    s, r, g = dev(slots), dev(rooms), dev(seeds)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    c.dp.mutation(s, r, g)
    torch.cuda.synchronize()
    print(f"tt_mutation {L.shape_id(dims)}: 8 rows in {1e3 * (time.perf_counter() - t0):.1f} ms")
    assert_rows((s, r, g), (ws, mm.expected_rooms(c.o, ws), wg), "mutation")


@pytest.mark.parametrize("skip", [0, 1])
@below_three
def test_breed_mutation_below_three_events(small, dims, skip):
    """tt_ga_breed with p_cross 0 and p_mut 1: every child is a copy of its first
    parent, mutated; the streams replay the breed's own draws and then the
    mutation's."""
    c = small(dims)
    slots, rooms, pen, seeds, (ws, wg, wf, _, kinds) = L.breed_case_below_three(dims, skip)
    assert (wf == 2).all() and set(kinds.tolist()) == {1, 2, 3}
    E, C = c.inst.E, len(seeds)
    gs, gr, gf, grng = empty_rows(C, E), empty_rows(C, E), dev(np.zeros(C, np.uint8)), dev(seeds)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    c.dp.ga_breed(dev(slots), dev(rooms), dev(pen), grng, gs, gr, gf, 0.0, 1.0, bool(skip))
    torch.cuda.synchronize()
    print(f"tt_ga_breed {L.shape_id(dims)} skip {skip}: 8 children in {1e3 * (time.perf_counter() - t0):.1f} ms")
    assert np.array_equal(host(gf), wf)
    assert_rows((gs, gr, grng), (ws, mm.expected_rooms(c.o, ws), wg), "breed")


# ================================================================ C. more than 65,535 students
@pytest.fixture(scope="module")
def big():
    cache = {}

    def get(case):
        if case not in cache:
            inst = L.big_instance(case)
            cache[case] = types.SimpleNamespace(inst=inst, o=L.big_problem(case), dp=native.DeviceProblem(inst))
        return cache[case]
    return get


big_cases = pytest.mark.parametrize("case", L.BIG_CASES, ids=L.big_id)


@big_cases
def test_big_derived(big, case):
    c = big(case)
    sn, corr, poss = c.dp.derived()
    osn, ocorr, oposs = c.o.derived()
    assert np.array_equal(sn, osn) and np.array_equal(poss, oposs)
    assert set(np.unique(corr)) <= {0, 1}
    assert np.array_equal(np.packbits(corr.astype(bool)), np.packbits(ocorr.astype(bool)))


@big_cases
def test_big_eval_variants(big, case):
    """The studentNumber packing of eval_tile5 on both sides of its test (R <= 16
    and max_sn <= 0xFFFF), scv sums beyond 16 bits."""
    c = big(case)
    slots, rooms, want = L.big_eval_case(case)
    assert want[1].max() > 65535 and len(set(want[0][:62].tolist())) > 1
    check_eval_variants(c.dp, slots, rooms, want, L.big_id(case))


@big_cases
def test_big_eval_parts(big, case):
    c = big(case)
    slots, rooms, want = L.big_eval_case(case)
    ok = want[0] >= 0
    parts, eh = (host(t) for t in c.dp.eval_parts(dev(slots), dev(rooms), event_hcv=True))
    assert (parts[~ok] == -1).all() and (eh[~ok] == -1).all()
    assert np.array_equal(parts[ok, :3].sum(1), want[0][ok]) and np.array_equal(parts[ok, 3:].sum(1), want[1][ok])
    assert np.array_equal(eh[ok].sum(1), 2 * (parts[ok, 0] + parts[ok, 1]))
    for i in (0, 41, 61):
        ev = validate.evaluate(c.inst, slots[i], rooms[i])
        assert parts[i].tolist() == [ev[k] for k in native.PART_NAMES], i


@big_cases
def test_big_local_search_eval(big, case):
    c = big(case)
    start = c.o.random_init(stream_seeds(3, 0, 8))
    s, r, g = (dev(x) for x in start)
    rows = start
    for steps in (100, 1000):
        rows = split_rows(c.o.local_search, rows, steps)
        out = eval_outputs(8)
        c.dp.local_search(s, r, g, steps, out=out)
        assert_rows((s, r, g), rows, f"{steps} steps")
        want = c.o.eval(rows[0], rows[1])
        assert want[1].max() > 65535                    # scv beyond 16 bits in the search's own evaluation
        assert_eval(out, want, f"{steps} steps")
    assert c.dp.status() == 0


@big_cases
def test_big_slot_swap(big, case):
    """Four rows (two random, one with random rooms, the one with every event
    in slot 44): the numpy model takes about 0.07 s per pass and row here."""
    c = big(case)
    slots, rooms, want = L.big_eval_case(case)
    pick = [0, 1, 40, 61]
    slots, rooms = slots[pick], rooms[pick]
    logs = [[] for _ in pick]
    for i in range(len(pick)):
        sm.descend(c.inst, slots[i], 64, deltas=sm.deltas_lut, log=logs[i])
    assert max(len(lg) for lg in logs) > 1
    for cap in (1, 64):
        rows, gain, passes, perm = sm.stack([sm.prefix(slots[i], logs[i], cap) for i in range(len(pick))])
        s, scv, pen = dev(slots), dev(want[1][pick]), dev(want[3][pick])
        ggain = torch.full((4,), 12345, dtype=torch.int32, device="cuda")
        gpasses = torch.full((4,), 12345, dtype=torch.int32, device="cuda")
        gperm = torch.full((4, 45), 99, dtype=torch.uint8, device="cuda")
        c.dp.slot_swap(s, cap, scv=scv, penalty=pen, gain=ggain, passes=gpasses, perm=gperm)
        got = (s, ggain, gpasses, gperm)
        for name, g, w in zip(("rows", "gain", "passes", "perm"), got, (rows, gain, passes, perm)):
            assert np.array_equal(host(g), w), (name, cap)
        h, sc, f, p = c.o.eval(rows, rooms)
        assert np.array_equal(h, want[0][pick]) and np.array_equal(sc, want[1][pick] - gain)
        assert np.array_equal(host(scv), sc) and np.array_equal(host(pen), p)
    assert (c.dp.status() & ~2) == 0


# ================================================================ D. the local search's layout edges
@pytest.mark.parametrize("dims", L.LS_EDGES, ids=L.shape_id)
def test_local_search_layout_edges(dims):
    """8 * S against kSmaskMaxBytes (phase-2 student masks up to S 512) and
    against kSinfBytes (the phase-1 slot summaries alias the masks from S 129
    up), on both sides of the one-launch limit E 64. A launch of 24 waves keeps
    every wave resident with the masks, so ls_mask_students gives S up to 512
    and 0 above; only E > 64 records it."""
    inst, o, start, first, second = L.ls_edge_case(dims)
    E, S = dims[0], dims[3]
    assert (o.eval(start[0], start[1])[0] > 0).all() and o.eval(first[0], first[1])[2].all()
    dp = native.DeviceProblem(inst)
    s, r, g = (dev(x) for x in start)
    for steps, want in ((300, first), (3000, second)):
        dp.local_search(s, r, g, steps)
        assert_rows((s, r, g), want, f"{steps} steps")
        if E > 64:
            assert dp.local_search_masks() == (S if S <= 512 else 0)
    assert dp.status() == 0
    dp.close()


# ================================================================ E. breed on out-of-range streams
@pytest.mark.parametrize("skip", [0, 1])
def test_breed_edge_seeds_vs_oracle(skip):
    """Streams outside [0, 2^31 - 1): the first draw takes the 64-bit Schrage
    step and lands in range for every one of these seeds, so with
    skip_init_draws the 3E - 1 draws behind it are one jump. (breed_kernel's
    sequential branch is for a first draw that stays out of range: the
    reference then draws outside [0, 1) and picks parents outside the
    population, which is undefined there and not tested.)"""
    inst = ttga.config_instance("sm")
    dp, o = native.DeviceProblem(inst), L.orc().problem(inst)
    N = C = 12
    seeds = np.array([0, 1, -1, -123456789, -2_000_000_000, 2**31 - 2, 2**31 - 1, 2**31, 2**31 + 5,
                      3_000_000_000, 4_000_000_000, 42], dtype=np.int64)
    assert all(0 <= step(int(x)) < IM for x in seeds)
    pop = oracle_population(o, N, 3, 50)
    cs, cr, fl, rng = o.ga_breed(pop["slot"], pop["room"], pop["penalty"], seeds, C, 0.8, 0.5, skip)
    gs, gr, gf, grng = empty_rows(C, inst.E), empty_rows(C, inst.E), dev(np.zeros(C, np.uint8)), dev(seeds)
    dp.ga_breed(dev(pop["slot"]), dev(pop["room"]), dev(pop["penalty"]), grng, gs, gr, gf, 0.8, 0.5, bool(skip))
    assert np.array_equal(host(gf), fl)
    assert_rows((gs, gr, grng), (cs, cr, rng), "breed")
    dp.close()
