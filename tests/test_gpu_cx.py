"""The conflict-guided crossover (include/ttga_cx.h) on the GPU against
tests/cx_model.py: slot rows, room rows (the model's slots through the oracle's
assign_rooms), final Random states, cost and repaired bit for bit; the uniform
crossover recovered on a cost-free instance; the replay check (no RNG) on the
GPU's own rows; a caller's and an invalid order; parents' genes >= 45;
tt_ga_breed_guided against the model's breed and against tt_ga_breed; the limit;
the point of it (fewer hard violations than the uniform children); Island with
crossover="guided"; and the two drivers with --crossover guided."""
import pathlib

import numpy as np
import pytest

import ttga
import cx_model as cm
import greedy_model as gm
from helpers import dev, host, json_lines
from oracle_lib import oracle
from stage_checks import GA, both_drivers, run_driver

pytestmark = pytest.mark.gpu

import torch  # noqa: E402
from ttga import native  # noqa: E402
from ttga.ga import Island, stream_seeds  # noqa: E402
from ttga.rng import random_slots  # noqa: E402

REPO = pathlib.Path(__file__).resolve().parent.parent
BAD_ORDER = 512                                             # tt_device_status bit 9

# seeds: 1, the largest in-range state, 0 (the stream stays 0), one above 2^31
# (pm_next's out-of-range first step), and ordinary ones
SPECIAL_SEEDS = np.array([1, 2147483646, 0, 3000000019, 1000, 1001], np.int64)

# E: fewer events than slots, the bitset word edges, both sides of the register/LDS
# split (448 | 449), a wider one; R = 1 (the full-slot term decides) and R = 64
SHAPES = {
    "E1": lambda: ttga.generate(1, 2, 2, 3, seed=3, min_att=1, max_att=1),
    "E44": lambda: ttga.generate(44, 3, 2, 30, seed=4, min_att=3, max_att=10),
    "E45": lambda: ttga.generate(45, 3, 2, 30, seed=5, min_att=3, max_att=10),
    "E64": lambda: ttga.generate(64, 4, 3, 40, seed=6),
    "E65": lambda: ttga.generate(65, 4, 3, 40, seed=7),
    "E128": lambda: ttga.generate(128, 5, 3, 60, seed=8),
    "E129": lambda: ttga.generate(129, 5, 3, 60, seed=9),
    "R1": lambda: ttga.generate(100, 1, 2, 40, seed=10),
    "R64": lambda: ttga.generate(120, 64, 4, 50, seed=11),
    "E448": lambda: ttga.generate(448, 10, 5, 150, seed=12),
    "E449": lambda: ttga.generate(449, 10, 5, 150, seed=13),
    "E1000R24": lambda: ttga.generate(1000, 24, 5, 250, seed=14),
    "sm": lambda: ttga.config_instance("sm"),
    "med": lambda: ttga.config_instance("med"),
    "free": lambda: ttga.generate(40, 64, 2, 0),           # no students: every cost is 0
    "free449": lambda: ttga.generate(449, 64, 2, 0),       # the same on the LDS-row path
}


@pytest.fixture(scope="module")
def orc():
    return oracle()


@pytest.fixture(scope="module")
def problems():
    cache = {}

    def get(name):
        if name not in cache:
            inst = SHAPES[name]()
            cache[name] = (inst, native.DeviceProblem(inst), gm.greedy_order(inst))
        return cache[name]
    return get


def parents_of(inst, order, kind, P, base=40):
    if kind == "greedy":
        rows, _ = gm.greedy_slots(inst, order, ttga.population_seeds(base, 2 * P))
        return rows[:P], rows[P:]
    return (random_slots(ttga.population_seeds(base, P), inst.E)[0],
            random_slots(ttga.population_seeds(base + 5000, P), inst.E)[0])


def gpu_cross(dp, A, B, seeds, repair, order=None, outputs=True):
    P = len(seeds)
    rng = dev(seeds)
    slot = torch.full((P, dp.E), 0xEE, dtype=torch.uint8, device="cuda")
    room = torch.full((P, dp.E), 0xEE, dtype=torch.uint8, device="cuda")
    cost = torch.full((P,), 12345, dtype=torch.int32, device="cuda") if outputs else None
    rep = torch.full((P,), 12345, dtype=torch.int32, device="cuda") if outputs else None
    dp.crossover_guided(dev(A), dev(B), rng, slot, room, order=order, repair=repair, cost=cost, repaired=rep)
    return host(slot), host(room), host(rng), (host(cost) if outputs else None), (host(rep) if outputs else None)


def check_exact(orc, inst, dp, order, A, B, seeds, repair, stats=None, order_dev=None):
    s, r, g, c, n = gpu_cross(dp, A, B, seeds, repair, order=order_dev)
    ws, wg, wc, wn = cm.guided_slots(inst, order, A, B, seeds, repair, stats)
    assert np.array_equal(s, ws), f"slot rows differ in {np.flatnonzero((s != ws).any(axis=1))[:8]}"
    assert np.array_equal(g, wg)
    assert np.array_equal(g, [gm.advanced(x, inst.E) for x in seeds])
    assert np.array_equal(c, wc) and np.array_equal(n, wn)
    assert np.array_equal(r, orc.problem(inst).assign_rooms(ws))
    if not repair:
        assert ((s == A) | (s == B)).all() and (n == 0).all()
    return s


# ---------------------------------------------------------------- bit-exact
CASES = [(n, "random") for n in SHAPES if not n.startswith("free")] + [("sm", "greedy"), ("med", "greedy")]


@pytest.mark.parametrize("repair", [0, 1])
@pytest.mark.parametrize("name,kind", CASES)
def test_bit_exact_shapes(orc, problems, name, kind, repair):
    inst, dp, order = problems(name)
    A, B = parents_of(inst, order, kind, len(SPECIAL_SEEDS))
    stats = {}
    check_exact(orc, inst, dp, order, A, B, SPECIAL_SEEDS, repair, stats)
    if name in ("sm", "med"):
        # random parents bring many unequal costs, greedy ones mostly ties: each branch occurs
        assert stats.get("coin", 0) > 0 and stats.get("cost", 0) > 0, stats
        assert (stats.get("fallback", 0) > 0) == bool(repair), stats
    if name == "R1":
        assert stats.get("cost", 0) > 0                    # the full-slot term decides
    assert dp.status() & BAD_ORDER == 0


@pytest.mark.parametrize("P", [1, 64, 65, 130])
def test_bit_exact_population_sizes(orc, problems, P):
    """P = 65 and 130 end in a partial workgroup (four children per workgroup at
    E <= 448)."""
    inst, dp, order = problems("sm")
    A, B = parents_of(inst, order, "random", P, base=900)
    check_exact(orc, inst, dp, order, A, B, ttga.population_seeds(31000, P), P & 1)


def test_bit_exact_wide_partial_population(orc, problems):
    inst, dp, order = problems("E449")
    A, B = parents_of(inst, order, "random", 67, base=901)
    check_exact(orc, inst, dp, order, A, B, ttga.population_seeds(32000, 67), 1)


@pytest.mark.parametrize("repair", [0, 1])
@pytest.mark.parametrize("name", ["free", "free449"])
def test_cost_free_identity_order_is_tt_crossover(problems, name, repair):
    inst, dp, _ = problems(name)
    A, B = parents_of(inst, None, "random", 6)
    s, r, g, c, n = gpu_cross(dp, A, B, SPECIAL_SEEDS, repair, order=dev(np.arange(inst.E, dtype=np.int32)))
    rng = dev(SPECIAL_SEEDS)
    us, ur = torch.empty((6, inst.E), dtype=torch.uint8, device="cuda"), torch.empty((6, inst.E), dtype=torch.uint8,
                                                                                  device="cuda")
    dp.crossover(dev(A), dev(B), rng, us, ur)
    assert np.array_equal(s, host(us)) and np.array_equal(r, host(ur)) and np.array_equal(g, host(rng))
    assert (c == 0).all() and (n == 0).all()


# ---------------------------------------------------------------- replay, orders
@pytest.mark.parametrize("name", ["med", "E449"])
def test_replay_of_gpu_rows(problems, name):
    """Independent of the model's RNG: every event of a GPU row obeys the rule
    given what was placed before it, in the GPU's own order."""
    inst, dp, _ = problems(name)
    order = host(dp.greedy_order())
    for kind in ("random", "greedy"):
        A, B = parents_of(inst, order, kind, 3, base=77)
        for repair in (0, 1):
            s, _, _, c, n = gpu_cross(dp, A, B, ttga.population_seeds(78, 3), repair)
            for i in range(3):
                cm.replay_check(inst, order, A[i], B[i], s[i], repair, c[i], n[i])


@pytest.mark.parametrize("reverse", [False, True])
def test_caller_order(orc, problems, reverse):
    """Any permutation is a valid order: the events by index, and reversed."""
    inst, dp, _ = problems("sm")
    order = np.arange(inst.E, dtype=np.int32)[::-1 if reverse else 1].copy()
    A, B = parents_of(inst, None, "random", 5, base=9)
    check_exact(orc, inst, dp, order, A, B, ttga.population_seeds(9, 5), 1, order_dev=dev(order))
    check_exact(orc, inst, dp, order, A, B, ttga.population_seeds(9, 5), 0, order_dev=dev(order))


@pytest.mark.parametrize("name", ["sm", "E449"])
def test_invalid_order(orc, name):
    """Entries outside 0..E-1 are skipped with their draw consumed, status bit 9
    is set, the events nobody names keep slot and room 255, and nothing is
    written outside the rows. Own handles: the status word is sticky."""
    inst = SHAPES[name]()
    dp = native.DeviceProblem(inst)
    E, P = inst.E, 5
    order = gm.greedy_order(inst).copy()
    lost = [int(order[3]), int(order[E // 2]), int(order[E - 1])]
    order[3], order[E // 2], order[E - 1] = -1, E, 2 ** 31 - 1
    seeds = ttga.population_seeds(600, P)
    A, B = parents_of(inst, None, "random", P, base=601)
    rng = dev(seeds)
    slot = torch.full((P + 2, E), 0xEE, dtype=torch.uint8, device="cuda")      # guard rows around the children
    room = torch.full((P + 2, E), 0xEE, dtype=torch.uint8, device="cuda")
    assert dp.status() == 0
    dp.crossover_guided(dev(A), dev(B), rng, slot[1:P + 1], room[1:P + 1], order=dev(order), repair=True)
    s, r, g = host(slot), host(room), host(rng)
    assert dp.status() == BAD_ORDER
    assert (s[0] == 0xEE).all() and (s[-1] == 0xEE).all() and (r[0] == 0xEE).all() and (r[-1] == 0xEE).all()
    assert np.array_equal(g, [gm.advanced(x, E) for x in seeds])
    s, r = s[1:-1], r[1:-1]
    assert (s[:, lost] == 255).all() and (r[:, lost] == 255).all()
    ws, wg, _, _ = cm.guided_slots(inst, order, A, B, seeds, 1)
    assert np.array_equal(s, ws) and np.array_equal(g, wg)
    named = np.setdiff1d(np.arange(E), lost)
    assert s[:, named].max() < 45 and r[:, named].max() < inst.R
    dp.close()


# ---------------------------------------------------------------- genes >= 45
@pytest.mark.parametrize("name", ["sm", "E449"])
def test_parents_genes_of_45_and_more(name):
    inst = SHAPES[name]()
    dp = native.DeviceProblem(inst)
    order = gm.greedy_order(inst)
    A, B = parents_of(inst, None, "random", 4, base=55)
    A[:, 4], B[:, 9] = 45, 255                              # one side only
    A[1, 12], B[1, 12] = 200, 45                            # both sides, one row
    A[3, 0], B[3, 0] = 45, 45
    seeds = ttga.population_seeds(56, 4)
    for repair in (0, 1):
        s, r, g, c, n = gpu_cross(dp, A, B, seeds, repair)
        ws, wg, wc, wn = cm.guided_slots(inst, order, A, B, seeds, repair)
        assert np.array_equal(s, ws) and np.array_equal(g, wg) and np.array_equal(c, wc) and np.array_equal(n, wn)
        assert np.array_equal(r, host(dp.assign_rooms(dev(s))))
        if repair:
            assert s.max() < 45 and (c >= 0).all() and n[1] >= 1 and n[3] >= 1
        else:
            assert np.array_equal(s[:, 4], B[:, 4]) and np.array_equal(s[:, 9], A[:, 9])
            assert s[1, 12] in (200, 45) and s[3, 0] == 45 and r[1, 12] == 255 and r[3, 0] == 255
            assert c[1] == -1 and c[3] == -1 and c[0] >= 0 and c[2] >= 0
    assert dp.status() == 0                                 # no status bit for parents' genes
    dp.close()


# ---------------------------------------------------------------- breed
@pytest.fixture(scope="module")
def breed_pops(orc, problems):
    cache = {}

    def get(name):
        if name not in cache:
            inst, dp, order = problems(name)
            o = orc.problem(inst)
            s, r, _ = o.random_init(ttga.population_seeds(700, 48))
            pen = o.eval(s, r)[3]
            pen[5] = -1                                     # an invalid genome never wins a tournament
            cache[name] = (o, s, r, pen)
        return cache[name]
    return get


def gpu_breed(dp, s, r, pen, seeds, p_cross, p_mut, skip, repair=None):
    C = len(seeds)
    rng = dev(seeds)
    cs = torch.full((C, dp.E), 0xEE, dtype=torch.uint8, device="cuda")
    cr = torch.full((C, dp.E), 0xEE, dtype=torch.uint8, device="cuda")
    fl = torch.full((C,), 0xEE, dtype=torch.uint8, device="cuda")
    if repair is None:
        dp.ga_breed(dev(s), dev(r), dev(pen), rng, cs, cr, fl, p_cross, p_mut, skip)
        return host(cs), host(cr), host(fl), host(rng)
    cost = torch.full((C,), 12345, dtype=torch.int32, device="cuda")
    rep = torch.full((C,), 12345, dtype=torch.int32, device="cuda")
    dp.ga_breed_guided(dev(s), dev(r), dev(pen), rng, cs, cr, fl, p_cross, p_mut, skip, repair=repair, cost=cost,
                       repaired=rep)
    return host(cs), host(cr), host(fl), host(rng), host(cost), host(rep)


def check_breed(problems, breed_pops, name, C, repair, p_cross, p_mut, skip):
    inst, dp, order = problems(name)
    o, s, r, pen = breed_pops(name)
    seeds = ttga.population_seeds(9100, C)
    got = gpu_breed(dp, s, r, pen, seeds, p_cross, p_mut, skip, repair)
    want = cm.breed(inst, o, order, s, r, pen, seeds, p_cross, p_mut, skip, repair)
    for a, b, what in zip(got, want, ("slot", "room", "flags", "rng", "cost", "repaired")):
        assert np.array_equal(a, b), what
    uni = gpu_breed(dp, s, r, pen, seeds, p_cross, p_mut, skip)
    assert np.array_equal(got[2], uni[2])                   # the flags are tt_ga_breed's
    if p_mut == 0:
        assert np.array_equal(got[3], uni[3])               # and so are the streams
    same = (got[2] & 1) == 0                                # not crossed: tt_ga_breed's child
    assert np.array_equal(got[0][same], uni[0][same]) and np.array_equal(got[1][same], uni[1][same])
    assert np.array_equal(got[3][same], uni[3][same])
    assert (got[4][same] == 0).all() and (got[5][same] == 0).all()
    return got


@pytest.mark.parametrize("skip", [0, 1])
@pytest.mark.parametrize("C,repair", [(1, 1), (4, 0), (5, 1), (130, 0), (130, 1)])
@pytest.mark.parametrize("p_cross,p_mut", [(1.0, 0.0), (0.8, 0.5), (0.0, 1.0)])
def test_breed_vs_model(problems, breed_pops, p_cross, p_mut, C, repair, skip):
    got = check_breed(problems, breed_pops, "sm", C, repair, p_cross, p_mut, skip)
    if C == 130 and p_cross == 0.8:
        crossed = (got[2] & 1) != 0
        assert 0 < crossed.sum() < C and 0 < ((got[2] & 2) != 0).sum() < C


def test_breed_vs_model_lds_row_path(problems, breed_pops):
    check_breed(problems, breed_pops, "E449", 5, 1, 0.8, 0.5, 1)


# ---------------------------------------------------------------- limit, arguments
def test_limit():
    """Past tt_assign_rooms's limit (12,521 events at one room) both calls are
    refused with nothing launched: every buffer untouched."""
    E = 12522
    A = np.zeros((4, E), np.int32)
    A[0, :3] = 1
    inst = ttga.Instance(E=E, R=1, F=1, S=4, room_size=np.array([10], np.int32), student_events=A,
                         room_features=np.ones((1, 1), np.int32), event_features=np.zeros((E, 1), np.int32))
    dp = native.DeviceProblem(inst)
    order = dp.greedy_order()
    seeds = ttga.population_seeds(40, 3)
    pa = random_slots(ttga.population_seeds(41, 3), E)[0]
    rng = dev(seeds)
    bufs = [torch.full((3, E), 0xEE, dtype=torch.uint8, device="cuda") for _ in range(2)]
    outs = [torch.full((3,), 12345, dtype=torch.int32, device="cuda") for _ in range(2)]
    fl = torch.full((3,), 0xEE, dtype=torch.uint8, device="cuda")
    with pytest.raises(native.TTError, match="instance too large") as ei:
        dp.crossover_guided(dev(pa), dev(pa), rng, bufs[0], bufs[1], order=order, repair=True, cost=outs[0],
                            repaired=outs[1])
    assert ei.value.code == native.TT_ERR_LIMIT
    with pytest.raises(native.TTError, match="instance too large") as ei:
        dp.ga_breed_guided(dev(pa), dev(pa), torch.zeros(3, dtype=torch.int32, device="cuda"), rng, bufs[0], bufs[1], fl,
                           order=order, cost=outs[0], repaired=outs[1])
    assert ei.value.code == native.TT_ERR_LIMIT
    assert np.array_equal(host(rng), seeds) and (host(fl) == 0xEE).all()
    assert all((host(b) == 0xEE).all() for b in bufs) and all((host(t) == 12345).all() for t in outs)
    assert dp.status() == 0
    dp.close()


def test_invalid_arguments_launch_nothing(problems):
    inst, dp, _ = problems("sm")
    lib, h = dp.lib, dp.handle
    seeds = ttga.population_seeds(40, 3)
    rng, pa = dev(seeds), dev(random_slots(seeds, inst.E)[0])
    slot = torch.full((3, inst.E), 0xEE, dtype=torch.uint8, device="cuda")
    room = torch.full((3, inst.E), 0xEE, dtype=torch.uint8, device="cuda")
    order = dp.greedy_order()
    p = lambda t: t.data_ptr()                                # noqa: E731
    assert lib.tt_crossover_guided(h, p(pa), p(pa), None, p(rng), p(slot), p(room), 3, 1, None, None, None) == 1
    assert lib.tt_crossover_guided(h, p(pa), p(pa), p(order), p(rng), p(slot), p(room), -1, 1, None, None, None) == 1
    assert lib.tt_crossover_guided(h, p(pa), None, p(order), p(rng), p(slot), p(room), 3, 1, None, None, None) == 1
    pen = torch.zeros(3, dtype=torch.int32, device="cuda")
    fl = torch.full((3,), 0xEE, dtype=torch.uint8, device="cuda")
    dbl = __import__("ctypes").c_double
    assert lib.tt_ga_breed_guided(h, p(pa), p(pa), p(pen), 3, None, p(rng), 3, dbl(0.8), dbl(0.5), 1, 1, p(slot), p(room),
                                  p(fl), None, None, None) == 1
    assert lib.tt_ga_breed_guided(h, p(pa), p(pa), p(pen), 0, p(order), p(rng), 3, dbl(0.8), dbl(0.5), 1, 1, p(slot),
                                  p(room), p(fl), None, None, None) == 1
    assert np.array_equal(host(rng), seeds) and (host(slot) == 0xEE).all() and (host(room) == 0xEE).all()
    assert (host(fl) == 0xEE).all()
    # P = 0 / C = 0: TT_OK, nothing written
    dp.crossover_guided(pa[:0], pa[:0], rng[:0], slot[:0], room[:0], repair=True)
    dp.ga_breed_guided(pa, pa, pen, rng[:0], slot[:0], room[:0], fl[:0])
    assert np.array_equal(host(rng), seeds) and (host(slot) == 0xEE).all()
    # every output NULL: the rows are the same
    A, B = parents_of(inst, None, "random", 3, base=66)
    with_out = gpu_cross(dp, A, B, seeds, 1)
    without = gpu_cross(dp, A, B, seeds, 1, outputs=False)
    assert all(np.array_equal(a, b) for a, b in zip(with_out[:3], without[:3]))


# ---------------------------------------------------------------- the point
def test_guided_repair_children_violate_less_than_uniform(problems):
    """med, 64 children of clash-free greedy parents, the same parents and
    streams: the mean tt_eval hcv of the guided-repair children is below the
    uniform children's."""
    inst, dp, order = problems("med")
    A, B = parents_of(inst, order, "greedy", 64, base=100)
    assert (cm.shared_pairs(inst, A) == 0).all() and (cm.shared_pairs(inst, B) == 0).all()
    seeds = ttga.population_seeds(500, 64)
    s, r, _, c, n = gpu_cross(dp, A, B, seeds, 1)
    rng = dev(seeds)
    us, ur = torch.empty((64, inst.E), dtype=torch.uint8, device="cuda"), torch.empty((64, inst.E), dtype=torch.uint8,
                                                                                   device="cuda")
    dp.crossover(dev(A), dev(B), rng, us, ur)
    guided = host(dp.eval(dev(s), dev(r))[0]).astype(np.float64).mean()
    uniform = host(dp.eval(us, ur)[0]).astype(np.float64).mean()
    print("mean hcv: guided + repair", guided, "uniform", uniform, "mean cost", c.mean(), "mean repaired", n.mean())
    assert guided < uniform


# ---------------------------------------------------------------- Island
def new_pop(n, E):
    return {"slot": torch.zeros((n, E), dtype=torch.uint8, device="cuda"),
            "room": torch.zeros((n, E), dtype=torch.uint8, device="cuda"),
            "hcv": torch.zeros(n, dtype=torch.int32, device="cuda"), "scv": torch.zeros(n, dtype=torch.int32, device="cuda"),
            "feasible": torch.zeros(n, dtype=torch.uint8, device="cuda"),
            "penalty": torch.zeros(n, dtype=torch.int32, device="cuda")}


def explicit_run(dp, N, C, parts, gens, steps, seed, repair, lahc, unique):
    """Island(crossover="guided") as explicit calls on one stream: the initial
    population, then per sub-batch h its breed, the replacement of sub-batch
    h - parts + 1, its search (and walk); the pending ones replaced at the end.
    Returns the population and the sums of the breeds' outputs."""
    def search(rows, rng):
        dp.local_search(rows["slot"], rows["room"], rng, steps, out=(rows["hcv"], rows["scv"], rows["feasible"],
                                                                      rows["penalty"]))
        if lahc:
            dp.lahc(rows["slot"], rows["room"], rng, lahc, 500, 0.5, scv=rows["scv"], penalty=rows["penalty"])

    def replace(child, n):
        if unique:
            dp.ga_replace_unique(pop, child, dp.ga_unique_work(N, n))
        else:
            dp.ga_replace(pop, child, dp.ga_work(N))
    pop, rng_init = new_pop(N, dp.E), dev(stream_seeds(seed, 0, N))
    dp.random_init(rng_init, pop["slot"], pop["room"])
    search(pop, rng_init)
    replace(None, 0)
    child, rng_child = new_pop(C, dp.E), dev(stream_seeds(seed, N, C))
    flags = torch.zeros(C, dtype=torch.uint8, device="cuda")
    cost, rep = torch.zeros(C, dtype=torch.int32, device="cuda"), torch.zeros(C, dtype=torch.int32, device="cuda")
    bounds = [0] + [int(b) for b in np.cumsum([len(x) for x in np.array_split(np.arange(C), parts)])]
    views = [slice(bounds[j], bounds[j + 1]) for j in range(parts)]
    sums = dict(children=0, crossed=0, clean=0, cost=0, repaired=0)
    pending = []
    for h in range(gens * parts):
        v = views[h % parts]
        c = {k: t[v] for k, t in child.items()}
        dp.ga_breed_guided(pop["slot"], pop["room"], pop["penalty"], rng_child[v], c["slot"], c["room"], flags[v], 0.8,
                           0.5, True, repair=repair, cost=cost[v], repaired=rep[v])
        x, cc, rr = (host(flags[v]) & 1) != 0, host(cost[v]), host(rep[v])
        sums["children"] += len(x)
        sums["crossed"] += int(x.sum())
        sums["clean"] += int((x & (cc == 0)).sum())
        sums["cost"] += int(cc.sum())
        sums["repaired"] += int(rr.sum())
        if len(pending) >= parts - 1 and pending:
            pc, pn = pending.pop(0)
            replace(pc, pn)
        search(c, rng_child[v])
        pending.append((c, v.stop - v.start))
        if len(pending) >= parts:
            pc, pn = pending.pop(0)
            replace(pc, pn)
    while pending:
        pc, pn = pending.pop(0)
        replace(pc, pn)
    return pop, sums


VARIANTS = {"batch": {}, "staggered": dict(schedule="staggered", parts=2), "lahc_unique": dict(lahc=200, unique=True)}


@pytest.mark.parametrize("repair", [False, True])
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_island_guided_is_the_explicit_calls(problems, variant, repair):
    inst, dp, _ = problems("sm")
    kw = VARIANTS[variant]
    N, C, gens, steps, seed = 12, 4, 6, 50, 31
    isl = Island(dp, pop_size=N, children=C, max_steps=steps, seed=seed, crossover="guided", crossover_repair=repair,
                 **kw)
    isl.initialize()
    for _ in range(gens):
        isl.step()
    isl.flush()
    want, sums = explicit_run(dp, N, C, kw.get("parts", 1), gens, steps, seed, repair, kw.get("lahc", 0),
                              kw.get("unique", False))
    for k in want:
        assert np.array_equal(host(isl.pop[k]), host(want[k])), k
    st = isl.cx_stats()
    print(variant, repair, st)
    assert st == sums
    assert st["children"] == gens * C and 0 < st["crossed"] <= st["children"]
    assert (st["repaired"] > 0) == repair
    isl.close()
    assert dp.status() & BAD_ORDER == 0


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_island_uniform_issues_no_guided_call(problems, variant, monkeypatch):
    inst, dp, _ = problems("sm")
    kw = VARIANTS[variant]

    def run(**extra):
        isl = Island(dp, pop_size=12, children=4, max_steps=50, seed=31, **kw, **extra)
        isl.initialize()
        for _ in range(5):
            isl.step()
        isl.flush()
        return isl
    plain = run()

    def boom(*a, **k):
        raise AssertionError("guided breed called with Island(crossover='uniform')")
    monkeypatch.setattr(dp, "ga_breed_guided", boom)
    monkeypatch.setattr(dp, "crossover_guided", boom)
    off = run(crossover="uniform")
    for k in plain.pop:
        assert np.array_equal(host(off.pop[k]), host(plain.pop[k])), k
    with pytest.raises(ValueError, match="cx_stats"):
        off.cx_stats()
    off.close()
    plain.close()


# ---------------------------------------------------------------- the drivers
def test_crossover_guided_in_both_drivers(tmp_path):
    tim = REPO / "tests" / "golden" / "sm.tim"
    inst = ttga.read_tim(tim)
    base = ["-i", str(tim), "-s", "29", "-p", "1", "--pop", "16", "--children", "8", "--generations", "10",
            "--kempe", "0.5"]
    py, cc, a, lines = both_drivers(tmp_path, base, ["--crossover", "guided", "--crossover-repair"], "crossover", inst)
    cc_plain = run_driver([str(GA), *base, "--crossover", "uniform"], tmp_path)
    assert len(lines) == 1 and set(lines[0]) == {"children", "clean", "crossed", "meanCost", "repaired"}
    k = lines[0]
    assert k["children"] == 80 and 0 < k["crossed"] <= 80 and 0 <= k["clean"] <= k["crossed"] and k["repaired"] > 0
    kinds = [next(iter(x)) for x in a]
    assert kinds.index("crossover") == kinds.index("solution") + 1 == kinds.index("kempe") - 1
    assert not any("crossover" in x for x in json_lines(cc_plain.stdout))          # uniform: no call, no line
