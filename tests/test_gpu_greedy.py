"""The greedy constructive initial population (include/ttga_greedy.h) on the GPU
against tests/greedy_model.py: the event order, slot rows, room rows (the
model's slots through the oracle's assign_rooms) and final Random states bit
for bit; the replay check (no RNG) on the GPU's own rows; the limit and an
invalid order; Island(init="greedy"); its effect on the local search; and the
two drivers with --init greedy."""
import pathlib
import subprocess
import sys

import numpy as np
import pytest

import ttga
import greedy_model as gm
from helpers import dev, host, json_lines
from oracle_lib import oracle
from stage_checks import GA, both_drivers, run_driver

pytestmark = pytest.mark.gpu

import torch  # noqa: E402
from ttga import native  # noqa: E402
from ttga.ga import Island, stream_seeds  # noqa: E402

REPO = pathlib.Path(__file__).resolve().parent.parent
PKG = REPO / "timetabling-ga-mpi-openmp_amd"

# seeds: 1, the largest in-range state, 0 (the stream stays 0: every pick is the first
# tie), one above 2^31 (pm_next's out-of-range first step), and ordinary ones
SPECIAL_SEEDS = np.array([1, 2147483646, 0, 3000000019, 1000, 1001], np.int64)

# name -> the instance; E: fewer events than slots, the bitset word edges, both sides of
# the register/LDS split (448 | 449), a wider one; R = 1 (the full-slot term decides from
# the second event in a slot) and R = 64
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
    "ties": lambda: ttga.generate(130, 3, 2, 4),      # four students: many events with equal keys
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


def gpu_init(dp, seeds, order=None):
    P = len(seeds)
    rng = dev(seeds)
    slot = torch.full((P, dp.E), 0xEE, dtype=torch.uint8, device="cuda")
    room = torch.full((P, dp.E), 0xEE, dtype=torch.uint8, device="cuda")
    dp.greedy_init(rng, slot, room, order=order)
    return host(slot), host(room), host(rng)


# ---------------------------------------------------------------- order
@pytest.mark.parametrize("name", ["sm", "med", "ties", "E1", "E449"])
def test_order_vs_model(problems, name):
    inst, dp, want = problems(name)
    got = host(dp.greedy_order())
    assert got.dtype == np.int32 and np.array_equal(got, want)
    if name == "ties":
        key = gm.greedy_keys(inst)
        assert len(np.unique(key)) < inst.E // 2        # the index tie-break is exercised
    assert dp.greedy_order() is dp.greedy_order()       # computed once
    assert dp.status() == 0


# ---------------------------------------------------------------- bit-exact
def check_exact(orc, problems, name, seeds):
    inst, dp, order = problems(name)
    s, r, g = gpu_init(dp, seeds)
    ws, wg = gm.greedy_slots(inst, order, seeds)
    assert np.array_equal(s, ws), f"{name}: slot rows differ in {np.flatnonzero((s != ws).any(axis=1))[:8]}"
    assert np.array_equal(g, wg)
    assert np.array_equal(g, [gm.advanced(x, inst.E) for x in seeds])
    assert np.array_equal(r, orc.problem(inst).assign_rooms(ws))
    assert dp.status() == 0
    return s


@pytest.mark.parametrize("name", [n for n in SHAPES if n != "ties"])
def test_bit_exact_shapes(orc, problems, name):
    check_exact(orc, problems, name, SPECIAL_SEEDS)


@pytest.mark.parametrize("P", [1, 64, 65, 130])
def test_bit_exact_population_sizes(orc, problems, P):
    """P = 65 and 130 end in a partial workgroup (four individuals per workgroup
    at E <= 448)."""
    check_exact(orc, problems, "sm", ttga.population_seeds(31000, P))


def test_bit_exact_wide_partial_population(orc, problems):
    check_exact(orc, problems, "E449", ttga.population_seeds(32000, 67))


# ---------------------------------------------------------------- replay, diversity
@pytest.mark.parametrize("name", ["med", "E449"])
def test_replay_of_gpu_rows(problems, name):
    """Independent of the model's RNG: every event of a GPU row sits in a slot
    that had minimum cost when it was placed, in the GPU's own order."""
    inst, dp, _ = problems(name)
    order = host(dp.greedy_order())
    s, _, _ = gpu_init(dp, ttga.population_seeds(77, 4))
    for row in s:
        gm.replay_check(inst, order, row)


def test_diversity_med(problems):
    inst, dp, _ = problems("med")
    s, _, _ = gpu_init(dp, ttga.population_seeds(5000, 64))
    assert len({row.tobytes() for row in s}) == 64
    assert dp.status() == 0


def test_caller_order(orc, problems):
    """Any permutation is a valid order: the events by index."""
    inst, dp, _ = problems("sm")
    order = np.arange(inst.E, dtype=np.int32)
    seeds = ttga.population_seeds(9, 5)
    s, r, g = gpu_init(dp, seeds, order=dev(order))
    ws, wg = gm.greedy_slots(inst, order, seeds)
    assert np.array_equal(s, ws) and np.array_equal(g, wg)
    assert np.array_equal(r, orc.problem(inst).assign_rooms(ws))


# ---------------------------------------------------------------- limit, invalid order
def test_limit(problems):
    """The documented limit is tt_assign_rooms's: 12,521 events at one room. The
    first E past it is refused with nothing launched (rng and the rows
    untouched); 12,521 itself runs. A handful of students keeps the instance
    cheap (a fraction of a second)."""
    def make(E):
        A = np.zeros((4, E), np.int32)
        A[0, :3] = 1
        return ttga.Instance(E=E, R=1, F=1, S=4, room_size=np.array([10], np.int32), student_events=A,
                             room_features=np.ones((1, 1), np.int32), event_features=np.zeros((E, 1), np.int32))
    seeds = ttga.population_seeds(40, 3)
    dp = native.DeviceProblem(make(12522))
    order = dp.greedy_order()
    torch.cuda.synchronize()
    rng = dev(seeds)
    slot = torch.full((3, dp.E), 0xEE, dtype=torch.uint8, device="cuda")
    room = torch.full((3, dp.E), 0xEE, dtype=torch.uint8, device="cuda")
    with pytest.raises(native.TTError, match="instance too large") as ei:
        dp.greedy_init(rng, slot, room, order=order)
    assert ei.value.code == native.TT_ERR_LIMIT
    with pytest.raises(native.TTError) as ei:
        dp.assign_rooms(slot, room)                          # not tighter than the matcher's own
    assert ei.value.code == native.TT_ERR_LIMIT
    assert np.array_equal(host(rng), seeds)
    assert (host(slot) == 0xEE).all() and (host(room) == 0xEE).all()
    assert dp.status() == 0
    dp.close()

    dp = native.DeviceProblem(make(12521))
    s, r, g = gpu_init(dp, seeds)
    assert s.max() < 45
    # one room: a slot is full with its first event, so the first 45 events of the order
    # take 45 different slots (after that every slot costs 1 and the draw alone decides)
    first = host(dp.greedy_order())[:45]
    assert first[:3].tolist() == [0, 1, 2]                   # the only correlated events
    assert all(len(set(row[first].tolist())) == 45 for row in s)
    # about 278 events per slot: most are past the matcher's 256 (ttga.h "Limits"), which writes
    # such rooms as 255 and reports it; the rooms are tt_assign_rooms's all the same
    assert np.array_equal(r, host(dp.assign_rooms(dev(s))))
    assert dp.status() == 1
    dp.close()


@pytest.mark.parametrize("name", ["sm", "E449"])
def test_invalid_order(orc, problems, name):
    """Entries outside 0..E-1 are skipped with their draw consumed, status bit 5
    is set, the events nobody names keep slot and room 255, and nothing is
    written outside the rows. Own handles: the status word is sticky."""
    inst = SHAPES[name]()
    dp = native.DeviceProblem(inst)
    E, P = inst.E, 5
    order = gm.greedy_order(inst).copy()
    lost = [int(order[3]), int(order[E // 2]), int(order[E - 1])]
    order[3], order[E // 2], order[E - 1] = -1, E, 2 ** 31 - 1
    seeds = ttga.population_seeds(600, P)
    rng = dev(seeds)
    # guard rows around the population
    slot = torch.full((P + 2, E), 0xEE, dtype=torch.uint8, device="cuda")
    room = torch.full((P + 2, E), 0xEE, dtype=torch.uint8, device="cuda")
    dp.greedy_init(rng, slot[1:P + 1], room[1:P + 1], order=dev(order))
    s, r, g = host(slot), host(room), host(rng)
    assert dp.status() == 32
    assert (s[0] == 0xEE).all() and (s[-1] == 0xEE).all() and (r[0] == 0xEE).all() and (r[-1] == 0xEE).all()
    assert np.array_equal(g, [gm.advanced(x, E) for x in seeds])
    s, r = s[1:-1], r[1:-1]
    assert (s[:, lost] == 255).all() and (r[:, lost] == 255).all()
    named = np.setdiff1d(np.arange(E), lost)
    assert s[:, named].max() < 45 and r[:, named].max() < inst.R
    hcv = host(dp.eval(dev(s), dev(r))[0])
    assert (hcv == -1).all()                                 # an invalid genome, as ttga.h documents
    dp.close()


# ---------------------------------------------------------------- Island
def explicit_population(dp, N, seed, steps, greedy, unique):
    rng = dev(stream_seeds(seed, 0, N))
    pop = {"slot": torch.zeros((N, dp.E), dtype=torch.uint8, device="cuda"),
           "room": torch.zeros((N, dp.E), dtype=torch.uint8, device="cuda"),
           "hcv": torch.zeros(N, dtype=torch.int32, device="cuda"), "scv": torch.zeros(N, dtype=torch.int32, device="cuda"),
           "feasible": torch.zeros(N, dtype=torch.uint8, device="cuda"),
           "penalty": torch.zeros(N, dtype=torch.int32, device="cuda")}
    if greedy:
        dp.greedy_init(rng, pop["slot"], pop["room"])
    else:
        dp.random_init(rng, pop["slot"], pop["room"])
    dp.local_search(pop["slot"], pop["room"], rng, steps, out=(pop["hcv"], pop["scv"], pop["feasible"], pop["penalty"]))
    if unique:
        dp.ga_replace_unique(pop, None, dp.ga_unique_work(N, 0))
    else:
        dp.ga_replace(pop, None, dp.ga_work(N))
    return pop, rng


@pytest.mark.parametrize("unique", [False, True])
@pytest.mark.parametrize("init", ["greedy", "random", None])
def test_island_initialize(problems, init, unique):
    """Island(init="greedy").initialize() is greedy_init, local_search with fused
    evaluation, ga_replace, field for field; the default (and "random") is still
    the random_init sequence."""
    inst, dp, _ = problems("sm")
    N, seed, steps = 24, 17, 50
    kw = {} if init is None else {"init": init}
    isl = Island(dp, pop_size=N, children=4, max_steps=steps, seed=seed, unique=unique, **kw)
    assert isl.init == (init or "random")
    isl.initialize()
    want, wrng = explicit_population(dp, N, seed, steps, init == "greedy", unique)
    for k in want:
        assert np.array_equal(host(isl.pop[k]), host(want[k])), k
    assert np.array_equal(host(isl.rng_init), host(wrng))
    other, _ = explicit_population(dp, N, seed, steps, init != "greedy", unique)
    assert not np.array_equal(host(other["slot"]), host(want["slot"]))
    isl.step()                                               # breeding goes on from either start
    assert isl.member_meta(0)[3] <= int(host(want["penalty"])[0])
    isl.close()
    assert dp.status() == 0


def test_island_rejects_bad_init_on_device(problems):
    inst, dp, _ = problems("sm")
    with pytest.raises(ValueError, match="init"):
        Island(dp, pop_size=8, children=2, init="best")


# ---------------------------------------------------------------- effect
def test_greedy_start_makes_the_search_feasible(orc):
    """comp01, 16 rows, local_search(200): strictly more rows end feasible from
    the greedy start than from the random one (the oracle's search gives 12
    against 0 from the same rows and seeds; the GPU search is bit-exact with it)."""
    inst = ttga.config_instance("comp01")
    dp = native.DeviceProblem(inst)
    P = 16
    seeds, ls_seeds = ttga.population_seeds(1000, P), ttga.population_seeds(2000, P)
    feasible = {}
    for kind in ("greedy", "random"):
        rng = dev(seeds)
        slot = torch.empty((P, inst.E), dtype=torch.uint8, device="cuda")
        room = torch.empty_like(slot)
        getattr(dp, kind + "_init")(rng, slot, room)
        out = tuple(torch.empty(P, dtype=dt, device="cuda") for dt in (torch.int32, torch.int32, torch.uint8, torch.int32))
        dp.local_search(slot, room, dev(ls_seeds), 200, out=out)
        feasible[kind] = int(host(out[2]).sum())
    print("feasible after local_search(200):", feasible)
    assert feasible["greedy"] > feasible["random"]
    assert dp.status() == 0
    dp.close()


# ---------------------------------------------------------------- the drivers
def test_init_greedy_in_both_drivers(tmp_path, problems):
    inst, dp, _ = problems("sm")
    tim = tmp_path / "sm.tim"
    ttga.write_tim(inst, tim)
    base = ["-i", str(tim), "-s", "29", "-p", "1", "--pop", "16", "--children", "8", "--generations", "10"]
    py, cc, a, _ = both_drivers(tmp_path, base, ["--init", "greedy"], None, inst)       # the stage prints no line
    py_plain = run_driver([sys.executable, "-m", "ttga.islands", *base], tmp_path)
    cc_plain = run_driver([str(GA), *base], tmp_path)
    cc_random = run_driver([str(GA), *base, "--init", "random"], tmp_path)
    plain = json_lines(py_plain.stdout)
    assert plain == json_lines(cc_plain.stdout) == json_lines(cc_random.stdout)
    assert a != plain                                        # another initial population
    # the first logEntry is the initial population's best: the model's rows, searched by the oracle
    o = oracle().problem(inst)
    seeds = stream_seeds(29, 0, 16)
    ws, _ = gm.greedy_slots(inst, gm.greedy_order(inst), seeds)
    s, r, _ = o.local_search(ws, o.assign_rooms(ws), np.array([gm.advanced(x, inst.E) for x in seeds], np.int64), 200)
    h, sc, f, pen = o.eval(s, r)
    k = int(np.argmin(pen.astype(np.uint32)))
    first = [x["logEntry"] for x in a if "logEntry" in x][0]
    assert first["best"] == (int(sc[k]) if f[k] else int(h[k]) * 1000000 + int(sc[k]))
    for r_ in (py, cc):
        out = subprocess.run([str(PKG / "ttga-check"), str(tim), "-"], input=r_.stdout, capture_output=True, text=True,
                             timeout=60)
        assert out.returncode == 0, out.stdout
