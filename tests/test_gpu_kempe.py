"""The Kempe-chain move (include/ttga_kempe.h) on the GPU against
tests/kempe_model.py: slot rows, Random states and chain_len bit for bit, the
rooms of the two touched slots against the oracle's assign_rooms of the model's
new slot row and every other room unchanged; the gate, the cap, crowded slots,
invalid genes, chain_len = NULL, the limit, Island(kempe=...) and the two
drivers with --kempe."""
import pathlib
import subprocess

import numpy as np
import pytest

import ttga
import kempe_model as km
from helpers import dev, host, json_lines
from oracle_lib import oracle
from stage_checks import GA, both_drivers, run_driver

pytestmark = pytest.mark.gpu

import torch  # noqa: E402
from ttga import native  # noqa: E402
from ttga.ga import Island, new_population, stream_seeds  # noqa: E402

REPO = pathlib.Path(__file__).resolve().parent.parent
PKG = REPO / "timetabling-ga-mpi-openmp_amd"

# tt_device_status bits 0 and 2..6: clear unless a test says otherwise
STATUS_MASK = 0b1111101

# seeds: 1, the largest in-range state, 0 (the stream stays 0: the gate passes, event 0,
# t2 = 0 or 1), one above 2^31 (pm_next's out-of-range first step), and ordinary ones
SPECIAL_SEEDS = np.concatenate([np.array([1, 2147483646, 0, 3000000019], np.int64), ttga.population_seeds(9000, 12)])


def no_students(E, R):
    return ttga.Instance(E, R, 2, 0, np.full(R, 5), np.zeros((0, E)), np.ones((R, 2)), np.zeros((E, 2)))


SHAPES = {
    "sm": lambda: ttga.config_instance("sm"),
    "med": lambda: ttga.config_instance("med"),
    "E1": lambda: ttga.generate(1, 2, 2, 3, seed=3, min_att=1, max_att=1),     # the chain is {e}
    "E65": lambda: ttga.generate(65, 4, 3, 40, seed=7),                       # two bitset words, one bit in the last
    "E449": lambda: ttga.generate(449, 17, 5, 150, seed=13),                  # R = 17: the wide matcher path
    "S0": lambda: no_students(90, 4),                                         # no correlations: every chain is {e}
    # every student attends >= 40 % of the events: a chain is all of t1 and t2
    "dense": lambda: ttga.generate(120, 6, 3, 30, seed=21, min_att=48, max_att=60),
}


@pytest.fixture(scope="module")
def problems():
    cache = {}

    def get(name):
        if name not in cache:
            inst = SHAPES[name]()
            cache[name] = (inst, native.DeviceProblem(inst), oracle().problem(inst), km.neighbours(inst))
        return cache[name]
    return get


def gpu_move(dp, slot, room, seeds, prob, max_chain=0, with_len=True):
    P = len(seeds)
    s, r, g = dev(slot), dev(room), dev(seeds)
    cl = torch.full((P,), 12345, dtype=torch.int32, device="cuda") if with_len else None
    dp.kempe_move(s, r, g, prob, max_chain, cl)
    return host(s), host(r), host(g), host(cl) if with_len else None


def check(problem, slot, room, seeds, prob, max_chain=0, status=0):
    """One call against the model and the oracle; returns the model's output."""
    inst, dp, o, nb = problem
    s, r, g, cl = gpu_move(dp, slot, room, seeds, prob, max_chain)
    ws, wg, wl, pairs = km.kempe_rows(inst, slot, seeds, prob, max_chain, room=room, nb=nb)
    wr = km.expected_rooms(o, ws, room, wl, pairs)
    assert np.array_equal(cl, wl), f"chain_len differs in rows {np.flatnonzero(cl != wl)[:8]}"
    assert np.array_equal(s, ws), f"slot rows differ in {np.flatnonzero((s != ws).any(axis=1))[:8]}"
    assert np.array_equal(g, wg), f"rng states differ in {np.flatnonzero(g != wg)[:8]}"
    assert np.array_equal(r, wr), f"room rows differ in {np.flatnonzero((r != wr).any(axis=1))[:8]}"
    assert dp.status() & STATUS_MASK == status
    return ws, wg, wl, pairs


def random_rows(problem, seeds):
    """RandomInitialSolution rows with their rooms (the oracle's, bit-equal to
    tt_random_init's: tests/test_gpu_parity.py)."""
    s, r, _ = problem[2].random_init(seeds)
    return s, r


# ---------------------------------------------------------------- shapes
@pytest.mark.parametrize("name", list(SHAPES))
def test_shapes_vs_model(problems, name):
    pb = problems(name)
    inst = pb[0]
    slot, room = random_rows(pb, ttga.population_seeds(500, len(SPECIAL_SEEDS)))
    ws, wg, wl, pairs = check(pb, slot, room, SPECIAL_SEEDS, 1.0)
    assert (wl >= 1).all()                                   # prob = 1: every row moves
    assert wg.tolist() == [km.advanced(x, 3) for x in SPECIAL_SEEDS]
    if name in ("E1", "S0"):
        assert (wl == 1).all()                               # a Move1 to another slot
    if name == "dense":
        both = [int(((slot[i] == t1) | (slot[i] == t2)).sum()) for i, (t1, t2) in enumerate(pairs)]
        assert wl.tolist() == both and max(both) > 4
    if name in ("sm", "med", "E449"):
        assert len(set(wl.tolist())) > 2                     # chains of several lengths


# ---------------------------------------------------------------- populations
@pytest.mark.parametrize("P", [1, 64, 65, 130])
def test_population_sizes(problems, P):
    """Rows from tt_random_init itself."""
    pb = problems("med")
    inst, dp = pb[0], pb[1]
    slot = torch.empty((P, inst.E), dtype=torch.uint8, device="cuda")
    room = torch.empty_like(slot)
    dp.random_init(dev(ttga.population_seeds(700 + P, P)), slot, room)
    check(pb, host(slot), host(room), ttga.population_seeds(31000, P), 1.0)


def test_searched_rows(problems):
    """64 med rows after tt_greedy_init + tt_local_search(3000): mostly
    feasible, the case the GA feeds the move."""
    pb = problems("med")
    inst, dp = pb[0], pb[1]
    P = 64
    rng = dev(ttga.population_seeds(800, P))
    slot = torch.empty((P, inst.E), dtype=torch.uint8, device="cuda")
    room = torch.empty_like(slot)
    dp.greedy_init(rng, slot, room)
    dp.local_search(slot, room, rng, 3000)
    feasible = host(dp.eval(slot, room)[2])
    print("feasible rows:", int(feasible.sum()), "of", P)
    assert feasible.any()
    ws, _, wl, _ = check(pb, host(slot), host(room), ttga.population_seeds(32000, P), 1.0)
    # the correlated pairs stay zero: a feasible row loses feasibility to rooms only
    parts = host(dp.eval_parts(dev(ws), dp.assign_rooms(dev(ws))))
    assert (parts[feasible.astype(bool), 1] == 0).all()


def test_eval_parts_before_and_after(problems):
    pb = problems("med")
    inst, dp = pb[0], pb[1]
    P = 64
    slot, room = random_rows(pb, ttga.population_seeds(900, P))
    before = host(dp.eval_parts(dev(slot), dev(room)))
    s, r, _, cl = gpu_move(dp, slot, room, ttga.population_seeds(33000, P), 1.0)
    after = host(dp.eval_parts(dev(s), dev(r)))
    assert (before[:, 1] > 0).any()                           # random rows do have such pairs
    assert np.array_equal(before[:, 1], after[:, 1])          # TT_PART_CORR_PAIRS
    assert (cl >= 1).all() and np.array_equal(np.abs(cl), (s != slot).sum(axis=1))
    assert dp.status() & STATUS_MASK == 0


# ---------------------------------------------------------------- gate, cap
def test_gate(problems):
    pb = problems("med")
    P = 130
    slot, room = random_rows(pb, ttga.population_seeds(1000, P))
    # the first draw of seed s < 127,773 is s / 127,773: seeds 1000 apart cover [0, 1)
    seeds = 1000 * np.arange(1, P + 1, dtype=np.int64)
    _, wg, wl, _ = check(pb, slot, room, seeds, 0.0)
    assert not wl.any() and wg.tolist() == [km.advanced(x, 1) for x in seeds]
    s, r, g, cl = gpu_move(pb[1], slot, room, seeds, 0.0)
    assert np.array_equal(s, slot) and np.array_equal(r, room)
    _, wg, wl, _ = check(pb, slot, room, seeds, 0.5)
    moved = wl > 0
    assert 30 <= moved.sum() <= 100                           # both outcomes, as the model has them
    assert all(wg[i] == km.advanced(seeds[i], 3 if moved[i] else 1) for i in range(P))


def test_cap(problems):
    """max_chain = 4 on 130 random med rows, move seeds 35000.. (chosen on the CPU:
    the model applies 19 of them and rejects 111; about 14 % of uniformly random
    med chains have at most 4 events)."""
    pb = problems("med")
    P = 130
    slot, room = random_rows(pb, ttga.population_seeds(1100, P))
    seeds = ttga.population_seeds(35000, P)
    ws, wg, wl, _ = check(pb, slot, room, seeds, 1.0, max_chain=4)
    applied, rejected = wl > 0, wl < 0
    print("applied", int(applied.sum()), "rejected", int(rejected.sum()))
    assert applied.sum() >= 8 and rejected.sum() >= 8 and (applied | rejected).all()
    assert (wl[applied] <= 4).all() and (wl[rejected] < -4).all()
    assert np.array_equal(ws[rejected], slot[rejected])
    assert wg.tolist() == [km.advanced(x, 3) for x in seeds]


# ---------------------------------------------------------------- crowded slots
def test_crowded_slots(problems):
    """150 events in each of two slots, the rest at random: chains of up to 300
    events, and the re-match of a slot of 65..256 events (one lane, tt_match.h)."""
    pb = problems("med")
    inst, dp, o, nb = pb
    P = 24
    rs = np.random.default_rng(5)
    slot = rs.integers(0, 45, size=(P, inst.E)).astype(np.uint8)
    for i in range(P):
        a, b = rs.choice(45, size=2, replace=False)
        ev = rs.permutation(inst.E)
        slot[i, ev[:150]] = a
        slot[i, ev[150:300]] = b
    room = o.assign_rooms(slot)
    seeds = ttga.population_seeds(36000, P)
    ws, _, wl, _ = check(pb, slot, room, seeds, 1.0)
    assert wl.max() > 64                                     # long chains did occur
    sizes = np.stack([np.bincount(row, minlength=45) for row in ws])
    assert sizes.max() <= 256 and (sizes > 64).any()


# ---------------------------------------------------------------- invalid genes, NULL, limit
def test_invalid_genes():
    """Rows with a slot gene 45 and rows with a room gene R among valid ones:
    untouched with their streams, chain_len 0, status bit 6. Own handle: the
    status word is sticky."""
    inst = SHAPES["sm"]()
    pb = (inst, native.DeviceProblem(inst), oracle().problem(inst), km.neighbours(inst))
    P = 12
    slot, room = random_rows(pb, ttga.population_seeds(1200, P))
    slot[2, 7] = 45
    slot[9, inst.E - 1] = 255
    room[4, 0] = inst.R
    room[7, 50] = 255
    bad = [2, 4, 7, 9]
    seeds = ttga.population_seeds(37000, P)
    assert pb[1].status() == 0
    ws, wg, wl, _ = check(pb, slot, room, seeds, 1.0, status=64)
    assert pb[1].status() == 64
    assert not wl[bad].any() and np.array_equal(wg[bad], seeds[bad]) and np.array_equal(ws[bad], slot[bad])
    good = np.setdiff1d(np.arange(P), bad)
    assert (wl[good] >= 1).all()
    pb[1].close()


def test_chain_len_null(problems):
    pb = problems("sm")
    P = 40
    slot, room = random_rows(pb, ttga.population_seeds(1300, P))
    seeds = 3000 * np.arange(1, P + 1, dtype=np.int64)      # first draws spread over [0, 1)
    for prob, cap in ((1.0, 0), (0.5, 3)):
        a = gpu_move(pb[1], slot, room, seeds, prob, cap)
        b = gpu_move(pb[1], slot, room, seeds, prob, cap, with_len=False)
        assert all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3]))
        assert not np.array_equal(a[0], slot)
    assert pb[1].status() & STATUS_MASK == 0


def test_limit():
    """The documented limit at R = 10 is E <= 12,108: 12,109 is refused with
    nothing launched (every buffer untouched), 12,108 runs. A handful of
    students keeps the instances cheap; about 269 events per slot is past the
    matcher's 256, so status bit 0 is expected there (ttga.h "Limits")."""
    def make(E):
        A = np.zeros((4, E), np.int32)
        A[0, :3] = 1
        return ttga.Instance(E=E, R=10, F=1, S=4, room_size=np.full(10, 10, np.int32), student_events=A,
                             room_features=np.ones((10, 1), np.int32), event_features=np.zeros((E, 1), np.int32))
    P = 3
    seeds = ttga.population_seeds(40, P)
    dp = native.DeviceProblem(make(12109))
    rng = dev(seeds)
    slot = torch.full((P, dp.E), 7, dtype=torch.uint8, device="cuda")
    room = torch.full((P, dp.E), 1, dtype=torch.uint8, device="cuda")
    cl = torch.full((P,), 12345, dtype=torch.int32, device="cuda")
    with pytest.raises(native.TTError, match="instance too large") as ei:
        dp.kempe_move(slot, room, rng, 1.0, 0, cl)
    assert ei.value.code == native.TT_ERR_LIMIT
    assert np.array_equal(host(rng), seeds) and (host(cl) == 12345).all()
    assert (host(slot) == 7).all() and (host(room) == 1).all()
    assert dp.status() == 0
    dp.close()

    dp = native.DeviceProblem(make(12108))
    rs = np.random.default_rng(3)
    before = rs.integers(0, 45, size=(P, dp.E)).astype(np.uint8)
    s, r, g, c = gpu_move(dp, before, np.zeros_like(before), seeds, 1.0)
    assert g.tolist() == [km.advanced(x, 3) for x in seeds]
    assert (c >= 1).all() and np.array_equal(c, (s != before).sum(axis=1))
    assert dp.status() & STATUS_MASK & ~1 == 0
    dp.close()


# ---------------------------------------------------------------- Island
def test_island_against_explicit_calls(problems):
    """Island(kempe=0.5): ga_breed, kempe_move, local_search with fused
    evaluation, ga_replace per generation, field for field; kempe_stats() is the
    sum over that run's chain_len."""
    inst, dp, _, _ = problems("sm")
    N, C, seed, steps, gens = 16, 8, 23, 50, 3
    isl = Island(dp, pop_size=N, children=C, max_steps=steps, seed=seed, kempe=0.5)
    plain = Island(dp, pop_size=N, children=C, max_steps=steps, seed=seed)
    with pytest.raises(ValueError, match="kempe_stats"):
        plain.kempe_stats()
    for i in (isl, plain):
        i.initialize()
        for _ in range(gens):
            i.step()
    # the explicit run
    pop, child = new_population(N, inst.E, "cuda"), new_population(C, inst.E, "cuda")
    rng_init, rng_child = dev(stream_seeds(seed, 0, N)), dev(stream_seeds(seed, N, C))
    flags = torch.zeros(C, dtype=torch.uint8, device="cuda")
    chain = torch.zeros(C, dtype=torch.int32, device="cuda")
    work = dp.ga_work(N)
    out = lambda p: (p["hcv"], p["scv"], p["feasible"], p["penalty"])    # noqa: E731
    dp.random_init(rng_init, pop["slot"], pop["room"])
    dp.local_search(pop["slot"], pop["room"], rng_init, steps, out=out(pop))
    dp.ga_replace(pop, None, work)
    lens = []
    for _ in range(gens):
        dp.ga_breed(pop["slot"], pop["room"], pop["penalty"], rng_child, child["slot"], child["room"], flags)
        dp.kempe_move(child["slot"], child["room"], rng_child, 0.5, 0, chain)
        lens.append(host(chain).copy())
        dp.local_search(child["slot"], child["room"], rng_child, steps, out=out(child))
        dp.ga_replace(pop, child, work)
    for k in pop:
        assert np.array_equal(host(isl.pop[k]), host(pop[k])), k
    assert np.array_equal(host(isl.rng_child), host(rng_child))
    lens = np.concatenate(lens)
    assert isl.kempe_stats() == {"children": gens * C, "moved": int((lens > 0).sum()), "rejected": 0,
                                 "chain_events": int(lens[lens > 0].sum())}
    assert 0 < (lens > 0).sum() < gens * C
    assert not np.array_equal(host(plain.pop["slot"]), host(pop["slot"]))     # the move did change the run
    isl.close()
    plain.close()
    assert dp.status() & STATUS_MASK == 0


# ---------------------------------------------------------------- the drivers
def test_kempe_in_both_drivers(tmp_path, problems):
    inst = problems("sm")[0]
    tim = tmp_path / "sm.tim"
    ttga.write_tim(inst, tim)
    base = ["-i", str(tim), "-s", "29", "-p", "1", "--pop", "16", "--children", "8", "--generations", "10"]
    py, cc, a, kempe = both_drivers(tmp_path, base, ["--kempe", "0.5", "--kempe-max-chain", "8"], "kempe", inst)
    cc_zero = run_driver([str(GA), *base, "--kempe", "0"], tmp_path)
    assert len(kempe) == 1 and set(kempe[0]) == {"children", "moved", "rejected", "meanChain"}
    k = kempe[0]
    assert k["children"] == 80 and 0 < k["moved"] and 0 <= k["rejected"] and k["moved"] + k["rejected"] < 80
    assert 1 <= k["meanChain"] <= 8
    kinds = [next(iter(x)) for x in a]
    assert kinds[kinds.index("kempe") - 1] == "solution"      # after its island's solution line
    assert not any("kempe" in x for x in json_lines(cc_zero.stdout))     # probability 0: no call, no line
    for r_ in (py, cc):
        out = subprocess.run([str(PKG / "ttga-check"), str(tim), "-"], input=r_.stdout, capture_output=True, text=True,
                             timeout=60)
        assert out.returncode == 0, out.stdout
