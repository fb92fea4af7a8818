"""Duplicate-free replacement on the GPU (include/ttga_unique.h) against numpy
and the CPU oracle, all comparisons exact: tt_genome_first (the first
occurrence of every genome), tt_ga_replace_unique (children already in the
population dropped, the rest replaced as tt_ga_replace does), Island(unique=True)
over whole generations in both schedules, and --unique in both drivers.

The expected values share no code with the kernels: the first occurrences come
from numpy.unique over the concatenated rows, the keep rule from those, the
replacement from the oracle's ga_replace with the kept children."""
import sys

import numpy as np
import pytest

import ttga
from helpers import dev, host, json_lines as _json_lines, oracle_population
from oracle_lib import oracle
from stage_checks import GA, both_drivers, run_driver, stage_lines

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
from ttga import native  # noqa: E402
from ttga.ga import Island, stream_seeds  # noqa: E402

KEYS = ("slot", "room", "hcv", "scv", "feasible", "penalty")


# ------------------------------------------------------------------ numpy side
def np_first(slot, room):
    """first[i] = the lowest j whose concatenated row equals i's."""
    g = np.concatenate([slot, room], axis=1)
    _, idx, inv = np.unique(g, axis=0, return_index=True, return_inverse=True)
    return idx[np.asarray(inv).ravel()].astype(np.int32)


def np_keep(pop, ch):
    """Child c is kept unless its genome equals a member's or a lower child's."""
    N = pop["slot"].shape[0]
    first = np_first(np.concatenate([pop["slot"], ch["slot"]]), np.concatenate([pop["room"], ch["room"]]))
    return first[N:] == np.arange(N, N + ch["slot"].shape[0])


def np_source(pop, ch, keep):
    """Where the new pop[0] comes from: a survivor's position p, or N + c."""
    N, D = pop["penalty"].shape[0], int(keep.sum())
    pen = np.concatenate([pop["penalty"][:N - D], ch["penalty"][keep]]).astype(np.uint32)
    src = np.concatenate([np.arange(N - D), N + np.flatnonzero(keep)])
    return int(src[np.lexsort((np.arange(pen.size), pen))[0]])


def model_replace(o, pop, ch):
    """The oracle's ga_replace with the kept children; (new pop, children dropped)."""
    keep = np_keep(pop, ch)
    return o.ga_replace(pop, {k: v[keep] for k, v in ch.items()}), int((~keep).sum())


def distinct(pop):
    return int((np_first(pop["slot"], pop["room"]) == np.arange(pop["slot"].shape[0])).sum())


# ------------------------------------------------------------ tt_genome_first
SHAPES = {"E1": (1, 5), "E63": (63, 5), "E64": (64, 5), "E65": (65, 5), "E100": (100, 5), "E449": (449, 5),
          "E100R64": (100, 64)}


@pytest.fixture(scope="module")
def problems():
    cache = {}

    def get(name):
        if name not in cache:
            E, R = SHAPES[name]
            inst = ttga.generate(E, R, 2, 10, seed=3)
            cache[name] = (inst, native.DeviceProblem(inst))
        return cache[name]
    return get


def planted_rows(rng, P, E, R):
    """Random rows with the planted cases; returns slot, room and the planted
    classes as {name: [(row, earlier row it is derived from)]}."""
    slot = rng.integers(0, 45, (P, E), dtype=np.uint8)
    room = rng.integers(0, R, (P, E), dtype=np.uint8)
    planted = {}
    if P < 40:
        if P >= 2:                                  # tiny populations: one copy
            slot[P - 1], room[P - 1] = slot[0], room[0]
            planted["copy"] = [(P - 1, 0)]
        return slot, room, planted
    rows = iter(rng.permutation(np.arange(20, P))[:16].tolist())

    def derive(name, src, edit=None):
        i = next(rows)
        slot[i], room[i] = slot[src], room[src]
        if edit:
            edit(i)
        planted.setdefault(name, []).append((i, src))
        return i
    c1 = derive("copy", 3)
    c2 = derive("copy", c1)                         # a copy of a copy
    derive("copy", c2)
    derive("copy", 0)

    def bump(a, k, mod):
        a[k] = (int(a[k]) + 1) % mod
    derive("first_slot", 5, lambda i: bump(slot[i], 0, 45))
    derive("room_byte", 7, lambda i: bump(room[i], E // 2, R))
    if E >= 2:
        derive("last_slot", 6, lambda i: bump(slot[i], E - 1, 45))

        def swap(i):
            a, b = 0, E - 1
            if slot[i][a] == slot[i][b]:
                slot[i][b] = (int(slot[i][b]) + 1) % 45
                slot[8][b] = slot[i][b]
            slot[i][a], slot[i][b] = slot[i][b], slot[i][a]
        derive("swap", 8, swap)
    # a row whose slot row is another's room row and vice versa (values valid in both)
    slot[9] = rng.integers(0, R, E, dtype=np.uint8)
    slot[9][0], room[9][0] = 1, 0                   # the two rows of row 9 differ
    i = next(rows)
    slot[i], room[i] = room[9].copy(), slot[9].copy()
    planted["crossed"] = [(i, 9)]
    return slot, room, planted


def check_planted(slot, room, planted, first, E):
    g = np.concatenate([slot, room], axis=1)
    for i, src in planted.get("copy", []):
        assert np.array_equal(g[i], g[src]) and first[i] == first[src] and first[i] < i
    for name in ("first_slot", "last_slot", "room_byte", "swap"):
        for i, src in planted.get(name, []):
            assert int((g[i] != g[src]).sum()) == (2 if name == "swap" else 1), name
            assert first[i] != first[src], name
    for i, src in planted.get("swap", []):
        assert sorted(slot[i]) == sorted(slot[src]) and not np.array_equal(slot[i], slot[src])
    for i, src in planted.get("crossed", []):
        assert np.array_equal(slot[i], room[src]) and np.array_equal(room[i], slot[src])
        assert first[i] != first[src]
    want = {"copy"} if len(slot) < 40 else ({"copy", "first_slot", "room_byte", "crossed"}
                                            | ({"last_slot", "swap"} if E >= 2 else set()))
    assert (set(planted) == want) if len(slot) >= 2 else not planted


@pytest.mark.parametrize("shape", list(SHAPES))
def test_genome_first_vs_numpy(problems, shape):
    """Every population with hash_bits 0, 8 and 1: the same first occurrences
    whether a run of equal hashes holds one genome or half the population."""
    inst, dp = problems(shape)
    rng = np.random.default_rng(inst.E * 100 + inst.R)
    for P in (1, 2, 5, 300, 1000) + ((9000,) if shape == "E65" else ()):
        slot, room, planted = planted_rows(rng, P, inst.E, inst.R)
        exp = np_first(slot, room)
        check_planted(slot, room, planted, exp, inst.E)
        gs, gr = dev(slot), dev(room)
        for bits in (0, 8, 1):
            got = host(dp.genome_first(gs, gr, hash_bits=bits))
            assert np.array_equal(got, exp), (P, bits, np.flatnonzero(got != exp)[:8])
    assert dp.status() == 0


def test_genome_first_identical_and_pairs(problems):
    inst, dp = problems("E100")
    rng = np.random.default_rng(4)
    one_s, one_r = rng.integers(0, 45, inst.E, dtype=np.uint8), rng.integers(0, inst.R, inst.E, dtype=np.uint8)
    slot, room = np.tile(one_s, (4096, 1)), np.tile(one_r, (4096, 1))
    assert not host(dp.genome_first(dev(slot), dev(room))).any()
    s = rng.integers(0, 45, (2048, inst.E), dtype=np.uint8)
    r = rng.integers(0, inst.R, (2048, inst.E), dtype=np.uint8)
    order = rng.permutation(np.tile(np.arange(2048), 2))
    slot, room = s[order], r[order]
    exp = np_first(slot, room)
    assert int((exp == np.arange(4096)).sum()) == 2048
    for bits in (0, 1):
        assert np.array_equal(host(dp.genome_first(dev(slot), dev(room), hash_bits=bits)), exp), bits
    empty = torch.empty((0, inst.E), dtype=torch.uint8, device="cuda")
    assert dp.genome_first(empty, empty).numel() == 0


# ------------------------------------------------------ tt_ga_replace_unique
@pytest.fixture(scope="module")
def e20():
    inst = ttga.generate(20, 5, 2, 10, seed=3)
    return inst, native.DeviceProblem(inst), oracle().problem(inst)


def rand_pop(rng, n, inst):
    pen = rng.integers(0, 40, n).astype(np.int32)           # many ties: checks the stable order
    pen[rng.integers(0, n, max(1, n // 50))] = -1            # invalid genomes sort last
    return dict(slot=rng.integers(0, 45, (n, inst.E), dtype=np.uint8),
                room=rng.integers(0, inst.R, (n, inst.E), dtype=np.uint8),
                hcv=rng.integers(0, 9, n).astype(np.int32), scv=rng.integers(0, 99, n).astype(np.int32),
                feasible=rng.integers(0, 2, n).astype(np.uint8), penalty=pen)


def copy_genome(dst, i, src, j):
    dst["slot"][i], dst["room"][i] = src["slot"][j], src["room"][j]


CASES = ("nodup", "alldup", "childdup", "tail", "best", "migrant")


def build_case(rng, inst, N, C, case):
    pop, ch = rand_pop(rng, N, inst), rand_pop(rng, C, inst)
    if case in ("best", "migrant"):
        pop["penalty"] = np.sort(pop["penalty"].astype(np.uint32)).astype(np.int32)       # key order: -1 last
    if case == "alldup":
        for c in range(C):                           # members anywhere, the last position included
            copy_genome(ch, c, pop, N - 1 if c == 0 else int(rng.integers(0, N)))
    elif case == "childdup":
        for c in range(1, C, 3):                     # copies of lower children, and copies of copies
            copy_genome(ch, c, ch, int(rng.integers(0, c)))
    elif case == "tail":
        for c in range(0, C, 2):                     # members at positions >= N - C only
            copy_genome(ch, c, pop, N - 1 - int(rng.integers(0, C)))
    elif case == "best":
        pop["penalty"][pop["penalty"] == 0] = 1
        b = C - 1                                    # the best child is the last one ...
        ch["penalty"][ch["penalty"] == 0] = 1
        ch["penalty"][b] = 0
        for c in range(0, b, 2):                     # ... behind dropped children
            copy_genome(ch, c, pop, int(rng.integers(0, N)))
    elif case == "migrant":
        pop["penalty"][0] = 39 + 1                   # a survivor out of order (position 0 always survives C < N;
        for c in range(0, C, 4):                     # with C = N and a dropped child it survives too)
            copy_genome(ch, c, pop, int(rng.integers(0, N)))
    return pop, ch


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("N,C", [(10, 1), (64, 16), (300, 300), (4096, 2048), (9000, 8500), (257, 257),
                                 (8192, 8192)])
def test_replace_unique_vs_oracle(e20, N, C, case):
    inst, dp, o = e20
    rng = np.random.default_rng(N * 7 + C + CASES.index(case))
    pop, ch = build_case(rng, inst, N, C, case)
    keep = np_keep(pop, ch)
    D = int(keep.sum())
    exp = o.ga_replace(pop, {k: v[keep] for k, v in ch.items()})
    src = np_source(pop, ch, keep)
    # the cases are what they claim to be
    if case == "nodup":
        assert D == C
    elif case == "alldup":
        assert D == 0 and src < N
        order = np.lexsort((np.arange(N), pop["penalty"].astype(np.uint32)))
        assert all(np.array_equal(exp[k], pop[k][order]) for k in KEYS) and src == order[0]
    elif case == "childdup":
        assert (D < C) == (C > 1) and keep[0]
        assert not np_keep({k: v[:0] for k, v in pop.items()}, ch)[~keep].any()    # each dropped for a lower child
    elif case == "tail":
        assert not keep[0] and D < C
    elif case == "best":
        assert keep[C - 1] and src == N + C - 1 and (C == 1 or not keep[0])
        assert np.array_equal(exp["slot"][0], ch["slot"][C - 1])
    elif case == "migrant":
        assert not keep[0] and np.any(np.diff(pop["penalty"][:N - D].astype(np.uint32).astype(np.int64)) < 0)
    work = dp.ga_unique_work(N, C)
    off = int(dp.lib.tt_ga_work_source_offset(N, inst.E))
    for bits in (0, 1):
        gpop = {k: dev(v) for k, v in pop.items()}
        gkeep, gn = dp.ga_replace_unique(gpop, {k: dev(v) for k, v in ch.items()}, work, hash_bits=bits)
        assert np.array_equal(host(gkeep), keep.astype(np.uint8)), bits
        assert int(host(gn)[0]) == D
        for k in KEYS:
            assert np.array_equal(host(gpop[k]), exp[k]), (k, bits)
        assert dp.ga_work_source(work, N) == src
        assert int(host(work[off:off + 4].view(torch.int32))[0]) == src
    if case == "nodup":                                # bit for bit what tt_ga_replace gives
        gpop = {k: dev(v) for k, v in pop.items()}
        dp.ga_replace(gpop, {k: dev(v) for k, v in ch.items()}, dp.ga_work(N))
        for k in KEYS:
            assert np.array_equal(host(gpop[k]), exp[k]), k
    assert dp.status() == 0


def test_replace_unique_no_children_and_caller_buffers(e20):
    """C = 0 is tt_ga_replace's sort (n_kept 0); keep / n_kept tensors of the
    caller are filled in place, and wrong ones are refused."""
    inst, dp, o = e20
    rng = np.random.default_rng(5)
    pop = rand_pop(rng, 50, inst)
    exp = o.ga_replace(pop, {k: v[:0] for k, v in pop.items()})
    gpop = {k: dev(v) for k, v in pop.items()}
    work = dp.ga_unique_work(50, 7)
    n_kept = torch.full((1,), 9, dtype=torch.int32, device="cuda")
    dp.ga_replace_unique(gpop, None, work, n_kept=n_kept)
    assert int(host(n_kept)[0]) == 0
    for k in KEYS:
        assert np.array_equal(host(gpop[k]), exp[k]), k
    assert dp.ga_work_source(work, 50) == int(np.lexsort((np.arange(50), pop["penalty"].astype(np.uint32)))[0])
    ch = rand_pop(rng, 7, inst)
    copy_genome(ch, 2, pop, 11)
    keep = torch.zeros(7, dtype=torch.uint8, device="cuda")
    k2, n2 = dp.ga_replace_unique(gpop, {k: dev(v) for k, v in ch.items()}, work, keep=keep, n_kept=n_kept)
    assert k2 is keep and n2 is n_kept and host(keep).tolist() == [1, 1, 0, 1, 1, 1, 1] and int(host(n_kept)[0]) == 6
    with pytest.raises(ValueError):
        dp.ga_replace_unique(gpop, {k: dev(v) for k, v in ch.items()}, work, keep=keep[:3])
    with pytest.raises(ValueError):
        dp.ga_replace_unique(gpop, {k: dev(v) for k, v in ch.items()}, dp.ga_work(50)[:64])
    with pytest.raises(native.TTError):
        dp.ga_replace_unique(gpop, {k: dev(v) for k, v in ch.items()}, work, hash_bits=32)


# ----------------------------------------------------------------- the island
@pytest.fixture(scope="module")
def sm():
    inst = ttga.config_instance("sm")
    return inst, native.DeviceProblem(inst), oracle().problem(inst)


def model_generations(o, N, C, gens, steps, seed, pop_seed=None):
    """Batch schedule: breed -> local search -> eval -> keep -> ga_replace. The
    initial population is that of pop_seed (the drivers' islands all start from
    island 0's), the child streams are the island's own."""
    pop = oracle_population(o, N, seed if pop_seed is None else pop_seed, steps)
    rng = stream_seeds(seed, N, C)
    dropped = []
    for _ in range(gens):
        cs, cr, fl, rng = o.ga_breed(pop["slot"], pop["room"], pop["penalty"], rng, C, 0.8, 0.5, 1)
        cs, cr, rng = o.local_search(cs, cr, rng, steps)
        h, sc, f, p = o.eval(cs, cr)
        pop, d = model_replace(o, pop, dict(slot=cs, room=cr, hcv=h, scv=sc, feasible=f, penalty=p))
        dropped.append(d)
    return pop, rng, dropped


@pytest.mark.parametrize("N,C,gens", [(64, 16, 40), (10, 1, 200), (32, 32, 12)])
def test_island_unique_generations_vs_oracle(sm, N, C, gens):
    inst, dp, o = sm
    steps, seed = 120, 29
    isl = Island(dp, pop_size=N, children=C, max_steps=steps, seed=seed, unique=True)
    isl.initialize()
    for _ in range(gens):
        isl.step()
    pop, rng, dropped = model_generations(o, N, C, gens, steps, seed)
    assert sum(dropped) > 0                              # otherwise nothing is shown
    if C == 1:
        assert max(dropped) == 1                         # a generation that kept none
    for k in KEYS:
        assert np.array_equal(host(isl.pop[k]), pop[k]), k
    assert np.array_equal(host(isl.rng_child), rng)
    assert distinct(pop) == N
    assert isl.unique_stats() == {"children": gens * C, "dropped": sum(dropped), "distinct": N}
    assert np.all(np.diff(pop["penalty"].astype(np.uint32).astype(np.int64)) >= 0)


def model_staggered(o, pop, rng_child, C, gens, steps, parts):
    """tests/test_gpu_ga.py's oracle_staggered with the keep rule at every
    replacement: sub-batch h bred behind the replacement of h - parts, h - parts
    + 1 replaced right behind that breed, the pending ones at the end."""
    sizes = [len(x) for x in np.array_split(np.arange(C), parts)]
    offs = np.cumsum([0] + sizes)
    rng = [rng_child[offs[j]:offs[j + 1]].copy() for j in range(parts)]
    pending, dropped = [], 0
    for _ in range(gens):
        for j in range(parts):
            cs, cr, fl, rng[j] = o.ga_breed(pop["slot"], pop["room"], pop["penalty"], rng[j], sizes[j], 0.8, 0.5, 1)
            if len(pending) >= parts - 1:
                pop, d = model_replace(o, pop, pending.pop(0))
                dropped += d
            cs, cr, rng[j] = o.local_search(cs, cr, rng[j], steps)
            h, sc, f, p = o.eval(cs, cr)
            pending.append(dict(slot=cs, room=cr, hcv=h, scv=sc, feasible=f, penalty=p))
    while pending:
        pop, d = model_replace(o, pop, pending.pop(0))
        dropped += d
    return pop, np.concatenate(rng), dropped


def test_island_unique_staggered_vs_oracle(sm):
    inst, dp, o = sm
    N, C, gens, steps, seed = 64, 48, 12, 120, 41
    isl = Island(dp, pop_size=N, children=C, max_steps=steps, seed=seed, unique=True, schedule="staggered", parts=2)
    isl.initialize()
    for _ in range(gens):
        isl.step()
    pop, rng, dropped = model_staggered(o, oracle_population(o, N, seed, steps), stream_seeds(seed, N, C), C, gens,
                                        steps, 2)
    assert dropped > 0
    isl.sync()
    for k in KEYS:
        assert np.array_equal(host(isl.pop[k]), pop[k]), k
    assert np.array_equal(host(isl.rng_child), rng)
    got = {k: host(isl.pop[k]) for k in ("slot", "room")}
    assert distinct(got) == N
    assert isl.unique_stats() == {"children": gens * C, "dropped": dropped, "distinct": N}


def test_island_unique_equals_plain_when_nothing_is_dropped(sm):
    inst, dp, o = sm
    N, C, gens, steps, seed = 16, 8, 3, 120, 29
    _, _, dropped = model_generations(o, N, C, gens, steps, seed)
    assert sum(dropped) == 0
    isls = [Island(dp, pop_size=N, children=C, max_steps=steps, seed=seed, unique=u) for u in (False, True)]
    for isl in isls:
        isl.initialize()
        for _ in range(gens):
            isl.step()
    for k in KEYS:
        assert np.array_equal(host(isls[0].pop[k]), host(isls[1].pop[k])), k
    assert np.array_equal(host(isls[0].rng_child), host(isls[1].rng_child))
    assert isls[0].best_thread() == isls[1].best_thread()
    assert isls[0].snapshot().values() == isls[1].snapshot().values()
    assert isls[1].unique_stats() == {"children": gens * C, "dropped": 0, "distinct": N}
    with pytest.raises(ValueError):
        isls[0].unique_stats()


# ---------------------------------------------------------------- the drivers
def test_unique_lines_of_both_drivers(tmp_path, sm):
    inst, dp, o = sm
    tim = tmp_path / "sm.tim"
    ttga.write_tim(inst, tim)
    base = ["-i", str(tim), "-s", "29", "-p", "1", "--pop", "32", "--children", "32", "--generations", "12"]
    py, cc, b, _ = both_drivers(tmp_path, base, ["--unique"], "unique", inst)
    py_plain = run_driver([sys.executable, "-m", "ttga.islands", *base], tmp_path)
    cc_plain = run_driver([str(GA), *base], tmp_path)
    raw = [stage_lines(r.stdout, "unique") for r in (py, cc, py_plain, cc_plain)]
    assert raw[0] == raw[1] and len(raw[0]) == 1 and raw[2] == [] and raw[3] == []
    assert _json_lines(py_plain.stdout) == _json_lines(cc_plain.stdout)
    u = [x["unique"] for x in b if "unique" in x][0]
    # the run is the model's (32, 32, 12) at the island's seed (ga.cpp:412 leaves island 0's as given)
    _, _, dropped = model_generations(o, 32, 32, 12, 200, 29)
    assert u == {"children": 12 * 32, "dropped": sum(dropped), "distinct": 32, "island": 0, "procID": 0}
    assert u["dropped"] > 0
    keys = [next(iter(x)) for x in b]
    assert keys.index("unique") == keys.index("solution") + 1 and keys[-1] == "runEntry"
    both = _json_lines(run_driver([str(GA), "--unique", "--report", *base], tmp_path).stdout)
    keys = [next(iter(x)) for x in both]
    assert keys.index("unique") == keys.index("solution") + 1 and keys.index("report") == keys.index("unique") + 1


def test_unique_lines_of_both_drivers_two_islands(tmp_path, sm):
    """Two islands in one process: island 1 never builds an initial population
    (it takes island 0's), and its line must count every one of its
    replacements all the same. Both drivers against the model of each island."""
    from ttga.islands import rank_seed
    inst, dp, o = sm
    tim = tmp_path / "sm.tim"
    ttga.write_tim(inst, tim)
    base = ["-i", str(tim), "-s", "29", "-p", "1", "--pop", "32", "--children", "32", "--generations", "12",
            "--islands", "2", "--unique"]
    py = run_driver([sys.executable, "-m", "ttga.islands", *base], tmp_path)
    cc = run_driver([str(GA), *base], tmp_path)
    raw = [stage_lines(r.stdout, "unique") for r in (py, cc)]
    assert raw[0] == raw[1] and len(raw[0]) == 2
    got = [x["unique"] for x in _json_lines(cc.stdout) if "unique" in x]
    for k in (0, 1):
        pop, _, dropped = model_generations(o, 32, 32, 12, 200, rank_seed(29, k), pop_seed=29)
        assert got[k] == {"children": 12 * 32, "dropped": sum(dropped), "distinct": distinct(pop), "island": k,
                          "procID": k}, k
        assert got[k]["dropped"] > 0 and got[k]["distinct"] == 32
    sols = [[x for x in _json_lines(r.stdout) if "solution" in x] for r in (py, cc)]
    assert sols[0] == sols[1] and len(sols[0]) == 2
