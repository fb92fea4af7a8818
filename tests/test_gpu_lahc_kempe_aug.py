"""tt_lahc_kempe_aug (include/ttga_lahc_kempe_aug.h) on the GPU against
tests/lahc_kempe_aug_model.py: slot, room, the rng state, gain, accepted,
best_step and the seven Kempe counts bit for bit, feasible and spoiled rows
mixed in one launch, and around every call tt_eval: hcv unchanged, scv lower by
exactly the gain, the scv / penalty updated in place equal to a fresh
evaluation. Then the calls that must equal tt_lahc_kempe and tt_lahc, invalid
genes and arguments, the LDS limit, Island(lahc_kempe_rooms="augment") and the
two drivers with --lahc-kempe-rooms augment."""
import pathlib

import numpy as np
import pytest

import ttga
import lahc_kempe_aug_model as am
import lahc_model as lm
import walk_checks as wc
from helpers import host
from stage_checks import VARIANTS, both_drivers, run_island, stage_lines
from walk_checks import BAD_GENE, NAMES

pytestmark = pytest.mark.gpu

from ttga import native  # noqa: E402

REPO = pathlib.Path(__file__).resolve().parent.parent

SHAPES = dict(lm.SHAPES, g300=lambda: ttga.generate(300, 12, 5, 150, seed=22),
              g600=lambda: ttga.generate(600, 64, 10, 300, seed=23))

# id: (shape, P, steps, history, p_swap, p_kempe, max_chain)
CASES = {
    "sm": ("sm", 33, 1000, 50, 0.25, 0.5, 0), "E65": ("E65", 33, 1000, 50, 0.25, 0.5, 0),
    "med": ("med", 9, 1000, 500, 0.25, 0.5, 0),
    "g300": ("g300", 9, 1000, 50, 0.25, 0.5, 0), "g600": ("g600", 5, 600, 50, 0.25, 0.5, 0),
    "sm-cap2": ("sm", 33, 1000, 50, 0.25, 0.5, 2),
    "E1": ("E1", 33, 1000, 50, 0.0, 1.0, 0), "E2": ("E2", 33, 1000, 50, 0.0, 1.0, 0),
    "E3": ("E3", 33, 1000, 50, 0.25, 0.5, 0),
    "E63": ("E63", 33, 1000, 50, 0.25, 0.5, 0), "E64": ("E64", 33, 1000, 50, 0.25, 0.5, 0),
    "R64": ("R64", 33, 1000, 50, 0.25, 0.5, 0),
    "S0": ("S0", 33, 1000, 50, 0.25, 0.5, 0), "extremes": ("extremes", 33, 1000, 50, 0.25, 0.5, 0),
    "tight": ("tight", 33, 1000, 50, 0.25, 0.5, 0),
    "steps0": ("sm", 33, 0, 50, 0.25, 0.5, 0), "steps1": ("sm", 33, 1, 50, 0.25, 0.5, 0),
    "kempe-only": ("sm", 33, 1000, 50, 0.0, 1.0, 0),
    "syn_sparse": ("syn_sparse", 4, 300, 100, 0.25, 0.5, 0),
}
# the longest path (holders moved) of an accepted chain that the model must show
LONGEST = {"sm": 3, "med": 4, "g300": 4}


@pytest.fixture(scope="module")
def problems():
    cache = {}

    def get(name):
        if name not in cache:
            inst = SHAPES[name]()
            cache[name] = (inst, native.DeviceProblem(inst), am.Model(inst))
        return cache[name]
    return get


def call(dp, a):
    return lambda s, r, g, **out: dp.lahc_kempe_aug(s, r, g, a["steps"], a["history"], a["p_swap"], a["p_kempe"],
                                                    a["max_chain"], a["room_rule"], **out)


def kempe_call(dp, a):
    return lambda s, r, g, **out: dp.lahc_kempe(s, r, g, a["steps"], a["history"], a["p_swap"], a["p_kempe"],
                                                a["max_chain"], **out)


def rows(model, slot, room, seeds, a, infos=None):
    return model.lahc_kempe_aug_rows(slot, room, seeds, a["steps"], a["history"], a["p_swap"], a["p_kempe"],
                                     a["max_chain"], a["room_rule"], infos)


def walk_args(steps, L, p_swap, p_kempe, cap=0, rule=1):
    return dict(steps=steps, history=L, p_swap=p_swap, p_kempe=p_kempe, max_chain=cap, room_rule=rule)


def check(problem, slot, room, seeds, steps, L, p_swap, p_kempe, cap, infos=None):
    inst, dp, model = problem
    a = walk_args(steps, L, p_swap, p_kempe, cap)
    want = rows(model, slot, room, seeds, a, infos)
    got, before, after, inplace = wc.run(dp, call(dp, a), slot, room, seeds, 7)
    wc.check_rows(got, want, before, after, inplace, slot, room, seeds, steps)
    return got, want, before[0]


@pytest.mark.parametrize("cid", list(CASES))
def test_rows_vs_model(problems, cid):
    shape, P, steps, L, p_swap, p_kempe, cap = CASES[cid]
    pb = problems(shape)
    inst, dp, model = pb
    slot, room, seeds = lm.population(inst, P, model)
    infos = []
    got, want, hcv0 = check(pb, slot, room, seeds, steps, L, p_swap, p_kempe, cap, infos)
    searched = [i for i in infos if i]
    chains = [n for i in searched for n in i["chains"]]
    longest = max([i["longest_path"] for i in searched], default=0)
    moved_k = sum(i["moved_chain_event"] for i in searched)
    high = max([i["high_room"] for i in searched], default=-1)
    tried, capped, no_room, k_acc, events, rescued, displaced = (int(x) for x in want[6].sum(axis=0))
    print(cid, "feasible", int((hcv0 == 0).sum()), "of", P, "gain", int(got[3].sum()), "accepted", int(got[4].sum()),
          "tried/capped/no room/accepted/events/rescued/displaced",
          (tried, capped, no_room, k_acc, events, rescued, displaced), "longest chain", max(chains, default=0),
          "longest path", longest, "paths that moved a chain event", moved_k, "highest room on a path", high)
    if shape in lm.NO_FEASIBLE_ROW:
        assert (hcv0 != 0).all()
        return
    assert 2 * int((hcv0 == 0).sum()) >= P
    assert (hcv0 != 0).any() or inst.E < 2                          # both kinds of rows in the launch
    if steps == 0:
        assert not got[4].any() and not got[6].any() and np.array_equal(got[0], slot) and np.array_equal(got[2], seeds)
        return
    wc.check_stream_advance(got, seeds, hcv0 != 0, 3 * steps)      # exactly 3 * steps draws a searched row
    assert k_acc == len(chains) and events == sum(chains)
    if steps > 1:
        assert got[4].sum() > 0 and tried > 0
    # what each case is in the list for, asserted on the model's side
    if cid in ("sm", "E65", "med", "g300", "g600"):
        assert rescued > 0 and displaced > 0
        assert longest >= LONGEST.get(cid, 1)
    if cid in ("sm", "med", "g300"):
        assert moved_k > 0                                          # a path displaced an event of K placed earlier
    if cid == "g600":
        assert high >= 32                                           # the upper half of the 64-bit room words
    if cid == "sm-cap2":
        assert capped > 0 and max(chains) <= 2
    if cid in ("E1", "E2", "kempe-only"):
        assert tried == steps * int((hcv0 == 0).sum())
    if cid == "R64":
        assert any((w == 63).any() for w in want[1])
    if cid == "S0":
        assert not got[3].any() and k_acc == tried - capped - no_room > 0
    assert dp.status() & BAD_GENE == 0


# ---------------------------------------------------------------- equal to tt_lahc_kempe and tt_lahc
def same_as_lahc_kempe(a, b):
    for name, x, y in zip(NAMES[:6], a[0], b[0]):
        assert np.array_equal(x, y), name
    assert np.array_equal(a[0][6][:, :5], b[0][6]) and not a[0][6][:, 5:].any()
    assert np.array_equal(a[3][0], b[3][0]) and np.array_equal(a[3][1], b[3][1])          # scv and penalty in place
    assert a[0][6][:, 0].sum() > 0 and a[0][4].sum() > 0


@pytest.mark.parametrize("shape", ["tight_rooms", "R1"])
def test_where_no_path_can_help_the_call_is_tt_lahc_kempe(problems, shape):
    """Every room possible for every event, or one room: an event without a
    free possible room has no augmenting path either."""
    inst, dp, model = problems(shape)
    slot, room, seeds = lm.population(inst, 33, model)
    args = walk_args(1000, 50, 0.25, 0.5)
    a = wc.run(dp, call(dp, args), slot, room, seeds, 7)
    b = wc.run(dp, kempe_call(dp, args), slot, room, seeds, 5)
    same_as_lahc_kempe(a, b)
    assert a[0][6][:, 2].sum() > 0                                   # and chains without a room there are


@pytest.mark.parametrize("p_swap", [0.0, 0.25])
def test_room_rule_0_is_tt_lahc_kempe(problems, p_swap):
    inst, dp, model = problems("sm")
    slot, room, seeds = lm.population(inst, 33, model)
    args = walk_args(1000, 50, p_swap, 0.5, rule=0)
    a = wc.run(dp, call(dp, args), slot, room, seeds, 7)
    b = wc.run(dp, kempe_call(dp, args), slot, room, seeds, 5)
    same_as_lahc_kempe(a, b)
    assert a[0][6][:, 2].sum() > 0


def test_without_chains_the_call_is_tt_lahc(problems):
    inst, dp, model = problems("sm")
    slot, room, seeds = lm.population(inst, 33, model)

    a = wc.run(dp, call(dp, walk_args(1000, 50, 0.5, 0.0, 3)), slot, room, seeds, 7)
    b = wc.run(dp, lambda s, r, g, **out: dp.lahc(s, r, g, 1000, 50, 0.5, **out), slot, room, seeds)
    for name, x, y in zip(NAMES[:6], a[0], b[0]):
        assert np.array_equal(x, y), name
    assert not a[0][6].any() and a[0][4].sum() > 0
    assert np.array_equal(a[3][0], b[3][0]) and np.array_equal(a[3][1], b[3][1])


# ---------------------------------------------------------------- invalid genes, errors, the limit
OK = walk_args(10, 5, 0.25, 0.5)
BAD = (dict(room_rule=-1), dict(room_rule=2), dict(steps=-1), dict(history=0), dict(history=-3),
       dict(p_swap=1.5, p_kempe=0.0), dict(p_swap=-0.1), dict(p_swap=float("nan")), dict(p_kempe=1.5, p_swap=0.0),
       dict(p_kempe=-0.1), dict(p_kempe=float("nan")), dict(max_chain=-1), dict(p_swap=0.75, p_kempe=0.5),
       dict(p_swap=0.25, p_kempe=1.0))


def test_invalid_genes():
    wc.invalid_genes(am.Model, call, rows, walk_args(500, 50, 0.25, 0.5), 7)


def test_invalid_arguments_launch_nothing(problems):
    wc.invalid_arguments_launch_nothing(problems("sm"), call, rows, OK, BAD,
                                        lambda dp, s, r, g: dp.lahc_kempe_aug(s, r, g, 200, 20, 0.25, 0.5), 7)


def test_limit(problems):
    """The header's formula for sm (E 100, S 80) without the history:
    8 * (47 * 2 + 45 + 80) + 4 * 100 + 1,552 = 3,704 bytes. With the largest
    history that fits, the search's state is the last of the image."""
    assert 8 * (47 * 2 + 45 + 80) + 4 * 100 + 1552 == 3704
    slot, room, want = wc.lds_limit(problems("sm"), call, rows, walk_args(300, 5, 0.25, 0.5), 3704, 7)
    assert np.array_equal(slot, want[0]) and np.array_equal(room, want[1])
    assert want[6][:, 5].sum() > 0


# ---------------------------------------------------------------- Island
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_island_augment(problems, variant):
    inst, dp, _ = problems("sm")
    kw = VARIANTS[variant]
    a = run_island(dp, lahc=500, lahc_kempe=0.5, lahc_kempe_rooms="augment", init="greedy", **kw)
    b = run_island(dp, lahc=500, lahc_kempe=0.5, lahc_kempe_rooms="augment", init="greedy", **kw)
    for k in a.pop:
        assert np.array_equal(host(a.pop[k]), host(b.pop[k])), k           # run twice: identical
    p = a.pop
    hcv, scv, feas, pen = (host(t) for t in dp.eval(p["slot"], p["room"]))
    assert np.array_equal(host(p["hcv"]), hcv) and np.array_equal(host(p["scv"]), scv)
    assert np.array_equal(host(p["feasible"]), feas) and np.array_equal(host(p["penalty"]), pen)
    st, walk = a.lahc_kempe_stats(), a.lahc_stats()
    print(variant, st, walk)
    assert set(st) == {"rows", "tried", "capped", "no_room", "accepted", "chain_events", "rescued", "displaced"}
    assert st["rows"] == walk["rows"] == 10 + 30 * kw.get("children", 1)
    assert 0 < st["accepted"] <= st["tried"] - st["capped"] - st["no_room"] and st["capped"] == 0
    assert 0 < st["rescued"] <= st["tried"] - st["no_room"] and st["displaced"] > 0
    assert "lahc_kempe" in a.on and st == b.lahc_kempe_stats()
    a.close()
    b.close()
    assert dp.status() & BAD_GENE == 0


def test_island_direct_never_calls_the_new_binding(problems, monkeypatch):
    inst, dp, _ = problems("sm")
    today = run_island(dp, gens=8, init="greedy", lahc=100, lahc_kempe=0.5, lahc_swap=0.25)

    def boom(*a, **k):
        raise AssertionError("lahc_kempe_aug called with Island(lahc_kempe_rooms='direct')")
    monkeypatch.setattr(dp, "lahc_kempe_aug", boom)
    direct = run_island(dp, gens=8, init="greedy", lahc=100, lahc_kempe=0.5, lahc_swap=0.25, lahc_kempe_rooms="direct")
    plain = run_island(dp, gens=8, init="greedy", lahc=100, lahc_kempe_rooms="direct")
    for k in today.pop:
        assert np.array_equal(host(direct.pop[k]), host(today.pop[k])), k
    st = direct.lahc_kempe_stats()
    assert st == today.lahc_kempe_stats() and set(st) == {"rows", "tried", "capped", "no_room", "accepted",
                                                          "chain_events"}
    assert "lahc_kempe" not in plain.on and plain.lahc_stats()["rows"] > 0
    for isl in (today, direct, plain):
        isl.close()


# ---------------------------------------------------------------- the drivers
def test_augment_in_both_drivers(tmp_path):
    tim = REPO / "tests" / "golden" / "sm.tim"
    inst = ttga.read_tim(tim)
    base = ["-i", str(tim), "-s", "29", "-p", "1", "--pop", "16", "--children", "8", "--generations", "10",
            "--init", "greedy"]
    flags = ["--lahc", "500", "--lahc-swap", "0.25", "--lahc-kempe", "0.5", "--lahc-kempe-rooms", "augment"]
    py, cc, a, lines = both_drivers(tmp_path, base, flags, "lahcKempe", inst)
    assert stage_lines(py.stdout, "lahc") == stage_lines(cc.stdout, "lahc")              # byte for byte
    assert len(lines) == 1
    k = lines[0]
    assert set(k) == {"tried", "capped", "noRoom", "accepted", "meanChain", "rescued", "displaced"}
    assert 0 < k["accepted"] <= k["tried"] - k["capped"] - k["noRoom"] and k["rescued"] > 0 and k["displaced"] >= 0
