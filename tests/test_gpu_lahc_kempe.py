"""tt_lahc_kempe (include/ttga_lahc_kempe.h) on the GPU against
tests/lahc_kempe_model.py: slot, room, the rng state, gain, accepted, best_step
and the five Kempe counts bit for bit, feasible and infeasible rows mixed in one
launch, and around every call tt_eval: hcv 0, scv lower by exactly the gain,
the scv / penalty updated in place equal to a fresh evaluation. Then the call
without chains against tt_lahc, invalid genes and arguments, the LDS limit,
Island(lahc_kempe=...) and the two drivers with --lahc-kempe."""
import pathlib
import sys

import numpy as np
import pytest

import ttga
import lahc_kempe_model as km
import lahc_model as lm
import walk_checks as wc
from helpers import host, json_lines
from stage_checks import GA, VARIANTS, both_drivers, run_driver, run_island, stage_lines
from walk_checks import BAD_GENE, NAMES

pytestmark = pytest.mark.gpu

from ttga import native  # noqa: E402

REPO = pathlib.Path(__file__).resolve().parent.parent

# id: (shape, P, steps, history, p_swap, p_kempe, max_chain)
CASES = {
    "sm": ("sm", 33, 1000, 50, 0.25, 0.5, 0), "sm-cap2": ("sm", 33, 1000, 50, 0.25, 0.5, 2),
    "med": ("med", 9, 1000, 500, 0.25, 0.5, 0),
    "E1": ("E1", 33, 1000, 50, 0.0, 1.0, 0), "E2": ("E2", 33, 1000, 50, 0.0, 1.0, 0),
    "E3": ("E3", 33, 1000, 50, 0.25, 0.5, 0),
    "E63": ("E63", 33, 1000, 50, 0.25, 0.5, 0), "E64": ("E64", 33, 1000, 50, 0.25, 0.5, 0),
    "E65": ("E65", 33, 1000, 50, 0.25, 0.5, 0),
    "R1": ("R1", 33, 1000, 50, 0.25, 0.5, 0), "R64": ("R64", 33, 1000, 50, 0.25, 0.5, 0),
    "S0": ("S0", 33, 1000, 50, 0.25, 0.5, 0), "extremes": ("extremes", 33, 1000, 50, 0.25, 0.5, 0),
    "tight_rooms": ("tight_rooms", 33, 1000, 50, 0.25, 0.5, 0),
    "syn_sparse": ("syn_sparse", 4, 300, 100, 0.25, 0.5, 0),
    "kempe-only": ("sm", 33, 1000, 50, 0.0, 1.0, 0), "no-move1": ("sm", 33, 1000, 50, 0.5, 0.5, 0),
    "steps0": ("sm", 33, 0, 50, 0.25, 0.5, 0), "steps1": ("sm", 33, 1, 50, 0.25, 0.5, 0),
    "tight": ("tight", 33, 1000, 50, 0.25, 0.5, 0),
}


@pytest.fixture(scope="module")
def problems():
    cache = {}

    def get(name):
        if name not in cache:
            inst = lm.SHAPES[name]()
            cache[name] = (inst, native.DeviceProblem(inst), km.Model(inst))
        return cache[name]
    return get


def call(dp, a):
    return lambda s, r, g, **out: dp.lahc_kempe(s, r, g, a["steps"], a["history"], a["p_swap"], a["p_kempe"],
                                                a["max_chain"], **out)


def rows(model, slot, room, seeds, a, infos=None):
    return model.lahc_kempe_rows(slot, room, seeds, a["steps"], a["history"], a["p_swap"], a["p_kempe"], a["max_chain"],
                                 infos)


def walk_args(steps, L, p_swap, p_kempe, cap=0):
    return dict(steps=steps, history=L, p_swap=p_swap, p_kempe=p_kempe, max_chain=cap)


def check(problem, slot, room, seeds, steps, L, p_swap, p_kempe, cap, infos=None):
    inst, dp, model = problem
    a = walk_args(steps, L, p_swap, p_kempe, cap)
    want = rows(model, slot, room, seeds, a, infos)
    got, before, after, inplace = wc.run(dp, call(dp, a), slot, room, seeds, 5)
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
    kinds = {k: sum(i[k] for i in searched)
             for k in ("move1", "move2", "kempe", "two_sided", "order_matters", "left_room")}
    chains = [n for i in searched for n in i["chains"]]
    tried, capped, no_room, k_acc, events = (int(x) for x in want[6].sum(axis=0))
    print(cid, "feasible", int((hcv0 == 0).sum()), "of", P, "gain", int(got[3].sum()), "accepted", int(got[4].sum()),
          kinds, "tried/capped/no room/accepted/events", (tried, capped, no_room, k_acc, events),
          "longest", max(chains, default=0))
    if shape in lm.NO_FEASIBLE_ROW:
        assert (hcv0 != 0).all()
        return
    assert 2 * int((hcv0 == 0).sum()) >= P
    assert (hcv0 != 0).any() or inst.E < 2                          # both kinds of rows in the launch
    if steps == 0:
        assert not got[4].any() and not got[6].any() and np.array_equal(got[0], slot) and np.array_equal(got[2], seeds)
        return
    wc.check_stream_advance(got, seeds, hcv0 != 0, 3 * steps)      # exactly 3 * steps draws a searched row
    assert k_acc == kinds["kempe"] == len(chains) and events == sum(chains)
    if steps > 1:
        assert got[4].sum() > 0 and tried > 0
    # what each case is in the list for, asserted on the model's side
    if cid == "sm":
        assert chains.count(1) > 0 and max(chains) >= 2 and kinds["two_sided"] > 0 and no_room > 0
        assert kinds["move1"] > 0 and kinds["move2"] > 0 and kinds["kempe"] > 0
        assert capped == 0
    if cid == "sm-cap2":
        assert capped > 0 and max(chains) <= 2
    if cid == "med":
        assert max(chains) >= 8
    if cid in ("E1", "E2", "kempe-only"):
        assert kinds["move1"] == kinds["move2"] == 0 and kinds["kempe"] > 0
        assert tried == steps * int((hcv0 == 0).sum())
    if cid == "no-move1":
        assert kinds["move1"] == 0 and kinds["move2"] > 0 and kinds["kempe"] > 0
    if cid in ("E63", "E64", "E65"):
        assert max(chains) >= 2
    if cid == "R1":                                                 # one room: a chain has one event a side
        assert set(chains) == {1, 2} and kinds["left_room"] == chains.count(2)
    if cid == "R64":
        assert any((w == 63).any() for w in want[1]) and int(want[1][hcv0 == 0][:, 0].min()) == 63
    if cid == "S0":                                                 # delta is 0 everywhere
        assert not got[3].any() and k_acc == tried - capped - no_room > 0
    if cid == "extremes":
        full = [i for i in range(P) if hcv0[i] == 0]
        assert full and all(len(set(want[0][i][:45].tolist())) == 45 for i in full)
        assert kinds["two_sided"] > 0
    assert dp.status() & BAD_GENE == 0


# ---------------------------------------------------------------- no chains: tt_lahc
@pytest.mark.parametrize("p_swap", [0.0, 0.5, 1.0])
def test_without_chains_the_call_is_tt_lahc(problems, p_swap):
    inst, dp, model = problems("sm")
    slot, room, seeds = lm.population(inst, 33, model)

    a = wc.run(dp, call(dp, walk_args(1000, 50, p_swap, 0.0, 3)), slot, room, seeds, 5)
    b = wc.run(dp, lambda s, r, g, **out: dp.lahc(s, r, g, 1000, 50, p_swap, **out), slot, room, seeds)
    for name, x, y in zip(NAMES[:6], a[0], b[0]):
        assert np.array_equal(x, y), name
    assert not a[0][6].any() and a[0][4].sum() > 0
    assert np.array_equal(a[3][0], b[3][0]) and np.array_equal(a[3][1], b[3][1])          # scv and penalty in place


# ---------------------------------------------------------------- invalid genes, errors, the limit
OK = walk_args(10, 5, 0.25, 0.5)
BAD = (dict(steps=-1), dict(history=0), dict(history=-3), dict(p_swap=1.5, p_kempe=0.0), dict(p_swap=-0.1),
       dict(p_swap=float("nan")), dict(p_kempe=1.5, p_swap=0.0), dict(p_kempe=-0.1), dict(p_kempe=float("nan")),
       dict(max_chain=-1), dict(p_swap=0.75, p_kempe=0.5), dict(p_swap=0.25, p_kempe=1.0))


def test_invalid_genes():
    wc.invalid_genes(km.Model, call, rows, walk_args(500, 50, 0.25, 0.5), 5)


def test_invalid_arguments_launch_nothing(problems):
    wc.invalid_arguments_launch_nothing(problems("sm"), call, rows, OK, BAD,
                                        lambda dp, s, r, g: dp.lahc_kempe(s, r, g, 200, 20, 0.25, 0.5), 5)


def test_limit(problems):
    """The header's formula for sm (E 100, S 80) without the history:
    8 * (47 * 2 + 45 + 80) + 4 * 100 + 1,168 = 3,320 bytes."""
    wc.lds_limit(problems("sm"), call, rows, OK, 3320, 5)


# ---------------------------------------------------------------- Island
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_island_lahc_kempe(problems, variant):
    inst, dp, _ = problems("sm")
    kw = VARIANTS[variant]
    a = run_island(dp, lahc=500, lahc_kempe=0.5, init="greedy", **kw)
    b = run_island(dp, lahc=500, lahc_kempe=0.5, init="greedy", **kw)
    for k in a.pop:
        assert np.array_equal(host(a.pop[k]), host(b.pop[k])), k           # run twice: identical
    p = a.pop
    hcv, scv, feas, pen = (host(t) for t in dp.eval(p["slot"], p["room"]))
    assert np.array_equal(host(p["hcv"]), hcv) and np.array_equal(host(p["scv"]), scv)
    assert np.array_equal(host(p["feasible"]), feas) and np.array_equal(host(p["penalty"]), pen)
    st, walk = a.lahc_kempe_stats(), a.lahc_stats()
    print(variant, st, walk)
    assert set(st) == {"rows", "tried", "capped", "no_room", "accepted", "chain_events"}
    assert st["rows"] == walk["rows"] == 10 + 30 * kw.get("children", 1)
    assert 0 < st["accepted"] <= st["tried"] - st["capped"] - st["no_room"] and st["capped"] == 0
    assert st["chain_events"] >= st["accepted"] and walk["accepted"] >= st["accepted"] and walk["gain"] > 0
    assert "lahc_kempe" in a.on and st == b.lahc_kempe_stats()
    a.close()
    b.close()
    assert dp.status() & BAD_GENE == 0


def test_island_lahc_kempe_0_never_calls_the_new_binding(problems, monkeypatch):
    inst, dp, _ = problems("sm")
    plain = run_island(dp, gens=8, init="greedy", lahc=100)

    def boom(*a, **k):
        raise AssertionError("lahc_kempe called with Island(lahc_kempe=0)")
    monkeypatch.setattr(dp, "lahc_kempe", boom)
    off = run_island(dp, gens=8, init="greedy", lahc=100, lahc_kempe=0.0, lahc_kempe_max_chain=4)
    for k in plain.pop:
        assert np.array_equal(host(off.pop[k]), host(plain.pop[k])), k
    with pytest.raises(ValueError, match="lahc_kempe_stats"):
        off.lahc_kempe_stats()
    assert "lahc_kempe" not in off.on and off.lahc_stats() == plain.lahc_stats()
    off.close()
    plain.close()


# ---------------------------------------------------------------- the drivers
def test_lahc_kempe_in_both_drivers(tmp_path):
    tim = REPO / "tests" / "golden" / "sm.tim"
    inst = ttga.read_tim(tim)
    base = ["-i", str(tim), "-s", "29", "-p", "1", "--pop", "16", "--children", "8", "--generations", "10",
            "--init", "greedy"]
    flags = ["--lahc", "500", "--lahc-history", "100", "--lahc-swap", "0.25", "--lahc-kempe", "0.5",
             "--lahc-kempe-max-chain", "8"]
    py, cc, a, lines = both_drivers(tmp_path, base, flags, "lahcKempe", inst)
    assert stage_lines(py.stdout, "lahc") == stage_lines(cc.stdout, "lahc")              # byte for byte
    assert len(lines) == 1 and set(lines[0]) == {"tried", "capped", "noRoom", "accepted", "meanChain"}
    k = lines[0]
    walk = [x["lahc"] for x in a if "lahc" in x]
    assert len(walk) == 1 and set(walk[0]) == {"accepted", "gain", "improved", "rows", "searched"}
    assert 0 < k["accepted"] <= k["tried"] - k["capped"] - k["noRoom"] and 1.0 <= k["meanChain"] <= 8.0
    assert k["accepted"] <= walk[0]["accepted"] and walk[0]["rows"] == 16 + 80
    kinds = [next(iter(x)) for x in a]
    assert kinds.index("lahcKempe") == kinds.index("lahc") + 1 > kinds.index("solution")


def test_all_stages_with_lahc_kempe_in_both_drivers(tmp_path):
    """tests/test_gpu_all_stages.py's run, batch schedule, with --lahc-kempe on too."""
    from test_gpu_all_stages import ARGS, STAGE_KINDS, _per_island
    kinds_all = STAGE_KINDS + ("lahcKempe",)
    tim = REPO / "tests" / "golden" / "sm.tim"
    inst = ttga.read_tim(tim)
    args = ["-i", str(tim), *ARGS, "--lahc-swap", "0.25", "--lahc-kempe", "0.5", "--lahc-kempe-max-chain", "6"]
    py = run_driver([sys.executable, "-m", "ttga.islands", *args], tmp_path)
    cc = run_driver([str(GA), *args], tmp_path)
    a, b = json_lines(py.stdout), json_lines(cc.stdout)
    assert _per_island(a) == _per_island(b) and a

    def stage_lines(text):
        return [ln for ln in text.splitlines() if ln.startswith(tuple('{"%s"' % k for k in kinds_all))]
    assert stage_lines(py.stdout) == stage_lines(cc.stdout)             # byte for byte
    kinds = [next(iter(x)) for x in a]
    tail = [k for k in kinds if k in kinds_all + ("solution",)]
    assert tail == (["solution", "crossover", "kempe"] * 2 + ["unique"] * 2 + ["slotSwap"] * 2 + ["lahc"] * 2
                    + ["lahcKempe"] * 2)
    assert kinds[kinds.index("solution"):] == tail + ["runEntry"]
    assert [x["lahc"]["rows"] for x in a if "lahc" in x] == [496, 480]
    for k in (x["lahcKempe"] for x in a if "lahcKempe" in x):
        assert 0 < k["accepted"] <= k["tried"] - k["capped"] - k["noRoom"] and k["meanChain"] <= 6.0
    from ttga.validate import check_text
    for r_ in (py, cc):
        reps = check_text(inst, r_.stdout)
        assert reps and all(x["ok"] for x in reps), reps
