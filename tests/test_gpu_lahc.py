"""The late-acceptance search (include/ttga_lahc.h) on the GPU against
tests/lahc_model.py: slot, room, the rng state, gain, accepted and best_step
bit for bit, feasible and infeasible rows mixed in one launch, and around every
call tt_eval: hcv 0, scv lower by exactly the gain, the scv / penalty updated
in place equal to a fresh evaluation, infeasible rows byte-identical with
their rng untouched. Then Island(lahc=...) and the two drivers with --lahc.

Two shapes of the list admit no feasible row at all and exercise the gate
only: tests/golden/tight.npz (27 events without a possible room) and syn
(2,000 events, 45 x 40 cells). Their feasible counterparts are tight_rooms
and syn_sparse (tests/lahc_model.py SHAPES); tests/test_lahc_cpu.py asserts
the feasible share of every other shape."""
import pathlib

import numpy as np
import pytest

import ttga
import lahc_model as lm
import walk_checks as wc
from helpers import host, json_lines
from stage_checks import GA, VARIANTS, both_drivers, run_driver, run_island
from walk_checks import BAD_GENE

pytestmark = pytest.mark.gpu

from ttga import native  # noqa: E402

REPO = pathlib.Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def problems():
    cache = {}

    def get(name):
        if name not in cache:
            inst = lm.SHAPES[name]()
            cache[name] = (inst, native.DeviceProblem(inst), lm.Model(inst))
        return cache[name]
    return get


def call(dp, a):
    return lambda s, r, g, **out: dp.lahc(s, r, g, a["steps"], a["history"], a["p_swap"], **out)


def rows(model, slot, room, seeds, a, infos=None):
    return model.lahc_rows(slot, room, seeds, a["steps"], a["history"], a["p_swap"], infos)


def check(problem, slot, room, seeds, steps, L, p_swap, infos=None):
    inst, dp, model = problem
    a = dict(steps=steps, history=L, p_swap=p_swap)
    want = rows(model, slot, room, seeds, a, infos)
    got, before, after, inplace = wc.run(dp, call(dp, a), slot, room, seeds)
    wc.check_rows(got, want, before, after, inplace, slot, room, seeds, steps)
    return got, want, before[0]


@pytest.mark.parametrize("cid", list(lm.CASES))
def test_rows_vs_model(problems, cid):
    shape, P, steps, L, p_swap = lm.CASES[cid]
    pb = problems(shape)
    inst, dp, model = pb
    slot, room, seeds = lm.population(inst, P, model)
    infos = []
    got, want, hcv0 = check(pb, slot, room, seeds, steps, L, p_swap, infos)
    searched = [i for i in infos if i]
    kinds = {k: sum(i[k] for i in searched) for k in ("move1", "move2", "both", "own_room")}
    print(cid, "feasible", int((hcv0 == 0).sum()), "of", P, "gain", int(got[3].sum()), "accepted", int(got[4].sum()), kinds)
    if shape in lm.NO_FEASIBLE_ROW:
        assert (hcv0 != 0).all()
        return
    assert 2 * int((hcv0 == 0).sum()) >= P
    assert P < 5 or (hcv0 != 0).any() or inst.E < 2                  # both kinds of rows in the launch
    if steps == 0:
        assert not got[4].any() and np.array_equal(got[0], slot) and np.array_equal(got[2], seeds)
        return
    wc.check_stream_advance(got, seeds, hcv0 != 0, 3 * steps)      # exactly 3 * steps draws a searched row
    if steps > 1:
        assert got[4].sum() > 0
    # what each shape is in the list for, asserted on the model's side
    if cid in ("E1", "p_swap0"):
        assert kinds["move2"] == 0 and kinds["move1"] > 0
    if cid == "p_swap1":
        assert kinds["move1"] == 0 and kinds["move2"] > 0
    if cid in ("E2", "E3"):
        assert kinds["move2"] > 0
    if cid == "S0":                                                 # delta is 0 everywhere
        assert not got[3].any() and got[4].sum() > 0
    if cid in ("sm-L50", "E3", "extremes"):                         # a student who attends both events of a swap
        assert kinds["both"] > 0
    if cid == "R1":                                                 # e1 can only take the room e2 leaves
        assert kinds["own_room"] > 0 and kinds["own_room"] == kinds["move2"]
    if cid == "R64":
        assert any((w == 63).any() for w in want[1]) and int(want[1][hcv0 == 0][:, 0].min()) == 63
    if cid == "extremes":
        full = [i for i in range(P) if hcv0[i] == 0]
        assert full and all(len(set(want[0][i][:45].tolist())) == 45 for i in full)
    if cid in ("sm-L50", "sm-L500", "med-L50", "med-L500"):
        # the best row came back, not the last current one
        restored = [k for k, i in enumerate(infos) if i and want[5][k] < steps
                    and not np.array_equal(i["cur_slot"], want[0][k])]
        assert restored
    if cid == "L3000":
        assert L > steps
    assert dp.status() & BAD_GENE == 0


def test_l1_p0_is_a_not_worse_walk(problems):
    """history 1 and p_swap 0 on the GPU: no accepted move ever raises the cost,
    so the exit row is the last current row and best_step is the last strict
    improvement; gain equals the fall of scv."""
    pb = problems("sm")
    inst, dp, model = pb
    slot, room, seeds = lm.population(inst, 16, model)
    infos = []
    got, want, hcv0 = check(pb, slot, room, seeds, 1500, 1, 0.0, infos)
    for k, i in enumerate(infos):
        if i:
            assert i["cur"] == i["scv0"] - want[3][k]                # the walk ended at its best cost


# ---------------------------------------------------------------- invalid genes, errors, the limit
OK = dict(steps=10, history=5, p_swap=0.5)


def test_invalid_genes():
    wc.invalid_genes(lm.Model, call, rows, dict(steps=500, history=50, p_swap=0.5))


def test_invalid_arguments_launch_nothing(problems):
    bad = (dict(steps=-1), dict(history=0), dict(history=-3), dict(p_swap=1.5), dict(p_swap=-0.1),
           dict(p_swap=float("nan")))
    wc.invalid_arguments_launch_nothing(problems("sm"), call, rows, OK, bad,
                                        lambda dp, s, r, g: dp.lahc(s, r, g, 200, 20))


def test_limit(problems):
    """sm takes 8 * (45 * 2 + 45 + 80) + 4 * 100 = 2,120 bytes without the history."""
    wc.lds_limit(problems("sm"), call, rows, OK, 2120)


# ---------------------------------------------------------------- Island
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_island_lahc(problems, variant):
    inst, dp, _ = problems("sm")
    kw = VARIANTS[variant]
    a = run_island(dp, lahc=500, init="greedy", **kw)
    b = run_island(dp, lahc=500, init="greedy", **kw)
    for k in a.pop:
        assert np.array_equal(host(a.pop[k]), host(b.pop[k])), k           # run twice: identical
    p = a.pop
    hcv, scv, feas, pen = (host(t) for t in dp.eval(p["slot"], p["room"]))
    assert np.array_equal(host(p["hcv"]), hcv) and np.array_equal(host(p["scv"]), scv)
    assert np.array_equal(host(p["feasible"]), feas) and np.array_equal(host(p["penalty"]), pen)
    st = a.lahc_stats()
    print(variant, st)
    assert set(st) == {"rows", "searched", "improved", "accepted", "gain"}
    assert st["rows"] == 10 + 30 * kw.get("children", 1)
    assert 0 < st["searched"] <= st["rows"] and st["gain"] > 0 and st["accepted"] >= st["improved"] > 0
    assert st["improved"] <= st["searched"]
    a.close()
    b.close()
    assert dp.status() & BAD_GENE == 0


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_island_lahc_0_issues_no_call(problems, variant, monkeypatch):
    inst, dp, _ = problems("sm")
    kw = VARIANTS[variant]
    plain = run_island(dp, gens=8, init="greedy", **kw)

    def boom(*a, **k):
        raise AssertionError("lahc called with Island(lahc=0)")
    monkeypatch.setattr(dp, "lahc", boom)
    off = run_island(dp, gens=8, init="greedy", lahc=0, **kw)
    for k in plain.pop:
        assert np.array_equal(host(off.pop[k]), host(plain.pop[k])), k
    with pytest.raises(ValueError, match="lahc_stats"):
        off.lahc_stats()
    off.close()
    plain.close()


# ---------------------------------------------------------------- the drivers
def test_lahc_in_both_drivers(tmp_path):
    tim = REPO / "tests" / "golden" / "sm.tim"
    inst = ttga.read_tim(tim)
    base = ["-i", str(tim), "-s", "29", "-p", "1", "--pop", "16", "--children", "8", "--generations", "10",
            "--init", "greedy"]
    flags = ["--lahc", "500", "--lahc-history", "100", "--lahc-swap", "0.25"]
    py, cc, a, lines = both_drivers(tmp_path, base, flags, "lahc", inst)
    cc_zero = run_driver([str(GA), *base, "--lahc", "0"], tmp_path)
    assert len(lines) == 1 and set(lines[0]) == {"accepted", "gain", "improved", "rows", "searched"}
    k = lines[0]
    assert k["rows"] == 16 + 80 and 0 < k["searched"] <= k["rows"] and k["gain"] > 0
    assert k["accepted"] >= k["improved"] > 0
    assert not any("lahc" in x for x in json_lines(cc_zero.stdout))                  # 0: no call, no line
