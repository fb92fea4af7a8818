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
import os
import pathlib
import subprocess
import sys

import numpy as np
import pytest

import ttga
import lahc_model as lm
from helpers import dev, host, json_lines

pytestmark = pytest.mark.gpu

import torch  # noqa: E402
from ttga import native  # noqa: E402
from ttga.ga import Island  # noqa: E402

REPO = pathlib.Path(__file__).resolve().parent.parent
PKG = REPO / "timetabling-ga-mpi-openmp_amd"
BAD_GENE = 256                                   # tt_device_status bit 8


@pytest.fixture(scope="module")
def problems():
    cache = {}

    def get(name):
        if name not in cache:
            inst = lm.SHAPES[name]()
            cache[name] = (inst, native.DeviceProblem(inst), lm.Model(inst))
        return cache[name]
    return get


def run(dp, slot, room, seeds, steps, L, p_swap, with_eval=True):
    """One call on numpy rows; returns the outputs and the evaluations around it."""
    P = slot.shape[0]
    s, r, g = dev(slot), dev(room), dev(seeds)
    before = [host(t) for t in dp.eval(s, r)] if with_eval else None
    scv = dev(before[1]) if with_eval else None
    pen = dev(before[3]) if with_eval else None
    out = [torch.full((P,), 12345, dtype=torch.int32, device="cuda") for _ in range(3)]
    dp.lahc(s, r, g, steps, L, p_swap, scv=scv, penalty=pen, gain=out[0], accepted=out[1], best_step=out[2])
    got = (host(s), host(r), host(g), host(out[0]), host(out[1]), host(out[2]))
    after = [host(t) for t in dp.eval(s, r)] if with_eval else None
    return got, before, after, (host(scv), host(pen)) if with_eval else None


NAMES = ("slot", "room", "rng", "gain", "accepted", "best_step")


def check(problem, slot, room, seeds, steps, L, p_swap, infos=None):
    inst, dp, model = problem
    P = slot.shape[0]
    want = model.lahc_rows(slot, room, seeds, steps, L, p_swap, infos)
    got, before, after, inplace = run(dp, slot, room, seeds, steps, L, p_swap)
    for name, g, w in zip(NAMES, got, want):
        diff = np.flatnonzero((g.reshape(P, -1) != w.reshape(P, -1)).any(axis=1))
        assert diff.size == 0, f"{name} differs in rows {diff[:8]}: gpu {g[diff[:2]]} model {w[diff[:2]]}"
    hcv0, scv0, feas0, pen0 = before
    hcv1, scv1, feas1, pen1 = after
    assert np.array_equal(hcv1, hcv0) and np.array_equal(feas1, feas0)
    assert np.array_equal(scv1, scv0 - got[3]) and (got[3] >= 0).all()
    assert np.array_equal(inplace[0], scv1) and np.array_equal(inplace[1], pen1)      # in place = a fresh tt_eval
    closed = hcv0 != 0                                                               # rows the gate keeps out
    assert np.array_equal(got[0][closed], slot[closed]) and np.array_equal(got[1][closed], room[closed])
    assert np.array_equal(got[2][closed], seeds[closed])
    assert not got[3][closed].any() and not got[4][closed].any() and not got[5][closed].any()
    assert (got[5] <= steps).all() and (got[4] <= steps).all()
    return got, want, hcv0


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
    # the streams of the searched rows advanced by exactly 3 * steps draws
    from ttga.rng import step
    i = int(np.flatnonzero(hcv0 == 0)[0])
    s = int(seeds[i])
    for _ in range(3 * steps):
        s = step(s)
    assert got[2][i] == s
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
def test_invalid_genes():
    """Rows with slot gene 45 / room gene R between valid ones: untouched, rng
    included, outputs 0, status bit 8; their neighbours walk as the model has
    them. Own handle: the status word is sticky."""
    inst = lm.SHAPES["sm"]()
    dp, model = native.DeviceProblem(inst), lm.Model(inst)
    slot, room, seeds = lm.population(inst, 6, model)
    slot[1, 7] = 45
    room[4, 3] = inst.R
    assert dp.status() == 0
    want = model.lahc_rows(slot, room, seeds, 500, 50, 0.5)
    got, _, _, _ = run(dp, slot, room, seeds, 500, 50, 0.5, with_eval=False)
    for name, g, w in zip(NAMES, got, want):
        assert np.array_equal(g, w), name
    for i in (1, 4):
        assert np.array_equal(got[0][i], slot[i]) and np.array_equal(got[1][i], room[i]) and got[2][i] == seeds[i]
        assert got[3][i] == got[4][i] == got[5][i] == 0
    assert got[4][0] > 0 and got[4][3] > 0 and got[4][5] > 0
    assert dp.status() & BAD_GENE == BAD_GENE
    dp.close()


def test_invalid_arguments_launch_nothing(problems):
    inst, dp, model = problems("sm")
    slot, room, seeds = lm.population(inst, 4, model)
    s, r, g = dev(slot), dev(room), dev(seeds)
    out = [torch.full((4,), 12345, dtype=torch.int32, device="cuda") for _ in range(5)]
    for kw in (dict(steps=-1, history=5), dict(steps=10, history=0), dict(steps=10, history=-3),
               dict(steps=10, history=5, p_swap=1.5), dict(steps=10, history=5, p_swap=-0.1),
               dict(steps=10, history=5, p_swap=float("nan"))):
        with pytest.raises(native.TTError) as ei:
            dp.lahc(s, r, g, kw["steps"], kw["history"], kw.get("p_swap", 0.5), scv=out[0], penalty=out[1], gain=out[2],
                    accepted=out[3], best_step=out[4])
        assert ei.value.code == native.TT_ERR_INVALID
    assert np.array_equal(host(s), slot) and np.array_equal(host(r), room) and np.array_equal(host(g), seeds)
    assert all((host(t) == 12345).all() for t in out)
    # every output NULL
    dp.lahc(s, r, g, 200, 20)
    want = model.lahc_rows(slot, room, seeds, 200, 20, 0.5)
    assert np.array_equal(host(s), want[0]) and np.array_equal(host(r), want[1]) and np.array_equal(host(g), want[2])


def test_limit(problems):
    """A history too long for the LDS: TT_ERR_LIMIT, every buffer untouched.
    sm takes 8 * (45 * 2 + 45 + 80) + 4 * 100 = 2,120 bytes without the history."""
    inst, dp, model = problems("sm")
    slot, room, seeds = lm.population(inst, 4, model)
    s, r, g = dev(slot), dev(room), dev(seeds)
    out = [torch.full((4,), 12345, dtype=torch.int32, device="cuda") for _ in range(5)]
    fits = (65536 - 2120) // 4
    with pytest.raises(native.TTError, match="too large") as ei:
        dp.lahc(s, r, g, 10, fits + 1, 0.5, scv=out[0], penalty=out[1], gain=out[2], accepted=out[3], best_step=out[4])
    assert ei.value.code == native.TT_ERR_LIMIT
    assert np.array_equal(host(s), slot) and np.array_equal(host(r), room) and np.array_equal(host(g), seeds)
    assert all((host(t) == 12345).all() for t in out)
    dp.lahc(s, r, g, 10, fits, 0.5, gain=out[2])                       # the largest history that fits
    assert np.array_equal(host(out[2]), model.lahc_rows(slot, room, seeds, 10, fits, 0.5)[3])


# ---------------------------------------------------------------- Island
def run_island(dp, gens=30, **kw):
    isl = Island(dp, pop_size=10, children=kw.pop("children", 1), max_steps=50, seed=31, **kw)
    isl.initialize()
    for _ in range(gens):
        isl.step()
    isl.flush()
    return isl


VARIANTS = {"batch": {}, "staggered": dict(schedule="staggered", parts=2, children=4), "unique": dict(unique=True),
            "slot_swap": dict(slot_swap=1)}


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
def _run(cmd, cwd):
    env = dict(os.environ, PYTHONPATH=str(PKG))
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=240, env=env, cwd=str(cwd))
    assert r.returncode == 0, r.stderr[-2000:]
    return r


def test_lahc_in_both_drivers(tmp_path):
    tim = REPO / "tests" / "golden" / "sm.tim"
    inst = ttga.read_tim(tim)
    exe = PKG / "ttga-ga"
    assert exe.exists(), "ttga-ga not built (make -C timetabling-ga-mpi-openmp_amd)"
    base = ["-i", str(tim), "-s", "29", "-p", "1", "--pop", "16", "--children", "8", "--generations", "10",
            "--init", "greedy"]
    flags = ["--lahc", "500", "--lahc-history", "100", "--lahc-swap", "0.25"]
    py = _run([sys.executable, "-m", "ttga.islands", *base, *flags], tmp_path)
    cc = _run([str(exe), *flags, *base], tmp_path)
    cc_zero = _run([str(exe), *base, "--lahc", "0"], tmp_path)
    a, b = json_lines(py.stdout), json_lines(cc.stdout)
    assert a == b and a
    assert [ln for ln in py.stdout.splitlines() if ln.startswith('{"lahc"')] == \
           [ln for ln in cc.stdout.splitlines() if ln.startswith('{"lahc"')]             # byte for byte
    lines = [x["lahc"] for x in a if "lahc" in x]
    assert len(lines) == 1 and set(lines[0]) == {"accepted", "gain", "improved", "rows", "searched"}
    k = lines[0]
    assert k["rows"] == 16 + 80 and 0 < k["searched"] <= k["rows"] and k["gain"] > 0
    assert k["accepted"] >= k["improved"] > 0
    kinds = [next(iter(x)) for x in a]
    assert kinds.index("lahc") > kinds.index("solution")
    assert not any("lahc" in x for x in json_lines(cc_zero.stdout))                  # 0: no call, no line
    from ttga.validate import check_text
    for r_ in (py, cc):
        reps = check_text(inst, r_.stdout)
        assert reps and all(x["ok"] for x in reps), reps
