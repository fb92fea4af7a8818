"""tt_lahc_kempe_aug (include/ttga_lahc_kempe_aug.h) on the GPU against
tests/lahc_kempe_aug_model.py: slot, room, the rng state, gain, accepted,
best_step and the seven Kempe counts bit for bit, feasible and spoiled rows
mixed in one launch, and around every call tt_eval: hcv unchanged, scv lower by
exactly the gain, the scv / penalty updated in place equal to a fresh
evaluation. Then the calls that must equal tt_lahc_kempe and tt_lahc, invalid
genes and arguments, the LDS limit, Island(lahc_kempe_rooms="augment") and the
two drivers with --lahc-kempe-rooms augment."""
import os
import pathlib
import subprocess
import sys

import numpy as np
import pytest

import ttga
import lahc_kempe_aug_model as am
import lahc_model as lm
from helpers import dev, host, json_lines

pytestmark = pytest.mark.gpu

import torch  # noqa: E402
from ttga import native  # noqa: E402
from test_gpu_lahc import VARIANTS, run_island  # noqa: E402

REPO = pathlib.Path(__file__).resolve().parent.parent
PKG = REPO / "timetabling-ga-mpi-openmp_amd"
BAD_GENE = 256                                   # tt_device_status bit 8

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
NAMES = ("slot", "room", "rng", "gain", "accepted", "best_step", "kempe_stats")


@pytest.fixture(scope="module")
def problems():
    cache = {}

    def get(name):
        if name not in cache:
            inst = SHAPES[name]()
            cache[name] = (inst, native.DeviceProblem(inst), am.Model(inst))
        return cache[name]
    return get


def run(dp, slot, room, seeds, steps, L, p_swap, p_kempe, cap, rule=1, with_eval=True, call=None, width=7):
    """One call on numpy rows; returns the outputs and the evaluations around it."""
    P = slot.shape[0]
    s, r, g = dev(slot), dev(room), dev(seeds)
    before = [host(t) for t in dp.eval(s, r)] if with_eval else None
    scv = dev(before[1]) if with_eval else None
    pen = dev(before[3]) if with_eval else None
    out = [torch.full((P,), 12345, dtype=torch.int32, device="cuda") for _ in range(3)]
    stats = torch.full((P, width), 12345, dtype=torch.int32, device="cuda")
    if call is None:
        dp.lahc_kempe_aug(s, r, g, steps, L, p_swap, p_kempe, cap, rule, scv=scv, penalty=pen, gain=out[0],
                          accepted=out[1], best_step=out[2], kempe_stats=stats)
    else:
        call(s, r, g, scv, pen, out, stats)
    got = (host(s), host(r), host(g), host(out[0]), host(out[1]), host(out[2]), host(stats))
    after = [host(t) for t in dp.eval(s, r)] if with_eval else None
    return got, before, after, (host(scv), host(pen)) if with_eval else None


def check(problem, slot, room, seeds, steps, L, p_swap, p_kempe, cap, infos=None):
    inst, dp, model = problem
    P = slot.shape[0]
    want = model.lahc_kempe_aug_rows(slot, room, seeds, steps, L, p_swap, p_kempe, cap, 1, infos)
    got, before, after, inplace = run(dp, slot, room, seeds, steps, L, p_swap, p_kempe, cap)
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
    assert not got[6][closed].any()
    assert (got[5] <= steps).all() and (got[4] <= steps).all()
    st = got[6].astype(np.int64)
    assert (st[:, 3] <= st[:, 0] - st[:, 1] - st[:, 2]).all() and (st[:, 3] <= got[4]).all()
    assert (st[:, 5] <= st[:, 0] - st[:, 1] - st[:, 2]).all()
    return got, want, hcv0


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
    from ttga.rng import step
    i = int(np.flatnonzero(hcv0 == 0)[0])                           # exactly 3 * steps draws
    s = int(seeds[i])
    for _ in range(3 * steps):
        s = step(s)
    assert got[2][i] == s
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
def kempe_call(dp, steps, L, p_swap, p_kempe, cap):
    def call(s, r, g, scv, pen, out, stats):
        dp.lahc_kempe(s, r, g, steps, L, p_swap, p_kempe, cap, scv=scv, penalty=pen, gain=out[0], accepted=out[1],
                      best_step=out[2], kempe_stats=stats)
    return call


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
    a = run(dp, slot, room, seeds, 1000, 50, 0.25, 0.5, 0, 1)
    b = run(dp, slot, room, seeds, 1000, 50, 0.25, 0.5, 0, call=kempe_call(dp, 1000, 50, 0.25, 0.5, 0), width=5)
    same_as_lahc_kempe(a, b)
    assert a[0][6][:, 2].sum() > 0                                   # and chains without a room there are


@pytest.mark.parametrize("p_swap", [0.0, 0.25])
def test_room_rule_0_is_tt_lahc_kempe(problems, p_swap):
    inst, dp, model = problems("sm")
    slot, room, seeds = lm.population(inst, 33, model)
    a = run(dp, slot, room, seeds, 1000, 50, p_swap, 0.5, 0, 0)
    b = run(dp, slot, room, seeds, 1000, 50, p_swap, 0.5, 0, call=kempe_call(dp, 1000, 50, p_swap, 0.5, 0), width=5)
    same_as_lahc_kempe(a, b)
    assert a[0][6][:, 2].sum() > 0


def test_without_chains_the_call_is_tt_lahc(problems):
    inst, dp, model = problems("sm")
    slot, room, seeds = lm.population(inst, 33, model)

    def plain(s, r, g, scv, pen, out, stats):
        dp.lahc(s, r, g, 1000, 50, 0.5, scv=scv, penalty=pen, gain=out[0], accepted=out[1], best_step=out[2])
    a = run(dp, slot, room, seeds, 1000, 50, 0.5, 0.0, 3, 1)
    b = run(dp, slot, room, seeds, 1000, 50, 0.5, 0.0, 0, call=plain)
    for name, x, y in zip(NAMES[:6], a[0], b[0]):
        assert np.array_equal(x, y), name
    assert not a[0][6].any() and a[0][4].sum() > 0
    assert np.array_equal(a[3][0], b[3][0]) and np.array_equal(a[3][1], b[3][1])


# ---------------------------------------------------------------- invalid genes, errors, the limit
def test_invalid_genes():
    """Rows with slot gene 45 / room gene R between valid ones: untouched, rng
    included, outputs 0, status bit 8; their neighbours walk as the model has
    them. Own handle: the status word is sticky."""
    inst = lm.SHAPES["sm"]()
    dp, model = native.DeviceProblem(inst), am.Model(inst)
    slot, room, seeds = lm.population(inst, 6, model)
    slot[1, 7] = 45
    room[4, 3] = inst.R
    assert dp.status() == 0
    want = model.lahc_kempe_aug_rows(slot, room, seeds, 500, 50, 0.25, 0.5)
    got, _, _, _ = run(dp, slot, room, seeds, 500, 50, 0.25, 0.5, 0, with_eval=False)
    for name, g, w in zip(NAMES, got, want):
        assert np.array_equal(g, w), name
    for i in (1, 4):
        assert np.array_equal(got[0][i], slot[i]) and np.array_equal(got[1][i], room[i]) and got[2][i] == seeds[i]
        assert got[3][i] == got[4][i] == got[5][i] == 0 and not got[6][i].any()
    assert got[4][0] > 0 and got[4][3] > 0 and got[4][5] > 0
    assert dp.status() & BAD_GENE == BAD_GENE
    dp.close()


def test_invalid_arguments_launch_nothing(problems):
    inst, dp, model = problems("sm")
    slot, room, seeds = lm.population(inst, 4, model)
    s, r, g = dev(slot), dev(room), dev(seeds)
    out = [torch.full((4,), 12345, dtype=torch.int32, device="cuda") for _ in range(5)]
    stats = torch.full((4, 7), 12345, dtype=torch.int32, device="cuda")
    ok = dict(steps=10, history=5, p_swap=0.25, p_kempe=0.5, max_chain=0, room_rule=1)
    for kw in (dict(room_rule=-1), dict(room_rule=2), dict(steps=-1), dict(history=0), dict(history=-3),
               dict(p_swap=1.5, p_kempe=0.0), dict(p_swap=-0.1), dict(p_swap=float("nan")),
               dict(p_kempe=1.5, p_swap=0.0), dict(p_kempe=-0.1), dict(p_kempe=float("nan")), dict(max_chain=-1),
               dict(p_swap=0.75, p_kempe=0.5), dict(p_swap=0.25, p_kempe=1.0)):
        a = {**ok, **kw}
        with pytest.raises(native.TTError) as ei:
            dp.lahc_kempe_aug(s, r, g, a["steps"], a["history"], a["p_swap"], a["p_kempe"], a["max_chain"],
                              a["room_rule"], scv=out[0], penalty=out[1], gain=out[2], accepted=out[3], best_step=out[4],
                              kempe_stats=stats)
        assert ei.value.code == native.TT_ERR_INVALID, kw
    assert np.array_equal(host(s), slot) and np.array_equal(host(r), room) and np.array_equal(host(g), seeds)
    assert all((host(t) == 12345).all() for t in out + [stats])
    # every output NULL
    dp.lahc_kempe_aug(s, r, g, 200, 20, 0.25, 0.5)
    want = model.lahc_kempe_aug_rows(slot, room, seeds, 200, 20, 0.25, 0.5)
    assert np.array_equal(host(s), want[0]) and np.array_equal(host(r), want[1]) and np.array_equal(host(g), want[2])


def test_limit(problems):
    """A history too long for the LDS: TT_ERR_LIMIT, every buffer untouched.
    The header's formula for sm (E 100, S 80) without the history:
    8 * (47 * 2 + 45 + 80) + 4 * 100 + 1,552 = 3,704 bytes."""
    inst, dp, model = problems("sm")
    slot, room, seeds = lm.population(inst, 4, model)
    s, r, g = dev(slot), dev(room), dev(seeds)
    out = [torch.full((4,), 12345, dtype=torch.int32, device="cuda") for _ in range(5)]
    stats = torch.full((4, 7), 12345, dtype=torch.int32, device="cuda")
    assert 8 * (47 * 2 + 45 + 80) + 4 * 100 + 1552 == 3704
    fits = (65536 - 3704) // 4
    with pytest.raises(native.TTError, match="too large") as ei:
        dp.lahc_kempe_aug(s, r, g, 300, fits + 1, 0.25, 0.5, 0, 1, scv=out[0], penalty=out[1], gain=out[2],
                          accepted=out[3], best_step=out[4], kempe_stats=stats)
    assert ei.value.code == native.TT_ERR_LIMIT
    assert np.array_equal(host(s), slot) and np.array_equal(host(r), room) and np.array_equal(host(g), seeds)
    assert all((host(t) == 12345).all() for t in out + [stats])
    # the largest history that fits: the search's state is the last of the image
    dp.lahc_kempe_aug(s, r, g, 300, fits, 0.25, 0.5, 0, 1, gain=out[2], kempe_stats=stats)
    want = model.lahc_kempe_aug_rows(slot, room, seeds, 300, fits, 0.25, 0.5)
    assert np.array_equal(host(s), want[0]) and np.array_equal(host(r), want[1])
    assert np.array_equal(host(out[2]), want[3]) and np.array_equal(host(stats), want[6])
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
def _run(cmd, cwd):
    env = dict(os.environ, PYTHONPATH=str(PKG))
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=240, env=env, cwd=str(cwd))
    assert r.returncode == 0, r.stderr[-2000:]
    return r


def _lines(text, key):
    return [ln for ln in text.splitlines() if ln.startswith('{"%s"' % key)]


def test_augment_in_both_drivers(tmp_path):
    tim = REPO / "tests" / "golden" / "sm.tim"
    inst = ttga.read_tim(tim)
    exe = PKG / "ttga-ga"
    assert exe.exists(), "ttga-ga not built (make -C timetabling-ga-mpi-openmp_amd)"
    base = ["-i", str(tim), "-s", "29", "-p", "1", "--pop", "16", "--children", "8", "--generations", "10",
            "--init", "greedy"]
    flags = ["--lahc", "500", "--lahc-swap", "0.25", "--lahc-kempe", "0.5", "--lahc-kempe-rooms", "augment"]
    py = _run([sys.executable, "-m", "ttga.islands", *base, *flags], tmp_path)
    cc = _run([str(exe), *flags, *base], tmp_path)
    a, b = json_lines(py.stdout), json_lines(cc.stdout)
    assert a == b and a
    assert _lines(py.stdout, "lahcKempe") == _lines(cc.stdout, "lahcKempe")               # byte for byte
    assert _lines(py.stdout, "lahc") == _lines(cc.stdout, "lahc")
    lines = [x["lahcKempe"] for x in a if "lahcKempe" in x]
    assert len(lines) == 1
    k = lines[0]
    assert set(k) == {"tried", "capped", "noRoom", "accepted", "meanChain", "rescued", "displaced"}
    assert 0 < k["accepted"] <= k["tried"] - k["capped"] - k["noRoom"] and k["rescued"] > 0 and k["displaced"] >= 0
    from ttga.validate import check_text
    for r_ in (py, cc):
        reps = check_text(inst, r_.stdout)
        assert reps and all(x["ok"] for x in reps), reps
