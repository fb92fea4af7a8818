"""tt_lahc_kempe (include/ttga_lahc_kempe.h) on the GPU against
tests/lahc_kempe_model.py: slot, room, the rng state, gain, accepted, best_step
and the five Kempe counts bit for bit, feasible and infeasible rows mixed in one
launch, and around every call tt_eval: hcv 0, scv lower by exactly the gain,
the scv / penalty updated in place equal to a fresh evaluation. Then the call
without chains against tt_lahc, invalid genes and arguments, the LDS limit,
Island(lahc_kempe=...) and the two drivers with --lahc-kempe."""
import os
import pathlib
import subprocess
import sys

import numpy as np
import pytest

import ttga
import lahc_kempe_model as km
import lahc_model as lm
from helpers import dev, host, json_lines

pytestmark = pytest.mark.gpu

import torch  # noqa: E402
from ttga import native  # noqa: E402
from test_gpu_lahc import VARIANTS, run_island  # noqa: E402

REPO = pathlib.Path(__file__).resolve().parent.parent
PKG = REPO / "timetabling-ga-mpi-openmp_amd"
BAD_GENE = 256                                   # tt_device_status bit 8

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
NAMES = ("slot", "room", "rng", "gain", "accepted", "best_step", "kempe_stats")


@pytest.fixture(scope="module")
def problems():
    cache = {}

    def get(name):
        if name not in cache:
            inst = lm.SHAPES[name]()
            cache[name] = (inst, native.DeviceProblem(inst), km.Model(inst))
        return cache[name]
    return get


def run(dp, slot, room, seeds, steps, L, p_swap, p_kempe, cap, with_eval=True, call=None):
    """One call on numpy rows; returns the outputs and the evaluations around it."""
    P = slot.shape[0]
    s, r, g = dev(slot), dev(room), dev(seeds)
    before = [host(t) for t in dp.eval(s, r)] if with_eval else None
    scv = dev(before[1]) if with_eval else None
    pen = dev(before[3]) if with_eval else None
    out = [torch.full((P,), 12345, dtype=torch.int32, device="cuda") for _ in range(3)]
    stats = torch.full((P, 5), 12345, dtype=torch.int32, device="cuda")
    if call is None:
        dp.lahc_kempe(s, r, g, steps, L, p_swap, p_kempe, cap, scv=scv, penalty=pen, gain=out[0], accepted=out[1],
                      best_step=out[2], kempe_stats=stats)
    else:
        call(s, r, g, scv, pen, out)
    got = (host(s), host(r), host(g), host(out[0]), host(out[1]), host(out[2]), host(stats))
    after = [host(t) for t in dp.eval(s, r)] if with_eval else None
    return got, before, after, (host(scv), host(pen)) if with_eval else None


def check(problem, slot, room, seeds, steps, L, p_swap, p_kempe, cap, infos=None):
    inst, dp, model = problem
    P = slot.shape[0]
    want = model.lahc_kempe_rows(slot, room, seeds, steps, L, p_swap, p_kempe, cap, infos)
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
    # the streams of the searched rows advanced by exactly 3 * steps draws
    from ttga.rng import step
    i = int(np.flatnonzero(hcv0 == 0)[0])
    s = int(seeds[i])
    for _ in range(3 * steps):
        s = step(s)
    assert got[2][i] == s
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

    def plain(s, r, g, scv, pen, out):
        dp.lahc(s, r, g, 1000, 50, p_swap, scv=scv, penalty=pen, gain=out[0], accepted=out[1], best_step=out[2])
    a = run(dp, slot, room, seeds, 1000, 50, p_swap, 0.0, 3)
    b = run(dp, slot, room, seeds, 1000, 50, p_swap, 0.0, 0, call=plain)
    for name, x, y in zip(NAMES[:6], a[0], b[0]):
        assert np.array_equal(x, y), name
    assert not a[0][6].any() and a[0][4].sum() > 0
    assert np.array_equal(a[3][0], b[3][0]) and np.array_equal(a[3][1], b[3][1])          # scv and penalty in place


# ---------------------------------------------------------------- invalid genes, errors, the limit
def test_invalid_genes():
    """Rows with slot gene 45 / room gene R between valid ones: untouched, rng
    included, outputs 0, status bit 8; their neighbours walk as the model has
    them. Own handle: the status word is sticky."""
    inst = lm.SHAPES["sm"]()
    dp, model = native.DeviceProblem(inst), km.Model(inst)
    slot, room, seeds = lm.population(inst, 6, model)
    slot[1, 7] = 45
    room[4, 3] = inst.R
    assert dp.status() == 0
    want = model.lahc_kempe_rows(slot, room, seeds, 500, 50, 0.25, 0.5)
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
    stats = torch.full((4, 5), 12345, dtype=torch.int32, device="cuda")
    ok = dict(steps=10, history=5, p_swap=0.25, p_kempe=0.5, max_chain=0)
    for kw in (dict(steps=-1), dict(history=0), dict(history=-3), dict(p_swap=1.5, p_kempe=0.0), dict(p_swap=-0.1),
               dict(p_swap=float("nan")), dict(p_kempe=1.5, p_swap=0.0), dict(p_kempe=-0.1),
               dict(p_kempe=float("nan")), dict(max_chain=-1), dict(p_swap=0.75, p_kempe=0.5),
               dict(p_swap=0.25, p_kempe=1.0)):
        a = {**ok, **kw}
        with pytest.raises(native.TTError) as ei:
            dp.lahc_kempe(s, r, g, a["steps"], a["history"], a["p_swap"], a["p_kempe"], a["max_chain"], scv=out[0],
                          penalty=out[1], gain=out[2], accepted=out[3], best_step=out[4], kempe_stats=stats)
        assert ei.value.code == native.TT_ERR_INVALID, kw
    assert np.array_equal(host(s), slot) and np.array_equal(host(r), room) and np.array_equal(host(g), seeds)
    assert all((host(t) == 12345).all() for t in out + [stats])
    # every output NULL
    dp.lahc_kempe(s, r, g, 200, 20, 0.25, 0.5)
    want = model.lahc_kempe_rows(slot, room, seeds, 200, 20, 0.25, 0.5)
    assert np.array_equal(host(s), want[0]) and np.array_equal(host(r), want[1]) and np.array_equal(host(g), want[2])


def test_limit(problems):
    """A history too long for the LDS: TT_ERR_LIMIT, every buffer untouched.
    The header's formula for sm (E 100, S 80) without the history:
    8 * (47 * 2 + 45 + 80) + 4 * 100 + 1,168 = 3,320 bytes."""
    inst, dp, model = problems("sm")
    slot, room, seeds = lm.population(inst, 4, model)
    s, r, g = dev(slot), dev(room), dev(seeds)
    out = [torch.full((4,), 12345, dtype=torch.int32, device="cuda") for _ in range(5)]
    stats = torch.full((4, 5), 12345, dtype=torch.int32, device="cuda")
    fits = (65536 - 3320) // 4
    with pytest.raises(native.TTError, match="too large") as ei:
        dp.lahc_kempe(s, r, g, 10, fits + 1, 0.25, 0.5, 0, scv=out[0], penalty=out[1], gain=out[2], accepted=out[3],
                      best_step=out[4], kempe_stats=stats)
    assert ei.value.code == native.TT_ERR_LIMIT
    assert np.array_equal(host(s), slot) and np.array_equal(host(r), room) and np.array_equal(host(g), seeds)
    assert all((host(t) == 12345).all() for t in out + [stats])
    dp.lahc_kempe(s, r, g, 10, fits, 0.25, 0.5, 0, gain=out[2], kempe_stats=stats)   # the largest history that fits
    want = model.lahc_kempe_rows(slot, room, seeds, 10, fits, 0.25, 0.5)
    assert np.array_equal(host(out[2]), want[3]) and np.array_equal(host(stats), want[6])


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
def _run(cmd, cwd):
    env = dict(os.environ, PYTHONPATH=str(PKG))
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=240, env=env, cwd=str(cwd))
    assert r.returncode == 0, r.stderr[-2000:]
    return r


def _lines(text, key):
    return [ln for ln in text.splitlines() if ln.startswith('{"%s"' % key)]


def test_lahc_kempe_in_both_drivers(tmp_path):
    tim = REPO / "tests" / "golden" / "sm.tim"
    inst = ttga.read_tim(tim)
    exe = PKG / "ttga-ga"
    assert exe.exists(), "ttga-ga not built (make -C timetabling-ga-mpi-openmp_amd)"
    base = ["-i", str(tim), "-s", "29", "-p", "1", "--pop", "16", "--children", "8", "--generations", "10",
            "--init", "greedy"]
    flags = ["--lahc", "500", "--lahc-history", "100", "--lahc-swap", "0.25", "--lahc-kempe", "0.5",
             "--lahc-kempe-max-chain", "8"]
    py = _run([sys.executable, "-m", "ttga.islands", *base, *flags], tmp_path)
    cc = _run([str(exe), *flags, *base], tmp_path)
    a, b = json_lines(py.stdout), json_lines(cc.stdout)
    assert a == b and a
    assert _lines(py.stdout, "lahcKempe") == _lines(cc.stdout, "lahcKempe")               # byte for byte
    assert _lines(py.stdout, "lahc") == _lines(cc.stdout, "lahc")
    lines = [x["lahcKempe"] for x in a if "lahcKempe" in x]
    assert len(lines) == 1 and set(lines[0]) == {"tried", "capped", "noRoom", "accepted", "meanChain"}
    k = lines[0]
    walk = [x["lahc"] for x in a if "lahc" in x]
    assert len(walk) == 1 and set(walk[0]) == {"accepted", "gain", "improved", "rows", "searched"}
    assert 0 < k["accepted"] <= k["tried"] - k["capped"] - k["noRoom"] and 1.0 <= k["meanChain"] <= 8.0
    assert k["accepted"] <= walk[0]["accepted"] and walk[0]["rows"] == 16 + 80
    kinds = [next(iter(x)) for x in a]
    assert kinds.index("lahcKempe") == kinds.index("lahc") + 1 > kinds.index("solution")
    from ttga.validate import check_text
    for r_ in (py, cc):
        reps = check_text(inst, r_.stdout)
        assert reps and all(x["ok"] for x in reps), reps


def test_all_stages_with_lahc_kempe_in_both_drivers(tmp_path):
    """tests/test_gpu_all_stages.py's run, batch schedule, with --lahc-kempe on too."""
    from test_gpu_all_stages import ARGS, STAGE_KINDS, _per_island
    kinds_all = STAGE_KINDS + ("lahcKempe",)
    tim = REPO / "tests" / "golden" / "sm.tim"
    inst = ttga.read_tim(tim)
    exe = PKG / "ttga-ga"
    args = ["-i", str(tim), *ARGS, "--lahc-swap", "0.25", "--lahc-kempe", "0.5", "--lahc-kempe-max-chain", "6"]
    py = _run([sys.executable, "-m", "ttga.islands", *args], tmp_path)
    cc = _run([str(exe), *args], tmp_path)
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
