"""Island(move1_descent=N) and --move1-descent in both drivers: the small
run of the walk-family modules (one island: between islands the order of the
native driver's logEntry lines is its threads') with --lahc 200 --move1-descent 4.
python -m ttga.islands and ttga-ga print the same lines, the move1Descent line
byte for byte and in the documented place (behind the lahc line, in front of
the report lines); its rows are the lahc line's; every member's penalty is a
fresh tt_eval's; Island(move1_descent=0) is the island without the keyword;
and python -m ttga.move1 on the run's output agrees with tests/move1_model.py
for the printed timetables."""
import json
import pathlib
import sys

import numpy as np
import pytest

import ttga
import lahc_model as lm
import move1_model as mm
from helpers import host, json_lines
from stage_checks import GA, PKG, VARIANTS, both_drivers, run_driver, run_island, stage_lines

pytestmark = pytest.mark.gpu

import torch  # noqa: E402,F401
from ttga import native  # noqa: E402

REPO = pathlib.Path(__file__).resolve().parent.parent
TIM = REPO / "tests" / "golden" / "sm.tim"
BASE = ["-i", str(TIM), "-s", "29", "-p", "1", "--pop", "16", "--children", "8", "--generations", "10", "--init", "greedy",
        "--report"]
FLAGS = ["--lahc", "200", "--lahc-history", "100", "--move1-descent", "4"]


@pytest.fixture(scope="module")
def sm():
    inst = lm.SHAPES["sm"]()
    return inst, native.DeviceProblem(inst)


@pytest.fixture(scope="module")
def driver_run(tmp_path_factory):
    inst = ttga.read_tim(TIM)
    tmp = tmp_path_factory.mktemp("move1_drivers")
    py, cc, a, lines = both_drivers(tmp, BASE, FLAGS, "move1Descent", inst)
    return inst, tmp, py, cc, a, lines


def test_line_in_both_drivers(driver_run):
    inst, tmp, py, cc, a, lines = driver_run
    assert len(lines) == 1 and all(set(k) == {"gain", "improved", "meanPasses", "rows"} for k in lines)
    assert stage_lines(py.stdout, "move1Descent") == stage_lines(cc.stdout, "move1Descent")      # byte for byte
    lahc = [x["lahc"] for x in a if "lahc" in x]
    assert [k["rows"] for k in lines] == [x["rows"] for x in lahc] == [16 + 80]      # the members too
    for k in lines:
        assert 0 < k["improved"] <= k["rows"] and k["gain"] >= k["improved"]
        assert 1.0 <= k["meanPasses"] <= 4.0
    kinds = [next(iter(x)) for x in a]
    tail = kinds[kinds.index("solution"):]
    assert tail == ["solution", "lahc", "move1Descent", "report", "runEntry"], tail


def test_flag_0_prints_no_line_and_changes_nothing(driver_run):
    inst, tmp, py, cc, a, lines = driver_run
    walk = [f for f in FLAGS if f not in ("--move1-descent", "4")]
    zero = run_driver([str(GA), *walk, "--move1-descent", "0", *BASE], tmp)
    plain = run_driver([str(GA), *walk, *BASE], tmp)
    assert not any("move1Descent" in x for x in json_lines(zero.stdout))
    assert json_lines(zero.stdout) == json_lines(plain.stdout)
    pz = run_driver([sys.executable, "-m", "ttga.islands", *BASE, *walk, "--move1-descent", "0"], tmp)
    assert json_lines(pz.stdout) == json_lines(zero.stdout)


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_island_move1_descent(sm, variant):
    inst, dp = sm
    kw = VARIANTS[variant]
    a = run_island(dp, lahc=200, lahc_history=100, move1_descent=4, init="greedy", **kw)
    b = run_island(dp, lahc=200, lahc_history=100, move1_descent=4, init="greedy", **kw)
    for k in a.pop:
        assert np.array_equal(host(a.pop[k]), host(b.pop[k])), k           # run twice: identical
    p = a.pop
    hcv, scv, feas, pen = (host(t) for t in dp.eval(p["slot"], p["room"]))
    assert np.array_equal(host(p["hcv"]), hcv) and np.array_equal(host(p["scv"]), scv)
    assert np.array_equal(host(p["feasible"]), feas) and np.array_equal(host(p["penalty"]), pen)
    st = a.move1_descent_stats()
    print(variant, st)
    assert list(st) == ["rows", "improved", "meanPasses", "gain"] and "move1_descent" in a.on
    assert st["rows"] == a.lahc_stats()["rows"] == 10 + 30 * kw.get("children", 1)
    assert 0 < st["improved"] <= st["rows"] and st["gain"] >= st["improved"] and 1.0 <= st["meanPasses"] <= 4.0
    a.close()
    b.close()
    assert dp.status() & 1024 == 0


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_island_move1_descent_0_issues_no_call(sm, variant, monkeypatch):
    inst, dp = sm
    kw = VARIANTS[variant]
    plain = run_island(dp, gens=8, init="greedy", lahc=100, **kw)

    def boom(*a, **k):
        raise AssertionError("move1_descent called with Island(move1_descent=0)")
    monkeypatch.setattr(dp, "move1_descent", boom)
    off = run_island(dp, gens=8, init="greedy", lahc=100, move1_descent=0, **kw)
    for k in plain.pop:
        assert np.array_equal(host(off.pop[k]), host(plain.pop[k])), k
    for name in ("rng_init", "rng_child"):
        assert np.array_equal(host(getattr(off, name)), host(getattr(plain, name))), name
    assert "move1_descent" not in off.on
    with pytest.raises(ValueError, match="move1_descent_stats"):
        off.move1_descent_stats()
    off.close()
    plain.close()


@pytest.mark.parametrize("event", [None, 7])
def test_move1_tool_on_the_run_s_output(driver_run, event):
    inst, tmp, py, cc, a, lines = driver_run
    out = tmp / "run.jsonl"
    out.write_text(cc.stdout)
    extra = [] if event is None else ["--event", str(event)]
    r = run_driver([sys.executable, "-m", "ttga.move1", str(TIM), str(out), *extra], tmp)
    got = [json.loads(ln)["move1"] for ln in r.stdout.splitlines() if ln.startswith('{"move1"')]
    sols = [x["solution"] for x in a if "solution" in x and x["solution"]["feasible"]]
    assert len(got) == len(sols) == 1
    model = mm.Model(inst)
    for g, sol in zip(got, sols):
        slot, room = np.array(sol["timeslots"], np.uint8), np.array(sol["rooms"], np.uint8)
        sm_, d, tr = model.scan(slot, room)
        assert sm_[0] == 1 and g["procID"] == sol["procID"]
        assert [g[k] for k in ("feasibleMoves", "improving", "bestDelta", "bestEvent", "bestSlot")] == sm_[1:].tolist()
        if event is None:
            assert set(g) == {"procID", "feasibleMoves", "improving", "bestDelta", "bestEvent", "bestSlot"}
        else:
            assert g["event"] == event and g["d_scv"] == d[event].tolist() and g["to_room"] == tr[event].tolist()
    # no feasible solution line: exit status 1
    empty = tmp / "empty.jsonl"
    empty.write_text('{"runEntry":{"procsNum":1}}\n')
    import os
    import subprocess
    env = dict(os.environ, PYTHONPATH=str(PKG))
    assert subprocess.run([sys.executable, "-m", "ttga.move1", str(TIM), str(empty)], env=env, timeout=120).returncode == 1
