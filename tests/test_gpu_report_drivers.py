"""--report in both GA drivers (python -m ttga.islands, ttga-ga): the same
report lines from both, nothing else changed in the output, and the best
member's parts reproduce the solution line."""
import pathlib
import subprocess
import sys

import pytest

import ttga
from helpers import json_lines as _json_lines
from stage_checks import run_driver
from ttga import native, validate

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

REPO = pathlib.Path(__file__).resolve().parent.parent
PKG = REPO / "timetabling-ga-mpi-openmp_amd"


def _raw_report_lines(text):
    return [ln for ln in text.splitlines() if ln.startswith('{"report"')]


@pytest.mark.parametrize("extra", [[], ["--stagger"]], ids=["batch", "stagger"])
def test_report_lines_of_both_drivers(tmp_path, extra):
    inst = ttga.config_instance("sm")
    tim = tmp_path / "sm.tim"
    ttga.write_tim(inst, tim)
    exe = PKG / "ttga-ga"
    assert exe.exists(), "ttga-ga not built (make -C timetabling-ga-mpi-openmp_amd)"
    base = ["-i", str(tim), "-s", "42", "-p", "1", "-c", "3", "--generations", "120", "--pop", "12", *extra]
    py = run_driver([sys.executable, "-m", "ttga.islands", *base, "--report"], tmp_path)
    cc = run_driver([str(exe), "--report", *base], tmp_path)
    plain = run_driver([str(exe), *base], tmp_path)

    # the report lines are the same bytes from both drivers; the rest of the output is
    # the run without the flag
    assert _raw_report_lines(py.stdout) == _raw_report_lines(cc.stdout)
    a, b = _json_lines(py.stdout), _json_lines(cc.stdout)
    assert a == b
    reports = [x["report"] for x in b if "report" in x]
    assert len(reports) == 1 and reports[0]["procID"] == 0 and reports[0]["island"] == 0
    assert [x for x in b if "report" not in x] == _json_lines(plain.stdout)
    keys = [next(iter(x)) for x in b]
    assert keys.index("report") == keys.index("solution") + 1 and keys[-1] == "runEntry"

    # the best member's parts against the solution line (ga.cpp:189-193)
    rep = reports[0]
    sol = [x["solution"] for x in b if "solution" in x][0]
    best = [rep["best"][k] for k in native.PART_NAMES]
    hard, soft = sum(best[:3]), sum(best[3:])
    assert sol["feasible"] == (hard == 0)
    assert sol["totalBest"] == (soft if sol["feasible"] else 1000000 * hard + soft)
    if "timeslots" in sol:
        ev = validate.evaluate(inst, sol["timeslots"], sol["rooms"])
        assert rep["best"] == {k: ev[k] for k in native.PART_NAMES}
    popu = rep["population"]
    assert popu["size"] == 12 and popu["invalid"] == 0 and 0 <= popu["feasible"] <= 12
    assert all(popu["nonzero"][k] <= 12 and popu["sum"][k] >= rep["best"][k] for k in native.PART_NAMES)
    assert rep["diversity"]["events"] == inst.E and rep["diversity"]["size"] == 12
    assert 0 <= rep["diversity"]["pairs_differing"] <= inst.E * 12 * 11 // 2

    # the validators skip the report line
    reps = validate.check_text(inst, cc.stdout)
    assert reps and all(r["ok"] for r in reps), reps
    out = subprocess.run([str(PKG / "ttga-check"), str(tim), "-"], input=cc.stdout, capture_output=True, text=True,
                         timeout=60)
    assert out.returncode == 0, out.stdout
