"""Every optional stage at once through both drivers: --init greedy, --unique,
--kempe, --slot-swap, --lahc and --crossover guided with repair, two islands,
sixty generations (the migration before generation 49 included), with the
batch and with the staggered schedule. python -m ttga.islands and ttga-ga
print the same lines (each island's logEntry lines in the same order; between
islands their order is the native driver's threads' and not fixed), the stage
lines byte for byte and in the documented order, and the stage lines count the
rows they should."""
import pathlib
import sys

import pytest

import ttga
from helpers import json_lines
from stage_checks import run_driver

pytestmark = pytest.mark.gpu

REPO = pathlib.Path(__file__).resolve().parent.parent
PKG = REPO / "timetabling-ga-mpi-openmp_amd"
STAGE_KINDS = ("crossover", "kempe", "unique", "slotSwap", "lahc")
ARGS = ["-s", "29", "-p", "1", "--pop", "16", "--children", "8", "--generations", "60", "--islands", "2",
        "--init", "greedy", "--unique", "--kempe", "0.5", "--kempe-max-chain", "4", "--slot-swap", "1",
        "--lahc", "200", "--lahc-history", "100", "--crossover", "guided", "--crossover-repair"]


def _per_island(lines):
    """Every line, in order, but for the order of the logEntry lines between
    islands: ttga-ga's islands are threads that log as their generations
    finish, so only each island's own logEntry lines have a fixed order."""
    logs, rest = {}, []
    for x in lines:
        if "logEntry" in x:
            logs.setdefault(x["logEntry"]["procID"], []).append(x)
        else:
            rest.append(x)
    return logs, rest


@pytest.mark.parametrize("stagger", [False, True], ids=["batch", "stagger"])
def test_all_stages_in_both_drivers(tmp_path, stagger):
    tim = REPO / "tests" / "golden" / "sm.tim"
    inst = ttga.read_tim(tim)
    exe = PKG / "ttga-ga"
    assert exe.exists(), "ttga-ga not built (make -C timetabling-ga-mpi-openmp_amd)"
    args = ["-i", str(tim), *ARGS, *(["--stagger"] if stagger else [])]
    py = run_driver([sys.executable, "-m", "ttga.islands", *args], tmp_path)
    cc = run_driver([str(exe), *args], tmp_path)
    a, b = json_lines(py.stdout), json_lines(cc.stdout)
    assert _per_island(a) == _per_island(b) and a

    def stage_lines(text):
        return [ln for ln in text.splitlines() if ln.startswith(tuple('{"%s"' % k for k in STAGE_KINDS))]
    assert stage_lines(py.stdout) == stage_lines(cc.stdout)             # byte for byte
    assert len(stage_lines(py.stdout)) == 2 * len(STAGE_KINDS)

    kinds = [next(iter(x)) for x in a]
    tail = [k for k in kinds if k in STAGE_KINDS + ("solution",)]
    assert tail == ["solution", "crossover", "kempe"] * 2 + ["unique"] * 2 + ["slotSwap"] * 2 + ["lahc"] * 2
    first = kinds.index("solution")
    assert kinds[first:] == tail + ["runEntry"] and "procsNum" in a[-1]["runEntry"]

    by_kind = {k: [x[k] for x in a if k in x] for k in STAGE_KINDS}
    for k in ("crossover", "kempe", "unique"):
        assert [x["children"] for x in by_kind[k]] == [480, 480], k
    for k in ("slotSwap", "lahc"):                  # island 0 alone runs initialize(): its 16 members too
        assert [x["rows"] for x in by_kind[k]] == [496, 480], k

    from ttga.validate import check_text
    for r_ in (py, cc):
        reps = check_text(inst, r_.stdout)
        assert reps and all(x["ok"] for x in reps), reps
