"""eval_tile5's lane phase -- a student's mask built as 32 << slot and its scv
terms taken from the two words (mask_scv_shift5) -- against the CPU oracle:
tt_eval variants 7 and 8, all four outputs, exact equality.

The golden instances sm at P = 65 (one full tile and a one-row tile) and med at
P = 130 (three tiles: the persistent loop's second and third tiles and both tile
buffers). Rows crafted by student_terms_cases put the largest student and an
odd-sized one (its id list ends in the sentinel column, slot byte 63) on the
edges of the form -- a whole day in consecutive slots, a run across a day
boundary, the day that straddles bit 32 of the plain mask (the first of the high
word here), slot 44, one event per day, every event in one slot, no event on
four days -- in the tile's first, last and middle lanes and in the short last
tile; one row carries an invalid slot byte (sentinel outputs, its neighbours
unaffected). A window counted across two days or two words, a field's top slot
lost or counted twice, or a sentinel that leaves a bit changes some row's scv.
A third problem gives one student 40 events: the plain loop for more than 32
ids (plain mask, mask_scv) still serves it beside the others.
Reference: Solution.cpp:63-170.
"""
import numpy as np
import pytest

from helpers import dev, host
from oracle_lib import oracle
from student_terms_cases import craft, golden_instance, spread_rows, with_long_student

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from ttga import native  # noqa: E402

NAMES = ("hcv", "scv", "feasible", "penalty")
CASES = {"sm": ("sm", 65, False), "med": ("med", 130, False), "sm_long_student": ("sm", 65, True)}

_cache = {}


def _problem(case, golden_dir):
    """device problem, population and expected outputs (built once, not modified afterwards)"""
    if case not in _cache:
        name, P, long_student = CASES[case]
        inst = golden_instance(golden_dir, name)
        if long_student:
            inst = with_long_student(inst)
        o = oracle().problem(inst)
        slots, _ = craft(inst, P, 4100 + P, spread_rows(P))
        rooms = o.assign_rooms(slots)
        exp = [a.copy() for a in o.eval(slots, rooms)]
        invalid = 33                                   # between two crafted rows of the first tile
        slots[invalid, int(np.flatnonzero(inst.student_events[0])[0])] = 200
        exp[0][invalid] = exp[1][invalid] = exp[3][invalid] = -1
        exp[2][invalid] = 0
        _cache[case] = dict(dp=native.DeviceProblem(inst), slots=slots, rooms=rooms, exp=exp)
    return _cache[case]


@pytest.mark.parametrize("variant", [7, 8], ids=["v7", "v8"])
@pytest.mark.parametrize("case", list(CASES))
def test_student_terms_vs_oracle(case, variant, golden_dir):
    c = _problem(case, golden_dir)
    got = c["dp"].eval(dev(c["slots"]), dev(c["rooms"]), variant=variant)
    for g, e, what in zip((host(t) for t in got), c["exp"], NAMES):
        bad = np.flatnonzero(g != e)
        assert bad.size == 0, f"{what}: rows {bad[:8]} got {g[bad[:8]]} expected {e[bad[:8]]}"
    assert c["dp"].status() == 0
