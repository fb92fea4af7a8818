"""tests/stage_checks.py and tests/walk_checks.py on planted defects (no GPU,
no rebuild): a clean consumer, clean export groups, clean canned driver outputs
and clean canned rows pass, and each defect the helpers are there to catch
makes them fail."""
import shutil
import types

import numpy as np
import pytest

import stage_checks as sc
import walk_checks as wc
from ttga import native

KEMPE = (sc.REPO / "include" / "ttga_kempe.h", "TTGA_KEMPE_H", "KEMPE_EXPORTS",
         sc.REPO / "tests" / "boundary_kempe_cxx98.cpp", {"tt_kempe_move"})

# make_instance and tt_last_error are used, fail is not: an inline function may stay unused
CONSUMER = """#include <cstdio>
#include "ttga.h"
#include "boundary_common_cxx98.h"
int main() {
    Instance in = make_instance();
    %s
    std::printf("TT_ERR_DEVICE %%d %%s\\nnull-handle checks: %%d wrong\\n", in.E, tt_last_error(), %d);
    return TT_ERR_DEVICE;
}
"""


def consumer(tmp_path, extra="", wrong=0):
    src = tmp_path / "consumer.cpp"
    src.write_text(CONSUMER % (extra, wrong))
    return src


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_consumer_build_and_run(tmp_path):
    assert sc.build_and_run_consumer(consumer(tmp_path), tmp_path).returncode == native.TT_ERR_DEVICE
    with pytest.raises(AssertionError, match="unused variable"):
        sc.build_and_run_consumer(consumer(tmp_path, extra="int left_over = 3;"), tmp_path)
    with pytest.raises(AssertionError):
        sc.build_and_run_consumer(consumer(tmp_path, wrong=1), tmp_path)


def fake_native(**groups):
    real = {n: getattr(native, n) for n in dir(native) if n.endswith("EXPORTS")}
    return types.SimpleNamespace(**{**real, **groups}, load=native.load)


def test_check_exports():
    assert sc.check_exports(*KEMPE) == {"tt_kempe_move"}
    assert sc.check_exports(*KEMPE, native=fake_native()) == {"tt_kempe_move"}
    with pytest.raises(AssertionError, match="KEMPE_EXPORTS"):           # missing from its group
        sc.check_exports(*KEMPE, native=fake_native(KEMPE_EXPORTS=()))
    with pytest.raises(AssertionError, match="LATER_STAGE_EXPORTS"):     # in a group no test module has heard of
        sc.check_exports(*KEMPE, native=fake_native(LATER_STAGE_EXPORTS=("tt_later", "tt_kempe_move")))
    with pytest.raises(AssertionError):                                  # a symbol the consumer never calls
        sc.check_exports(KEMPE[0], KEMPE[1], KEMPE[2], sc.REPO / "tests" / "boundary_lahc_cxx98.cpp")


def output(stage='{"kempe":{"children":80,"meanChain":2.5,"moved":3,"rejected":9}}', stage_first=False):
    lines = ['{"logEntry":{"best":7,"procID":0,"time":0.25}}', '{"solution":{"procID":0,"totalTime":1.5}}', stage,
             '{"runEntry":{"procID":0,"totalTime":%s}}']
    if stage_first:
        lines[1], lines[2] = lines[2], lines[1]
    return "\n".join(lines) + "\n"


def test_same_output():
    a, lines = sc.same_output(output() % 1.5, output() % 2.25, "kempe")          # the wall clock may differ
    assert lines == [{"children": 80, "meanChain": 2.5, "moved": 3, "rejected": 9}] and len(a) == 4
    other = output('{"kempe":{"children":80,"meanChain":2.50,"moved":3,"rejected":9}}')
    assert sc.same_output(other % 1, other % 1, "kempe")[1] == lines
    with pytest.raises(AssertionError):                                  # the same JSON, one more byte
        sc.same_output(output() % 1, other % 1, "kempe")
    early = output(stage_first=True)
    with pytest.raises(AssertionError):                                  # both agree, but the line comes too early
        sc.same_output(early % 1, early % 1, "kempe")
    with pytest.raises(AssertionError):                                  # a stage that printed nothing
        sc.same_output(output() % 1, output() % 1, "slotSwap")


def rows():
    """Four rows of three events around a call of 50 steps; row 2 is closed (hcv 1)."""
    slot = np.arange(12, dtype=np.uint8).reshape(4, 3)
    room = np.ones((4, 3), np.uint8)
    seeds = np.array([11, 12, 13, 14], np.int64)
    hcv = np.array([0, 0, 1, 0], np.int32)
    scv = np.array([30, 20, 9, 5], np.int32)
    before = (hcv, scv, (hcv == 0).astype(np.int32), np.where(hcv == 0, scv, 1000000 * hcv + scv))
    gain = np.array([4, 0, 0, 5], np.int32)
    open_ = hcv == 0
    stats = np.array([[20, 2, 3, 6, 9], [20, 0, 20, 0, 0], [0] * 5, [9, 0, 0, 7, 7]], np.int32)
    got = [np.where(open_[:, None], slot[:, ::-1], slot), room.copy(), np.where(open_, seeds + 1000, seeds), gain,
           np.array([17, 3, 0, 7], np.int32), np.array([50, 0, 0, 6], np.int32), stats]
    after = (hcv, scv - gain, before[2], before[3] - gain * open_)
    return got, before, after, [after[1].copy(), after[3].copy()], slot, room, seeds


def test_check_rows():
    got, before, after, inplace, slot, room, seeds = rows()
    closed = wc.check_rows(got, [g.copy() for g in got], before, after, inplace, slot, room, seeds, 50)
    assert closed.tolist() == [False, False, True, False]
    assert wc.check_rows(got, None, before, after, inplace, slot, room, seeds, 50)[2]

    def fails(change, want=False):
        got, before, after, inplace, slot, room, seeds = rows()
        model = [g.copy() for g in got] if want else None
        change(got, after, inplace)
        with pytest.raises(AssertionError):
            wc.check_rows(got, model, before, after, inplace, slot, room, seeds, 50)

    def rng_of_a_closed_row(got, after, inplace):
        got[2][2] += 1

    def one_less_than_the_gain(got, after, inplace):
        after[1][0] += 1                 # scv fell by gain - 1, in place too
        inplace[0][0] += 1

    def stale_in_place(got, after, inplace):
        inplace[1][3] += 5

    def a_count_in_a_closed_row(got, after, inplace):
        got[6][2, 0] = 1

    def more_accepted_than_steps(got, after, inplace):
        got[4][0] = 51

    def more_chains_accepted_than_placed(got, after, inplace):
        got[6][0, 3] = 16

    def one_gene(got, after, inplace):
        got[0][3, 1] ^= 1
    for change in (rng_of_a_closed_row, one_less_than_the_gain, stale_in_place, a_count_in_a_closed_row,
                   more_accepted_than_steps, more_chains_accepted_than_placed):
        fails(change)
    fails(one_gene, want=True)
