"""CPU checks of the timeslot-swap descent (no GPU): the boundary of
include/ttga_slotswap.h as a C++98 consumer sees it, the argument handling of
tt_slot_swap before any device call, the --slot-swap flag's place in the
Control-style parse and in the native driver, Island's check of its argument,
the slotSwap line, and the numpy model (tests/slotswap_model.py): its table
form against its brute-force form and against ttga.validate."""
import ctypes
import pathlib
import shutil

import numpy as np
import pytest

import ttga
import slotswap_model as sm
from stage_checks import (Sink, build_and_run_consumer, check_exports, rejected_by_native_driver,
                          rejected_by_parse_control, stripped_before_pair_count)
from ttga import native
from ttga.ga import Island, slot_swap_line
from ttga.islands import parse_control
from ttga.validate import evaluate

REPO = pathlib.Path(__file__).resolve().parent.parent
HEADER = REPO / "include" / "ttga_slotswap.h"
CONSUMER = REPO / "tests" / "boundary_slotswap_cxx98.cpp"
UNCAPPED = 2 ** 31 - 1


def test_header_symbols_are_exported_listed_and_called():
    check_exports(HEADER, "TTGA_SLOTSWAP_H", "SLOTSWAP_EXPORTS", CONSUMER, {"tt_slot_swap"})
    assert '#include "ttga.h"' in HEADER.read_text()
    top = (REPO / "include" / "ttga.h").read_text()
    assert "ttga_slotswap.h" in top and "bit 7 (128)" in top


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_cxx98_slotswap_consumer_builds_and_links(tmp_path):
    build_and_run_consumer(CONSUMER, tmp_path)


def test_argument_errors_without_a_device():
    lib = native.load()
    buf = (ctypes.c_int32 * 64)()
    # a null handle is named, whatever else is wrong
    for args in ((None, buf, 1, 1, buf, buf, buf, buf, buf, None), (None, None, 1, 1, None, None, None, None, None, None),
                 (None, buf, -1, 1, buf, buf, buf, buf, buf, None), (None, buf, 0, 1, buf, buf, buf, buf, buf, None),
                 (None, buf, 1, 0, buf, buf, buf, buf, buf, None)):
        assert lib.tt_slot_swap(*args) == native.TT_ERR_INVALID
        assert b"null tt_problem" in lib.tt_last_error()
    # with a handle, every argument is checked before any device call: a stand-in
    # handle that the library must not look into
    fake = ctypes.cast((ctypes.c_uint8 * 8)(), ctypes.c_void_p)
    assert lib.tt_slot_swap(fake, None, 1, 1, buf, buf, buf, buf, buf, None) == native.TT_ERR_INVALID
    assert b"null tt_problem" not in lib.tt_last_error()
    assert lib.tt_slot_swap(fake, buf, -1, 1, buf, buf, buf, buf, buf, None) == native.TT_ERR_INVALID
    for max_passes in (0, -1):
        for P in (0, 1):
            assert lib.tt_slot_swap(fake, buf, P, max_passes, buf, buf, buf, buf, buf, None) == native.TT_ERR_INVALID
            assert b"max_passes" in lib.tt_last_error()
    for max_passes in (1, 64, UNCAPPED):                     # P = 0: no launch; every output may be NULL
        assert lib.tt_slot_swap(fake, buf, 0, max_passes, buf, buf, buf, buf, buf, None) == native.TT_OK
        assert lib.tt_slot_swap(fake, buf, 0, max_passes, None, None, None, None, None, None) == native.TT_OK


BAD_FLAGS = (["-i", "x.tim", "--slot-swap", "-1"], ["-i", "x.tim", "--slot-swap"], ["-i", "x.tim", "--slot-swap", "2.5"],
             ["-i", "x.tim", "--slot-swap", "nan"], ["-i", "x.tim", "--slot-swap", "many"])


def test_slot_swap_flag_in_the_control_parse():
    ctl = parse_control(["-i", "x.tim", "--slot-swap", "4", "-s", "42"], out=Sink(), err=Sink())
    assert ctl["slot_swap"] == 4 and ctl["seed"] == 42 and ctl["input"] == "x.tim"
    assert parse_control(["--slot-swap", "0", "-i", "x.tim"], out=Sink(), err=Sink())["slot_swap"] == 0
    plain = parse_control(["-i", "x.tim", "-s", "42"], out=Sink(), err=Sink())                  # absent: no key
    assert "slot_swap" not in plain
    both = parse_control(["--unique", "-i", "x.tim", "--slot-swap", "64", "--kempe", "0.25", "--pop", "20"],
                         out=Sink(), err=Sink())
    assert both["slot_swap"] == 64 and both["kempe"] == 0.25 and both["unique"] is True and both["pop"] == 20
    for bad in BAD_FLAGS:
        rejected_by_parse_control(bad, "--slot-swap must be a non-negative integer", exact=True)


def test_slot_swap_flag_in_the_native_driver():
    for bad in BAD_FLAGS:
        rejected_by_native_driver(bad, "--slot-swap must be a non-negative integer", exact=True)
    stripped_before_pair_count(["--slot-swap", "4"])


def test_island_rejects_a_negative_slot_swap_before_any_device_call():
    class NoDevice:                      # any use of it would raise AttributeError
        pass
    with pytest.raises(ValueError, match=r"slot_swap must be >= 0 \(0: off\)"):
        Island(NoDevice(), slot_swap=-1)


def test_slot_swap_line():
    line = slot_swap_line({"rows": 30, "improved": 7, "passes": 16, "gain": 41})
    assert line == '{"slotSwap":{"gain":41,"improved":7,"meanPasses":%.17g,"rows":30}}' % (16 / 7)
    assert '"meanPasses":0,' in slot_swap_line({"rows": 4, "improved": 0, "passes": 0, "gain": 0})


# ---------------------------------------------------------------- the model
def instance(name):
    return sm.load_golden(name) if name == "tight" else ttga.config_instance(name)


def rows(inst, P, seed):
    return np.random.default_rng(seed).integers(0, 45, size=(P, inst.E)).astype(np.uint8)


@pytest.mark.parametrize("name", ["sm", "tight"])
def test_table_form_equals_brute_force_on_all_990_pairs(name):
    inst = instance(name)
    assert len(sm.PAIRS) == 990
    for row in rows(inst, 3, 21):
        assert sm.scv_of(inst, row) == evaluate(inst, row, np.zeros(inst.E, np.int64))["scv"]
        brute, table = sm.deltas_brute(inst, row), sm.deltas_table(inst, row)
        assert np.array_equal(brute, table), np.argwhere(brute != table)[:8]
        assert (brute != sm.NO_PAIR).sum() == 990
        # the kernel's form of the 180 pairs on one day: co-occurrence counts of the windows of three
        assert np.array_equal(brute, sm.deltas_windows(inst, row))
    # a row the students clash in: every event in slot 8, three of them moved
    row = np.full(inst.E, 8, np.uint8)
    row[:3] = 17
    assert np.array_equal(sm.deltas_brute(inst, row), sm.deltas_table(inst, row))


@pytest.mark.parametrize("name", ["sm", "tight"])
def test_descent_against_the_validator(name):
    inst = instance(name)
    rooms = np.random.default_rng(5).integers(0, inst.R, size=inst.E)
    tied = applied = 0
    for row in rows(inst, 4, 22):
        log = []
        new, gain, passes, perm = sm.descend(inst, row, UNCAPPED, log=log)
        before, after = evaluate(inst, row, rooms), evaluate(inst, new, rooms)
        assert passes == len(log) >= 1 and gain == -sum(dl for dl, _, _, _ in log) > 0
        assert all(dl < 0 and a < b for dl, a, b, _ in log)
        assert after["scv"] == before["scv"] - gain
        for k in ("hcv", "room_pairs", "corr_pairs", "unsuitable"):
            assert after[k] == before[k], k
        assert sorted(perm.tolist()) == list(range(45)) and np.array_equal(perm[row], new)
        # the table form took the steps the brute-force form takes (the first three compared)
        b3 = sm.descend(inst, row, 3, deltas=sm.deltas_brute)
        p3 = sm.prefix(row, log, 3)
        assert np.array_equal(b3[0], p3[0]) and b3[1:3] == p3[1:3] and np.array_equal(b3[3], p3[3])
        # a row at its local optimum: nothing to do
        again = sm.descend(inst, new, UNCAPPED)
        assert np.array_equal(again[0], new) and again[1:3] == (0, 0) and np.array_equal(again[3], np.arange(45))
        tied += sum(t for _, _, _, t in log)
        applied += passes
    print(name, "passes", applied, "with a tied best delta", tied)
    assert tied >= 1                                         # the tie rule was exercised


def test_model_leaves_an_invalid_row_alone():
    inst = instance("sm")
    row = rows(inst, 1, 23)[0]
    row[7] = 45
    new, gain, passes, perm = sm.descend(inst, row, UNCAPPED)
    assert np.array_equal(new, row) and (gain, passes) == (0, 0) and np.array_equal(perm, np.arange(45))
