"""CPU checks of the greedy constructive initial population (no GPU): the
boundary of include/ttga_greedy.h as a C++98 consumer sees it, the argument
handling of its entry points before any device call, the --init flag's place in
the Control-style parse, Island's check of `init`, and the numpy model
(tests/greedy_model.py) against its own replay checker and against the
prototype's figures on comp01."""
import ctypes
import pathlib
import shutil

import numpy as np
import pytest

import ttga
import greedy_model as gm
from oracle_lib import ORACLE_PATH, oracle
from stage_checks import (Sink, build_and_run_consumer, check_exports, rejected_by_native_driver,
                          rejected_by_parse_control, stripped_before_pair_count)
from ttga import native
from ttga.ga import Island
from ttga.islands import parse_control

REPO = pathlib.Path(__file__).resolve().parent.parent
HEADER = REPO / "include" / "ttga_greedy.h"
CONSUMER = REPO / "tests" / "boundary_greedy_cxx98.cpp"


def test_header_symbols_are_exported_listed_and_called():
    check_exports(HEADER, "TTGA_GREEDY_H", "GREEDY_EXPORTS", CONSUMER,
                  {"tt_greedy_work_bytes", "tt_greedy_order", "tt_greedy_init"})
    assert '#include "ttga.h"' in HEADER.read_text()
    assert "ttga_greedy.h" in (REPO / "include" / "ttga.h").read_text()


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_cxx98_greedy_consumer_builds_and_links(tmp_path):
    build_and_run_consumer(CONSUMER, tmp_path)


def test_argument_errors_without_a_device():
    lib = native.load()
    buf = (ctypes.c_int64 * 64)()
    assert lib.tt_greedy_work_bytes(None) == 0
    # a null handle is named, whatever else is wrong
    for args in ((None, buf, buf, None), (None, None, None, None), (None, buf, None, None)):
        assert lib.tt_greedy_order(*args) == native.TT_ERR_INVALID
        assert b"null tt_problem" in lib.tt_last_error()
    for args in ((None, buf, buf, buf, buf, 1, None), (None, None, None, None, None, 1, None),
                 (None, buf, buf, buf, buf, -1, None), (None, buf, buf, buf, buf, 0, None)):
        assert lib.tt_greedy_init(*args) == native.TT_ERR_INVALID
        assert b"null tt_problem" in lib.tt_last_error()
    # with a handle, sizes and buffers are checked before any device call: a stand-in
    # handle that the library must not look into
    fake = ctypes.cast((ctypes.c_uint8 * 8)(), ctypes.c_void_p)
    for args in ((fake, None, buf, None), (fake, buf, None, None)):
        assert lib.tt_greedy_order(*args) == native.TT_ERR_INVALID
        assert b"null tt_problem" not in lib.tt_last_error()
    for k in (1, 2, 3, 4):                                   # order, rng, slot, room
        args = [fake, buf, buf, buf, buf, 1, None]
        args[k] = None
        assert lib.tt_greedy_init(*args) == native.TT_ERR_INVALID
        assert b"null tt_problem" not in lib.tt_last_error()
    assert lib.tt_greedy_init(fake, buf, buf, buf, buf, -1, None) == native.TT_ERR_INVALID
    assert lib.tt_greedy_init(fake, buf, buf, buf, buf, 0, None) == native.TT_OK        # no launch


def test_init_flag_in_the_control_parse():
    ctl = parse_control(["-i", "x.tim", "--init", "greedy", "-s", "42"], out=Sink(), err=Sink())
    assert ctl["init"] == "greedy" and ctl["seed"] == 42 and ctl["input"] == "x.tim"
    assert parse_control(["--init", "random", "-i", "x.tim"], out=Sink(), err=Sink())["init"] == "random"
    assert "init" not in parse_control(["-i", "x.tim", "-s", "42"], out=Sink(), err=Sink())     # absent: no key
    both = parse_control(["--unique", "-i", "x.tim", "--init", "greedy", "--pop", "20"], out=Sink(), err=Sink())
    assert both["init"] == "greedy" and both["unique"] is True and both["pop"] == 20
    for bad in (["-i", "x.tim", "--init", "best"], ["-i", "x.tim", "--init"]):
        rejected_by_parse_control(bad, "--init must be random or greedy", exact=True)


def test_init_flag_in_the_native_driver():
    for bad in (["-i", "x.tim", "--init", "best"], ["-i", "x.tim", "--init"]):
        rejected_by_native_driver(bad, "--init must be random or greedy", exact=True)
    stripped_before_pair_count(["--init", "greedy"])


def test_island_rejects_a_bad_init_before_any_device_call():
    class NoDevice:                      # any use of it would raise AttributeError
        pass
    for bad in ("best", "", None, "Greedy"):
        with pytest.raises(ValueError, match="init must be"):
            Island(NoDevice(), init=bad)


def test_model_against_its_replay_checker_on_sm():
    inst = ttga.config_instance("sm")
    order = gm.greedy_order(inst)
    key = gm.greedy_keys(inst)
    assert sorted(order.tolist()) == list(range(inst.E))
    assert all((key[a], -a) >= (key[b], -b) for a, b in zip(order[:-1], order[1:]))
    seeds = np.array([1, 0, 2147483646, 3000000019, 77], np.int64)
    slot, states = gm.greedy_slots(inst, order, seeds)
    assert slot.max() < 45
    for row in slot:
        gm.replay_check(inst, order, row)
    assert states.tolist() == [gm.advanced(s, inst.E) for s in seeds]
    # the stream of seed 0 stays 0: every pick is the first of the ties
    assert states[1] == 0
    # the checker rejects a row that is not greedy: the second event of the order moved
    # into the first one's slot, when they are correlated
    nb = inst.correlations()
    a = int(order[0])
    b = next(int(e) for e in order[1:] if nb[a, e])
    wrong = slot[0].copy()
    wrong[b] = wrong[a]
    with pytest.raises(AssertionError):
        gm.replay_check(inst, order, wrong)


@pytest.fixture(scope="module")
def comp01_rows():
    inst = ttga.config_instance("comp01")
    seeds = ttga.population_seeds(1000, 16)
    slot, _ = gm.greedy_slots(inst, gm.greedy_order(inst), seeds)
    return inst, seeds, slot


def test_model_rows_are_distinct_on_comp01(comp01_rows):
    inst, seeds, slot = comp01_rows
    assert len({row.tobytes() for row in slot}) == 16


@pytest.mark.skipif(not ORACLE_PATH.exists(), reason="oracle/libttoracle.so not built")
def test_model_reproduces_the_prototype_on_comp01(comp01_rows):
    """The condition: the greedy start's mean hcv is at most a tenth of the random
    start's on the same seeds. The absolute values (0.5 against 445.8, the
    prototype's) are the cross-check of the model."""
    inst, seeds, slot = comp01_rows
    o = oracle().problem(inst)
    greedy = o.eval(slot, o.assign_rooms(slot))[0]
    rs, rr, _ = o.random_init(seeds)
    random = o.eval(rs, rr)[0]
    print("mean hcv: greedy", greedy.mean(), "random", random.mean())
    assert greedy.mean() * 10 <= random.mean()
    assert greedy.mean() == 0.5 and greedy.max() == 1
    assert abs(random.mean() - 445.8) < 0.05
