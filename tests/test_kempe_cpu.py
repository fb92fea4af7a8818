"""CPU checks of the Kempe-chain move (no GPU): the boundary of
include/ttga_kempe.h as a C++98 consumer sees it, the argument handling of
tt_kempe_move before any device call, the --kempe flags' place in the
Control-style parse and in the native driver, Island's check of its arguments,
and the numpy model (tests/kempe_model.py) against an independent union-find
and against ttga.validate's correlated-pairs count."""
import ctypes
import pathlib
import shutil

import numpy as np
import pytest

import ttga
import kempe_model as km
from stage_checks import (Sink, build_and_run_consumer, check_exports, rejected_by_native_driver,
                          rejected_by_parse_control, stripped_before_pair_count)
from ttga import native
from ttga.ga import Island, kempe_line
from ttga.islands import parse_control
from ttga.rng import ParkMiller
from ttga.validate import evaluate

REPO = pathlib.Path(__file__).resolve().parent.parent
HEADER = REPO / "include" / "ttga_kempe.h"
CONSUMER = REPO / "tests" / "boundary_kempe_cxx98.cpp"


def test_header_symbols_are_exported_listed_and_called():
    check_exports(HEADER, "TTGA_KEMPE_H", "KEMPE_EXPORTS", CONSUMER, {"tt_kempe_move"})
    assert '#include "ttga.h"' in HEADER.read_text()
    top = (REPO / "include" / "ttga.h").read_text()
    assert "ttga_kempe.h" in top and "bit 6 (64)" in top


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_cxx98_kempe_consumer_builds_and_links(tmp_path):
    build_and_run_consumer(CONSUMER, tmp_path)


def test_argument_errors_without_a_device():
    lib = native.load()
    buf = (ctypes.c_int64 * 64)()
    nan = float("nan")
    # a null handle is named, whatever else is wrong
    for args in ((None, buf, buf, buf, 1, 0.5, 0, buf, None), (None, None, None, None, 1, 0.5, 0, None, None),
                 (None, buf, buf, buf, -1, 0.5, 0, buf, None), (None, buf, buf, buf, 0, 0.5, 0, buf, None),
                 (None, buf, buf, buf, 1, 1.5, -1, buf, None), (None, buf, buf, buf, 1, nan, 0, buf, None)):
        assert lib.tt_kempe_move(*args) == native.TT_ERR_INVALID
        assert b"null tt_problem" in lib.tt_last_error()
    # with a handle, every argument is checked before any device call: a stand-in
    # handle that the library must not look into
    fake = ctypes.cast((ctypes.c_uint8 * 8)(), ctypes.c_void_p)
    for k in (1, 2, 3):                                      # slot, room, rng
        args = [fake, buf, buf, buf, 1, 0.5, 0, buf, None]
        args[k] = None
        assert lib.tt_kempe_move(*args) == native.TT_ERR_INVALID
        assert b"null tt_problem" not in lib.tt_last_error()
    assert lib.tt_kempe_move(fake, buf, buf, buf, -1, 0.5, 0, buf, None) == native.TT_ERR_INVALID
    assert lib.tt_kempe_move(fake, buf, buf, buf, 1, 0.5, -1, buf, None) == native.TT_ERR_INVALID
    assert b"max_chain" in lib.tt_last_error()
    for prob in (-0.1, 1.5, nan):
        assert lib.tt_kempe_move(fake, buf, buf, buf, 1, prob, 0, buf, None) == native.TT_ERR_INVALID
        assert b"prob" in lib.tt_last_error()
        assert lib.tt_kempe_move(fake, buf, buf, buf, 0, prob, 0, buf, None) == native.TT_ERR_INVALID
    for prob in (0.0, 0.5, 1.0):                             # no launch; chain_len may be NULL
        assert lib.tt_kempe_move(fake, buf, buf, buf, 0, prob, 0, buf, None) == native.TT_OK
        assert lib.tt_kempe_move(fake, buf, buf, buf, 0, prob, 7, None, None) == native.TT_OK


MESSAGE = "--kempe must be a probability in [0, 1], --kempe-max-chain an integer >= 0"


def test_kempe_flags_in_the_control_parse():
    ctl = parse_control(["-i", "x.tim", "--kempe", "0.5", "-s", "42"], out=Sink(), err=Sink())
    assert ctl["kempe"] == 0.5 and "kempe_max_chain" not in ctl and ctl["seed"] == 42 and ctl["input"] == "x.tim"
    ctl = parse_control(["--kempe-max-chain", "8", "-i", "x.tim", "--kempe", "1"], out=Sink(), err=Sink())
    assert ctl["kempe"] == 1.0 and ctl["kempe_max_chain"] == 8
    plain = parse_control(["-i", "x.tim", "-s", "42"], out=Sink(), err=Sink())                  # absent: no key
    assert "kempe" not in plain and "kempe_max_chain" not in plain
    both = parse_control(["--unique", "-i", "x.tim", "--kempe", "0.25", "--init", "greedy", "--pop", "20"],
                         out=Sink(), err=Sink())
    assert both["kempe"] == 0.25 and both["unique"] is True and both["init"] == "greedy" and both["pop"] == 20
    for bad in (["-i", "x.tim", "--kempe", "1.5"], ["-i", "x.tim", "--kempe", "-0.1"], ["-i", "x.tim", "--kempe"],
                ["-i", "x.tim", "--kempe", "nan"], ["-i", "x.tim", "--kempe", "half"],
                ["-i", "x.tim", "--kempe-max-chain", "-1"], ["-i", "x.tim", "--kempe-max-chain"]):
        rejected_by_parse_control(bad, MESSAGE, exact=True)


def test_kempe_flags_in_the_native_driver():
    for bad in (["-i", "x.tim", "--kempe", "1.5"], ["-i", "x.tim", "--kempe"], ["-i", "x.tim", "--kempe", "nan"],
                ["-i", "x.tim", "--kempe", "half"], ["-i", "x.tim", "--kempe-max-chain", "-1"]):
        rejected_by_native_driver(bad, MESSAGE, exact=True)
    stripped_before_pair_count(["--kempe", "0.5", "--kempe-max-chain", "4"])


def test_island_rejects_bad_kempe_values_before_any_device_call():
    class NoDevice:                      # any use of it would raise AttributeError
        pass
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="kempe must be"):
            Island(NoDevice(), kempe=bad)
    with pytest.raises(ValueError, match="kempe_max_chain"):
        Island(NoDevice(), kempe=0.5, kempe_max_chain=-1)


def test_kempe_line():
    line = kempe_line({"children": 24, "moved": 3, "rejected": 9, "chain_events": 7})
    assert line == '{"kempe":{"children":24,"meanChain":%.17g,"moved":3,"rejected":9}}' % (7 / 3)
    assert '"meanChain":0,' in kempe_line({"children": 4, "moved": 0, "rejected": 4, "chain_events": 0})


# ---------------------------------------------------------------- the model
def union_find_component(nb, members, e):
    idx = np.flatnonzero(members)
    parent = {int(i): int(i) for i in idx}

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a
    for a in idx:
        for b in idx:
            if a < b and nb[a, b]:
                parent[find(int(a))] = find(int(b))
    root = find(int(e))
    return np.array([i for i in idx if find(int(i)) == root], np.int64)


@pytest.mark.parametrize("name", ["sm", "med"])
def test_model_properties(name):
    inst = ttga.config_instance(name)
    nb = km.neighbours(inst)
    assert not nb.diagonal().any() and np.array_equal(nb, nb.T)
    P = 64
    slot = np.random.default_rng(11).integers(0, 45, size=(P, inst.E)).astype(np.uint8)
    seeds = ttga.population_seeds(4200, P)
    new, states, chain, pairs = km.kempe_rows(inst, slot, seeds, 1.0, nb=nb)
    rooms = np.zeros(inst.E, np.int64)
    sizes = []
    for i in range(P):
        t1, t2 = pairs[i]
        assert t1 != t2 and 0 <= t1 < 45 and 0 <= t2 < 45
        assert states[i] == km.advanced(seeds[i], 3)
        changed = np.flatnonzero(new[i] != slot[i])
        # K: the component an independent union-find gives, containing the chosen event
        g = ParkMiller(int(seeds[i]))
        g.next()
        e = g.pick(inst.E)
        assert slot[i][e] == t1
        K = union_find_component(nb, (slot[i] == t1) | (slot[i] == t2), e)
        assert chain[i] == len(K) and np.array_equal(changed, K)
        assert all((slot[i][k], new[i][k]) in ((t1, t2), (t2, t1)) for k in K)
        # no correlated pair joins K to the rest of the two slots
        rest = np.setdiff1d(np.flatnonzero((slot[i] == t1) | (slot[i] == t2)), K)
        assert not nb[np.ix_(K, rest)].any()
        assert evaluate(inst, new[i], rooms)["corr_pairs"] == evaluate(inst, slot[i], rooms)["corr_pairs"]
        sizes.append(len(K))
    assert max(sizes) > 1 and len(set(sizes)) > 2          # real chains, not Move1 in disguise
    # the cap refuses exactly the chains above it and spends the same three draws
    capped, cstates, cchain, _ = km.kempe_rows(inst, slot, seeds, 1.0, max_chain=4, nb=nb)
    assert np.array_equal(cstates, states)
    for i in range(P):
        if chain[i] > 4:
            assert cchain[i] == -chain[i] and np.array_equal(capped[i], slot[i])
        else:
            assert cchain[i] == chain[i] and np.array_equal(capped[i], new[i])
    # the gate: prob 0 spends one draw and changes nothing
    same, gstates, gchain, gpairs = km.kempe_rows(inst, slot, seeds, 0.0, nb=nb)
    assert np.array_equal(same, slot) and not gchain.any() and gpairs == [None] * P
    assert gstates.tolist() == [km.advanced(s, 1) for s in seeds]
    # an invalid gene: nothing happens, no draw
    bad = slot[:2].copy()
    bad[0, 3] = 45
    room = np.zeros_like(bad)
    room[1, 5] = inst.R
    _, bstates, bchain, _ = km.kempe_rows(inst, bad, seeds[:2], 1.0, room=room, nb=nb)
    assert bstates.tolist() == seeds[:2].tolist() and not bchain.any()
