"""CPU checks of the Kempe-chain candidates in the late-acceptance walk (no
GPU): the model (tests/lahc_kempe_model.py) against tests/lahc_model.py where
no chain is drawn and against ttga.validate after every accepted step, the
chain's invariant on rows of any kind, a hand-built instance in which the
ascending order of the room rule matters, the boundary of tt_lahc_kempe as a
C++98 consumer sees it, its argument handling before any device call, the
--lahc-kempe flags in both drivers' parse, stages.validate and the lahcKempe
line."""
import ctypes
import pathlib
import shutil

import numpy as np
import pytest

import ttga
import lahc_kempe_model as km
import lahc_model as lm
from stage_checks import (Sink, build_and_run_consumer, check_exports, rejected_by_native_driver,
                          rejected_by_parse_control, stripped_before_pair_count)
from ttga import native, stages
from ttga.ga import Island, lahc_kempe_line
from ttga.islands import parse_control
from ttga.rng import ParkMiller
from ttga.validate import evaluate

REPO = pathlib.Path(__file__).resolve().parent.parent
HEADER = REPO / "include" / "ttga_lahc_kempe.h"
CONSUMER = REPO / "tests" / "boundary_lahc_kempe_cxx98.cpp"


# ---------------------------------------------------------------- the model
@pytest.mark.parametrize("cid", [c for c, v in lm.CASES.items() if v[1] <= 8])
def test_without_chains_the_model_is_lahc_model(cid):
    shape, P, steps, L, p_swap = lm.CASES[cid]
    inst = lm.SHAPES[shape]()
    m = km.Model(inst)
    slot, room, seeds = lm.population(inst, P, m)
    want = m.lahc_rows(slot, room, seeds, steps, L, p_swap)
    got = m.lahc_kempe_rows(slot, room, seeds, steps, L, p_swap, 0.0)
    for g, w in zip(got, want):
        assert np.array_equal(g, w)
    assert not got[6].any()


@pytest.fixture(scope="module")
def small():
    out = {}
    for name, inst in (("E20", ttga.generate(20, 3, 2, 30, seed=11)), ("E61", ttga.generate(61, 5, 3, 40, seed=12))):
        m = km.Model(inst)
        slot, room = lm.feasible_rows(inst, 6, 3, m)
        out[name] = (inst, m, slot, room)
    return out


def corr_pairs(m, slot, a, t):
    """Correlated pairs inside slot a plus those inside slot t."""
    sets = m.slot_sets(slot)
    return sum(bin(m.corr[e] & sets[s] & ~(1 << e)).count("1") for s in (a, t) for e in km._events(sets[s])) // 2


@pytest.mark.parametrize("name", ["E20", "E61"])
@pytest.mark.parametrize("history,p_swap,p_kempe,cap", [(1, 0.25, 0.5, 0), (20, 0.25, 0.5, 0), (300, 0.0, 1.0, 0),
                                                         (20, 0.5, 0.5, 0), (20, 0.25, 0.5, 2)])
def test_every_accepted_step_is_feasible_and_costs_cur(small, name, history, p_swap, p_kempe, cap):
    inst, m, slot, room = small[name]
    walked, chains = 0, []
    for i in range(len(slot)):
        if evaluate(inst, slot[i], room[i])["hcv"] != 0:
            continue
        seen, touched, last = [], np.zeros(inst.E, bool), [slot[i].copy(), room[i].copy()]

        def on_accept(k, s, r, cur):
            ev = evaluate(inst, s, r)
            assert ev["hcv"] == 0 and ev["scv"] == cur, (k, ev, cur)
            assert m.hcv_of(s, r) == 0 and m.scv_of(s) == cur
            seen.append(cur)
            moved = s != last[0]
            assert moved.sum() >= 1 and not ((r != last[1]) & ~moved).any()      # only moved events change rooms
            slots = set(s[moved].tolist()) | set(last[0][moved].tolist())
            assert len(slots) == 2                                                   # between two slots
            a, t = sorted(slots)
            assert (s[moved].astype(int) + last[0][moved] == a + t).all()            # every one changed sides
            assert corr_pairs(m, s, a, t) == corr_pairs(m, last[0], a, t) == 0
            touched[moved] = True
            last[0], last[1] = s.copy(), r.copy()
        info = {}
        s1, r1, state, gain, accepted, best_step, stats = m.lahc_kempe(
            slot[i], room[i], 77 + i, 400, history, p_swap, p_kempe, cap, on_accept=on_accept, info=info)
        tried, capped, no_room, k_acc, events = stats
        assert accepted == len(seen) > 0 and accepted == info["move1"] + info["move2"] + info["kempe"]
        assert k_acc == info["kempe"] == len(info["chains"]) and events == sum(info["chains"])
        assert k_acc <= tried - capped - no_room and (cap > 0 or capped == 0)
        assert cap == 0 or max(info["chains"], default=0) <= cap
        assert p_kempe < 1.0 or info["move1"] == info["move2"] == 0
        assert p_swap + p_kempe < 1.0 or info["move1"] == 0
        before, after = evaluate(inst, slot[i], room[i]), evaluate(inst, s1, r1)
        assert before["scv"] == info["scv0"] and after["hcv"] == 0 and after["scv"] == info["scv0"] - gain
        assert gain >= 0 and gain == info["scv0"] - min(seen + [info["scv0"]])
        assert (best_step == 0) == (gain == 0) and best_step <= 400
        assert np.array_equal(r1[~touched], room[i][~touched]) and np.array_equal(s1[~touched], slot[i][~touched])
        g = ParkMiller(77 + i)                                   # exactly three draws a step
        for _ in range(3 * 400):
            g.next()
        assert state == g.seed
        chains += info["chains"]
        walked += 1
    assert walked >= 3 and chains and (cap or max(chains) >= 2)


def test_a_chain_keeps_the_correlated_pairs_of_any_row(small):
    """ttga_kempe.h's invariant, on random (infeasible) rows: moving the whole
    component leaves the correlated-pairs count of the two slots as it was."""
    inst, m, _, _ = small["E61"]
    g = np.random.default_rng(5)
    longest = 0
    for _ in range(40):
        slot = g.integers(0, 12, inst.E)                          # crowded slots: long chains
        e1 = int(g.integers(0, inst.E))
        a = int(slot[e1])
        t = int(g.integers(0, 11))
        t += t >= a
        sets = m.slot_sets(slot)
        k = m.component(sets[a] | sets[t], e1)
        events = km._events(k)
        assert e1 in events and all(int(slot[e]) in (a, t) for e in events)
        outside = (sets[a] | sets[t]) & ~k
        assert not any(m.corr[e] & outside for e in events)      # a whole component
        moved = slot.copy()
        moved[events] = a + t - slot[events]
        assert corr_pairs(m, moved, a, t) == corr_pairs(m, slot, a, t)
        longest = max(longest, len(events))
    assert longest >= 4


def test_model_leaves_infeasible_and_invalid_rows_alone(small):
    inst, m, slot, room = small["E61"]
    for spoil in ("pair", "slot", "room"):
        s, r = slot[0].copy(), room[0].copy()
        if spoil == "pair":
            s[1], r[1] = s[0], r[0]
        elif spoil == "slot":
            s[5] = 45
        else:
            r[5] = inst.R
        out = m.lahc_kempe(s, r, 123, 200, 10, 0.25, 0.5)
        assert np.array_equal(out[0], s) and np.array_equal(out[1], r) and out[2:] == (123, 0, 0, 0, (0, 0, 0, 0, 0))


def order_instance(first_is_choosy):
    """Three events, two rooms: events 0 and 1 share slot 0, event 2 is alone
    in slot 1 and has a student in common with each of them, so the three are
    one chain. One of events 0 and 1 can only take room 0 (it needs the
    feature that room 0 alone has), the other takes either room."""
    student_events = np.array([[1, 0, 1], [0, 1, 1]], np.int32)
    room_features = np.array([[1], [0]], np.int32)
    event_features = np.zeros((3, 1), np.int32)
    event_features[0 if first_is_choosy else 1, 0] = 1
    inst = ttga.Instance(3, 2, 1, 2, np.array([2, 2], np.int32), student_events, room_features, event_features)
    slot = np.array([0, 0, 1], np.uint8)
    room = np.array([0, 1, 0], np.uint8) if first_is_choosy else np.array([1, 0, 0], np.uint8)
    return inst, slot, room


def test_the_ascending_order_of_the_room_rule_matters():
    # event 0 is the choosy one: ascending, it takes room 0 and event 1 room 1;
    # descending, event 1 takes room 0 and event 0 finds none
    inst, slot, room = order_instance(True)
    m = km.Model(inst)
    assert m.hcv_of(slot, room) == 0
    occ = [0] * km.SLOTS
    occ[0], occ[1] = 0b11, 0b01
    k = m.component(m.slot_sets(slot)[0] | m.slot_sets(slot)[1], 0)
    assert k == 0b111
    assert m.chain_rooms(slot, room, occ, k, 0, 1) == [(0, 1, 0), (1, 1, 1), (2, 0, 0)]
    assert m.chain_rooms(slot, room, occ, k, 0, 1, descending=True) is None
    # event 1 is the choosy one: ascending, event 0 takes room 0 and event 1 finds none
    inst2, slot2, room2 = order_instance(False)
    m2 = km.Model(inst2)
    assert m2.hcv_of(slot2, room2) == 0
    assert m2.chain_rooms(slot2, room2, occ, k, 0, 1) is None
    assert m2.chain_rooms(slot2, room2, occ, k, 0, 1, descending=True) == [(0, 1, 1), (1, 1, 0), (2, 0, 0)]
    # and in the walk: chains only, a long history accepts every feasible candidate
    seen = {"order": 0, "no_room": 0}
    for seed in range(1, 9):
        info = {}

        def on_accept(k_, s, r, cur):
            assert m.hcv_of(s, r) == 0
        out = m.lahc_kempe(slot, room, seed, 300, 1000, 0.0, 1.0, on_accept=on_accept, info=info)
        seen["order"] += info["order_matters"]
        seen["no_room"] += m2.lahc_kempe(slot2, room2, seed, 300, 1000, 0.0, 1.0)[6][2]
        assert out[6][0] == 300
    assert seen["order"] > 0 and seen["no_room"] > 0


# ---------------------------------------------------------------- the boundary
def test_header_symbol_is_exported_listed_and_called():
    check_exports(HEADER, "TTGA_LAHC_KEMPE_H", "LAHC_KEMPE_EXPORTS", CONSUMER, {"tt_lahc_kempe"})
    assert '#include "ttga_lahc_kempe.h"' in (REPO / "include" / "ttga_lahc.h").read_text()


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_cxx98_consumer_builds_and_links(tmp_path):
    build_and_run_consumer(CONSUMER, tmp_path)


def test_argument_errors_without_a_device():
    lib = native.load()
    buf = (ctypes.c_int32 * 64)()
    dbl = ctypes.c_double

    def call(h, slot, room, rng, P, steps, history, p_swap, p_kempe, max_chain, outs=buf):
        return lib.tt_lahc_kempe(h, slot, room, rng, P, steps, history, dbl(p_swap), dbl(p_kempe), max_chain, outs, outs,
                                 outs, outs, outs, outs, None)
    for args in ((None, buf, buf, buf, 1, 10, 5, 0.25, 0.5, 0), (None, None, None, None, -1, -1, 0, 2.0, 2.0, -1)):
        assert call(*args) == native.TT_ERR_INVALID
        assert b"null tt_problem" in lib.tt_last_error()
    # a stand-in handle that the library must not look into
    fake = ctypes.cast((ctypes.c_uint8 * 8)(), ctypes.c_void_p)
    for args, word in (((fake, None, buf, buf, 1, 10, 5, 0.25, 0.5, 0), b"null population"),
                       ((fake, buf, buf, None, 1, 10, 5, 0.25, 0.5, 0), b"rng"),
                       ((fake, buf, buf, buf, -1, 10, 5, 0.25, 0.5, 0), b"negative population"),
                       ((fake, buf, buf, buf, 1, -1, 5, 0.25, 0.5, 0), b"steps"),
                       ((fake, buf, buf, buf, 1, 10, 0, 0.25, 0.5, 0), b"history"),
                       ((fake, buf, buf, buf, 1, 10, 5, 1.5, 0.0, 0), b"p_swap"),
                       ((fake, buf, buf, buf, 1, 10, 5, float("nan"), 0.0, 0), b"p_swap"),
                       ((fake, buf, buf, buf, 1, 10, 5, 0.25, 1.0000001, 0), b"p_kempe"),
                       ((fake, buf, buf, buf, 1, 10, 5, 0.25, -1e-9, 0), b"p_kempe"),
                       ((fake, buf, buf, buf, 0, 10, 5, 0.0, float("nan"), 0), b"p_kempe"),
                       ((fake, buf, buf, buf, 1, 10, 5, 0.25, 0.5, -1), b"max_chain"),
                       ((fake, buf, buf, buf, 1, 10, 5, 0.5, 0.5000001, 0), b"1 - p_kempe"),
                       ((fake, buf, buf, buf, 0, 10, 5, 1e-9, 1.0, 0), b"1 - p_kempe")):
        assert call(*args) == native.TT_ERR_INVALID, args
        assert word in lib.tt_last_error(), (args, lib.tt_last_error())
    for steps in (0, 1, 2 ** 31 - 1):                        # P = 0: no launch; every output may be NULL
        assert call(fake, buf, buf, buf, 0, steps, 1, 0.5, 0.5, 0) == native.TT_OK
        assert call(fake, buf, buf, buf, 0, steps, 500, 0.0, 1.0, 7, outs=None) == native.TT_OK
        assert call(fake, buf, buf, buf, 0, steps, 500, 1.0, 0.0, 0, outs=None) == native.TT_OK


# ---------------------------------------------------------------- the flags, Island, the line
PROB = "--lahc-kempe must be a probability in [0, 1]"
CHAIN = "--lahc-kempe-max-chain must be a non-negative integer"
BAD_FLAGS = ((["-i", "x.tim", "--lahc", "10", "--lahc-kempe", "1.5"], PROB),
             (["-i", "x.tim", "--lahc", "10", "--lahc-kempe", "-0.1"], PROB),
             (["-i", "x.tim", "--lahc", "10", "--lahc-kempe", "nan"], PROB),
             (["-i", "x.tim", "--lahc", "10", "--lahc-kempe", "half"], PROB),
             (["-i", "x.tim", "--lahc", "10", "--lahc-kempe"], PROB),
             (["-i", "x.tim", "--lahc", "10", "--lahc-kempe-max-chain", "-1"], CHAIN),
             (["-i", "x.tim", "--lahc", "10", "--lahc-kempe-max-chain", "2.5"], CHAIN),
             (["-i", "x.tim", "--lahc", "10", "--lahc-kempe-max-chain"], CHAIN),
             (["-i", "x.tim", "--lahc-kempe", "0.5", "--lahc-swap", "0.25"], "--lahc-kempe needs --lahc"),
             (["-i", "x.tim", "--lahc", "0", "--lahc-kempe", "0.5", "--lahc-swap", "0.25"], "--lahc-kempe needs --lahc"),
             # --lahc-swap's default is 0.5
             (["-i", "x.tim", "--lahc", "10", "--lahc-kempe", "0.75"],
              "--lahc-swap and --lahc-kempe must not add up to more than 1"),
             (["-i", "x.tim", "--lahc", "10", "--lahc-kempe", "0.5", "--lahc-swap", "0.75"],
              "--lahc-swap and --lahc-kempe must not add up to more than 1"))


def test_flags_in_the_control_parse():
    ctl = parse_control(["-i", "x.tim", "--lahc", "400", "--lahc-kempe", "0.5", "-s", "42"], out=Sink(), err=Sink())
    assert ctl["lahc"] == 400 and ctl["lahc_kempe"] == 0.5 and ctl["seed"] == 42 and ctl["input"] == "x.tim"
    assert "lahc_kempe_max_chain" not in ctl and "lahc_swap" not in ctl     # absent: Island's defaults
    ctl = parse_control(["--lahc-kempe-max-chain", "8", "--lahc-kempe", "0.75", "--lahc-swap", "0.25", "--lahc", "5",
                         "-i", "x.tim", "--kempe", "0.5", "--kempe-max-chain", "3"], out=Sink(), err=Sink())
    assert (ctl["lahc_kempe"], ctl["lahc_kempe_max_chain"], ctl["lahc_swap"], ctl["lahc"]) == (0.75, 8, 0.25, 5)
    assert (ctl["kempe"], ctl["kempe_max_chain"]) == (0.5, 3)
    # 0 goes with anything: tt_lahc as before
    ctl = parse_control(["-i", "x.tim", "--lahc-kempe", "0", "--lahc-swap", "1"], out=Sink(), err=Sink())
    assert ctl["lahc_kempe"] == 0 and "lahc" not in ctl
    assert "lahc_kempe" not in parse_control(["-i", "x.tim", "--lahc", "5"], out=Sink(), err=Sink())
    for bad, msg in BAD_FLAGS:
        rejected_by_parse_control(bad, msg, exact=True)


def test_flags_in_the_native_driver():
    for bad, msg in BAD_FLAGS:
        rejected_by_native_driver(bad, msg, exact=True)
    stripped_before_pair_count(["--lahc", "4", "--lahc-kempe", "0.5", "--lahc-kempe-max-chain", "7", "--lahc-swap", "0.5"])


def test_flags_are_in_the_table_for_the_tools():
    import argparse
    keys = [f.key for f in stages.FLAGS]
    assert keys.index("lahc_kempe") > keys.index("lahc_swap") and "lahc_kempe_max_chain" in stages.KEYS
    ap = argparse.ArgumentParser()
    stages.add_arguments(ap)
    ns = ap.parse_args(["--lahc", "7", "--lahc-kempe", "0.5", "--lahc-kempe-max-chain", "8"])
    kw = stages.island_kwargs(ns)
    assert (kw["lahc"], kw["lahc_kempe"], kw["lahc_kempe_max_chain"]) == (7, 0.5, 8)
    none = stages.island_kwargs(ap.parse_args([]))
    assert none["lahc_kempe"] == 0.0 and none["lahc_kempe_max_chain"] == 0


def test_validate():
    base = ("random", 0.0, 0, 0, 10, 500, 0.5, "uniform", False)
    stages.validate(*base)                                       # the two new parameters have defaults
    stages.validate(*base, 0.5, 0)
    stages.validate(*base, lahc_kempe=0.25, lahc_kempe_max_chain=8)
    stages.validate("random", 0.0, 0, 0, 0, 500, 1.0, "uniform", False, 0.0, 3)      # 0 goes with anything
    stages.validate("random", 0.0, 0, 0, 10, 500, 0.0, "uniform", False, 1.0)
    for args, message in (((*base, 1.5), r"lahc_kempe must be a probability in \[0, 1\]"),
                          ((*base, -0.1), r"lahc_kempe must be a probability in \[0, 1\]"),
                          ((*base, float("nan")), r"lahc_kempe must be a probability in \[0, 1\]"),
                          ((*base, 0.5, -1), r"lahc_kempe_max_chain must be >= 0 \(0: no cap\)"),
                          ((*base, 0.75), r"lahc_swap \+ lahc_kempe must be <= 1"),
                          (("random", 0.0, 0, 0, 0, 500, 0.5, "uniform", False, 0.5), "lahc_kempe > 0 needs lahc > 0")):
        with pytest.raises(ValueError, match=message):
            stages.validate(*args)


def test_island_checks_its_arguments_before_any_device_call():
    class NoDevice:                      # any use of it would raise AttributeError
        pass
    with pytest.raises(ValueError, match="lahc_kempe > 0 needs lahc > 0"):
        Island(NoDevice(), lahc_kempe=0.5, lahc_swap=0.25)
    with pytest.raises(ValueError, match=r"lahc_swap \+ lahc_kempe must be <= 1"):
        Island(NoDevice(), lahc=10, lahc_kempe=0.75)
    with pytest.raises(ValueError, match=r"lahc_kempe must be a probability in \[0, 1\]"):
        Island(NoDevice(), lahc=10, lahc_kempe=1.5)
    with pytest.raises(ValueError, match="lahc_kempe_max_chain must be >= 0"):
        Island(NoDevice(), lahc=10, lahc_kempe=0.5, lahc_kempe_max_chain=-2)


def test_lahc_kempe_line():
    line = lahc_kempe_line({"rows": 30, "tried": 900, "capped": 4, "no_room": 50, "accepted": 8, "chain_events": 20})
    assert line == '{"lahcKempe":{"accepted":8,"capped":4,"meanChain":2.5,"noRoom":50,"tried":900}}'
    assert '"meanChain":0,' in lahc_kempe_line({"tried": 0, "capped": 0, "no_room": 0, "accepted": 0,
                                                 "chain_events": 0})
