"""CPU checks of the augmenting-path room rule of the walk's Kempe chains (no
GPU): the model (tests/lahc_kempe_aug_model.py) against
tests/lahc_kempe_model.py where the rule cannot differ, what it rescues on sm,
its exactness against a maximum matching written here, the boundary of
tt_lahc_kempe_aug as a C++98 consumer sees it, its argument handling before any
device call, --lahc-kempe-rooms in both drivers' parse, stages.validate, Island
and the lahcKempe line."""
import ctypes
import pathlib
import shutil

import numpy as np
import pytest

import lahc_kempe_aug_model as am
import lahc_kempe_model as km
import lahc_model as lm
from stage_checks import (Sink, build_and_run_consumer, check_exports, rejected_by_native_driver,
                          rejected_by_parse_control, stripped_before_pair_count)
from ttga import native, stages
from ttga.ga import Island, lahc_kempe_line
from ttga.islands import parse_control

REPO = pathlib.Path(__file__).resolve().parent.parent
HEADER = REPO / "include" / "ttga_lahc_kempe_aug.h"
CONSUMER = REPO / "tests" / "boundary_lahc_kempe_aug_cxx98.cpp"
SM = ("sm", 33, 1000, 50, 0.25, 0.5)             # the GPU tests' sm case


@pytest.fixture(scope="module")
def sm():
    """sm's rows with the direct model's and the augmenting model's outputs."""
    shape, P, steps, L, p_swap, p_kempe = SM
    inst = lm.SHAPES[shape]()
    m = am.Model(inst)
    slot, room, seeds = lm.population(inst, P, m)
    direct = km.Model(inst).lahc_kempe_rows(slot, room, seeds, steps, L, p_swap, p_kempe)
    infos = []
    aug = m.lahc_kempe_aug_rows(slot, room, seeds, steps, L, p_swap, p_kempe, 0, 1, infos)
    return inst, m, (slot, room, seeds), direct, aug, [i for i in infos if i]


# ---------------------------------------------------------------- the model
def test_room_rule_0_is_the_direct_model(sm):
    inst, m, (slot, room, seeds), direct, _, _ = sm
    shape, P, steps, L, p_swap, p_kempe = SM
    got = m.lahc_kempe_aug_rows(slot, room, seeds, steps, L, p_swap, p_kempe, 0, 0)
    for g, w in zip(got[:6], direct[:6]):
        assert np.array_equal(g, w)
    assert np.array_equal(got[6][:, :5], direct[6]) and not got[6][:, 5:].any() and direct[6][:, 2].sum() > 0


@pytest.mark.parametrize("shape", ["tight_rooms", "R1"])
def test_where_no_path_can_help_the_rule_changes_nothing(shape):
    """Every room possible for every event, or one room: the holders of an
    event's possible rooms can go nowhere the event could not."""
    inst = lm.SHAPES[shape]()
    m = am.Model(inst)
    slot, room, seeds = lm.population(inst, 33, m)
    want = km.Model(inst).lahc_kempe_rows(slot, room, seeds, 1000, 50, 0.25, 0.5)
    got = m.lahc_kempe_aug_rows(slot, room, seeds, 1000, 50, 0.25, 0.5)
    for g, w in zip(got[:6], want[:6]):
        assert np.array_equal(g, w)
    assert np.array_equal(got[6][:, :5], want[6]) and not got[6][:, 5:].any() and want[6][:, 2].sum() > 0


def test_what_the_rule_rescues_on_sm(sm):
    _, _, _, direct, aug, infos = sm
    tried, capped, no_room, accepted, events, rescued, displaced = (int(x) for x in aug[6].sum(axis=0))
    print("sm direct", direct[6].sum(axis=0).tolist(), "augment", aug[6].sum(axis=0).tolist(),
          "longest path", max(i["longest_path"] for i in infos))
    assert tried == int(direct[6][:, 0].sum()) and capped == 0
    assert no_room < int(direct[6][:, 2].sum())
    assert rescued > 0 and displaced > 0
    assert max(i["longest_path"] for i in infos) >= 2                # some path changes at least 2 rooms
    assert sum(i["moved_chain_event"] for i in infos) > 0
    assert (aug[3] >= 0).all()


def has_complete_matching(poss, events):
    """Kuhn's depth-first search: can every event of `events` have a room of
    its own out of poss[event]?"""
    owner = {}

    def place(e, seen):
        for r in km._events(poss[e]):
            if r not in seen:
                seen.add(r)
                if r not in owner or place(owner[r], seen):
                    owner[r] = e
                    return True
        return False
    return all(place(e, set()) for e in events)


@pytest.mark.parametrize("shape,P,steps,L", [("sm", 8, 400, 50), ("med", 3, 300, 500), ("g300", 4, 400, 50)])
def test_no_room_is_exact_and_accepted_rows_are_feasible(shape, P, steps, L):
    import ttga
    inst = ttga.generate(300, 12, 5, 150, seed=22) if shape == "g300" else lm.SHAPES[shape]()
    m = am.Model(inst)
    slot, room, seeds = lm.population(inst, P, m)
    seen = {"refused": 0, "placed": 0, "accepted": 0}

    def on_kempe(s, r, kbits, a, t, result):
        after = {a: [], t: []}                                       # the events either slot would hold
        for e in range(inst.E):
            if int(s[e]) in after:
                after[a + t - int(s[e]) if (kbits >> e) & 1 else int(s[e])].append(e)
        complete = [has_complete_matching(m.poss, after[x]) for x in (a, t)]
        if result is None:
            assert not all(complete)
            seen["refused"] += 1
        else:
            assert all(complete)
            chain, displaced, _ = result
            rooms = {x: {} for x in (a, t)}
            for e in range(inst.E):
                if int(s[e]) in rooms and not (kbits >> e) & 1:
                    rooms[int(s[e])][e] = int(r[e])
            for e, x, q in chain + displaced:
                rooms[x][e] = q
            for x in (a, t):                                         # a complete assignment to possible rooms
                assert sorted(rooms[x]) == sorted(after[x]) and len(set(rooms[x].values())) == len(rooms[x])
                assert all((m.poss[e] >> q) & 1 for e, q in rooms[x].items())
            seen["placed"] += 1

    def on_accept(k, s, r, cur):
        assert m.valid(s, r) and m.hcv_of(s, r) == 0 and m.scv_of(s) == cur
        seen["accepted"] += 1
    for i in range(P):
        out = m.lahc_kempe_aug(slot[i], room[i], int(seeds[i]), steps, L, 0.25, 0.5, on_accept=on_accept,
                               on_kempe=on_kempe)
        assert m.valid(out[0], out[1]) or m.hcv_of(slot[i], room[i]) != 0
    print(shape, seen)
    assert seen["refused"] > 0 and seen["placed"] > 0 and seen["accepted"] > 0


# ---------------------------------------------------------------- the boundary
def test_header_symbol_is_exported_listed_and_called():
    check_exports(HEADER, "TTGA_LAHC_KEMPE_AUG_H", "LAHC_KEMPE_AUG_EXPORTS", CONSUMER, {"tt_lahc_kempe_aug"})
    assert '#include "ttga_lahc_kempe_aug.h"' in (REPO / "include" / "ttga_lahc.h").read_text()
    assert "1,552" in HEADER.read_text() and native.ROOM_RULES == ("direct", "augment")


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_cxx98_consumer_builds_and_links(tmp_path):
    build_and_run_consumer(CONSUMER, tmp_path)


def test_argument_errors_without_a_device():
    lib = native.load()
    buf = (ctypes.c_int32 * 64)()
    dbl = ctypes.c_double

    def call(h, slot, room, rng, P, steps, history, p_swap, p_kempe, max_chain, room_rule, outs=buf):
        return lib.tt_lahc_kempe_aug(h, slot, room, rng, P, steps, history, dbl(p_swap), dbl(p_kempe), max_chain,
                                     room_rule, outs, outs, outs, outs, outs, outs, None)
    assert call(None, buf, buf, buf, 1, 10, 5, 0.25, 0.5, 0, 1) == native.TT_ERR_INVALID
    assert b"null tt_problem" in lib.tt_last_error()
    fake = ctypes.cast((ctypes.c_uint8 * 8)(), ctypes.c_void_p)     # a stand-in handle the library must not look into
    for args, word in (((fake, None, buf, buf, 1, 10, 5, 0.25, 0.5, 0, 1), b"null population"),
                       ((fake, buf, buf, None, 1, 10, 5, 0.25, 0.5, 0, 1), b"rng"),
                       ((fake, buf, buf, buf, 1, -1, 5, 0.25, 0.5, 0, 1), b"steps"),
                       ((fake, buf, buf, buf, 1, 10, 0, 0.25, 0.5, 0, 1), b"history"),
                       ((fake, buf, buf, buf, 1, 10, 5, 1.5, 0.0, 0, 1), b"p_swap"),
                       ((fake, buf, buf, buf, 1, 10, 5, 0.25, float("nan"), 0, 1), b"p_kempe"),
                       ((fake, buf, buf, buf, 1, 10, 5, 0.25, 0.5, -1, 1), b"max_chain"),
                       ((fake, buf, buf, buf, 1, 10, 5, 0.25, 0.5, 0, -1), b"room_rule"),
                       ((fake, buf, buf, buf, 1, 10, 5, 0.25, 0.5, 0, 2), b"room_rule"),
                       ((fake, buf, buf, buf, 0, 10, 5, 0.25, 0.5, 0, 2), b"room_rule"),
                       ((fake, buf, buf, buf, 1, 10, 5, 0.5, 0.5000001, 0, 1), b"1 - p_kempe")):
        assert call(*args) == native.TT_ERR_INVALID, args
        assert word in lib.tt_last_error(), (args, lib.tt_last_error())
    for rule in (0, 1):                                      # P = 0: no launch; every output may be NULL
        assert call(fake, buf, buf, buf, 0, 10, 500, 0.0, 1.0, 7, rule, outs=None) == native.TT_OK


# ---------------------------------------------------------------- the flag, Island, the line
ROOMS = "--lahc-kempe-rooms must be direct or augment"
NEEDS = "--lahc-kempe-rooms augment needs --lahc-kempe"
WALK = ["-i", "x.tim", "--lahc", "10", "--lahc-swap", "0.25"]
BAD_FLAGS = (([*WALK, "--lahc-kempe", "0.5", "--lahc-kempe-rooms", "matching"], ROOMS),
             ([*WALK, "--lahc-kempe", "0.5", "--lahc-kempe-rooms", ""], ROOMS),
             ([*WALK, "--lahc-kempe", "0.5", "--lahc-kempe-rooms"], ROOMS),
             ([*WALK, "--lahc-kempe-rooms", "augment"], NEEDS),
             ([*WALK, "--lahc-kempe", "0", "--lahc-kempe-rooms", "augment"], NEEDS),
             (["-i", "x.tim", "--lahc-kempe-rooms", "augment"], NEEDS),
             # the older messages come first
             (["-i", "x.tim", "--lahc-kempe", "0.5", "--lahc-swap", "0.25", "--lahc-kempe-rooms", "augment"],
              stages.LAHC_KEMPE_NEEDS_LAHC))


def test_flag_in_the_control_parse():
    ctl = parse_control([*WALK, "--lahc-kempe", "0.5", "--lahc-kempe-rooms", "augment", "-s", "42"], out=Sink(),
                        err=Sink())
    assert ctl["lahc_kempe_rooms"] == "augment" and ctl["lahc_kempe"] == 0.5 and ctl["seed"] == 42
    ctl = parse_control(["--lahc-kempe-rooms", "direct", *WALK], out=Sink(), err=Sink())     # direct goes with anything
    assert ctl["lahc_kempe_rooms"] == "direct" and "lahc_kempe" not in ctl
    assert "lahc_kempe_rooms" not in parse_control([*WALK, "--lahc-kempe", "0.5"], out=Sink(), err=Sink())
    assert stages.LAHC_KEMPE_ROOMS_NEEDS_KEMPE == NEEDS
    for bad, msg in BAD_FLAGS:
        rejected_by_parse_control(bad, msg, exact=True)


def test_flag_in_the_native_driver():
    for bad, msg in BAD_FLAGS:
        rejected_by_native_driver(bad, msg, exact=True)
    stripped_before_pair_count(["--lahc", "4", "--lahc-kempe", "0.5", "--lahc-kempe-rooms", "augment"])


def test_flag_is_in_the_table_for_the_tools():
    import argparse
    f = {x.key: x for x in stages.FLAGS}["lahc_kempe_rooms"]
    assert (f.flag, f.kind, f.arg, f.message) == ("--lahc-kempe-rooms", "choice", ("direct", "augment"), ROOMS)
    ap = argparse.ArgumentParser()
    stages.add_arguments(ap)
    kw = stages.island_kwargs(ap.parse_args(["--lahc", "7", "--lahc-kempe", "0.5", "--lahc-kempe-rooms", "augment"]))
    assert (kw["lahc"], kw["lahc_kempe"], kw["lahc_kempe_rooms"]) == (7, 0.5, "augment")
    assert stages.island_kwargs(ap.parse_args([]))["lahc_kempe_rooms"] == "direct"


def test_validate():
    base = ("random", 0.0, 0, 0, 10, 500, 0.5, "uniform", False)
    stages.validate(*base)                                       # as before: the keyword has a default
    stages.validate(*base, 0.5, 0)
    stages.validate(*base, 0.5, 0, "direct")
    stages.validate(*base, 0.5, 0, lahc_kempe_rooms="augment")
    stages.validate(*base, lahc_kempe_rooms="direct")
    for args, kw, message in (((*base, 0.5, 0), dict(lahc_kempe_rooms="matching"),
                               "lahc_kempe_rooms must be 'direct' or 'augment'"),
                              ((*base,), dict(lahc_kempe_rooms="augment"),
                               "lahc_kempe_rooms='augment' needs lahc_kempe > 0"),
                              ((*base, 0.0, 4), dict(lahc_kempe_rooms="augment"),
                               "lahc_kempe_rooms='augment' needs lahc_kempe > 0")):
        with pytest.raises(ValueError, match=message):
            stages.validate(*args, **kw)


def test_island_checks_its_arguments_before_any_device_call():
    class NoDevice:                      # any use of it would raise AttributeError
        pass
    with pytest.raises(ValueError, match="lahc_kempe_rooms='augment' needs lahc_kempe > 0"):
        Island(NoDevice(), lahc=10, lahc_kempe_rooms="augment")
    with pytest.raises(ValueError, match="lahc_kempe_rooms must be 'direct' or 'augment'"):
        Island(NoDevice(), lahc=10, lahc_kempe=0.5, lahc_kempe_rooms="paths")


def test_lahc_kempe_line():
    five = {"rows": 30, "tried": 900, "capped": 4, "no_room": 50, "accepted": 8, "chain_events": 20}
    assert lahc_kempe_line(five) == '{"lahcKempe":{"accepted":8,"capped":4,"meanChain":2.5,"noRoom":50,"tried":900}}'
    line = lahc_kempe_line(dict(five, rescued=70, displaced=3))
    assert line == ('{"lahcKempe":{"accepted":8,"capped":4,"displaced":3,"meanChain":2.5,"noRoom":50,"rescued":70,'
                    '"tried":900}}')
