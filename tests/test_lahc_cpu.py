"""CPU checks of the late-acceptance search (no GPU): the model
(tests/lahc_model.py) against ttga.validate after every accepted step and
against a plain not-worse walk written here, the feasible share of the rows
that tests/test_gpu_lahc.py runs on, the boundary of include/ttga_lahc.h as a
C++98 consumer sees it, the argument handling of tt_lahc before any device
call, the --lahc flags in both drivers' parse, Island's argument checks and
the lahc line."""
import ctypes
import pathlib
import shutil

import numpy as np
import pytest

import ttga
import lahc_model as lm
from stage_checks import (Sink, build_and_run_consumer, check_exports, rejected_by_native_driver,
                          rejected_by_parse_control, stripped_before_pair_count)
from ttga import native
from ttga.ga import Island, lahc_line
from ttga.islands import parse_control
from ttga.rng import ParkMiller
from ttga.validate import evaluate

REPO = pathlib.Path(__file__).resolve().parent.parent
HEADER = REPO / "include" / "ttga_lahc.h"
CONSUMER = REPO / "tests" / "boundary_lahc_cxx98.cpp"


# ---------------------------------------------------------------- the model
@pytest.fixture(scope="module")
def small():
    out = {}
    for name, inst in (("E20", ttga.generate(20, 3, 2, 30, seed=11)), ("E61", ttga.generate(61, 5, 3, 40, seed=12))):
        m = lm.Model(inst)
        slot, room = lm.feasible_rows(inst, 6, 3, m)
        out[name] = (inst, m, slot, room)
    return out


@pytest.mark.parametrize("name", ["E20", "E61"])
@pytest.mark.parametrize("history,p_swap", [(1, 0.5), (20, 0.5), (300, 1.0), (20, 0.0)])
def test_every_accepted_step_is_feasible_and_costs_cur(small, name, history, p_swap):
    inst, m, slot, room = small[name]
    walked = 0
    for i in range(len(slot)):
        if evaluate(inst, slot[i], room[i])["hcv"] != 0:
            continue
        seen, touched, last = [], np.zeros(inst.E, bool), [slot[i].copy(), room[i].copy()]

        def on_accept(k, s, r, cur):
            ev = evaluate(inst, s, r)
            assert ev["hcv"] == 0 and ev["scv"] == cur, (k, ev, cur)
            seen.append(cur)
            changed = (s != last[0]) | (r != last[1])
            assert 1 <= changed.sum() <= 2 and (s != last[0]).sum() == changed.sum()
            touched[changed] = True
            last[0], last[1] = s.copy(), r.copy()
        info = {}
        s1, r1, state, gain, accepted, best_step = m.lahc(slot[i], room[i], 77 + i, 400, history, p_swap,
                                                          on_accept=on_accept, info=info)
        assert accepted == len(seen) > 0
        before, after = evaluate(inst, slot[i], room[i]), evaluate(inst, s1, r1)
        assert before["scv"] == info["scv0"] and after["hcv"] == 0 and after["scv"] == info["scv0"] - gain
        assert gain >= 0 and gain == info["scv0"] - min(seen + [info["scv0"]])
        assert (best_step == 0) == (gain == 0) and best_step <= 400
        assert np.array_equal(r1[~touched], room[i][~touched]) and np.array_equal(s1[~touched], slot[i][~touched])
        g = ParkMiller(77 + i)                                   # exactly three draws a step
        for _ in range(3 * 400):
            g.next()
        assert state == g.seed
        walked += 1
    assert walked >= 3


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
        out = m.lahc(s, r, 123, 200, 10)
        assert np.array_equal(out[0], s) and np.array_equal(out[1], r) and out[2:] == (123, 0, 0, 0)


def not_worse_walk(inst, m, slot, room, seed, steps):
    """Move1 only, accept iff the new scv (ttga.validate) is not above the
    current one; written from the rules, sharing nothing with Model.lahc but
    the instance's correlation and possible-room sets."""
    slot, room = slot.copy(), room.copy()
    g = ParkMiller(seed)
    corr, poss = inst.correlations(), inst.possible_rooms()
    cur = evaluate(inst, slot, room)["scv"]
    accepted = 0
    for _ in range(steps):
        e = g.pick(inst.E)
        g.next()
        t = int(g.next() * 44)
        t += t >= slot[e]
        there = np.flatnonzero(slot == t)
        if corr[e, there].any():
            continue
        rooms = [r for r in range(inst.R) if poss[e, r] and r not in room[there]]
        if not rooms:
            continue
        s2, r2 = slot.copy(), room.copy()
        s2[e], r2[e] = t, rooms[0]
        new = evaluate(inst, s2, r2)["scv"]
        if new <= cur:
            slot, room, cur, accepted = s2, r2, new, accepted + 1
    return slot, room, g.seed, cur, accepted


@pytest.mark.parametrize("name", ["E20", "E61"])
def test_history_1_without_swaps_is_a_plain_not_worse_walk(small, name):
    inst, m, slot, room = small[name]
    i = next(i for i in range(len(slot)) if evaluate(inst, slot[i], room[i])["hcv"] == 0)
    s, r, state, cur, accepted = not_worse_walk(inst, m, slot[i], room[i], 4242, 600)
    info = {}
    out = m.lahc(slot[i], room[i], 4242, 600, 1, 0.0, info=info)
    assert accepted > 0 and out[4] == accepted and out[2] == state
    assert np.array_equal(info["cur_slot"], s) and np.array_equal(info["cur_room"], r) and info["cur"] == cur
    assert out[3] == info["scv0"] - cur                          # never worse: the last cost is the best
    assert evaluate(inst, out[0], out[1])["scv"] == cur


# ---------------------------------------------------------------- the rows of the GPU cases
@pytest.mark.parametrize("shape", list(lm.SHAPES))
def test_gpu_rows_are_at_least_half_feasible(shape):
    """So that tests/test_gpu_lahc.py cannot pass on closed gates alone. Two
    shapes have no feasible row at all, which is shown here from the
    instance; tight_rooms and syn_sparse stand beside them."""
    inst = lm.SHAPES[shape]()
    P = max(p for s, p, _, _, _ in lm.CASES.values() if s == shape)
    if shape == "tight":
        assert (inst.possible_rooms().sum(axis=1) == 0).sum() == 27            # events no room is possible for
        return
    if shape == "syn":
        assert inst.E > 45 * inst.R                                            # more events than cells
        return
    m = lm.Model(inst)
    slot, room, seeds = lm.population(inst, P, m)
    feasible = sum(m.hcv_of(slot[i], room[i]) == 0 for i in range(P))      # the validator's: test_model_hcv_is_...
    print(shape, feasible, "of", P)
    assert 2 * feasible >= P
    assert feasible < P or inst.E < 2 or P < 3                                 # and some rows are not
    assert seeds.min() >= 1 and seeds.max() < 2 ** 31 - 1


def test_model_hcv_is_the_validators():
    inst = ttga.config_instance("sm")
    m = lm.Model(inst)
    g = np.random.default_rng(1)
    for _ in range(3):
        s, r = g.integers(0, 45, inst.E), g.integers(0, inst.R, inst.E)
        ev = evaluate(inst, s, r)
        assert m.hcv_of(s, r) == ev["hcv"] and m.scv_of(s) == ev["scv"]


# ---------------------------------------------------------------- the boundary
def test_header_symbols_are_exported_listed_and_called():
    check_exports(HEADER, "TTGA_LAHC_H", "LAHC_EXPORTS", CONSUMER, {"tt_lahc"})
    assert '#include "ttga.h"' in HEADER.read_text()
    top = (REPO / "include" / "ttga.h").read_text()
    assert "ttga_lahc.h" in top and "bit 8 (256)" in top


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_cxx98_lahc_consumer_builds_and_links(tmp_path):
    build_and_run_consumer(CONSUMER, tmp_path)


def test_argument_errors_without_a_device():
    lib = native.load()
    buf = (ctypes.c_int32 * 64)()
    dbl = ctypes.c_double

    def call(h, slot, room, rng, P, steps, history, p_swap, outs=buf):
        return lib.tt_lahc(h, slot, room, rng, P, steps, history, dbl(p_swap), outs, outs, outs, outs, outs, None)
    # a null handle is named, whatever else is wrong
    for args in ((None, buf, buf, buf, 1, 10, 5, 0.5), (None, None, None, None, -1, -1, 0, 2.0),
                 (None, buf, buf, buf, 0, 10, 5, 0.5)):
        assert call(*args) == native.TT_ERR_INVALID
        assert b"null tt_problem" in lib.tt_last_error()
    # with a handle, every argument is checked before any device call: a stand-in
    # handle that the library must not look into
    fake = ctypes.cast((ctypes.c_uint8 * 8)(), ctypes.c_void_p)
    for args, word in (((fake, None, buf, buf, 1, 10, 5, 0.5), b"null population"),
                       ((fake, buf, None, buf, 1, 10, 5, 0.5), b"null population"),
                       ((fake, buf, buf, None, 1, 10, 5, 0.5), b"rng"),
                       ((fake, buf, buf, buf, -1, 10, 5, 0.5), b"negative population"),
                       ((fake, buf, buf, buf, 1, -1, 5, 0.5), b"steps"),
                       ((fake, buf, buf, buf, 1, 10, 0, 0.5), b"history"),
                       ((fake, buf, buf, buf, 0, 10, -4, 0.5), b"history"),
                       ((fake, buf, buf, buf, 1, 10, 5, 1.0000001), b"p_swap"),
                       ((fake, buf, buf, buf, 1, 10, 5, -1e-9), b"p_swap"),
                       ((fake, buf, buf, buf, 0, 10, 5, float("nan")), b"p_swap")):
        assert call(*args) == native.TT_ERR_INVALID, args
        assert word in lib.tt_last_error(), (args, lib.tt_last_error())
    for steps in (0, 1, 2 ** 31 - 1):                        # P = 0: no launch; every output may be NULL
        assert call(fake, buf, buf, buf, 0, steps, 1, 0.0) == native.TT_OK
        assert call(fake, buf, buf, buf, 0, steps, 500, 1.0, outs=None) == native.TT_OK


# ---------------------------------------------------------------- the flags, Island, the line
BAD_FLAGS = ((["-i", "x.tim", "--lahc", "-1"], "--lahc must be a non-negative integer"),
             (["-i", "x.tim", "--lahc"], "--lahc must be a non-negative integer"),
             (["-i", "x.tim", "--lahc", "2.5"], "--lahc must be a non-negative integer"),
             (["-i", "x.tim", "--lahc", "many"], "--lahc must be a non-negative integer"),
             (["-i", "x.tim", "--lahc-history", "0"], "--lahc-history must be a positive integer"),
             (["-i", "x.tim", "--lahc-history", "x"], "--lahc-history must be a positive integer"),
             (["-i", "x.tim", "--lahc-swap", "1.5"], "--lahc-swap must be a probability in [0, 1]"),
             (["-i", "x.tim", "--lahc-swap", "nan"], "--lahc-swap must be a probability in [0, 1]"),
             (["-i", "x.tim", "--lahc-swap"], "--lahc-swap must be a probability in [0, 1]"))


def test_lahc_flags_in_the_control_parse():
    ctl = parse_control(["-i", "x.tim", "--lahc", "400", "-s", "42"], out=Sink(), err=Sink())
    assert ctl["lahc"] == 400 and ctl["seed"] == 42 and ctl["input"] == "x.tim"
    assert "lahc_history" not in ctl and "lahc_swap" not in ctl           # absent: Island's defaults
    ctl = parse_control(["--lahc-swap", "0.25", "--lahc", "0", "--lahc-history", "1", "-i", "x.tim"], out=Sink(),
                        err=Sink())
    assert (ctl["lahc"], ctl["lahc_history"], ctl["lahc_swap"]) == (0, 1, 0.25)
    assert "lahc" not in parse_control(["-i", "x.tim", "-s", "42"], out=Sink(), err=Sink())
    both = parse_control(["--unique", "-i", "x.tim", "--slot-swap", "1", "--lahc", "2000", "--pop", "20"], out=Sink(),
                         err=Sink())
    assert both["slot_swap"] == 1 and both["lahc"] == 2000 and both["unique"] is True and both["pop"] == 20
    for bad, msg in BAD_FLAGS:
        rejected_by_parse_control(bad, msg, exact=True)


def test_lahc_flags_in_the_native_driver():
    for bad, msg in BAD_FLAGS:
        rejected_by_native_driver(bad, msg, exact=True)
    stripped_before_pair_count(["--lahc", "4", "--lahc-history", "7", "--lahc-swap", "0.5"])


def test_island_checks_its_lahc_arguments_before_any_device_call():
    class NoDevice:                      # any use of it would raise AttributeError
        pass
    with pytest.raises(ValueError, match=r"lahc must be >= 0 \(0: off\)"):
        Island(NoDevice(), lahc=-1)
    with pytest.raises(ValueError, match="lahc_history must be >= 1"):
        Island(NoDevice(), lahc=10, lahc_history=0)
    for bad in (-0.1, 1.1, float("nan")):
        with pytest.raises(ValueError, match=r"lahc_swap must be a probability in \[0, 1\]"):
            Island(NoDevice(), lahc=10, lahc_swap=bad)


def test_lahc_line():
    line = lahc_line({"rows": 30, "searched": 21, "improved": 7, "accepted": 160, "gain": 41})
    assert line == '{"lahc":{"accepted":160,"gain":41,"improved":7,"rows":30,"searched":21}}'
