"""CPU checks of the walk's parallel walkers (no GPU): the thin model
(tests/lahc_multi_model.py) against tests/lahc_kempe_aug_model.py with one
walker, its seed chaining against ttga.rng.step, the winner rule on constructed
rows, what the GPU cases must show, the boundary of tt_lahc_multi as a C++98
consumer sees it, its argument handling before any device call, --lahc-walkers
in both drivers' parse, stages.validate, Island and the lahcWalkers line."""
import ctypes
import pathlib
import shutil

import numpy as np
import pytest

import lahc_kempe_aug_model as am
import lahc_model as lm
import lahc_multi_model as mm
from stage_checks import (Sink, build_and_run_consumer, check_exports, rejected_by_native_driver,
                          rejected_by_parse_control, stripped_before_pair_count)
from ttga import native, stages
from ttga.ga import Island, lahc_walkers_line
from ttga.islands import parse_control
from ttga.rng import step

REPO = pathlib.Path(__file__).resolve().parent.parent
PKG = REPO / "timetabling-ga-mpi-openmp_amd"
HEADER = REPO / "include" / "ttga_lahc_multi.h"
CONSUMER = REPO / "tests" / "boundary_lahc_multi_cxx98.cpp"
SM = (9, 300, 50, 0.25, 0.5)                     # P, steps, history, p_swap, p_kempe on sm


@pytest.fixture(scope="module")
def sm():
    inst = lm.SHAPES["sm"]()
    m = mm.Model(inst)
    return inst, m, lm.population(inst, SM[0], m)


# ---------------------------------------------------------------- the model
@pytest.mark.parametrize("rule", [0, 1])
def test_one_walker_is_the_walk(sm, rule):
    inst, m, (slot, room, seeds) = sm
    P, steps, L, p_swap, p_kempe = SM
    want = am.Model(inst).lahc_kempe_aug_rows(slot, room, seeds, steps, L, p_swap, p_kempe, 0, rule)
    got = m.lahc_multi_rows(slot, room, seeds, 1, steps, L, p_swap, p_kempe, 0, rule)
    for g, w in zip(got[:7], want):
        assert np.array_equal(g, w)
    assert not got[7].any() and np.array_equal(got[8][:, 0], want[3]) and want[3].sum() > 0


def test_seed_chaining_is_three_draws_a_step(sm):
    """Walker w starts 3 * steps * w draws on, the row's state ends 3 * steps *
    K draws on, and every walker equals the single walk started there."""
    inst, m, (slot, room, seeds) = sm
    P, steps, L, p_swap, p_kempe = SM
    K, single = 4, am.Model(inst)
    for i in (0, 1):
        got = m.lahc_multi(slot[i], room[i], int(seeds[i]), K, steps, L, p_swap, p_kempe)
        s, gains = int(seeds[i]), []
        for w in range(K):
            gains.append(single.lahc_kempe_aug(slot[i], room[i], s, steps, L, p_swap, p_kempe)[3])
            for _ in range(3 * steps):
                s = step(s)
        assert got[2] == s and got[8] == tuple(gains) and got[3] == max(gains)
    closed = m.lahc_multi(slot[2], room[2], int(seeds[2]), K, steps, L, p_swap, p_kempe)     # row 2 is spoiled
    assert closed[2] == int(seeds[2]) and closed[3:] == (0, 0, 0, (0,) * 7, 0, (0,) * K)
    assert np.array_equal(closed[0], slot[2]) and np.array_equal(closed[1], room[2])
    still = m.lahc_multi(slot[0], room[0], int(seeds[0]), K, 0, L, p_swap, p_kempe)          # steps 0
    assert still[2] == int(seeds[0]) and still[3:] == (0, 0, 0, (0,) * 7, 0, (0,) * K)


def test_a_later_walker_wins_and_the_row_is_its_row(sm):
    inst, m, (slot, room, seeds) = sm
    P, steps, L, p_swap, p_kempe = SM
    out = m.lahc_multi_rows(slot, room, seeds, 5, steps, L, p_swap, p_kempe)
    later = np.flatnonzero(out[7] > 0)
    assert later.size > 0
    single = am.Model(inst)
    for i in later[:2]:
        w, s = int(out[7][i]), int(seeds[i])
        assert out[8][i, w] == out[8][i].max() == out[3][i] and (out[8][i, :w] < out[3][i]).all()
        for _ in range(3 * steps * w):
            s = step(s)
        walk = single.lahc_kempe_aug(slot[i], room[i], s, steps, L, p_swap, p_kempe)
        assert np.array_equal(walk[0], out[0][i]) and np.array_equal(walk[1], out[1][i])
        assert (walk[3], walk[4], walk[5]) == (out[3][i], out[4][i], out[5][i]) and walk[6] == tuple(out[6][i])
        assert m.hcv_of(out[0][i], out[1][i]) == 0 and m.scv_of(out[0][i]) == m.scv_of(slot[i]) - out[3][i]


class Scripted(mm.Model):
    """The walk replaced by a script of gains: walker w comes back with gain
    script[w] and a row that says which walker it was (slot gene 0 = w)."""

    def __init__(self, inst, script):
        mm.Model.__init__(self, inst)
        self.script, self.calls = script, 0

    def lahc_kempe_aug(self, slot, room, seed, *a, **k):
        w, self.calls = self.calls, self.calls + 1
        s = np.array(slot, np.uint8)
        s[0] = w
        return s, np.array(room, np.uint8), step(int(seed)), self.script[w], 10 + w, 20 + w, (w,) * 7


@pytest.mark.parametrize("script, winner", [((3, 5, 5, 2), 1), ((7, 7, 7), 0), ((0, 0, 0, 0), 0), ((1, 2, 3), 2),
                                            ((0, 4, 0, 4), 1)])
def test_ties_go_to_the_lowest_walker(sm, script, winner):
    inst, _, (slot, room, seeds) = sm
    m = Scripted(inst, script)
    out = m.lahc_multi(slot[0], room[0], 5, len(script), 10, 5)
    assert m.calls == len(script) and out[7] == winner and out[8] == script and out[3] == script[winner]
    assert out[0][0] == winner and (out[4], out[5], out[6]) == (10 + winner, 20 + winner, (winner,) * 7)
    s = 5
    for _ in script:
        s = step(s)
    assert out[2] == s                                               # the state behind the last walker


def test_a_tie_in_a_real_walk():
    """E2: two events, so every walker of a row that can improve finds the same
    gain: walker 0 keeps the row."""
    inst = lm.SHAPES["E2"]()
    m = mm.Model(inst)
    shape, P, K, steps, L, p_swap, p_kempe, rule = mm.CASES["E2"]
    slot, room, seeds = mm.case_rows("E2", inst, m)
    out = m.lahc_multi_rows(slot, room, seeds, K, steps, L, p_swap, p_kempe, 0, rule)
    tied = np.flatnonzero((out[8] > 0).all(axis=1) & (out[8] == out[8][:, :1]).all(axis=1))
    assert tied.size > 0 and not out[7][tied].any()


def test_what_the_gpu_cases_must_show():
    """Over the GPU tests' cases: some row is won by a walker other than 0, some
    walked row has winner 0 with gain 0, and the out-of-range seed's row walks."""
    later = idle = 0
    for cid in ("sm-plain", "sm", "S0"):
        shape, P, K, steps, L, p_swap, p_kempe, rule = mm.CASES[cid]
        inst = lm.SHAPES[shape]()
        m = mm.Model(inst)
        slot, room, seeds = mm.case_rows(cid, inst, m)
        out = m.lahc_multi_rows(slot, room, seeds, K, steps, L, p_swap, p_kempe, 0, rule)
        walked = np.array([m.hcv_of(slot[i], room[i]) == 0 for i in range(P)])
        later += int((out[7] > 0).sum())
        idle += int((walked & (out[7] == 0) & (out[3] == 0)).sum())
        assert (out[2][walked] != seeds[walked]).all() and np.array_equal(out[2][~walked], seeds[~walked])
        if cid == "sm":
            assert seeds[0] == mm.WIDE_SEED == 2 ** 40 + 7 and walked[0] and out[3][0] > 0
            s = int(seeds[0])
            for _ in range(3 * steps * K):
                s = step(s)
            assert out[2][0] == s
    assert later > 0 and idle > 0


# ---------------------------------------------------------------- the boundary
def test_header_symbols_are_exported_listed_and_called():
    check_exports(HEADER, "TTGA_LAHC_MULTI_H", "LAHC_MULTI_EXPORTS", CONSUMER,
                  {"tt_lahc_multi", "tt_lahc_multi_work_bytes"})
    text = (REPO / "include" / "ttga_lahc.h").read_text()
    assert text.index('#include "ttga_lahc_kempe_aug.h"') < text.index('#include "ttga_lahc_multi.h"')
    assert "1,552" in HEADER.read_text() and native.MAX_WALKERS == 1024


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_cxx98_consumer_builds_and_links(tmp_path):
    build_and_run_consumer(CONSUMER, tmp_path)


def test_argument_errors_without_a_device():
    lib = native.load()
    buf = (ctypes.c_int64 * 64)()
    dbl = ctypes.c_double

    def call(h, slot, room, rng, P, walkers, steps, history, p_swap, p_kempe, max_chain, room_rule, outs=buf, work=buf):
        return lib.tt_lahc_multi(h, slot, room, rng, P, walkers, steps, history, dbl(p_swap), dbl(p_kempe), max_chain,
                                 room_rule, outs, outs, outs, outs, outs, outs, outs, outs, work, None)
    assert call(None, buf, buf, buf, 1, 4, 10, 5, 0.25, 0.5, 0, 1) == native.TT_ERR_INVALID
    assert b"null tt_problem" in lib.tt_last_error()
    assert lib.tt_lahc_multi_work_bytes(None, 4, 4) == 0
    fake = ctypes.cast((ctypes.c_uint8 * 8)(), ctypes.c_void_p)     # a stand-in handle the library must not look into
    for args, kw, word in (((fake, None, buf, buf, 1, 4, 10, 5, 0.25, 0.5, 0, 1), {}, b"null population"),
                           ((fake, buf, buf, None, 1, 4, 10, 5, 0.25, 0.5, 0, 1), {}, b"rng"),
                           ((fake, buf, buf, buf, 1, 0, 10, 5, 0.25, 0.5, 0, 1), {}, b"walkers"),
                           ((fake, buf, buf, buf, 1, -1, 10, 5, 0.25, 0.5, 0, 1), {}, b"walkers"),
                           ((fake, buf, buf, buf, 1, 1025, 10, 5, 0.25, 0.5, 0, 1), {}, b"walkers"),
                           ((fake, buf, buf, buf, 1, 4, -1, 5, 0.25, 0.5, 0, 1), {}, b"steps"),
                           ((fake, buf, buf, buf, 1, 4, 10, 0, 0.25, 0.5, 0, 1), {}, b"history"),
                           ((fake, buf, buf, buf, 1, 4, 10, 5, 1.5, 0.0, 0, 1), {}, b"p_swap"),
                           ((fake, buf, buf, buf, 1, 4, 10, 5, 0.25, float("nan"), 0, 1), {}, b"p_kempe"),
                           ((fake, buf, buf, buf, 1, 4, 10, 5, 0.25, 0.5, -1, 1), {}, b"max_chain"),
                           ((fake, buf, buf, buf, 1, 4, 10, 5, 0.25, 0.5, 0, 2), {}, b"room_rule"),
                           ((fake, buf, buf, buf, 0, 4, 10, 5, 0.25, 0.5, 0, -1), {}, b"room_rule"),
                           ((fake, buf, buf, buf, 1, 4, 10, 5, 0.5, 0.5000001, 0, 1), {}, b"1 - p_kempe"),
                           ((fake, buf, buf, buf, 1, 2, 10, 5, 0.25, 0.5, 0, 1), dict(work=None), b"work"),
                           ((fake, buf, buf, buf, 0, 1024, 10, 5, 0.25, 0.5, 0, 1), dict(work=None), b"work"),
                           ((fake, buf, buf, buf, 1, 2, 10, 5, 0.25, 0.5, 0, 1),
                            dict(work=ctypes.c_void_p(ctypes.addressof(buf) + 4)), b"work")):
        assert call(*args, **kw) == native.TT_ERR_INVALID, args
        assert word in lib.tt_last_error(), (args, lib.tt_last_error())
    for K, work in ((1, None), (1, buf), (64, buf), (1024, buf)):      # P = 0: no launch; every output may be NULL
        assert call(fake, buf, buf, buf, 0, K, 10, 500, 0.0, 1.0, 7, 1, outs=None, work=work) == native.TT_OK


# ---------------------------------------------------------------- the flag, Island, the line
RANGE = "--lahc-walkers must be an integer from 1 to 1024"
NEEDS = "--lahc-walkers needs --lahc"
WALK = ["-i", "x.tim", "--lahc", "10"]
BAD_FLAGS = (([*WALK, "--lahc-walkers", "0"], RANGE), ([*WALK, "--lahc-walkers", "1025"], RANGE),
             ([*WALK, "--lahc-walkers", "-4"], RANGE), ([*WALK, "--lahc-walkers", "2.5"], RANGE),
             ([*WALK, "--lahc-walkers", "many"], RANGE), ([*WALK, "--lahc-walkers"], RANGE),
             (["-i", "x.tim", "--lahc-walkers", "4"], NEEDS),
             (["-i", "x.tim", "--lahc", "0", "--lahc-walkers", "4"], NEEDS),
             # the older messages come first
             (["-i", "x.tim", "--lahc-kempe", "0.5", "--lahc-swap", "0.25", "--lahc-walkers", "4"],
              stages.LAHC_KEMPE_NEEDS_LAHC),
             ([*WALK, "--lahc-kempe-rooms", "augment", "--lahc-walkers", "4"], stages.LAHC_KEMPE_ROOMS_NEEDS_KEMPE))


def test_flag_in_the_control_parse():
    ctl = parse_control([*WALK, "--lahc-walkers", "16", "-s", "42"], out=Sink(), err=Sink())
    assert ctl["lahc_walkers"] == 16 and ctl["lahc"] == 10 and ctl["seed"] == 42
    ctl = parse_control(["--lahc-walkers", "1", "-i", "x.tim"], out=Sink(), err=Sink())      # 1 goes with anything
    assert ctl["lahc_walkers"] == 1 and "lahc" not in ctl
    assert "lahc_walkers" not in parse_control(WALK, out=Sink(), err=Sink())
    assert parse_control([*WALK, "--lahc-walkers", "1024"], out=Sink(), err=Sink())["lahc_walkers"] == 1024
    assert stages.LAHC_WALKERS_NEEDS_LAHC == NEEDS
    for bad, msg in BAD_FLAGS:
        rejected_by_parse_control(bad, msg, exact=True)


def test_flag_in_the_native_driver():
    assert f'"{NEEDS}"' in (PKG / "host" / "ttga_ga.cpp").read_text()
    for bad, msg in BAD_FLAGS:
        rejected_by_native_driver(bad, msg, exact=True)
    stripped_before_pair_count(["--lahc", "4", "--lahc-walkers", "4"])


def test_flag_is_in_the_table_for_the_tools():
    import argparse
    keys = [x.key for x in stages.FLAGS]
    f = stages.FLAGS[keys.index("lahc_walkers")]
    assert (f.flag, f.kind, f.arg, f.message) == ("--lahc-walkers", "int", (1, 1024), RANGE)
    assert keys.index("lahc_walkers") == max(i for i, k in enumerate(keys) if k.startswith("lahc")) \
        == keys.index("lahc_kempe_rooms") + 1                        # behind the other --lahc flags
    ap = argparse.ArgumentParser()
    stages.add_arguments(ap)
    kw = stages.island_kwargs(ap.parse_args(["--lahc", "7", "--lahc-walkers", "16"]))
    assert (kw["lahc"], kw["lahc_walkers"]) == (7, 16)
    assert stages.island_kwargs(ap.parse_args([]))["lahc_walkers"] == 1


def test_validate():
    base = ("random", 0.0, 0, 0, 10, 500, 0.5, "uniform", False)
    stages.validate(*base)                                       # as before: the keyword has a default
    stages.validate(*base, 0.5, 0, "augment")
    stages.validate(*base, 0.5, 0, "augment", 16)
    stages.validate(*base, lahc_walkers=1024)
    stages.validate("random", 0.0, 0, 0, 0, 500, 0.5, "uniform", False, lahc_walkers=1)      # no walk, one walker
    for args, kw, message in (((*base,), dict(lahc_walkers=0), "lahc_walkers must be from 1 to 1024"),
                              ((*base,), dict(lahc_walkers=1025), "lahc_walkers must be from 1 to 1024"),
                              (("random", 0.0, 0, 0, 0, 500, 0.5, "uniform", False), dict(lahc_walkers=2),
                               "lahc_walkers > 1 needs lahc > 0")):
        with pytest.raises(ValueError, match=message):
            stages.validate(*args, **kw)


def test_island_checks_its_arguments_before_any_device_call():
    class NoDevice:                      # any use of it would raise AttributeError
        pass
    with pytest.raises(ValueError, match="lahc_walkers > 1 needs lahc > 0"):
        Island(NoDevice(), lahc_walkers=4)
    with pytest.raises(ValueError, match="lahc_walkers must be from 1 to 1024"):
        Island(NoDevice(), lahc=10, lahc_walkers=0)
    with pytest.raises(ValueError, match="lahc_walkers must be from 1 to 1024"):
        Island(NoDevice(), lahc=10, lahc_walkers=2000)


def test_lahc_walkers_line():
    stats = {"rows": 30, "walkers": 16, "gain": 900, "gainFirst": 640, "winnerLater": 21}
    assert lahc_walkers_line(stats) == ('{"lahcWalkers":{"gain":900,"gainFirst":640,"rows":30,"walkers":16,'
                                        '"winnerLater":21}}')
