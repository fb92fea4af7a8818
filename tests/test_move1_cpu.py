"""CPU checks of the single-event neighbourhood (no GPU): the model
(tests/move1_model.py) against lahc_model.Model.scv_of and hcv_of on whole small
rows, the descent's early stop, the planted defects that the GPU comparison
of tests/test_gpu_move1.py must be able to see, the boundary of
include/ttga/move1.h as a C++98 consumer sees it, the argument handling of
both entry points before any device call, the --move1-descent flag in both
drivers' parse, Island's argument check and the move1Descent line."""
import ctypes
import pathlib
import shutil

import numpy as np
import pytest

import ttga
import lahc_model as lm
import move1_model as mm
from stage_checks import (Sink, build_and_run_consumer, check_exports, rejected_by_native_driver,
                          rejected_by_parse_control, stripped_before_pair_count)
from ttga import native, stages
from ttga.ga import Island, move1_descent_line
from ttga.islands import parse_control

REPO = pathlib.Path(__file__).resolve().parent.parent
PKG = REPO / "timetabling-ga-mpi-openmp_amd"
HEADER = REPO / "include" / "ttga" / "move1.h"
CONSUMER = REPO / "tests" / "boundary_move1_cxx98.cpp"
INT_MAX = 2 ** 31 - 1


# ---------------------------------------------------------------- the model
@pytest.fixture(scope="module")
def small():
    """Feasible rows of small instances (E <= 65): few rooms, so that every
    kind of to_room entry occurs."""
    out = {}
    for name, inst in (("E20", ttga.generate(20, 3, 2, 30, seed=11)), ("E61", ttga.generate(61, 5, 3, 40, seed=12)),
                       ("E65", lm.SHAPES["E65"]()), ("R1", lm.SHAPES["R1"]())):
        m = mm.Model(inst)
        slot, room = lm.feasible_rows(inst, 4, 3, m)
        keep = [i for i in range(len(slot)) if m.scanned(slot[i], room[i])]
        assert len(keep) >= 2, name
        out[name] = (inst, m, slot[keep], room[keep])
    return out


@pytest.mark.parametrize("name", ["E20", "E61", "E65", "R1"])
def test_d_scv_is_the_difference_of_whole_row_costs_and_feasible_moves_keep_hcv_0(small, name):
    """Every (e, t) of whole rows: d_scv against scv_of of the moved row, whether
    or not the move is feasible; every feasible entry applied keeps hcv_of at
    0, every other off-diagonal entry breaks it."""
    inst, m, slot, room = small[name]
    kinds = set()
    for i in range(2):
        sm, d, tr = m.scan(slot[i], room[i])
        scv0 = m.scv_of(slot[i])
        for e in range(inst.E):
            for t in range(45):
                s2, r2 = slot[i].copy(), room[i].copy()
                s2[e] = t
                assert m.scv_of(s2) - scv0 == d[e, t], (e, t)
                if t == slot[i][e]:
                    assert tr[e, t] == room[i][e] and d[e, t] == 0
                    continue
                kinds.add(int(tr[e, t]) if tr[e, t] >= mm.NO_ROOM else "room")
                if tr[e, t] < 64:
                    r2[e] = tr[e, t]
                    assert m.hcv_of(s2, r2) == 0, (e, t)
                else:
                    assert all(m.hcv_of(s2, np.where(np.arange(inst.E) == e, r, r2)) > 0 for r in range(inst.R)), (e, t)
        feas = (tr < 64) & (np.arange(45)[None, :] != slot[i][:, None])
        assert sm[0] == 1 and sm[1] == feas.sum() and sm[2] == (feas & (d < 0)).sum() and sm[3] == d[feas].min()
        assert feas[sm[4], sm[5]] and d[sm[4], sm[5]] == sm[3]
        first = np.argwhere(feas & (d == sm[3]))[0]
        assert (sm[4], sm[5]) == tuple(first)                              # the least event, then the least slot
    assert "room" in kinds and mm.CLASH in kinds
    if name in ("E65", "R1"):
        assert mm.NO_ROOM in kinds


def test_model_leaves_infeasible_and_invalid_rows_unscanned(small):
    inst, m, slot, room = small["E61"]
    for spoil in ("pair", "slot", "room"):
        s, r = slot[0].copy(), room[0].copy()
        if spoil == "pair":
            s[1], r[1] = s[0], r[0]
        elif spoil == "slot":
            s[5] = 45
        else:
            r[5] = inst.R
        sm, d, tr = m.scan(s, r)
        assert tuple(sm) == mm.UNSCANNED_SUMMARY and (d == mm.NONE).all() and (tr == mm.UNSCANNED).all()
        out = m.descent(s, r, 5)
        assert np.array_equal(out[0], s) and np.array_equal(out[1], r) and out[2:] == (0, 0)


@pytest.mark.parametrize("name", ["E20", "E61"])
def test_descent_falls_strictly_keeps_rooms_and_stops_at_a_local_optimum(small, name):
    inst, m, slot, room = small[name]
    for i in range(len(slot)):
        scv0 = m.scv_of(slot[i])
        trail = [scv0]
        for k in range(1, 4):                                               # capped: k rounds of scan + apply
            s, r, gain, passes = m.descent(slot[i], room[i], k)
            assert passes <= k and m.hcv_of(s, r) == 0 and m.scv_of(s) == scv0 - gain
            trail.append(scv0 - gain)
            moved = s != slot[i]
            assert moved.sum() <= passes and np.array_equal(r[~moved], room[i][~moved])
        s, r, gain, passes = m.descent(slot[i], room[i], INT_MAX)
        assert passes > 0 and gain >= passes                                # every pass lowers scv by at least 1
        assert all(a > b for a, b in zip(trail, trail[1:])) or passes < 3
        sm, d, tr = m.scan(s, r)
        assert sm[0] == 1 and sm[2] == 0                                    # an early stop: no improving move is left
        short = m.descent(slot[i], room[i], passes)                         # the cap at the natural length changes nothing
        assert np.array_equal(short[0], s) and short[2:] == (gain, passes)


# ---------------------------------------------------------------- planted defects
def test_planted_defects_show_in_the_compared_outputs():
    """What a kernel could get wrong without breaking an invariant: each defect
    changes an output that tests/test_gpu_move1.py compares bit for bit, on the
    rows it runs (sm, and R1 for the rooms)."""
    inst = lm.SHAPES["sm"]()
    m = mm.Model(inst)
    slot, room = mm.population(inst, 12, m)
    rows = [i for i in range(12) if m.scanned(slot[i], room[i])]
    seen = dict.fromkeys(mm.DEFECTS, 0)
    for i in rows:
        good = m.scan(slot[i], room[i])
        for defect in mm.DEFECTS:
            bad = m.scan(slot[i], room[i], defect=defect)
            seen[defect] += any(not np.array_equal(g, b) for g, b in zip(good, bad))
        # a tie towards the larger event shows in the summary alone, a clash reported as NO_ROOM in to_room alone
        tie, clash = m.scan(slot[i], room[i], defect="tie_larger_event"), m.scan(slot[i], room[i], defect="clash_as_no_room")
        assert np.array_equal(tie[1], good[1]) and np.array_equal(tie[2], good[2])
        assert np.array_equal(clash[0], good[0]) and not np.array_equal(clash[2], good[2])
    assert seen["clash_as_no_room"] == len(rows) and seen["highest_room"] == len(rows), seen
    assert seen["tie_larger_event"] > 0, seen
    r1 = lm.SHAPES["R1"]()                          # one room: the highest free room is the lowest
    m1 = mm.Model(r1)
    s1, o1 = mm.population(r1, 3, m1)
    assert all(np.array_equal(a, b) for a, b in zip(m1.scan(s1[0], o1[0]), m1.scan(s1[0], o1[0], defect="highest_room")))


# ---------------------------------------------------------------- the boundary
def test_header_symbols_are_exported_listed_and_called():
    check_exports(HEADER, "TTGA_MOVE1_H", "MOVE1_EXPORTS", CONSUMER, {"tt_move1_scan", "tt_move1_descent"})
    text = HEADER.read_text()
    assert '#include "../ttga.h"' in text
    for name, value in (("CLASH", mm.CLASH), ("NO_ROOM", mm.NO_ROOM), ("UNSCANNED", mm.UNSCANNED)):
        assert f"#define TT_MOVE1_{name}" in text and f" {value} " in text.split(f"#define TT_MOVE1_{name}")[1][:12]
        assert getattr(native, f"MOVE1_{name}") == value
    assert "#define TT_MOVE1_NONE 0x7fffffff" in text and native.MOVE1_NONE == mm.NONE == 0x7FFFFFFF
    top = (REPO / "include" / "ttga.h").read_text()
    assert "ttga/move1.h" in top and "bit 10 (1024)" in top
    # the header is in the library's and the native driver's dependencies
    make = (PKG / "Makefile").read_text()
    assert make.count("../include/ttga/move1.h") == 2
    # flat in include/ the prototypes would land in tests/test_gpu_footprint.py's scan of include/*.h
    assert not list((REPO / "include").glob("*move1*"))


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_cxx98_move1_consumer_builds_and_links(tmp_path):
    build_and_run_consumer(CONSUMER, tmp_path)


def test_argument_errors_without_a_device():
    lib = native.load()
    buf = (ctypes.c_int32 * 64)()

    def scan(h, slot, room, P, outs=buf):
        return lib.tt_move1_scan(h, slot, room, P, outs, outs, outs, None)

    def descent(h, slot, room, P, max_passes, outs=buf):
        return lib.tt_move1_descent(h, slot, room, P, max_passes, outs, outs, outs, outs, None)
    # a null handle is named, whatever else is wrong
    for rc in (scan(None, buf, buf, 1), scan(None, None, None, -1), scan(None, buf, buf, 0),
               descent(None, buf, buf, 1, 1), descent(None, None, None, -1, 0), descent(None, buf, buf, 0, 1)):
        assert rc == native.TT_ERR_INVALID
        assert b"null tt_problem" in lib.tt_last_error()
    # with a handle, every argument is checked before any device call: a stand-in
    # handle that the library must not look into
    fake = ctypes.cast((ctypes.c_uint8 * 8)(), ctypes.c_void_p)
    for rc, word in ((lambda: scan(fake, None, buf, 1), b"tt_move1_scan: null population"),
                     (lambda: scan(fake, buf, None, 1), b"tt_move1_scan: null population"),
                     (lambda: scan(fake, buf, buf, -1), b"negative population"),
                     (lambda: descent(fake, None, buf, 1, 1), b"tt_move1_descent: null population"),
                     (lambda: descent(fake, buf, None, 1, 1), b"tt_move1_descent: null population"),
                     (lambda: descent(fake, buf, buf, -1, 1), b"negative population"),
                     (lambda: descent(fake, buf, buf, 1, 0), b"tt_move1_descent: max_passes"),
                     (lambda: descent(fake, buf, buf, 0, -1), b"tt_move1_descent: max_passes")):
        assert rc() == native.TT_ERR_INVALID
        assert word in lib.tt_last_error(), lib.tt_last_error()
    # P = 0: no launch; every output may be NULL
    assert scan(fake, buf, buf, 0) == native.TT_OK and scan(fake, buf, buf, 0, outs=None) == native.TT_OK
    for rc in (scan(fake, None, None, 0), scan(fake, buf, None, 0), descent(fake, None, buf, 0, 1)):   # null: also at P = 0
        assert rc == native.TT_ERR_INVALID and b"null population" in lib.tt_last_error()
    for passes in (1, INT_MAX):
        assert descent(fake, buf, buf, 0, passes) == native.TT_OK
        assert descent(fake, buf, buf, 0, passes, outs=None) == native.TT_OK


# ---------------------------------------------------------------- the flag, Island, the line
MESSAGE = "--move1-descent must be a non-negative integer"
BAD_FLAGS = (["-i", "x.tim", "--move1-descent", "-1"], ["-i", "x.tim", "--move1-descent"],
             ["-i", "x.tim", "--move1-descent", "2.5"], ["-i", "x.tim", "--move1-descent", "many"],
             ["-i", "x.tim", "--move1-descent", ""], ["-i", "x.tim", "--move1-descent", "2147483648"])


def test_flag_in_the_control_parse():
    ctl = parse_control(["-i", "x.tim", "--move1-descent", "64", "-s", "42"], out=Sink(), err=Sink())
    assert ctl["move1_descent"] == 64 and ctl["seed"] == 42 and ctl["input"] == "x.tim"
    assert "move1_descent" not in parse_control(["-i", "x.tim", "-s", "42"], out=Sink(), err=Sink())
    ctl = parse_control(["--move1-descent", "0", "--lahc", "200", "-i", "x.tim", "--unique"], out=Sink(), err=Sink())
    assert ctl["move1_descent"] == 0 and ctl["lahc"] == 200 and ctl["unique"] is True
    assert parse_control(["-i", "x.tim", "--move1-descent", str(INT_MAX)], out=Sink(), err=Sink())["move1_descent"] == INT_MAX
    for bad in BAD_FLAGS:
        rejected_by_parse_control(bad, MESSAGE, exact=True)


def test_flag_in_the_native_driver():
    for bad in BAD_FLAGS:
        rejected_by_native_driver(bad, MESSAGE, exact=True)
    stripped_before_pair_count(["--move1-descent", "4"])
    stripped_before_pair_count(["--lahc", "4", "--move1-descent", "4", "--slot-swap", "1"])


def test_flag_is_in_the_table_for_the_tools():
    import argparse
    f = stages.FLAGS[-1]                                            # appended: the older flags keep their places
    assert (f.flag, f.key, f.kind, f.arg, f.message) == ("--move1-descent", "move1_descent", "int", (0, INT_MAX), MESSAGE)
    assert stages.KEYS[-1] == "move1_descent" and stages.KEYS.count("move1_descent") == 1
    ap = argparse.ArgumentParser()
    stages.add_arguments(ap)
    assert stages.island_kwargs(ap.parse_args([]))["move1_descent"] == 0
    assert stages.island_kwargs(ap.parse_args(["--move1-descent", "64"]))["move1_descent"] == 64
    for tool in ("bench_ga.py", "ga_quality.py"):
        assert "stages.add_arguments" in (REPO / "tools" / tool).read_text()


def test_validate_and_island_check_before_any_device_call():
    import inspect
    base = ("random", 0.0, 0, 0, 0, 500, 0.5, "uniform", False)
    stages.validate(*base)                                          # as before: the keyword has a default
    stages.validate(*base, 0.0, 0, "direct", 1, 0)
    stages.validate(*base, move1_descent=INT_MAX)
    assert list(inspect.signature(stages.validate).parameters)[-1] == "move1_descent"
    assert list(inspect.signature(Island.__init__).parameters)[-1] == "move1_descent"
    assert inspect.signature(Island.__init__).parameters["move1_descent"].default == 0
    with pytest.raises(ValueError, match=r"move1_descent must be >= 0 \(0: off\)"):
        stages.validate(*base, move1_descent=-1)

    class NoDevice:                      # any use of it would raise AttributeError
        pass
    with pytest.raises(ValueError, match=r"move1_descent must be >= 0 \(0: off\)"):
        Island(NoDevice(), move1_descent=-1)


def test_move1_descent_line():
    line = move1_descent_line({"rows": 30, "improved": 8, "meanPasses": 2.5, "gain": 41})
    assert line == '{"move1Descent":{"gain":41,"improved":8,"meanPasses":2.5,"rows":30}}'
    none = move1_descent_line({"rows": 3, "improved": 0, "meanPasses": 0.0, "gain": 0})
    assert '"meanPasses":0,' in none                                # jsoncpp's %.17g, as the other lines


def test_tool_leaves_out_what_the_validator_would_flag():
    """python -m ttga.move1's reading of a driver's output: timetables of another
    length, genes out of range (256 would wrap to 0 as a uint8) and rows with
    hcv != 0 are left out and counted, with a word each."""
    from ttga.move1 import solutions
    inst = lm.SHAPES["E65"]()
    m = mm.Model(inst)
    slot, room = lm.feasible_rows(inst, 4, 3, m)
    i = next(i for i in range(4) if m.scanned(slot[i], room[i]))
    t, r = slot[i].tolist(), room[i].tolist()

    def line(ts, rs, proc):
        import json
        return json.dumps({"solution": {"procID": proc, "feasible": True, "totalBest": 1, "timeslots": ts, "rooms": rs}})
    clash = list(t)
    clash[1], twin = t[0], list(r)
    twin[1] = r[0]
    text = "\n".join(["not json", line(t, r, 0), line(t[:-1], r[:-1], 1), line([256] + t[1:], r, 2), line(t, [inst.R] + r[1:], 3),
                      line(clash, twin, 4), '{"solution":{"procID":5,"feasible":false,"totalBest":3000012}}',
                      '{"runEntry":{"procsNum":1}}'])
    err = Sink()
    found, left_out = solutions(inst, text, err)
    assert [(f[0], f[1], f[2]) for f in found] == [(0, t, r)] and left_out == 4
    said = err.text.splitlines()
    assert len(said) == 4 and [int(s.split()[3]) for s in said] == [1, 2, 3, 4] and "hcv" in said[3]
