"""CPU checks of the conflict-guided crossover (no GPU): the model
(tests/cx_model.py) pinned to the oracle's ga_breed where the two must agree,
the rule by replay, the children's quality against the uniform crossover on
the recipe the feature was measured with, the boundary of include/ttga_cx.h as
a C++98 consumer sees it, the argument handling before any device call, the
--crossover flags in both drivers' parse, Island's argument checks and the
crossover line."""
import ctypes
import pathlib
import shutil

import numpy as np
import pytest

import ttga
import cx_model as cm
import greedy_model as gm
from oracle_lib import oracle
from stage_checks import (Sink, build_and_run_consumer, check_exports, rejected_by_native_driver,
                          rejected_by_parse_control, stripped_before_pair_count)
from ttga import native
from ttga.ga import Island, crossover_line
from ttga.islands import parse_control

REPO = pathlib.Path(__file__).resolve().parent.parent
HEADER = REPO / "include" / "ttga_cx.h"
CONSUMER = REPO / "tests" / "boundary_cx_cxx98.cpp"


# ---------------------------------------------------------------- the model pinned to the oracle
def random_population(o, N, base):
    s, r, _ = o.random_init(ttga.population_seeds(base, N))
    return s, r, o.eval(s, r)[3]


@pytest.mark.parametrize("p_mut", [0.0, 1.0])
@pytest.mark.parametrize("skip", [0, 1])
def test_breed_without_crossover_is_the_oracles(p_mut, skip):
    inst = ttga.config_instance("sm")
    o = oracle().problem(inst)
    s, r, pen = random_population(o, 48, 700)
    pen[5] = -1                                              # an invalid genome never wins a tournament
    seeds = ttga.population_seeds(9100, 20)
    want = o.ga_breed(s, r, pen, seeds, 20, 0.0, p_mut, skip)
    got = cm.breed(inst, o, gm.greedy_order(inst), s, r, pen, seeds, 0.0, p_mut, skip, repair=1)
    for a, b, what in zip(got[:4], want, ("slot", "room", "flags", "rng")):
        assert np.array_equal(a, b), what
    assert (got[4] == 0).all() and (got[5] == 0).all()
    assert ((got[2] & cm.FLAG_MUTATE) != 0).all() == (p_mut == 1.0) and not (got[2] & cm.FLAG_CROSS).any()


@pytest.mark.parametrize("repair", [0, 1])
def test_breed_on_a_cost_free_instance_is_the_oracles(repair):
    """No students, so no correlations; 40 events against 64 rooms, so no slot
    is ever full: every cost is 0 and the guided crossover in event order is
    the uniform one, draw for draw."""
    inst = ttga.generate(40, 64, 2, 0)
    assert not inst.correlations().any()
    o = oracle().problem(inst)
    s, r, pen = random_population(o, 48, 800)
    seeds = ttga.population_seeds(9200, 20)
    order = np.arange(inst.E, dtype=np.int32)
    for p_mut in (0.0, 0.5):
        want = o.ga_breed(s, r, pen, seeds, 20, 1.0, p_mut, 1)
        got = cm.breed(inst, o, order, s, r, pen, seeds, 1.0, p_mut, 1, repair)
        for a, b, what in zip(got[:4], want, ("slot", "room", "flags", "rng")):
            assert np.array_equal(a, b), (what, p_mut)
        assert (got[4] == 0).all() and (got[5] == 0).all() and (got[2] & cm.FLAG_CROSS).all()


# ---------------------------------------------------------------- the rule
@pytest.fixture(scope="module")
def sm_parents():
    inst = ttga.config_instance("sm")
    order = gm.greedy_order(inst)
    rows, _ = gm.greedy_slots(inst, order, ttga.population_seeds(100, 32))
    return inst, order, rows


@pytest.mark.parametrize("repair", [0, 1])
@pytest.mark.parametrize("parents", ["random", "greedy"])
def test_model_rows_obey_the_rule(sm_parents, parents, repair):
    inst, order, greedy = sm_parents
    P = 6
    if parents == "random":
        A, _ = ttga.rng.random_slots(ttga.population_seeds(11, P), inst.E)
        B, _ = ttga.rng.random_slots(ttga.population_seeds(31, P), inst.E)
    else:
        A, B = greedy[:P], greedy[P:2 * P]
    seeds = np.array([1, 2147483646, 0, 3000000019, 1000, 1001], np.int64)
    stats = {}
    slot, state, cost, rep = cm.guided_slots(inst, order, A, B, seeds, repair, stats)
    assert np.array_equal(state, [gm.advanced(x, inst.E) for x in seeds])        # exactly E draws
    for i in range(P):
        cm.replay_check(inst, order, A[i], B[i], slot[i], repair, cost[i], rep[i])
    if not repair:
        assert ((slot == A) | (slot == B)).all() and (rep == 0).all()
    else:
        assert slot.max() < 45
    assert stats.get("coin", 0) > 0 and stats.get("cost", 0) > 0
    assert (stats.get("fallback", 0) > 0) == bool(repair)


def test_replay_check_rejects_a_wrong_row(sm_parents):
    inst, order, greedy = sm_parents
    A, B = greedy[0], greedy[1]
    slot, _, cost, rep = cm.guided_slots(inst, order, A[None], B[None], [5], 0)
    e = int(np.flatnonzero(A != B)[0])
    bad = slot[0].copy()
    bad[e] = next(t for t in range(45) if t not in (A[e], B[e]))          # neither parent's slot
    with pytest.raises(AssertionError):
        cm.replay_check(inst, order, A, B, bad, 0, cost[0], rep[0])
    with pytest.raises(AssertionError):
        cm.replay_check(inst, order, A, B, slot[0], 0, cost[0] + 1, rep[0])


def test_genes_of_45_and_more():
    """One side only: the other parent's gene; both sides: kept with cost -1
    without repair, repaired with it."""
    inst = ttga.generate(30, 3, 2, 20, seed=3)
    order = gm.greedy_order(inst)
    A, _ = ttga.rng.random_slots([7], inst.E)
    B, _ = ttga.rng.random_slots([8], inst.E)
    A[0, 4], B[0, 9] = 45, 255
    A[0, 12], B[0, 12] = 200, 45
    slot, _, cost, rep = cm.guided_slots(inst, order, A, B, [3], 0)
    assert slot[0, 4] == B[0, 4] and slot[0, 9] == A[0, 9] and slot[0, 12] in (200, 45) and cost[0] == -1
    slot, _, cost, rep = cm.guided_slots(inst, order, A, B, [3], 1)
    assert slot.max() < 45 and cost[0] >= 0 and rep[0] >= 1


# ---------------------------------------------------------------- quality against uniform
def test_guided_children_clash_less_than_uniform(sm_parents):
    """32 greedy rows of sm, none with two correlated events in one timeslot;
    40 random pairs crossed. Correlated pairs sharing a slot, mean over the 40
    children: measured 13.2 guided against 35.6 uniform, and 0 in all 40 with
    the repair."""
    inst, order, rows = sm_parents
    assert (cm.shared_pairs(inst, rows) == 0).all()
    g = np.random.default_rng(1)
    pairs = np.array([g.choice(32, 2, replace=False) for _ in range(40)])
    seeds = np.arange(500, 540, dtype=np.int64)
    A, B = rows[pairs[:, 0]], rows[pairs[:, 1]]
    uniform = oracle().problem(inst).crossover(A, B, seeds)[0]
    guided = cm.guided_slots(inst, order, A, B, seeds, 0)[0]
    repaired, _, cost, rep = cm.guided_slots(inst, order, A, B, seeds, 1)
    u, gd, rp = (cm.shared_pairs(inst, x) for x in (uniform, guided, repaired))
    print("uniform", u.mean(), "guided", gd.mean(), "repaired: clean", int((rp == 0).sum()), "of 40, mean fallback",
          rep.mean(), "share of genes from a parent", ((repaired == A) | (repaired == B)).mean())
    assert gd.mean() <= 0.5 * u.mean()
    assert (rp == 0).sum() >= 36                                # >= 90 % of the 40
    assert ((cost == 0) == (rp == 0)).all()                     # cost 0 means no clash (R = 5 here never fills)


# ---------------------------------------------------------------- the boundary
def test_header_symbols_are_exported_listed_and_called():
    check_exports(HEADER, "TTGA_CX_H", "CX_EXPORTS", CONSUMER, {"tt_crossover_guided", "tt_ga_breed_guided"})
    text = HEADER.read_text()
    assert '#include "ttga.h"' in text and "no counterpart in the reference" in text and "ga.cpp:562-566" in text
    top = (REPO / "include" / "ttga.h").read_text()
    assert "ttga_cx.h" in top and "bit 9 (512)" in top


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_cxx98_cx_consumer_builds_and_links(tmp_path):
    build_and_run_consumer(CONSUMER, tmp_path)


def test_argument_errors_without_a_device():
    lib = native.load()
    buf = (ctypes.c_int32 * 64)()
    dbl = ctypes.c_double

    def cross(h, s1, s2, order, rng, slot, room, P, outs=buf):
        return lib.tt_crossover_guided(h, s1, s2, order, rng, slot, room, P, 1, outs, outs, None)

    def breed(h, ps, pr, pen, N, order, rng, C, cs, cr, fl, outs=buf):
        return lib.tt_ga_breed_guided(h, ps, pr, pen, N, order, rng, C, dbl(0.8), dbl(0.5), 1, 1, cs, cr, fl, outs, outs,
                                      None)
    # a null handle is named, whatever else is wrong
    for args in ((None, buf, buf, buf, buf, buf, buf, 1), (None, None, None, None, None, None, None, -1),
                 (None, buf, buf, buf, buf, buf, buf, 0)):
        assert cross(*args) == native.TT_ERR_INVALID
        assert b"null tt_problem" in lib.tt_last_error()
    for args in ((None, buf, buf, buf, 4, buf, buf, 1, buf, buf, buf), (None, None, None, None, 0, None, None, -1, None,
                                                                       None, None)):
        assert breed(*args) == native.TT_ERR_INVALID
        assert b"null tt_problem" in lib.tt_last_error()
    # with a handle, every argument is checked before any device call: a stand-in
    # handle that the library must not look into
    fake = ctypes.cast((ctypes.c_uint8 * 8)(), ctypes.c_void_p)
    good = [fake, buf, buf, buf, buf, buf, buf, 1]
    for k, word in ((1, b"null population"), (2, b"null population"), (3, b"order"), (4, b"rng"),
                    (5, b"null population"), (6, b"null population")):
        args = list(good)
        args[k] = None
        assert cross(*args) == native.TT_ERR_INVALID, k
        assert word in lib.tt_last_error(), (k, lib.tt_last_error())
    assert cross(fake, buf, buf, buf, buf, buf, buf, -1) == native.TT_ERR_INVALID
    assert b"negative population" in lib.tt_last_error()
    assert cross(fake, buf, buf, buf, buf, buf, buf, 0) == native.TT_OK          # P = 0: no launch
    assert cross(fake, buf, buf, buf, buf, buf, buf, 0, outs=None) == native.TT_OK
    good = [fake, buf, buf, buf, 4, buf, buf, 1, buf, buf, buf]
    for k in (1, 2, 3, 5, 6, 8, 9, 10):
        args = list(good)
        args[k] = None
        assert breed(*args) == native.TT_ERR_INVALID, k
        assert (b"order" if k == 5 else b"population") in lib.tt_last_error(), (k, lib.tt_last_error())
    for N, C in ((0, 1), (4, -1)):
        args = list(good)
        args[4], args[7] = N, C
        assert breed(*args) == native.TT_ERR_INVALID, (N, C)
    args = list(good)
    args[7] = 0
    assert breed(*args) == native.TT_OK                                          # C = 0: no launch
    assert breed(*args, outs=None) == native.TT_OK


# ---------------------------------------------------------------- the flags, Island, the line
BAD_FLAGS = ((["-i", "x.tim", "--crossover", "best"], "--crossover must be uniform or guided"),
             (["-i", "x.tim", "--crossover"], "--crossover must be uniform or guided"),
             (["-i", "x.tim", "--crossover", "Guided"], "--crossover must be uniform or guided"),
             (["-i", "x.tim", "--crossover-repair"], "--crossover-repair needs --crossover guided"),
             (["-i", "x.tim", "--crossover-repair", "--crossover", "uniform"],
              "--crossover-repair needs --crossover guided"))


def test_crossover_flags_in_the_control_parse():
    ctl = parse_control(["-i", "x.tim", "--crossover", "guided", "-s", "42"], out=Sink(), err=Sink())
    assert ctl["crossover"] == "guided" and "crossover_repair" not in ctl and ctl["seed"] == 42
    ctl = parse_control(["--crossover-repair", "-i", "x.tim", "--crossover", "guided", "--lahc", "10"], out=Sink(),
                        err=Sink())
    assert ctl["crossover"] == "guided" and ctl["crossover_repair"] is True and ctl["lahc"] == 10
    ctl = parse_control(["-i", "x.tim", "--crossover", "uniform"], out=Sink(), err=Sink())
    assert ctl["crossover"] == "uniform"
    assert "crossover" not in parse_control(["-i", "x.tim", "-s", "42"], out=Sink(), err=Sink())
    for bad, msg in BAD_FLAGS:
        rejected_by_parse_control(bad, msg, exact=True)


def test_crossover_flags_in_the_native_driver():
    for bad, msg in BAD_FLAGS:
        rejected_by_native_driver(bad, msg, exact=True)
    stripped_before_pair_count(["--crossover", "guided", "--crossover-repair"])


def test_island_checks_its_crossover_arguments_before_any_device_call():
    class NoDevice:                      # any use of it would raise AttributeError
        pass
    for bad in ("best", "", None, "Guided"):
        with pytest.raises(ValueError, match="crossover must be 'uniform' or 'guided'"):
            Island(NoDevice(), crossover=bad)
    with pytest.raises(ValueError, match="crossover_repair needs crossover='guided'"):
        Island(NoDevice(), crossover_repair=True)
    with pytest.raises(ValueError, match="crossover_repair needs crossover='guided'"):
        Island(NoDevice(), crossover="uniform", crossover_repair=True)


def test_crossover_line():
    line = crossover_line({"children": 80, "crossed": 64, "clean": 40, "cost": 96, "repaired": 17})
    assert line == '{"crossover":{"children":80,"clean":40,"crossed":64,"meanCost":1.5,"repaired":17}}'
    line = crossover_line({"children": 3, "crossed": 0, "clean": 0, "cost": 0, "repaired": 0})
    assert line == '{"crossover":{"children":3,"clean":0,"crossed":0,"meanCost":0,"repaired":0}}'
