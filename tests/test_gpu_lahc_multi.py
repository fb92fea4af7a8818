"""tt_lahc_multi (include/ttga_lahc_multi.h) on the GPU. Against
tests/lahc_multi_model.py: slot, room, the rng state, gain, accepted,
best_step, the seven Kempe counts, winner and walker_gain bit for bit, feasible
and spoiled rows mixed in one launch, and around every call tt_eval: hcv
unchanged, scv lower by exactly the gain, the scv / penalty updated in place
equal to a fresh evaluation. Against the library itself: K stream-chained calls
of tt_lahc_kempe_aug on copies of the rows, the winner picked by torch. Then one
walker against tt_lahc_kempe_aug, tt_lahc_kempe and tt_lahc, the edges, invalid
genes and arguments, the limits, two streams, Island(lahc_walkers=K) and the two
drivers with --lahc-walkers."""
import pathlib
import sys

import numpy as np
import pytest

import ttga
import lahc_model as lm
import lahc_multi_model as mm
import walk_checks as wc
from helpers import dev, host, json_lines
from stage_checks import GA, both_drivers, run_driver, run_island, stage_lines
from walk_checks import BAD_GENE, FILL, NAMES, same

pytestmark = pytest.mark.gpu

import torch  # noqa: E402
from ttga import native  # noqa: E402

REPO = pathlib.Path(__file__).resolve().parent.parent
SEEN = {"later": 0, "idle": 0, "cases": 0}      # over test_rows_vs_model's cases


@pytest.fixture(scope="module")
def problems():
    cache = {}

    def get(name):
        if name not in cache:
            inst = lm.SHAPES[name]()
            cache[name] = (inst, native.DeviceProblem(inst), mm.Model(inst))
        return cache[name]
    return get


def outputs(P, K):
    """gain, accepted, best_step [P], kempe_stats [P, 7], winner [P], walker_gain [P, K], sentinel-filled."""
    return [wc.filled(P), wc.filled(P), wc.filled(P), wc.filled(P, 7), wc.filled(P), wc.filled(P, K)]


def call(dp, a):
    """tt_lahc_multi for walk_checks.run; work "own": a tensor of the documented size, None: the binding's."""
    def launch(s, r, g, **out):
        work = a.get("work", "own")
        if isinstance(work, str):
            work = torch.empty(dp.lahc_multi_work_bytes(s.shape[0], a["K"]), dtype=torch.uint8, device="cuda")
        dp.lahc_multi(s, r, g, a["K"], a["steps"], a["history"], a["p_swap"], a["p_kempe"], a.get("max_chain", 0),
                      a.get("room_rule", 1), work=work, **out)
    return launch


def rows(model, slot, room, seeds, a):
    return model.lahc_multi_rows(slot, room, seeds, a["K"], a["steps"], a["history"], a["p_swap"], a["p_kempe"])


def run(dp, slot, room, seeds, K, steps, L, p_swap, p_kempe, cap=0, rule=1, with_eval=True, work="own"):
    """One call on numpy rows; returns the outputs and the evaluations around it."""
    a = dict(K=K, steps=steps, history=L, p_swap=p_swap, p_kempe=p_kempe, max_chain=cap, room_rule=rule, work=work)
    return wc.run(dp, call(dp, a), slot, room, seeds, 7, with_eval, winner=(), walker_gain=(K,))


def around(got, want, before, after, inplace, slot, room, seeds, steps):
    """walk_checks.check_rows, and the winner: the lowest walker of the largest gain."""
    closed = wc.check_rows(got, want, before, after, inplace, slot, room, seeds, steps)
    K = got[8].shape[1]
    assert (got[7] >= 0).all() and (got[7] < K).all()
    assert np.array_equal(got[3], got[8].max(axis=1)) and np.array_equal(got[7], got[8].argmax(axis=1))
    return closed


# ---------------------------------------------------------------- against the model
@pytest.mark.parametrize("cid", list(mm.CASES))
def test_rows_vs_model(problems, cid):
    shape, P, K, steps, L, p_swap, p_kempe, rule = mm.CASES[cid]
    inst, dp, model = problems(shape)
    slot, room, seeds = mm.case_rows(cid, inst, model)
    want = model.lahc_multi_rows(slot, room, seeds, K, steps, L, p_swap, p_kempe, 0, rule)
    got, before, after, inplace = run(dp, slot, room, seeds, K, steps, L, p_swap, p_kempe, 0, rule)
    closed = around(got, want, before, after, inplace, slot, room, seeds, steps)
    print(cid, "walked", int((~closed).sum()), "of", P, "winner", got[7].tolist(), "gain", got[3].tolist(),
          "walker 0", got[8][:, 0].tolist())
    SEEN["cases"] += 1
    SEEN["later"] += int((got[7] > 0).sum())
    SEEN["idle"] += int((~closed & (got[7] == 0) & (got[3] == 0)).sum())
    if shape in lm.NO_FEASIBLE_ROW:
        assert closed.all()
        return
    # both kinds of rows in the launch (population spoils rows 2, 7, ...: none among syn_sparse's two)
    assert (~closed).any() and (closed.any() or inst.E < 2 or P <= 2)
    i = wc.check_stream_advance(got, seeds, closed, 3 * steps * K)   # exactly 3 * steps * K draws a searched row
    if cid == "sm":
        assert i == 0 and seeds[0] == 2 ** 40 + 7 and got[3][0] > 0  # the state out of range walks, and is row 0
    if cid == "sm-plain":
        assert not got[6].any()                                      # no chains: tt_lahc's walk
    if cid in ("sm", "E65", "med", "R64"):
        assert got[6][:, 0].sum() > 0 and (got[7] > 0).any()
    assert dp.status() & BAD_GENE == 0


def test_the_cases_show_a_later_winner_and_an_idle_walk():
    """Runs behind test_rows_vs_model: over its cases some row is won by a
    walker other than 0, and some walked row has winner 0 with gain 0."""
    assert SEEN["cases"] == len(mm.CASES), "run the whole module: this test sums up test_rows_vs_model"
    assert SEEN["later"] > 0 and SEEN["idle"] > 0


# ---------------------------------------------------------------- against the library itself
@pytest.fixture(scope="module")
def med_rows(problems):
    """33 rows of med, feasible and spoiled, computed once and never written."""
    inst, dp, model = problems("med")
    slot, room, seeds = lm.population(inst, 33, model)
    seeds[1] = mm.WIDE_SEED
    for a in (slot, room, seeds):
        a.setflags(write=False)
    return slot, room, seeds


def chained(dp, slot, room, seeds, K, steps, L, p_swap, p_kempe, rule):
    """K calls of tt_lahc_kempe_aug on copies of the rows, the stream running on
    from one to the next; torch picks the winner (the lowest index of the
    largest gain) and lowers scv and penalty under tt_lahc's rule."""
    P = slot.shape[0]
    s0, r0, g = dev(slot), dev(room), dev(seeds)
    hcv, scv, feas, pen = dp.eval(s0, r0)
    rows_s = torch.empty((K, P, slot.shape[1]), dtype=torch.uint8, device="cuda")
    rows_r = torch.empty_like(rows_s)
    nums = torch.full((K, 3, P), FILL, dtype=torch.int32, device="cuda")
    stats = torch.full((K, P, 7), FILL, dtype=torch.int32, device="cuda")
    for w in range(K):
        rows_s[w].copy_(s0)
        rows_r[w].copy_(r0)
        dp.lahc_kempe_aug(rows_s[w], rows_r[w], g, steps, L, p_swap, p_kempe, 0, rule, gain=nums[w, 0],
                          accepted=nums[w, 1], best_step=nums[w, 2], kempe_stats=stats[w])
    gains = nums[:, 0, :]                                            # [K, P]
    top = gains.max(dim=0).values
    index = torch.arange(K, device="cuda")[:, None].expand(K, P)
    winner = torch.where(gains == top[None, :], index, K).min(dim=0).values
    rows = torch.arange(P, device="cuda")
    pen = torch.where((pen >= 0) & (pen < 1000000), pen - top, pen)
    want = (rows_s[winner, rows], rows_r[winner, rows], g, top, nums[winner, 1, rows], nums[winner, 2, rows],
            stats[winner, rows], winner.to(torch.int32), gains.t().contiguous())
    return [host(t) for t in want], host(scv - top), host(pen), host(hcv)


@pytest.mark.parametrize("P, K", [(33, 64), (1, 1024), (513, 2)])
def test_equals_chained_calls_of_the_walk(problems, med_rows, P, K):
    inst, dp, _ = problems("med")
    steps, L, p_swap, p_kempe, rule = 500, 500, 0.25, 0.5, 1
    take = np.arange(P) % 33                                         # the 33 rows over again, each with its own stream
    slot, room = med_rows[0][take], med_rows[1][take]
    seeds = med_rows[2][take] + 104729 * (np.arange(P) // 33)
    want, scv_want, pen_want, hcv0 = chained(dp, slot, room, seeds, K, steps, L, p_swap, p_kempe, rule)
    got, before, after, inplace = run(dp, slot, room, seeds, K, steps, L, p_swap, p_kempe, 0, rule)
    closed = around(got, want, before, after, inplace, slot, room, seeds, steps)
    assert np.array_equal(inplace[0], scv_want) and np.array_equal(inplace[1], pen_want)
    assert np.array_equal(closed, hcv0 != 0) and not closed[0] and got[3][0] > 0
    print(P, K, "later winners", int((got[7] > 0).sum()), "gain", int(got[3].sum()), "walker 0", int(got[8][:, 0].sum()))
    if K > 2:
        assert (got[7] > 0).any() and got[7].max() >= 2
    if P > 1:
        assert closed.any() and seeds[1] == mm.WIDE_SEED and got[3][1] > 0


# ---------------------------------------------------------------- one walker
def single(dp, slot, room, seeds, call):
    """An older entry point on the same rows, through `call(s, r, g, scv, pen, gain, accepted, best_step)`."""
    s, r, g = dev(slot), dev(room), dev(seeds)
    before = [host(t) for t in dp.eval(s, r)]
    scv, pen = dev(before[1]), dev(before[3])
    out = [torch.full((slot.shape[0],), FILL, dtype=torch.int32, device="cuda") for _ in range(3)]
    call(s, r, g, scv, pen, *out)
    return [host(t) for t in (s, r, g, *out, scv, pen)]


@pytest.mark.parametrize("older", ["tt_lahc_kempe_aug", "tt_lahc_kempe", "tt_lahc"])
def test_one_walker_is_the_older_call(problems, older):
    inst, dp, model = problems("sm")
    slot, room, seeds = lm.population(inst, 33, model)
    steps, L = 500, 50
    width = {"tt_lahc_kempe_aug": 7, "tt_lahc_kempe": 5, "tt_lahc": 0}[older]
    p_swap, p_kempe, rule = {"tt_lahc_kempe_aug": (0.25, 0.5, 1), "tt_lahc_kempe": (0.25, 0.5, 0),
                             "tt_lahc": (0.5, 0.0, 0)}[older]
    stats = torch.full((33, max(width, 1)), FILL, dtype=torch.int32, device="cuda")

    def call(s, r, g, scv, pen, gain, accepted, best_step):
        kw = dict(scv=scv, penalty=pen, gain=gain, accepted=accepted, best_step=best_step)
        if older == "tt_lahc_kempe_aug":
            dp.lahc_kempe_aug(s, r, g, steps, L, p_swap, p_kempe, 0, rule, kempe_stats=stats, **kw)
        elif older == "tt_lahc_kempe":
            dp.lahc_kempe(s, r, g, steps, L, p_swap, p_kempe, 0, kempe_stats=stats, **kw)
        else:
            dp.lahc(s, r, g, steps, L, p_swap, **kw)
    want = single(dp, slot, room, seeds, call)
    got, before, after, inplace = run(dp, slot, room, seeds, 1, steps, L, p_swap, p_kempe, 0, rule, work=None)
    for name, g, w in zip(NAMES[:6], got, want):
        assert np.array_equal(g, w), name
    assert np.array_equal(inplace[0], want[6]) and np.array_equal(inplace[1], want[7])       # scv and penalty in place
    assert np.array_equal(got[6][:, :width], host(stats)[:, :width]) and not got[6][:, width:].any()
    assert not got[7].any() and np.array_equal(got[8][:, 0], got[3]) and got[3].sum() > 0
    around(got, None, before, after, inplace, slot, room, seeds, steps)


# ---------------------------------------------------------------- edges
@pytest.mark.parametrize("steps", [0, 1])
def test_steps_0_and_1(problems, steps):
    inst, dp, model = problems("sm")
    slot, room, seeds = lm.population(inst, 9, model)
    want = model.lahc_multi_rows(slot, room, seeds, 4, steps, 50, 0.25, 0.5)
    got, before, after, inplace = run(dp, slot, room, seeds, 4, steps, 50, 0.25, 0.5)
    closed = around(got, want, before, after, inplace, slot, room, seeds, steps)
    if steps == 0:                                                   # changes nothing
        assert np.array_equal(got[0], slot) and np.array_equal(got[1], room) and np.array_equal(got[2], seeds)
        assert not any(got[k].any() for k in range(3, 9))
    else:
        assert (got[2][~closed] != seeds[~closed]).all() and (got[5] <= 1).all()


def test_invalid_genes():
    """walk_checks.invalid_genes; row 2 is spoiled: closed too, no status bit for it."""
    a = dict(K=3, steps=300, history=50, p_swap=0.25, p_kempe=0.5)
    wc.invalid_genes(mm.Model, call, rows, a, 7, closed=(1, 2, 4), winner=(), walker_gain=(3,))


def test_all_rows_closed_and_no_status_bit_for_hcv():
    inst = lm.SHAPES["sm"]()
    dp, model = native.DeviceProblem(inst), mm.Model(inst)
    slot, room, seeds = lm.population(inst, 5, model)
    slot[:, 1], room[:, 1] = slot[:, 0], room[:, 0]                  # every row spoiled: hcv != 0
    got, before, after, inplace = run(dp, slot, room, seeds, 4, 200, 50, 0.25, 0.5)
    assert np.array_equal(got[0], slot) and np.array_equal(got[1], room) and np.array_equal(got[2], seeds)
    assert not any(got[k].any() for k in range(3, 9)) and (before[0] != 0).all()
    assert np.array_equal(inplace[0], before[1]) and np.array_equal(inplace[1], before[3])
    assert dp.status() == 0
    dp.close()


def test_null_optional_outputs(problems):
    inst, dp, model = problems("sm")
    slot, room, seeds = lm.population(inst, 9, model)
    want = model.lahc_multi_rows(slot, room, seeds, 3, 200, 20, 0.25, 0.5)
    s, r, g = dev(slot), dev(room), dev(seeds)
    dp.lahc_multi(s, r, g, 3, 200, 20, 0.25, 0.5)                    # every output NULL, the work buffer the binding's
    assert np.array_equal(host(s), want[0]) and np.array_equal(host(r), want[1]) and np.array_equal(host(g), want[2])
    s, r, g = dev(slot), dev(room), dev(seeds)
    wg = torch.full((9, 1), FILL, dtype=torch.int32, device="cuda")
    dp.lahc_multi(s, r, g, 1, 200, 20, 0.25, 0.5, walker_gain=wg)    # one walker: walker_gain without gain
    one = model.lahc_multi_rows(slot, room, seeds, 1, 200, 20, 0.25, 0.5)
    assert np.array_equal(host(s), one[0]) and np.array_equal(host(wg), one[8]) and np.array_equal(host(g), one[2])
    win = torch.full((9,), FILL, dtype=torch.int32, device="cuda")
    s, r, g = dev(slot), dev(room), dev(seeds)
    dp.lahc_multi(s, r, g, 1, 200, 20, 0.25, 0.5, winner=win)
    assert not host(win).any() and np.array_equal(host(s), one[0])


def untouched(dp, slot, room, seeds, code, match, K=4, P=None, work="own", **kw):
    """A refused call: the error code, and every buffer as it was."""
    P = slot.shape[0] if P is None else P
    a = {**dict(steps=10, history=5, p_swap=0.25, p_kempe=0.5, max_chain=0, room_rule=1), **kw}
    s, r, g = dev(slot), dev(room), dev(seeds)
    scv = torch.full((slot.shape[0],), FILL, dtype=torch.int32, device="cuda")
    pen = torch.full_like(scv, FILL)
    out = outputs(slot.shape[0], max(min(K, 1024), 1))
    if work == "own":
        work = torch.full((max(dp.lahc_multi_work_bytes(slot.shape[0], max(min(K, 1024), 1)), 8),), 0x5A,
                          dtype=torch.uint8, device="cuda")
    ptr = lambda t: None if t is None else t.data_ptr()      # noqa: E731
    rc = dp.lib.tt_lahc_multi(dp.handle, s.data_ptr(), r.data_ptr(), g.data_ptr(), P, K, a["steps"], a["history"],
                              a["p_swap"], a["p_kempe"], a["max_chain"], a["room_rule"], scv.data_ptr(), pen.data_ptr(),
                              out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), out[3].data_ptr(),
                              out[4].data_ptr(), out[5].data_ptr(), ptr(work), None)
    assert rc == code, (kw, K, rc)
    assert match in dp.lib.tt_last_error().decode(), (kw, K, dp.lib.tt_last_error())
    assert np.array_equal(host(s), slot) and np.array_equal(host(r), room) and np.array_equal(host(g), seeds)
    assert all((host(t) == FILL).all() for t in out + [scv, pen])
    assert work is None or (host(work) == 0x5A).all()


def test_invalid_arguments_launch_nothing(problems):
    inst, dp, model = problems("sm")
    slot, room, seeds = lm.population(inst, 4, model)
    for kw in (dict(room_rule=-1), dict(room_rule=2), dict(steps=-1), dict(history=0), dict(history=-3),
               dict(p_swap=1.5, p_kempe=0.0), dict(p_swap=-0.1), dict(p_swap=float("nan")),
               dict(p_kempe=1.5, p_swap=0.0), dict(p_kempe=-0.1), dict(p_kempe=float("nan")), dict(max_chain=-1),
               dict(p_swap=0.75, p_kempe=0.5), dict(p_swap=0.25, p_kempe=1.0), dict(P=-1)):
        untouched(dp, slot, room, seeds, native.TT_ERR_INVALID, "", **kw)
    for K in (0, -1, 1025, 2 ** 20):
        untouched(dp, slot, room, seeds, native.TT_ERR_INVALID, "walkers", K=K)
    untouched(dp, slot, room, seeds, native.TT_ERR_INVALID, "work", K=2, work=None)
    untouched(dp, slot, room, seeds, native.TT_ERR_INVALID, "work", K=1024, work=None)
    with pytest.raises(ValueError, match="work must be"):            # the binding: a work tensor too small
        dp.lahc_multi(dev(slot), dev(room), dev(seeds), 4, 10, 5, work=torch.empty(64, dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError, match="walker_gain must be"):
        dp.lahc_multi(dev(slot), dev(room), dev(seeds), 4, 10, 5,
                      walker_gain=torch.empty((4, 3), dtype=torch.int32, device="cuda"))
    assert dp.lahc_multi_work_bytes(4, 4) == 8 * 4 + (48 + 2 * inst.E) * 16
    for P, K in ((4, 0), (4, 1025), (-1, 4), (2 ** 31 - 1, 2), (2 ** 22, 1024)):
        assert dp.lahc_multi_work_bytes(P, K) == 0
    assert dp.lahc_multi_work_bytes(0, 4) == 0 and dp.lahc_multi_work_bytes(2 ** 21, 1023) > 0


def test_limits(problems):
    """A history too long for the LDS, for every set of arguments, and P *
    walkers past 2^31 - 1: TT_ERR_LIMIT, every buffer untouched. The header's
    formula for sm (E 100, S 80) without the history:
    8 * (47 * 2 + 45 + 80) + 4 * 100 + 1,552 = 3,704 bytes."""
    inst, dp, model = problems("sm")
    slot, room, seeds = lm.population(inst, 4, model)
    assert 8 * (47 * 2 + 45 + 80) + 4 * 100 + 1552 == 3704
    fits = (65536 - 3704) // 4
    for K, kw in ((4, {}), (1, {}), (4, dict(p_kempe=0.0, p_swap=0.5, room_rule=0)), (4, dict(room_rule=0)),
                  (1, dict(p_kempe=0.0, p_swap=0.5, room_rule=0))):
        untouched(dp, slot, room, seeds, native.TT_ERR_LIMIT, "too large", K=K, history=fits + 1, **kw)
    # P * walkers: the count alone is refused, before any buffer of that size is looked at
    untouched(dp, slot, room, seeds, native.TT_ERR_LIMIT, "P * walkers", K=1024, P=2 ** 21)
    untouched(dp, slot, room, seeds, native.TT_ERR_LIMIT, "P * walkers", K=2, P=2 ** 31 - 1)
    # the largest history that fits
    want = model.lahc_multi_rows(slot, room, seeds, 3, 200, fits, 0.25, 0.5)
    got, _, _, _ = run(dp, slot, room, seeds, 3, 200, fits, 0.25, 0.5, with_eval=False)
    same(got, want)


def test_two_streams_two_work_buffers(problems):
    inst, dp, model = problems("sm")
    slot, room, seeds = lm.population(inst, 9, model)
    args = ((4, 300, 50, 0.25, 0.5, 0, 1), (3, 200, 20, 0.5, 0.0, 0, 0))

    def call(a, stream):
        s, r, g = dev(slot), dev(room), dev(seeds + 17 * a[0])
        out = outputs(9, a[0])
        work = torch.empty(dp.lahc_multi_work_bytes(9, a[0]), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        return (s, r, g, *out), work, stream

    def launch(bufs, work, stream, a):
        s, r, g, *out = bufs
        with torch.cuda.stream(stream) if stream is not None else torch.cuda.stream(torch.cuda.current_stream()):
            dp.lahc_multi(s, r, g, a[0], *a[1:], gain=out[0], accepted=out[1], best_step=out[2], kempe_stats=out[3],
                          winner=out[4], walker_gain=out[5], work=work)
    serial = []
    for a in args:                                                   # one after the other
        bufs, work, _ = call(a, None)
        launch(bufs, work, None, a)
        serial.append([host(t) for t in bufs])
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    pending = [call(a, st) for a, st in zip(args, streams)]
    for (bufs, work, st), a in zip(pending, args):                   # both in flight
        launch(bufs, work, st, a)
    for (bufs, _, _), want in zip(pending, serial):
        same([host(t) for t in bufs], want)
    assert serial[0][3].sum() > 0 and serial[1][3].sum() > 0


# ---------------------------------------------------------------- Island
def walkers_island(dp, **kw):
    return run_island(dp, **{**dict(gens=6, children=2, init="greedy"), **kw})


@pytest.mark.parametrize("variant", ["plain", "augment", "staggered"])
def test_island_walkers(problems, variant):
    inst, dp, _ = problems("sm")
    kw = {"plain": {}, "augment": dict(lahc_swap=0.25, lahc_kempe=0.5, lahc_kempe_rooms="augment"),
          "staggered": dict(schedule="staggered", parts=2, children=4, lahc_swap=0.25, lahc_kempe=0.5)}[variant]
    a = walkers_island(dp, lahc=200, lahc_walkers=4, **kw)
    b = walkers_island(dp, lahc=200, lahc_walkers=4, **kw)
    for k in a.pop:
        assert np.array_equal(host(a.pop[k]), host(b.pop[k])), k           # run twice: identical
    p = a.pop
    hcv, scv, feas, pen = (host(t) for t in dp.eval(p["slot"], p["room"]))
    assert np.array_equal(host(p["hcv"]), hcv) and np.array_equal(host(p["scv"]), scv)
    assert np.array_equal(host(p["feasible"]), feas) and np.array_equal(host(p["penalty"]), pen)
    st, walk = a.lahc_walkers_stats(), a.lahc_stats()
    print(variant, st, walk)
    assert set(st) == {"rows", "walkers", "gain", "gainFirst", "winnerLater"} and st == b.lahc_walkers_stats()
    assert st["walkers"] == 4 and st["rows"] == walk["searched"] > 0 and st["gain"] == walk["gain"]
    assert st["gain"] >= st["gainFirst"] > 0 and 0 < st["winnerLater"] <= st["rows"]
    assert walk["rows"] == 10 + 6 * kw.get("children", 2)
    if "lahc_kempe" in kw:
        ks = a.lahc_kempe_stats()
        assert ("rescued" in ks) == (variant == "augment") and ks["tried"] > 0 and ks["rows"] == walk["rows"]
    a.close()
    b.close()
    assert dp.status() & BAD_GENE == 0


def test_island_one_walker_issues_the_calls_of_today(problems, monkeypatch):
    inst, dp, _ = problems("sm")
    kw = dict(lahc=100, lahc_swap=0.25, lahc_kempe=0.5, lahc_kempe_rooms="augment")
    today = walkers_island(dp, **kw)

    def boom(*a, **k):
        raise AssertionError("lahc_multi called with Island(lahc_walkers=1)")
    monkeypatch.setattr(dp, "lahc_multi", boom)
    one = walkers_island(dp, lahc_walkers=1, **kw)
    for k in today.pop:
        assert np.array_equal(host(one.pop[k]), host(today.pop[k])), k
    assert one.lahc_stats() == today.lahc_stats() and one.lahc_kempe_stats() == today.lahc_kempe_stats()
    assert "lahc_walkers" not in one.on
    with pytest.raises(ValueError, match="lahc_walkers > 1"):
        one.lahc_walkers_stats()
    today.close()
    one.close()


# ---------------------------------------------------------------- the drivers
def test_walkers_in_both_drivers(tmp_path):
    tim = REPO / "tests" / "golden" / "sm.tim"
    inst = ttga.read_tim(tim)
    base = ["-i", str(tim), "-s", "29", "-p", "1", "--pop", "16", "--children", "8", "--generations", "10",
            "--init", "greedy"]
    py, cc, a, lines = both_drivers(tmp_path, base, ["--lahc", "200", "--lahc-walkers", "4"], "lahcWalkers", inst)
    assert stage_lines(py.stdout, "lahc") == stage_lines(cc.stdout, "lahc")              # byte for byte
    assert len(lines) == 1
    k = lines[0]
    assert set(k) == {"rows", "walkers", "gain", "gainFirst", "winnerLater"} and k["walkers"] == 4
    assert k["gain"] >= k["gainFirst"] > 0 and 0 < k["winnerLater"] <= k["rows"]
    walk = [x["lahc"] for x in a if "lahc" in x][0]
    assert walk["gain"] == k["gain"] and walk["searched"] == k["rows"]
    # without the flag (the Python driver) and with one walker (the native one): no such line, the same output
    plain_py = run_driver([sys.executable, "-m", "ttga.islands", *base, "--lahc", "200"], tmp_path)
    plain_cc = run_driver([str(GA), "--lahc", "200", "--lahc-walkers", "1", *base], tmp_path)
    assert not stage_lines(plain_py.stdout, "lahcWalkers") and not stage_lines(plain_cc.stdout, "lahcWalkers")
    assert json_lines(plain_py.stdout) == json_lines(plain_cc.stdout)
