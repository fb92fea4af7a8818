"""The single-event neighbourhood (include/ttga/move1.h) on the GPU against
tests/move1_model.py: summary, d_scv and to_room bit for bit, scanned and
unscanned rows mixed in one launch; the descent's rows, gain, passes, scv and
penalty bit for bit, with tt_eval around it; then, without the model, sampled
table entries applied on the host and evaluated by tt_eval.

The counts asserted under "conditions" are the model's: they say that the
rows exercise what each shape is in the list for (tests/test_move1_cpu.py
shows the defects the comparison can see)."""
import ctypes

import numpy as np
import pytest

import ttga
import lahc_model as lm
import move1_model as mm
from helpers import dev, host

pytestmark = pytest.mark.gpu

import torch  # noqa: E402
from ttga import native  # noqa: E402

BAD_GENE = 1024                                  # tt_device_status bit 10
FILL = 12345
INT_MAX = 2 ** 31 - 1
T = np.arange(45)


@pytest.fixture(scope="module")
def problems():
    cache = {}

    def get(name):
        if name not in cache:
            inst = lm.SHAPES[name]()
            cache[name] = (inst, native.DeviceProblem(inst), mm.Model(inst))
        return cache[name]
    return get


@pytest.fixture(scope="module")
def rows(problems):
    """(slot, room, the model's scan) of a shape's first P rows, computed once."""
    cache = {}

    def get(name, P):
        if (name, P) not in cache:
            inst, _, model = problems(name)
            slot, room = mm.population(inst, P, model)
            cache[name, P] = (slot, room, model.scan_rows(slot, room))
        return cache[name, P]
    return get


def filled(dtype, *shape):
    return torch.full(shape, FILL if dtype != "uint8" else 77, dtype=getattr(torch, dtype), device="cuda")


def gpu_scan(dp, slot, room, summary=True, d_scv=True, to_room=True):
    """tt_move1_scan on numpy rows: (summary, d_scv, to_room), None for an
    output that was not asked for; the inputs must come back as they went."""
    P, E = slot.shape
    s, r = dev(slot), dev(room)
    sm = filled("int32", P, 6) if summary else None
    d = filled("int32", P, E, 45) if d_scv else None
    tr = filled("uint8", P, E, 45) if to_room else None
    dp.move1_scan(s, r, summary=sm, d_scv=d, to_room=tr)
    assert np.array_equal(host(s), slot) and np.array_equal(host(r), room)
    return tuple(None if t is None else host(t) for t in (sm, d, tr))


def same_scan(got, want):
    for name, g, w in zip(("summary", "d_scv", "to_room"), got, want):
        if g is None:
            continue
        assert g.shape == w.shape and g.dtype == w.dtype, name
        P = len(g)
        diff = np.flatnonzero((g.reshape(P, -1) != w.reshape(P, -1)).any(axis=1))
        assert diff.size == 0, f"{name} differs in rows {diff[:8]}: gpu {g[diff[0]]} want {w[diff[0]]}"


# ---------------------------------------------------------------- the scan
# id: (shape, P, rows the model scans)
SCAN_CASES = {
    "sm": ("sm", 67, 54), "E1": ("E1", 67, 67), "E2": ("E2", 67, 54), "E3": ("E3", 67, 54), "E63": ("E63", 67, 54),
    "E64": ("E64", 67, 54), "E65": ("E65", 67, 54), "R1": ("R1", 67, 54), "R64": ("R64", 67, 54), "S0": ("S0", 67, 54),
    "extremes": ("extremes", 67, 46), "tight_rooms": ("tight_rooms", 6, 5), "tight": ("tight", 6, 0),
    "syn": ("syn", 2, 0), "syn_sparse": ("syn_sparse", 2, None), "med": ("med", 8, None), "P1": ("sm", 1, 1),
    "P65": ("sm", 65, None),
}


@pytest.mark.parametrize("cid", list(SCAN_CASES))
def test_scan_vs_model(problems, rows, cid):
    shape, P, n_scanned = SCAN_CASES[cid]
    inst, dp, model = problems(shape)
    slot, room, want = rows(shape, P)
    same_scan(gpu_scan(dp, slot, room), want)
    sm, d, tr = want
    scanned = sm[:, 0] == 1
    print(cid, "scanned", int(scanned.sum()), "of", P, "feasible moves", sm[scanned, 1].tolist()[:4], "improving",
          sm[scanned, 2].tolist()[:4])
    # conditions
    assert n_scanned is None or scanned.sum() == n_scanned
    if shape in lm.NO_FEASIBLE_ROW:
        assert not scanned.any() and (d == mm.NONE).all() and (tr == mm.UNSCANNED).all()
        return
    assert scanned.any() and (sm[scanned, 1] >= 1).all()                # every scanned row has a feasible move
    assert P < 5 or inst.E < 2 or not scanned.all()                      # both kinds of rows in the launch
    assert (tr[scanned] == mm.UNSCANNED).sum() == 0 and (d[scanned] != mm.NONE).all()
    if shape == "sm":
        assert (sm[scanned, 2] >= 1).all()                               # ... and improving ones
    if cid in ("E2", "E65", "R1", "S0"):
        assert (tr[scanned] == mm.NO_ROOM).any()
    if cid == "R64":
        assert (tr[scanned] == 63).any()
    if inst.E >= 3 and inst.S > 0:
        assert (tr[scanned] == mm.CLASH).any()
    if cid == "S0":
        assert not d[scanned].any()
    assert dp.status() & BAD_GENE == 0


def test_invalid_genes():
    """A slot gene 45 and a room gene R between valid rows: unscanned, status bit
    10, inputs untouched (gpu_scan); the descent leaves them alone too. Own
    handle: the status word is sticky."""
    inst = lm.SHAPES["sm"]()
    dp, model = native.DeviceProblem(inst), mm.Model(inst)
    slot, room = mm.population(inst, 6, model)
    slot[1, 7] = 45
    room[4, 3] = inst.R
    assert dp.status() == 0
    want = model.scan_rows(slot, room)
    assert want[0][:, 0].tolist() == [1, 0, 0, 1, 0, 1]
    same_scan(gpu_scan(dp, slot, room), want)
    assert dp.status() & BAD_GENE == BAD_GENE
    dp.close()
    dp = native.DeviceProblem(inst)
    got = gpu_descent(dp, slot, room, 8, with_eval=False)
    same_descent(got, model.descent_rows(slot, room, 8))
    assert not got[3][[1, 2, 4]].any() and (got[3][[0, 3, 5]] == 8).all()
    assert dp.status() & BAD_GENE == BAD_GENE
    dp.close()


def test_each_output_may_be_null(problems, rows):
    inst, dp, model = problems("sm")
    slot, room, want = rows("sm", 67)
    for ask in ((True, False, False), (False, True, False), (False, False, True), (False, True, True),
                (True, False, True), (True, True, False)):
        got = gpu_scan(dp, slot, room, *ask)
        assert [g is not None for g in got] == list(ask)
        same_scan(got, want)
    # no output at all: TT_OK, and nothing to launch
    assert gpu_scan(dp, slot, room, False, False, False) == (None, None, None)
    s, r = dev(slot), dev(room)                                         # P == 0: TT_OK on real addresses, nothing written
    sm = filled("int32", 67, 6)
    vp = ctypes.c_void_p
    assert dp.lib.tt_move1_scan(dp.handle, vp(s.data_ptr()), vp(r.data_ptr()), 0, vp(sm.data_ptr()), None, None, None) == 0
    assert dp.lib.tt_move1_descent(dp.handle, vp(s.data_ptr()), vp(r.data_ptr()), 0, 3, None, None, None, None, None) == 0
    assert (host(sm) == FILL).all() and np.array_equal(host(s), slot) and np.array_equal(host(r), room)


def full_house():
    """45 events in one room, event e in slot e, every student in one event:
    no two events are correlated and every other slot's room is taken."""
    A = np.zeros((45, 45), np.int32)
    A[np.arange(45), np.arange(45)] = 1
    inst = ttga.Instance(45, 1, 1, 45, np.array([5], np.int32), A, np.ones((1, 1), np.int32), np.zeros((45, 1), np.int32))
    return inst, np.arange(45, dtype=np.uint8)[None, :].copy(), np.zeros((1, 45), np.uint8)


def test_full_house():
    inst, slot, room = full_house()
    assert inst.possible_rooms().all()
    dp, model = native.DeviceProblem(inst), mm.Model(inst)
    sm, d, tr = gpu_scan(dp, slot, room)
    same_scan((sm, d, tr), model.scan_rows(slot, room))
    assert sm[0].tolist() == [1, 0, 0, 0, -1, -1]
    off = ~np.eye(45, dtype=bool)
    assert (tr[0][off] == mm.NO_ROOM).all() and not tr[0][~off].any()
    assert d[0].any() and not d[0][~off].any()                          # the deltas are there all the same
    got = gpu_descent(dp, slot, room, INT_MAX)
    assert got[3].tolist() == [0] and got[2].tolist() == [0] and np.array_equal(got[0], slot)
    dp.close()


# ---------------------------------------------------------------- the descent
def gpu_descent(dp, slot, room, max_passes, with_eval=True):
    """tt_move1_descent on numpy rows: (slot, room, gain, passes, scv, penalty in
    place, tt_eval before, tt_eval after)."""
    P = slot.shape[0]
    s, r = dev(slot), dev(room)
    before = [host(t) for t in dp.eval(s, r)] if with_eval else None
    scv = dev(before[1]) if with_eval else None
    pen = dev(before[3]) if with_eval else None
    gain, passes = filled("int32", P), filled("int32", P)
    dp.move1_descent(s, r, max_passes, scv=scv, penalty=pen, gain=gain, passes=passes)
    after = [host(t) for t in dp.eval(s, r)] if with_eval else None
    return (host(s), host(r), host(gain), host(passes), host(scv) if with_eval else None,
            host(pen) if with_eval else None, before, after)


def same_descent(got, want):
    for name, g, w in zip(("slot", "room", "gain", "passes"), got, want):
        P = len(g)
        diff = np.flatnonzero((g.reshape(P, -1) != w.reshape(P, -1)).any(axis=1))
        assert diff.size == 0, f"{name} differs in rows {diff[:8]}: gpu {g[diff[0]]} want {w[diff[0]]}"


def check_descent(dp, model, slot, room, max_passes, ties=None):
    """The model's rows bit for bit, and around the call tt_eval: hcv and the
    feasible flag unchanged, scv lower by exactly the gain, scv and penalty in
    place equal to a fresh evaluation (the model's credit too); unscanned rows
    byte-identical with gain = passes = 0; the rooms of unmoved events kept."""
    want = model.descent_rows(slot, room, max_passes, ties)
    got = gpu_descent(dp, slot, room, max_passes)
    same_descent(got, want)
    s, r, gain, passes, scv, pen, before, after = got
    assert np.array_equal(after[0], before[0]) and np.array_equal(after[2], before[2])
    assert np.array_equal(after[1], before[1] - gain) and (gain >= passes).all() and (passes >= 0).all()
    assert np.array_equal(scv, after[1]) and np.array_equal(pen, after[3])
    credited = mm.credit(before[1], before[3], gain)
    assert np.array_equal(scv, credited[0]) and np.array_equal(pen, credited[1])
    closed = before[0] != 0
    assert np.array_equal(s[closed], slot[closed]) and np.array_equal(r[closed], room[closed])
    assert not gain[closed].any() and not passes[closed].any()
    assert (passes <= max_passes).all()
    unmoved = s == slot
    assert np.array_equal(r[unmoved], room[unmoved]) and ((~unmoved).sum(axis=1) <= passes).all()
    return got


def early_stop_is_a_local_optimum(dp, got, max_passes):
    """Rows that stopped before the cap: their rescan has no improving move."""
    s, r, gain, passes = got[:4]
    sm = gpu_scan(dp, s, r, True, False, False)[0]
    stopped = (sm[:, 0] == 1) & (passes < max_passes)
    assert stopped.any() and not sm[stopped, 2].any() and (sm[stopped, 3] >= 0).all()
    return stopped


@pytest.mark.parametrize("shape", ["E1", "E2", "E3", "E63", "E64", "E65", "R1", "R64", "S0", "extremes", "tight_rooms"])
def test_descent_uncapped_small_shapes(problems, rows, shape):
    inst, dp, model = problems(shape)
    P = SCAN_CASES[shape][1]
    slot, room, _ = rows(shape, P)
    got = check_descent(dp, model, slot, room, INT_MAX)
    print(shape, "gain", int(got[2].sum()), "passes", int(got[3].min()), "to", int(got[3].max()))
    early_stop_is_a_local_optimum(dp, got, INT_MAX)
    if shape == "S0":
        assert not got[2].any() and not got[3].any()                    # no student: every delta is 0
    elif inst.E >= 60:
        assert (got[3] > 1).any()
    assert dp.status() & BAD_GENE == 0


def test_descent_uncapped_sm(problems, rows):
    """All 67 rows of sm (the model takes about three seconds); the conditions:
    every scanned row descends for 29 to 52 passes, and more than 1,000 of the
    passes had several feasible moves of the least delta, so the tie rule decides."""
    inst, dp, model = problems("sm")
    slot, room, want = rows("sm", 67)
    ties = []
    got = check_descent(dp, model, slot, room, INT_MAX, ties)
    scanned = want[0][:, 0] == 1
    passes = got[3]
    print("sm passes", int(passes[scanned].min()), "to", int(passes[scanned].max()), "tied", sum(t > 1 for t in ties),
          "of", len(ties), "gain", int(got[2].sum()))
    assert passes[scanned].min() >= 29 and passes[scanned].max() <= 52 and len(ties) == passes.sum()
    assert sum(t > 1 for t in ties) > 1000
    assert early_stop_is_a_local_optimum(dp, got, INT_MAX).sum() == scanned.sum()
    assert np.array_equal(got[0][:16], model.descent_rows(slot[:16], room[:16], INT_MAX)[0])


@pytest.mark.parametrize("cap", [1, 8])
def test_descent_capped_sm(problems, rows, cap):
    inst, dp, model = problems("sm")
    slot, room, want = rows("sm", 67)
    got = check_descent(dp, model, slot, room, cap)
    scanned = want[0][:, 0] == 1
    assert (got[3][scanned] == cap).all()                               # sm's rows go on for 29 passes at least
    if cap == 1:                                                        # one pass applies the summary's move
        sm = want[0]
        assert np.array_equal(got[2][scanned], -sm[scanned, 3])
        for i in np.flatnonzero(scanned):
            assert got[0][i][sm[i, 4]] == sm[i, 5] and got[1][i][sm[i, 4]] == want[2][i][sm[i, 4], sm[i, 5]]


def test_descent_capped_med(problems, rows):
    inst, dp, model = problems("med")
    slot, room, want = rows("med", 8)
    got = check_descent(dp, model, slot[:4], room[:4], 3)
    assert (got[3][want[0][:4, 0] == 1] == 3).all() and (want[0][:4, 0] == 1).any()


@pytest.mark.parametrize("shape,K", [("sm", 5), ("E65", 20), ("R1", 3)])
def test_k_host_rounds_of_scan_and_apply_equal_max_passes_k(problems, rows, shape, K):
    """The host applies the GPU scan's own summary K times (the room from the
    GPU's to_room); tt_move1_descent(max_passes=K) gives the same rows."""
    inst, dp, model = problems(shape)
    slot, room, _ = rows(shape, 67)
    s, r = slot.copy(), room.copy()
    gain, passes = np.zeros(67, np.int64), np.zeros(67, np.int64)
    for _ in range(K):
        sm, _, tr = gpu_scan(dp, s, r, True, False, True)
        for i in np.flatnonzero((sm[:, 0] == 1) & (sm[:, 1] > 0) & (sm[:, 3] < 0)):
            e, t = sm[i, 4], sm[i, 5]
            s[i, e], r[i, e] = t, tr[i, e, t]
            gain[i] -= sm[i, 3]
            passes[i] += 1
    got = gpu_descent(dp, slot, room, K)
    same_descent(got, (s, r, gain, passes))
    assert passes.max() == K                                            # rows that the cap stopped
    assert shape != "E65" or (passes[passes > 0] < K).any()            # ... and, on E65, rows that stopped by themselves


# ---------------------------------------------------------------- independent of the model
# every shape whose scanned rows hold 200 feasible and 200 refused entries; E1, E2 and E3 have
# fewer than 200 refused ones in all 67 rows (0, 54 and 215 entries, and E3's feasible rows are
# 128 a row), syn_sparse is left to the model: its rows cost the model seconds each
@pytest.mark.parametrize("shape", ["sm", "E63", "E64", "E65", "R1", "R64", "S0", "extremes", "tight_rooms", "med"])
def test_sampled_entries_against_tt_eval(problems, rows, shape):
    """200 feasible entries: the move applied on the host has hcv 0 and scv
    higher by d_scv under tt_eval. 200 CLASH or NO_ROOM entries: the event
    moved with its old room has hcv > 0, and its scv differs by d_scv all the same."""
    inst, dp, model = problems(shape)
    P = SCAN_CASES[shape][1]
    slot, room, _ = rows(shape, P)
    sm, d, tr = gpu_scan(dp, slot, room)
    hcv0, scv0, _, _ = (host(t) for t in dp.eval(dev(slot), dev(room)))
    assert np.array_equal(sm[:, 0] == 1, hcv0 == 0)
    g = np.random.default_rng(5)
    off = T[None, None, :] != slot[:, :, None]
    scanned = (sm[:, 0] == 1)[:, None, None]
    for kind, pick in (("feasible", scanned & off & (tr < 64)), ("refused", scanned & off & (tr >= mm.NO_ROOM))):
        cells = np.argwhere(pick)
        assert len(cells) >= 200, (kind, len(cells))
        cells = cells[g.choice(len(cells), 200, replace=False)]
        s2, r2 = slot[cells[:, 0]].copy(), room[cells[:, 0]].copy()
        k = np.arange(200)
        s2[k, cells[:, 1]] = cells[:, 2]
        if kind == "feasible":
            r2[k, cells[:, 1]] = tr[cells[:, 0], cells[:, 1], cells[:, 2]]
        hcv, scv, _, _ = (host(t) for t in dp.eval(dev(s2), dev(r2)))
        assert np.array_equal(scv - scv0[cells[:, 0]], d[cells[:, 0], cells[:, 1], cells[:, 2]]), kind
        assert (hcv == 0).all() if kind == "feasible" else (hcv > 0).all(), kind


# ---------------------------------------------------------------- limits and arguments
def test_lds_limit_launches_nothing():
    """8,200 students: 8 * (45 + 45 + 8200) + 80 = 66,400 bytes, the masks alone pass 64 KB."""
    inst = ttga.generate(40, 3, 2, 8200)
    dp = native.DeviceProblem(inst)
    g = np.random.default_rng(3)
    slot, room = g.integers(0, 45, (4, 40)).astype(np.uint8), g.integers(0, 3, (4, 40)).astype(np.uint8)
    s, r = dev(slot), dev(room)
    outs = [filled("int32", 4, 6), filled("int32", 4, 40, 45), filled("uint8", 4, 40, 45)]
    with pytest.raises(native.TTError, match="too large") as ei:
        dp.move1_scan(s, r, *outs)
    assert ei.value.code == native.TT_ERR_LIMIT
    four = [filled("int32", 4) for _ in range(4)]
    with pytest.raises(native.TTError, match="too large") as ei:
        dp.move1_descent(s, r, 5, *four)
    assert ei.value.code == native.TT_ERR_LIMIT
    assert np.array_equal(host(s), slot) and np.array_equal(host(r), room)
    assert all((host(t) == (77 if t.element_size() == 1 else FILL)).all() for t in outs + four)
    dp.close()


def test_invalid_arguments_are_named_and_launch_nothing(problems, rows):
    inst, dp, model = problems("sm")
    slot, room, _ = rows("sm", 67)
    s, r = dev(slot[:4]), dev(room[:4])
    outs = [filled("int32", 4, 6), filled("int32", 4, inst.E, 45), filled("uint8", 4, inst.E, 45)]
    four = [filled("int32", 4) for _ in range(4)]
    lib, h, vp = dp.lib, dp.handle, ctypes.c_void_p
    sp, rp = vp(s.data_ptr()), vp(r.data_ptr())
    o = [vp(t.data_ptr()) for t in outs]
    f = [vp(t.data_ptr()) for t in four]
    for call, word in ((lambda: lib.tt_move1_scan(None, sp, rp, 4, *o, None), b"null tt_problem"),
                       (lambda: lib.tt_move1_scan(None, None, None, -1, *o, None), b"null tt_problem"),
                       (lambda: lib.tt_move1_scan(h, sp, rp, -1, *o, None), b"negative population size"),
                       (lambda: lib.tt_move1_scan(h, None, rp, 4, *o, None), b"tt_move1_scan: null population buffer"),
                       (lambda: lib.tt_move1_scan(h, sp, None, 4, *o, None), b"tt_move1_scan: null population buffer"),
                       (lambda: lib.tt_move1_descent(None, sp, rp, 4, 0, *f, None), b"null tt_problem"),
                       (lambda: lib.tt_move1_descent(h, sp, rp, -1, 1, *f, None), b"negative population size"),
                       (lambda: lib.tt_move1_descent(h, None, rp, 4, 1, *f, None),
                        b"tt_move1_descent: null population buffer"),
                       (lambda: lib.tt_move1_descent(h, sp, None, 4, 1, *f, None),
                        b"tt_move1_descent: null population buffer"),
                       (lambda: lib.tt_move1_descent(h, sp, rp, 4, 0, *f, None), b"tt_move1_descent: max_passes"),
                       (lambda: lib.tt_move1_descent(h, sp, rp, 4, -7, *f, None), b"tt_move1_descent: max_passes")):
        assert call() == native.TT_ERR_INVALID
        assert word in lib.tt_last_error(), lib.tt_last_error()
    assert np.array_equal(host(s), slot[:4]) and np.array_equal(host(r), room[:4])
    assert all((host(t) == (77 if t.element_size() == 1 else FILL)).all() for t in outs + four)
    # and with every output NULL the descent still descends
    dp.move1_descent(s, r, 2)
    want = model.descent_rows(slot[:4], room[:4], 2)
    assert np.array_equal(host(s), want[0]) and np.array_equal(host(r), want[1])
