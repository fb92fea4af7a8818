"""Population report on the GPU (include/ttga_report.h): tt_eval_parts' six
constraint parts and eventHcv, tt_slot_histogram, ttga.report and
Island.report(), against references that share no code with the kernels:
ttga.validate.evaluate (numpy, from the definitions) for the parts, a numpy
eventHcv written here from Solution.cpp:173-191, np.bincount for the histogram,
tt_eval and the CPU oracle for the hcv / scv totals. Integer work: every
comparison is exact."""
import ctypes

import numpy as np
import pytest

import ttga
from helpers import dev, host
from oracle_lib import oracle
from ttga import validate

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from ttga import native  # noqa: E402
from ttga.ga import Island  # noqa: E402
from ttga.report import population_report  # noqa: E402

NAMES = ["sm", "med", "tight"]
SHAPES = [(65, 1, 2, 30), (333, 9, 6, 170), (448, 11, 5, 300), (449, 10, 5, 200), (250, 64, 4, 120)]
WIDE = [(1000, 20, 6, 700), (2600, 12, 5, 150)]


def load(golden_dir, name):
    z = np.load(golden_dir / f"{name}.npz")
    E, R, F, S = (int(x) for x in z["dims"])
    return ttga.Instance(E, R, F, S, z["room_size"], z["student_events"], z["room_features"], z["event_features"]), z


def ref_parts(inst, slots, rooms, rows=None):
    """[rows, 6] from ttga.validate.evaluate, one timetable per call."""
    rows = range(slots.shape[0]) if rows is None else rows
    out = []
    for i in rows:
        ev = validate.evaluate(inst, slots[i], rooms[i])
        out.append([ev[k] for k in native.PART_NAMES])
    return np.array(out, np.int32).reshape(-1, 6)


def ref_event_hcv(inst, slots, rooms):
    """Solution::eventHcv (Solution.cpp:173-191) for every event of every row:
    the other events of e's slot in e's room + those correlated with e."""
    A = inst.student_events.astype(np.int64)
    corr = (A.T @ A) > 0
    out = np.zeros(slots.shape, np.int32)
    for i in range(slots.shape[0]):
        same = slots[i][:, None] == slots[i][None, :]
        np.fill_diagonal(same, False)
        out[i] = (same & (rooms[i][:, None] == rooms[i][None, :])).sum(1) + (same & corr).sum(1)
    return out


def population(inst, orc, P, seed):
    """P random timetables: rooms half random, half from the oracle's assignRooms."""
    slots, _ = ttga.random_slots(ttga.population_seeds(seed, P), inst.E)
    rooms = np.random.default_rng(seed).integers(0, inst.R, size=(P, inst.E), dtype=np.uint8)
    rooms[::2] = orc.problem(inst).assign_rooms(slots[::2])
    return slots, rooms


def check_all(inst, orc, slots, rooms, part_rows=None, with_eval=True):
    """Parts (on part_rows, default all), eventHcv, the totals against tt_eval
    (unless with_eval is False) and the oracle, and the eventHcv identity, on
    one population."""
    dp = native.DeviceProblem(inst)
    parts, eh = (host(t) for t in dp.eval_parts(dev(slots), dev(rooms), event_hcv=True))
    assert parts.shape == (slots.shape[0], 6) and parts.dtype == np.int32
    rows = list(range(slots.shape[0])) if part_rows is None else part_rows
    assert np.array_equal(parts[rows], ref_parts(inst, slots, rooms, rows))
    assert np.array_equal(eh, ref_event_hcv(inst, slots, rooms))
    ohcv, oscv, _, _ = orc.problem(inst).eval(slots, rooms)
    assert np.array_equal(parts[:, :3].sum(1), ohcv) and np.array_equal(parts[:, 3:].sum(1), oscv)
    if with_eval:
        hcv, scv, _, _ = (host(t) for t in dp.eval(dev(slots), dev(rooms)))
        assert np.array_equal(hcv, ohcv) and np.array_equal(scv, oscv)
    assert np.array_equal(eh.sum(1), 2 * (parts[:, 0] + parts[:, 1]))
    only = host(dp.eval_parts(dev(slots), dev(rooms)))
    assert np.array_equal(only, parts)
    return parts, eh


@pytest.fixture(scope="module")
def orc():
    return oracle()


@pytest.mark.parametrize("name", NAMES)
def test_parts_golden(golden_dir, orc, name):
    inst, z = load(golden_dir, name)
    check_all(inst, orc, z["slots"], z["rooms"])
    check_all(inst, orc, z["skew_slots"], z["skew_rooms"])


@pytest.mark.parametrize("dims", SHAPES, ids=lambda d: "E%dR%d" % d[:2])
def test_parts_generated(orc, dims):
    """The 64-bit word edge of the event bitsets (E 65, 448), R = 1 and R = 64
    (bit 63 of possibleRooms), both sides of the 448-event path boundary; a
    ragged population and a single individual."""
    inst = ttga.generate(*dims, seed=11)
    slots, rooms = population(inst, orc, 67, 4242)
    check_all(inst, orc, slots, rooms)
    check_all(inst, orc, slots[66:], rooms[66:])


@pytest.mark.parametrize("dims", WIDE, ids=lambda d: "E%dR%d" % d[:2])
def test_parts_wide(orc, dims):
    """E > 448: the bucket form. Totals and eventHcv on every row, the parts
    against validate.evaluate on three rows (seconds per row at E 2600)."""
    inst = ttga.generate(*dims, seed=13)
    slots, rooms = population(inst, orc, 9, 777)
    check_all(inst, orc, slots, rooms, part_rows=[0, 4, 8])


def test_parts_crowded_cell(orc):
    """Every event in one (slot, room) cell: a cell counter narrower than 9
    bits goes wrong."""
    inst = ttga.generate(300, 4, 3, 150, seed=3)
    slots = np.full((2, 300), 8, np.uint8)
    rooms = np.zeros((2, 300), np.uint8)
    parts, eh = check_all(inst, orc, slots, rooms)
    assert parts[0, 0] == 44850
    assert (eh >= 299).all()
    assert parts[0, 3] == int(inst.student_events.sum())


def test_parts_degenerate_instances(orc):
    one = ttga.Instance(1, 1, 1, 0, np.array([5], np.int32), np.zeros((0, 1), np.int32), np.ones((1, 1), np.int32),
                        np.zeros((1, 1), np.int32))
    parts, eh = check_all(one, orc, np.array([[8]], np.uint8), np.zeros((1, 1), np.uint8))
    assert not parts.any() and not eh.any()

    # an event nobody attends (its correlation diagonal is 0) and a student with no events
    g = ttga.generate(130, 3, 3, 60, seed=5)
    A = g.student_events.copy()
    A[:, 64] = 0
    A[7, :] = 0
    inst = ttga.Instance(g.E, g.R, g.F, g.S, g.room_size, A, g.room_features, g.event_features)
    slots, rooms = population(inst, orc, 5, 99)
    slots[:, :] = slots % 3 * 9 + 8                   # crowded slots: event 64 has company
    check_all(inst, orc, slots, rooms)

    # one student with all nine slots of day 0 and one class on each other day
    E = 13
    inst = ttga.Instance(E, 1, 1, 1, np.array([5], np.int32), np.ones((1, E), np.int32), np.ones((1, 1), np.int32),
                         np.zeros((E, 1), np.int32))
    slots = np.array([list(range(9)) + [9, 18, 27, 36]], np.uint8)
    parts, _ = check_all(inst, orc, slots, np.zeros((1, E), np.uint8))
    assert parts[0].tolist() == [0, 0, 0, 1, 7, 4]


@pytest.mark.parametrize("dims", [(333, 9, 6, 170), (449, 10, 5, 200)], ids=["bits", "bucket"])
def test_parts_invalid_genes(orc, dims):
    inst = ttga.generate(*dims, seed=11)
    dp = native.DeviceProblem(inst)
    slots, rooms = population(inst, orc, 67, 4242)
    parts, eh = (host(t) for t in dp.eval_parts(dev(slots), dev(rooms), event_hcv=True))
    slots[5, inst.E - 1] = 45
    slots[6, 0] = 255
    rooms[7, inst.E // 2] = inst.R
    bparts, beh = (host(t) for t in dp.eval_parts(dev(slots), dev(rooms), event_hcv=True))
    bonly = host(dp.eval_parts(dev(slots), dev(rooms)))
    ok = np.ones(67, bool)
    ok[[5, 6, 7]] = False
    assert (bparts[~ok] == -1).all() and (beh[~ok] == -1).all() and (bonly[~ok] == -1).all()
    assert np.array_equal(bparts[ok], parts[ok]) and np.array_equal(beh[ok], eh[ok])
    assert np.array_equal(bonly, bparts)


def test_parts_without_event_hcv_writes_only_parts(golden_dir):
    """event_hcv = NULL: parts alone are written -- the poisoned words that
    follow them (where a [P][E] array could be taken to start) stay."""
    inst, z = load(golden_dir, "sm")
    dp = native.DeviceProblem(inst)
    P = 37
    slot, room = dev(z["slots"][:P]), dev(z["rooms"][:P])
    want, eh = dp.eval_parts(slot, room, event_hcv=True)
    buf = torch.full((P * 6 + P * inst.E,), -7777, dtype=torch.int32, device="cuda")
    out = dp.eval_parts(slot, room, out=buf[:P * 6].view(P, 6))
    assert out.data_ptr() == buf.data_ptr()
    got = host(buf)
    assert np.array_equal(got[:P * 6].reshape(P, 6), host(want))
    assert (got[P * 6:] == -7777).all()
    assert (host(eh) != -7777).all()


def test_parts_are_stream_ordered(orc):
    """Issued on a side stream right behind a tt_random_init on that stream,
    with no synchronisation in between."""
    inst = ttga.config_instance("sm")
    dp = native.DeviceProblem(inst)
    P = 4096
    rng = dev(ttga.population_seeds(2024, P))
    slot = torch.zeros((P, inst.E), dtype=torch.uint8, device="cuda")
    room = torch.zeros_like(slot)
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        dp.random_init(rng, slot, room)
        parts, eh = dp.eval_parts(slot, room, event_hcv=True)
        hist = dp.slot_histogram(slot)
    st.synchronize()
    torch.cuda.synchronize()
    parts2, eh2 = dp.eval_parts(slot, room, event_hcv=True)
    assert np.array_equal(host(parts), host(parts2)) and np.array_equal(host(eh), host(eh2))
    assert np.array_equal(host(hist), host(dp.slot_histogram(slot)))
    s, r = host(slot), host(room)
    hcv, scv, _, _ = orc.problem(inst).eval(s, r)
    p = host(parts)
    assert hcv.any() and np.array_equal(p[:, :3].sum(1), hcv) and np.array_equal(p[:, 3:].sum(1), scv)


def ref_hist(slots, E):
    h = np.zeros((E, 45), np.int32)
    for e in range(E):
        col = slots[:, e]
        h[e] = np.bincount(col[col < 45], minlength=45)
    return h


@pytest.mark.parametrize("P", [1, 65, 1000])
@pytest.mark.parametrize("E", [1, 449])
def test_slot_histogram(P, E):
    inst = ttga.generate(E, 3, 2, 20, seed=2) if E > 1 else ttga.Instance(
        1, 1, 1, 0, np.array([5], np.int32), np.zeros((0, 1), np.int32), np.ones((1, 1), np.int32),
        np.zeros((1, 1), np.int32))
    dp = native.DeviceProblem(inst)
    slots = np.random.default_rng(P + E).integers(0, 45, size=(P, E), dtype=np.uint8)
    slots[::7, E // 2] = 45                            # genes >= 45 are counted nowhere
    slots[P // 2, E - 1] = 255
    assert np.array_equal(host(dp.slot_histogram(dev(slots))), ref_hist(slots, E))
    # the output is overwritten, not accumulated
    buf = torch.full((E, 45), 123456, dtype=torch.int32, device="cuda")
    s = dev(slots)
    rc = dp.lib.tt_slot_histogram(dp.handle, s.data_ptr(), P, buf.data_ptr(),
                                  ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0 and np.array_equal(host(buf), ref_hist(slots, E))


def test_pairs_differing_against_pair_count(golden_dir):
    inst, z = load(golden_dir, "sm")
    dp = native.DeviceProblem(inst)
    P = 65
    slots = z["slots"][:P].copy()
    slots[40:] = slots[3]                              # duplicates: pairs that differ nowhere
    pop = {"slot": dev(slots), "room": dev(z["rooms"][:P])}
    rep = population_report(dp, pop)
    want = sum(int((slots[i] != slots[j]).sum()) for i in range(P) for j in range(i + 1, P))
    assert rep["diversity"] == {"events": inst.E, "size": P, "pairs_differing": want}
    assert all(type(v) is int for v in rep["diversity"].values())


@pytest.mark.parametrize("schedule", ["batch", "staggered"])
def test_island_report(golden_dir, schedule):
    inst, _ = load(golden_dir, "sm")
    dp = native.DeviceProblem(inst)
    isl = Island(dp, pop_size=12, children=4, max_steps=200, seed=42, schedule=schedule, parts=2)
    isl.initialize()
    for _ in range(20):
        isl.step()
    rep = isl.report()
    best = isl.member(0)
    ev = validate.evaluate(inst, best["slot"], best["room"])
    assert rep["best"] == {k: ev[k] for k in native.PART_NAMES}
    assert sum(rep["best"][k] for k in native.PART_NAMES[:3]) == best["hcv"]
    assert sum(rep["best"][k] for k in native.PART_NAMES[3:]) == best["scv"]
    parts = host(dp.eval_parts(isl.pop["slot"], isl.pop["room"]))
    popu = rep["population"]
    assert popu["size"] == 12 and popu["invalid"] == 0
    assert [popu["sum"][k] for k in native.PART_NAMES] == parts.sum(0).tolist()
    assert [popu["nonzero"][k] for k in native.PART_NAMES] == (parts != 0).sum(0).tolist()
    assert popu["feasible"] == int(host(isl.pop["feasible"]).sum())
    assert rep["diversity"]["events"] == inst.E and rep["diversity"]["size"] == 12
    isl.close()


def test_population_report_counts_invalid_rows(golden_dir):
    inst, z = load(golden_dir, "sm")
    dp = native.DeviceProblem(inst)
    slots, rooms = z["slots"][:20].copy(), z["rooms"][:20].copy()
    slots[4, 0] = 45
    rooms[9, 3] = inst.R
    rep = population_report(dp, {"slot": dev(slots), "room": dev(rooms)})
    ok = [i for i in range(20) if i not in (4, 9)]
    want = ref_parts(inst, slots, rooms, ok)
    assert rep["population"]["invalid"] == 2 and rep["population"]["size"] == 20
    assert [rep["population"]["sum"][k] for k in native.PART_NAMES] == want.sum(0).tolist()
    assert [rep["population"]["nonzero"][k] for k in native.PART_NAMES] == (want != 0).sum(0).tolist()
    assert rep["population"]["feasible"] == int((want[:, :3].sum(1) == 0).sum())
