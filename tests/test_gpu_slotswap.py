"""The timeslot-swap descent (include/ttga_slotswap.h) on the GPU against
tests/slotswap_model.py: the new rows, gain, passes and perm bit for bit, and
around every call tt_eval and tt_eval_parts: hcv, feasibility and the three
hard parts unchanged, scv lower by exactly the gain, and the scv / penalty
updated in place equal to a fresh evaluation. Then Island(slot_swap=...) and
the two drivers with --slot-swap."""
import numpy as np
import pytest

import ttga
import slotswap_model as sm
from helpers import dev, host, json_lines
from stage_checks import GA, both_drivers, run_driver, run_island

pytestmark = pytest.mark.gpu

import torch  # noqa: E402
from ttga import native  # noqa: E402

UNCAPPED = 2 ** 31 - 1
# tt_device_status bits 0 and 2..7 (bit 1 is the local search's): clear unless a test says otherwise
STATUS_MASK = 0b11111101


def variant(inst, student_events):
    return ttga.Instance(inst.E, inst.R, inst.F, student_events.shape[0], inst.room_size, student_events,
                         inst.room_features, inst.event_features)


def extremes():
    """A student who attends nothing and one who attends 45 of the 60 events."""
    inst = ttga.generate(60, 5, 3, 30, seed=5)
    A = inst.student_events.copy()
    A[0, :] = 0
    A[1, :] = 0
    A[1, :45] = 1
    return variant(inst, A)


SHAPES = {
    "sm": lambda: ttga.config_instance("sm"),                 # S 80: 2.5 MFMA K-steps
    "med": lambda: ttga.config_instance("med"),
    "tight": lambda: sm.load_golden("tight"),                 # S 100, E 120
    "S7": lambda: ttga.generate(60, 5, 3, 7, seed=7),         # less than one K-step
    "S64": lambda: ttga.generate(60, 5, 3, 64, seed=8),       # exactly one chunk
    "S65": lambda: ttga.generate(60, 5, 3, 65, seed=9),       # one student in the second chunk
    "S1100": lambda: ttga.generate(60, 5, 3, 1100, seed=10),  # 18 chunks, the last of 12 students
    "extremes": extremes,
    "E20": lambda: ttga.generate(20, 3, 2, 30, seed=11),      # most slots are empty
    "E61": lambda: ttga.generate(61, 5, 3, 40, seed=12),      # E not a multiple of 4
    "syn": lambda: ttga.config_instance("syn"),               # E 2000, S 5000
}


@pytest.fixture(scope="module")
def problems():
    cache = {}

    def get(name):
        if name not in cache:
            inst = SHAPES[name]()
            cache[name] = (inst, native.DeviceProblem(inst))
        return cache[name]
    return get


def random_rows(inst, P, seed):
    return np.random.default_rng(seed).integers(0, 45, size=(P, inst.E)).astype(np.uint8)


def evaluation(dp, slot, room, parts=True):
    hcv, scv, feas, pen = (host(t) for t in dp.eval(slot, room))
    return hcv, scv, feas, pen, host(dp.eval_parts(slot, room)) if parts else None


def check(problem, slot, max_passes, want, room=None, parts=True):
    """One call on the rows `slot` (numpy) against `want` = the model's (rows,
    gain, passes, perm), with the evaluation before and after."""
    inst, dp = problem
    P = slot.shape[0]
    s = dev(slot)
    room = dp.assign_rooms(s) if room is None else room
    hcv0, scv0, feas0, pen0, parts0 = evaluation(dp, s, room, parts)
    scv, pen = dev(scv0), dev(pen0)
    gain = torch.full((P,), 12345, dtype=torch.int32, device="cuda")
    passes = torch.full((P,), 12345, dtype=torch.int32, device="cuda")
    perm = torch.full((P, 45), 99, dtype=torch.uint8, device="cuda")
    dp.slot_swap(s, max_passes, scv=scv, penalty=pen, gain=gain, passes=passes, perm=perm)
    got = host(s), host(gain), host(passes), host(perm)
    for name, g, w in zip(("rows", "gain", "passes", "perm"), got, want):
        assert np.array_equal(g, w), f"{name} differ: gpu {g.reshape(P, -1)[:4]} model {w.reshape(P, -1)[:4]}"
    hcv1, scv1, feas1, pen1, parts1 = evaluation(dp, s, room, parts)
    assert np.array_equal(hcv1, hcv0) and np.array_equal(feas1, feas0)
    if parts:
        assert np.array_equal(parts1[:, :3], parts0[:, :3])           # room pairs, correlated pairs, unsuitable
    assert np.array_equal(scv1, scv0 - got[1])
    assert np.array_equal(host(scv), scv1) and np.array_equal(host(pen), pen1)     # in place = a fresh tt_eval
    ok = (slot < 45).all(axis=1)                                                   # new slot = perm[old slot]
    assert np.array_equal(got[3][np.flatnonzero(ok)[:, None], slot[ok]], got[0][ok])
    return got


def searched_rows(dp, P, seed, steps=200):
    rng = dev(ttga.population_seeds(seed, P))
    slot = torch.empty((P, dp.E), dtype=torch.uint8, device="cuda")
    room = torch.empty_like(slot)
    dp.random_init(rng, slot, room)
    dp.local_search(slot, room, rng, steps)
    return host(slot), room


# ---------------------------------------------------------------- sm and med, P = 67
@pytest.mark.parametrize("kind", ["random", "searched"])
@pytest.mark.parametrize("name", ["sm", "med"])
def test_rows_vs_model(problems, name, kind):
    pb = problems(name)
    inst, dp = pb
    P = 67
    if kind == "random":
        slot, room = random_rows(inst, P, 100), None
    else:
        slot, room = searched_rows(dp, P, 2100)
    logs = [[] for _ in range(P)]
    # the model's quickest form (tests/test_slotswap_cpu.py: equal to its other two on all 990 pairs)
    full = sm.stack([sm.descend(inst, slot[i], UNCAPPED, deltas=sm.deltas_windows, log=logs[i]) for i in range(P)])
    print(name, kind, "passes", full[2].tolist(), "gain", full[1].tolist())
    check(pb, slot, UNCAPPED, full, room)
    for cap in (1, 3):
        check(pb, slot, cap, sm.stack([sm.prefix(slot[i], logs[i], cap) for i in range(P)]), room)
    assert full[2].max() > 3 or kind == "searched"            # the caps did cut descents short
    if kind == "random":
        assert any(t for lg in logs for (_, _, _, t) in lg)    # tied best deltas occurred: the tie rule counted
    assert dp.status() & STATUS_MASK == 0


# ---------------------------------------------------------------- other shapes
@pytest.mark.parametrize("name", ["tight", "S7", "S64", "S65", "S1100", "extremes", "E20", "E61"])
def test_shapes_vs_model(problems, name):
    pb = problems(name)
    inst = pb[0]
    slot = random_rows(inst, 8, 200)
    want = sm.descend_rows(inst, slot, UNCAPPED)
    assert want[2].min() >= 1
    check(pb, slot, UNCAPPED, want)
    check(pb, slot, 2, sm.descend_rows(inst, slot, 2))
    assert pb[1].status() & STATUS_MASK == 0


def test_every_event_in_slot_8(problems):
    """All events in the last slot of day 0: the students clash, so W counts a
    student once per event while the attendance mask counts them once."""
    pb = problems("sm")
    inst = pb[0]
    slot = np.full((2, inst.E), 8, np.uint8)
    slot[1, :3] = 17
    want = sm.descend_rows(inst, slot, UNCAPPED)
    assert want[2][0] == 1 and want[1][0] > 0
    check(pb, slot, UNCAPPED, want)


@pytest.mark.parametrize("P", [1, 3])
def test_small_populations(problems, P):
    pb = problems("sm")
    slot = random_rows(pb[0], P, 300 + P)
    check(pb, slot, UNCAPPED, sm.descend_rows(pb[0], slot, UNCAPPED))


def test_syn(problems):
    """E 2000, S 5000: 79 student chunks, 157 K-steps."""
    pb = problems("syn")
    slot = random_rows(pb[0], 2, 400)
    want = sm.descend_rows(pb[0], slot, 3)
    assert (want[2] == 3).all()
    check(pb, slot, 3, want)
    assert pb[1].status() & STATUS_MASK == 0


# ---------------------------------------------------------------- invalid gene, NULL outputs, a second call
def test_invalid_gene():
    """A row with gene 45 between two valid ones: untouched, gain 0, passes 0,
    the identity, status bit 7; its neighbours descend as the model has them.
    Own handle: the status word is sticky."""
    inst = SHAPES["sm"]()
    dp = native.DeviceProblem(inst)
    slot = random_rows(inst, 3, 500)
    slot[1, 7] = 45
    want = sm.descend_rows(inst, slot, UNCAPPED)
    assert want[2].tolist()[1] == 0 and want[2][0] > 0 and want[2][2] > 0
    assert dp.status() == 0
    got = check((inst, dp), slot, UNCAPPED, want, room=torch.zeros((3, inst.E), dtype=torch.uint8, device="cuda"),
                parts=False)
    assert dp.status() & STATUS_MASK == 128
    assert np.array_equal(got[0][1], slot[1]) and np.array_equal(got[3][1], np.arange(45))
    dp.close()


def test_null_outputs_and_second_call(problems):
    pb = problems("sm")
    inst, dp = pb
    slot = random_rows(inst, 9, 600)
    want = sm.descend_rows(inst, slot, UNCAPPED)
    s = dev(slot)
    dp.slot_swap(s, UNCAPPED)                                  # every output NULL
    assert np.array_equal(host(s), want[0]) and not np.array_equal(want[0], slot)
    # the rows are at their local optimum now
    check(pb, want[0], UNCAPPED, (want[0], np.zeros(9, np.int32), np.zeros(9, np.int32),
                                  np.tile(np.arange(45, dtype=np.uint8), (9, 1))))
    assert dp.status() & STATUS_MASK == 0


def test_limit():
    """The documented limit is E <= 50,272: 50,273 is refused with nothing
    launched (every buffer untouched). One student keeps the instance cheap."""
    E = 50273
    A = np.zeros((1, E), np.int32)
    A[0, :3] = 1
    dp = native.DeviceProblem(ttga.Instance(E=E, R=2, F=1, S=1, room_size=np.full(2, 10, np.int32), student_events=A,
                                            room_features=np.ones((2, 1), np.int32),
                                            event_features=np.zeros((E, 1), np.int32)))
    slot = torch.full((2, E), 7, dtype=torch.uint8, device="cuda")
    out = [torch.full((2,), 12345, dtype=torch.int32, device="cuda") for _ in range(4)]
    perm = torch.full((2, 45), 99, dtype=torch.uint8, device="cuda")
    with pytest.raises(native.TTError, match="instance too large") as ei:
        dp.slot_swap(slot, 1, scv=out[0], penalty=out[1], gain=out[2], passes=out[3], perm=perm)
    assert ei.value.code == native.TT_ERR_LIMIT
    assert (host(slot) == 7).all() and (host(perm) == 99).all() and all((host(t) == 12345).all() for t in out)
    assert dp.status() == 0
    dp.close()


# ---------------------------------------------------------------- Island
def test_island_slot_swap_0_issues_no_call(problems, monkeypatch):
    inst, dp = problems("sm")
    plain = run_island(dp, gens=5, children=4)

    def boom(*a, **k):
        raise AssertionError("slot_swap called with Island(slot_swap=0)")
    monkeypatch.setattr(dp, "slot_swap", boom)
    off = run_island(dp, gens=5, children=4, slot_swap=0)
    for k in plain.pop:
        assert np.array_equal(host(off.pop[k]), host(plain.pop[k])), k
    with pytest.raises(ValueError, match="slot_swap_stats"):
        off.slot_swap_stats()
    off.close()
    plain.close()


@pytest.mark.parametrize("schedule", ["batch", "staggered"])
def test_island_slot_swap(problems, schedule):
    inst, dp = problems("sm")
    isl = run_island(dp, gens=5, children=4, slot_swap=4, schedule=schedule, parts=2)
    p = isl.pop
    hcv, scv, feas, pen = (host(t) for t in dp.eval(p["slot"], p["room"]))
    assert np.array_equal(host(p["hcv"]), hcv) and np.array_equal(host(p["scv"]), scv)
    assert np.array_equal(host(p["feasible"]), feas) and np.array_equal(host(p["penalty"]), pen)
    u = pen.astype(np.uint32)
    assert (u[:-1] <= u[1:]).all()                             # in penalty order
    st = isl.slot_swap_stats()
    print(schedule, st)
    assert st["rows"] == 10 + 5 * 4
    assert 0 < st["improved"] <= st["rows"]
    assert st["improved"] <= st["passes"] <= 4 * st["improved"] and st["gain"] >= st["passes"]
    isl.close()
    assert dp.status() & STATUS_MASK == 0


# ---------------------------------------------------------------- the drivers
def test_slot_swap_in_both_drivers(tmp_path, problems):
    inst = problems("sm")[0]
    tim = tmp_path / "sm.tim"
    ttga.write_tim(inst, tim)
    base = ["-i", str(tim), "-s", "29", "-p", "1", "--pop", "16", "--children", "8", "--generations", "10"]
    py, cc, a, lines = both_drivers(tmp_path, base, ["--slot-swap", "4"], "slotSwap", inst)
    cc_zero = run_driver([str(GA), *base, "--slot-swap", "0"], tmp_path)
    assert len(lines) == 1 and set(lines[0]) == {"gain", "improved", "meanPasses", "rows"}
    k = lines[0]
    assert k["rows"] == 16 + 80 and 0 < k["improved"] <= k["rows"] and 1 <= k["meanPasses"] <= 4 and k["gain"] > 0
    assert not any("slotSwap" in x for x in json_lines(cc_zero.stdout))            # 0: no call, no line
