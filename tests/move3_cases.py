"""Inputs of the Move3 tests (imported like helpers; no fixtures, CPU only).

tests/test_gpu_ls_move3.py runs these cases on the GPU against the oracle and
tests/test_oracle.py runs the small ones on the oracle against the reference
build, so both build exactly the same rows and streams from here.
"""
import numpy as np

import ttga
from oracle_lib import split_rows

# (p1, p2, p3), maxSteps: Move3 alone, all moves at every visit, and two mixes
TRIPLES = [((0.0, 0.0, 1.0), 300), ((1.0, 1.0, 1.0), 300), ((0.5, 0.3, 0.2), 300), ((0.2, 0.2, 0.6), 1000)]

# dims, instance seed, attendances, population, maxSteps of the Move1/Move2
# pre-search that makes the phase-2 starts, crowded rows, population seed base
SHAPES = {
    "E50_one_launch": dict(dims=(50, 5, 4, 40), seed=19, att=None, P=32, pre=4000, crowd=False, base=31000),
    "E120": dict(dims=(120, 6, 4, 90), seed=41, att=None, P=32, pre=4000, crowd=False, base=17000),
    # 1500 steps: feasible, but not yet a Move1/Move2 optimum
    "E300_R12": dict(dims=(300, 12, 4, 150), seed=31, att=None, P=32, pre=1500, crowd=False, base=33000),
    "E400_redo": dict(dims=(400, 10, 5, 200), seed=47, att=None, P=30, pre=4000, crowd=True, base=34004),
    "E449R40_redo": dict(dims=(449, 40, 5, 220), seed=47, att=(4, 16), P=30, pre=4000, crowd=True, base=35000),
}
SMALL = ("E50_one_launch", "E120")

# tests/golden/move3.npz (oracle/gen_golden.py move3): shapes, rows per start set, cases
GOLDEN_SHAPES = {"e120": "E120", "e300": "E300_R12"}
GOLDEN_ROWS = 8
GOLDEN_CASES = [((0.0, 0.0, 1.0), 64), ((1.0, 1.0, 1.0), 300), ((0.5, 0.3, 0.2), 300)]

BUDGETS = (1, 2, 3, 4, 5, 8, 9, 17, 33, 64, 65)
# every step a Move3 trial (the budget ends after the first and after the second
# trial of a pair, at both parities), and a mix with the Move1/Move2 windows
BUDGET_TRIPLES = [(0.0, 0.0, 1.0), (0.0, 0.0, 0.5), (0.9, 0.35, 0.5)]


def instance(key):
    c = SHAPES[key]
    kw = dict(min_att=c["att"][0], max_att=c["att"][1]) if c["att"] else {}
    return ttga.generate(*c["dims"], seed=c["seed"], **kw)


def starts(o, key):
    """{"a": (slots, rooms), "b": (slots, rooms)}: (a) RandomInitialSolution
    rows (phase 1), every third one with 65..119 events in one slot where the
    shape is a crowded one; (b) the feasible rows among (a) after
    localSearch(pre) with prob3 = 0 (phase 2)."""
    c = SHAPES[key]
    P, base = c["P"], c["base"]
    s0, r0, _ = o.random_init(ttga.population_seeds(base, P))
    if c["crowd"]:
        rng = np.random.default_rng(base)
        for k in range(1, P, 3):
            idx = rng.choice(o.E, size=int(rng.integers(65, 120)), replace=False)
            s0[k, idx] = int(rng.integers(0, 45))
        r0 = o.assign_rooms(s0)
    s1, r1, _ = split_rows(o.local_search, (s0, r0, ttga.population_seeds(base + 100, P)), c["pre"])
    feas = o.eval(s1, r1)[2].astype(bool)
    return {"a": (s0, r0), "b": (np.ascontiguousarray(s1[feas]), np.ascontiguousarray(r1[feas]))}


def run_seeds(key, which, n):
    return ttga.population_seeds(SHAPES[key]["base"] + (200 if which == "a" else 300), n)


def changed_rows(s0, r0, s1, r1):
    return int(((s0 != s1).any(1) | (r0 != r1).any(1)).sum())


def hot_events(inst, s, r):
    """Per individual: events with eventHcv > 0 (Solution.cpp:173-191)."""
    A = inst.student_events.astype(np.int64)
    C = (A.T @ A) > 0
    np.fill_diagonal(C, False)
    out = []
    for sl, rm in zip(s, r):
        same_slot = sl[:, None] == sl[None, :]
        clash = same_slot & (rm[:, None] == rm[None, :])
        np.fill_diagonal(clash, False)
        out.append(int(((clash | (C & same_slot)).any(axis=1)).sum()))
    return np.array(out)


def flagged_starts(o, inst):
    """The starts of test_local_search_flagged_events_vs_oracle: feasible rows
    with one to three events moved to random slots (GA-child-like: few events
    with eventHcv > 0)."""
    P = 48
    s0, r0, _ = o.random_init(ttga.population_seeds(2201, P))
    s1, r1, _ = split_rows(o.local_search, (s0, r0, ttga.population_seeds(2301, P)), 3000)
    feas = o.eval(s1, r1)[2].astype(bool)
    rng = np.random.default_rng(7)
    s2 = s1[feas].copy()
    for k in range(s2.shape[0]):
        idx = rng.choice(inst.E, size=int(rng.integers(1, 4)), replace=False)
        s2[k, idx] = rng.integers(0, 45, size=idx.size)
    return s2, o.assign_rooms(s2), int(feas.sum()), P


def golden_instance(z, tag):
    """The instance stored in tests/golden/move3.npz under `tag`."""
    E, R, F, S = (int(x) for x in z[f"{tag}_dims"])
    A = np.unpackbits(z[f"{tag}_student_bits"], axis=1)[:, :E]
    return ttga.Instance(E, R, F, S, z[f"{tag}_room_size"], A, z[f"{tag}_room_features"], z[f"{tag}_event_features"])


def check_golden(z, tag, search):
    """search(slots, rooms, seeds, steps, p1, p2, p3) -> (slots, rooms, rng)
    against every case of the fixture; returns the rows changed per case."""
    changed = {}
    for w in "ab":
        s0, r0, seeds = z[f"{tag}_{w}_slots"], z[f"{tag}_{w}_rooms"], z[f"{tag}_{w}_seeds"]
        for k, (p, steps) in enumerate(GOLDEN_CASES):
            s, r, g = search(s0, r0, seeds, steps, *p)
            what = (tag, w, p, steps)
            assert np.array_equal(s, z[f"{tag}_{w}{k}_slots"]), what
            assert np.array_equal(r, z[f"{tag}_{w}{k}_rooms"]), what
            assert np.array_equal(g, z[f"{tag}_{w}{k}_rng"]), what
            changed[w, k] = changed_rows(s0, r0, z[f"{tag}_{w}{k}_slots"], z[f"{tag}_{w}{k}_rooms"])
    return changed
