"""eval_tile5's wave phase against the CPU oracle on populations built to catch
what its workspace clear and row addressing can get wrong: all four outputs,
exact equality.

A wave of the kernel evaluates rows q, q + NW, q + 2 NW, ... of a 64-row tile
one after the other in ONE workspace (per-slot event bitsets + room-cell
counters), cleared before each valid row and not touched for an invalid one.
The rows a wave sees in turn are therefore made as different as possible:

* crowded: every event in slot 0, room 0 -- one bitset row full, one cell
  counter at E, per-lane hcv parts past the packed reduction's 1024;
* spread: random slots (ttga.random_slots), the oracle's assignRooms;
* corner: every event in slot 44, room R - 1 -- the last bitset row and the last
  cell counter, next to the neighbouring wave's workspace;
* invalid: slot 45 at event 0, slot 255 at event E - 1, or room R at event
  E // 2 in a spread row: the -1/-1/0/-1 sentinels, and the rows before and
  after it in the same wave exact.

Stale bits from the previous row, a clear that reaches into the next wave's
workspace or the partial sums behind the last one, a wrong word offset in a
correlation read or a first tile read before its DMA has landed all change
some row's hcv or scv. P = 131 is three tiles, the last with 3 rows; the shapes
cover 1, 2, 6 and 7 event words with full and partial last words, the three
possibleRooms forms (R <= 16, <= 32, <= 64), workspaces that are no multiple of
256 B and below 1 KiB, and both the byte-staging and the LDS-DMA path.
Reference: Solution.cpp:63-170.
"""
import numpy as np
import pytest

import ttga
from helpers import dev, host
from oracle_lib import oracle

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from ttga import native  # noqa: E402

P = 131
SHAPES = [(50, 5), (64, 16), (65, 17), (333, 9), (400, 10), (448, 40)]
# tt_eval_variant: 7 = 4 waves per tile, 8 = 8 waves; 64 << 4 forces the persistent
# grid, 128 << 4 one tile per workgroup
VARIANTS = [7, 8, 8 | (64 << 4), 8 | (128 << 4)]
# what a wave meets in turn (its k-th row of a tile, k mod 8): the invalid rows (I)
# sit between valid ones
CYCLE = "CSISKSIC"      # Crowded, Spread, Invalid, Spread, Korner, Spread, Invalid, Crowded

_cache = {}


def _problem(E, R):
    key = (E, R)
    if key not in _cache:
        inst = ttga.generate(E, R, 5, 120, seed=1000 + E + R)
        _cache[key] = (inst, oracle().problem(inst), {})
    return _cache[key]


def build_population(inst, o, NW, seed):
    """slots, rooms and the expected four outputs of P rows laid out for NW waves
    per tile (host only: the oracle evaluates every row pattern)."""
    E, R = inst.E, inst.R
    slots, _ = ttga.random_slots(ttga.population_seeds(seed, P), E)
    rooms = o.assign_rooms(slots)
    kinds = []
    for p in range(P):
        q = p % 64
        kinds.append(CYCLE[(q // NW) % 8])
        if kinds[-1] == "C":
            slots[p], rooms[p] = 0, 0
        elif kinds[-1] == "K":
            slots[p], rooms[p] = 44, R - 1
    exp = [a.copy() for a in o.eval(slots, rooms)]
    n_bad = 0
    for p in range(P):
        if kinds[p] != "I":
            continue
        which = n_bad % 3
        n_bad += 1
        if which == 0:
            slots[p, 0] = 45
        elif which == 1:
            slots[p, E - 1] = 255
        else:
            rooms[p, E // 2] = R
        exp[0][p] = exp[1][p] = exp[3][p] = -1
        exp[2][p] = 0
    assert n_bad >= 3 and kinds.count("C") > 0 and kinds.count("K") > 0
    return slots, rooms, exp


def _population(E, R, NW, seed=77):
    inst, o, pops = _problem(E, R)
    if (NW, seed) not in pops:
        pops[(NW, seed)] = build_population(inst, o, NW, seed)
    return inst, pops[(NW, seed)]


def _device_problem(E, R):
    inst, _, pops = _problem(E, R)
    if "dp" not in pops:
        pops["dp"] = native.DeviceProblem(inst)
    return pops["dp"]


@pytest.mark.parametrize("variant", VARIANTS, ids=["v7", "v8", "v8_persistent", "v8_one_tile"])
@pytest.mark.parametrize("dims", SHAPES, ids=[f"E{e}R{r}" for e, r in SHAPES])
def test_wave_rows_vs_oracle(dims, variant):
    NW = 4 if (variant & 15) == 7 else 8
    inst, (slots, rooms, exp) = _population(*dims, NW)
    dp = _device_problem(*dims)
    got = [host(t) for t in dp.eval(dev(slots), dev(rooms), variant=variant)]
    for g, e, what in zip(got, exp, ("hcv", "scv", "feasible", "penalty")):
        bad = np.flatnonzero(g != e)
        assert bad.size == 0, f"{what}: rows {bad[:8]} got {g[bad[:8]]} expected {e[bad[:8]]}"
    assert dp.status() == 0


def test_back_to_back_launches_vs_oracle():
    """Two launches on one stream over two populations, read only after both:
    the second kernel's prologue (first tile's DMA, invariant loads) under a
    running launch."""
    dims = (400, 10)
    dp = _device_problem(*dims)
    _, (s1, r1, e1) = _population(*dims, 8, seed=77)
    _, (s2, r2, e2) = _population(*dims, 8, seed=78)
    assert not np.array_equal(s1, s2)
    d1, d2 = (dev(s1), dev(r1)), (dev(s2), dev(r2))
    out1 = dp.eval(*d1)
    out2 = dp.eval(*d2)
    for out, exp in ((out1, e1), (out2, e2)):
        for g, e in zip((host(t) for t in out), exp):
            assert np.array_equal(g, e)
    assert dp.status() == 0
