"""eval_tile5's prologue against the CPU oracle: all four outputs, exact equality.

The kernel keeps its launch invariants (the upper-triangle correlation words,
possibleRooms and studentNumber of the lane's events) in registers, filled once
per launch from the problem's lane-ready image: through LDS (tile buffer 1)
beside the first tile's DMA where the image fits in a tile buffer, from global
memory otherwise and in the kernels that stage by vector copies. A wrong row
order or padding in the image, a fill that reads the buffer before the DMA has
landed or after the second tile's DMA has started, or registers that do not
survive from one tile to the next all change some row's hcv or scv.

Shapes (E, R):
  (64, 16)   one full event word, PK 1;
  (68, 10)   two words, four events in the last: the zero padding of the
             correlation and per-event rows;
  (132, 17)  PK 2 (u32 room mask + studentNumber);
  (400, 10)  the headline form, 16 events in word 6;
  (448, 40)  seven full words, PK 0 (u64 room mask);
  (333, 9)   E no multiple of 4: the kernel that stages by vector copies
             (image from global memory behind the first tile's loads);
  (8, 17)    the image (1,024 B, PK 2) is larger than a tile buffer (768 B): the
             global-memory fill in an LDS-DMA kernel. (At every E >= 12 the
             image fits: its 256 EWC (EWC + 2..4) bytes against a tile's
             64 (E + 4) or more.)
Each with 4 and 8 waves, the persistent and the one-tile grid, at P = 131
(three tiles, the last with 3 rows). Rows are random slots with the oracle's
assignRooms, one crowded row (every event in slot 0, room 0) and one row with
an invalid gene (the -1/-1/0/-1 sentinels).
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
SHAPES = [(64, 16), (68, 10), (132, 17), (400, 10), (448, 40), (333, 9), (8, 17)]
VARIANTS = [7, 8, 8 | (64 << 4), 8 | (128 << 4)]
NAMES = ("hcv", "scv", "feasible", "penalty")

_cache = {}


def _problem(E, R):
    """instance, oracle problem, device problem and populations of a shape (built once)."""
    if (E, R) not in _cache:
        inst = ttga.generate(E, R, 5, 120, seed=2000 + E + R)
        _cache[(E, R)] = dict(inst=inst, o=oracle().problem(inst), dp=native.DeviceProblem(inst), pops={})
    return _cache[(E, R)]


def _population(E, R, n=P, seed=91):
    """slots, rooms and the oracle's four outputs for n rows (not modified afterwards)."""
    c = _problem(E, R)
    if (n, seed) not in c["pops"]:
        slots, _ = ttga.random_slots(ttga.population_seeds(seed, n), E)
        rooms = c["o"].assign_rooms(slots)
        slots[1], rooms[1] = 0, 0                              # crowded
        exp = [a.copy() for a in c["o"].eval(slots, rooms)]
        slots[n // 2, E - 1] = 45                              # invalid gene
        exp[0][n // 2] = exp[1][n // 2] = exp[3][n // 2] = -1
        exp[2][n // 2] = 0
        c["pops"][(n, seed)] = (slots, rooms, exp)
    return c["pops"][(n, seed)]


def _check(got, exp):
    for g, e, what in zip((host(t) for t in got), exp, NAMES):
        bad = np.flatnonzero(g != e)
        assert bad.size == 0, f"{what}: rows {bad[:8]} got {g[bad[:8]]} expected {e[bad[:8]]}"


@pytest.mark.parametrize("variant", VARIANTS, ids=["v7", "v8", "v8_persistent", "v8_one_tile"])
@pytest.mark.parametrize("dims", SHAPES, ids=[f"E{e}R{r}" for e, r in SHAPES])
def test_prologue_vs_oracle(dims, variant):
    dp = _problem(*dims)["dp"]
    slots, rooms, exp = _population(*dims)
    _check(dp.eval(dev(slots), dev(rooms), variant=variant), exp)
    assert dp.status() == 0


def test_multi_tile_workgroups():
    """P = 64 (4 x CU count) + 65 with the automatic variant: the workgroups of the
    persistent grid run several tiles each, the last tile partial; the registers
    filled in the prologue serve all of them. The population repeats 997 distinct
    rows (a prime: every tile differs from its neighbours)."""
    dims = (64, 16)
    dp = _problem(*dims)["dp"]
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = 64 * 4 * cus + 65
    slots, rooms, exp = _population(*dims, n=997, seed=92)
    idx = np.arange(n) % 997
    _check(dp.eval(dev(slots[idx]), dev(rooms[idx])), [e[idx] for e in exp])
    assert dp.status() == 0


def test_two_live_handles():
    """Two problems of different shape evaluated alternately on one stream, read at
    the end: each launch takes its own handle's image."""
    a, b = (68, 10), (400, 10)
    pa, pb = _problem(*a)["dp"], _problem(*b)["dp"]
    sa, ra, ea = _population(*a)
    sb, rb, eb = _population(*b)
    da, db = (dev(sa), dev(ra)), (dev(sb), dev(rb))
    outs = [(pa.eval(*da), ea), (pb.eval(*db), eb), (pa.eval(*da), ea), (pb.eval(*db), eb)]
    for got, exp in outs:
        _check(got, exp)
    assert pa.status() == 0 and pb.status() == 0


def test_two_populations_back_to_back():
    """One handle, two different populations, two launches, read after both."""
    dims = (400, 10)
    dp = _problem(*dims)["dp"]
    s1, r1, e1 = _population(*dims, seed=91)
    s2, r2, e2 = _population(*dims, seed=93)
    assert not np.array_equal(s1, s2)
    d1, d2 = (dev(s1), dev(r1)), (dev(s2), dev(r2))
    out1 = dp.eval(*d1)
    out2 = dp.eval(*d2)
    _check(out1, e1)
    _check(out2, e2)
    assert dp.status() == 0
