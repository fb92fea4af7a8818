"""eval_tile5's packed tail blocks against the CPU oracle: all four outputs, exact equality.

With T <= 16 events in the last event word (and a full word before it) the kernel
counts the correlated same-slot pairs (i, j) with j in the tail from the tail
event's side, four event words per 64-lane operation (lane l: tail event l & 15,
word l >> 4 of the operation), from packed rows of the problem's invariant image;
the full words keep the upper-triangle scheme among themselves. Every other tail
length runs the unpacked kernel. A wrong packed row, a lost or doubled block, a
tail lane that reads the wrong B row, or a lane without an event or a word that
counts something all change some row's hcv.

Shapes (E, R):
  (65, 10)   T = 1;
  (80, 10)   T = 16: one full word plus the packed diagonal, blocks 2 and 3 idle;
  (96, 10)   T = 32: unpacked (a two-way packing was not kept);
  (97, 10)   T = 33: unpacked, byte staging;
  (16, 10)   one event word: unpacked (no full word to pack against);
  (336, 17)  six words, T = 16, PK 2;
  (400, 10)  the headline form: the second packed operation's block 3 has no word;
  (416, 40)  T = 32, PK 0: unpacked;
  (269, 9)   T = 13, E no multiple of 4: the kernels that stage by vector copies
             (image from global memory).
Each with 4 and 8 waves, the persistent and the one-tile grid, at P = 131 (three
tiles, the last with 3 rows). Rows: random slots with the oracle's assignRooms;
row 1 crowded (every event in slot 0, room 0: every correlated pair counts);
row 2 with the tail events alone in slot 44 (the packed diagonal on its own);
row 3 with each tail event sharing a slot of its own with one correlated event of
a full word and with no other event (the packed off-diagonal blocks on their own);
row P // 2 with an invalid gene in the last tail event (the -1/-1/0/-1 sentinels).
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
SHAPES = [(65, 10), (80, 10), (96, 10), (97, 10), (16, 10), (336, 17), (400, 10), (416, 40), (269, 9)]
VARIANTS = [7, 8, 8 | (64 << 4), 8 | (128 << 4)]
NAMES = ("hcv", "scv", "feasible", "penalty")
CROWDED, DIAGONAL, PAIRS, INVALID = 1, 2, 3, P // 2

_cache = {}


def _tail_rows(inst, slots):
    """Rows DIAGONAL and PAIRS of slots, in place; returns the number of pairs made."""
    E = inst.E
    first = 64 * ((E - 1) // 64)                                # first event of the last word
    tail = np.arange(first, E)
    # the tail events alone in slot 44, everything else below it
    slots[DIAGONAL, :first] %= 44
    slots[DIAGONAL, first:] = 44
    # tail event k and one correlated full-word event in slot k, every other event above those
    n = len(tail)
    assert n < 45
    slots[PAIRS, :first] = n + slots[PAIRS, :first] % (45 - n)
    slots[PAIRS, first:] = np.arange(n)
    se = inst.student_events.astype(np.int64)
    shared = se[:, :first].T @ se[:, first:]                    # [first, n] common students
    used, pairs = set(), 0
    for k in range(n):
        for i in np.flatnonzero(shared[:, k]):
            if int(i) not in used:
                used.add(int(i))
                slots[PAIRS, i] = k
                pairs += 1
                break
    return pairs


def _problem(E, R):
    """instance, oracle problem, device problem, population and expected outputs (built once,
    not modified afterwards)."""
    if (E, R) not in _cache:
        inst = ttga.generate(E, R, 5, 120, seed=3000 + E + R)
        o = oracle().problem(inst)
        slots, _ = ttga.random_slots(ttga.population_seeds(97, P), E)
        pairs = _tail_rows(inst, slots)
        rooms = o.assign_rooms(slots)
        slots[CROWDED], rooms[CROWDED] = 0, 0
        exp = [a.copy() for a in o.eval(slots, rooms)]
        slots[INVALID, E - 1] = 45
        exp[0][INVALID] = exp[1][INVALID] = exp[3][INVALID] = -1
        exp[2][INVALID] = 0
        _cache[(E, R)] = dict(dp=native.DeviceProblem(inst), slots=slots, rooms=rooms, exp=exp, pairs=pairs)
    return _cache[(E, R)]


@pytest.mark.parametrize("variant", VARIANTS, ids=["v7", "v8", "v8_persistent", "v8_one_tile"])
@pytest.mark.parametrize("dims", SHAPES, ids=[f"E{e}R{r}" for e, r in SHAPES])
def test_tailpack_vs_oracle(dims, variant):
    c = _problem(*dims)
    if dims[0] > 64:
        assert c["pairs"] > 0, "no tail event is correlated with an event of a full word"
    got = c["dp"].eval(dev(c["slots"]), dev(c["rooms"]), variant=variant)
    for g, e, what in zip((host(t) for t in got), c["exp"], NAMES):
        bad = np.flatnonzero(g != e)
        assert bad.size == 0, f"{what}: rows {bad[:8]} got {g[bad[:8]]} expected {e[bad[:8]]}"
    assert c["dp"].status() == 0
