"""tt_move1_scan and tt_move1_descent on a population whose d_scv table passes
2^32 bytes: tests/large_rows.py's periodic check. The base block is 4,099
pairwise distinct feasible rows of a 448-event instance -- a few rows of the
CPU constructor, each relabelled by random permutations of the 45 slot labels,
which keeps hcv 0 (the hard constraints only see which events share a slot) --
repeated down some 57,000 rows. Every output of the big call must have the
block's period and equal the call on the block alone, whose first rows the
model judges. A row offset i * E * 45 that wrapped at 2^32 bytes (or 2^31)
would land on another base row, or in the middle of one."""
import gc

import numpy as np
import pytest

import ttga
import lahc_model as lm
import large_rows as lr
import move1_model as mm
from helpers import dev, host

pytestmark = pytest.mark.gpu

import torch  # noqa: E402
from ttga import native  # noqa: E402

M = lr.M_ROWS
E = 448
LINE = 1 << 32
MODEL_ROWS = 8
U8_FILL, I32_FILL = 0xEE, -77                       # no room code and no delta or count


def u8(*shape):
    return torch.full(shape, U8_FILL, dtype=torch.uint8, device="cuda")


def i32(*shape):
    return torch.full(shape, I32_FILL, dtype=torch.int32, device="cuda")


@pytest.fixture(scope="module")
def block():
    inst = ttga.generate(E, 10, 5, 150, seed=12)
    model = mm.Model(inst)
    seeds_slot, seeds_room = lm.feasible_rows(inst, 4, 7, model)
    assert all(model.scanned(seeds_slot[i], seeds_room[i]) for i in range(4))
    g = np.random.default_rng(2024)
    perms = np.stack([g.permutation(45) for _ in range(M)]).astype(np.uint8)
    src = np.arange(M) % 4
    slot = np.take_along_axis(perms, seeds_slot[src].astype(np.int64), axis=1)        # slot label s becomes perm[s]
    room = seeds_room[src].copy()
    assert len({row.tobytes() for row in slot}) == M                                  # pairwise distinct
    dp = native.DeviceProblem(inst)
    hcv = host(dp.eval(dev(slot), dev(room))[0])
    assert not hcv.any()                                                              # and feasible, all of them
    yield inst, dp, model, slot, room
    dp.close()


@pytest.fixture(autouse=True)
def free_between_cases():
    yield
    torch.cuda.synchronize()
    gc.collect()
    torch.cuda.empty_cache()


def test_scan_past_4_gib_of_d_scv(block):
    inst, dp, model, slot, room = block
    P = lr.rows_past(LINE, E * 45 * 4)
    assert P * E * 45 * 4 >= LINE + M * E * 45 * 4 and P * E * 45 > (1 << 30) and P % 64    # to_room past 2^30 bytes
    lr.need_device_memory(P * E * 45 * 5 + P * E * 2)
    bs, br = dev(slot), dev(room)
    bsm, bd, btr = i32(M, 6), i32(M, E, 45), u8(M, E, 45)
    dp.move1_scan(bs, br, bsm, bd, btr)
    want = model.scan_rows(slot[:MODEL_ROWS], room[:MODEL_ROWS])
    for name, got, w in zip(("summary", "d_scv", "to_room"), (bsm, bd, btr), want):
        assert np.array_equal(host(got[:MODEL_ROWS]), w), name
    assert (host(bsm)[:, 0] == 1).all() and (host(bsm)[:, 2] > 0).all()
    s, r = lr.tile_rows(bs, P), lr.tile_rows(br, P)
    sm, d, tr = i32(P, 6), i32(P, E, 45), u8(P, E, 45)
    dp.move1_scan(s, r, sm, d, tr)
    lr.assert_periodic(sm, bsm, "tt_move1_scan: summary")
    lr.assert_periodic(d, bd, "tt_move1_scan: d_scv")
    lr.assert_periodic(tr, btr, "tt_move1_scan: to_room")
    lr.assert_periodic(s, bs, "tt_move1_scan: slot")
    lr.assert_periodic(r, br, "tt_move1_scan: room")
    assert dp.status() == 0
    print(f"\nLARGE_ROWS case=tt_move1_scan P={P} d_scv_GiB={P * E * 45 * 4 / 2 ** 30:.2f}")


def test_descent_on_that_population(block):
    inst, dp, model, slot, room = block
    P = lr.rows_past(LINE, E * 45 * 4)
    lr.need_device_memory(P * E * 2 + P * 16)
    bs, br = dev(slot), dev(room)
    _, scv0, _, pen0 = dp.eval(bs, br)
    bscv, bpen, bgain, bpass = scv0.clone(), pen0.clone(), i32(M), i32(M)
    dp.move1_descent(bs, br, 2, bscv, bpen, bgain, bpass)
    want = model.descent_rows(slot[:MODEL_ROWS], room[:MODEL_ROWS], 2)
    for name, got, w in zip(("slot", "room", "gain", "passes"), (bs, br, bgain, bpass), want):
        assert np.array_equal(host(got[:MODEL_ROWS]), w), name
    assert (host(bpass) == 2).all() and np.array_equal(host(bscv), host(scv0) - host(bgain))
    s, r = lr.tile_rows(dev(slot), P), lr.tile_rows(dev(room), P)
    scv, pen, gain, passes = lr.tile_rows(scv0, P), lr.tile_rows(pen0, P), i32(P), i32(P)
    dp.move1_descent(s, r, 2, scv, pen, gain, passes)
    for name, big, base in (("slot", s, bs), ("room", r, br), ("scv", scv, bscv), ("penalty", pen, bpen),
                            ("gain", gain, bgain), ("passes", passes, bpass)):
        lr.assert_periodic(big, base, f"tt_move1_descent: {name}")
    assert dp.status() == 0
